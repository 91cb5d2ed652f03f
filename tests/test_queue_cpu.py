"""The synthesis queue without a GPU: the integer schedule of synthesize.queue_schedule -- list scheduling of N utterances
on R decoder rows --, the numpy restatement of the two kernels of csrc/queue.hip driven by it, generate_gestures_queue's host-side refusals,
and the C header's declarations."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import queue_ref as Q
import utterance_ref as U


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def test_schedule_of_the_kernel_tests_shape(syn):
    rounds, table, row, first = syn.queue_schedule([1, 3, 2, 1, 2], 3)
    assert rounds == 3 and row.tolist() == [1, 0, 1, 2, 2] and first.tolist() == [2, 0, 0, 2, 0]         # longest first: 9 windows, no idle entry
    assert table.tolist() == [[[1, 0], [2, 0], [4, 0]], [[1, 1], [2, 1], [4, 1]], [[1, 2], [0, 0], [3, 0]]]
    rounds, table, row, first = syn.queue_schedule([1, 3, 2, 1, 2], 3, order="given")
    assert rounds == 4 and (table[:, :, 0] < 0).sum() == 3 and row.tolist() == [0, 1, 2, 0, 0]
    # lock-step in groups of three would take max(1, 3, 2) + max(1, 2) = 5 rounds
    rounds, table, _, _ = syn.queue_schedule([2], 4)                                    # surplus rows idle throughout
    assert rounds == 2 and (table[:, 1:] == -1).all() and table[:, 0].tolist() == [[0, 0], [0, 1]]


@pytest.mark.parametrize("order", ["longest_first", "given"])
def test_schedule_properties_on_random_sets(syn, order):
    rng = np.random.default_rng(33)
    for case in range(300):
        N = int(rng.integers(1, 41))
        n_win = [int(v) for v in rng.integers(1, 51, size=N)]
        rows = int(rng.integers(1, 9)) if case % 5 else N + int(rng.integers(1, 4))     # every fifth case: more rows than utterances
        rounds, table, row, first = syn.queue_schedule(n_win, rows, order)
        Q.check_schedule(n_win, rows, rounds, table, row, first, order)
        syn._check_schedule(table, n_win, rows)
        if rows > N:
            assert rounds == max(n_win) and sorted(row.tolist()) == list(range(N))


def test_the_upload_check_refuses_a_broken_schedule(syn):
    n_win = [1, 3, 2]
    _, table, _, _ = syn.queue_schedule(n_win, 2)
    for edit in ("two_rows", "gap", "order", "missing", "twice"):
        t = table.copy()
        if edit == "two_rows":                                                          # utterance 1 continues in the other row
            t = np.array([[[1, 0], [2, 0]], [[2, 1], [1, 1]], [[1, 2], [0, 0]]], np.int32)
        elif edit == "gap":
            t = np.array([[[1, 0], [2, 0]], [[-1, -1], [2, 1]], [[1, 1], [0, 0]], [[1, 2], [-1, -1]]], np.int32)
        elif edit == "order":
            t[0, 0], t[1, 0] = table[1, 0], table[0, 0]
        elif edit == "missing":
            t[2, 0] = -1
        else:
            t = np.concatenate([table, table[-1:]])
        with pytest.raises(ValueError, match="queue schedule"):
            syn._check_schedule(t, n_win, 2)


def test_schedule_refusals(syn):
    for bad in ([], [0, 2], [1.5], [2, -1]):
        with pytest.raises(ValueError, match="n_win"):
            syn.queue_schedule(bad, 2)
    for rows in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="rows"):
            syn.queue_schedule([1, 2], rows)
    with pytest.raises(ValueError, match="order"):
        syn.queue_schedule([1, 2], 2, order="shortest_first")


def test_numpy_kernels_run_a_whole_queue(syn):
    """The restated kernels, driven for `rounds` rounds with nothing but the uploaded tables, stack every utterance's windows as a row-by-row
    loop over the utterance does -- whatever the other rows held -- and leave the rows' counters at `rounds`."""
    rng = np.random.default_rng(34)
    n_win, R, T, n, D, L, W = [1, 3, 2, 1, 2], 3, 10, 2, 3, 7, 5
    N, stride = len(n_win), T - n
    windows = [[dict(audio=rng.standard_normal(L).astype(np.float32), text=rng.integers(1, 9, size=int(rng.integers(2, W + 1)))) for _ in range(k)]
               for k in n_win]
    seeds, seed_on = rng.standard_normal((N, n, D)).astype(np.float32), np.array([1, 0, 1, 1, 0], np.int32)
    draws, vids = rng.standard_normal((sum(n_win), 16)).astype(np.float32), np.arange(10, 10 + N)
    off = np.concatenate([[0], np.cumsum(n_win)])

    def model(row):                                                                  # a row-local "forward": a row's result depends on its own inputs only
        return (row["seed"][:n].sum() + row["audio"].sum() + row["text"][:row["len"]].sum() + row["vid"] + row["draw"].sum()
                + np.arange(T * D, dtype=np.float32).reshape(T, D)).astype(np.float32)

    want = []
    for u in range(N):                                                               # one utterance at a time
        tot, tail = np.zeros((n_win[u] * stride + n, D), np.float32), None
        seed = Q.pre_seq(seeds[u], T) if seed_on[u] else np.zeros((T, D + 1), np.float32)
        for i in range(n_win[u]):
            text = np.zeros(W, np.int64); text[:len(windows[u][i]["text"])] = windows[u][i]["text"]
            res = model(dict(seed=seed, audio=windows[u][i]["audio"], text=text, len=len(windows[u][i]["text"]), vid=vids[u], draw=draws[off[u] + i]))
            win = Q.blend(tail, res) if i else res
            tot[i * stride:i * stride + T] = win
            tail = win[T - n:].copy()
            seed = Q.pre_seq(tail, T)
        want.append(tot)
    for order in ("longest_first", "given"):
        rounds, sched, _, _ = syn.queue_schedule(n_win, R, order)
        bufs = dict(audio=np.full((R, L), 9, np.float32), text=np.full((R, W), 9, np.int64), len=np.full(R, 2, np.int64), vid=np.zeros(R, np.int64),
                    draw=np.zeros((R, 16), np.float32), seed=np.full((R, T, D + 1), 9, np.float32))
        rnd, tail, total = np.zeros(R, np.int32), np.full((R, n, D), 9, np.float32), np.zeros((N, max(n_win) * stride + n, D), np.float32)
        for _ in range(rounds):
            Q.stage(sched, rnd, n_win, windows, bufs, vids=vids, draws=draws, seeds=seeds, seed_on=seed_on, T=T)
            res = np.stack([model({k: v[b] for k, v in bufs.items()}) for b in range(R)])
            Q.handover(sched, rnd, n_win, res, total, tail, bufs["seed"])
        assert rnd.tolist() == [rounds] * R
        for u in range(N):
            assert np.array_equal(total[u, :len(want[u])], want[u]) and not total[u, len(want[u]):].any(), (order, u)


def fake_model():
    return SimpleNamespace(parameters=lambda: iter([torch.zeros(1)]))


def test_generate_gestures_queue_refuses_on_the_host(syn):
    lang, audios = U.Lang(), [U.make_audio(20000, 1), U.make_audio(50000, 2)]
    words = [U.WORD_LISTS["two_on_one_frame"], U.WORD_LISTS["empty"]]
    run = lambda model, rows=2, **kw: syn.generate_gestures_queue(U.make_args(model), fake_model(), lang, audios, words, rows, **kw)
    with pytest.raises(ValueError, match="speech2gesture model has no window decoder"):
        run("speech2gesture")
    for model, rows in (("multimodal_context", 0), ("multimodal_context", 129), ("joint_embedding", 5), ("seq2seq", 5), ("seq2seq", 2.0), ("seq2seq", True)):
        with pytest.raises(ValueError, match="rows"):
            run(model, rows)
    with pytest.raises(ValueError, match="order"):
        run("multimodal_context", order="random")
    with pytest.raises(ValueError, match="no utterance"):
        syn.generate_gestures_queue(U.make_args(), fake_model(), lang, [], [], 2)
    with pytest.raises(ValueError, match="max_words"):                                 # window 0 of utterance 0 holds three words
        run("seq2seq", max_words=2)
    with pytest.raises(ValueError, match="max_words"):
        run("seq2seq", max_words=127)
    with pytest.raises(ValueError, match="window_decoder must be a WindowDecoder"):
        run("multimodal_context", window_decoder=object())
    with pytest.raises(ValueError, match="window_decoder must be a Seq2SeqWindowDecoder"):
        run("seq2seq", window_decoder=object())
    with pytest.raises(ValueError, match="vids holds 3"):
        run("multimodal_context", vids=[1, 2, 3])
    with pytest.raises(ValueError, match="takes no draws"):
        run("seq2seq", _draws=[np.zeros((1, 16)), np.zeros((2, 16))])
    with pytest.raises(ValueError, match="takes eps_list"):
        run("joint_embedding", _draws=[np.zeros((1, 16)), np.zeros((2, 16))])
    with pytest.raises(ValueError, match="audio_sr must be 16000"):
        run("multimodal_context", input_sr=48000, audio_sr=8000)


def test_header_declares_the_queue_entries(pkg):
    L = pkg._lib
    assert L.ABI_VERSION == 11                                                         # new symbols only
    for name, n_args in (("tg_queue_stage", 29), ("tg_queue_handover", 16)):
        assert name in L.SIGNATURES and len(L.SIGNATURES[name]) == n_args and L.DECLARED[name][0] == "int"
    with open(L.HEADER_PATH) as f:
        text = f.read()
    assert re.search(r"int tg_queue_stage\(const int32_t\* sched, const int32_t\* rnd,", text)
    assert re.search(r"int tg_queue_handover\(const float\* res, float\* total, int64_t F,", text)
