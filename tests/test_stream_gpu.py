"""Streaming synthesis on the GPU (csrc/stream.hip, synthesize.GestureStream).

The two kernels copy, so they are compared with numpy exactly.  End to end, everything push() and close() return, concatenated, must be BIT-EQUAL
to generate_gestures_batch(on_device=True) on the finished utterance with the same injected draws: the window inputs are bit-equal (every length
used here satisfies stream_matches_offline, tests/test_stream_cpu.py) and the same decoder kernels run, so there is no tolerance.  The offline
word list is cut at the utterance's end (a word cannot start after the audio has ended); the stream receives every word with the chunk that
holds its start time."""
import numpy as np
import pytest
import torch

import stream_ref as R
import utterance_ref as U
from test_utterance_gpu import guarded, guards_intact, joint_embed, multimodal          # the model builders of the on-device utterance tests

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE
MAX_CHUNK = 5000


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


# ------------------------------------------------------------------------------------------------------------------ the kernels against numpy
def new_state(pkg, dev, B, max_chunk=MAX_CHUNK, W=8):
    st = pkg.ops.stream_state(B, A + max_chunk, S, A, W, T, dev)                 # the smallest legal ring
    st["ring"].fill_(float("nan"))                                               # stale contents must never reach an output
    return st


@pytest.mark.parametrize("B", [1, 3])
def test_push_and_stage_on_the_smallest_ring(pkg, dev, B):
    """Chunks of 1, 7, 4099 and max_chunk samples in turn until three windows are complete: the wrap point falls inside chunks and inside staged
    windows; every complete window is staged as soon as it is complete and equals the stream's samples bit for bit.  The ring starts as NaN."""
    ops, st = pkg.ops, new_state(pkg, dev, B)
    Rr = st["R"]
    stream = np.stack([U.make_audio(2 * S + A + 9107, 40 + b) for b in range(B)])
    sizes, pushed, w, k = [1, 7, 4099, MAX_CHUNK], 0, 0, 0
    chunk_wraps = window_wraps = 0
    while w < 3:
        n = sizes[k % 4]; k += 1
        src = torch.from_numpy(stream[:, pushed:pushed + n]).to(dev)
        if k % 2:                                                                # a strided source: rows of a wider buffer
            wide = torch.full((B, n + 5), 9.0, device=dev)
            wide[:, :n] = src
            src = wide[:, :n]
        ops.stream_push(st, src)
        chunk_wraps += pushed // Rr != (pushed + n - 1) // Rr
        pushed += n
        while pushed >= w * S + A:
            abuf, a_out = guarded((B, A), dev)
            ops.stream_stage(st, None, a_out)
            torch.cuda.synchronize()
            assert guards_intact(abuf)
            assert np.array_equal(a_out.cpu().numpy().view(np.uint32), stream[:, w * S:w * S + A].view(np.uint32)), w
            window_wraps += (w * S) // Rr != (w * S + A - 1) // Rr
            ops.counter_inc(st["win"])
            w += 1
    assert chunk_wraps >= 2 and window_wraps >= 2
    assert st["written"].tolist() == [pushed] * B and int(st["win"][0]) == 3 and st["n_words"].tolist() == [0] * B


@pytest.mark.parametrize("B", [1, 3])
def test_staging_with_fewer_than_a_window_available(pkg, dev, B):
    """The closing windows of a stream: what has not been pushed reads as exact zeros, never as the ring's stale contents (NaN here; the second
    window's range wraps over samples of the first)."""
    ops, st = pkg.ops, new_state(pkg, dev, B)
    n_total = S + 4321
    stream = np.stack([U.make_audio(n_total, 50 + b) for b in range(B)])
    for p in range(0, n_total, MAX_CHUNK):
        ops.stream_push(st, torch.from_numpy(stream[:, p:p + MAX_CHUNK]).to(dev))
    for w, avail in ((0, A), (1, 4321), (2, 0)):
        abuf, a_out = guarded((B, A), dev)
        ops.stream_stage(st, None, a_out)
        torch.cuda.synchronize()
        got = a_out.cpu().numpy()
        assert guards_intact(abuf) and not np.isnan(got).any()
        assert np.array_equal(got[:, :avail].view(np.uint32), stream[:, w * S:w * S + avail].view(np.uint32))
        assert np.array_equal(got[:, avail:].view(np.uint32), np.zeros((B, A - avail), np.uint32))          # +0.0, bit for bit
        ops.counter_inc(st["win"])


def test_text_staging_last_record_wins_and_other_windows_are_ignored(pkg, dev):
    ops, B, W = pkg.ops, 2, 8
    st = new_state(pkg, dev, B, W=W)
    one = torch.zeros(B, 1, device=dev)

    def push(rows, live):
        m = max(len(r) for r in rows)
        table = np.zeros((B, 1 + 3 * m), np.int32)
        for b, r in enumerate(rows):
            table[b, 0] = len(r)
            table[b, 1:1 + 3 * len(r)] = np.asarray(r, np.int32).reshape(-1)
        ops.stream_push(st, one, torch.from_numpy(table).to(dev), m, live)

    def staged():
        tbuf, t_out = guarded((B, T), dev, torch.int64)
        ops.stream_stage(st, t_out, None)
        torch.cuda.synchronize()
        assert guards_intact(tbuf)
        return t_out.cpu().numpy()

    rows = [[(0, 3, 11), (0, 3, 12), (1, 3, 13), (0, 0, 14), (0, T - 1, 15), (0, T, 16)], [(1, 5, 21), (0, 5, 22)]]
    push(rows, 0)
    assert np.array_equal(staged(), np.stack([R.replay(r, 0) for r in rows]))
    assert staged()[0, 3] == 12 and staged()[1, 5] == 22
    # five more records per row: the word ring (8 slots) wraps, its oldest records are gone, the order of the rest decides
    more = [[(1, 3, 31), (1, 4, 32), (1, 4, 33), (2, 0, 34), (1, 3, 35)], [(1, 5, 41), (1, 6, 42), (1, 5, 43), (1, 0, 44), (1, 33, 45)]]
    push(more, 3)
    ops.counter_inc(st["win"])
    kept = [(rows[b] + more[b])[-W:] for b in range(B)]
    assert np.array_equal(staged(), np.stack([R.replay(k, 1) for k in kept]))
    assert staged()[0, 3] == 35 and staged()[0, 4] == 33 and staged()[1, 5] == 43
    assert st["n_words"].tolist() == [11, 7]


@pytest.mark.parametrize("case", ["B_5", "ring_below_A_plus_n", "n_0", "word_ring_overflow"])
def test_calls_outside_the_envelope_are_refused_and_leave_everything_untouched(pkg, dev, case):
    ops = pkg.ops
    B, n, R_ = (5 if case == "B_5" else 2), (0 if case == "n_0" else 100), A + (99 if case == "ring_below_A_plus_n" else 100)
    st = ops.stream_state(B, R_, S, A, 8, T, dev)
    st["ring"].fill_(3.0); st["words"].fill_(5); st["written"].fill_(17); st["n_words"].fill_(2)
    recs, m, live = None, 0, 0
    if case == "word_ring_overflow":
        recs, m, live = torch.ones(B, 1 + 3 * 4, dtype=torch.int32, device=dev), 4, 5
    with pytest.raises(RuntimeError, match="envelope"):
        ops.stream_push(st, torch.ones(B, n, device=dev), recs, m, live)
    if case == "B_5":
        abuf, a_out = guarded((B, A), dev)
        tbuf, t_out = guarded((B, T), dev, torch.int64)
        with pytest.raises(RuntimeError, match="envelope"):
            ops.stream_stage(st, t_out, a_out)
        torch.cuda.synchronize()
        assert bool((abuf == 7).all()) and bool((tbuf == 7).all())
    torch.cuda.synchronize()
    assert bool((st["ring"] == 3.0).all()) and bool((st["words"] == 5).all())
    assert st["written"].tolist() == [17] * B and st["n_words"].tolist() == [2] * B


# ------------------------------------------------------------------------------------------------------------------ end to end
def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def model_of(name, multimodal, joint_embed):
    """(args, net, the per-window draws (3 rows), the keyword that carries them, offline keywords that select the same decoder kernels)."""
    if name == "multimodal":
        args, net, draws = multimodal
        return args, net, draws, "_draws", dict(vids=[3, 9, 16])
    args, net, eps = joint_embed
    return args, net, eps, "eps_list", dict(window_decoder=True)                 # the stream runs on a JointEmbedWindowDecoder: so must the yardstick


def rows_of(draws, rows):
    return [d[rows] for d in draws]


_audio = {}


def audio_of(n, b=0):
    if (n, b) not in _audio:
        _audio[n, b] = U.make_audio(n, 700 + 13 * b + n % 97)
    return _audio[n, b]


_offline = {}


def offline(syn, name, n, model, rows=(0,), **opts):
    """generate_gestures_batch(on_device=True) on the finished utterances of `rows`, computed once per case and shared."""
    key = (name, n, tuple(rows), tuple(sorted(opts.items())))
    if key not in _offline:
        args, net, draws, dkw, kw = model
        kw = dict(kw)
        if "vids" in kw:
            kw["vids"] = [kw["vids"][b] for b in rows]
        kw[dkw] = rows_of(draws, list(rows))
        _offline[key] = syn.generate_gestures_batch(args, net, U.Lang(), [audio_of(n, b) for b in rows],
                                                    [R.words_until(R.ROW_WORDS[b], n / U.SR) for b in rows], on_device=True, **kw, **opts)
    return _offline[key]


def run_stream(syn, model, n, chunk, rows=(0,), check_schedule=False, close_opts=None, **ctor):
    """A stream over the utterances of `rows` in pushes of `chunk` samples -> (pieces of push, what close returned, the stream).  st.copies:
    a copy of every non-empty piece taken the moment push returned it (a stream-ordered device copy: it holds what the piece held then)."""
    args, net, draws, dkw, kw = model
    rows = list(rows)
    ctor.setdefault("max_chunk", max(chunk, 1))
    ctor[dkw] = rows_of(draws, rows)
    if "vids" in kw:
        ctor["vids"] = [kw["vids"][b] for b in rows]
    st = syn.GestureStream(args, net, U.Lang(), batch=len(rows), **ctor)
    audio = np.stack([audio_of(n, b) for b in rows])
    pieces, frames, st.copies = [], 0, []
    for p in range(0, n, chunk):
        q = min(p + chunk, n)
        words = [R.words_until(R.ROW_WORDS[b], q / U.SR, p / U.SR) for b in rows]
        pieces.append(st.push(audio[:, p:q], words if any(words) else None))
        frames += pieces[-1].shape[1]
        if pieces[-1].shape[1]:
            st.copies.append(pieces[-1].clone())
        if check_schedule:
            assert frames == syn.complete_windows(q, S, A) * STRIDE, (q, frames)
    return pieces, st.close(**(close_opts or {})), st


CHUNKS = {"160": 160, "irregular_1237": 1237, "single_push": None}


@pytest.mark.parametrize("chunking", list(CHUNKS))
@pytest.mark.parametrize("length", list(R.LENGTHS))
@pytest.mark.parametrize("name", ["multimodal", "joint_embedding"])
def test_stream_is_bit_equal_to_the_offline_result(syn, dev, multimodal, joint_embed, name, length, chunking):
    """Also early availability: after every push the frames returned so far are complete_windows(pushed) * stride, and a piece never changes
    after it was returned: the copy taken at that moment equals the piece as it reads after every later push and close, and both are the
    final result's frames."""
    n, model = R.LENGTHS[length], model_of(name, multimodal, joint_embed)
    assert syn.stream_matches_offline(model[0], n)
    want = offline(syn, name, n, model)[0]
    pieces, last, st = run_stream(syn, model, n, CHUNKS[chunking] or n, check_schedule=True)
    got = torch.cat(pieces + [last], dim=1)
    early = torch.cat(st.copies + [last], dim=1)
    assert len(st.copies) == sum(1 for p in pieces if p.shape[1]) and torch.equal(early, got)
    assert tuple(got.shape) == (1,) + want.shape and got.dtype == torch.float32 and st.late_words == 0
    assert last.shape[1] == want.shape[0] - syn.complete_windows(n, S, A) * STRIDE
    assert np.array_equal(bits(got[0]), bits(want)), f"max |diff| {float(np.abs(got[0].cpu().numpy() - want).max()):.3e}"


@pytest.mark.parametrize("length", ["under_one_window", "exactly_A", "three_windows_padded"])
@pytest.mark.parametrize("name", ["multimodal", "joint_embedding"])
def test_close_options_fade_out_and_joints(syn, dev, multimodal, joint_embed, name, length):
    """exactly_A: the last window ran in a push, close returns its final n_pre frames (and the fade-out's zero frames); the other two lengths end
    inside a padded window that close itself runs."""
    n, model = R.LENGTHS[length], model_of(name, multimodal, joint_embed)
    want = offline(syn, name, n, model, fade_out=True)[0]
    pieces, last, _ = run_stream(syn, model, n, 4099, close_opts=dict(fade_out=True))
    got = torch.cat(pieces + [last], dim=1)[0]
    assert np.array_equal(bits(got), bits(want)), (got.shape, want.shape)
    want, want_j = (x[0] for x in offline(syn, name, n, model, joints=True))
    args, net, draws, dkw, kw = model
    st = syn.GestureStream(args, net, U.Lang(), max_chunk=4099, **{dkw: rows_of(draws, [0])}, **({"vids": [3]} if "vids" in kw else {}))
    fr, jt = [], []
    for p in range(0, n, 4099):
        q = min(p + 4099, n)
        f, j = st.push(audio_of(n)[p:q], R.words_until(R.WORDS, q / U.SR, p / U.SR), joints=True)
        fr.append(f); jt.append(j)
    f, j = st.close(joints=True, numpy=True)
    got = np.concatenate([x.cpu().numpy() for x in fr] + [f], axis=1)[0]
    got_j = np.concatenate([x.cpu().numpy() for x in jt] + [j], axis=1)[0]
    assert got_j.dtype == np.float64 and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_j), bits(want_j))


@pytest.mark.parametrize("name", ["multimodal", "joint_embedding"])
def test_three_rows_share_a_clock(syn, dev, multimodal, joint_embed, name):
    """B = 3 against the B = 3 offline batch, for both models.  Neither decoder path promises rows that keep their bits from B = 1 to B = 3: the
    products of the generator and of the context encoder choose kernels by their row count.  Measured on the MI355X: the rows of a B = 3
    joint-embedding stream differ from three B = 1 streams in the last bits (about 10 fp32 ulps on the first elements), exactly as the B = 3
    and B = 1 offline results differ from each other -- each stream is bit-equal to the offline call of its own batch size (the B = 1 cases
    above).  So the yardstick here is the B = 3 offline batch alone."""
    n, model = R.LENGTHS["three_windows_padded"], model_of(name, multimodal, joint_embed)
    want = offline(syn, name, n, model, rows=(0, 1, 2))
    pieces, last, st = run_stream(syn, model, n, 1237, rows=(0, 1, 2), check_schedule=True)
    got = torch.cat(pieces + [last], dim=1)
    assert st.late_words == 0
    for b in range(3):
        assert np.array_equal(bits(got[b]), bits(want[b])), b


@pytest.mark.parametrize("name", ["multimodal", "joint_embedding"])
def test_a_second_stream_on_a_kept_decoder_replays_the_graph(syn, dev, multimodal, joint_embed, name):
    n, model = R.LENGTHS["three_windows_padded"], model_of(name, multimodal, joint_embed)
    args, net = model[0], model[1]
    if name == "multimodal":
        dec = syn.WindowDecoder(args, net, 1, dev, graph=True, replay_draws=True)
    else:
        dec = syn.JointEmbedWindowDecoder(args, net, 1, dev, graph=True, replay_draws=True)
    runs = []
    for _ in range(2):
        pieces, last, _ = run_stream(syn, model, n, 1237, window_decoder=dec)
        runs.append(torch.cat(pieces + [last], dim=1).clone())
        assert dec.graph is not None
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    assert np.array_equal(bits(runs[0][0]), bits(offline(syn, name, n, model)[0]))
    with pytest.raises(ValueError, match="window_decoder must be"):
        syn.GestureStream(args, net, U.Lang(), batch=2, window_decoder=dec, **{model[3]: model[2]})


def test_refusals(syn, dev, multimodal):
    args, net, draws = multimodal
    st = syn.GestureStream(args, net, U.Lang(), max_chunk=100, vids=[3], _draws=rows_of(draws, [0]))
    with pytest.raises(ValueError, match="max_chunk is 100"):
        st.push(np.zeros(101, np.float32))
    with pytest.raises(ValueError, match="must be float32"):
        st.push(np.zeros(10, np.float64))
    with pytest.raises(ValueError, match="must be float32"):
        st.push(torch.zeros(1, 10, dtype=torch.float16, device=dev))
    with pytest.raises(ValueError, match="expected"):
        st.push(np.zeros((2, 10), np.float32))
    with pytest.raises(ValueError, match="nothing was pushed"):
        st.close()
    assert st.push(np.zeros(100, np.float32)).shape == (1, 0, U.D) and st.pushed == 100          # the refused calls pushed nothing
    assert st.close().shape == (1, T, U.D)
    with pytest.raises(ValueError, match="the stream is closed"):
        st.push(np.zeros(10, np.float32))
    for model, why in (("seq2seq", "smoothing rewrites frames"), ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match=why):
            syn.GestureStream(U.make_args(model), net, U.Lang())
    with pytest.raises(ValueError, match="1 to 4 rows"):
        syn.GestureStream(args, net, U.Lang(), batch=5)
    with pytest.raises(ValueError, match="word ring's capacity"):
        few = syn.GestureStream(args, net, U.Lang(), vids=[3], _draws=rows_of(draws, [0]), word_ring=4)
        few.push(np.zeros(10, np.float32), R.WORDS)


def test_a_late_word_is_counted_and_changes_no_emitted_frame(syn, dev, multimodal):
    """The same utterance twice; the second stream learns of a word of window 0 (and of the overlap with window 1) only after window 0 ran: it is
    counted once, window 0's frames are those of a stream that never heard the word, and window 1 -- not yet run -- does get it."""
    args, net, draws = multimodal
    n, late = 90000, ["overlap", 2.1, 2.2]
    audio, words = audio_of(n), [w for w in R.WORDS if w[0] != "overlap"]
    kw = dict(max_chunk=40000, vids=[3], _draws=rows_of(draws, [0]))
    never = syn.GestureStream(args, net, U.Lang(), **kw)
    a0 = never.push(audio[:40000], words).clone()
    heard = syn.GestureStream(args, net, U.Lang(), **kw)
    b0 = heard.push(audio[:40000], words)                                        # (kept as returned: later pushes must not write into it)
    assert a0.shape == (1, STRIDE, U.D) and torch.equal(a0, b0)
    a1 = never.push(audio[40000:80000])
    b1 = heard.push(audio[40000:80000], [late])
    assert heard.late_words == 1 and never.late_words == 0
    assert torch.equal(b0, a0)
    ids = heard.dec.text[0].cpu().numpy()                                         # window 1's text as it was staged
    want = syn.window_inputs(args, U.Lang(), audio, sorted(words + [late], key=lambda w: w[1]), 1)[1]
    assert np.array_equal(ids, want) and (ids == U.Lang().get_word_index("overlap")).any()
    assert a1.shape == b1.shape == (1, STRIDE, U.D) and not torch.equal(a1[:, N_PRE:], b1[:, N_PRE:])
