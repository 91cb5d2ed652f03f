"""Seq2Seq streaming on the GPU (csrc/stream_seq.hip, synthesize.Seq2SeqWindowDecoder / Seq2SeqGestureStream).

tg_stream_stage_text copies integers: it is compared with its host model exactly.  End to end, everything push() and close() return,
concatenated, must be BIT-EQUAL to generate_gestures_batch(on_device=True) on the finished utterance with the encoder's row_local_eval set to
the stream's row_local_encoder: the window texts are equal (tests/test_seq2seq_stream_cpu.py), a row's result depends neither on the text
buffer's width nor on the other rows, and smoothing a window when it runs is the offline smoothing -- so there is no tolerance.  Every
length used here satisfies stream_matches_offline."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seq2seq_stream_ref as SR
import stream_ref as R
import utterance_ref as U
from test_utterance_gpu import guarded, guards_intact, seq2seq          # the small Seq2SeqNet of the on-device utterance tests

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE
MAX_CHUNK = 40000


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


@pytest.fixture(scope="module")
def shipped(pkg, dev):
    """hidden_size 200, n_layers 2: the shipped Seq2Seq configuration."""
    torch.manual_seed(15)
    args = SimpleNamespace(model="seq2seq", hidden_size=200, n_layers=2, dropout_prob=0.0, n_pre_poses=U.N_PRE, n_poses=U.N_POSES,
                           GAN_noise_size=0, motion_resampling_framerate=U.FPS, z_type="none", mean_dir_vec=[0.0] * U.D)
    return args, pkg.Seq2SeqNet(args, U.D, U.N_POSES, U.V, 16, None).to(dev).eval()


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------ the kernel against its host model
@pytest.mark.parametrize("B", [1, 4])
def test_stage_text_against_its_host_model(pkg, dev, B):
    """A word ring of 8 slots that wraps, max_words = 5 (Te = 7): windows with no word, with exactly max_words words and -- the clamp -- with
    more; records of other windows in between; the output buffers start as garbage and lie between guard rows."""
    ops, W, Te, sos, eos = pkg.ops, 8, 7, 1, 2
    st = ops.stream_state(B, A + 1, S, A, W, T, dev)
    st["words"].fill_(-7)
    one = torch.zeros(B, 1, device=dev)
    pushed = [[] for _ in range(B)]

    def push(rows, live):
        m = max(len(r) for r in rows)
        table = np.zeros((B, 1 + 3 * m), np.int32)
        for b, r in enumerate(rows):
            table[b, 0] = len(r)
            table[b, 1:1 + 3 * len(r)] = np.asarray(r, np.int32).reshape(-1) if r else []
            pushed[b] += r
        ops.stream_push(st, one, torch.from_numpy(table).to(dev), m, live)

    def check(window):
        tbuf, t_out = guarded((B, Te), dev, torch.int64, fill=-5)
        lbuf, l_out = guarded((B,), dev, torch.int64, fill=-5)
        ops.stream_stage_text(st, sos, eos, t_out, l_out)
        torch.cuda.synchronize()
        assert guards_intact(tbuf, -5) and guards_intact(lbuf, -5)
        for b in range(B):
            text, ln = SR.stage_text_model(pushed[b], window, Te, sos, eos, ring=W)
            assert int(l_out[b]) == ln and np.array_equal(t_out[b].cpu().numpy(), text), (window, b, t_out[b].tolist(), text)
        return l_out.tolist()

    # window 0: row 0 exactly max_words words (two on one frame), row 1 none, row 2 one word between records of window 1, row 3 three
    rows = [[(0, 3, 11), (0, 3, 12), (1, 0, 90), (0, 9, 13), (0, 20, 14), (0, 33, 15)], [(1, 5, 21)], [(1, 0, 31), (0, 7, 32), (1, 2, 33)],
            [(0, 1, 41), (0, 2, 42), (0, 30, 43)]][:B]
    push(rows, 0)
    assert check(0) == [7, 2, 3, 5][:B]
    # five more records per row: the ring wraps, the oldest records are gone; window 1 of row 0 now has six records in the ring: clamped
    more = [[(1, 1, 51), (1, 2, 52), (1, 3, 53), (1, 4, 54), (1, 5, 55)], [(1, 6, 61), (2, 0, 62), (1, 7, 63), (1, 8, 64), (1, 9, 65)],
            [(2, 0, 71), (1, 3, 72), (2, 1, 73), (1, 4, 74), (2, 2, 75)], [(1, 0, 81), (1, 0, 82), (2, 5, 83), (1, 1, 84), (1, 33, 85)]][:B]
    push(more, 3)
    ops.counter_inc(st["win"])
    assert check(1) == [7, 7, 6, 6][:B]
    ops.counter_inc(st["win"])
    assert check(2) == [2, 3, 5, 3][:B]
    ops.counter_inc(st["win"])
    assert check(3) == [2] * B                                                   # no records at all: [SOS, EOS]
    st5 = ops.stream_state(5, A + 1, S, A, W, T, dev)
    with pytest.raises(RuntimeError, match="envelope"):
        ops.stream_stage_text(st5, sos, eos, torch.zeros(5, Te, dtype=torch.int64, device=dev), torch.zeros(5, dtype=torch.int64, device=dev))


# ------------------------------------------------------------------------------------------------------------------ end to end
_audio, _offline, _seeds = {}, {}, {}


def audio_of(n, b=0):
    if (n, b) not in _audio:
        _audio[n, b] = U.make_audio(n, 900 + 13 * b + n % 97)
    return _audio[n, b]


def seeds_of(rows):
    key = tuple(rows)
    if key not in _seeds:
        _seeds[key] = [np.random.default_rng(60 + b).standard_normal((N_PRE + 1, U.D)).astype(np.float32) for b in rows]
    return _seeds[key]


def offline(syn, tag, model, n, rows=(0,), row_local=True, seeded=False, **opts):
    """generate_gestures_batch(on_device=True) on the finished utterances of `rows` with the encoder's row_local_eval = row_local, computed once
    per case and shared."""
    key = (tag, n, tuple(rows), row_local, seeded, tuple(sorted(opts.items())))
    if key not in _offline:
        args, net = model
        net.encoder.row_local_eval = row_local
        try:
            _offline[key] = syn.generate_gestures_batch(args, net, U.Lang(), [audio_of(n, b) for b in rows],
                                                        [R.words_until(R.ROW_WORDS[b], n / U.SR) for b in rows],
                                                        seed_seqs=seeds_of(rows) if seeded else None, on_device=True, **opts)
        finally:
            net.encoder.row_local_eval = False
    return _offline[key]


def schedule(n, chunking):
    if chunking == "160":
        return [160] * (n // 160) + ([n % 160] if n % 160 else [])
    if chunking == "max_chunk":
        return [MAX_CHUNK] * (n // MAX_CHUNK) + ([n % MAX_CHUNK] if n % MAX_CHUNK else [])
    sizes, out, left, k = [1, 36265, 7, 4099, 39999, 1237], [], n, 0       # ragged: one sample, almost a window, small and large pieces in turn
    while left:
        out.append(min(sizes[k % len(sizes)], left)); left -= out[-1]; k += 1
    return out


def run_stream(syn, model, n, chunking, rows=(0,), close_opts=None, seeded=False, push_joints=False, **ctor):
    """A stream over the utterances of `rows` -> (pieces of push, what close returned, the stream).  After every push the frames handed out so
    far must be complete_windows(pushed) * stride: no extra lag."""
    args, net = model
    rows = list(rows)
    st = syn.Seq2SeqGestureStream(args, net, U.Lang(), batch=len(rows), max_chunk=MAX_CHUNK, seed_seqs=seeds_of(rows) if seeded else None, **ctor)
    audio = np.stack([audio_of(n, b) for b in rows])
    pieces, frames, p = [], 0, 0
    for c in schedule(n, chunking):
        q = p + c
        words = [R.words_until(R.ROW_WORDS[b], q / U.SR, p / U.SR) for b in rows]
        got = st.push(audio[:, p:q], words if any(words) else None, joints=push_joints)
        if (got[0] if push_joints else got).shape[1]:
            pieces.append(tuple(g.clone() for g in got) if push_joints else got.clone())
            frames += (got[0] if push_joints else got).shape[1]
        assert frames == syn.complete_windows(q, S, A) * STRIDE, (q, frames)
        p = q
    return pieces, st.close(**(close_opts or {})), st


@pytest.mark.parametrize("chunking", ["160", "max_chunk", "ragged"])
@pytest.mark.parametrize("length", list(SR.LENGTHS))
def test_stream_is_bit_equal_to_the_offline_result(syn, dev, seq2seq, length, chunking):
    n = SR.LENGTHS[length]
    assert syn.stream_matches_offline(seq2seq[0], n)
    want = offline(syn, "small", seq2seq, n)[0]
    pieces, last, st = run_stream(syn, seq2seq, n, chunking)
    got = torch.cat(pieces + [last], dim=1)
    assert tuple(got.shape) == (1,) + want.shape and got.dtype == torch.float32 and st.late_words == 0
    assert last.shape[1] == want.shape[0] - syn.complete_windows(n, S, A) * STRIDE
    if length in ("exactly_A", "exactly_two"):
        assert last.shape[1] == N_PRE                                            # close ran no window
    assert np.array_equal(bits(got[0]), bits(want)), f"max |diff| {float(np.abs(got[0].cpu().numpy() - want).max()):.3e}"


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("row_local", [True, False], ids=["one_launch_encoder", "per_step_encoder"])
@pytest.mark.parametrize("B", [1, 3])
def test_both_encoders_graph_or_not_one_row_and_three(syn, dev, seq2seq, B, row_local, graph):
    n, rows = SR.LENGTHS["five_windows"], tuple(range(B))
    want = offline(syn, "small", seq2seq, n, rows=rows, row_local=row_local)
    pieces, last, st = run_stream(syn, seq2seq, n, "ragged", rows=rows, row_local_encoder=row_local, graph=graph)
    got = torch.cat(pieces + [last], dim=1)
    assert st.late_words == 0 and (st.dec.graph is not None) == graph and st.dec.row_local == row_local
    assert seq2seq[1].encoder.row_local_eval is False                            # the decoder leaves the module's flag as it found it
    for b in range(B):
        assert np.array_equal(bits(got[b]), bits(want[b])), b


@pytest.mark.parametrize("row_local", [True, False], ids=["one_launch_encoder", "per_step_encoder"])
@pytest.mark.parametrize("length", ["one_window", "exactly_two", "A_plus_1", "five_windows"])
def test_close_options_fade_out_joints_and_seed_poses(syn, dev, seq2seq, length, row_local):
    """exactly_two: the last window ran in a push, close returns its final n_pre frames and the fade-out's growth.  A_plus_1: close runs a second
    window that is all padding but one sample; its fade-out starts inside its smoothing segment, so the order smoothing -> fade-out shows."""
    n, args = SR.LENGTHS[length], seq2seq[0]
    n_win = syn.num_windows(n / U.SR)
    rel = syn._fade_start_frame(n_win * STRIDE + N_PRE, syn.end_padding_samples(args, n), args) - (n_win - 1) * STRIDE
    if length == "A_plus_1":
        assert 0 < rel < 3 * N_PRE
    want = offline(syn, "small", seq2seq, n, row_local=row_local, seeded=True, fade_out=True)[0]
    pieces, last, _ = run_stream(syn, seq2seq, n, "ragged", seeded=True, row_local_encoder=row_local, close_opts=dict(fade_out=True))
    got = torch.cat(pieces + [last], dim=1)[0]
    assert np.array_equal(bits(got), bits(want)), (got.shape, want.shape)
    plain = offline(syn, "small", seq2seq, n, row_local=row_local)[0]
    assert not np.array_equal(plain[:T], want[:T])                                # (the seed poses matter)
    for fade in (False, True):
        want, want_j = (x[0] for x in offline(syn, "small", seq2seq, n, row_local=row_local, joints=True, fade_out=fade))
        pieces, (f, j), _ = run_stream(syn, seq2seq, n, "max_chunk", row_local_encoder=row_local, push_joints=True,
                                       close_opts=dict(joints=True, fade_out=fade, numpy=True))
        got = np.concatenate([x[0].cpu().numpy() for x in pieces] + [f], axis=1)[0]
        got_j = np.concatenate([x[1].cpu().numpy() for x in pieces] + [j], axis=1)[0]
        assert got_j.dtype == np.float64 and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_j), bits(want_j)), fade


@pytest.mark.parametrize("row_local", [True, False], ids=["one_launch_encoder", "per_step_encoder"])
def test_the_shipped_configuration(syn, dev, shipped, row_local):
    n = R.LENGTHS["three_windows_padded"]
    assert syn.stream_matches_offline(shipped[0], n)
    want = offline(syn, "shipped", shipped, n, row_local=row_local, fade_out=True)[0]
    pieces, last, st = run_stream(syn, shipped, n, "ragged", row_local_encoder=row_local, close_opts=dict(fade_out=True))
    assert st.dec.graph is not None
    assert np.array_equal(bits(torch.cat(pieces + [last], dim=1)[0]), bits(want))


# ------------------------------------------------------------------------------------------------------------------ host behaviour
def test_a_late_word_is_counted_and_changes_no_emitted_frame(syn, dev, seq2seq):
    args, net = seq2seq
    n, late = 90000, ["overlap", 2.1, 2.2]
    audio, words = audio_of(n), [w for w in R.WORDS if w[0] != "overlap"]
    never = syn.Seq2SeqGestureStream(args, net, U.Lang(), max_chunk=40000)
    a0 = never.push(audio[:40000], words).clone()
    heard = syn.Seq2SeqGestureStream(args, net, U.Lang(), max_chunk=40000)
    b0 = heard.push(audio[:40000], words)                                        # (kept as returned: later pushes must not write into it)
    assert a0.shape == (1, STRIDE, U.D) and torch.equal(a0, b0)
    a1 = never.push(audio[40000:80000])
    b1 = heard.push(audio[40000:80000], [late])
    assert heard.late_words == 1 and never.late_words == 0 and torch.equal(b0, a0)
    ln = int(heard.dec.len[0])
    text = heard.dec.text[0, :ln].cpu().numpy()                                  # window 1's text as it was staged: the late word last
    want = syn.seq2seq_window_text(U.Lang(), words, 1)
    assert list(text) == list(want[:-1]) + [U.Lang().get_word_index("overlap"), U.Lang().EOS_token]
    assert a1.shape == b1.shape == (1, STRIDE, U.D) and not torch.equal(a1[:, N_PRE:], b1[:, N_PRE:])


def test_a_push_over_max_words_is_refused_and_leaves_the_stream_usable(syn, dev, seq2seq):
    args, net = seq2seq
    n = SR.LENGTHS["exactly_two"]
    words = R.words_until(R.WORDS, n / U.SR)
    want = offline(syn, "small", seq2seq, n)[0]
    st = syn.Seq2SeqGestureStream(args, net, U.Lang(), max_chunk=MAX_CHUNK, max_words=8)
    audio = audio_of(n)
    crowd = [[f"w{j}", 0.5 + 0.01 * j, 0.6 + 0.01 * j] for j in range(9)]
    with pytest.raises(ValueError, match="max_words is 8"):
        st.push(audio[:1000], crowd)
    assert st.pushed == 0 and st.late_words == 0 and st._n_rec == [0] and st._win_words == [{}] and int(st.state["n_words"][0]) == 0
    p, pieces = 0, []
    for c in schedule(n, "max_chunk"):
        pieces.append(st.push(audio[p:p + c], R.words_until(words, (p + c) / U.SR, p / U.SR)).clone())
        p += c
        if p == MAX_CHUNK:                                                       # window 0 ran; window 1 holds two words ("overlap", "end") so far
            assert st.next_window == 1 and st._win_words == [{1: 2}]
            with pytest.raises(ValueError, match="window 1 would hold 10 words, max_words is 8"):
                st.push(audio[:1], [[f"v{j}", 2.5, 2.6] for j in range(8)])
            assert st.pushed == MAX_CHUNK and st.late_words == 0 and st._win_words == [{1: 2}]
    got = torch.cat(pieces + [st.close()], dim=1)[0]
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(ValueError, match="the stream is closed"):
        st.push(audio[:10])


def test_a_second_stream_on_a_kept_decoder_replays_the_graph(syn, dev, seq2seq):
    args, net = seq2seq
    n = SR.LENGTHS["five_windows"]
    dec = syn.Seq2SeqWindowDecoder(args, net, 1, dev, graph=True)
    runs = []
    for _ in range(2):
        pieces, last, _ = run_stream(syn, seq2seq, n, "ragged", window_decoder=dec)
        runs.append(torch.cat(pieces + [last], dim=1).clone())
        assert dec.graph is not None
    assert np.array_equal(bits(runs[0]), bits(runs[1]))
    assert np.array_equal(bits(runs[0][0]), bits(offline(syn, "small", seq2seq, n)[0]))
    for over in (dict(batch=2), dict(max_words=8), dict(row_local_encoder=False)):
        with pytest.raises(ValueError, match="window_decoder must be"):
            syn.Seq2SeqGestureStream(args, net, U.Lang(), window_decoder=dec, **over)


def test_refusals(syn, dev, seq2seq):
    args, net = seq2seq
    for model, why in (("seq2seq", "smoothing rewrites frames"), ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match=why):
            syn.GestureStream(U.make_args(model), net, U.Lang())
    with pytest.raises(ValueError, match="smoothing segment"):
        syn.Seq2SeqGestureStream(SimpleNamespace(**dict(vars(args), n_poses=15)), net, U.Lang())
    with pytest.raises(ValueError, match="the model decodes"):
        syn.Seq2SeqGestureStream(SimpleNamespace(**dict(vars(args), n_poses=64)), net, U.Lang())
    with pytest.raises(ValueError, match="1 to 4 rows"):
        syn.Seq2SeqGestureStream(args, net, U.Lang(), batch=5)
    st = syn.Seq2SeqGestureStream(args, net, U.Lang(), max_chunk=100)
    with pytest.raises(ValueError, match="max_chunk is 100"):
        st.push(np.zeros(101, np.float32))
    with pytest.raises(ValueError, match="nothing was pushed"):
        st.close()
    assert st.push(np.zeros(100, np.float32)).shape == (1, 0, U.D) and st.pushed == 100
    assert st.close().shape == (1, T, U.D)
