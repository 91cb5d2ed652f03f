"""Long-utterance synthesis on the device (csrc/utterance.hip, synthesize.UtteranceBatch, generate_gestures*(on_device=True)).

Staging moves bits, so tg_window_stage / tg_spec_stage and every on_device forward must be BIT-EQUAL to the default (host) path: the forward is
the same code on bit-equal inputs.  The fits of tg_utterance_finish and numpy's polyfit both compute in fp64 (agreement near 1e-13 relative,
tests/test_utterance_cpu.py) and round once to fp32: an element may differ by one fp32 ulp at the segment's scale, 2^-23 x the largest
magnitude among the fitted segment's inputs and the reference's outputs; everything outside the fitted segments and the zeroed tail is
bit-equal.  Joint positions are emitted in fp64 and gated at 1e-12 absolute against convert_dir_vec_to_pose on fp64 numpy."""
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import utterance_ref as U

pytestmark = pytest.mark.gpu
H_SMALL, LAYERS_SMALL = 32, 2                      # the generators under test: small, their decoders are general in both
ULP = 2.0 ** -23
# 1, 2 and 3 windows; the first length is odd, so the second utterance starts at an odd offset of the packed buffer
LENGTHS = [20001, 50000, 100001]
WORDS = [U.WORD_LISTS["two_on_one_frame"], U.WORD_LISTS["starts_before_window"], U.WORD_LISTS["starts_at_end_time"]]
L = int(U.N_POSES / U.FPS * U.SR)


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


@pytest.fixture(scope="module")
def audios():
    return [U.make_audio(n, 100 + n) for n in LENGTHS]


def guarded(shape, dev, dtype=torch.float32, fill=7):
    """A contiguous tensor of `shape` between two guard rows that must keep their fill."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev)
    return buf, buf[1:-1]


def guards_intact(buf, fill=7):
    return bool((buf[0] == fill).all()) and bool((buf[-1] == fill).all())


# ------------------------------------------------------------------------------------------------------------------ staging
def test_window_stage_is_bit_equal_to_window_inputs(syn, dev, audios):
    args, lang = U.make_args(), U.Lang()
    ub = syn.UtteranceBatch(args, lang, audios, WORDS, dev)
    assert ub.n_win == [1, 2, 3] and int(ub.plan["audio_off"][1]) % 2 == 1
    for i in range(3):
        want = [syn.window_inputs(args, lang, a, w, min(i, n - 1)) for a, w, n in zip(audios, WORDS, ub.n_win)]       # idle rows repeat their last window
        runs = []
        for _ in range(2):
            abuf, a_out = guarded((3, L), dev)
            tbuf, t_out = guarded((3, U.N_POSES), dev, torch.int64)
            ub.stage(i, t_out, a_out)
            torch.cuda.synchronize()
            assert guards_intact(abuf) and guards_intact(tbuf)
            runs.append((a_out.cpu().numpy(), t_out.cpu().numpy()))
        assert np.array_equal(runs[0][0].view(np.uint32), np.stack([w[0] for w in want]).view(np.uint32))
        assert np.array_equal(runs[0][1], np.stack([w[1] for w in want]))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # text or audio alone
    abuf, a_out = guarded((3, L), dev)
    ub.stage(2, None, a_out)
    assert np.array_equal(a_out.cpu().numpy(), runs[0][0]) and guards_intact(abuf)
    with pytest.raises(IndexError):
        ub.stage(3, None, a_out)


def test_window_stage_seq2seq_lists_and_spectrogram_slices(syn, dev, audios):
    lang = U.Lang()
    ub = syn.UtteranceBatch(U.make_args("seq2seq"), lang, audios, WORDS, dev)
    for i in range(3):
        texts = [syn.seq2seq_window_text(lang, w, min(i, n - 1)) for w, n in zip(WORDS, ub.n_win)]
        assert ub.seq_lens(i) == [len(t) for t in texts]
        want = np.zeros((3, max(map(len, texts))), np.int64)
        for b, t in enumerate(texts):
            want[b, :len(t)] = t
        out = ub.text_buffer(want.shape[1])
        out.fill_(-5)
        ub.stage(i, text_out=out)
        assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError):
        ub.stage(0, audio_out=torch.zeros(3, L, device=dev))                   # this model's batch holds no samples
    # spectrogram slices: random (128, frames) spectrograms, one of them too short for a full last slice
    sa = U.make_args("speech2gesture")
    ub = syn.UtteranceBatch(sa, None, audios, None, dev)
    width, g = syn.spec_slice_length(U.N_POSES, U.FPS), torch.Generator().manual_seed(3)
    for dtype in (torch.float16, torch.float32):
        specs = [torch.randn(128, f, generator=g).to(dtype).to(dev) for f in (40, 98, 196)]      # 98 < 64 + 71: window 1 of utterance 1 is short
        ub.set_spectrograms(specs)
        for i in range(3):
            starts = [syn.spec_window_start(min(i, n - 1), len(a) / U.SR) for a, n in zip(audios, ub.n_win)]
            buf, out = guarded((3, 128, width), dev, dtype)
            ub.stage_spec(i, out)
            torch.cuda.synchronize()
            assert guards_intact(buf)
            for b in range(3):
                piece = specs[b][:, starts[b]:starts[b] + width]
                assert ub.spec_widths(i, width)[b] == piece.shape[1]
                assert torch.equal(out[b, :, :piece.shape[1]], piece) and not out[b, :, piece.shape[1]:].any()


# ------------------------------------------------------------------------------------------------------------------ finish
def segment_bound(before, ref, s, e):
    return ULP * max(float(np.abs(before[s:min(e, len(before))]).max(initial=0.0)), float(np.abs(ref[s:e]).max(initial=0.0)))


def check_smooth(tag, got, before, ref, n_win):
    assert got.shape == ref.shape and got.dtype == np.float32
    fitted = np.zeros(len(ref), bool)
    for s, e in U.smooth_segments(n_win):
        err, bound = float(np.abs(got[s:e].astype(np.float64) - ref[s:e]).max()), segment_bound(before, ref, s, e)
        print(f"{tag} smoothing [{s}, {e}): error {err:.3e} bound {bound:.3e}")
        assert err <= bound, (tag, s, err, bound)
        fitted[s:e] = True
    assert np.array_equal(got[~fitted], ref[~fitted])


def check_fade(tag, got, before, ref, start, head_equal=True):
    """head_equal=False: the frames in front of the fade went through the smoothing and were checked by check_smooth."""
    assert got.shape == ref.shape and got.dtype == np.float32, (tag, got.shape, ref.shape)
    s, e = start, start + 2 * U.N_PRE
    err, bound = float(np.abs(got[s:e].astype(np.float64) - ref[s:e]).max()), segment_bound(before, ref, s, e)
    print(f"{tag} fade-out [{s}, {e}): error {err:.3e} bound {bound:.3e}")
    assert err <= bound, (tag, err, bound)
    assert (not head_equal or np.array_equal(got[:s], ref[:s])) and not got[e:].any() and not ref[e:].any()


def test_utterance_finish_against_numpy(syn, dev, audios, pkg):
    """The three parts of tg_utterance_finish on random stacked windows of 1, 2 and 3 windows (fade-out: 20001 and 50000 samples end inside the last
    window, no padding of the result; 100001 samples fill theirs and the result grows), twice, bit-identical."""
    rng = np.random.default_rng(9)
    mean = rng.standard_normal(U.D)
    args = U.make_args("seq2seq", mean_dir_vec=mean.tolist())
    ub = syn.UtteranceBatch(args, U.Lang(), audios, WORDS, dev)
    F = ub.frames(fade_out=True)
    base = rng.standard_normal((3, F, U.D)).astype(np.float32)               # rows are random past their length too: the kernel must not use that
    runs = []
    for _ in range(2):
        total = torch.from_numpy(base).to(dev)
        rows, jrows = ub.finish(total, fade_out=True, joints=True)
        torch.cuda.synchronize()
        runs.append(([r.cpu().numpy() for r in rows], [j.cpu().numpy() for j in jrows]))
    for b in range(3):
        n_frames = ub.lengths[b]
        before = base[b, :n_frames].copy()
        smoothed = syn.seq2seq_smooth(before.copy(), ub.n_win[b])
        pad = syn.end_padding_samples(args, LENGTHS[b])
        ref = syn.fade_out_to_mean(smoothed.copy(), pad, args)
        start = syn._fade_start_frame(n_frames, pad, args)
        got, joints = runs[0][0][b], runs[0][1][b]
        assert (len(ref) > n_frames) == (b == 2)
        check_smooth(f"row {b}", got[:min(start, n_frames)], before[:min(start, n_frames)], smoothed[:min(start, n_frames)],
                     sum(1 for s, e in U.smooth_segments(ub.n_win[b]) if e <= start))
        assert all(e <= start or s >= start + 2 * U.N_PRE for s, e in U.smooth_segments(ub.n_win[b]))       # the fade's inputs are untouched by the smoothing
        check_fade(f"row {b}", got, smoothed, ref, start, head_equal=False)
        want_j = pkg.eval_metrics.convert_dir_vec_to_pose(got.astype(np.float64) + mean)
        assert joints.dtype == np.float64 and joints.shape == want_j.shape
        jerr = float(np.abs(joints - want_j).max())
        print(f"row {b} joints: error {jerr:.3e} (gate 1e-12)")
        assert jerr <= 1e-12
        assert np.array_equal(got, runs[1][0][b]) and np.array_equal(joints, runs[1][1][b])
    # smoothing alone leaves everything outside the segments as it was, and rows stop at their own window count
    total = torch.from_numpy(base).to(dev)
    rows, none = ub.finish(total)
    assert none is None
    for b in range(3):
        before = base[b, :ub.lengths[b]].copy()
        check_smooth(f"row {b} alone", rows[b].cpu().numpy(), before, syn.seq2seq_smooth(before.copy(), ub.n_win[b]), ub.n_win[b])
        assert np.array_equal(total[b, ub.lengths[b]:].cpu().numpy(), base[b, ub.lengths[b]:])


@pytest.mark.parametrize("case", ["n_pre_9", "D_65"])
def test_utterance_finish_refuses_shapes_outside_its_envelope(pkg, dev, case):
    n_pre, n_poses, D = (9, 40, 27) if case == "n_pre_9" else (4, 34, 65)
    buf, total = guarded((2, 2 * (n_poses - n_pre) + 3 * n_pre, D), dev)
    total.fill_(3)
    n_win = torch.tensor([2, 1], dtype=torch.int32, device=dev)
    proj = torch.full((13 * n_pre * n_pre,), 0.5, dtype=torch.float64, device=dev)
    fade = torch.tensor([40, 20], dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="envelope"):
        pkg.ops.utterance_finish(total, n_win, 2, n_poses, n_pre, smooth=True, proj=proj, fade_start=fade)
    torch.cuda.synchronize()
    assert bool((total == 3).all()) and guards_intact(buf)


# ------------------------------------------------------------------------------------------------------------------ the models
def same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = (v.cpu().numpy() if isinstance(v, torch.Tensor) else v for v in (x, y))
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.fixture(scope="module")
def multimodal(pkg, dev):
    from harness import make_args
    torch.manual_seed(11)
    args = make_args(hidden_size=H_SMALL, n_layers=LAYERS_SMALL, z_type="speaker")
    args.motion_resampling_framerate = U.FPS
    args.mean_dir_vec = np.random.default_rng(12).standard_normal(U.D).tolist()
    G = pkg.PoseGenerator(args, U.D, U.V, H_SMALL, None, pkg.Vocab.speakers(U.N_SPEAKERS)).to(dev).eval()
    draws = [torch.randn(3, 16, generator=torch.Generator().manual_seed(20 + i)) for i in range(3)]
    return args, G, draws


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_multimodal_on_device_is_bit_equal(syn, dev, audios, multimodal, graph):
    args, G, draws = multimodal
    kw = dict(vids=[3, 9, 16], graph=graph, _draws=draws)
    ref = syn.generate_gestures_batch(args, G, U.Lang(), audios, WORDS, **kw)
    got = syn.generate_gestures_batch(args, G, U.Lang(), audios, WORDS, on_device=True, **kw)
    same_rows(got, ref)
    rows, joints = syn.generate_gestures_batch(args, G, U.Lang(), audios, WORDS, on_device=True, return_device=True, joints=True, **kw)
    assert all(isinstance(r, torch.Tensor) and r.is_cuda for r in rows) and all(j.is_cuda and j.dtype == torch.float64 for j in joints)
    same_rows(rows, ref)
    mean = np.asarray(args.mean_dir_vec)
    ev = import_module(syn.__name__.rsplit(".", 1)[0] + ".eval_metrics")
    for r, j in zip(ref, joints):
        assert float(np.abs(j.cpu().numpy() - ev.convert_dir_vec_to_pose(r.astype(np.float64) + mean)).max()) <= 1e-12


@pytest.mark.parametrize("b", [2, 1], ids=["padded_result", "ends_inside_the_window"])
def test_multimodal_fade_out_on_device(syn, dev, audios, multimodal, b):
    args, G, draws = multimodal
    kw = dict(vid=5, _draws=[d[:1] for d in draws])
    plain = syn.generate_gestures(args, G, U.Lang(), audios[b], WORDS[b], **kw)
    ref = syn.generate_gestures(args, G, U.Lang(), audios[b], WORDS[b], fade_out=True, **kw)
    got = syn.generate_gestures(args, G, U.Lang(), audios[b], WORDS[b], fade_out=True, on_device=True, **kw)
    start = syn._fade_start_frame(len(plain), syn.end_padding_samples(args, LENGTHS[b]), args)
    assert (len(ref) > len(plain)) == (b == 2)
    check_fade(f"multimodal utterance {b}", got, plain, ref, start)


@pytest.fixture(scope="module")
def joint_embed(pkg, dev):
    torch.manual_seed(13)
    args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=U.N_PRE,
                           n_poses=U.N_POSES, z_type="none", motion_resampling_framerate=U.FPS, wordembed_dim=300, mean_dir_vec=[0.0] * U.D)
    net = pkg.EmbeddingNet(args, U.D, U.N_POSES, U.V, 300, None, mode="random").to(dev).eval()       # (its GRUs have the reference's fixed sizes)
    eps = [torch.randn(3, 32, generator=torch.Generator().manual_seed(30 + i)) for i in range(3)]
    return args, net, eps


@pytest.mark.parametrize("window_decoder", [False, True], ids=["per_window", "window_decoder"])
def test_joint_embedding_on_device_is_bit_equal(syn, dev, audios, joint_embed, window_decoder):
    args, net, eps = joint_embed
    kw = dict(eps_list=eps, window_decoder=window_decoder)
    ref = syn.generate_gestures_batch(args, net, U.Lang(), audios, WORDS, **kw)
    same_rows(syn.generate_gestures_batch(args, net, U.Lang(), audios, WORDS, on_device=True, **kw), ref)
    same_rows(syn.generate_gestures_batch(args, net, U.Lang(), audios, WORDS, on_device=True, return_device=True, **kw), ref)


def test_speech2gesture_on_device_is_bit_equal(pkg, syn, dev):
    from test_s2g_synthesis_gpu import make_generator, s2g_args, utterance
    gen = make_generator(pkg, dev)
    auds = [utterance(6.3, 2), utterance(8.0, 3), utterance(11.0, 4)]              # 6.3 s: the last slice is one frame short
    ref = syn.generate_gestures_batch(s2g_args(), gen, None, auds, None)
    same_rows(syn.generate_gestures_batch(s2g_args(), gen, None, auds, None, on_device=True), ref)
    same_rows(syn.generate_gestures_batch(s2g_args(), gen, None, auds, None, on_device=True, return_device=True), ref)


@pytest.fixture(scope="module")
def seq2seq(pkg, dev):
    torch.manual_seed(14)
    args = SimpleNamespace(model="seq2seq", hidden_size=H_SMALL, n_layers=LAYERS_SMALL, dropout_prob=0.0, n_pre_poses=U.N_PRE, n_poses=U.N_POSES,
                           GAN_noise_size=0, motion_resampling_framerate=U.FPS, z_type="none", mean_dir_vec=[0.0] * U.D)
    return args, pkg.Seq2SeqNet(args, U.D, U.N_POSES, U.V, 16, None).to(dev).eval()


def test_seq2seq_on_device_against_the_numpy_smoothing(syn, dev, audios, seq2seq):
    args, net = seq2seq
    raw, n_win = syn._seq2seq_gestures_batch(args, net, U.Lang(), audios, WORDS, None, U.SR)        # the stacked windows before the fit
    raw = [r.copy() for r in raw]
    ref = syn.generate_gestures_batch(args, net, U.Lang(), audios, WORDS)
    got = syn.generate_gestures_batch(args, net, U.Lang(), audios, WORDS, on_device=True)
    dev_rows = syn.generate_gestures_batch(args, net, U.Lang(), audios, WORDS, on_device=True, return_device=True)
    for b in range(3):
        check_smooth(f"seq2seq utterance {b}", got[b], raw[b], ref[b], n_win[b])
    same_rows(dev_rows, got)


@pytest.mark.parametrize("b", [2, 1], ids=["padded_result", "ends_inside_the_window"])
def test_seq2seq_fade_out_on_device(syn, dev, audios, seq2seq, b):
    args, net = seq2seq
    plain = syn.generate_gestures(args, net, U.Lang(), audios[b], WORDS[b])
    ref = syn.generate_gestures(args, net, U.Lang(), audios[b], WORDS[b], fade_out=True)
    got = syn.generate_gestures(args, net, U.Lang(), audios[b], WORDS[b], fade_out=True, on_device=True)
    start = syn._fade_start_frame(len(plain), syn.end_padding_samples(args, LENGTHS[b]), args)
    n_win = syn.num_windows(LENGTHS[b] / U.SR)
    raw = syn._seq2seq_gestures_batch(args, net, U.Lang(), [audios[b]], [WORDS[b]], None, U.SR)[0][0].copy()    # the stacked windows before the fit
    keep = min(start, len(plain))
    assert (len(ref) > len(plain)) == (b == 2) and all(e <= keep for s, e in U.smooth_segments(n_win))      # the fade's inputs are untouched by the smoothing
    check_smooth(f"seq2seq utterance {b}", got[:keep], raw[:keep], ref[:keep], n_win)
    check_fade(f"seq2seq utterance {b}", got, plain, ref, start, head_equal=False)
