"""Speech2Gesture synthesis from raw audio (synthesize.generate_gestures with args.model == 'speech2gesture';
scripts/synthesize.py:42-44,52-56,65,86-93,137-138 with the window loop of :122-126,142-160).

There is no reference fixture for this path: scripts/synthesize.py cannot be imported without librosa and gentle.  The expected output is
built here from pieces pinned elsewhere -- the device spectrogram (tests/test_logmel_gpu.py) pulled to the host, slices by the reference's
formula restated below, the eager Generator.forward per window in eval mode (pinned against the reference by the g13 / g14 tests), and
the cross-fade / vstack as numpy.

Bounds: unblended frames must be bit-identical (the same kernels on the same operands, data movement apart).  The n_pre_poses blended frames of
a window are prev * (n - j) / (n + 1) + next * (j + 1) / (n + 1): two products and a sum, each rounded once in fp32 whatever the order and
contraction, so device and numpy may differ by at most 4 ulps of the larger blended operand."""
import argparse
import math
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from harness import O, fixture_lang, make_args, rel, synth_case
from tests.s2g_inputs import fill_state

pytestmark = pytest.mark.gpu

SR, T, N_PRE, FPS, D = 16000, 34, 4, 15, 27


def s2g_args():
    return argparse.Namespace(model="speech2gesture", n_poses=T, n_pre_poses=N_PRE, motion_resampling_framerate=FPS, mean_dir_vec=[0.0] * D,
                              z_type="none")


def make_generator(pkg, dev, seed=31):
    """Seeded weights (tests/s2g_inputs.fill_state) and non-trivial BatchNorm running statistics, so that eval mode differs from train mode."""
    s2g = import_module(pkg.__name__ + ".speech2gesture")
    G = fill_state(s2g.Generator(T, D, N_PRE), seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in G.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return G.to(dev)


def utterance(seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / SR
    y = sum(np.sin(2 * np.pi * 110 * h * t + rng.uniform(0, 6.28)) / h for h in range(1, 12))
    return (0.1 * y * (0.6 + 0.4 * np.sin(2 * np.pi * 2.5 * t)) + 1e-3 * rng.standard_normal(n)).astype(np.float32)


def expected(pkg, dev, G, audio, seed_seq=None):
    """scripts/synthesize.py:52-65,82-93,122-126,137-160 on the host, the model being the eager Generator.forward at batch 1."""
    spec = pkg.extract_melspectrogram(audio, device=dev).cpu().numpy()               # (128, F) fp16
    clip_length = len(audio) / SR
    unit_time, stride_time = T / FPS, (T - N_PRE) / FPS
    n_sub = 1 if clip_length < unit_time else math.ceil((clip_length - unit_time) / stride_time) + 1
    width = int(round(unit_time * SR / 512))
    pre = np.zeros((1, N_PRE, D), np.float32)
    if seed_seq is not None:
        pre[0] = seed_seq[:N_PRE]
    out_list, blended = [], []
    was = G.training
    G.eval()
    with torch.no_grad():
        for i in range(n_sub):
            a0 = math.floor(i * stride_time / clip_length * spec.shape[0])          # :90, shape[0] = mels
            in_spec = torch.from_numpy(np.ascontiguousarray(spec[:, a0:a0 + width])).unsqueeze(0).to(dev)
            out_seq = G(in_spec, torch.from_numpy(pre).to(dev))[0].cpu().numpy()
            pre = out_seq[None, -N_PRE:].copy()
            lo = np.zeros_like(out_seq[:N_PRE])
            if out_list:
                last = out_list[-1][-N_PRE:]
                out_list[-1] = out_list[-1][:-N_PRE]
                for j in range(N_PRE):
                    lo[j] = np.maximum(np.abs(last[j]), np.abs(out_seq[j]))
                    out_seq[j] = last[j] * (N_PRE - j) / (N_PRE + 1) + out_seq[j] * (j + 1) / (N_PRE + 1)
            blended.append(lo)
            out_list.append(out_seq)
    G.train(was)
    # per-frame bound: 0 (bit-identical) off the blended frames, 4 ulps of the larger operand on them
    tol = np.zeros((n_sub * (T - N_PRE) + N_PRE, D), np.float32)
    for i in range(1, n_sub):
        tol[i * (T - N_PRE):i * (T - N_PRE) + N_PRE] = 4 * np.spacing(blended[i])
    return np.vstack(out_list), tol, n_sub


def assert_matches(out, want, tol, tag):
    assert out.shape == want.shape and out.dtype == np.float32, (tag, out.shape, want.shape)
    diff = np.abs(out.astype(np.float64) - want.astype(np.float64))
    exact = tol == 0
    print(f"s2g synthesis {tag}: unblended max diff {diff[exact].max():.3e}, blended max diff / bound {float((diff[~exact] / tol[~exact]).max()) if (~exact).any() else 0:.3f}")
    assert np.array_equal(out[exact], want[exact]), (tag, float(diff[exact].max()))
    assert (diff <= tol).all(), (tag, float((diff - tol).max()))


@pytest.fixture(scope="module")
def gen(pkg, dev):
    return make_generator(pkg, dev)


@pytest.mark.parametrize("seconds", [8.0, 11.0])
def test_generate_gestures_speech2gesture_equals_window_loop(pkg, dev, gen, seconds):
    syn = pkg.synthesize
    audio = utterance(seconds, int(seconds))
    want, tol, n_sub = expected(pkg, dev, gen, audio)
    assert n_sub == {8.0: 4, 11.0: 6}[seconds] and want.shape == (n_sub * 30 + 4, D)
    for mode in (False, True):                                                    # the generator comes back in the mode it was in
        gen.train(mode)
        out = syn.generate_gestures(s2g_args(), gen, None, audio, None)
        assert gen.training is mode and all(m.training is mode for m in gen.modules())
        assert_matches(out, want, tol, f"{seconds} s train={mode}")
    gen.eval()
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-3 and (tol > 0).sum() == (n_sub - 1) * N_PRE * D


def test_seed_poses_and_fade_out(pkg, dev, gen):
    syn = pkg.synthesize
    gen.eval()
    audio = utterance(8.0, 5)
    seed_seq = np.random.default_rng(7).standard_normal((6, D)).astype(np.float32) * 0.3
    want, tol, _ = expected(pkg, dev, gen, audio, seed_seq)
    plain, _, _ = expected(pkg, dev, gen, audio)
    assert np.abs(want[:30] - plain[:30]).max() > 1e-4                                # the seed reaches the first window
    out = syn.generate_gestures(s2g_args(), gen, None, audio, None, seed_seq=seed_seq)
    assert_matches(out, want, tol, "seed_seq")
    # fade_out: the reference's tail treatment (:188-207) applied to the same frames
    args = s2g_args()
    faded = syn.generate_gestures(args, gen, None, audio, None, seed_seq=seed_seq, fade_out=True)
    pad = syn.end_padding_samples(args, len(audio))
    assert pad == int(T / FPS * SR) - (len(audio) - math.floor(3 * 2.0 / 8.0 * len(audio)))         # :96-102 for the 4th window
    ref = syn.fade_out_to_mean(out.copy(), pad, args)
    assert faded.shape == ref.shape and np.array_equal(faded, ref)
    start = len(out) - int(pad / SR * FPS)
    assert np.array_equal(faded[:start], out[:start]) and not np.array_equal(faded[start:], out[start:len(faded)])


def test_ragged_batch_equals_single_runs(pkg, dev, gen):
    """Two utterances of 4 and 6 windows in lock-step.  Eval-mode BatchNorm uses running statistics and every product row is formed on its own,
    so an utterance's frames do not depend on its neighbour in the batch: the comparison is for equality."""
    syn = pkg.synthesize
    gen.eval()
    audios = [utterance(8.0, 11), utterance(11.0, 12)]
    seeds = [np.full((N_PRE, D), 0.1, np.float32), np.full((N_PRE, D), -0.2, np.float32)]
    both = syn.generate_gestures_batch(s2g_args(), gen, None, audios, None, seed_seqs=seeds)
    assert [b.shape for b in both] == [(124, D), (184, D)]
    for a, s, b in zip(audios, seeds, both):
        one = syn.generate_gestures(s2g_args(), gen, None, a, None, seed_seq=s)
        print("s2g ragged batch vs single: max diff", float(np.abs(one - b).max()))
        assert np.array_equal(one, b)


def test_short_utterance_raises_on_the_device_path_too(pkg, dev, gen):
    with pytest.raises(ValueError, match="minimum"):
        pkg.synthesize.generate_gestures(s2g_args(), gen, None, utterance(5.0, 1), None)
    out = pkg.synthesize.generate_gestures(s2g_args(), gen, None, utterance(6.3, 2), None)
    assert out.shape == (4 * 30 + 4, D)


def test_multimodal_path_is_untouched(pkg, dev):
    """One g9 case through the public function, with args.model == 'multimodal_context': the same gate as tests/test_engine_gpu.py."""
    syn = pkg.synthesize
    g = np.load(GOLDEN + "/g9_generate_gestures.npz", allow_pickle=False)
    V, S = int(g["n_words"]), int(g["n_speakers"])
    name = "w2"
    assert name in [str(c) for c in g["cases"]]
    c = synth_case(g, name)
    zt = c["z_type"]
    args = make_args(z_type=zt, model="multimodal_context", motion_resampling_framerate=15, mean_dir_vec=[0.0] * 27)
    z_obj = pkg.Vocab.speakers(S) if zt == "speaker" else (1 if zt == "random" else None)
    G = pkg.PoseGenerator(args, 27, V, 300, None, z_obj).to(dev)
    G.load_state_dict(O.clone_state(O.make_generator_state(int(g["g_seed"]), V, S, z_mode=zt if zt != "none" else None)), strict=True)
    G.eval()
    n = c["win_text"].shape[0]
    draws = None if zt == "none" else [torch.from_numpy(c["draws"][i:i + 1]) for i in range(n)]
    import random
    random.seed(4321 + dict(zip([str(k) for k in g["cases"]], (1, 1, 2, 2, 3, 3, 4, 5, 6)))[name])      # the seed of the fixture run, as in test_engine_gpu.py
    out = syn.generate_gestures(args, G, fixture_lang(pkg.Vocab, V), c["audio"], c["words"], vid=c["vid_arg"], seed_seq=c["seed_seq"],
                                fade_out=c["fade_out"], _draws=draws)
    assert out.shape == c["out"].shape and rel(out, c["out"]) < 1e-5, rel(out, c["out"])
