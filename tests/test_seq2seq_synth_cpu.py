"""CPU-side checks of Seq2Seq synthesis: the window-text builder and the host smoothing of synthesize.py against the real reference (fixture
g20), the fp64 chain with the window loop (tests/seq2seq_synth_ref.py) against the reference's fp32 outputs, per-row-length attention against
B = 1 runs, checkpoint.init_model routing, and the C ABI of csrc/seq2seq_decode.hip.  No GPU needed."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seq2seq_ref as R
import seq2seq_synth_ref as SR
from conftest import GOLDEN

N_POSES, N_PRE, FPS = 34, 4, 15
NEW = {"tg_seq2seq_decode_supported": 11, "tg_seq2seq_decode_eval": 34}


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "g20_seq2seq_synth.npz"))
    return {k: z[k] for k in z.files}


def sub(c, prefix):
    return {k[len(prefix):]: v for k, v in c.items() if k.startswith(prefix)}


def lang_of(pkg, fx):
    lang = pkg.Vocab("words")
    for w in fx["vocab_words"].tolist():
        lang.index_word(w)
    return lang


def words_of(fx, name):
    return [[w, float(t[0]), float(t[1])] for w, t in zip(fx[name + "/words"].tolist(), fx[name + "/word_times"])]


def args_of(fx):
    return SimpleNamespace(model="seq2seq", hidden_size=12, n_layers=2, dropout_prob=0.0, n_pre_poses=N_PRE, n_poses=N_POSES, GAN_noise_size=0,
                           z_type="none", motion_resampling_framerate=FPS, wordembed_dim=10, mean_dir_vec=fx["mean_dir_vec"].tolist())


def test_fixture_covers_the_cases_the_feature_needs(fx):
    names = fx["cases"].tolist()
    assert sorted({len(fx[n + "/win_text_len"]) for n in names}) == [1, 2, 4]
    assert {bool(fx[n + "/fade_out"]) for n in names} == {False, True} and {len(fx[n + "/seed_seq"]) > 0 for n in names} == {False, True}
    assert any(2 in fx[n + "/win_text_len"].tolist() for n in names)                       # a window without a word: [SOS, EOS]


def test_window_text_builder_reproduces_every_recorded_in_text(pkg, fx):
    lang = lang_of(pkg, fx)
    for name in fx["cases"].tolist():
        words, lens = words_of(fx, name), fx[name + "/win_text_len"].tolist()
        flat, o = fx[name + "/win_text"], 0
        assert pkg.synthesize.num_windows(int(fx[name + "/audio_len"]) / 16000, N_POSES, N_PRE, FPS) == len(lens)
        for i, n in enumerate(lens):
            got = pkg.synthesize.seq2seq_window_text(lang, words, i, N_POSES, N_PRE, FPS)
            assert got.dtype == np.int64 and np.array_equal(got, flat[o:o + n]), (name, i)
            assert got[0] == lang.SOS_token and got[-1] == lang.EOS_token
            o += n


def test_smoothing_and_fade_out_reproduce_final_from_stacked(pkg, fx):
    """The stored arrays are fp32 and the reference assigns its fp64 fits back into them, so the functions run on fp32 here as well.  Gate: the
    fits are fp64 least squares over at most 12 points (condition about 1e5 for a cubic on x = 0 .. 11): noise of at most 1e5 x 2^-53 = 1e-11
    of the values, which can move a result across an fp32 rounding boundary -- one fp32 ulp, 2^-23 of the tensor's largest magnitude."""
    args, worst = args_of(fx), 0.0
    for name in fx["cases"].tolist():
        stacked, final = fx[name + "/stacked"], fx[name + "/final"]
        assert stacked.dtype == np.float32 and final.dtype == np.float32
        out = pkg.synthesize.seq2seq_smooth(stacked.copy(), len(fx[name + "/win_text_len"]), N_POSES, N_PRE)
        if bool(fx[name + "/fade_out"]):
            out = pkg.synthesize.fade_out_to_mean(out, pkg.synthesize.end_padding_samples(args, int(fx[name + "/audio_len"])), args)
        assert out.shape == final.shape and not np.array_equal(out[:len(stacked)], stacked)
        err = float(np.abs(out.astype(np.float64) - final).max() / np.abs(final).max())
        worst = max(worst, err)
        print(f"{name}: smoothing + fade-out differ from the reference by {err:.3e} of the largest magnitude")
        assert err <= 2.0 ** -23, (name, err)
    report = json.load(open(os.path.join(GOLDEN, "golden_report_seq2seq_synth.json")))
    recorded = max(c["smooth_and_fade_rel_err"] for c in report["cases"].values())
    assert recorded <= 2.0 ** -23 and worst <= 2.0 ** -23


def test_window_loop_of_the_chain_reproduces_the_reference_within_four_fp32_errors(pkg, fx):
    """The reference ran in fp32: the fp64 chain must sit within 4 x the error of the same chain in fp32 (floored at 1e-6 of the largest
    magnitude), window by window: in_text, pre_seq_partial, raw output, and the stacked output."""
    lang, state = lang_of(pkg, fx), sub(fx, "state/")
    for name in fx["cases"].tolist():
        seed = fx[name + "/seed_seq"]
        res = {}
        for dt in (torch.float64, torch.float32):
            res[dt] = SR.generate_gestures(R.RefSeq2Seq(state, 2, N_POSES, N_PRE, dt), int(fx[name + "/audio_len"]), words_of(fx, name),
                                           lang.get_word_index, seed_seq=seed if len(seed) else None)
        (s64, w64), (s32, w32) = res[torch.float64], res[torch.float32]
        lens, o = fx[name + "/win_text_len"].tolist(), 0
        assert len(w64) == len(lens)
        for i, n in enumerate(lens):
            assert w64[i][0] == fx[name + "/win_text"][o:o + n].tolist()
            o += n
            for j, key in ((1, "win_pre"), (2, "win_raw")):
                gate = max(4.0 * float(np.abs(w32[i][j] - w64[i][j]).max()), 1e-6 * float(np.abs(w64[i][j]).max()))
                err = float(np.abs(w64[i][j] - fx[name + "/" + key][i]).max())
                assert err <= gate, (name, i, key, err, gate)
        gate = max(4.0 * float(np.abs(s32 - s64).max()), 1e-6 * float(np.abs(s64).max()))
        err = float(np.abs(s64 - fx[name + "/stacked"]).max())
        print(f"{name}: stacked output of the fp64 chain against the reference {err:.3e}, gate {gate:.3e}")
        assert s64.shape == fx[name + "/stacked"].shape and err <= gate


def test_chain_eval_outputs_match_the_reference_batched_forward(fx):
    state = sub(fx, "state/")
    text, lens, poses = torch.as_tensor(fx["eval/text0"]), fx["eval/lengths0"].tolist(), torch.as_tensor(fx["eval/target0"])
    r64 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE), text, lens, poses, per_row=False)
    r32 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE, torch.float32), text, lens, poses, per_row=False)
    gate = max(4.0 * float((r32.double() - r64).abs().max()), 1e-6 * float(r64.abs().max()))
    assert float((r64 - torch.as_tensor(fx["ckpt/eval_outputs"]).double()).abs().max()) <= gate
    # ... and the masked step with te_len = None is seq2seq_ref's own step
    ref = R.RefSeq2Seq(state, 2, N_POSES, N_PRE)
    with torch.no_grad():
        assert torch.equal(ref(text, lens, poses.double(), training=False), r64)


def test_per_row_length_attention_of_a_padded_batch_equals_the_single_row_runs(fx):
    state = sub(fx, "state/")
    ref = R.RefSeq2Seq(state, 2, N_POSES, N_PRE)
    for i in range(2):
        text, lens, poses = torch.as_tensor(fx[f"eval/text{i}"]), fx[f"eval/lengths{i}"].tolist(), torch.as_tensor(fx[f"eval/target{i}"])
        batch = SR.forward(ref, text, lens, poses, per_row=True)
        padded = SR.forward(ref, text, lens, poses, per_row=False)
        for b, n in enumerate(lens):
            one = SR.forward(ref, text[b:b + 1, :n], [n], poses[b:b + 1])
            assert float((one[0] - batch[b]).abs().max()) <= 1e-12                          # exact up to summation order
            if n < max(lens):
                assert float((padded[b] - batch[b]).abs().max()) > 1e-6                     # padded positions carry weight without the lengths


def test_init_model_routes_seq2seq_and_still_refuses_joint_embedding(pkg, fx):
    args, lang = args_of(fx), lang_of(pkg, fx)
    lang.word_embedding_weights = None
    gen, dis, loss_fn = pkg.checkpoint.init_model(args, lang, None, 27, "cpu")
    assert isinstance(gen, pkg.Seq2SeqNet) and dis is None and isinstance(loss_fn, torch.nn.L1Loss)
    gen.load_state_dict({k: torch.as_tensor(v) for k, v in sub(fx, "state/").items()}, strict=True)
    with pytest.raises(NotImplementedError):                                              # no vocabulary to size the text encoder from
        pkg.checkpoint.init_model(args, None, None, 27, "cpu")
    args.model = "joint_embedding"
    with pytest.raises(NotImplementedError):
        pkg.checkpoint.init_model(args, lang, None, 27, "cpu")
    _a, g2, lf, lm, spk, pd = pkg.checkpoint.load_checkpoint_and_model(os.path.join(GOLDEN, "g20_seq2seq_checkpoint.bin"), "cpu")
    assert isinstance(g2, pkg.Seq2SeqNet) and not g2.training and pd == 27 and spk is None and lm.n_words == lang.n_words
    for k, v in g2.state_dict().items():
        assert torch.equal(v, torch.as_tensor(fx["state/" + k])), k


def test_new_entries_are_declared_bound_and_check_their_arguments(pkg):
    lib = pkg._lib.load()
    for name, n_args in NEW.items():
        assert n_args == len(pkg._lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
    assert isinstance(pkg.ops.SEQ2SEQ_DECODE_ENVELOPE, str) and pkg.seq2seq.FUSED_EVAL_DECODE is True
    ok = dict(B=3, Te=34, H=200, nl=2, nf=34, n_pre=4, Pd=27, Po=27, Z=0, S8=0)
    sup = lambda **kw: pkg.ops.seq2seq_decode_supported(*{**ok, **kw}.values())
    assert sup() and sup(B=1, Te=1, H=8, nl=1, nf=2, n_pre=0) and sup(Te=128, H=320, nl=4) and sup(nf=2, n_pre=1, Pd=30, Po=27) and sup(Z=4, S8=8)
    for bad in (dict(H=6), dict(H=10), dict(H=324), dict(Te=129), dict(Te=0), dict(nl=5), dict(nl=0), dict(nf=1), dict(n_pre=35), dict(Pd=30),
                dict(B=0), dict(Pd=900, Po=900)):
        assert not sup(**bad), bad
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    table = (ctypes.c_void_p * 16)(*([p.value] * 16))
    call = lambda B, Te, H, nl, tab=table, enc=p: lib.tg_seq2seq_decode_eval(enc, p, None, p, p, 4, None, None, p, p, p, p, p, p, p, p, 1e-5, tab, p,
                                                                               p, p, p, None, B, Te, H, nl, 34, 4, 27, 27, 0, 0, None)
    for B, Te, H, nl in ((1, 1, 6, 1), (1, 129, 8, 1), (1, 1, 8, 5), (0, 1, 8, 1), (1, 1, 324, 1)):
        assert call(B, Te, H, nl) != 0 and b"tg_seq2seq_decode_eval" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()
    assert call(1, 1, 8, 1, enc=None) != 0 and b"null" in lib.tg_last_error()
    assert call(1, 1, 8, 2, tab=(ctypes.c_void_p * 8)()) != 0 and b"GRU parameter" in lib.tg_last_error()
    with pytest.raises(TypeError):
        z = torch.zeros
        pkg.ops.seq2seq_decode_eval(z(1, 1, 8), z(1, 1, 8), z(1, 1, 8), z(1, 1, 27), 2, 1, z(8, 16), z(8), z(8, 35), z(8), z(8), z(8), z(8), z(8), 1e-5,
                                    [(z(24, 8), z(24, 8), z(24), z(24))], z(27, 8), z(27), z(1, 2, 27), z(1, 1, 8))
    with pytest.raises(ValueError):
        pkg.ops.seq2seq_decode_lengths([1, 5], 2, 4, "cpu")
    with pytest.raises(ValueError):
        pkg.ops.seq2seq_decode_lengths([1], 2, 4, "cpu")
