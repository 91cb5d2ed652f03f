"""Joint-embedding synthesis without a GPU: the host restatement (tests/joint_embed_synth_ref.py) and the product's host functions against the
real reference's recorded results (fixture g22, tests/golden/make_golden_joint_embed_synth.py), and the declarations of the one-direction
few-row recurrence.

Gates (DESIGN.md sections 18-19): a chain result is compared with the reference's fp32 result within 4 x the fp32 chain's own error against
fp64, floored at 1e-6 of the largest magnitude; host arithmetic on stored values within one fp32 ulp of the largest magnitude."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joint_embed_ref as JR
import joint_embed_synth_ref as SR
from conftest import GOLDEN, ROOT

N_POSES, N_PRE = 34, 4
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "g22_joint_embed_synth.npz"))
    return {k: z[k] for k in z.files}


def fixture_args(fx):
    return SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=N_PRE,
                           n_poses=N_POSES, z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=fx["mean_dir_vec"].tolist())


def fixture_lang(pkg, fx):
    lang = pkg.Vocab("words")
    for w in fx["vocab_words"].tolist():
        lang.index_word(w)
    return lang


def gate_of(ref64, ref32):
    ref64, ref32 = torch.as_tensor(ref64).double(), torch.as_tensor(ref32).double()
    return max(4.0 * float((ref32 - ref64).abs().max()), 1e-6 * float(ref64.abs().max()))


@pytest.mark.parametrize("name", ["w1", "w1_fade_seed", "w2_seed", "w2_fade", "w4", "w4_fade_seed"])
def test_fp32_chain_reproduces_the_reference_windows(pkg, fx, name):
    lang = fixture_lang(pkg, fx)
    assert lang.n_words == len(fx["vocab_words"]) + 4
    s64, w64, _ = SR.chain_run(fx, name, torch.float64, lang.get_word_index)
    s32, w32, _ = SR.chain_run(fx, name, torch.float32, lang.get_word_index)
    assert len(w32) == len(fx[name + "/win_raw"])
    for i, (a, b) in enumerate(zip(w64, w32)):
        g = gate_of(a[3], b[3])
        err = float(np.abs(b[3].astype(np.float64) - fx[name + "/win_raw"][i]).max())
        print(f"{name} window {i}: fp32 chain against the reference {err:.3e} gate {g:.3e}")
        assert err <= g
        assert np.array_equal(b[0], fx[name + "/win_text"][i])
        assert float(np.abs(b[2].astype(np.float64) - fx[name + "/win_pre"][i]).max()) <= g
    g = gate_of(s64, s32)
    assert float(np.abs(s32.astype(np.float64) - fx[name + "/stacked"]).max()) <= g


def test_window_inputs_reproduce_every_recorded_text_and_audio_slice(pkg, fx):
    lang, args = fixture_lang(pkg, fx), fixture_args(fx)
    for name in fx["cases"].tolist():
        audio = SR.make_audio(fx[name + "/audio_seed"], int(fx[name + "/audio_len"]))
        words = SR.words_of(fx, name)
        n_win = pkg.synthesize.num_windows(len(audio) / 16000, N_POSES, N_PRE, 15)
        assert n_win == len(fx[name + "/win_text"]) == SR.num_windows(len(audio))
        for i in range(n_win):
            piece, ids, pad = pkg.synthesize.window_inputs(args, lang, audio, words, i)
            assert np.array_equal(ids, fx[name + "/win_text"][i]), (name, i)
            assert len(piece) == int(fx[name + "/win_audio_len"][i]) and piece.dtype == np.float32
            samples, sums = SR.audio_digest(piece)
            assert np.array_equal(samples, fx[name + "/win_audio_samples"][i]) and np.array_equal(sums, fx[name + "/win_audio_sums"][i]), (name, i)
            piece2, ids2, pad2 = SR.window_inputs(audio, words, lang.get_word_index, i)
            assert np.array_equal(piece, piece2) and np.array_equal(ids, ids2) and pad == pad2


def test_fade_out_reproduces_final_from_stacked(pkg, fx):
    args = fixture_args(fx)
    for name in fx["cases"].tolist():
        stacked, final = fx[name + "/stacked"], fx[name + "/final"]
        if bool(fx[name + "/fade_out"]):
            out = pkg.synthesize.fade_out_to_mean(stacked.copy(), pkg.synthesize.end_padding_samples(args, int(fx[name + "/audio_len"])), args)
            assert out.shape == final.shape
            err, bound = float(np.abs(out.astype(np.float64) - final).max()), ULP * float(np.abs(final).max())
            print(f"{name}: fade-out differs from the reference by {err:.3e} (bound {bound:.3e})")
            assert err <= bound
        else:
            assert np.array_equal(stacked, final)                 # no extra smoothing for this model
        # the cross-fade: rebuilt from the raw windows by the blend of tg_window_blend's definition (synthesize.py:145-153)
        raw = fx[name + "/win_raw"]
        total = np.zeros((len(raw) * (N_POSES - N_PRE) + N_PRE, 27), np.float32)
        for i, w in enumerate(raw):
            w = w.copy()
            if i:
                for j in range(N_PRE):
                    w[j] = raw[i - 1][N_POSES - N_PRE + j] * (N_PRE - j) / (N_PRE + 1) + w[j] * (j + 1) / (N_PRE + 1)
            total[i * 30:i * 30 + N_POSES] = w
        assert float(np.abs(total.astype(np.float64) - stacked).max()) <= ULP * float(np.abs(stacked).max())


def test_evaluate_testset_loss_arithmetic_matches_the_fixture(fx):
    targets = [JR.make_inputs(int(s), 3, len(fx["vocab_words"]) + 4)[2] for s in fx["eval/input_seeds"]]
    loss = SR.eval_loss([fx["eval/recon0"], fx["eval/recon1"]], targets)
    want = float(fx["eval/loss"])
    print(f"loss {loss:.9f} reference {want:.9f}")
    assert abs(loss - want) <= 2.0 ** -22 * abs(want)


def test_header_and_bindings_declare_the_one_direction_entries(pkg):
    header = open(os.path.join(ROOT, "include", "trimodal_hip.h")).read()
    for name, nargs in (("tg_gru_vec1_supported", 3), ("tg_gru_forward_vec1", 10)):
        assert len(pkg._lib.SIGNATURES[name]) == nargs
    assert "ONE DIRECTION COUNT" in header
    assert pkg._lib.ABI_VERSION == 11
    lib = pkg._lib.load()                                        # a library built before the change fails here on the missing symbol
    assert lib.tg_gru_forward_vec1(None, None, None, None, None, 0, 1, 1, 256, None) != 0 and b"tg_gru_forward_vec1" in lib.tg_last_error()


def test_few_row_eval_is_off_by_default_and_synthesize_needs_eval_mode(pkg):
    assert pkg.rnn.GRU(8, 68, 2).few_row_eval is False
    assert pkg.rnn.GRU(64, 300, 4, bidirectional=True, batch_first=True).few_row_eval is False
    args = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34)
    net = pkg.EmbeddingNet(args, 27, 34, 12, 300, None, mode="random")
    assert not net.context_encoder.gru.few_row_eval and not net.decoder.gru.few_row_eval
    with pytest.raises(RuntimeError, match="eval"):
        net.synthesize(torch.zeros(1, 34, dtype=torch.int64), torch.zeros(1, 36266), torch.zeros(1, 4, 27))
    with pytest.raises(ValueError):
        pkg.EmbeddingNet(args, 27, 34).synthesize(None, None, None)
