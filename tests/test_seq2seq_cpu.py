"""CPU-side checks of the Seq2Seq baseline (csrc/attn.hip, the loss / clip entries of csrc/losses.hip, seq2seq.py): the C ABI, the envelope, the
state-dict contract, the host-side validation, and the fp64 chain the GPU tests lean on against the real reference (fixture g19).  No GPU
needed."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seq2seq_ref as R
from conftest import GOLDEN

NEW = {"tg_attn_step_supported": 4, "tg_attn_step_forward": 11, "tg_attn_step_backward": 15, "tg_seq2seq_loss": 12, "tg_sumsq_accumulate": 5,
       "tg_clip_scale": 4, "tg_scale_by": 4}
CASES = {"h8_clip": 8, "h12_noclip": 12}


def fixture_case(name):
    z = np.load(os.path.join(GOLDEN, "g19_seq2seq.npz"))
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


def sub(c, prefix):
    return {k[len(prefix):]: v for k, v in c.items() if k.startswith(prefix)}


def make_args(H, w=(1.0, 0.1, 0.1), dropout=0.0, noise=0):
    return SimpleNamespace(hidden_size=H, n_layers=2, dropout_prob=dropout, n_pre_poses=2, GAN_noise_size=noise, loss_regression_weight=w[0],
                           loss_kld_weight=w[1], loss_reg_weight=w[2])


def test_new_symbols_are_declared_exported_and_bound_with_matching_argument_counts(pkg):
    lib = pkg._lib.load()
    for name, n_args in NEW.items():
        assert n_args == len(pkg._lib.SIGNATURES[name]), name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert pkg._lib.ABI_VERSION == 11
    for fn in ("attn_step_supported", "attn_step_forward", "attn_step_backward", "seq2seq_loss", "grad_sumsq", "clip_scale"):
        assert callable(getattr(pkg.ops, fn))
    assert isinstance(pkg.ops.ATTN_ENVELOPE, str)
    for cls in ("Attn", "BahdanauAttnDecoderRNN", "Generator", "Seq2SeqNet", "train_iter_seq2seq"):
        assert getattr(pkg, cls) is getattr(pkg.seq2seq, cls)
    assert callable(pkg.seq2seq.build_model)


@pytest.mark.parametrize("shape, want", [((1, 1, 8), True), ((3, 128, 320), True), ((33, 34, 200), True), ((3, 7, 4), False), ((3, 7, 324), False),
                                         ((3, 7, 10), False), ((3, 0, 200), False), ((3, 129, 200), False), ((0, 7, 200), False)])
def test_attn_step_supported_answers_the_envelope_edges(pkg, shape, want):
    assert pkg.ops.attn_step_supported(*shape) is want


def test_entries_outside_the_envelope_fail_loudly_and_launch_nothing(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, Te, H in ((1, 1, 4), (1, 1, 324), (1, 1, 10), (1, 0, 8), (1, 129, 8), (0, 1, 8)):
        rc = lib.tg_attn_step_forward(p, p, p, p, p, p, H, B, Te, H, None)
        assert rc != 0 and b"tg_attn_step_forward" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()
        rc = lib.tg_attn_step_backward(p, H, p, p, p, p, p, p, p, p, p, B, Te, H, None)
        assert rc != 0 and b"tg_attn_step_backward" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_dict_keys_and_shapes_equal_the_reference_and_load_strictly_both_ways(pkg, name):
    c, H = fixture_case(name), CASES[name]
    state = {k: torch.as_tensor(v) for k, v in sub(c, "state/").items()}
    net = pkg.Seq2SeqNet(make_args(H), 27, 6, 30, 10, None)
    ours = net.state_dict()
    assert set(ours) == set(state)
    for k, v in ours.items():
        assert tuple(v.shape) == tuple(state[k].shape) and v.dtype == state[k].dtype, k
    net.load_state_dict(state, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), k
    # ... and into torch's own layers under the reference's names (what the reference's Seq2SeqNet is made of)
    assert set(k for k, _ in net.named_buffers()) == {"decoder.decoder.pre_linear.1.running_mean", "decoder.decoder.pre_linear.1.running_var",
                                                      "decoder.decoder.pre_linear.1.num_batches_tracked"}
    gru = torch.nn.GRU(H, H, 2, dropout=0.0)
    gru.load_state_dict({k[len("decoder.decoder.gru."):]: v for k, v in ours.items() if k.startswith("decoder.decoder.gru.")}, strict=True)
    enc_gru = torch.nn.GRU(10, H, 2, bidirectional=True)
    enc_gru.load_state_dict({k[len("encoder.gru."):]: v for k, v in ours.items() if k.startswith("encoder.gru.")}, strict=True)
    assert tuple(ours["decoder.decoder.attn.attn.weight"].shape) == (H, 2 * H) and tuple(ours["decoder.decoder.attn.v"].shape) == (H,)
    assert tuple(ours["decoder.decoder.pre_linear.0.weight"].shape) == (H, 27 + H)


def test_attention_parameters_are_initialised_as_the_reference_does(pkg):
    torch.manual_seed(5)
    a = pkg.Attn(200)
    assert abs(float(a.v.std()) - 1 / np.sqrt(200)) < 0.02 and abs(float(a.v.mean())) < 0.02          # normal(0, 1 / sqrt(H))
    assert float(a.attn.weight.abs().max()) <= 1 / np.sqrt(400) + 1e-7                                 # nn.Linear(2H, H)'s default


def test_speaker_model_and_noise_widen_pre_linear(pkg):
    spk = SimpleNamespace(n_words=7)
    net = pkg.Seq2SeqNet(make_args(8, noise=3), 27, 6, 30, 10, None, speaker_model=spk)
    sd = net.state_dict()
    assert tuple(sd["decoder.decoder.speaker_embedding.weight"].shape) == (7, 8)
    assert tuple(sd["decoder.decoder.pre_linear.0.weight"].shape) == (8, 27 + 3 + 8 + 8)


def test_discrete_representation_raises(pkg):
    with pytest.raises(NotImplementedError):
        pkg.BahdanauAttnDecoderRNN(27, 8, 27, 2, discrete_representation=True)
    with pytest.raises(NotImplementedError):
        pkg.Generator(make_args(8), 27, discrete_representation=True)


def test_cpu_input_raises_type_error(pkg):
    net = pkg.Seq2SeqNet(make_args(8), 27, 6, 30, 10, None)
    with pytest.raises(TypeError):
        net(torch.ones(2, 3, dtype=torch.int64), [3, 2], torch.zeros(2, 6, 27), None)
    with pytest.raises(TypeError):
        pkg.ops.attn_step_forward(torch.zeros(2, 8), torch.zeros(2, 3, 8), torch.zeros(2, 3, 8), torch.zeros(8), torch.zeros(2, 3), torch.zeros(2, 8))
    with pytest.raises(TypeError):
        pkg.ops.seq2seq_loss(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), (1, 1, 1), torch.zeros(4), torch.zeros(2, 3, 4))


def test_word_seq_collate_fn_sorts_pads_and_returns_the_reference_arity(pkg):
    mk = lambda n, tag: (torch.arange(1, n + 1), torch.full((4,), n), torch.full((6, 27), float(n)), torch.full((6, 27), float(n)),
                         torch.full((10,), float(n)), torch.full((3, 2), float(n)), {"vid": tag})
    batch = [mk(2, "a"), mk(5, "b"), mk(3, "c")]
    out = pkg.data.word_seq_collate_fn(batch)
    assert len(out) == 8                                   # lmdb_data_loader.py:41
    word_seq, words_lengths, text_padded, poses_seq, vec_seq, audio, spectrogram, aux = out
    assert words_lengths.tolist() == [5, 3, 2] and words_lengths.dtype == torch.int64
    assert word_seq.dtype == torch.int64 and tuple(word_seq.shape) == (3, 5)
    assert word_seq[1].tolist() == [1, 2, 3, 0, 0] and word_seq[2].tolist() == [1, 2, 0, 0, 0]
    for t in (text_padded, poses_seq, vec_seq, audio, spectrogram):
        assert t.reshape(3, -1)[:, 0].tolist() == [5, 3, 2]
    assert aux["vid"] == ["b", "c", "a"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_chain_reproduces_the_reference_fixture(name):
    c = fixture_case(name)
    w = tuple(float(x) for x in c["loss_weights"])
    text, poses, lens = torch.as_tensor(c["text1"]), torch.as_tensor(c["poses1"]), c["lengths"].tolist()
    ref = R.RefSeq2Seq(sub(c, "state/"), 2, 6, 2)
    out = ref(text, lens, poses, training=True)
    assert float((out.detach() - torch.as_tensor(c["train_outputs"])).abs().max()) <= 1e-12 * max(1.0, float(np.abs(c["train_outputs"]).max()))
    loss, _ = R.custom_loss(out, poses, *w)
    assert abs(float(loss) - float(c["loss"])) <= 1e-12 * max(1.0, abs(float(c["loss"])))
    loss.backward()
    grads = ref.grads()
    want = sub(c, "grad/")
    assert set(grads) == set(want)
    for k, g in grads.items():
        assert float((g - torch.as_tensor(want[k])).abs().max()) <= 1e-12 * max(1.0, float(np.abs(want[k]).max())), k
    _, coef = R.clip_coef(list(grads.values()))
    for k, g in grads.items():
        wantc = c["step1/grad_clipped/" + k]
        assert float((g * coef - torch.as_tensor(wantc)).abs().max()) <= 1e-12 * max(1.0, float(np.abs(wantc).max())), k
    assert (float(coef) < 1.0) == (name == "h8_clip")
    d = "decoder.decoder.pre_linear.1."
    assert float((ref.running_mean - torch.as_tensor(c["buffers_after/" + d + "running_mean"])).abs().max()) <= 1e-12
    rv = c["buffers_after/" + d + "running_var"]
    assert float((ref.running_var - torch.as_tensor(rv)).abs().max()) <= 1e-12 * max(1.0, float(np.abs(rv).max()))
    assert ref.nbt == int(c["buffers_after/" + d + "num_batches_tracked"]) == 5
    for key, sl in (("eval_outputs", slice(None)), ("eval_outputs_b1", slice(0, 1))):
        ev = R.RefSeq2Seq(sub(c, "state/"), 2, 6, 2)
        with torch.no_grad():
            o = ev(text[sl], lens[sl], poses[sl], training=False)
        assert float((o - torch.as_tensor(c[key])).abs().max()) <= 1e-12 * max(1.0, float(np.abs(c[key]).max())), key
