"""CPU-side checks of the joint-embedding baseline (csrc/latent_head.hip, joint_embed.py, EmbeddingNet(mode='random')): the C ABI and its
envelope, the state-dict contract against the reference's key list (fixture g21), the checkpoint entry points, and the refusals that
stay.  No GPU needed."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import joint_embed_ref as R
from conftest import GOLDEN

NEW = {"tg_latent_head_supported": 6, "tg_latent_head_fwd": 35, "tg_latent_head_bwd": 37}
ARGS = dict(hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False, n_pre_poses=4, n_poses=34, wordembed_dim=300,
            model="joint_embedding")
V = 32


def make_net(pkg, mode="random"):
    return pkg.EmbeddingNet(SimpleNamespace(**ARGS), 27, 34, V, 300, None, mode=mode)


def test_new_symbols_are_declared_exported_and_bound_with_matching_argument_counts(pkg):
    lib = pkg._lib.load()
    for name, n_args in NEW.items():
        assert n_args == len(pkg._lib.SIGNATURES[name]), name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert isinstance(pkg.ops.LATENT_HEAD_ENVELOPE, str)
    for name in ("ContextEncoder", "PoseDecoderGRU", "JointEmbedTrainer", "train_iter_embed"):
        assert getattr(pkg, name) is getattr(pkg.joint_embed, name)
    assert callable(pkg.joint_embed.build_model) and callable(pkg.joint_embed.load_checkpoint_and_model)


@pytest.mark.parametrize("shape, want", [((1, 256, 128, 32, 0), True), ((1, 256, 128, 32, 1), False), ((2, 108, 32, 32, 1), True),
                                         ((512, 384, 256, 64, 1), True), ((513, 384, 256, 64, 0), False), ((4, 385, 256, 64, 0), False),
                                         ((4, 384, 257, 64, 0), False), ((4, 384, 256, 65, 0), False), ((0, 8, 8, 8, 0), False),
                                         ((4, 0, 8, 8, 0), False)])
def test_latent_head_supported_answers_the_envelope_edges(pkg, shape, want):
    assert pkg.ops.latent_head_supported(*shape) is want


def test_entries_outside_the_envelope_fail_loudly_and_launch_nothing(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for B, K0, N1, N2, tr in ((1, 8, 8, 8, 1), (513, 8, 8, 8, 0), (2, 385, 8, 8, 1), (2, 8, 257, 8, 1), (2, 8, 8, 65, 1), (0, 8, 8, 8, 0)):
        rc = lib.tg_latent_head_fwd(p, K0, *[p] * 15, 0, p, N2, *[p] * 6, B, K0, N1, N2, tr, 0.0, 1e-5, 0.1, None)
        assert rc != 0 and b"tg_latent_head_fwd" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()
        rc = lib.tg_latent_head_bwd(p, N2, p, p, p, K0, *[p] * 23, K0, B, K0, N1, N2, tr, 0.0, None)
        assert rc != 0 and b"tg_latent_head_bwd" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()


def test_state_dict_keys_shapes_and_dtypes_equal_the_reference(pkg):
    net = make_net(pkg)
    ours = net.state_dict()
    ref = json.load(open(os.path.join(GOLDEN, "golden_report_joint_embed.json")))["state_keys"]      # written from the real reference
    assert set(ours) == set(ref)
    for k, v in ours.items():
        assert list(v.shape) == ref[k]["shape"] and str(v.dtype) == ref[k]["dtype"], k
    st = R.make_state(3, V)
    assert set(st) == set(ref)
    net.load_state_dict(st, strict=True)
    sd = net.state_dict()
    pre = "context_encoder.text_encoder.tcn.network.0."
    assert sd[pre + "conv1.weight_v"].data_ptr() == sd[pre + "net.0.weight_v"].data_ptr()
    assert sd["decoder.pre_pose_net.1.num_batches_tracked"].dtype == torch.int64


def test_saved_checkpoint_loads_strictly_through_the_joint_embed_entry_point(pkg, tmp_path):
    """(No reference-written checkpoint file is committed: with the decoder GRU's configured 5.6 M parameters it cannot stay below the
    size limit of a committed file.  The reference's own modules load this key set strictly: the fixture maker does exactly that.)"""
    from harness import fixture_lang
    lang = fixture_lang(pkg.Vocab, V)
    args = SimpleNamespace(**ARGS)
    gen = pkg.joint_embed.build_model(args, lang, 27, "cpu")[0]
    gen.load_state_dict(R.make_state(5, lang.n_words), strict=True)
    out = str(tmp_path / "ours.bin")
    pkg.checkpoint.save_checkpoint({"args": args, "epoch": 1, "lang_model": lang, "speaker_model": None, "pose_dim": 27,
                                    "gen_dict": gen.state_dict()}, out)
    ref = json.load(open(os.path.join(GOLDEN, "golden_report_joint_embed.json")))["state_keys"]
    assert set(pkg.checkpoint.load_checkpoint(out)["gen_dict"]) == set(ref)
    args2, again, loss_fn, lang2, spk, pose_dim = pkg.joint_embed.load_checkpoint_and_model(out, "cpu")
    assert args2.model == "joint_embedding" and pose_dim == 27 and loss_fn is None and spk is None and not again.training and again.mode == "random"
    for k, v in gen.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    with pytest.raises(NotImplementedError):
        pkg.checkpoint.load_checkpoint_and_model(out, "cpu")


def test_init_model_still_refuses_joint_embedding_and_pose_mode_is_the_old_network(pkg):
    lang = SimpleNamespace(n_words=V, word_embedding_weights=None)
    with pytest.raises(NotImplementedError):
        pkg.checkpoint.init_model(SimpleNamespace(**ARGS), lang, None, 27, "cpu")
    ae = make_net(pkg, "pose")
    assert ae.context_encoder is None and len(ae.state_dict()) == 70 and sum(p.numel() for p in ae.parameters()) == 190_691
    assert type(ae.decoder).__name__ == "_PoseDecoderParams"
    with pytest.raises(NotImplementedError):
        pkg.EmbeddingNet(SimpleNamespace(**ARGS), 27, 64, V, 300, None, mode="random")
    gen, dis, loss_fn = pkg.joint_embed.build_model(SimpleNamespace(**ARGS), lang, 27, "cpu")
    assert dis is None and loss_fn is None and gen.mode == "random"


def test_host_side_validation_raises_without_a_gpu(pkg):
    net = make_net(pkg)
    with pytest.raises(TypeError):
        net(torch.zeros(2, 34, dtype=torch.int64), torch.zeros(2, 36267), torch.zeros(2, 4, 27), torch.zeros(2, 34, 27), "speech")
    with pytest.raises(NotImplementedError):
        net(None, None, torch.zeros(2, 4, 27), torch.zeros(2, 34, 27), "pose", variational_encoding=True)


def test_the_chain_reproduces_the_reference_fixture():
    """tests/joint_embed_ref.py against the real reference (fixture g21, written by tests/golden/make_golden_joint_embed.py): forwards,
    losses, sampled gradients and the BatchNorm statistics of both encoders, to the tolerance tests/test_seq2seq_cpu.py uses (1e-12)."""
    z = np.load(os.path.join(GOLDEN, "g21_joint_embed.npz"))
    st = R.make_state(int(z["state_seed"]), V)
    for mode in ("speech", "pose"):
        ids, audio, target, _ = R.make_inputs(int(z["eval_inputs_seed"]), int(z["eval_B"]), V)
        net = R.build(st).eval()
        with torch.no_grad():
            out = net(ids, audio.double(), target[:, :4].double(), target.double(), mode, {"c.eps": torch.as_tensor(z[f"eval/{mode}/eps"])})
        for i, o in enumerate(out):
            key = f"eval/{mode}/out{i}"
            assert (o is None) == (key not in z.files)
            if o is not None:
                assert float((o - torch.as_tensor(z[key])).abs().max()) <= 1e-12 * max(1.0, float(o.abs().max())), key
        ids, audio, target, _ = R.make_inputs(int(z["train_inputs_seed"]), int(z["train_B"]), V)
        net = R.build(st).train()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        loss = R.train_iter_embed(net, opt, ids, audio.double(), target.double(), mode, {"c.eps": torch.as_tensor(z[f"train/{mode}/eps"])})
        assert abs(loss - float(z[f"train/{mode}/loss"])) <= 1e-12 * abs(loss)
        for k, p in net.named_parameters():
            nk = f"train/{mode}/grad_norm/{k}"
            if p.grad is None:
                assert nk not in z.files, k
                continue
            # R.ZERO_GRAD_BIASES: exact gradient 0, rounding noise on both sides, measured against the sibling weight gradient
            sib = f"train/{mode}/grad_norm/{k[:-4]}weight"
            scale = max(float(z[nk]), float(z[sib])) if k in R.ZERO_GRAD_BIASES else max(float(z[nk]), 1e-300)
            assert abs(float(p.grad.norm()) - float(z[nk])) <= 1e-10 * scale, k
            idx = torch.as_tensor(z[f"train/{mode}/grad_idx/{k}"])
            ref = torch.as_tensor(z[f"train/{mode}/grad_val/{k}"])
            assert float((p.grad.flatten()[idx] - ref).abs().max()) <= 1e-12 * max(float(p.grad.abs().max()), scale), k
        sd = net.state_dict()
        for k, v in sd.items():
            if "running_" in k or k.endswith("num_batches_tracked"):
                assert float((v.double() - torch.as_tensor(z[f"train/{mode}/after/{k}"]).double()).abs().max()) <= 1e-12, k
            elif v.dtype.is_floating_point:
                assert abs(float(v.norm()) - float(z[f"train/{mode}/after_norm/{k}"])) <= 1e-10 * float(v.norm()), k
