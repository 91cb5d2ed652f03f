"""The constant-input few-row recurrence and the joint-embedding window decoder without a GPU: the header declares the two new entries and the
built library exports them with host-side argument checks, and the Python layers above them (rnn.GRU.forward_constant,
PoseDecoderGRU.forward_constant, synthesize.JointEmbedWindowDecoder, the window_decoder keyword) validate on the host and raise before any
GPU call."""
import inspect
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT


def test_header_and_library_declare_the_constant_input_entries(pkg):
    header = open(os.path.join(ROOT, "include", "trimodal_hip.h")).read()
    for name, nargs in (("tg_gru_vec_const_supported", 4), ("tg_gru_forward_vec_const", 14)):
        assert len(pkg._lib.SIGNATURES[name]) == nargs
    assert "MAY SHARE" in header and "ONE DIRECTION COUNT" in header            # the workspace rule and its extension are documented
    assert pkg._lib.ABI_VERSION == 11
    lib = pkg._lib.load()                                        # a library built before the change fails here on the missing symbol
    assert lib.tg_gru_forward_vec_const(None, 0, None, None, None, None, None, None, 0, 1, 1, 256, 2, None) != 0
    assert b"tg_gru_forward_vec_const" in lib.tg_last_error()
    assert lib.tg_gru_vec_const_supported(1, 256, 2, None) != 0 and b"tg_gru_vec_const_supported" in lib.tg_last_error()
    # outside the envelope (here also: no device) the query answers 0 with a zero status, n_dir = 3 included
    import ctypes as C
    for B, H, nd in ((5, 256, 2), (1, 64, 2), (1, 324, 1), (1, 70, 2), (1, 256, 3)):
        out = C.c_int32(7)
        assert lib.tg_gru_vec_const_supported(B, H, nd, C.cast(C.byref(out), C.c_void_p)) == 0 and out.value == 0, (B, H, nd)
    # the envelope is checked before anything is launched: valid host pointers, a shape outside it
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.tg_gru_forward_vec_const(p, 0, p, p, p, p, p, p, 1 << 20, 1, 3, 256, 3, None) != 0
    assert b"envelope" in lib.tg_last_error()


def _args(**over):
    a = dict(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34,
             motion_resampling_framerate=15)
    a.update(over)
    return SimpleNamespace(**a)


def test_forward_constant_validates_on_the_host(pkg):
    g = pkg.rnn.GRU(64, 300, 4, batch_first=True, bidirectional=True)
    assert g.training
    with pytest.raises(ValueError, match="eval"):
        g.forward_constant(torch.zeros(1, 64), 34)
    g.eval()
    with pytest.raises(ValueError, match="initial"):
        g.forward_constant(torch.zeros(1, 64), 34, hx=torch.zeros(8, 1, 300))
    with pytest.raises(ValueError, match="B"):
        g.forward_constant(torch.zeros(5, 64), 34)
    with pytest.raises(ValueError, match="x_row"):
        g.forward_constant(torch.zeros(1, 34, 64), 34)           # a repeated input is GRU.forward's business
    with pytest.raises(TypeError, match="CUDA"):
        g.forward_constant(torch.zeros(1, 64), 34)               # no torch fallback
    net = pkg.EmbeddingNet(_args(), 27, 34, 12, 300, None, mode="random")
    with pytest.raises(ValueError, match="eval"):
        net.decoder.forward_constant(torch.zeros(1, 32), torch.zeros(1, 4, 27))
    with pytest.raises(RuntimeError, match="eval"):              # synthesize keeps its own refusal, with or without the keyword
        net.synthesize(torch.zeros(1, 34, dtype=torch.int64), torch.zeros(1, 36266), torch.zeros(1, 4, 27), constant_input=True)
    assert inspect.signature(net.synthesize).parameters["constant_input"].default is False


def test_window_decoder_and_keyword_validate_before_any_gpu_call(pkg):
    S = pkg.synthesize
    net = pkg.EmbeddingNet(_args(), 27, 34, 12, 300, None, mode="random")
    dev = torch.device("cuda:0")                                 # never touched: every refusal below comes first
    with pytest.raises(ValueError, match="eval"):
        S.JointEmbedWindowDecoder(_args(), net, 1, dev)          # a train-mode model
    net.eval()
    with pytest.raises(ValueError, match="n_pre_poses"):
        S.JointEmbedWindowDecoder(_args(n_pre_poses=5), net, 1, dev)
    with pytest.raises(ValueError, match="n_pre_poses"):
        S.JointEmbedWindowDecoder(_args(n_poses=30), net, 1, dev)
    with pytest.raises(ValueError, match="joint_embedding"):
        S.JointEmbedWindowDecoder(_args(model="multimodal_context"), net, 1, dev)
    with pytest.raises(ValueError, match="1 to 4"):
        S.JointEmbedWindowDecoder(_args(), net, 5, dev)
    with pytest.raises(ValueError, match="EmbeddingNet"):
        S.JointEmbedWindowDecoder(_args(), pkg.EmbeddingNet(_args(), 27, 34).eval(), 1, dev)       # mode='pose' has no context encoder
    assert net.context_encoder.gru.few_row_eval is False         # a refused construction changes nothing
    audio = [0.0] * 40000
    for model in ("seq2seq", "speech2gesture", "multimodal_context"):
        with pytest.raises(ValueError, match="joint_embedding"):
            S.generate_gestures_batch(_args(model=model), net, None, [audio], [[]], window_decoder=True)
        with pytest.raises(ValueError, match="joint_embedding"):
            S.generate_gestures(_args(model=model), net, None, audio, [], window_decoder=True)
    with pytest.raises(ValueError, match="at most 4"):
        S.generate_gestures_batch(_args(), net, None, [audio] * 5, [[]] * 5, window_decoder=True)
    for f in (S.generate_gestures, S.generate_gestures_batch):
        assert inspect.signature(f).parameters["window_decoder"].default is False
    sig = inspect.signature(S.JointEmbedWindowDecoder.__init__).parameters
    assert list(sig)[:7] == ["self", "args", "net", "batch", "device", "graph", "replay_draws"]
