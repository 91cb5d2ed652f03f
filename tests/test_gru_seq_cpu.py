"""CPU-side checks of the general GRU recurrence (csrc/gru_seq.hip): its C ABI, the fp64 references the GPU tests lean on, and the host-side
validation.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gru_seq_ref as R
from conftest import GOLDEN

NEW = {"tg_gru_seq_supported": 5, "tg_gru_seq_forward": 16, "tg_gru_seq_backward": 15}


def test_new_symbols_are_declared_exported_and_bound_with_matching_argument_counts(pkg):
    lib = pkg._lib.load()
    for name, n_args in NEW.items():
        assert n_args == len(pkg._lib.SIGNATURES[name]), name
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert pkg._lib.ABI_VERSION == 11
    for fn in ("gru_seq_supported", "gru_seq_forward", "gru_seq_backward", "gru_seq_check"):
        assert callable(getattr(pkg.ops, fn))
    assert callable(pkg.layers.gru_seq_stack_fwd) and callable(pkg.layers.gru_seq_stack_bwd)
    assert pkg.GRU is pkg.rnn.GRU and pkg.EncoderRNN is pkg.rnn.EncoderRNN


@pytest.mark.parametrize("shape, want", [((1, 1, 4, 1), False), ((1, 1, 8, 1), True), ((3, 7, 320, 2), True), ((3, 7, 324, 2), False),
                                         ((3, 7, 10, 1), False), ((3, 7, 202, 2), False), ((3, 7, 200, 3), False), ((3, 7, 200, 2), True),
                                         ((0, 7, 200, 1), False), ((3, 0, 200, 1), False)])
def test_supported_answers_the_envelope_edges(pkg, shape, want):
    assert pkg.ops.gru_seq_supported(*shape) is want


def test_entries_outside_the_envelope_fail_loudly_and_launch_nothing(pkg):
    lib = pkg._lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for H, D in ((4, 1), (324, 1), (10, 1), (16, 3)):
        rc = lib.tg_gru_seq_forward(p, p, p, p, p, None, None, p, p, None, None, 1, 1, H, D, None)
        assert rc != 0 and b"tg_gru_seq_forward" in lib.tg_last_error() and b"envelope" in lib.tg_last_error()
        rc = lib.tg_gru_seq_backward(p, None, p, p, p, None, p, p, None, p, 1, 1, H, D, None)
        assert rc != 0 and b"tg_gru_seq_backward" in lib.tg_last_error()


def test_host_lengths_are_validated(pkg):
    ops = pkg.ops
    cpu = torch.device("cpu")
    for bad in ([3, 0, 2], [3, 5, 2], [3, -1, 2], [3, 2]):
        with pytest.raises(ValueError):
            ops.gru_seq_lengths(bad, 3, 4, cpu)
        with pytest.raises(ValueError):
            ops.gru_seq_lengths(torch.tensor(bad), 3, 4, cpu)
    ldev, flag = ops.gru_seq_lengths([4, 1, 2], 3, 4, cpu)
    assert ldev.dtype == torch.int64 and ldev.tolist() == [4, 1, 2] and flag is None
    assert ops.gru_seq_lengths(None, 3, 4, cpu) == (None, None)


def test_module_rejects_what_the_kernels_do_not_take(pkg):
    with pytest.raises(NotImplementedError):
        pkg.GRU(8, 8, bias=False)
    m = pkg.GRU(6, 8)
    with pytest.raises(TypeError):
        m(torch.zeros(3, 2, 6))                    # a CPU tensor: no torch fallback
    import types
    for name in ("seq2seq", "joint_embedding"):        # the baselines themselves are not part of this change
        with pytest.raises(NotImplementedError):
            pkg.checkpoint.init_model(types.SimpleNamespace(model=name), None, None, 27, "cpu")


def _g18(H):
    z = np.load(os.path.join(GOLDEN, "g18_seq2seq_encoder.npz"))
    pre = f"h{H}/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


@pytest.mark.parametrize("H", [8, 12])
def test_reference_chain_reproduces_the_reference_encoder(H):
    """tests/gru_seq_ref.RefEncoder (single-layer double nn.GRU modules, enforce_sorted=False) against the reference's own EncoderRNN."""
    g = _g18(H)
    state = {k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state/")}
    enc = R.RefEncoder(state, 2)
    out, hid = enc(torch.from_numpy(g["input_seqs"]), g["lengths"].tolist())
    assert float((out.detach() - torch.from_numpy(g["outputs"])).abs().max()) <= 1e-12
    assert float((hid.detach() - torch.from_numpy(g["hidden"])).abs().max()) <= 1e-12
    ((out * torch.from_numpy(g["c_out"])).sum() + (hid * torch.from_numpy(g["c_hid"])).sum()).backward()
    grads = enc.grads()
    assert set(grads) == set(state)
    for k, v in grads.items():
        ref = torch.from_numpy(g["grad/" + k])
        assert float((v - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k
    assert float(grads["embedding.weight"][0].abs().max()) == 0.0          # token 0 is padding only


@pytest.mark.parametrize("D, lengths, with_h0", [(1, [5, 1, 3], False), (2, [2, 5, 1], True), (2, [4, 4, 4], False)])
def test_reference_chain_matches_the_numpy_cell_loop(D, lengths, with_h0):
    g = torch.Generator().manual_seed(5)
    B, T, K, H, n_layers = len(lengths), max(lengths), 6, 8, 2
    state = {}
    for l in range(n_layers):
        for s in ("", "_reverse")[:D]:
            state[f"weight_ih_l{l}{s}"] = torch.randn(3 * H, K if l == 0 else D * H, generator=g, dtype=torch.float64) * 0.4
            state[f"weight_hh_l{l}{s}"] = torch.randn(3 * H, H, generator=g, dtype=torch.float64) * 0.4
            state[f"bias_ih_l{l}{s}"] = torch.randn(3 * H, generator=g, dtype=torch.float64) * 0.1
            state[f"bias_hh_l{l}{s}"] = torch.randn(3 * H, generator=g, dtype=torch.float64) * 0.1
    x = torch.randn(B, T, K, generator=g, dtype=torch.float64)
    h0 = torch.randn(n_layers * D, B, H, generator=g, dtype=torch.float64) if with_h0 else None
    with torch.no_grad():
        y, hn = R.RefGRU(state, n_layers, D)(x, lengths, h0)
    cur, hs = x.numpy(), []
    for l in range(n_layers):
        outs = []
        for d, s in enumerate(("", "_reverse")[:D]):
            yl, hl = R.numpy_layer(cur, *(state[f"{k}_l{l}{s}"].numpy() for k in R.PARAM_KINDS), lengths,
                                   None if h0 is None else h0[l * D + d].numpy(), reverse=(d == 1))
            outs.append(yl); hs.append(hl)
        cur = np.concatenate(outs, axis=2)
    assert float(np.abs(y.numpy() - cur).max()) <= 1e-12
    assert float(np.abs(hn.numpy() - np.stack(hs)).max()) <= 1e-12
