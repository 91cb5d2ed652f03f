"""fp64 references of the general GRU recurrence (csrc/gru_seq.hip) and of the modules on it (rnn.GRU, rnn.EncoderRNN).

The reference is torch.nn.GRU in double on the CPU -- ONE single-layer module per layer, fed through pack_padded_sequence(enforce_sorted=False),
inter-layer masks multiplied in between the layers, h0 passed, h_n and every gradient from autograd -- so it restates nothing of the
kernels' arithmetic.  numpy_layer is an independent dozen-line cell loop that pins what nn.GRU itself computes."""
import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

PARAM_KINDS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def param_names(n_layers, D):
    return [f"{k}_l{l}{s}" for l in range(n_layers) for s in ("", "_reverse")[:D] for k in PARAM_KINDS]


class RefGRU:
    """A stack of single-layer double nn.GRU modules holding the weights of `state` (nn.GRU's multi-layer names)."""

    def __init__(self, state, n_layers, D, dtype=torch.float64):
        """dtype=torch.float32: torch's own fp32 CPU nn.GRU, the yardstick the gradient gates of the GPU tests are measured from."""
        self.n_layers, self.D = n_layers, D
        H = state["weight_hh_l0"].shape[1]
        self.H, self.layers = H, []
        for l in range(n_layers):
            K = state[f"weight_ih_l{l}"].shape[1]
            m = nn.GRU(K, H, 1, batch_first=True, bidirectional=(D == 2)).to(dtype)
            with torch.no_grad():
                for s in ("", "_reverse")[:D]:
                    for k in PARAM_KINDS:
                        getattr(m, f"{k}_l0{s}").copy_(torch.as_tensor(state[f"{k}_l{l}{s}"]).to(dtype).cpu())
            self.layers.append(m)

    def __call__(self, x, lengths=None, h0=None, masks=None):
        """x (B, T, K) double; lengths: list or None; h0 (n_layers * D, B, H) or None; masks: {layer: (B, T, D*H)} applied to that layer's
        output.  Returns (y (B, T, D*H) with zeros at t >= length, h_n (n_layers * D, B, H))."""
        B, T, _ = x.shape
        lens = torch.as_tensor([T] * B if lengths is None else list(lengths), dtype=torch.int64)
        cur, hs = x, []
        for l, m in enumerate(self.layers):
            packed = pack_padded_sequence(cur, lens, batch_first=True, enforce_sorted=False)
            out, h = m(packed, None if h0 is None else h0[l * self.D:(l + 1) * self.D])
            cur, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
            hs.append(h)
            if masks is not None and l in masks:
                cur = cur * masks[l]
        return cur, torch.cat(hs, 0)

    def grads(self):
        out = {}
        for l, m in enumerate(self.layers):
            for s in ("", "_reverse")[:self.D]:
                for k in PARAM_KINDS:
                    g = getattr(m, f"{k}_l0{s}").grad
                    out[f"{k}_l{l}{s}"] = torch.zeros_like(getattr(m, f"{k}_l0{s}")) if g is None else g
        return out


def numpy_layer(x, w_ih, w_hh, b_ih, b_hh, lengths, h0, reverse):
    """One direction of one layer as a plain cell loop (fp64 numpy): y (B, T, H) with zeros at t >= length, and the last state."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    y, hn = np.zeros((B, T, H)), np.zeros((B, H))
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    for b in range(B):
        h = np.zeros(H) if h0 is None else h0[b].copy()
        ts = range(lengths[b] - 1, -1, -1) if reverse else range(lengths[b])
        for t in ts:
            gi, gh = w_ih @ x[b, t] + b_ih, w_hh @ h + b_hh
            r, z = sig(gi[:H] + gh[:H]), sig(gi[H:2 * H] + gh[H:2 * H])
            n = np.tanh(gi[2 * H:] + r * gh[2 * H:])
            h = (1.0 - z) * n + z * h
            y[b, t] = h
        hn[b] = h
    return y, hn


class RefEncoder:
    """EncoderRNN (model/seq2seq_net.py:14-56) on RefGRU: embedding -> packed bidirectional GRU -> directions summed.  state: the module's
    state dict (embedding.weight, gru.*)."""

    def __init__(self, state, n_layers, dtype=torch.float64):
        self.emb = torch.as_tensor(state["embedding.weight"]).to(dtype).clone().requires_grad_(True)
        self.gru = RefGRU({k[4:]: v for k, v in state.items() if k.startswith("gru.")}, n_layers, 2, dtype)

    def __call__(self, input_seqs, lengths, hidden=None):
        T = max(lengths)
        x = self.emb[input_seqs[:T].t()]                      # (B, T, E)
        y, h = self.gru(x, lengths, hidden)
        H = self.gru.H
        return (y[..., :H] + y[..., H:]).transpose(0, 1), h

    def grads(self):
        out = {"gru." + k: v for k, v in self.gru.grads().items()}
        out["embedding.weight"] = self.emb.grad
        return out


def grad_gate(ref64, ref32):
    """The gate of a gradient the project had no gate for: 4 x the error of torch's fp32 CPU nn.GRU against the fp64 reference on the same case
    (the margin covers another summation order and the operand split), floored at 1e-6 of the tensor's largest magnitude."""
    e32 = float((ref32.double() - ref64).abs().max())
    return max(4.0 * e32, 1e-6 * float(ref64.abs().max())), e32
