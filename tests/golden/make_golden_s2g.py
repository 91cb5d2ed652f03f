#!/usr/bin/env python3
"""Speech2Gesture fixtures from the REAL reference (build container only; imports the reference like make_golden.py).

The installed torch rejects nn.Conv1d/2d(padding='SAME'); the old torch the reference was written for accepted the string and Conv*_tf
overwrote it and padded in its own forward.  The only patch here: _ConvNd.__init__ maps 'SAME' / 'VALID' to padding 0 before Conv*_tf
resets self.padding.  Parameters and inputs: tests/s2g_inputs.py.

    python tests/golden/make_golden_s2g.py   -> golden_s2g_keys.json, g13_s2g_b4.npz, g14_s2g_b128.npz

Deviation from running the reference untouched, besides the shim: the fixtures are fp64 runs, and AudioEncoder.forward casts its input
with .float(); torch.Tensor.float is the identity while the reference runs (nothing else in it calls .float()), so the modules stay fp64.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402
from tests.s2g_inputs import fill_state, make_inputs  # noqa: E402

SEED_G, SEED_D, SEED_X = 11, 12, 13


def _shim():
    from torch.nn.modules import conv
    orig = conv._ConvNd.__init__

    def init(self, *a, **kw):
        a = list(a)
        if len(a) >= 5 and isinstance(a[4], str) and a[4] in ("SAME", "VALID"):     # (in, out, kernel, stride, padding, ...) positional
            a[4] = (0,) * len(a[2])
        orig(self, *a, **kw)
    conv._ConvNd.__init__ = init


def import_reference():
    sys.path.insert(0, MG.REF)
    _shim()
    import model.speech2gesture as s2g
    import train_eval.train_speech2gesture as tr
    return s2g, tr


def main():
    torch.set_num_threads(8)
    s2g, tr = import_reference()
    torch.manual_seed(0)
    G = fill_state(s2g.Generator(34, 27, 4), SEED_G).double()
    D = fill_state(s2g.Discriminator(27), SEED_D).double()
    keys = {"gen": [[k, list(v.shape)] for k, v in G.state_dict().items()], "dis": [[k, list(v.shape)] for k, v in D.state_dict().items()],
            "gen_params": sum(p.numel() for p in G.parameters()), "dis_params": sum(p.numel() for p in D.parameters())}
    with open(os.path.join(HERE, "golden_s2g_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")

    # fp64 throughout: AudioEncoder.forward's .float() would drop the fp64 modules' input to fp32, so Tensor.float is the identity while the
    # reference runs (the fp16 spectrogram is exact in fp64; nothing else calls it)
    orig_float = torch.Tensor.float
    torch.Tensor.float = lambda t: t
    try:
        for B, name in ((4, "g13_s2g_b4.npz"), (128, "g14_s2g_b128.npz")):
            # B = 4: a data seed without LeakyReLU near-ties in the 1-D layers (tie_free_seed); B = 128 has ~5 M such inputs per iteration,
            # so no seed is free of them: SEED_X, with the count of near-ties recorded as evidence
            seed = tie_free_seed(s2g, B) if B == 4 else SEED_X
            spec, poses = make_inputs(B, seed)
            out = {"data_seed": np.array(seed), "batch": np.array(B)}
            G = fill_state(s2g.Generator(34, 27, 4), SEED_G).double()
            D = fill_state(s2g.Discriminator(27), SEED_D).double()
            run(G, D, tr, spec, poses, out, full=B == 4)
            gradients(s2g, spec, poses, out)
            np.savez_compressed(os.path.join(HERE, name), **out)
            print(name, "losses", out["losses"], "1-D near-ties", out.get("near_ties"))
    finally:
        torch.Tensor.float = orig_float
    print("keys", len(keys["gen"]), len(keys["dis"]), keys["gen_params"], keys["dis_params"])


MARGIN = 1.5e-5


def tie_free_seed(s2g, B):
    """The first data seed from SEED_X on whose train-mode forward every LeakyReLU input of the 1-D layers (U-Net, decoder) and of the
    discriminator keeps |x| >= MARGIN.  An element closer to zero than the fp32 path's forward error (~7e-6 relative) can take the other
    branch there and move single gradient entries above it by tens of percent (a 4.4e-6 input did at seed 13); the 2-D blocks have
    10^5..10^6 elements per channel, where one flip moves nothing measurable, and are not screened."""
    for seed in range(SEED_X, SEED_X + 1000):
        G = fill_state(s2g.Generator(34, 27, 4), SEED_G).double().train()
        D = fill_state(s2g.Discriminator(27), SEED_D).double().train()
        low = [float("inf")]

        def hook(mod, inp):
            low[0] = min(low[0], float(inp[0].abs().min()))
        for n, m in list(G.named_modules()) + list(D.named_modules()):
            if isinstance(m, torch.nn.LeakyReLU) and "first_net" not in n:
                m.register_forward_pre_hook(hook)
        spec, poses = make_inputs(B, seed)
        with torch.no_grad():
            o = G(spec.double(), poses[:, :4].double())
            D(poses.double()[:, 1:] - poses.double()[:, :-1])
            D(o[:, 1:] - o[:, :-1])
        if low[0] >= MARGIN:
            print("data seed", seed, "smallest LeakyReLU input", low[0])
            return seed
    raise RuntimeError("no tie-free data seed")


def gradients(s2g, spec, poses, out):
    """Both steps' gradients at the SEEDED parameters (fresh modules, train mode): d dis_error / d D, then d (100 L1 + 10 mse(1, D(G)))
    / d G through the same D.  In the iteration itself the G step sees the Adam-stepped D, whose first step is lr * sign(g): D weights
    with a gradient within rounding of zero move by +-lr on noise there, so its G gradient is compared through this pinned D instead."""
    G = fill_state(s2g.Generator(34, 27, 4), SEED_G).double().train()
    D = fill_state(s2g.Discriminator(27), SEED_D).double().train()
    s, p = spec.double(), poses.double()
    o = G(s, p[:, :4])
    tm, om = p[:, 1:] - p[:, :-1], o[:, 1:] - o[:, :-1]
    dr, df = D(tm), D(om.detach())
    (F.mse_loss(torch.ones_like(dr), dr) + F.mse_loss(torch.zeros_like(df), df)).backward()
    for k, q in D.named_parameters():
        t = q.grad.reshape(-1).numpy()
        out["gradD." + k] = t if t.size <= 64 else t[MG.sample_idx(t.size, 64)]
        out["gradnormD." + k] = np.array(np.linalg.norm(t))
    D.zero_grad()
    do = D(om)
    (100.0 * torch.nn.L1Loss()(o, p) + 10.0 * F.mse_loss(torch.ones_like(do), do)).backward()
    for k, q in G.named_parameters():
        t = q.grad.reshape(-1).numpy()
        out["gradG." + k] = t if t.size <= 64 else t[MG.sample_idx(t.size, 64)]
        out["gradnormG." + k] = np.array(np.linalg.norm(t))


def run(G, D, tr, spec, poses, out, full=True):
    """One train_iter_speech2gesture.  full: also the eval- and train-mode forward outputs (B = 4 only; B = 128 keeps scalars and samples)."""
    G.eval()
    with torch.no_grad():
        o = G(spec.double(), poses[:, :4].double()).numpy()
        if full:
            out["eval_out"] = o
    G.train()
    # one full iteration in fp64 (the fp16 spectrogram is exact in fp64; the reference casts with .float(), which is exact too)
    args = argparse.Namespace(n_pre_poses=4, loss_regression_weight=100.0, loss_gan_weight=10.0)
    g_opt = torch.optim.Adam(G.parameters(), lr=1e-3, betas=(0.5, 0.999))
    d_opt = torch.optim.Adam(D.parameters(), lr=1e-3 * 0.2, betas=(0.5, 0.999))
    low = []

    def hook(mod, inp):
        low.append(int((inp[0].abs() < 2e-6).sum()))
    hooks = [m.register_forward_pre_hook(hook) for n, m in G.named_modules() if isinstance(m, torch.nn.LeakyReLU) and "first_net" not in n]
    with torch.no_grad():
        o = G(spec.double(), poses[:, :4].double()).numpy()
        if full:
            out["train_out"] = o
    for h in hooks:
        h.remove()
    out["near_ties"] = np.array(sum(low))                   # 1-D LeakyReLU inputs of the train forward with |x| < 2e-6
    fill_state(G, SEED_G)                                    # the extra forward moved G's running stats: start again from the seed
    for m in G.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.reset_running_stats()
    losses = tr.train_iter_speech2gesture(args, spec.double(), poses.double(), G, D, g_opt, d_opt, torch.nn.L1Loss())
    out["losses"] = np.array([losses["loss"], losses["gen"], losses["dis"]])
    for k, q in G.named_parameters():                       # the G step's own gradients (G was zeroed before it): 64 sampled entries
        t = q.grad.reshape(-1).numpy()
        out["itgradG." + k] = t if t.size <= 64 else t[MG.sample_idx(t.size, 64)]
    for k, v in list(D.state_dict().items()) + [("G." + k, v) for k, v in G.state_dict().items()]:
        k = k if k.startswith("G.") else "D." + k
        t = v.reshape(-1).numpy()
        out[k] = t if t.size <= 64 else t[MG.sample_idx(t.size, 64)]       # post-Adam parameters / BatchNorm buffers: 64 sampled entries


if __name__ == "__main__":
    main()
