#!/usr/bin/env python3
"""The joint-embedding baseline at the reference configuration, HIP path against the same model on torch-ROCm's own layers (MI355X only; no
fallback).

B = 128, vocabulary 20 000, embedding 300, TCN 300 x 4, 34 frames, 4 pre-poses, pose_dim 27, 36 267 audio samples.  The comparator is the
stock-torch chain of tests/joint_embed_ref.py in fp32 on the same GPU in the same invocation, from the same seeded state.  Dropout is 0 on
both sides (the chain takes dropout only as injected masks, so neither side draws one and the two compute the same function); eps is drawn
by each side itself.  Rows: ms per train_iter_embed ('speech', 'pose': zero gradients, forward of both encoders, loss, backward, Adam, one
host read), ms per eval 'speech' forward at B = 1 and B = 128, us per latent-head launch (ContextEncoder.out + fc_mu / fc_logvar +
reparameterize: 256 -> 128 -> 32 with the tail; pre_pose_net: 108 -> 32 -> 32) against the same head on torch's ops.  `--warmup` untimed
runs per side, then `--repeats` runs alternating between the two sides, each timed with HIP events around a device synchronisation; medians
and ranges are reported.  Prints one JSON line; --out also writes the table to a text file.

    python tools/joint_embed_bench.py --out profiles/joint_embed.txt
"""
import argparse
import importlib
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import joint_embed_ref as R
    pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")
    ops = pkg.ops
    dev = torch.device("cuda")
    B, V = a.batch, a.words
    args = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34, wordembed_dim=300)
    state = R.make_state(7, V)

    def hip_net():
        net = pkg.EmbeddingNet(args, 27, 34, V, 300, None, mode="random")
        net.load_state_dict(state, strict=True)
        net = net.to(dev)
        net.context_encoder.tcn_dropout = net.context_encoder.emb_dropout = 0.0
        net.decoder.gru.dropout = 0.0
        return net

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def pair(hip_fn, ref_fn):
        for _ in range(a.warmup):
            hip_fn(); ref_fn()
        th, tr = [], []
        for _ in range(a.repeats):
            th.append(timed(hip_fn)); tr.append(timed(ref_fn))
        f = lambda t: {"median": statistics.median(t), "min": min(t), "max": max(t)}
        return f(th), f(tr)

    rows = {}
    ids, audio, target, _ = R.make_inputs(9, B, V)
    ids, audio, target = ids.to(dev), audio.to(dev), target.to(dev)
    for mode in ("speech", "pose"):
        net, ref = hip_net().train(), R.build(state, torch.float32, dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        ropt = torch.optim.Adam(ref.parameters(), lr=5e-4, betas=(0.5, 0.999))
        def ref_step():
            R.train_iter_embed(ref, ropt, ids, audio, target, mode, {"c.eps": torch.randn(B, 32, device=dev)})
        rows[f"train_iter_embed '{mode}' B={B} [ms]"] = pair(lambda: pkg.train_iter_embed(args, 0, ids, audio, target, net, opt, mode), ref_step)
    for b in (1, B):
        net, ref = hip_net().eval(), R.build(state, torch.float32, dev).eval()
        i_, a_, t_ = ids[:b].contiguous(), audio[:b].contiguous(), target[:b].contiguous()
        p_ = t_[:, :4].contiguous()
        def hip_fwd():
            with torch.no_grad():
                net(i_, a_, p_, None, "speech")
        def ref_fwd():
            with torch.no_grad():
                ref(i_, a_, p_, None, "speech", {"c.eps": torch.randn(b, 32, device=dev)})
        rows[f"eval 'speech' forward B={b} [ms]"] = pair(hip_fwd, ref_fwd)
    # the latent heads alone, one launch each way against torch's ops for the same arithmetic
    g = torch.Generator().manual_seed(3)
    for name, (b, K0, N1, N2, tail, training) in {"context head train": (B, 256, 128, 32, True, True), "pre_pose head train": (B, 108, 32, 32, False, True),
                                                   "context head eval": (B, 256, 128, 32, True, False), "context head eval B=1": (1, 256, 128, 32, True, False)}.items():
        r = lambda *s: torch.randn(*s, generator=g).to(dev)
        x, w1, b1, ga, be, w2, b2 = r(b, K0), r(N1, K0) / K0 ** 0.5, r(N1), 1 + 0.1 * r(N1), r(N1), r(N2, N1) / N1 ** 0.5, r(N2)
        rm, rv, nbt = torch.zeros(N1, device=dev), torch.ones(N1, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        tl = (r(N2, N2) / N2 ** 0.5, r(N2), 0.1 * r(N2, N2), r(N2)) if tail else None
        eps, dout, out = r(b, N2), r(b, N2), torch.empty(b, N2, device=dev)
        def hip_f():
            return ops.latent_head_fwd(x, w1, b1, ga, be, rm, rv, nbt, w2, b2, out, training=training, slope=0.0, tail=tl, eps=eps if tail else None)
        def ref_f(xx=x):
            h = F.linear(F.relu(F.batch_norm(F.linear(xx, w1, b1), rm, rv, ga, be, training, 0.1, 1e-5)), w2, b2)
            if tail:
                mu, lv = F.linear(h, tl[0], tl[1]), F.linear(h, tl[2], tl[3])
                h = mu + eps * torch.exp(0.5 * lv)
            return h
        def ref_nograd():
            with torch.no_grad():
                ref_f()
        rows[f"{name} ({b}, {K0}, {N1}, {N2}) forward [us]"] = tuple({k: 1e3 * v for k, v in d.items()} for d in pair(hip_f, ref_nograd))
        if training:
            tp = hip_f()
            dx = torch.empty_like(x)
            ps = [w1, b1, ga, be, w2, b2] + (list(tl) if tail else [])
            def hip_b():
                ops.latent_head_bwd(dout, tp, w1, ga, be, w2, tail=(tl[0], tl[2]) if tail else None, dx=dx)
            xr = x.clone().requires_grad_(True)
            for p in ps:
                p.requires_grad_(True)
            y = ref_f(xr)
            def ref_b():
                torch.autograd.grad(y, [xr] + ps, dout, retain_graph=True)
            rows[f"{name} ({b}, {K0}, {N1}, {N2}) backward [us]"] = tuple({k: 1e3 * v for k, v in d.items()} for d in pair(hip_b, ref_b))
            for p in ps:
                p.requires_grad_(False)
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "batch": B, "words": V, "warmup": a.warmup, "repeats": a.repeats,
           "rows": {k: {"hip": h, "torch_fp32_chain": t, "torch_over_hip": t["median"] / h["median"]} for k, (h, t) in rows.items()}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/joint_embed_bench.py  {res['device']}  torch {res['torch']}  B = {B}, V = {V}, warm-up {a.warmup}, {a.repeats} timed runs per side\n")
            f.write("# medians (min .. max); comparator: the stock-torch chain of tests/joint_embed_ref.py in fp32 on the same GPU, same invocation\n")
            f.write(f"{'row':64s} {'HIP path':>28s} {'torch fp32 chain':>28s} {'torch / HIP':>12s}\n")
            for k, (h, t) in rows.items():
                c = lambda d: f"{d['median']:9.3f} ({d['min']:.3f} .. {d['max']:.3f})"
                f.write(f"{k:64s} {c(h):>28s} {c(t):>28s} {t['median'] / h['median']:12.2f}\n")


if __name__ == "__main__":
    main()
