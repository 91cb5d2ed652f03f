#!/usr/bin/env python3
"""Times the autoencoder's VAE training step against its AE step on the layer engine (and the fused 18-launch AE step for scale) at one batch
size, same box, same process, interleaved rounds; prints one JSON line.  Also counts the library launches of each step.

    python tools/vae_bench.py [--batch 128] [--steps 200] [--warmup 30] [--rounds 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")
    dev = torch.device("cuda:0")
    args = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False, n_pre_poses=4, n_poses=34, wordembed_dim=300)
    torch.manual_seed(0)
    poses = 0.1 * torch.randn(a.batch, 34, 27, device=dev)
    kinds = {"vae_layer": dict(fused=False, variational_encoding=True), "ae_layer": dict(fused=False), "ae_fused": dict()}
    trainers = {}
    for k, kw in kinds.items():
        torch.manual_seed(1)
        trainers[k] = pkg.fgd.AutoencoderTrainer(pkg.EmbeddingNet(args, 27, 34).to(dev).train(), **kw)
    launches = {}
    real_call = pkg._lib.call
    for k, tr in trainers.items():
        for _ in range(a.warmup):
            tr.train_iter(poses, epoch=20) if k == "vae_layer" else tr.train_iter(poses)
        n = [0]

        def counting(name, *args_, _n=n):
            _n[0] += 1
            return real_call(name, *args_)
        pkg.ops.call = counting
        for mod in (pkg.layers, pkg.engine, pkg.fgd):
            if hasattr(mod, "call"):
                mod.call = counting
        tr.train_iter(poses, epoch=20) if k == "vae_layer" else tr.train_iter(poses)
        pkg.ops.call = real_call
        launches[k] = n[0]
    times = {k: [] for k in kinds}
    for _ in range(a.rounds):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                tr.train_iter(poses, epoch=20) if k == "vae_layer" else tr.train_iter(poses)
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.steps)
    out = {"batch": a.batch, "steps": a.steps, "rounds": a.rounds, "library_calls": launches,
           "ms_per_step_median": {k: statistics.median(v) for k, v in times.items()}, "ms_per_step_rounds": times}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
