#!/usr/bin/env python3
"""A validation pass of FGD through both evaluators on one network (MI355X only; no fallback).

200 pushes of B = 128 (T = 34, pose_dim = 27) into fgd.EmbeddingSpaceEvaluator (features copied to the host per batch, numpy / scipy finish) and
into fgd.DeviceEmbeddingSpaceEvaluator (streaming moments and Jacobi finish on the device, csrc/fgd.hip), each followed by get_scores().  A pass is
timed with HIP events around the push loop and with the host clock from the first push to the returned scores (get_scores ends in a host read,
so the clock sees finished work).  One untimed warm-up pass per evaluator, then `--repeats` passes alternating between the two; medians and
ranges are reported, and the two scores next to each other.  Prints one JSON line; --out also writes it, with a heading, to a text file.

    python tools/fgd_bench.py --out profiles/fgd_device.txt
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_pass(torch, ev, batches):
    ev.reset()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for gen, real in batches:
        ev.push_samples(None, None, gen, real)
    e1.record()
    t_issued = time.perf_counter()
    scores = ev.get_scores()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return {"loop_ms_events": e0.elapsed_time(e1), "loop_ms_host_issue": (t_issued - t0) * 1e3, "pass_ms_wall": (t1 - t0) * 1e3}, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fgd_bench: needs a GPU (nothing is measured without one)")
    hip = importlib.import_module("gesture-generation-from-trimodal-context_amd")
    dev = torch.device("cuda:0")
    args = hip.config.load_config("multimodal_context")
    torch.manual_seed(0)
    net = hip.EmbeddingNet(args, 27, 34, None, None, None, mode="pose").to(dev)
    gen_t = torch.Generator(device="cpu").manual_seed(1)
    distinct = [(0.3 * torch.randn(a.batch, 34, 27, generator=gen_t)).to(dev) for _ in range(16)]           # 8 (generated, real) pairs, cycled
    batches = [(distinct[(2 * i) % 16], distinct[(2 * i + 1) % 16]) for i in range(a.pushes)]
    evs = {"host": hip.fgd.EmbeddingSpaceEvaluator.from_net(net, 4), "device": hip.fgd.DeviceEmbeddingSpaceEvaluator.from_net(net, 4)}
    scores, runs = {}, {k: [] for k in evs}
    for k, ev in evs.items():                                                                                # warm-up: code objects, allocator
        one_pass(torch, ev, batches)
    for _ in range(a.repeats):
        for k, ev in evs.items():
            t, scores[k] = one_pass(torch, ev, batches)
            runs[k].append(t)
    res = {"tool": "fgd_bench", "pushes": a.pushes, "batch": a.batch, "repeats": a.repeats, "device_name": torch.cuda.get_device_name(0)}
    for k in evs:
        for f in ("loop_ms_events", "loop_ms_host_issue", "pass_ms_wall"):
            v = [r[f] for r in runs[k]]
            res[f"{k}_{f}"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        res[f"{k}_scores"] = [float(scores[k][0]), float(scores[k][1])]
    res["wall_ratio_host_over_device"] = res["host_pass_ms_wall"]["median"] / res["device_pass_ms_wall"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("FGD validation pass, host evaluator against device evaluator (tools/fgd_bench.py), measured on " + res["device_name"] + ".\n"
                    "loop_ms_events: HIP events around the push loop; pass_ms_wall: host clock from the first push to the returned scores.\n"
                    "No speed threshold gates this path; the numbers are a record.\n\n" + line + "\n")


if __name__ == "__main__":
    main()
