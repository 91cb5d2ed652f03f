#!/usr/bin/env python3
"""EncoderRNN forward + backward at the Seq2Seq configuration, HIP path against torch-ROCm's own nn.GRU (MI355X only; no fallback).

B = 128 rows of lengths drawn from 1 .. 34, vocabulary 20 000, embed 300, 2 bidirectional layers of H = 200 (model/seq2seq_net.py:14-56; train
mode, which MIOpen's RNN backward requires, with the inter-layer dropout set to 0 on both sides so that neither draws a mask).  One iteration = forward, a sum-of-squares loss formed by torch on both sides, backward to every
parameter.  The yardstick runs the reference's own chain on the same packed input: nn.Embedding -> pack_padded_sequence -> nn.GRU ->
pad_packed_sequence -> sum of the halves.  `--warmup` untimed iterations per side, then `--repeats` iterations alternating between the two,
each timed with HIP events; medians and ranges are reported.  Prints one JSON line; --out also writes it, with a heading, to a text file.

    python tools/gru_seq_bench.py --out profiles/gru_seq.txt
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=34)
    ap.add_argument("--hidden", type=int, default=200)
    ap.add_argument("--embed", type=int, default=300)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import torch.nn as nn
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    if not torch.cuda.is_available():
        raise SystemExit("gru_seq_bench: needs a GPU (nothing is measured without one)")
    hip = importlib.import_module("gesture-generation-from-trimodal-context_amd")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = hip.EncoderRNN(a.words, a.embed, a.hidden, n_layers=2, dropout=0.0).to(dev).train()
    emb = nn.Embedding(a.words, a.embed).to(dev)
    gru = nn.GRU(a.embed, a.hidden, 2, dropout=0.0, bidirectional=True).to(dev).train()
    emb.load_state_dict(enc.embedding.state_dict()); gru.load_state_dict(enc.gru.state_dict(), strict=True)
    g = torch.Generator().manual_seed(1)
    lens = sorted(torch.randint(1, a.steps + 1, (a.batch,), generator=g).tolist(), reverse=True)
    lens[0] = a.steps
    seqs = torch.randint(1, a.words, (a.steps, a.batch), generator=g)
    for b, n in enumerate(lens):
        seqs[n:, b] = 0
    seqs = seqs.to(dev)

    def hip_iter():
        for p in enc.parameters():
            p.grad = None
        out, hid = enc(seqs, lens)
        ((out ** 2).sum() + (hid ** 2).sum()).backward()
        return out

    def torch_iter():
        for p in list(emb.parameters()) + list(gru.parameters()):
            p.grad = None
        out, hid = gru(pack_padded_sequence(emb(seqs), lens))
        out, _ = pad_packed_sequence(out)
        out = out[:, :, :a.hidden] + out[:, :, a.hidden:]
        ((out ** 2).sum() + (hid ** 2).sum()).backward()
        return out

    sides = {"hip": hip_iter, "torch": torch_iter}
    outs = {}
    for k, fn in sides.items():
        for _ in range(a.warmup):
            outs[k] = fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(a.repeats):
        for k, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"tool": "gru_seq_bench", "batch": a.batch, "steps": a.steps, "hidden": a.hidden, "embed": a.embed, "words": a.words, "layers": 2,
           "warmup": a.warmup, "repeats": a.repeats, "device_name": torch.cuda.get_device_name(0),
           "outputs_max_abs_diff": float((outs["hip"].detach() - outs["torch"].detach()).abs().max())}
    for k in sides:
        res[f"{k}_fwd_bwd_ms"] = {"median": statistics.median(times[k]), "min": min(times[k]), "max": max(times[k])}
    res["ratio_torch_over_hip"] = res["torch_fwd_bwd_ms"]["median"] / res["hip_fwd_bwd_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("EncoderRNN forward + backward at the Seq2Seq configuration, HIP path against torch-ROCm nn.GRU on the same packed input\n"
                    "(tools/gru_seq_bench.py), measured on " + res["device_name"] + ".  HIP events around one iteration, medians over the repeats.\n"
                    "No speed threshold gates this path; the numbers are a record.\n\n" + line + "\n")


if __name__ == "__main__":
    main()
