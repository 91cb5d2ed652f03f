#!/usr/bin/env python3
"""Eval-mode Seq2Seq decode: the one-launch kernel (csrc/seq2seq_decode.hip) against the per-step path (seq2seq.FUSED_EVAL_DECODE = False), same
process, same weights (MI355X only; no fallback).

H = 200, 2 layers, 34 frames, 4 pre-poses, pose_dim 27; (B, Te) = (1, 12), (32, 34), (128, 34).  One decode = BahdanauAttnDecoderRNN.decode
from given encoder outputs (keys product included on both sides).  Then one whole generate_gestures call for a 4-window utterance (encoder,
windows, host smoothing) both ways.  `--warmup` untimed runs per side, then `--repeats` runs alternating between the two, each timed with HIP
events; medians and ranges are reported.  Prints one JSON line; --out also writes it, with a heading, to a text file.

    python tools/seq2seq_synth_bench.py --out profiles/seq2seq_synth.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")
    dev = torch.device("cuda:0")
    H, NF, NPRE, PD = 200, 34, 4, 27
    args = SimpleNamespace(model="seq2seq", hidden_size=H, n_layers=2, dropout_prob=0.0, n_pre_poses=NPRE, n_poses=NF, GAN_noise_size=0,
                           z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * PD)
    torch.manual_seed(0)
    net = pkg.Seq2SeqNet(args, PD, NF, 2000, 300, None).to(dev).eval()
    dec = net.decoder.decoder

    def timed(fn, fused):
        pkg.seq2seq.FUSED_EVAL_DECODE = fused
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def compare(fn):
        for fused in (True, False):
            for _ in range(a.warmup):
                timed(fn, fused)
        t = {True: [], False: []}
        for _ in range(a.repeats):
            for fused in (True, False):
                t[fused].append(timed(fn, fused))
        stat = lambda v: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
        return dict(fused=stat(t[True]), per_step=stat(t[False]), speedup=round(statistics.median(t[False]) / statistics.median(t[True]), 2))

    res = {"config": dict(H=H, n_layers=2, n_frames=NF, n_pre=NPRE, repeats=a.repeats, warmup=a.warmup), "decode": {}}
    with torch.no_grad():
        for B, Te in ((1, 12), (32, 34), (128, 34)):
            enc, h0, poses = torch.randn(B, Te, H, device=dev), torch.randn(2, B, H, device=dev), torch.randn(B, NPRE, PD, device=dev)
            res["decode"][f"B{B}_Te{Te}"] = compare(lambda: dec.decode(enc, h0, poses, NF, NPRE))
        lang = pkg.Vocab("words")
        words, t = [], 0.05
        r = np.random.RandomState(3)
        for i in range(40):
            lang.index_word(f"w{i}")
        while t < 7.9:
            d = float(r.uniform(0.12, 0.5))
            words.append([f"w{int(r.randint(40))}", round(t, 3), round(t + d, 3)])
            t += d + float(r.uniform(0.0, 0.3))
        audio = np.zeros(8 * 16000, np.float32)
        res["generate_gestures_4_windows"] = compare(lambda: pkg.synthesize.generate_gestures(args, net, lang, audio, words))
    pkg.seq2seq.FUSED_EVAL_DECODE = True
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("Seq2Seq eval decode, one-launch kernel against the per-step path (tools/seq2seq_synth_bench.py), times in ms\n" + line + "\n")


if __name__ == "__main__":
    main()
