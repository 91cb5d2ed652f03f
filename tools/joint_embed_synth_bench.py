#!/usr/bin/env python3
"""Joint-embedding synthesis: rnn.GRU's few-row eval dispatch (csrc/gru_vec.hip, one launch per GRU layer) against the per-step path
(few_row_eval = False: csrc/gru_seq.hip, one launch per time step), same process, same weights (MI355X only; no fallback).

EmbeddingNet(mode='random') of the reference's geometry (context GRU H = 256 x 1 direction x 2 layers, decoder GRU H = 300 x 2 directions x 4
layers, 34 frames, pose_dim 27, 36 266 audio samples per window) at B = 1, 2, 4: one eval 'speech' forward (EmbeddingNet.synthesize on
one side, the eval forward with the dispatch off on the other), then one whole generate_gestures_batch call for B four-window utterances.
`--warmup` untimed runs per side, then `--repeats` runs alternating between the two, each timed with HIP events; medians and ranges are
reported.  Prints one JSON line; --out also writes it, with a heading, to a text file.

    python tools/joint_embed_synth_bench.py --out profiles/joint_embed_synth.txt
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
    NF, NPRE, PD, V = 34, 4, 27, 2000
    args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False, n_pre_poses=NPRE,
                           n_poses=NF, z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * PD)
    torch.manual_seed(0)
    net = pkg.EmbeddingNet(args, PD, NF, V, 300, None, mode="random").to(dev).eval()
    grus = (net.context_encoder.gru, net.decoder.gru)

    def forward(few, ids, audio, pre):
        if few:
            return net.synthesize(ids, audio, pre)
        for g in grus:
            g.few_row_eval = False
        return net(ids, audio, pre, None, "speech")[6]

    def timed(fn, few):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(few)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def compare(fn):
        for few in (True, False):
            for _ in range(a.warmup):
                timed(fn, few)
        t = {True: [], False: []}
        for _ in range(a.repeats):
            for few in (True, False):
                t[few].append(timed(fn, few))
        stat = lambda v: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
        return dict(few_row=stat(t[True]), per_step=stat(t[False]), speedup=round(statistics.median(t[False]) / statistics.median(t[True]), 2))

    lang = pkg.Vocab("words")
    for i in range(40):
        lang.index_word(f"w{i}")
    r = np.random.RandomState(3)
    words, t = [], 0.05
    while t < 7.9:
        d = float(r.uniform(0.12, 0.5))
        words.append([f"w{int(r.randint(40))}", round(t, 3), round(t + d, 3)])
        t += d + float(r.uniform(0.0, 0.3))
    res = {"config": dict(n_frames=NF, n_pre=NPRE, vocabulary=V, repeats=a.repeats, warmup=a.warmup), "eval_speech_forward": {},
           "generate_gestures_4_windows": {}}
    with torch.no_grad():
        for B in (1, 2, 4):
            ids = torch.randint(0, V, (B, NF), device=dev)
            audio, pre = 0.1 * torch.randn(B, 36266, device=dev), 0.5 * torch.randn(B, NPRE, PD, device=dev)
            res["eval_speech_forward"][f"B{B}"] = compare(lambda few: forward(few, ids, audio, pre))
            audios = [(0.1 * r.randn(8 * 16000)).astype(np.float32) for _ in range(B)]

            def gen(few):
                if few:
                    return pkg.synthesize.generate_gestures_batch(args, net, lang, audios, [words] * B)
                # the parent's path under the same window loop
                net.synthesize = lambda i_, a_, p_, inject=None: forward(False, i_, a_, p_)
                try:
                    return pkg.synthesize.generate_gestures_batch(args, net, lang, audios, [words] * B)
                finally:
                    del net.synthesize
            res["generate_gestures_4_windows"][f"B{B}"] = compare(gen)
    pkg.ops.check_async_errors()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("Joint-embedding synthesis, few-row GRU dispatch against the per-step path (tools/joint_embed_synth_bench.py), times in ms\n" + line + "\n")


if __name__ == "__main__":
    main()
