#!/usr/bin/env python3
"""Joint-embedding synthesis: rnn.GRU's few-row eval dispatch (csrc/gru_vec.hip, one launch per GRU layer) against the per-step path
(few_row_eval = False: csrc/gru_seq.hip, one launch per time step), same process, same weights (MI355X only; no fallback).

EmbeddingNet(mode='random') of the reference's geometry (context GRU H = 256 x 1 direction x 2 layers, decoder GRU H = 300 x 2 directions x 4
layers, 34 frames, pose_dim 27, 36 266 audio samples per window) at B = 1, 2, 4: one eval 'speech' forward (EmbeddingNet.synthesize on
one side, the eval forward with the dispatch off on the other), then one whole generate_gestures_batch call for B four-window utterances.
`--warmup` untimed runs per side, then `--repeats` runs alternating between the two, each timed with HIP events; medians and ranges are
reported.  Prints one JSON line; --out also writes it, with a heading, to a text file.

    python tools/joint_embed_synth_bench.py --out profiles/joint_embed_synth.txt

--window adds the third variant, the opt-in paths: EmbeddingNet.synthesize(constant_input=True) for the single forward, and for the
four-window utterance generate_gestures_batch(window_decoder=True) without and with the hipGraph (a decoder built, and with the graph
captured, inside every timed call -- what a caller of generate_gestures pays) and the same four windows on a decoder that is KEPT across
utterances (seed() + window() x 4: capture paid once, outside the timed runs).  All variants alternate inside one repeat loop; each ratio is
against the few-row path, the parent's default.

    python tools/joint_embed_synth_bench.py --window --out profiles/joint_embed_window.txt
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
    ap.add_argument("--window", action="store_true", help="also time the constant-input decoder and the window decoder (graph off / on)")
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
        if few == "const":
            return net.synthesize(ids, audio, pre, constant_input=True)
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

    NAMES = {True: "few_row", False: "per_step"}

    def compare(fn, extra=()):
        sides = (True, False) + tuple(extra)
        for few in sides:
            for _ in range(a.warmup):
                timed(fn, few)
        t = {few: [] for few in sides}
        for _ in range(a.repeats):
            for few in sides:
                t[few].append(timed(fn, few))
        stat = lambda v: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
        out = {NAMES.get(few, few): stat(t[few]) for few in sides}
        out["speedup"] = round(statistics.median(t[False]) / statistics.median(t[True]), 2)
        for few in extra:                                        # the opt-in paths against the parent's default; kept if median < its minimum
            out[few]["few_row_over_this"] = round(statistics.median(t[True]) / statistics.median(t[few]), 2)
            out[few]["median_below_few_row_min"] = bool(statistics.median(t[few]) < min(t[True]))
        return out

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
            res["eval_speech_forward"][f"B{B}"] = compare(lambda few: forward(few, ids, audio, pre), ("const",) if a.window else ())
            audios = [(0.1 * r.randn(8 * 16000)).astype(np.float32) for _ in range(B)]

            kept = {}

            def kept_decoder(graph):
                """Four windows on a decoder kept across utterances: seed() + window() per window + the stacked result on the host."""
                S = pkg.synthesize
                if graph not in kept:
                    kept[graph] = S.JointEmbedWindowDecoder(args, net, B, dev, graph=graph)
                dec = kept[graph]
                dec.seed(None)
                n_win = S.num_windows(len(audios[0]) / 16000, NF, NPRE, 15)
                total = torch.zeros(B, n_win * (NF - NPRE) + NPRE, PD, device=dev)
                for i in range(n_win):
                    ins = [S.window_inputs(args, lang, au, words, i) for au in audios]
                    out = dec.window(torch.from_numpy(np.stack([x[1] for x in ins])), torch.from_numpy(np.stack([x[0] for x in ins])), first=(i == 0))
                    total[:, i * (NF - NPRE):i * (NF - NPRE) + NF].copy_(out)
                return total.cpu().numpy()

            def gen(few):
                if few in ("window_decoder", "window_decoder_graph"):                # a decoder (and its graph) per call
                    S = pkg.synthesize
                    dec = S.JointEmbedWindowDecoder(args, net, B, dev, graph=True) if few == "window_decoder_graph" else True
                    return S.generate_gestures_batch(args, net, lang, audios, [words] * B, window_decoder=dec)
                if few in ("kept_decoder", "kept_decoder_graph"):
                    return kept_decoder(few == "kept_decoder_graph")
                if few:
                    return pkg.synthesize.generate_gestures_batch(args, net, lang, audios, [words] * B)
                # the parent's path under the same window loop
                net.synthesize = lambda i_, a_, p_, inject=None: forward(False, i_, a_, p_)
                try:
                    return pkg.synthesize.generate_gestures_batch(args, net, lang, audios, [words] * B)
                finally:
                    del net.synthesize
            res["generate_gestures_4_windows"][f"B{B}"] = compare(
                gen, ("window_decoder", "window_decoder_graph", "kept_decoder", "kept_decoder_graph") if a.window else ())
    pkg.ops.check_async_errors()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            head = ("Joint-embedding synthesis, few-row GRU dispatch against the per-step path" +
                    (", the constant-input decoder and the window decoder (tools/joint_embed_synth_bench.py --window)" if a.window
                     else " (tools/joint_embed_synth_bench.py)"))
            f.write(head + ", times in ms\n" + line + "\n")


if __name__ == "__main__":
    main()
