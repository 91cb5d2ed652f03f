"""End-to-end time of a long utterance through synthesize.generate_gestures_batch: the default path (per-window numpy slicing, word loop and
host-to-device copies; numpy fits at the end) against on_device=True (csrc/utterance.hip), measured ALTERNATELY in one process.

    python tools/utterance_bench.py [--seconds 60] [--reps 20] [--warmup 5] [--out profiles/utterance.txt]

Cases: the multimodal model at B = 1 and B = 4, seq2seq at B = 4; a 60 s utterance is 30 windows.  return_device is off on both sides, so both
read the result back.  Per case and path: median wall clock (perf_counter around the call, which ends with the read-back) and median HIP
event time on the current stream over the same calls."""
import argparse
import importlib
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")
syn = pkg.synthesize
V, SR = 20000, 16000


class Lang:
    SOS_token, EOS_token = 1, 2

    def get_word_index(self, w):
        return 4 + (sum(map(ord, w)) % (V - 4))


def utterances(B, seconds):
    rng = np.random.default_rng(1)
    audios = [(0.1 * rng.standard_normal(int(seconds * SR))).astype(np.float32) for _ in range(B)]
    words = [[[f"w{b}_{k}", 0.4 * k, 0.4 * k + 0.3] for k in range(int(seconds / 0.4))] for b in range(B)]
    return audios, words


def timed(fn, reps, warmup):
    """fns: {name: callable}; one call of each in turn per repetition.  Returns {name: (median wall ms, median event ms)}."""
    wall, evt = {k: [] for k in fn}, {k: [] for k in fn}
    for r in range(warmup + reps):
        for name, f in fn.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= warmup:
                wall[name].append((t1 - t0) * 1e3); evt[name].append(e0.elapsed_time(e1))
    return {k: (statistics.median(wall[k]), statistics.median(evt[k])) for k in fn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = importlib.import_module(pkg.__name__ + ".config")
    m_args = cfg.load_config("multimodal_context")
    m_args.motion_resampling_framerate = 15
    G = pkg.PoseGenerator(m_args, 27, V, 300, None, pkg.Vocab.speakers(1371)).to(dev).eval()
    s_args = SimpleNamespace(model="seq2seq", hidden_size=200, n_layers=2, dropout_prob=0.0, n_pre_poses=4, n_poses=34, GAN_noise_size=0,
                             motion_resampling_framerate=15, z_type="none", mean_dir_vec=[0.0] * 27)
    S = pkg.Seq2SeqNet(s_args, 27, 34, V, 300, None).to(dev).eval()
    lang, lines = Lang(), []
    for tag, args, net, B in (("multimodal B=1", m_args, G, 1), ("multimodal B=4", m_args, G, 4), ("seq2seq B=4", s_args, S, 4)):
        audios, words = utterances(B, a.seconds)
        kw = dict(vids=list(range(1, B + 1))) if net is G else {}
        res = timed({"default": lambda: syn.generate_gestures_batch(args, net, lang, audios, words, **kw),
                     "on_device": lambda: syn.generate_gestures_batch(args, net, lang, audios, words, on_device=True, **kw)}, a.reps, a.warmup)
        n_win = syn.num_windows(a.seconds)
        (dw, de), (ow, oe) = res["default"], res["on_device"]
        lines.append(f"{tag:15s} {n_win} windows  default: wall {dw:8.3f} ms, events {de:8.3f} ms   on_device: wall {ow:8.3f} ms, events {oe:8.3f} ms   "
                     f"wall ratio {dw / ow:.3f}")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"tools/utterance_bench.py --seconds {a.seconds} --reps {a.reps} --warmup {a.warmup}: medians, the two paths measured alternately\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
