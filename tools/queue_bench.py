"""Wall time of the synthesis queue (synthesize.generate_gestures_queue, csrc/queue.hip) against lock-step synthesis
(synthesize.generate_gestures_batch(on_device=True)) on one ragged utterance set, full-size models.

    python tools/queue_bench.py [--utterances 64] [--passes 5] [--out profiles/queue.txt]

The set: `--utterances` clips with lengths log-uniform in 2 to 60 s from a fixed seed, a word every 0.4 s.  Per model the configurations ALTERNATE
in one process after one warm-up pass of each; a pass is one whole call on the whole set with return_device=True, timed by the host clock
around the call and a device synchronise (the read-back is the same for all and left out).  Reported per configuration: the median wall time
over the passes with the range, the rounds (forwards) the set takes, useful row-windows / (rounds x rows) -- integers, computed on the host --
and wall time per round.
  multimodal_context   lock-step with all utterances in one batch; lock-step in groups of R (a call per group, in the given order); the queue at
                       R = 4, 8, 16, 64.  Lock-step builds its window decoder and captures its graph in every call (the only way that path has);
                       the queue runs on a decoder kept across calls (graph captured in the warm-up pass) and, as `fresh`, on one built per call.
  joint_embedding      lock-step in groups of 4 on a kept JointEmbedWindowDecoder against the queue at R = 4 on a kept one.
  seq2seq              lock-step in groups of 4 against the queue at R = 4 on a kept Seq2SeqWindowDecoder.
The device RNG draws everywhere (timing; the tests compare bits)."""
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


def utterance_set(n, seed=7):
    rng = np.random.default_rng(seed)
    secs = np.exp(rng.uniform(np.log(2.0), np.log(60.0), size=n))
    audios = [(0.1 * rng.standard_normal(int(s * SR))).astype(np.float32) for s in secs]
    words = [[[f"w{k}", 0.4 * k, 0.4 * k + 0.3] for k in range(int(len(a) / SR / 0.4))] for a in audios]
    return secs, audios, words


def lockstep_rounds(n_win, R):
    return sum(max(n_win[g:g + R]) for g in range(0, len(n_win), R))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def compare(configs, passes):
    """configs: [(name, rows, rounds, fn)].  One warm-up pass of each, then `passes` timed passes, the configurations alternating."""
    for _, _, _, fn in configs:
        timed(fn)
    times = [[] for _ in configs]
    for _ in range(passes):
        for k, (_, _, _, fn) in enumerate(configs):
            times[k].append(timed(fn))
    return times


def report(lines, title, configs, times, useful):
    lines.append(f"\n{title}")
    lines.append(f"  {'configuration':<34}{'wall ms (median)':>17}{'range':>19}{'rounds':>8}{'useful':>8}{'ms/round':>10}")
    best = None
    for (name, rows, rounds, _), t in zip(configs, times):
        m = statistics.median(t)
        lines.append(f"  {name:<34}{m:>17.2f}{f'{min(t):.2f} .. {max(t):.2f}':>19}{rounds:>8}{useful / (rounds * rows):>8.3f}{m / rounds:>10.3f}")
        best = (m, name) if best is None or m < best[0] else best
    lines.append(f"  fastest for this set: {best[1]} ({best[0]:.2f} ms)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("queue_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    secs, audios, words = utterance_set(a.utterances)
    N, lang = len(audios), Lang()
    n_win = [syn.num_windows(len(x) / SR) for x in audios]
    useful = sum(n_win)
    lines = [f"tools/queue_bench.py --utterances {N} --passes {a.passes}: {N} utterances of {secs.min():.1f} to {secs.max():.1f} s (log-uniform, seed 7), "
             f"{useful} windows, the longest {max(n_win)}; configurations alternate, median of {a.passes} passes after one warm-up pass each"]
    vids = [1 + u % 1370 for u in range(N)]

    # ---- multimodal_context
    cfg = importlib.import_module(pkg.__name__ + ".config")
    m_args = cfg.load_config("multimodal_context")
    m_args.motion_resampling_framerate = 15
    G = pkg.PoseGenerator(m_args, 27, V, 300, None, pkg.Vocab.speakers(1371)).to(dev).eval()

    def lock(args, net, R, **kw):
        def run():
            for g in range(0, N, R):
                syn.generate_gestures_batch(args, net, lang, audios[g:g + R], words[g:g + R], on_device=True, return_device=True,
                                            **{k: (v[g:g + R] if k == "vids" else v) for k, v in kw.items()})
        return run

    def queue(args, net, R, dec=None, **kw):
        return lambda: syn.generate_gestures_queue(args, net, lang, audios, words, R, window_decoder=dec, return_device=True, **kw)

    configs = [(f"lock-step, one batch of {N}", N, lockstep_rounds(n_win, N), lock(m_args, G, N, vids=vids))]
    for R in (4, 8, 16):
        configs.append((f"lock-step, groups of {R}", R, lockstep_rounds(n_win, R), lock(m_args, G, R, vids=vids)))
    for R in (4, 8, 16, 64):
        rounds = syn.queue_schedule(n_win, R)[0]
        configs.append((f"queue, R = {R}, kept decoder", R, rounds, queue(m_args, G, R, syn.WindowDecoder(m_args, G, R, dev), vids=vids)))
        configs.append((f"queue, R = {R}, fresh decoder", R, rounds, queue(m_args, G, R, vids=vids)))
    report(lines, "multimodal_context (hidden 300, 4 layers)", configs, compare(configs, a.passes), useful)
    del configs

    # ---- joint_embedding
    j_args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34,
                             z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * 27)
    E = pkg.EmbeddingNet(j_args, 27, 34, V, 300, None, mode="random").to(dev).eval()
    assert N % 4 == 0, "the kept lock-step decoder takes whole groups of 4"
    configs = [("lock-step, groups of 4, kept decoder", 4, lockstep_rounds(n_win, 4),
                lock(j_args, E, 4, window_decoder=syn.JointEmbedWindowDecoder(j_args, E, 4, dev))),
               ("queue, R = 4, kept decoder", 4, syn.queue_schedule(n_win, 4)[0], queue(j_args, E, 4, syn.JointEmbedWindowDecoder(j_args, E, 4, dev)))]
    report(lines, "joint_embedding (hidden 300, 4 layers)", configs, compare(configs, a.passes), useful)

    # ---- seq2seq
    s_args = SimpleNamespace(model="seq2seq", hidden_size=200, n_layers=2, dropout_prob=0.0, n_pre_poses=4, n_poses=34, GAN_noise_size=0,
                             motion_resampling_framerate=15, z_type="none", mean_dir_vec=[0.0] * 27)
    S = pkg.Seq2SeqNet(s_args, 27, 34, V, 300, None).to(dev).eval()
    configs = [("lock-step, groups of 4", 4, lockstep_rounds(n_win, 4), lock(s_args, S, 4)),
               ("queue, R = 4, kept decoder", 4, syn.queue_schedule(n_win, 4)[0], queue(s_args, S, 4, syn.Seq2SeqWindowDecoder(s_args, S, 4, dev)))]
    report(lines, "seq2seq (hidden 200, 2 layers)", configs, compare(configs, a.passes), useful)

    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
