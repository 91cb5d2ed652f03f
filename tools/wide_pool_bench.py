"""One tick of a serving process on the wide stream pool (synthesize.WideStreamPool, csrc/stream_pool_wide.hip) against the same tick on pools
of four (synthesize.StreamPool), full-size multimodal model, 160-sample pushes (10 ms of audio).

    python tools/wide_pool_bench.py [--sessions 4 32 128] [--strides 2] [--reps 3] [--out profiles/wide_pool.txt]
    python tools/wide_pool_bench.py --input-sr 44100 [...] [--out profiles/wide_pool_rs.txt]

S sessions are open; session i joins at tick (i * ticks per stride) // S, so the sessions' windows complete at phases spread over a stride
(200 ticks) and a tick completes windows of few sessions or of none.  A tick pushes 160 samples to every open session, two ways:
  wide     one WideStreamPool of S slots: one packed upload, one push launch, then the rounds
  fours    S / 4 StreamPools of four slots, each on a WindowDecoder of its own, driven in turn on one stream
After the join phase and one warm-up stride of each (graph capture), passes of `strides` strides ALTERNATE between the two, `reps` each.
Every tick is timed on the host: t_call = the push calls have returned, t_done = a device synchronise behind them has returned.
  push, no window     median t_call of the ticks that complete no window (what the serving thread pays per 10 ms)
  push with windows   median t_done of the ticks that complete at least one window
  per window          sum of t_done over those ticks / windows they emitted
  memory              torch.cuda.memory_allocated delta around construction, S opens, one tick and one closing window, per session
Medians over all passes; the spread is the range of the per-pass medians.  No words are pushed (the word path is a few integers per tick).

--input-sr SR (a multiple of 100) runs the pool for audio at another rate instead (synthesize.WideResampledStreamPool,
csrc/stream_pool_wide_rs.hip): a tick is still 10 ms, SR / 100 input samples per session, and three drivers alternate:
  wide_rs  one WideResampledStreamPool(SR) of S slots: one packed upload, one fused resample-and-push launch, then the rounds
  fours_rs S / 4 StreamPool(input_sr=SR) of four slots: per pool an upload, a resample launch and a push launch
  wide16   one WideStreamPool on the same ticks' audio resampled beforehand (160 samples): what the resampler itself costs"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")
syn = pkg.synthesize
V, SR, CHUNK = 20000, 16000, 160
med = statistics.median


class Lang:
    SOS_token, EOS_token = 1, 2

    def get_word_index(self, w):
        return 4 + (sum(map(ord, w)) % (V - 4))


class Wide:
    """S sessions on one WideStreamPool -- or, input_sr: on one WideResampledStreamPool, `chunk` input samples per push."""

    def __init__(self, args, net, n, input_sr=None, chunk=CHUNK):
        if input_sr is None:
            self.pool = syn.WideStreamPool(args, net, Lang(), slots=n, max_chunk=chunk)
        else:
            self.pool = syn.WideResampledStreamPool(args, net, Lang(), input_sr, slots=n, max_chunk=chunk)
        self.n, self.open = n, []

    def join(self):
        self.open.append(self.pool.open(vid=7))

    def tick(self, block):
        self.pool.push({b: block[b] for b in self.open})

    def windows(self):
        return sum(self.pool.next_window)

    def first_window(self):
        self.pool.close(0)


class Fours:
    """S sessions on S / 4 StreamPools of four."""

    def __init__(self, args, net, n, input_sr=None, chunk=CHUNK):
        self.pools = [syn.StreamPool(args, net, Lang(), slots=4, max_chunk=chunk, input_sr=input_sr) for _ in range(n // 4)]
        self.n, self.open = n, []

    def join(self):
        k = len(self.open)
        self.open.append((k // 4, self.pools[k // 4].open(vid=7)))

    def tick(self, block):
        for p, pool in enumerate(self.pools):
            rows = {b: block[4 * p + b] for q, b in self.open[4 * p:4 * p + 4]}
            if rows:
                pool.push(rows)

    def windows(self):
        return sum(sum(pool.next_window) for pool in self.pools)

    def first_window(self):
        for pool in self.pools:
            pool.close(0)


def run_ticks(drv, block, ticks, join_at=()):
    """`ticks` ticks -> per tick (t_call us, t_done us, windows emitted)."""
    out, block = [], getattr(drv, "block", block)                        # (--input-sr: every driver brings the block of its own rate)
    for t in range(ticks):
        for _ in range(join_at.count(t) if join_at else 0):
            drv.join()
        before = drv.windows()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        drv.tick(block)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        out.append(((t1 - t0) * 1e6, (t2 - t0) * 1e6, drv.windows() - before))
    return out


def allocated(make):
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    keep = make()
    torch.cuda.synchronize()
    return (torch.cuda.memory_allocated() - m0) / 2 ** 20, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[4, 32, 128])
    ap.add_argument("--strides", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--input-sr", type=int, default=None)
    a = ap.parse_args()
    if a.input_sr is not None and (a.input_sr % 100 or a.input_sr == SR):
        raise SystemExit("--input-sr: a multiple of 100 other than 16000")
    if not torch.cuda.is_available():
        raise SystemExit("wide_pool_bench needs a GPU")
    if any(n % 4 or not 4 <= n <= 128 for n in a.sessions):
        raise SystemExit("--sessions: multiples of 4 from 4 to 128")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = importlib.import_module(pkg.__name__ + ".config")
    args = cfg.load_config("multimodal_context")
    args.motion_resampling_framerate = 15
    G = pkg.PoseGenerator(args, 27, V, 300, None, pkg.Vocab.speakers(1371)).to(dev).eval()
    S, A = syn.stream_geometry(args)
    per_stride = S // CHUNK
    chunk_in = CHUNK if a.input_sr is None else a.input_sr // 100
    lines = [f"tools/wide_pool_bench.py --sessions {' '.join(map(str, a.sessions))} --strides {a.strides} --reps {a.reps}"
             f"{'' if a.input_sr is None else f' --input-sr {a.input_sr}'}: {chunk_in}-sample pushes to every open "
             f"session per tick, {per_stride} ticks per stride, phases spread over a stride; the drivers' passes alternate; host clock, us"]
    # (key, name, driver class, input_sr): the drivers of a run, the first against the others
    if a.input_sr is None:
        kinds = [("wide", "one WideStreamPool({n})", Wide, None), ("fours", "{q} StreamPool(4)", Fours, None)]
    else:
        kinds = [("wide_rs", "one WideResampledStreamPool({n})", Wide, a.input_sr), ("fours_rs", "{q} StreamPool(4, input_sr)", Fours, a.input_sr),
                 ("wide16", "one WideStreamPool({n}), 16 kHz", Wide, None)]
    rng = lambda v: f"{min(v):.0f} .. {max(v):.0f}"
    for n in a.sessions:
        block = (0.1 * np.random.default_rng(n).standard_normal((n, chunk_in))).astype(np.float32)
        block16 = block if a.input_sr is None else np.stack(syn.resample_audio(list(block), a.input_sr))        # (SR / 100 samples -> 160)

        def new(kind, sr):
            drv = kind(args, G, n) if a.input_sr is None else kind(args, G, n, sr, chunk_in if sr else CHUNK)
            drv.block = block if sr or a.input_sr is None else block16
            return drv

        def made(kind, sr):
            drv = new(kind, sr)
            for _ in range(n):
                drv.join()
            drv.tick(drv.block)
            drv.first_window()
            return drv

        for _, _, kind, sr in kinds:                                     # process-wide workspaces are made on first use: charged to nobody
            made(kind, sr)
        mem = {}
        for key, _, kind, sr in kinds:
            mem[key], keep = allocated(lambda: made(kind, sr))
            del keep
        drivers = {key: new(kind, sr) for key, _, kind, sr in kinds}
        join_at = [(i * per_stride) // n for i in range(n)]
        for drv in drivers.values():                                     # the join phase, the first (eager, captured) windows, one more stride
            run_ticks(drv, block, -(-A // CHUNK) + 2 * per_stride, join_at)
        stat = {k: dict(call=[], done=[], per_win=[], all_call=[], all_done=[]) for k in drivers}
        for _ in range(a.reps):
            for key, drv in drivers.items():
                ticks = run_ticks(drv, block, a.strides * per_stride)
                idle, busy = [t for t in ticks if t[2] == 0], [t for t in ticks if t[2] > 0]
                st = stat[key]
                st["call"].append(med(t[0] for t in idle)); st["all_call"] += [t[0] for t in idle]
                st["done"].append(med(t[1] for t in busy)); st["all_done"] += [t[1] for t in busy]
                st["per_win"].append(sum(t[1] for t in busy) / sum(t[2] for t in busy))
                st["shape"] = (len(idle), len(busy), sum(t[2] for t in busy))
        lines.append(f"S = {n} sessions:")
        for key, name, _, _ in kinds:
            st, name = stat[key], name.format(n=n, q=n // 4)
            lines.append(f"  {name:{24 if a.input_sr is None else 36}s} push, no window {med(st['all_call']):8.1f} us (per pass {rng(st['call'])});  push with windows, to completion "
                         f"{med(st['all_done']):8.1f} us ({rng(st['done'])});  per emitted window {med(st['per_win']):8.1f} us ({rng(st['per_win'])});  "
                         f"memory {mem[key]:8.2f} MiB = {mem[key] / n:6.2f} per session;  "
                         f"per pass {st['shape'][0]} ticks without and {st['shape'][1]} with windows, {st['shape'][2]} windows")
        w = stat[kinds[0][0]]
        for key, _, _, _ in kinds[1:]:
            f = stat[key]
            lines.append(f"  {kinds[0][0]} / {key}: push, no window {med(w['all_call']) / med(f['all_call']):.3f};  push with windows "
                         f"{med(w['all_done']) / med(f['all_done']):.3f};  per emitted window {med(w['per_win']) / med(f['per_win']):.3f}")
        print("\n".join(lines[-2 * len(kinds):]), flush=True)
        del drivers
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
