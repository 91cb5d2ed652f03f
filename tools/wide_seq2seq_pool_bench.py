"""One tick of a serving process on the wide Seq2Seq stream pool (synthesize.WideSeq2SeqStreamPool, csrc/stream_pool_wide_seq.hip) against the
same tick on pools of four (synthesize.Seq2SeqStreamPool), the shipped model size (hidden 200, 2 layers, vocabulary 20 000), ticks of 160
samples (10 ms of audio), and the bare pooled window of the window decoder by row count.  The tick protocol is tools/wide_pool_bench.py's,
whose helpers run here unchanged.

    python tools/wide_seq2seq_pool_bench.py [--sessions 4 32 128] [--strides 2] [--reps 3] [--windows 1 4 32 128] [--out profiles/wide_seq2seq_pool.txt]

S sessions are open; session i joins at tick (i * ticks per stride) // S, so the sessions' windows complete at phases spread over a stride
(200 ticks) and a tick completes windows of few sessions or of none.  A tick advances every open session by 160 samples, two ways:
  wide     one WideSeq2SeqStreamPool of S slots, pushed the sample COUNT: one packed upload of integers, one push launch, then the rounds
  fours    S / 4 Seq2SeqStreamPools of four slots, each on a Seq2SeqWindowDecoder of its own, pushed the 160 samples, driven in turn on one stream
After the join phase and one warm-up stride of each (graph capture), passes of `strides` strides ALTERNATE between the two, `reps` each.
Every tick is timed on the host: t_call = the push calls have returned, t_done = a device synchronise behind them has returned.
  push, no window     median t_call of the ticks that complete no window (what the serving thread pays per 10 ms)
  push with windows   median t_done of the ticks that complete at least one window
  per window          sum of t_done over those ticks / windows they emitted
  memory              torch.cuda.memory_allocated delta around construction, S opens, one tick and one closing window, per session
Medians over all passes; the spread is the range of the per-pass medians.  No words are pushed (every window's list is [SOS, EOS]).

The bare pooled window: window_pooled with every row active on a decoder of B rows (Seq2SeqWindowDecoder up to four rows,
WideSeq2SeqWindowDecoder above), every row a list of 7 ids, one captured graph replayed -- HIP events around each replay, `reps` passes of 20
replays per row count, the row counts' passes alternating.  One workgroup per row decodes; the rows share the weights through L2."""
import argparse
import os
from types import SimpleNamespace

import numpy as np
import torch

from wide_pool_bench import CHUNK, SR, V, Lang, allocated, med, pkg, run_ticks, syn


class Wide:
    """S sessions on one WideSeq2SeqStreamPool, advanced by sample counts."""

    def __init__(self, args, net, n):
        self.pool = syn.WideSeq2SeqStreamPool(args, net, Lang(), slots=n, max_chunk=CHUNK)
        self.n, self.open = n, []

    def join(self):
        self.open.append(self.pool.open())

    def tick(self, block):
        self.pool.push({b: CHUNK for b in self.open})

    def windows(self):
        return sum(self.pool.next_window)

    def first_window(self):
        self.pool.close(0)


class Fours:
    """S sessions on S / 4 Seq2SeqStreamPools of four."""

    def __init__(self, args, net, n):
        self.pools = [syn.Seq2SeqStreamPool(args, net, Lang(), slots=4, max_chunk=CHUNK) for _ in range(n // 4)]
        self.n, self.open = n, []

    def join(self):
        k = len(self.open)
        self.open.append((k // 4, self.pools[k // 4].open()))

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


def bare_windows(args, net, dev, counts, reps, lines):
    """Device time of one pooled window (all rows active, graph replay) by row count; the row counts' passes alternate."""
    decs = {}
    for B in counts:
        kind = syn.Seq2SeqWindowDecoder if B <= 4 else syn.WideSeq2SeqWindowDecoder
        dec = kind(args, net, B, dev, graph=True)
        ids = torch.randint(4, V, (B, 5), generator=torch.Generator().manual_seed(B))
        text = torch.zeros(B, dec.Te, dtype=torch.int64)
        text[:, 0], text[:, 1:6], text[:, 6] = 1, ids, 2
        dec.text.copy_(text); dec.len.fill_(7)
        dec.pool_buffers()
        for _ in range(3):                                                # the eager pass, the capture, a replay
            dec.window_pooled(active=[1] * B)
        decs[B] = dec
    torch.cuda.synchronize()
    times = {B: [] for B in counts}
    per_pass = {B: [] for B in counts}
    for _ in range(reps):
        for B, dec in decs.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
            for e0, e1 in evs:
                e0.record()
                dec.window_pooled()
                e1.record()
            torch.cuda.synchronize()
            ms = [e0.elapsed_time(e1) for e0, e1 in evs]
            times[B] += ms
            per_pass[B].append(med(ms))
    one = med(times[counts[0]])
    lines.append(f"bare pooled window (graph replay, every row active, 7-id lists), device time by HIP events, {reps} x 20 replays per row count:")
    for B in counts:
        t = med(times[B])
        lines.append(f"  B = {B:3d}: {t:7.3f} ms (per-pass medians {min(per_pass[B]):.3f} .. {max(per_pass[B]):.3f}, fastest {min(times[B]):.3f});  "
                     f"{t / one:5.2f} x the B = {counts[0]} window;  {1e3 * t / B:8.1f} us per row")
    print("\n".join(lines[-len(counts) - 1:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="*", default=[4, 32, 128])
    ap.add_argument("--windows", type=int, nargs="*", default=[1, 4, 32, 128])
    ap.add_argument("--strides", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_seq2seq_pool_bench needs a GPU")
    if any(n % 4 or not 4 <= n <= 128 for n in a.sessions):
        raise SystemExit("--sessions: multiples of 4 from 4 to 128")
    if any(not 1 <= n <= 128 for n in a.windows):
        raise SystemExit("--windows: row counts from 1 to 128")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    args = SimpleNamespace(model="seq2seq", hidden_size=200, n_layers=2, dropout_prob=0.0, n_pre_poses=4, n_poses=34, GAN_noise_size=0,
                           motion_resampling_framerate=15, z_type="none", mean_dir_vec=[0.0] * 27)
    net = pkg.Seq2SeqNet(args, 27, 34, V, 300, None).to(dev).eval()
    S, A = syn.stream_geometry(args)
    per_stride = S // CHUNK
    lines = [f"tools/wide_seq2seq_pool_bench.py --sessions {' '.join(map(str, a.sessions))} --strides {a.strides} --reps {a.reps} --windows "
             f"{' '.join(map(str, a.windows))}: {CHUNK}-sample ticks to every open session, {per_stride} ticks per stride, phases spread over a stride; "
             "the drivers' passes alternate; host clock, us"]
    kinds = [("wide", "one WideSeq2SeqStreamPool({n})", Wide), ("fours", "{q} Seq2SeqStreamPool(4)", Fours)]
    rng = lambda v: f"{min(v):.0f} .. {max(v):.0f}"
    for n in a.sessions:
        block = (0.1 * np.random.default_rng(n).standard_normal((n, CHUNK))).astype(np.float32)

        def made(kind):
            drv = kind(args, net, n)
            for _ in range(n):
                drv.join()
            drv.tick(block)
            drv.first_window()
            return drv

        for _, _, kind in kinds:                                         # process-wide workspaces are made on first use: charged to nobody
            made(kind)
        mem = {}
        for key, _, kind in kinds:
            mem[key], keep = allocated(lambda: made(kind))
            del keep
        drivers = {key: kind(args, net, n) for key, _, kind in kinds}
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
        for key, name, _ in kinds:
            st, name = stat[key], name.format(n=n, q=n // 4)
            lines.append(f"  {name:32s} push, no window {med(st['all_call']):8.1f} us (per pass {rng(st['call'])});  push with windows, to completion "
                         f"{med(st['all_done']):8.1f} us ({rng(st['done'])});  per emitted window {med(st['per_win']):8.1f} us ({rng(st['per_win'])});  "
                         f"memory {mem[key]:8.2f} MiB = {mem[key] / n:6.2f} per session;  "
                         f"per pass {st['shape'][0]} ticks without and {st['shape'][1]} with windows, {st['shape'][2]} windows")
        w, f = stat["wide"], stat["fours"]
        lines.append(f"  wide / fours: push, no window {med(w['all_call']) / med(f['all_call']):.3f};  push with windows "
                     f"{med(w['all_done']) / med(f['all_done']):.3f};  per emitted window {med(w['per_win']) / med(f['per_win']):.3f}")
        print("\n".join(lines[-4:]), flush=True)
        del drivers
        torch.cuda.empty_cache()
    if a.windows:
        bare_windows(args, net, dev, a.windows, a.reps, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
