"""Latencies and memory of the stream pool (synthesize.StreamPool, csrc/stream_pool.hip) against synthesize.GestureStream, full-size models,
160-sample pushes (10 ms of audio), HIP events.

    python tools/stream_pool_bench.py [--seconds 12] [--reps 3] [--out profiles/stream_pool.txt]

Per model, pool and yardstick passes ALTERNATE in one process after one warm-up pass of each (which also captures the graphs):
  one session      chunk in -> frames ready (events around the push that completes a window, windows 2 and later) for one open session of a
                   capacity-4 pool, against (a) GestureStream(batch=1) and (b) GestureStream(batch=4)
  four sessions    four sessions offset by S / 4 on one pool against four GestureStream(batch=1) on four decoders: device time of the
                   window-completing pushes, summed, per emitted window
  memory           torch.cuda.memory_allocated deltas around construction + first window (FrozenWeights operands included): a pool of 4 against
                   four one-row streams with a decoder each, after one throw-away run of both (process-wide workspaces exist by then)
  push, no window  host time of the call and host time to completion of a push that completes no window
Medians over all windows of all passes; the spread is the range of the per-pass medians."""
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
syn, ops = pkg.synthesize, pkg.ops
V, SR, CHUNK = 20000, 16000, 160
med = statistics.median


class Lang:
    SOS_token, EOS_token = 1, 2

    def get_word_index(self, w):
        return 4 + (sum(map(ord, w)) % (V - 4))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def words_of(words, p, q):
    return [x for x in words if p / SR <= x[1] < q / SR]


def one_session(push, next_window, close, audio, words, S, A):
    """One utterance in 160-sample pushes -> (host us of the window-less pushes, event ms of the window-completing ones from window 2 on)."""
    enq, lat, k = [], [], 0
    for p in range(0, len(audio), CHUNK):
        q = min(p + CHUNK, len(audio))
        w = words_of(words, p, q)
        if syn.complete_windows(q, S, A) > next_window():
            ms = timed(lambda: push(audio[p:q], w))
            if next_window() > 2:
                lat.append(ms)
        else:
            t0 = time.perf_counter()
            push(audio[p:q], w)
            enq.append((time.perf_counter() - t0) * 1e6)
            k += 1
            if k % 64 == 0:
                torch.cuda.synchronize()                               # keeps the queue short
    close()
    torch.cuda.synchronize()
    return enq, lat


def four_sessions(push_tick, close, audio, S, A):
    """Four sessions of the same audio, session i joining at sample i * S / 4.  push_tick({i: chunk}) pushes one tick of the running sessions.
    Returns (summed event ms of the ticks that completed a window, windows completed), first two windows of every session left out."""
    n_ticks, off = -(-len(audio) // CHUNK), S // 4 // CHUNK
    total, windows, done = 0.0, 0, [0] * 4
    for t in range(n_ticks + 3 * off):
        tick, completes = {}, 0
        for i in range(4):
            k = t - i * off
            if 0 <= k < n_ticks:
                tick[i] = audio[k * CHUNK:(k + 1) * CHUNK]
                now = syn.complete_windows(min((k + 1) * CHUNK, len(audio)), S, A)
                completes += (now > done[i]) and now > 2
                done[i] = now
        if completes:
            total += timed(lambda: push_tick(tick))
            windows += completes
        else:
            push_tick(tick)
        for i in range(4):
            if t - i * off == n_ticks - 1:
                close(i)
    torch.cuda.synchronize()
    return total, windows


def completion_times(fn, n=50):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def allocated(make_and_run):
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    keep = make_and_run()
    torch.cuda.synchronize()
    return (torch.cuda.memory_allocated() - m0) / 2 ** 20, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_pool_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = importlib.import_module(pkg.__name__ + ".config")
    m_args = cfg.load_config("multimodal_context")
    m_args.motion_resampling_framerate = 15
    G = pkg.PoseGenerator(m_args, 27, V, 300, None, pkg.Vocab.speakers(1371)).to(dev).eval()
    j_args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34,
                             z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * 27)
    E = pkg.EmbeddingNet(j_args, 27, 34, V, 300, None, mode="random").to(dev).eval()
    n = int(a.seconds * SR) - 1234
    audio = (0.1 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    words = [[f"w{k}", 0.4 * k, 0.4 * k + 0.3] for k in range(int(n / SR / 0.4))]
    lang = Lang()
    S, A = syn.stream_geometry(m_args)
    lines = [f"tools/stream_pool_bench.py --seconds {a.seconds} --reps {a.reps}: {CHUNK}-sample pushes, {n} samples = {syn.num_windows(n / SR)} windows per "
             "session; pool and yardstick passes alternate"]
    cases = (("multimodal", m_args, G, lambda B: syn.WindowDecoder(m_args, G, B, dev, graph=True), lambda B: dict(vids=[7] * B)),
             ("joint_embedding", j_args, E, lambda B: syn.JointEmbedWindowDecoder(j_args, E, B, dev, graph=True), lambda B: {}))
    for tag, args, net, make_dec, kw in cases:
        # ---- memory first, on a quiet allocator: a pool of 4 against four one-row streams, construction + first window
        def pool_of_4():
            pool = syn.StreamPool(args, net, lang, slots=4, max_chunk=CHUNK)
            for _ in range(4):
                pool.open(vid=7)
            pool.push({0: audio[:CHUNK]})
            pool.close(0)
            return pool

        def four_streams():
            sts = [syn.GestureStream(args, net, lang, max_chunk=CHUNK, **kw(1)) for _ in range(4)]
            for st in sts:
                st.push(audio[:CHUNK])
                st.close()
            return sts

        pool_of_4(); four_streams()                                     # process-wide workspaces are made on first use: not charged to either
        torch.cuda.synchronize()
        mem_pool, keep_p = allocated(pool_of_4)
        mem_four, keep_s = allocated(four_streams)
        del keep_p, keep_s
        # ---- one session on a pool of 4 against GestureStream(batch=1) and GestureStream(batch=4)
        p_dec, d1, d4, four_dec = make_dec(4), make_dec(1), make_dec(4), [make_dec(1) for _ in range(4)]

        def pool_pass():
            pool = syn.StreamPool(args, net, lang, slots=4, max_chunk=CHUNK, window_decoder=p_dec)
            b = pool.open(vid=7)
            return one_session(lambda c, w: pool.push({b: (c, w)}), lambda: pool.next_window[b], lambda: pool.close(b), audio, words, S, A)

        def stream_pass(dec, B):
            st = syn.GestureStream(args, net, lang, batch=B, max_chunk=CHUNK, window_decoder=dec, **kw(B))
            rep = (lambda c: c) if B == 1 else (lambda c: np.ascontiguousarray(np.broadcast_to(c, (B, len(c)))))
            return one_session(lambda c, w: st.push(rep(c), [w] * B if w else None), lambda: st.next_window, st.close, audio, words, S, A)

        def pool_four():
            pool = syn.StreamPool(args, net, lang, slots=4, max_chunk=CHUNK, window_decoder=p_dec)
            slot = {}

            def tick(chunks):
                for i in chunks:
                    if i not in slot:
                        slot[i] = pool.open(vid=7)
                pool.push({slot[i]: c for i, c in chunks.items()})
            return four_sessions(tick, lambda i: pool.close(slot[i]), audio, S, A)

        def streams_four():
            sts = {}

            def tick(chunks):
                for i, c in chunks.items():
                    if i not in sts:
                        sts[i] = syn.GestureStream(args, net, lang, max_chunk=CHUNK, window_decoder=four_dec[i], **kw(1))
                    sts[i].push(c)
            return four_sessions(tick, lambda i: sts[i].close(), audio, S, A)

        pool_pass(); stream_pass(d1, 1); stream_pass(d4, 4); pool_four(); streams_four()                   # warm-up, graph capture
        enq_p, enq_s, lat = [], [], {"pool": [], "b1": [], "b4": []}
        meds = {"pool": [], "b1": [], "b4": []}
        four = {"pool": [], "streams": []}
        for _ in range(a.reps):
            for key, run in (("pool", pool_pass), ("b1", lambda: stream_pass(d1, 1)), ("b4", lambda: stream_pass(d4, 4))):
                e, l = run()
                lat[key] += l; meds[key].append(med(l))
                if key == "pool":
                    enq_p += e
                elif key == "b1":
                    enq_s += e
            for key, run in (("pool", pool_four), ("streams", streams_four)):
                ms, wins = run()
                four[key].append(ms / wins)
        pool = syn.StreamPool(args, net, lang, slots=4, max_chunk=CHUNK, window_decoder=p_dec)
        b = pool.open(vid=7)
        st = syn.GestureStream(args, net, lang, max_chunk=CHUNK, window_decoder=d1, **kw(1))
        done_p, done_s = [], []
        for _ in range(4):                                             # alternating blocks of 50, all below one window (32 000 samples in all)
            done_p += completion_times(lambda: pool.push({b: audio[:CHUNK]}))
            done_s += completion_times(lambda: st.push(audio[:CHUNK]))
        rng = lambda v: f"{min(v):.3f} .. {max(v):.3f}"
        lines += [f"{tag}:",
                  f"  one session, chunk in -> frames ready: pool of 4, one row open {med(lat['pool']):7.3f} ms (per-pass medians {rng(meds['pool'])});  "
                  f"GestureStream(batch=1) {med(lat['b1']):7.3f} ms ({rng(meds['b1'])});  GestureStream(batch=4) {med(lat['b4']):7.3f} ms ({rng(meds['b4'])});  "
                  f"pool / batch=1 = {med(lat['pool']) / med(lat['b1']):.3f}, pool / batch=4 = {med(lat['pool']) / med(lat['b4']):.3f}",
                  f"  four sessions offset by S/4, device time per emitted window: one pool {med(four['pool']):7.3f} ms (per pass {rng(four['pool'])});  "
                  f"four GestureStream(batch=1) on four decoders {med(four['streams']):7.3f} ms ({rng(four['streams'])})",
                  f"  device memory, construction + first window: pool of 4 {mem_pool:8.2f} MiB = {mem_pool / 4:.2f} per session;  four one-row streams "
                  f"{mem_four:8.2f} MiB = {mem_four / 4:.2f} per session",
                  f"  push, no window: pool enqueue {med(enq_p):6.1f} us (p90 {np.percentile(enq_p, 90):6.1f}), to completion {med(done_p):6.1f} us;  "
                  f"GestureStream(batch=1) enqueue {med(enq_s):6.1f} us (p90 {np.percentile(enq_s, 90):6.1f}), to completion {med(done_s):6.1f} us"]
        print("\n".join(lines[-5:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
