"""Latencies and memory of the Seq2Seq stream pool (synthesize.Seq2SeqStreamPool, csrc/stream_pool_seq.hip) against
synthesize.Seq2SeqGestureStream, the shipped model size (hidden 200, 2 layers, vocabulary 20 000), 160-sample pushes (10 ms of audio), HIP
events.  The passes and their rules are tools/stream_pool_bench.py's, whose helpers run here unchanged.

    python tools/seq2seq_pool_bench.py [--seconds 12] [--reps 3] [--out profiles/seq2seq_pool.txt]

Pool and yardstick passes ALTERNATE in one process after one warm-up pass of each (which also captures the graphs):
  one session      chunk in -> frames ready (events around the push that completes a window, windows 2 and later) for one open session of a
                   capacity-4 pool, against Seq2SeqGestureStream(batch=1)
  four in step     the same push with all four slots of the pool open on one clock (one round of four active rows), against
                   Seq2SeqGestureStream(batch=4)
  four sessions    four sessions offset by S / 4 on one pool against four Seq2SeqGestureStream(batch=1) on four decoders: device time of the
                   window-completing pushes, summed, per emitted window
  memory           torch.cuda.memory_allocated deltas around construction + first window (FrozenWeights operands included): a pool of 4 against
                   four one-row streams with a decoder each, after one throw-away run of both (process-wide workspaces exist by then)
  push, no window  host time of the call and host time to completion of a push that completes no window
Medians over all windows of all passes; the spread is the range of the per-pass medians."""
import argparse
from types import SimpleNamespace

import numpy as np
import torch

from stream_pool_bench import CHUNK, SR, V, Lang, allocated, completion_times, four_sessions, med, one_session, pkg, syn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq2seq_pool_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    args = SimpleNamespace(model="seq2seq", hidden_size=200, n_layers=2, dropout_prob=0.0, n_pre_poses=4, n_poses=34, GAN_noise_size=0,
                           motion_resampling_framerate=15, z_type="none", mean_dir_vec=[0.0] * 27)
    net = pkg.Seq2SeqNet(args, 27, 34, V, 300, None).to(dev).eval()
    lang = Lang()
    n = int(a.seconds * SR) - 1234
    audio = (0.1 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    words = [[f"w{k}", 0.4 * k, 0.4 * k + 0.3] for k in range(int(n / SR / 0.4))]
    S, A = syn.stream_geometry(args)
    lines = [f"tools/seq2seq_pool_bench.py --seconds {a.seconds} --reps {a.reps}: {CHUNK}-sample pushes, {n} samples = {syn.num_windows(n / SR)} windows per "
             "session; pool and yardstick passes alternate"]
    make_dec = lambda B: syn.Seq2SeqWindowDecoder(args, net, B, dev, graph=True)

    # ---- memory first, on a quiet allocator: a pool of 4 against four one-row streams, construction + first window
    def pool_of_4():
        pool = syn.Seq2SeqStreamPool(args, net, lang, slots=4, max_chunk=CHUNK)
        for _ in range(4):
            pool.open()
        pool.push({0: audio[:CHUNK]})
        pool.close(0)
        return pool

    def four_streams():
        sts = [syn.Seq2SeqGestureStream(args, net, lang, max_chunk=CHUNK) for _ in range(4)]
        for st in sts:
            st.push(audio[:CHUNK])
            st.close()
        return sts

    pool_of_4(); four_streams()                                         # process-wide workspaces are made on first use: not charged to either
    torch.cuda.synchronize()
    mem_pool, keep_p = allocated(pool_of_4)
    mem_four, keep_s = allocated(four_streams)
    del keep_p, keep_s
    p_dec, d1, d4, four_dec = make_dec(4), make_dec(1), make_dec(4), [make_dec(1) for _ in range(4)]

    def pool_pass(rows):
        """`rows` slots open on one clock; the events are around the push of all of them."""
        pool = syn.Seq2SeqStreamPool(args, net, lang, slots=4, max_chunk=CHUNK, window_decoder=p_dec)
        slots = [pool.open() for _ in range(rows)]
        return one_session(lambda c, w: pool.push({b: (c, w) for b in slots}), lambda: pool.next_window[slots[0]],
                           lambda: [pool.close(b) for b in slots], audio, words, S, A)

    def stream_pass(dec, B):
        st = syn.Seq2SeqGestureStream(args, net, lang, batch=B, max_chunk=CHUNK, window_decoder=dec)
        rep = (lambda c: c) if B == 1 else (lambda c: np.ascontiguousarray(np.broadcast_to(c, (B, len(c)))))
        return one_session(lambda c, w: st.push(rep(c), [w] * B if w else None), lambda: st.next_window, st.close, audio, words, S, A)

    def pool_four():
        pool = syn.Seq2SeqStreamPool(args, net, lang, slots=4, max_chunk=CHUNK, window_decoder=p_dec)
        slot = {}

        def tick(chunks):
            for i in chunks:
                if i not in slot:
                    slot[i] = pool.open()
            pool.push({slot[i]: c for i, c in chunks.items()})
        return four_sessions(tick, lambda i: pool.close(slot[i]), audio, S, A)

    def streams_four():
        sts = {}

        def tick(chunks):
            for i, c in chunks.items():
                if i not in sts:
                    sts[i] = syn.Seq2SeqGestureStream(args, net, lang, max_chunk=CHUNK, window_decoder=four_dec[i])
                sts[i].push(c)
        return four_sessions(tick, lambda i: sts[i].close(), audio, S, A)

    runs = (("pool1", lambda: pool_pass(1)), ("pool4", lambda: pool_pass(4)), ("b1", lambda: stream_pass(d1, 1)), ("b4", lambda: stream_pass(d4, 4)))
    for _, run in runs:                                                 # warm-up, graph capture
        run()
    pool_four(); streams_four()
    enq = {k: [] for k, _ in runs}
    lat = {k: [] for k, _ in runs}
    meds = {k: [] for k, _ in runs}
    four = {"pool": [], "streams": []}
    for _ in range(a.reps):
        for key, run in runs:
            e, l = run()
            enq[key] += e; lat[key] += l; meds[key].append(med(l))
        for key, run in (("pool", pool_four), ("streams", streams_four)):
            ms, wins = run()
            four[key].append(ms / wins)
    pool = syn.Seq2SeqStreamPool(args, net, lang, slots=4, max_chunk=CHUNK, window_decoder=p_dec)
    b = pool.open()
    st = syn.Seq2SeqGestureStream(args, net, lang, max_chunk=CHUNK, window_decoder=d1)
    done_p, done_s = [], []
    for _ in range(4):                                                  # alternating blocks of 50, all below one window (32 000 samples in all)
        done_p += completion_times(lambda: pool.push({b: audio[:CHUNK]}))
        done_s += completion_times(lambda: st.push(audio[:CHUNK]))
    rng = lambda v: f"{min(v):.3f} .. {max(v):.3f}"
    m = {k: med(v) for k, v in lat.items()}
    lines += ["seq2seq (hidden 200, 2 layers, max_words 32, one-launch encoder):",
              f"  one session, chunk in -> frames ready: pool of 4, one row open {m['pool1']:7.3f} ms (per-pass medians {rng(meds['pool1'])});  "
              f"Seq2SeqGestureStream(batch=1) {m['b1']:7.3f} ms ({rng(meds['b1'])});  pool / batch=1 = {m['pool1'] / m['b1']:.3f}",
              f"  four sessions in step, chunk in -> frames ready: pool of 4, four rows open {m['pool4']:7.3f} ms ({rng(meds['pool4'])});  "
              f"Seq2SeqGestureStream(batch=4) {m['b4']:7.3f} ms ({rng(meds['b4'])});  pool / batch=4 = {m['pool4'] / m['b4']:.3f};  "
              f"per session {m['pool4'] / 4:.3f} ms",
              f"  four sessions offset by S/4, device time per emitted window: one pool {med(four['pool']):7.3f} ms (per pass {rng(four['pool'])});  "
              f"four Seq2SeqGestureStream(batch=1) on four decoders {med(four['streams']):7.3f} ms ({rng(four['streams'])})",
              f"  device memory, construction + first window: pool of 4 {mem_pool:8.2f} MiB = {mem_pool / 4:.2f} per session;  four one-row streams "
              f"{mem_four:8.2f} MiB = {mem_four / 4:.2f} per session",
              f"  push, no window: pool enqueue {med(enq['pool1']):6.1f} us (p90 {np.percentile(enq['pool1'], 90):6.1f}), to completion {med(done_p):6.1f} us;  "
              f"Seq2SeqGestureStream(batch=1) enqueue {med(enq['b1']):6.1f} us (p90 {np.percentile(enq['b1'], 90):6.1f}), to completion {med(done_s):6.1f} us"]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
