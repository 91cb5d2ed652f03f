"""Latencies of streaming synthesis (synthesize.GestureStream, csrc/stream.hip) at B = 1 with 160-sample pushes (10 ms of audio), for the
multimodal and the joint-embedding model at their full sizes, against the window loop of generate_gestures_batch(on_device=True).

    python tools/stream_bench.py [--seconds 20] [--reps 5] [--out profiles/stream.txt]

Per model, measured ALTERNATELY in one process (a streaming pass, then an offline pass, `reps` times, after one warm-up pass of each that also
captures the window graphs):
  push, no window   a push that completes no window: host time of the call (enqueue) and host time to completion (call + synchronize), beside
                    an empty launch (tg_counter_inc) timed the same way
  window latency    HIP events around the push that completes a window: chunk in -> that window's frames ready on the device
  offline window    HIP events around one iteration of the offline loop's body (UtteranceBatch.stage, the decoder's window, the copy into the
                    stacked result), the same statements as generate_gestures_batch(on_device=True), on a kept decoder of the same kind
Windows 0 and 1 (eager first window, graph capture) are left out of both.  Medians over all windows of all passes; the spread is the range of
the per-pass medians."""
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


class Lang:
    SOS_token, EOS_token = 1, 2

    def get_word_index(self, w):
        return 4 + (sum(map(ord, w)) % (V - 4))


def med(x):
    return statistics.median(x)


def stream_pass(make_stream, audio, words):
    """One utterance through a stream -> (enqueue us of window-less pushes, event ms of window-completing pushes from window 2 on)."""
    st = make_stream()
    enq, lat, k = [], [], 0
    for p in range(0, len(audio), CHUNK):
        q = min(p + CHUNK, len(audio))
        w = [x for x in words if p / SR <= x[1] < q / SR] or None
        completes = syn.complete_windows(q, st.S, st.A) > st.next_window
        if completes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.push(audio[p:q], w)
            e1.record()
            torch.cuda.synchronize()
            if st.next_window > 2:
                lat.append(e0.elapsed_time(e1))
        else:
            t0 = time.perf_counter()
            st.push(audio[p:q], w)
            enq.append((time.perf_counter() - t0) * 1e6)
            k += 1
            if k % 64 == 0:
                torch.cuda.synchronize()                               # keeps the queue short: the enqueue time is not the time of a full queue
    st.close()
    torch.cuda.synchronize()
    return enq, lat


def offline_pass(args, lang, dec, run_window, audio, words):
    """The body of the on_device window loop, timed per window -> event ms from window 2 on."""
    ub = syn.UtteranceBatch(args, lang, [audio], [words], dec.dev)
    stride = args.n_poses - args.n_pre_poses
    total = torch.zeros(1, ub.frames(False), dec.D, device=dec.dev)
    dec.seed(None)
    lat = []
    for i in range(ub.max_win):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ub.stage(i, dec.text, dec.audio)
        out = run_window(dec, i)
        total[:, i * stride:i * stride + args.n_poses, :].copy_(out)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            lat.append(e0.elapsed_time(e1))
    return lat


def completion_times(fn, n=200):
    """Host us from the call to its completion on the device, per call."""
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = importlib.import_module(pkg.__name__ + ".config")
    m_args = cfg.load_config("multimodal_context")
    m_args.motion_resampling_framerate = 15
    G = pkg.PoseGenerator(m_args, 27, V, 300, None, pkg.Vocab.speakers(1371)).to(dev).eval()
    j_args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34,
                             z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * 27)
    E = pkg.EmbeddingNet(j_args, 27, 34, V, 300, None, mode="random").to(dev).eval()
    n = int(a.seconds * SR) - 1234                                     # the last window is partly padded
    while not syn.stream_matches_offline(m_args, n):
        n -= 1
    audio = (0.1 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    words = [[f"w{k}", 0.4 * k, 0.4 * k + 0.3] for k in range(int(n / SR / 0.4))]
    lang = Lang()
    lines = [f"tools/stream_bench.py --seconds {a.seconds} --reps {a.reps}: B = 1, {CHUNK}-sample pushes, {n} samples = {syn.num_windows(n / SR)} windows; "
             "streaming and offline passes alternate"]
    cases = (("multimodal", m_args, G, lambda: syn.WindowDecoder(m_args, G, 1, dev, graph=True), dict(vids=[7]),
              lambda d, i: d.window(None, None, torch.tensor([7]) if i == 0 else None, first=(i == 0))),
             ("joint_embedding", j_args, E, lambda: syn.JointEmbedWindowDecoder(j_args, E, 1, dev, graph=True), {},
              lambda d, i: d.window(None, None, first=(i == 0))))
    for tag, args, net, make_dec, kw, run_window in cases:
        s_dec, o_dec = make_dec(), make_dec()
        make_stream = lambda: syn.GestureStream(args, net, lang, max_chunk=CHUNK, window_decoder=s_dec, **kw)
        stream_pass(make_stream, audio, words); offline_pass(args, lang, o_dec, run_window, audio, words)          # warm-up, graph capture
        enq, s_lat, o_lat, s_med, o_med = [], [], [], [], []
        for _ in range(a.reps):
            e, l = stream_pass(make_stream, audio, words)
            enq += e; s_lat += l; s_med.append(med(l))
            l = offline_pass(args, lang, o_dec, run_window, audio, words)
            o_lat += l; o_med.append(med(l))
        st = make_stream()
        chunk = torch.from_numpy(audio[:CHUNK]).to(dev)[None]
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        push_done, empty_done = [], []
        for _ in range(4):                                             # alternating blocks of 50
            push_done += completion_times(lambda: st.push(chunk), 50)
            empty_done += completion_times(lambda: ops.counter_inc(counter), 50)
        t0 = time.perf_counter()
        for _ in range(50):
            ops.counter_inc(counter)
        empty_enq = (time.perf_counter() - t0) / 50 * 1e6
        torch.cuda.synchronize()
        lines += [f"{tag}:",
                  f"  push, no window : enqueue {med(enq):7.1f} us (p90 {np.percentile(enq, 90):7.1f}), to completion {med(push_done):7.1f} us;  "
                  f"empty launch: enqueue {empty_enq:7.1f} us, to completion {med(empty_done):7.1f} us",
                  f"  window latency  : streaming {med(s_lat):7.3f} ms (per-pass medians {min(s_med):.3f} .. {max(s_med):.3f});  offline loop body "
                  f"{med(o_lat):7.3f} ms (per-pass medians {min(o_med):.3f} .. {max(o_med):.3f});  difference {1e3 * (med(s_lat) - med(o_lat)):+.1f} us"]
        print("\n".join(lines[-3:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
