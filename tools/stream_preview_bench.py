"""Cost of GestureStream.preview() (csrc/stream_preview.hip) against the final-window latency of the same stream, full-size
models, B = 1, 160-sample pushes, with and without input_sr=48000.

    python tools/stream_preview_bench.py [--seconds 12] [--reps 3] [--every 20] [--out profiles/stream_preview.txt]

Per model and input rate, after one warm-up pass of each kind (which also captures the graphs), two kinds of passes ALTERNATE in one process:
  preview pass   a stream that calls preview() after every `every`-th window-less push, from window 2 on.  The calls alternate between two
                 measurements: host time of the call alone (perf_counter around it, the queue drained before), and time to completion
                 (the same with a synchronize behind the call).  The window-completing pushes of this pass are timed too (HIP events).
  window pass    the same stream without previews: chunk in -> frames ready of the window-completing pushes, windows 2 and later -- the
                 final-window latency of profiles/stream.txt, re-measured here.
Also timed, in alternating blocks on one stream below its first window: preview(fade_out=True, joints=True) to completion against
preview() to completion.  Medians over all calls of all passes; the spread is the range of the per-pass medians."""
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


def one_pass(st, audio, words, rate, S, A, every):
    """One utterance in 160-sample pushes.  every > 0: preview() after every `every`-th window-less push once two windows have run.  Returns
    (host us of preview calls, completion us of preview calls, event ms of the window-completing pushes from window 2 on)."""
    host, done, lat, k = [], [], [], 0
    for p in range(0, len(audio), CHUNK):
        q = min(p + CHUNK, len(audio))
        w = [x for x in words if p / rate <= x[1] < q / rate]
        before = st.next_window
        ms = timed(lambda: st.push(audio[p:q], w or None))
        if st.next_window > before:
            if st.next_window > 2:
                lat.append(ms)
            continue
        k += 1
        if every and st.next_window >= 2 and k % every == 0:
            t0 = time.perf_counter()
            st.preview()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if (k // every) % 2:
                host.append((t1 - t0) * 1e6)
            else:
                done.append((t2 - t0) * 1e6)
    st.close()
    torch.cuda.synchronize()
    return host, done, lat


def completion_times(fn, n=50):
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
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_preview_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = importlib.import_module(pkg.__name__ + ".config")
    m_args = cfg.load_config("multimodal_context")
    m_args.motion_resampling_framerate = 15
    G = pkg.PoseGenerator(m_args, 27, V, 300, None, pkg.Vocab.speakers(1371)).to(dev).eval()
    j_args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34,
                             z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * 27)
    E = pkg.EmbeddingNet(j_args, 27, 34, V, 300, None, mode="random").to(dev).eval()
    lang = Lang()
    S, A = syn.stream_geometry(m_args)
    lines = [f"tools/stream_preview_bench.py --seconds {a.seconds} --reps {a.reps} --every {a.every}: B = 1, {CHUNK}-sample pushes; preview passes and "
             "window passes alternate"]
    cases = (("multimodal", m_args, G, lambda: syn.WindowDecoder(m_args, G, 1, dev, graph=True), dict(vids=[7])),
             ("joint_embedding", j_args, E, lambda: syn.JointEmbedWindowDecoder(j_args, E, 1, dev, graph=True), {}))
    rng = lambda v: f"{min(v):.3f} .. {max(v):.3f}"
    for tag, args, net, make_dec, kw in cases:
        lines.append(f"{tag}:")
        for rate in (SR, 48000):
            n = int(a.seconds * rate) - 1234 * rate // SR
            audio = (0.1 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
            words = [[f"w{k}", 0.4 * k, 0.4 * k + 0.3] for k in range(int(n / rate / 0.4))]
            dec = make_dec()
            new = lambda: syn.GestureStream(args, net, lang, max_chunk=CHUNK, window_decoder=dec, input_sr=None if rate == SR else rate, **kw)
            one_pass(new(), audio, words, rate, S, A, a.every); one_pass(new(), audio, words, rate, S, A, 0)       # warm-up, graph capture
            host, done, lat_p, lat_w, m_host, m_done, m_p, m_w = [], [], [], [], [], [], [], []
            for _ in range(a.reps):
                h, d, l = one_pass(new(), audio, words, rate, S, A, a.every)
                host += h; done += d; lat_p += l
                m_host.append(med(h)); m_done.append(med(d)); m_p.append(med(l))
                _, _, l = one_pass(new(), audio, words, rate, S, A, 0)
                lat_w += l; m_w.append(med(l))
            st = new()
            for p in range(0, 20 * CHUNK, CHUNK):
                st.push(audio[p:p + CHUNK])
            plain, full = [], []
            for _ in range(4):                                         # alternating blocks of 50
                plain += completion_times(st.preview)
                full += completion_times(lambda: st.preview(fade_out=True, joints=True))
            lines += [f"  {'16 kHz' if rate == SR else 'input_sr=48000'} ({len(audio)} samples, {len(host) + len(done)} previews, {len(lat_w)} windows):",
                      f"    preview(): host time of the call {med(host):7.1f} us (p90 {np.percentile(host, 90):7.1f}; per-pass medians {rng(m_host)});  "
                      f"to completion {med(done) / 1e3:6.3f} ms (per-pass medians {rng([m / 1e3 for m in m_done])})",
                      f"    final window, chunk in -> frames ready: {med(lat_w):6.3f} ms (per-pass medians {rng(m_w)});  in the passes that preview "
                      f"{med(lat_p):6.3f} ms ({rng(m_p)});  preview to completion / final window = {med(done) / 1e3 / med(lat_w):.2f}",
                      f"    below the first window, to completion: preview() {med(plain) / 1e3:6.3f} ms;  preview(fade_out=True, joints=True) "
                      f"{med(full) / 1e3:6.3f} ms"]
            print("\n".join(lines[-4:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
