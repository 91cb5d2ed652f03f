"""What resampling to 16 kHz on the device costs (synthesize.resample_audio, GestureStream(input_sr=...), csrc/resample.hip).

    python tools/resample_bench.py [--reps 400] [--out profiles/resample.txt]

  push, no window   a GestureStream push that completes no window, host time of the call (enqueue) and host time to completion (call +
                    synchronize): 480 samples at 48 kHz (input_sr=48000: upload to the staging buffer, tg_resample_stream, tg_stream_push)
                    against the same 10 ms of audio as 160 samples at 16 kHz (the path as it was: upload, tg_stream_push), on the same box, in
                    alternating blocks, on the joint-embedding model's stream (the window decoder is idle in these pushes)
  offline           resample_audio of a 60 s utterance at 48 and 44.1 kHz (one upload, one tg_resample launch, no read-back): HIP events
                    around the call, and around the launch alone with the audio already on the device, with the bytes it moves
Medians; nothing here is a promise, the numbers are recorded as measured."""
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
V = 20000


class Lang:
    SOS_token, EOS_token = 1, 2

    def get_word_index(self, w):
        return 4 + (sum(map(ord, w)) % (V - 4))


def med(x):
    return statistics.median(x)


def push_times(st, chunk, n):
    """(enqueue us, to-completion us) of n window-less pushes each."""
    enq, done = [], []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.push(chunk)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        enq.append((t1 - t0) * 1e6); done.append((time.perf_counter() - t0) * 1e6)
    return enq, done


def event_ms(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    args = SimpleNamespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34,
                           z_type="none", motion_resampling_framerate=15, wordembed_dim=300, mean_dir_vec=[0.0] * 27)
    net = pkg.EmbeddingNet(args, 27, 34, V, 300, None, mode="random").to(dev).eval()
    rng = np.random.default_rng(1)
    lines = [f"tools/resample_bench.py --reps {a.reps}"]
    # ---- the push
    block = 50
    streams = {16000: syn.GestureStream(args, net, Lang(), max_chunk=160, graph=False),
               48000: syn.GestureStream(args, net, Lang(), max_chunk=480, graph=False, input_sr=48000)}
    chunks = {sr: (0.1 * rng.standard_normal(sr // 100)).astype(np.float32) for sr in streams}
    res = {sr: ([], []) for sr in streams}
    for sr, st in streams.items():
        push_times(st, chunks[sr], 20)                                  # warm-up (far fewer samples than a window: no push completes one)
    for _ in range(max(1, a.reps // block)):
        for sr, st in streams.items():
            if st.pushed + (block + 1) * 160 >= st.A:                   # stay below the first window: a fresh stream
                st = streams[sr] = syn.GestureStream(args, net, Lang(), max_chunk=sr // 100, graph=False, input_sr=None if sr == 16000 else sr)
            e, d = push_times(st, chunks[sr], block)
            res[sr][0].extend(e); res[sr][1].extend(d)
    for sr in streams:
        e, d = res[sr]
        lines.append(f"push, no window, {sr // 100:3d} samples at {sr} Hz: enqueue {med(e):7.1f} us (p90 {np.percentile(e, 90):7.1f}), to completion "
                     f"{med(d):7.1f} us (p90 {np.percentile(d, 90):7.1f}), {len(e)} pushes")
    lines.append(f"  difference 48 kHz - 16 kHz: enqueue {med(res[48000][0]) - med(res[16000][0]):+.1f} us, to completion "
                 f"{med(res[48000][1]) - med(res[16000][1]):+.1f} us")
    print("\n".join(lines), flush=True)
    # ---- offline, 60 s
    for sr in (48000, 44100):
        x = (0.1 * rng.standard_normal(60 * sr)).astype(np.float32)
        taps, L, M, K = pkg.resample.device_taps(sr, dev)
        xd = torch.from_numpy(x).to(dev)
        syn.resample_audio(x, sr, device=dev, return_device=True); ops.resample(xd, [len(x)], taps, L, M, K)          # warm-up
        whole = event_ms(lambda: syn.resample_audio(x, sr, device=dev, return_device=True), 20)
        launch = event_ms(lambda: ops.resample(xd, [len(x)], taps, L, M, K), 50)
        n_out = syn.resampled_length(len(x), L, M)
        mb = 4e-6 * (len(x) + n_out)
        lines.append(f"offline, 60 s at {sr} Hz ({len(x)} -> {n_out} samples, L/M = {L}/{M}, K = {K}): resample_audio from host memory "
                     f"{med(whole):.3f} ms; ops.resample on device audio (offset upload, output allocation, tg_resample) {med(launch):.3f} ms = "
                     f"{mb / med(launch):.1f} GB/s of the {mb:.1f} MB it must move, {2e-6 * K * n_out / med(launch):.1f} GFLOP/s")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
