"""Wall-clock timing of the preprocessing stage -> profiles/preprocess_bench.txt: preprocess.DataPreprocessor.run (device path: packing,
copies, four launches per batch, read-back, compaction) against DataPreprocessor.run_numpy (the module's numpy restatement of the same
steps on the host's CPU share) on generated clips, by default 64 clips of 60 s at 25 -> 15 fps with their spectrograms given.
Per path: one warm-up run (code-object load, allocator), then `--reps` timed runs, each ending in a device synchronise; median and
minimum, the ratio of the medians, and the share of the device path spent in host work (planning, table building, packing, compaction:
DataPreprocessor.host_seconds).  Needs a GPU: there is no fallback."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench: needs a GPU")
    from bench import host_cores
    torch.set_num_threads(host_cores(cap=16))
    P = pkg.preprocess
    rs = np.random.RandomState(0)
    base = np.asarray(P.SYNTHETIC_DIRS, dtype=np.float64)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    mean_pose = P.synthetic_pose(base)
    videos = [{"vid": f"v{i // 8}", "clips": [P.synthetic_clip(rs, a.seconds, 25, with_feat=True)]} for i in range(a.clips)]

    def device_run():
        dp = P.DataPreprocessor(34, 10, 15, mean_pose, base)
        t0 = time.perf_counter()
        samples, filtered = dp.run(videos)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, dp.host_seconds, len(samples), sum(filtered.values())

    def numpy_run():
        dp = P.DataPreprocessor(34, 10, 15, mean_pose, base)
        t0 = time.perf_counter()
        samples, filtered = dp.run_numpy(videos)
        return time.perf_counter() - t0, len(samples), sum(filtered.values())

    device_run()
    dev = [device_run() for _ in range(a.reps)]
    numpy_run()
    host = [numpy_run() for _ in range(a.reps)]
    d_med, d_min = statistics.median(r[0] for r in dev), min(r[0] for r in dev)
    h_med, h_min = statistics.median(r[0] for r in host), min(r[0] for r in host)
    share = statistics.median(r[1] / r[0] for r in dev)
    lines = [f"device: {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}; wall clock, each run ends in a device synchronise; "
             f"1 warm-up run, then {a.reps} timed runs per path",
             f"input: {a.clips} clips of {a.seconds:g} s, 25 -> 15 fps, n_poses 34, stride 10, spectrograms given",
             f"device path: {dev[0][2]} samples kept, {dev[0][3]} filtered out; numpy path: {host[0][1]} kept, {host[0][2]} filtered out"
             + ("" if dev[0][2:] == host[0][1:] else "  (DIFFERENT: a statistic of a generated window sits on a threshold)"),
             f"device path (DataPreprocessor.run):       median {d_med * 1e3:9.1f} ms  min {d_min * 1e3:9.1f} ms",
             f"numpy path  (DataPreprocessor.run_numpy): median {h_med * 1e3:9.1f} ms  min {h_min * 1e3:9.1f} ms",
             f"ratio numpy / device (medians): {h_med / d_med:.2f}",
             f"host share of the device path (planning, tables, packing, compaction): {100 * share:.1f} %"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
