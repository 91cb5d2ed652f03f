"""HIP-event timing of the log-mel spectrogram (csrc/logmel.hip: two launches per call) -> profiles/logmel_bench.txt.
Cases: one 10 s utterance (N = 1, L = 160 000: synthesis) and a preprocessing batch (N = 256, L = 36 267: the clips of one training batch).
Per case: 20 warm-up calls, then 200 timed calls, each between its own pair of events on the stream (median and minimum reported), and the
same loop around an 4-byte launch of the library (tg_zero) as the launch-latency floor of this machine."""
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")


def timed(fn, warmup=20, reps=200):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(us), us[0]


def main():
    dev = torch.device("cuda:0")
    ops, ms = pkg.ops, pkg.melspec
    lines = [f"device: {torch.cuda.get_device_name(0)}; times in microseconds between HIP events, median / minimum of 200 calls after 20 warm-up calls"]
    word = torch.zeros(4, device=dev)
    med, mn = timed(lambda: ops.zero_(word[:1]))
    lines.append(f"launch floor (one 4-byte tg_zero launch): median {med:.1f} min {mn:.1f}")
    tables = ms.device_tables(dev)
    for N, L in ((1, 160000), (256, 36267)):
        audio = torch.randn(N, L, device=dev) * 0.1
        F, _, ws_bytes = ops.logmel_query(N, L)
        ws = torch.empty(ws_bytes // 4, device=dev)
        for dt in (torch.float16, torch.float32):
            out = torch.empty(N, 128, F, device=dev, dtype=dt)
            for mode in ("reflect", "constant"):
                med, mn = timed(lambda: ops.logmel(audio, out, ws, pad_mode=mode, tables=tables))
                gb = (audio.numel() * 4 + out.numel() * out.element_size()) / 1e9
                lines.append(f"N {N:4d} L {L:6d} F {F:4d} {str(dt)[6:]:8s} {mode:8s}: median {med:8.1f} min {mn:8.1f}  "
                             f"({N * F / mn:.2f} frames/us, {gb / (mn * 1e-6):.0f} GB/s of audio read + spectrogram written at the minimum)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "logmel_bench.txt"), "w") as f:
        f.write(text)

if __name__ == "__main__":
    main()
