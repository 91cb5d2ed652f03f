"""Timing of the Human3.6M feed -> one JSON line (and --out: profiles/h36m_feed.txt): samples/s of stage A + stage B on the device
(h36m.Human36M: ops.h36m_normalize over every frame, then one ops.h36m_samples launch over every window) with augment off and on, against
the module's numpy restatement of the same two stages on the host's CPU share; the time of ONE augmented stage-B launch for a batch of 128
against the fused autoencoder step that consumes it (fgd.AutoencoderTrainer.train_iter, B = 128), both measured in this run; and the time
of one epoch of fgd.train_autoencoder fed by the device path and fed by the numpy restatement.
Device times are HIP event times around the launches alone: one warm-up (code-object load, allocator), then `--blocks` blocks of `--reps`
back-to-back repetitions, the median over the blocks of the per-repetition time.  Host and epoch times are wall clock, ending in a device
synchronise.  Generated positions stand in for the dataset.  Needs a GPU: there is no fallback."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("gesture-generation-from-trimodal-context_amd")


def event_time(fn, blocks, reps):
    """Median over `blocks` of the mean time (s) of `reps` back-to-back calls, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / reps)
    return statistics.median(out)


class NumpyFeed:
    """The `batches` side of h36m.Human36M served by the numpy restatement: normalised once on the host, every batch built by
    samples_numpy and copied to the device (what a host loader does)."""

    def __init__(self, data, mean, is_train, device):
        H = pkg.h36m
        self.actions, self.win, arrays = H.window_table(data, is_train)
        self.skel = np.concatenate([H.normalize_numpy(a) for a in arrays])
        self.mean, self.device, self.rs = mean, device, np.random.RandomState(0)

    def __len__(self):
        return len(self.win)

    def n_batches(self, b, drop_last=True):
        return len(self) // b if drop_last else -(-len(self) // b)

    def batches(self, b, shuffle, drop_last=True):
        order = self.rs.permutation(len(self)) if shuffle else np.arange(len(self))
        for i in range(self.n_batches(b, drop_last)):
            poses, vec = pkg.h36m.samples_numpy(self.skel, self.win[order[i * b:(i + 1) * b]], self.mean)
            yield torch.from_numpy(poses).to(self.device), torch.from_numpy(vec).to(self.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actions", type=int, default=8, help="generated actions per subject (S1, S5, S11)")
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("h36m_bench: needs a GPU")
    from bench import host_cores
    torch.set_num_threads(host_cores(cap=16))
    dev = torch.device("cuda:0")
    H, ops, fgd = pkg.h36m, pkg.ops, pkg.fgd
    args = pkg.config.load_config("gesture_autoencoder", epochs=1, batch_size=128, name="h36m_bench", model_save_path=None)
    mean = np.squeeze(np.array(args.mean_dir_vec))
    data = H.synthetic_dataset(seed=0, actions_per_subject=a.actions, n_frames=a.frames)
    _, win_host, arrays = H.window_table(data, True)
    raw = torch.from_numpy(np.concatenate(arrays)).to(dev)
    F, N = raw.shape[0], len(win_host)
    ds = H.Human36M(data, mean, is_train=True, augment=True, device=dev)
    val = H.Human36M(data, mean, is_train=False, device=dev)
    skel = torch.empty(F, 30, device=dev)
    poses, vec = torch.empty(N, 34, 30, device=dev), torch.empty(N, 34, 27, device=dev)
    flag = torch.empty(N, device=dev, dtype=torch.int32)
    rng = (ds.rng_state, H.NOISE_SITE, H.SELECT_SITE, H.P_LARGE, H.STD_LARGE, H.STD_SMALL)
    t_a = event_time(lambda: ops.h36m_normalize(raw, skel), a.blocks, a.reps)
    t_b = event_time(lambda: ops.h36m_samples(skel, ds.win_row0, 34, 2, ds._mean, poses, vec, flag), a.blocks, a.reps)
    t_b_aug = event_time(lambda: ops.h36m_samples(skel, ds.win_row0, 34, 2, ds._mean, poses, vec, flag, rng=rng), a.blocks, a.reps)
    # one augmented batch of 128 against the step that consumes it
    idx = torch.randperm(N, device=dev)[:128]
    t_batch = event_time(lambda: ds.build(idx), a.blocks, a.reps * 5)
    tab = ds.win_row0[idx].contiguous()
    bp, bv, bf = poses[:128], vec[:128], flag[:128]
    t_launch = event_time(lambda: ops.h36m_samples(skel, tab, 34, 2, ds._mean, bp, bv, bf, rng=rng), a.blocks, a.reps * 5)
    net = pkg.EmbeddingNet(args, 27, 34, None, None, None, mode="pose").to(dev)
    trainer = fgd.AutoencoderTrainer(net, lr=args.learning_rate)
    target = ds.build(idx)[1]
    t_step = event_time(lambda: trainer.train_iter(target), a.blocks, a.reps * 5)
    # the numpy restatement on the host
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        s = np.concatenate([H.normalize_numpy(x) for x in arrays])
        H.samples_numpy(s, win_host, mean)
        host.append(time.perf_counter() - t0)
    t_host = statistics.median(host)
    # one epoch of the training loop fed by each
    def epoch(train_set, val_set):
        g = pkg.EmbeddingNet(args, 27, 34, None, None, None, mode="pose").to(dev)
        fgd.train_autoencoder(args, train_set, val_set, save_dir=None, log=lambda s: None, generator=g)     # warm-up epoch (plans, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fgd.train_autoencoder(args, train_set, val_set, save_dir=None, log=lambda s: None, generator=g)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    plain = H.Human36M(data, mean, is_train=True, augment=False, device=dev)
    e_dev, e_aug = epoch(plain, val), epoch(ds, val)
    e_host = epoch(NumpyFeed(data, mean, True, dev), NumpyFeed(data, mean, False, dev))
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "frames": F, "windows": N,
           "stage_a_ms": t_a * 1e3, "stage_b_ms": t_b * 1e3, "stage_b_augment_ms": t_b_aug * 1e3,
           "device_samples_per_s": N / (t_a + t_b), "device_samples_per_s_augment": N / (t_a + t_b_aug), "numpy_samples_per_s": N / t_host,
           "augmented_batch128_launch_us": t_launch * 1e6, "augmented_batch128_build_us": t_batch * 1e6, "fused_ae_step_b128_us": t_step * 1e6,
           "epoch_s_device": e_dev, "epoch_s_device_augment": e_aug, "epoch_s_numpy_feed": e_host, "epoch_batches": plain.n_batches(128)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
