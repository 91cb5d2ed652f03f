#!/usr/bin/env python3
"""Train the FGD autoencoder from raw Human3.6M-shaped positions, end to end on the device, on generated motion.

    python examples/train_autoencoder_h36m.py --epochs 5 --actions 4 --frames 1500 [--augment] [--data data/h36m/data_3d_h36m.npz]

h36m.Human36M normalises and frontalises the positions and builds the (poses, dir_vec) batches on the device (csrc/h36m.hip);
fgd.train_autoencoder is the loop of the reference's train_feature_extractor.py: validation, best-checkpoint bookkeeping, one pass of the
fused training step per epoch.  The checkpoint it writes is the `eval_net_path` of the generator configs.  Without --data the positions
come from h36m.synthetic_dataset, which stands in for the dataset file.
"""
import argparse
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip = importlib.import_module("gesture-generation-from-trimodal-context_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None, help="data_3d_h36m.npz; generated motion when absent")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--actions", type=int, default=4)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--augment", action="store_true")
    ap.add_argument("--save_dir", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    save_dir = a.save_dir or tempfile.mkdtemp(prefix="h36m_autoencoder_")
    args = hip.config.load_config("gesture_autoencoder", epochs=a.epochs, batch_size=a.batch, model_save_path=save_dir)
    mean_dir_vec = np.squeeze(np.array(args.mean_dir_vec))
    data = a.data or hip.h36m.synthetic_dataset(seed=0, actions_per_subject=a.actions, n_frames=a.frames)
    train_set = hip.Human36M(data, mean_dir_vec, is_train=True, augment=a.augment, device=dev)
    val_set = hip.Human36M(data, mean_dir_vec, is_train=False, augment=False, device=dev)
    print(f"{len(train_set)} training and {len(val_set)} validation samples from {len(train_set.actions)} actions, {train_set.skel.shape[0]} frames")
    best, history = hip.fgd.train_autoencoder(args, train_set, val_set)
    for h in history:
        print("epoch {epoch}: validation {val_loss:.4f}, training {train_loss:.4f}, {samples_per_s:.0f} samples/s".format(**h))
    path = os.path.join(save_dir, f"{args.name}_checkpoint_best.bin")
    evaluator = hip.fgd.EmbeddingSpaceEvaluator(args, path, None, dev)
    print(f"best validation loss {best[0]:.4f} at epoch {best[1]}; {path} loads into EmbeddingSpaceEvaluator "
          f"({sum(p.numel() for p in evaluator.net.parameters())} parameters)")


if __name__ == "__main__":
    main()
