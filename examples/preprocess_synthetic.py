#!/usr/bin/env python3
"""Raw clips -> training samples -> one device batch, on generated data.

    python examples/preprocess_synthetic.py --clips 8 --seconds 12 --batch 16

calculate_data_mean gives the `mean_pose` / `mean_dir_vec` constants a config carries, DataPreprocessor.run turns the clips into samples
in the stored format (resampling, windows, the three motion filters, direction vectors, audio and spectrogram slices on the device; the
spectrogram itself from melspec.extract_melspectrogram because the clips carry no 'audio_feat'), and a DeviceRecordFeeder assembles the
first `--batch` samples into the static input tensors a captured training step reads.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip = importlib.import_module("gesture-generation-from-trimodal-context_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    videos = [{"vid": f"speaker{i % 3}", "clips": [hip.preprocess.synthetic_clip(rs, a.seconds, 25, 30.0 * i, lively=i % 4 != 3)]} for i in range(a.clips)]
    mean_pose, mean_dir_vec, bone_lengths, seconds = hip.calculate_data_mean(videos)
    print("mean bone lengths", np.round(bone_lengths, 4), f"over {seconds:.0f} s")
    dp = hip.DataPreprocessor(34, 10, 15, mean_pose, mean_dir_vec)
    samples, n_filtered_out = dp.run(videos)
    print(f"{len(samples)} samples, filtered out: {dict(n_filtered_out)}")
    lang = hip.Vocab("words")
    for i in range(40):
        lang.index_word(f"w{i}")
    dataset = hip.data.SpeechMotionDataset(samples, 34, 10, 15)
    dataset.set_lang_model(lang)
    B = min(a.batch, len(samples))
    text = torch.zeros(B, 34, dtype=torch.int64, device=dev)
    audio = torch.zeros(B, 36267, device=dev)
    target = torch.zeros(B, 34, 27, device=dev)
    vid = torch.zeros(B, dtype=torch.int64, device=dev)
    feeder = hip.data.DeviceRecordFeeder(text, audio, target, vid, lang, dataset.speaker_model)
    feeder.put(samples[:B])
    feeder.ready()
    torch.cuda.synchronize()
    ref = dataset[0]
    assert torch.equal(text[0].cpu(), ref[1]) and torch.equal(target[0].cpu(), ref[3]) and torch.equal(audio[0].cpu(), ref[4])
    print(f"device batch of {B}: text {tuple(text.shape)}, audio {tuple(audio.shape)}, target {tuple(target.shape)}; "
          f"sample 0 equals SpeechMotionDataset.__getitem__")


if __name__ == "__main__":
    main()
