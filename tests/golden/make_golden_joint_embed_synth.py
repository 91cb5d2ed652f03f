#!/usr/bin/env python3
"""Golden values of joint-embedding synthesis and evaluation from the REAL reference on the CPU (build container only):
scripts/synthesize.py:generate_gestures with args.model == 'joint_embedding' (:36-209, the branch at :132-133) and
scripts/train.py:evaluate_testset (:234-329, the joint_embedding branch at :269-271).  The reference runs in fp32 here (generate_gestures
forces .float()).

As make_golden_joint_embed.py does, the state comes from tests/joint_embed_ref.make_state(seed, n_words) and is never stored (the decoder
alone is 22 MB); audio comes from joint_embed_synth_ref.make_audio(seed, n).  ContextEncoder reparameterises in eval mode too: the module-level
reparameterize is replaced by one that makes the same torch.randn_like draw and records it, so the fixture holds the reference's own eps.
generate_gestures cases: 1, 2 and 4 windows, with and without seed poses, with and without fade-out.  Per window the fixture keeps in_text,
pre_seq_partial, eps, the raw output, and of the 36 266-sample audio slice every 61st sample with its float64 sums
(joint_embed_synth_ref.audio_digest); per case the stacked output (rebuilt from the raw outputs by the reference's own cross-fade lines) and
the returned result.  evaluate_testset: two batches of B = 3 from joint_embed_ref.make_inputs.  Writes g22_joint_embed_synth.npz and
golden_report_joint_embed_synth.json next to this file.

    python tests/golden/make_golden_joint_embed_synth.py
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from make_golden_eval import MEAN_DIR_VEC, import_reference_callers      # noqa: E402
from make_golden_seq2seq_synth import VOCAB, synth_words                 # noqa: E402

POSE_DIM, N_POSES, N_PRE, FPS, STATE_SEED = 27, 34, 4, 15, 2200
CASES = (  # name, seconds, fade_out, seed poses, words seed, audio seed
    ("w1", 1.5, False, False, 1, 11), ("w1_fade_seed", 1.5, True, True, 1, 12), ("w2_seed", 3.5, False, True, 2, 13),
    ("w2_fade", 3.5, True, False, 2, 14), ("w4", 8.0, False, False, 3, 15), ("w4_fade_seed", 8.0, True, True, 3, 16))


def make_args():
    return argparse.Namespace(model="joint_embedding", hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=N_PRE,
                              n_poses=N_POSES, z_type="none", motion_resampling_framerate=FPS, wordembed_dim=300, mean_dir_vec=list(MEAN_DIR_VEC))


def main():
    R = import_reference_callers()
    import joint_embed_ref as JR
    import joint_embed_synth_ref as SR
    import importlib
    hip_syn = importlib.import_module("gesture-generation-from-trimodal-context_amd.synthesize")
    torch.set_num_threads(4)
    args = make_args()
    lang = R["vocab"].Vocab("words")
    for w in VOCAB:
        lang.index_word(w)
    lang.word_embedding_weights = None
    state = JR.make_state(STATE_SEED, lang.n_words)
    net = R["embedding_net"].EmbeddingNet(args, POSE_DIM, N_POSES, lang.n_words, 300, None, "random")
    net.load_state_dict(state, strict=True)
    net.float().train(False)
    draws = []

    def reparameterize(mu, logvar):                        # embedding_net.py:10-13 with the draw recorded
        std = torch.exp(0.5 * logvar)
        eps = torch.randn_like(std)
        draws.append(eps.detach().numpy().copy())
        return mu + eps * std
    R["embedding_net"].reparameterize = reparameterize
    torch.manual_seed(STATE_SEED + 1)
    store = dict(state_seed=np.array(STATE_SEED), vocab_words=np.array(VOCAB), cases=np.array([c[0] for c in CASES]), mean_dir_vec=np.array(MEAN_DIR_VEC))
    report = {"torch": torch.__version__, "numpy": np.__version__, "state_seed": STATE_SEED, "n_words": lang.n_words, "cases": {}}

    for name, secs, fade, use_seed, wseed, aseed in CASES:
        n_audio = int(round(secs * 16000))
        audio = SR.make_audio(aseed, n_audio)
        words = synth_words(secs, wseed, None)
        seed_seq = (0.1 * np.random.RandomState(50 + wseed).randn(6, POSE_DIM)).astype(np.float32) if use_seed else None
        calls, fwd = [], net.forward
        del draws[:]

        def spy(in_text, in_audio, pre_poses, poses, input_mode=None, variational_encoding=False, _fwd=fwd, _calls=calls):
            assert poses is None and input_mode == "speech" and not variational_encoding
            out = _fwd(in_text, in_audio, pre_poses, poses, input_mode, variational_encoding)
            _calls.append((in_text[0].numpy().copy(), in_audio[0].numpy().copy(), pre_poses[0].detach().numpy().copy(), out[6][0].detach().numpy().copy()))
            return out
        net.forward = spy
        stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
        try:
            with torch.no_grad():
                final = R["synthesize"].generate_gestures(args, net, lang, audio, words, seed_seq=seed_seq, fade_out=fade)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
            del net.forward
        assert len(draws) == len(calls)
        out_list = []                                      # the reference's cross-fade lines (:145-155) over the recorded raw outputs
        for _, _, _, raw in calls:
            out_seq = raw.copy()
            if out_list:
                last = out_list[-1][-N_PRE:]
                out_list[-1] = out_list[-1][:-N_PRE]
                for j in range(len(last)):
                    n = len(last)
                    out_seq[j] = last[j] * (n - j) / (n + 1) + out_seq[j] * (j + 1) / (n + 1)
            out_list.append(out_seq)
        stacked = np.vstack(out_list)
        redo = stacked.copy()
        if fade:
            redo = hip_syn.fade_out_to_mean(redo, hip_syn.end_padding_samples(args, n_audio), args)
        assert redo.shape == final.shape, (name, redo.shape, final.shape)
        smooth_err = float(np.abs(redo.astype(np.float64) - final).max() / np.abs(final).max())
        pre = name + "/"
        digests = [SR.audio_digest(c[1]) for c in calls]
        store[pre + "audio_len"], store[pre + "audio_seed"] = np.array(n_audio), np.array(aseed)
        store[pre + "words"] = np.array([w[0] for w in words])
        store[pre + "word_times"] = np.array([[w[1], w[2]] for w in words])
        store[pre + "fade_out"] = np.array(fade)
        store[pre + "seed_seq"] = seed_seq if seed_seq is not None else np.zeros((0, POSE_DIM), np.float32)
        store[pre + "win_text"] = np.stack([c[0] for c in calls])
        store[pre + "win_audio_samples"] = np.stack([d[0] for d in digests])
        store[pre + "win_audio_sums"] = np.stack([d[1] for d in digests])
        store[pre + "win_audio_len"] = np.array([len(c[1]) for c in calls])
        store[pre + "win_pre"] = np.stack([c[2] for c in calls])
        store[pre + "win_eps"] = np.stack([d[0] for d in draws])
        store[pre + "win_raw"] = np.stack([c[3] for c in calls])
        store[pre + "stacked"], store[pre + "final"] = stacked, final
        report["cases"][name] = dict(windows=len(calls), shape=list(final.shape), fade_rel_err=smooth_err, dtype=str(final.dtype),
                                     words_per_window=[int((c[0] != 0).sum()) for c in calls])
    assert sorted({v["windows"] for v in report["cases"].values()}) == [1, 2, 4]

    # ---- evaluate_testset: two batches of B = 3
    loader, seeds = [], (STATE_SEED + 31, STATE_SEED + 32)
    for s_ in seeds:
        ids, audio, target, _ = JR.make_inputs(s_, 3, lang.n_words)
        loader.append((torch.zeros(3, 5, dtype=torch.int64), torch.tensor([5, 5, 5]), ids, torch.zeros(3, N_POSES, 30), target.clone(), audio,
                       torch.zeros(3, 1), {}))
    store["eval/input_seeds"] = np.array(seeds)
    meters, AM = {}, R["train"].AverageMeter

    class SpyMeter(AM):
        def __init__(self, name, *a, **k):
            super().__init__(name, *a, **k)
            meters[name] = self
    R["train"].AverageMeter = SpyMeter
    del draws[:]
    recons, fwd = [], net.forward

    def spy_eval(*a, _fwd=fwd, **k):
        out = _fwd(*a, **k)
        recons.append(out[6].detach().numpy().copy())
        return out
    net.forward = spy_eval
    try:
        ret = R["train"].evaluate_testset(loader, net, None, None, args)
    finally:
        del net.forward
        R["train"].AverageMeter = AM
    net.train(False)
    assert len(draws) == 2 and len(recons) == 2
    for i in range(2):
        store[f"eval/eps{i}"], store[f"eval/recon{i}"] = draws[i], recons[i]
    store["eval/loss"], store["eval/joint_mae"], store["eval/accel"] = np.array(ret["loss"]), np.array(ret["joint_mae"]), np.array(meters["accel"].avg)
    report["evaluate_testset"] = dict(loss=float(ret["loss"]), joint_mae=float(ret["joint_mae"]), accel=float(meters["accel"].avg))
    path = os.path.join(HERE, "g22_joint_embed_synth.npz")
    np.savez_compressed(path, **store)
    report["fixture_bytes"] = os.path.getsize(path)
    with open(os.path.join(HERE, "golden_report_joint_embed_synth.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
