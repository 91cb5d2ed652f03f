#!/usr/bin/env python3
"""Golden values of Seq2Seq synthesis, evaluation and checkpoint loading from the REAL reference on the CPU (build container only):
scripts/synthesize.py:generate_gestures with args.model == 'seq2seq' (:36-209), scripts/train.py:evaluate_testset (:234-329, the seq2seq
branch) and utils/train_utils.py:load_checkpoint_and_model on a checkpoint written in the reference's format.  As make_golden_eval.py does,
the libraries this image lacks are replaced by empty stub modules before the import.  The reference runs in fp32 here (generate_gestures
forces .float()).

Model: hidden_size 12, 2 layers, pose_dim 27, vocabulary 4 + 27 words, embedding 10, n_poses 34, n_pre_poses 4, 15 fps, z_type none; the
BatchNorm buffers are moved off their initial values.  generate_gestures cases: 1, 2 and 4 windows, with and without seed poses, fade_out
False / True, one utterance with a window that holds no word (in_text = [SOS, EOS]).  Audio matters through its length only: the length is
stored, the reference is fed zeros.  Every window's in_text, pre_seq_partial and raw output are recorded by spying on forward; the stacked
output before the cubic smoothing is rebuilt from them by the reference's own cross-fade lines.  Writes g20_seq2seq_synth.npz,
g20_seq2seq_checkpoint.bin and golden_report_seq2seq_synth.json next to this file.

    python tests/golden/make_golden_seq2seq_synth.py
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

H, N_LAYERS, POSE_DIM, EMBED, N_POSES, N_PRE, FPS = 12, 2, 27, 10, 34, 4, 15
VOCAB = ("so what i want to talk about today is how we move our hands when speak and why it matters for the people who listen because gesture").split()
assert len(VOCAB) == len(set(VOCAB)) == 27
CASES = (  # name, seconds, fade_out, seed poses, words seed, silent interval (no word starts or ends inside it) or None
    ("w1", 1.5, False, False, 1, None), ("w1_fade_seed", 1.5, True, True, 1, None), ("w2_seed", 3.5, False, True, 2, None),
    ("w2_fade", 3.5, True, False, 2, None), ("w4", 8.0, False, False, 3, None), ("w4_fade_seed", 8.0, True, True, 3, None),
    ("w4_silent_window", 8.0, True, False, 4, (3.9, 6.4)))


def make_args():
    return argparse.Namespace(model="seq2seq", hidden_size=H, n_layers=N_LAYERS, dropout_prob=0.0, n_pre_poses=N_PRE, n_poses=N_POSES,
                              GAN_noise_size=0, z_type="none", motion_resampling_framerate=FPS, wordembed_dim=EMBED,
                              mean_dir_vec=list(MEAN_DIR_VEC), loss_regression_weight=1.0, loss_kld_weight=0.1, loss_reg_weight=0.1)


def synth_words(duration, seed, silent):
    r = np.random.RandomState(seed)
    t, words = 0.05, []
    while t < duration - 0.1:
        d = float(r.uniform(0.12, 0.5))
        if silent is None or t + d <= silent[0] or t >= silent[1]:
            words.append([VOCAB[int(r.randint(len(VOCAB)))] if r.rand() > 0.1 else "zzzunknown", round(t, 3), round(t + d, 3)])
        t += d + float(r.uniform(0.0, 0.6))
    return words


def main():
    R = import_reference_callers()
    from model.seq2seq_net import Seq2SeqNet
    import utils.train_utils as tu
    torch.set_num_threads(4)
    torch.serialization.add_safe_globals([argparse.Namespace, R["vocab"].Vocab])      # the reference's plain torch.load under torch >= 2.6
    args = make_args()
    lang = R["vocab"].Vocab("words")
    for w in VOCAB:
        lang.index_word(w)
    lang.word_embedding_weights = None
    torch.manual_seed(2020)
    net = Seq2SeqNet(args, POSE_DIM, N_POSES, lang.n_words, EMBED, None)
    bn = net.decoder.decoder.pre_linear[1]
    with torch.no_grad():
        bn.running_mean.copy_(0.3 * torch.randn(H)); bn.running_var.copy_(0.5 + torch.rand(H)); bn.num_batches_tracked.fill_(7)
    net.train(False)
    store = {"state/" + k: v.numpy().copy() for k, v in net.state_dict().items()}
    store.update(vocab_words=np.array(VOCAB), cases=np.array([c[0] for c in CASES]), mean_dir_vec=np.array(MEAN_DIR_VEC))
    report = {"torch": torch.__version__, "numpy": np.__version__, "cases": {}}

    # ---- generate_gestures
    import importlib
    hip_syn = importlib.import_module("gesture-generation-from-trimodal-context_amd.synthesize")
    for name, secs, fade, use_seed, wseed, silent in CASES:
        n_audio = int(round(secs * 16000))
        words = synth_words(secs, wseed, silent)
        seed_seq = (0.1 * np.random.RandomState(50 + wseed).randn(6, POSE_DIM)).astype(np.float32) if use_seed else None
        calls, fwd = [], net.forward

        def spy(in_text, in_lengths, poses, vid, _fwd=fwd, _calls=calls):
            out = _fwd(in_text, in_lengths, poses, vid)
            assert vid is None and int(in_lengths[0]) == in_text.shape[1]
            _calls.append((in_text[0].numpy().copy(), poses[0].detach().numpy().copy(), out[0].detach().numpy().copy()))
            return out
        net.forward = spy
        stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
        try:
            with torch.no_grad():
                final = R["synthesize"].generate_gestures(args, net, lang, np.zeros(n_audio, np.float32), words, seed_seq=seed_seq, fade_out=fade)
        finally:
            sys.stdout.close()
            sys.stdout = stdout
            del net.forward
        out_list = []                                      # the reference's cross-fade lines (:145-155) over the recorded raw outputs
        for _, _, raw in calls:
            out_seq = raw.copy()
            if out_list:
                last = out_list[-1][-N_PRE:]
                out_list[-1] = out_list[-1][:-N_PRE]
                for j in range(len(last)):
                    n = len(last)
                    out_seq[j] = last[j] * (n - j) / (n + 1) + out_seq[j] * (j + 1) / (n + 1)
            out_list.append(out_seq)
        stacked = np.vstack(out_list)
        # the product's host functions on the stacked output: the error recorded here is what tests/test_seq2seq_synth_cpu.py gates
        redo = hip_syn.seq2seq_smooth(stacked.copy(), len(calls), N_POSES, N_PRE)
        if fade:
            redo = hip_syn.fade_out_to_mean(redo, hip_syn.end_padding_samples(args, n_audio), args)
        assert redo.shape == final.shape, (name, redo.shape, final.shape)
        smooth_err = float(np.abs(redo.astype(np.float64) - final).max() / np.abs(final).max())
        texts = [c[0] for c in calls]
        for i, t in enumerate(texts):
            assert np.array_equal(t, hip_syn.seq2seq_window_text(lang, words, i, N_POSES, N_PRE, FPS)), (name, i)
        pre = name + "/"
        store[pre + "audio_len"] = np.array(n_audio)
        store[pre + "words"] = np.array([w[0] for w in words])
        store[pre + "word_times"] = np.array([[w[1], w[2]] for w in words])
        store[pre + "fade_out"] = np.array(fade)
        store[pre + "seed_seq"] = seed_seq if seed_seq is not None else np.zeros((0, POSE_DIM), np.float32)
        store[pre + "win_text_len"] = np.array([len(t) for t in texts])
        store[pre + "win_text"] = np.concatenate(texts)
        store[pre + "win_pre"] = np.stack([c[1] for c in calls])
        store[pre + "win_raw"] = np.stack([c[2] for c in calls])
        store[pre + "stacked"], store[pre + "final"] = stacked, final
        report["cases"][name] = dict(windows=len(calls), text_lengths=[len(t) for t in texts], shape=list(final.shape),
                                     smooth_and_fade_rel_err=smooth_err, dtype=str(final.dtype))
    assert any(2 in v["text_lengths"] for v in report["cases"].values()), "no window without a word"
    assert sorted({v["windows"] for v in report["cases"].values()}) == [1, 2, 4]

    # ---- evaluate_testset: two batches of B = 3, lengths sorted (the reference's pack_padded_sequence wants them so)
    g = torch.Generator().manual_seed(77)
    loader = []
    for i, lens in enumerate(([7, 4, 2], [5, 5, 3])):
        text = torch.randint(4, lang.n_words, (3, max(lens)), generator=g)
        for b, n in enumerate(lens):
            text[b, 0], text[b, n - 1] = 1, 2
            text[b, n:] = 0
        target = 0.2 * torch.randn(3, N_POSES, POSE_DIM, generator=g)
        store[f"eval/text{i}"], store[f"eval/lengths{i}"], store[f"eval/target{i}"] = text.numpy(), np.array(lens), target.numpy().copy()
        loader.append((text, torch.tensor(lens), torch.zeros(3, N_POSES, dtype=torch.int64), torch.zeros(3, N_POSES, 30), target.clone(),
                       torch.zeros(3, 8), torch.zeros(3, 1), {}))
    meters, AM = {}, R["train"].AverageMeter

    class SpyMeter(AM):
        def __init__(self, name, *a, **k):
            super().__init__(name, *a, **k)
            meters[name] = self
    R["train"].AverageMeter = SpyMeter
    ret = R["train"].evaluate_testset(loader, net, torch.nn.L1Loss(), None, args)
    R["train"].AverageMeter = AM
    net.train(False)
    store["eval/loss"], store["eval/joint_mae"], store["eval/accel"] = np.array(ret["loss"]), np.array(ret["joint_mae"]), np.array(meters["accel"].avg)
    report["evaluate_testset"] = dict(loss=float(ret["loss"]), joint_mae=float(ret["joint_mae"]), accel=float(meters["accel"].avg))

    # ---- a checkpoint in the reference's format (utils/train_utils.py:147-149 as train_eval writes it), read back by the reference's loader
    path = os.path.join(HERE, "g20_seq2seq_checkpoint.bin")
    tu.save_checkpoint({"args": args, "epoch": 3, "lang_model": lang, "speaker_model": None, "pose_dim": POSE_DIM, "gen_dict": net.state_dict()}, path)
    _a, gen, loss_fn, _l, _s, pd = tu.load_checkpoint_and_model(path, torch.device("cpu"))
    assert pd == POSE_DIM and isinstance(loss_fn, torch.nn.L1Loss) and not gen.training
    text, lens, poses = torch.as_tensor(store["eval/text0"]), store["eval/lengths0"].tolist(), torch.as_tensor(store["eval/target0"])
    with torch.no_grad():
        store["ckpt/eval_outputs"] = gen(text, torch.tensor(lens), poses, None).numpy()
    report["checkpoint_bytes"] = os.path.getsize(path)
    np.savez_compressed(os.path.join(HERE, "g20_seq2seq_synth.npz"), **store)
    with open(os.path.join(HERE, "golden_report_seq2seq_synth.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
