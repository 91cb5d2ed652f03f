#!/usr/bin/env python3
"""Golden values of the Seq2Seq baseline (build container only): the REAL reference's Seq2SeqNet (model/seq2seq_net.py) and
train_iter_seq2seq (train_eval/train_seq2seq.py) in double on the CPU.

Two cases (hidden_size 8 and 12; 2 layers, pose_dim 27, n_frames 6, n_pre_poses 2, B = 5, sorted lengths 7, 5, 5, 2, 1 -- the reference's
pack_padded_sequence wants them sorted -- vocabulary 30, embedding 10, dropout_prob 0 since the reference's draws cannot be injected):
`h8_clip` has targets scaled so that clip_grad_norm_(.., 5) engages, `h12_noclip` has loss weights small enough that it does not.  Each
stores the state dict (fp32 values, exactly), two batches of inputs, and for the first batch the train-mode outputs, the loss, the gradients
of custom_loss before and after the clip, the BatchNorm buffers after the forward, eval-mode outputs at B = 5 and B = 1; then the losses,
the clipped gradients of both steps and every parameter and buffer after TWO train_iter_seq2seq calls (batch 1, batch 2) with
Adam(lr=1e-3, betas=(0.5, 0.999)).  Writes g19_seq2seq.npz and golden_report_seq2seq.json next to this file.

    python tests/golden/make_golden_seq2seq.py
"""
import copy
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = "/root/reference"

N_WORDS, EMBED, N_LAYERS, POSE_DIM, N_FRAMES, N_PRE, LENGTHS = 30, 10, 2, 27, 6, 2, [7, 5, 5, 2, 1]
CASES = {"h8_clip": dict(H=8, seed=1908, pose_scale=400.0, w=(1.0, 0.1, 0.1)),
         "h12_noclip": dict(H=12, seed=1912, pose_scale=1.0, w=(0.05, 0.01, 0.01))}
SMALL = 1e-6      # gradient elements below this share of their tensor's largest leave the two-step parameter comparison (Adam divides by |g|)


def batch(g, scale):
    B, T = len(LENGTHS), max(LENGTHS)
    text = torch.randint(1, N_WORDS - 6, (B, T), generator=g)          # the last 6 tokens never occur: their embedding rows must not move
    for b, n in enumerate(LENGTHS):
        text[b, n:] = 0
    poses = torch.randn(B, N_FRAMES, POSE_DIM, generator=g, dtype=torch.float64) * scale
    return text, poses


def main():
    sys.path.insert(0, os.path.join(REF, "scripts"))
    from model.seq2seq_net import Seq2SeqNet
    from train_eval.train_seq2seq import custom_loss, train_iter_seq2seq
    arrays, report = {}, {"cases": {}}
    for name, c in CASES.items():
        args = SimpleNamespace(hidden_size=c["H"], n_layers=N_LAYERS, dropout_prob=0.0, n_pre_poses=N_PRE, GAN_noise_size=0,
                               loss_regression_weight=c["w"][0], loss_kld_weight=c["w"][1], loss_reg_weight=c["w"][2])
        torch.manual_seed(c["seed"])
        torch.set_default_dtype(torch.float32)
        net0 = Seq2SeqNet(args, POSE_DIM, N_FRAMES, N_WORDS, EMBED, None).double()      # fp32 initialisation, double arithmetic
        torch.set_default_dtype(torch.float64)                                          # (the forward's torch.zeros output buffer follows it)
        g = torch.Generator().manual_seed(c["seed"] * 7)
        text1, poses1 = batch(g, c["pose_scale"])
        _, poses2 = batch(g, c["pose_scale"])
        valid = text1 > 0                                   # batch 2: the same tokens in another order (a token met in one batch only has an
        text2 = text1.clone()                               # exactly-zero gradient in the other, which the Adam comparison would leave out)
        text2[valid] = text1[valid][torch.randperm(int(valid.sum()), generator=g)]
        pre = name + "/"
        for k, v in net0.state_dict().items():
            arrays[pre + "state/" + k] = v.numpy().astype(np.float32) if v.dtype.is_floating_point else v.numpy()
        arrays[pre + "lengths"] = np.array(LENGTHS)
        arrays[pre + "text1"], arrays[pre + "poses1"], arrays[pre + "text2"], arrays[pre + "poses2"] = (text1.numpy(), poses1.numpy(), text2.numpy(),
                                                                                                         poses2.numpy())
        arrays[pre + "loss_weights"] = np.array(c["w"])
        # first batch, train mode: outputs, loss, gradients before / after the clip, buffers
        net = copy.deepcopy(net0).train()
        out = net(text1, LENGTHS, poses1, None)
        loss = custom_loss(out, poses1, args, 0)
        loss.backward()
        arrays[pre + "train_outputs"], arrays[pre + "loss"] = out.detach().numpy(), np.array(float(loss))
        for k, p in net.named_parameters():
            arrays[pre + "grad/" + k] = p.grad.numpy().copy()
        norm = float(torch.nn.utils.clip_grad_norm_(net.parameters(), 5))
        for k, b in net.named_buffers():
            arrays[pre + "buffers_after/" + k] = b.numpy().copy()
        # eval mode
        net = copy.deepcopy(net0).eval()
        with torch.no_grad():
            arrays[pre + "eval_outputs"] = net(text1, LENGTHS, poses1, None).numpy()
            arrays[pre + "eval_outputs_b1"] = net(text1[:1], LENGTHS[:1], poses1[:1], None).numpy()
        # two training iterations
        net = copy.deepcopy(net0).train()
        optim = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
        small = {k: torch.zeros_like(p, dtype=torch.bool) for k, p in net.named_parameters()}
        for i, (tx, ps) in enumerate(((text1, poses1), (text2, poses2)), 1):
            r = train_iter_seq2seq(args, 0, tx, LENGTHS, ps, net, optim)
            arrays[pre + f"step{i}/loss"] = np.array(r["loss"])
            for k, p in net.named_parameters():
                arrays[pre + f"step{i}/grad_clipped/" + k] = p.grad.numpy().copy()
                small[k] |= p.grad.abs() < SMALL * p.grad.abs().max()
        for k, v in net.state_dict().items():
            arrays[pre + "after2/" + k] = v.numpy().copy()
        used = set(text1.flatten().tolist()) | set(text2.flatten().tolist())
        absent = [i for i in range(N_WORDS) if i not in used]
        n_cmp = n_out = 0
        for k, p in net.named_parameters():
            m = small[k].clone()
            if k == "encoder.embedding.weight":
                m[absent] = False                        # compared bit for bit instead
                n_cmp -= len(absent) * p.shape[1]
            n_cmp += p.numel(); n_out += int(m.sum())
        report["cases"][name] = {"grad_norm_before_clip": norm, "clip_engages": norm > 5.0, "loss": float(loss),
                                 "absent_tokens": absent, "left_out_share": n_out / n_cmp, "left_out": n_out, "compared": n_cmp}
        assert (norm > 5.0) == (name == "h8_clip"), (name, norm)
        assert n_out / n_cmp <= 0.01, (name, n_out, n_cmp)
    np.savez_compressed(os.path.join(HERE, "g19_seq2seq.npz"), **arrays)
    report["torch"] = torch.__version__
    with open(os.path.join(HERE, "golden_report_seq2seq.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
