#!/usr/bin/env python3
"""Golden values of the Seq2Seq text encoder (build container only): the REAL reference's EncoderRNN (model/seq2seq_net.py:14-56) in double.

For hidden_size 8 and 12 (input_size 20, embed_size 12, n_layers 2, eval mode; B = 5 rows of lengths 9, 7, 7, 3, 1; token 0 only as padding)
this records the module's state dict (fp32 values, exactly), the inputs, `outputs` and `hidden`, and the gradients of a seeded linear functional
sum(outputs * c_out) + sum(hidden * c_hid) with respect to every parameter.  Writes g18_seq2seq_encoder.npz and
golden_report_seq2seq_encoder.json next to this file.

    python tests/golden/make_golden_seq2seq_encoder.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = "/root/reference"

INPUT_SIZE, EMBED, N_LAYERS, LENGTHS, HIDDEN = 20, 12, 2, [9, 7, 7, 3, 1], (8, 12)


def main():
    sys.path.insert(0, os.path.join(REF, "scripts"))
    from model.seq2seq_net import EncoderRNN
    arrays, report = {}, {"cases": {}}
    T, B = max(LENGTHS), len(LENGTHS)
    for H in HIDDEN:
        torch.manual_seed(1800 + H)
        enc = EncoderRNN(INPUT_SIZE, EMBED, H, N_LAYERS, dropout=0.5).eval()        # fp32 initialisation: the weights are fp32 values ...
        enc = enc.double()                                                           # ... and the arithmetic on them is double
        g = torch.Generator().manual_seed(18 * H)
        seqs = torch.randint(1, INPUT_SIZE, (T, B), generator=g)
        for b, n in enumerate(LENGTHS):
            seqs[n:, b] = 0
        c_out = torch.randn(T, B, H, generator=g, dtype=torch.float64)
        c_hid = torch.randn(2 * N_LAYERS, B, H, generator=g, dtype=torch.float64)
        outputs, hidden = enc(seqs, LENGTHS)
        ((outputs * c_out).sum() + (hidden * c_hid).sum()).backward()
        pre = f"h{H}/"
        for k, v in enc.state_dict().items():
            arrays[pre + "state/" + k] = v.numpy().astype(np.float32)               # (exact)
        for k, p in enc.named_parameters():
            arrays[pre + "grad/" + k] = p.grad.numpy()
        arrays[pre + "input_seqs"], arrays[pre + "lengths"] = seqs.numpy(), np.array(LENGTHS)
        arrays[pre + "outputs"], arrays[pre + "hidden"] = outputs.detach().numpy(), hidden.detach().numpy()
        arrays[pre + "c_out"], arrays[pre + "c_hid"] = c_out.numpy(), c_hid.numpy()
        report["cases"][f"h{H}"] = {"outputs_absmax": float(outputs.detach().abs().max()), "hidden_absmax": float(hidden.detach().abs().max()),
                                    "grad_absmax": {k: float(p.grad.abs().max()) for k, p in enc.named_parameters()},
                                    "embedding_grad_row0_absmax": float(enc.embedding.weight.grad[0].abs().max())}
    np.savez_compressed(os.path.join(HERE, "g18_seq2seq_encoder.npz"), **arrays)
    report["torch"] = torch.__version__
    with open(os.path.join(HERE, "golden_report_seq2seq_encoder.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
