#!/usr/bin/env python3
"""Golden values of the variational pose embedding (build container only), from the REAL reference.

/root/reference/scripts/model/embedding_net.py: EmbeddingNet(mode='pose') is run with variational_encoding=True at B = 4 on the seeded state of
oracle.make_autoencoder_state and seeded poses; torch.randn_like is wrapped for the call so that the eps the reference draws is the seeded one
and is recorded.  Recorded: an eval-mode and a train-mode forward (z / mu / logvar / recon), and ONE training step: train_iter of
/root/reference/scripts/train_feature_extractor.py is taken from that file's text with its literal `variational_encoding = False` flipped to
True (the switch the reference's users flip by hand) and run at an epoch with a non-zero KL weight -- its return dict, every parameter
gradient (norm and 2048 sampled entries each; fc_mu and fc_logvar in full) and the norm of every parameter after Adam.
Writes g23_vae.npz and golden_report_vae.json next to this file.

Stand-in, and why: `fasttext` is not installed and model/vocab.py, which embedding_net.py imports at the top, imports it; nothing called here
touches a vocabulary.  An empty module of that name stands in.  train_feature_extractor.py itself is not imported (it needs lmdb and the
dataset stack at import): only the text of its train_iter function is executed.

    python tests/golden/make_golden_vae.py
"""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

REF = "/root/reference"
AE_SEED, POSE_SEED, EPS_SEED, B, EPOCH = 9, 41, 43, 4, 20


def reference_train_iter():
    src = open(os.path.join(REF, "scripts", "train_feature_extractor.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "train_iter")
    text = ast.get_source_segment(src, fn)
    assert text.count("variational_encoding = False") == 1
    ns = {"torch": torch, "F": F}
    exec(text.replace("variational_encoding = False", "variational_encoding = True"), ns)
    return ns["train_iter"]


def main():
    import vae_ref as R
    from harness import sample_idx
    from oracle import ref_model as O
    sys.path.insert(0, os.path.join(REF, "scripts"))
    sys.modules.setdefault("fasttext", types.ModuleType("fasttext"))
    import model.embedding_net as EN
    st = O.clone_state(O.make_autoencoder_state(AE_SEED), torch.float64)
    poses = R.make_poses(POSE_SEED, B).double()
    arrays = {"ae_seed": np.array(AE_SEED), "pose_seed": np.array(POSE_SEED), "eps_seed": np.array(EPS_SEED), "B": np.array(B), "epoch": np.array(EPOCH)}
    drawn = []
    real_randn_like = torch.randn_like

    def randn_like(t, *a, **k):
        e = R.make_eps(EPS_SEED + len(drawn), t.shape[0]).to(t.dtype)
        assert e.shape == t.shape
        drawn.append(e)
        return e

    def build():
        net = EN.EmbeddingNet(None, 27, 34, None, None, None, "pose").double()
        net.load_state_dict(O.clone_state(st, torch.float64), strict=True)
        return net

    torch.randn_like = randn_like
    try:
        for what in ("eval", "train"):
            net = build().train(what == "train")
            with torch.no_grad():
                out = net(None, None, None, poses, None, variational_encoding=True)
            arrays[f"{what}/eps"] = drawn[-1].numpy()
            for name, o in zip(("z", "mu", "logvar", "recon"), out[3:]):
                arrays[f"{what}/{name}"] = o.numpy()
        net = build().train()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        ret = reference_train_iter()(None, EPOCH, poses, net, opt)
        arrays["step/eps"] = drawn[-1].numpy()
    finally:
        torch.randn_like = real_randn_like
    arrays["step/loss"], arrays["step/KLD"] = np.array(ret["loss"]), np.array(ret["KLD"])
    for k, p in net.named_parameters():
        g = p.grad
        arrays[f"step/grad_norm/{k}"] = np.array(float(g.norm()))
        idx = sample_idx(g.numel())
        arrays[f"step/grad_idx/{k}"] = np.asarray(idx)
        arrays[f"step/grad_val/{k}"] = g.flatten()[torch.as_tensor(np.asarray(idx))].numpy()
        if ".fc_" in k:
            arrays[f"step/grad/{k}"] = g.numpy()
        arrays[f"step/after_norm/{k}"] = np.array(float(p.detach().norm()))
    np.savez_compressed(os.path.join(HERE, "g23_vae.npz"), **arrays)
    report = {"torch": torch.__version__, "loss": ret["loss"], "KLD": ret["KLD"], "eps_draws": len(drawn),
              "fc_logvar_grad_norm": float(arrays["step/grad_norm/pose_encoder.fc_logvar.weight"])}
    with open(os.path.join(HERE, "golden_report_vae.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(report, os.path.getsize(os.path.join(HERE, "g23_vae.npz")))


if __name__ == "__main__":
    main()
