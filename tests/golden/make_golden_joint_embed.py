#!/usr/bin/env python3
"""Golden values of the joint-embedding baseline (build container only): the REAL reference's EmbeddingNet(mode='random')
(model/embedding_net.py) and train_iter_embed (train_eval/train_joint_embed.py) in double on the CPU.

The state comes from tests/joint_embed_ref.make_state(seed) and the inputs from make_inputs(seed, B) (V = 32 words; B = 3 for the eval
forwards, B = 4 for the train steps), so the fixture holds seeds, the injected eps, outputs, losses, per-tensor gradient norms, 48 sampled
gradient entries per tensor, the BatchNorm buffers of both encoders after the step and the stepped-parameter norms -- never the state.
Every dropout has p = 0 (ATen's draws are not recordable); reparameterize's eps is injected by replacing the module-level function.
One eval forward and one train_iter_embed step (Adam lr 5e-4, betas (0.5, 0.999)) per input mode ('speech', 'pose').  ReLU near-ties: the maker ASSERTS that no input of the latent heads' ReLUs lies within 1e-4 of zero
(relative to the tensor's maximum) and takes the first seed that passes; for the activation tensors of 1e4 .. 1e6 elements that cannot hold
(see the comment in main), and the census of every seed tried goes into the report.  Writes g21_joint_embed.npz and golden_report_joint_embed.json (with the reference's state_dict key list) next to this file.

    python tests/golden/make_golden_joint_embed.py
"""
import json
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/scripts"
V, N_SAMPLED = 32, 48


def main():
    import joint_embed_ref as R
    sys.path.insert(0, REF)
    for name in ("fasttext", "umap"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import model.embedding_net as embedding_net            # must come first (circular import)
    from train_eval.train_joint_embed import train_iter_embed
    args = SimpleNamespace(hidden_size=300, n_layers=4, dropout_prob=0.0, freeze_wordembed=False, n_pre_poses=4, n_poses=34)

    def ref_net(state):
        torch.set_default_dtype(torch.float32)
        net = embedding_net.EmbeddingNet(args, 27, 34, V, 300, None, "random")
        net.load_state_dict(state, strict=True)
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if isinstance(m, torch.nn.GRU):
                m.dropout = 0.0
        return net.double()

    def inject(eps):
        embedding_net.reparameterize = lambda mu, logvar: mu + eps * torch.exp(0.5 * logvar)

    # ReLU near-ties.  The census (joint_embed_ref.relu_stats) covers the functional ReLUs of the TCN too, skips exact zeros and tensors without
    # negative elements.  What CAN be kept 1e-4 (relative) away from its kink is asserted and decides the seed: the ReLUs of the two
    # latent heads this change adds kernels for (HEADS: ContextEncoder.out.2 with B x 128 inputs, decoder.pre_pose_net.2 with B x 32).
    # The other activation inputs hold 1e4 .. 1e6 elements (WavEncoder: B x 16 x 7 000, the TCN: B x 34 x 300 per conv, PoseEncoderConv:
    # B x 32 x 32 and more): with a density of ~0.1 / sigma at zero and a maximum of ~4 sigma, a window of 1e-4 of the maximum catches ~1e-4 N of
    # them, i.e. at least one with near certainty.  The census of every seed tried is written to the report as the evidence.
    HEADS, TRIED = ("context_encoder.out.2", "decoder.pre_pose_net.2"), 6
    census, seed, chosen = {}, 2100, None
    for s_ in range(2100, 2100 + TRIED):
        state = R.make_state(s_, V)
        chain = R.build(state).train()
        worst_small, big = 1.0, {}
        for b_ in (3, 4):                                             # the eval inputs (B = 3) and the train inputs (B = 4)
            ids, audio, target, draws = R.make_inputs(s_ + b_, b_, V)
            st = R.relu_stats(chain, ids, audio.double(), target.double(), "speech", {k: v.double() for k, v in draws.items()})
            for name, v in st.items():
                if name in HEADS:
                    worst_small = min(worst_small, v["margin"])
                else:
                    big[name] = big.get(name, 0) + v["near"]
        census[s_] = {"small_tensor_margin": worst_small, "large_tensor_near_ties": big}
        if chosen is None and worst_small > 1e-4:
            chosen = s_
    assert chosen is not None, "no seed keeps the latent heads' ReLU inputs 1e-4 away from zero"
    seed = chosen
    state = R.make_state(seed, V)
    assert census[seed]["small_tensor_margin"] > 1e-4
    margin = census[seed]["small_tensor_margin"]
    seeds_with_a_clean_large_tensor_set = [s_ for s_, c in census.items() if sum(c["large_tensor_near_ties"].values()) == 0]
    arrays = {"state_seed": np.array(seed)}
    report = {"state_seed": seed, "relu_margin_latent_heads": margin, "relu_census": {str(k): v for k, v in census.items()},
              "seeds_without_large_tensor_near_ties": seeds_with_a_clean_large_tensor_set, "torch": torch.__version__}
    report["state_keys"] = {k: {"shape": list(v.shape), "dtype": str(v.dtype)} for k, v in ref_net(state).float().state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    for mode in ("speech", "pose"):
        ids, audio, target, draws = R.make_inputs(seed + 3, 3, V)
        arrays["eval_inputs_seed"], arrays["eval_B"] = np.array(seed + 3), np.array(3)
        eps = draws["c.eps"].double()
        arrays[f"eval/{mode}/eps"] = eps.numpy()
        net = ref_net(state).eval()
        inject(eps)
        with torch.no_grad():
            out = net(ids, audio.double(), target[:, :4].double(), target.double(), mode)
        for i, o in enumerate(out):
            if o is not None:
                arrays[f"eval/{mode}/out{i}"] = o.numpy()
        ids, audio, target, draws = R.make_inputs(seed + 4, 4, V)
        arrays["train_inputs_seed"], arrays["train_B"] = np.array(seed + 4), np.array(4)
        eps = draws["c.eps"].double()
        arrays[f"train/{mode}/eps"] = eps.numpy()
        net = ref_net(state).train()
        optim = torch.optim.Adam(net.parameters(), lr=5e-4, betas=(0.5, 0.999))
        inject(eps)
        r = train_iter_embed(args, 0, ids, audio.double(), target.double(), net, optim, mode)
        arrays[f"train/{mode}/loss"] = np.array(r["loss"])
        report[f"loss_{mode}"] = r["loss"]
        for k, p in net.named_parameters():
            if p.grad is None:
                continue
            arrays[f"train/{mode}/grad_norm/{k}"] = np.array(float(p.grad.norm()))
            idx = torch.randint(0, p.numel(), (min(N_SAMPLED, p.numel()),), generator=g)
            arrays[f"train/{mode}/grad_idx/{k}"] = idx.numpy()
            arrays[f"train/{mode}/grad_val/{k}"] = p.grad.flatten()[idx].numpy()
        for k, v in net.state_dict().items():
            if "running_" in k or k.endswith("num_batches_tracked"):
                arrays[f"train/{mode}/after/{k}"] = v.numpy().copy()
            elif v.dtype.is_floating_point:
                arrays[f"train/{mode}/after_norm/{k}"] = np.array(float(v.norm()))
    np.savez_compressed(os.path.join(HERE, "g21_joint_embed.npz"), **arrays)
    with open(os.path.join(HERE, "golden_report_joint_embed.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in report.items() if k not in ("state_keys",)}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
