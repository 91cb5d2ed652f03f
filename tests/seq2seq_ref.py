"""fp64 reference of the Seq2Seq baseline (model/seq2seq_net.py, train_eval/train_seq2seq.py) on top of gru_seq_ref: the attention, the
decoder step, the autoregressive loop, custom_loss and the gradient clip as plain torch expressions on the CPU, every gradient from autograd.
Unlike the reference's own modules it takes unsorted lengths and injected dropout masks, and runs in fp32 as well (the yardstick the gates
of the GPU tests are measured from).  tests/test_seq2seq_cpu.py shows that it reproduces the real reference (fixture g19) to 1e-12."""
import torch

from gru_seq_ref import RefEncoder, RefGRU


def attn_chain(q, keys, enc, v):
    """The attention step kernels' contract: (w (B, Te), ctx (B, H)) from q (B, H), keys / enc (B, Te, H), v (H)."""
    s = (torch.tanh(q[:, None, :] + keys) * v).sum(-1)
    w = torch.softmax(s, dim=1)
    return w, (w[:, :, None] * enc).sum(1)


def custom_loss(output, target, w_reg, w_cont, w_var):
    """train_seq2seq.py:6-33 -> (total, (mse term, continuity term, variance term))."""
    n = output.numel()
    mse = ((output - target) ** 2).mean() * w_reg
    cont = (output[:, 1:] - output[:, :-1]).abs().sum() / n * w_cont
    var = -torch.norm(output, 2, 1).sum() / n * w_var
    return mse + cont + var, (mse, cont, var)


def clip_coef(grads, max_norm=5.0):
    """clip_grad_norm_'s (total norm, coefficient clamped to 1)."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    return total, torch.clamp(max_norm / (total + 1e-6), max=1.0)


class RefSeq2Seq:
    """Seq2SeqNet from a state dict (the reference's keys).  bn_momentum / eps are BatchNorm1d's defaults."""

    def __init__(self, state, n_layers, n_frames, n_pre_poses, dtype=torch.float64):
        self.dtype, self.n_layers, self.n_frames, self.n_pre = dtype, n_layers, n_frames, n_pre_poses
        st = {k: torch.as_tensor(v) for k, v in state.items()}
        self.enc = RefEncoder({k[len("encoder."):]: v for k, v in st.items() if k.startswith("encoder.")}, n_layers, dtype)
        d = "decoder.decoder."
        self.gru = RefGRU({k[len(d + "gru."):]: v for k, v in st.items() if k.startswith(d + "gru.")}, n_layers, 1, dtype)
        self.p = {}
        for k in ("attn.attn.weight", "attn.attn.bias", "attn.v", "pre_linear.0.weight", "pre_linear.0.bias", "pre_linear.1.weight",
                  "pre_linear.1.bias", "out.weight", "out.bias", "speaker_embedding.weight"):
            if d + k in st:
                self.p[k] = st[d + k].to(dtype).clone().requires_grad_(True)
        self.running_mean = st[d + "pre_linear.1.running_mean"].to(dtype).clone()
        self.running_var = st[d + "pre_linear.1.running_var"].to(dtype).clone()
        self.nbt = int(st[d + "pre_linear.1.num_batches_tracked"])
        self.H = self.p["out.weight"].shape[1]

    def __call__(self, in_text, in_lengths, poses, vid_indices=None, z=None, training=True, masks=None):
        """in_text (B, T) int64; poses (B, n_frames, P); masks: None or one {layer: (B, 1, H)} dict per decoded frame (decoder GRU inter-layer
        dropout).  Returns outputs (B, n_frames, P)."""
        p, H = self.p, self.H
        poses = poses.to(self.dtype)
        enc_out, enc_hidden = self.enc(in_text.t(), [int(v) for v in in_lengths])
        enc_bt = enc_out.transpose(0, 1)
        hidden = enc_hidden[:self.n_layers]
        outs, dec_in = [poses[:, 0]], poses[:, 0]
        for t in range(1, self.n_frames):
            x_in = dec_in if z is None else torch.cat([dec_in, z.to(self.dtype)], 1)
            out, hidden, _ = self.step(x_in, hidden, enc_bt, vid_indices, training, None if masks is None else masks[t - 1])
            outs.append(out)
            dec_in = poses[:, t] if t < self.n_pre else out
        return torch.stack(outs, 1)

    def step(self, motion_input, hidden, enc_bt, vid_indices=None, training=True, mask=None):
        """One decoder step (seq2seq_net.py:140-187): motion_input (B, dim [+ noise]), hidden (n_layers, B, H), enc_bt (B, Te, H) ->
        (output (B, P), hidden, attention weights (B, Te))."""
        p, H = self.p, self.H
        keys = enc_bt @ p["attn.attn.weight"][:, H:].t() + p["attn.attn.bias"]
        q = hidden[-1] @ p["attn.attn.weight"][:, :H].t()
        w, ctx = attn_chain(q, keys, enc_bt, p["attn.v"])
        parts = [motion_input, ctx]
        if "speaker_embedding.weight" in p:
            parts.append(p["speaker_embedding.weight"][vid_indices])
        x = torch.cat(parts, 1) @ p["pre_linear.0.weight"].t() + p["pre_linear.0.bias"]
        if training:
            mean, var = x.mean(0), x.var(0, unbiased=False)
            n = x.shape[0]
            with torch.no_grad():
                self.running_mean = 0.9 * self.running_mean + 0.1 * mean
                self.running_var = 0.9 * self.running_var + 0.1 * var * (n / (n - 1) if n > 1 else float("nan"))
                self.nbt += 1
        else:
            mean, var = self.running_mean, self.running_var
        x = torch.relu((x - mean) / torch.sqrt(var + 1e-5) * p["pre_linear.1.weight"] + p["pre_linear.1.bias"])
        y, hidden = self.gru(x[:, None, :], None, hidden, mask)
        return y[:, 0] @ p["out.weight"].t() + p["out.bias"], hidden, w

    def grads(self):
        """Gradients under the reference's parameter names (zeros where none arrived)."""
        g = {"encoder." + k: v for k, v in self.enc.grads().items()}
        g.update({"decoder.decoder.gru." + k: v for k, v in self.gru.grads().items()})
        for k, v in self.p.items():
            g["decoder.decoder." + k] = torch.zeros_like(v) if v.grad is None else v.grad
        return g


def named_leaves(ref):
    """{reference parameter name: the leaf tensor the chain holds for it} of a RefSeq2Seq (what an optimiser over the chain steps)."""
    from gru_seq_ref import PARAM_KINDS
    out = {"encoder.embedding.weight": ref.enc.emb}
    for prefix, gru in (("encoder.gru.", ref.enc.gru), ("decoder.decoder.gru.", ref.gru)):
        for l, m in enumerate(gru.layers):
            for sfx in ("", "_reverse")[:gru.D]:
                for k in PARAM_KINDS:
                    out[f"{prefix}{k}_l{l}{sfx}"] = getattr(m, f"{k}_l0{sfx}")
    out.update({"decoder.decoder." + k: v for k, v in ref.p.items()})
    return out


def train_steps(ref, batches, lens, weights, lr=1e-3, betas=(0.5, 0.999), max_norm=5.0):
    """train_iter_seq2seq on the chain for each (text, poses) of `batches`: zero_grad, forward, custom_loss, backward, clip_grad_norm_, Adam.
    Returns the losses; the parameters are named_leaves(ref)."""
    leaves = list(named_leaves(ref).values())
    optim = torch.optim.Adam(leaves, lr=lr, betas=betas)
    losses = []
    for text, poses in batches:
        optim.zero_grad()
        loss, _ = custom_loss(ref(text, lens, poses, training=True), poses.to(ref.dtype), *weights)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, max_norm)
        optim.step()
        losses.append(float(loss))
    return losses
