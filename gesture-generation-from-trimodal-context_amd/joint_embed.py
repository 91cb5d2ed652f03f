"""The joint-embedding baseline (model/embedding_net.py:130-162, 220-314, train_eval/train_joint_embed.py) on the HIP path: ContextEncoder,
PoseDecoderGRU, the speech / random modes of EmbeddingNet and their training step.

The classes keep the reference's constructor signatures, attribute names and state_dict keys (reference checkpoints load strictly).  All
arithmetic runs in libtrimodal_hip.so; torch is plumbing (parameter containers, views, the autograd bridge):
  * text and audio encoders: the stages of engine.GeneratorEngine (_text_fwd / _audio_fwd and their backwards) -- the kernels PoseGenerator
    runs, reached through a stage object that takes its parameters from the autograd function instead of a slab;
  * both GRUs: rnn.GRU (csrc/gru_seq.hip admits H = 256 x 1 direction and H = 300 x 2 directions);
  * the latent heads (ContextEncoder.out + fc_mu / fc_logvar + reparameterize, PoseDecoderGRU.pre_pose_net): tg_latent_head_fwd / _bwd, one
    launch each way (csrc/latent_head.hip);
  * the pose encoder: engine.AutoencoderEngine.encode / encode_backward; with variational_encoding=True its fc_mu / fc_logvar /
    reparameterisation tail is tg_vae_latent_fwd / _bwd and the KL term of the training step tg_vae_kld (csrc/vae_latent.hip).
CPU tensors raise TypeError, shapes outside a kernel envelope raise ValueError: there is no torch fallback.  init_model /
checkpoint.load_checkpoint_and_model keep refusing args.model == 'joint_embedding'; this module's build_model / load_checkpoint_and_model
are the entry points.
"""
import random

import torch
import torch.nn as nn

from . import layers as L
from . import ops
from .autograd_fns import L1MeanFn, LinearFn, RepeatRowsFn
from .engine import AutoencoderEngine, DeviceRNG, GeneratorEngine
from .layers import need_cuda
from .modules import EmbeddingNet, _need_cuda_variational, _TextEncoderParams, _WavEncoderParams
from .optim import ParamAdam, adopt
from .rnn import GRU, _SumHalvesFn


# ------------------------------------------------------------------------------------------------------------------ engine stages
class _GeneratorStages(GeneratorEngine):
    """GeneratorEngine's text / audio encoder stages without a parameter slab: P, G and the buffers are handed in per call."""

    def __init__(self, n_layers, p_drop):
        self.n_layers, self.p_drop = n_layers, p_drop
        self.use_audio = self.use_text = True
        self.c_audio, self.c_text = 0, 32             # ContextEncoder concatenates (audio, text): embedding_net.py:250
        self._side_work_ran = False
        self._rng_obj = None

    @property
    def rng(self):
        return self._rng_obj


class _AutoencoderStages(AutoencoderEngine):
    def __init__(self):
        self._views = None

    def views(self):
        return self._views


class _ContextFrontFn(torch.autograd.Function):
    """audio (B, samples), word ids (B, T) -> (B, T, 64) = [WavEncoder features | TextEncoderTCN features]."""

    @staticmethod
    def forward(ctx, cfg, in_audio, *params):
        stages, names, buffers, in_text, training, inject, save, embed_frozen = cfg
        P = dict(zip(names, params))
        B, T = in_text.shape
        in_data = L.empty(B, T, 64, like=in_audio)
        tp = {"in_text": in_text}
        stages._audio_fwd(P, buffers, in_audio, in_data, 0, tp, L.Fork(in_audio.device, enabled=False), training, 1)
        stages._text_fwd(P, in_text, in_data, tp, training, inject, "c", save)
        ctx.saved = (stages, names, P, tp, B, T, embed_frozen) if save else None
        return in_data

    @staticmethod
    def backward(ctx, d_in):
        if ctx.saved is None:
            raise NotImplementedError("ContextEncoder: the forward ran without a tape")
        stages, names, P, tp, B, T, embed_frozen = ctx.saved
        G = {n: ops.zeros_like(P[n]) for n in names}
        d_in = d_in.contiguous()
        stages._audio_bwd(P, G, tp, d_in[:, :, :32], 0, B, 0)
        stages._text_bwd(P, G, tp, d_in.view(B * T, 64)[:, 32:], slice(0, B), B * T, B, T, embed_frozen)
        return (None, None) + tuple(G[n] if ctx.needs_input_grad[2 + i] else None for i, n in enumerate(names))


class _PoseEncoderFn(torch.autograd.Function):
    """PoseEncoderConv (embedding_net.py:42-82) through AutoencoderEngine.encode: poses (B, 34, D) -> (z, mu, logvar).  variational False:
    z IS mu (one tensor, returned twice); True: z = mu + eps exp(logvar / 2) from ops.vae_latent_fwd, eps injected or drawn by the launch."""

    @staticmethod
    def forward(ctx, cfg, poses, *params):
        names, buffers, training, save, variational, eps, draw = cfg
        P = {"pose_encoder." + n: p for n, p in zip(names, params)}
        st = _AutoencoderStages()
        st._views = (P, None, {"pose_encoder." + k: v for k, v in buffers.items()})
        tape = {} if save else None
        ctx.saved = (st, names, P, tape, variational)
        ctx.set_materialize_grads(False)
        if variational:
            return st.encode(poses, training=training, tape=tape, variational=True, eps=eps, draw=draw)
        mu, logvar = st.encode(poses, training=training, tape=tape)
        return mu.view_as(mu), mu, logvar

    @staticmethod
    def backward(ctx, dz, dmu, dlv):
        st, names, P, tape, variational = ctx.saved
        if tape is None:
            raise NotImplementedError("pose encoder: the forward ran without a tape")
        if dlv is not None and not variational:
            raise ValueError("pose encoder: a gradient through logvar needs variational_encoding=True (fc_logvar feeds nothing otherwise)")
        G = {n: ops.zeros_like(p) for n, p in P.items()}
        st._views = (P, G, st._views[2])
        cont = lambda t: None if t is None else t.contiguous()
        if variational:
            if dz is not None or dmu is not None or dlv is not None:
                st.encode_backward(tape, cont(dz), dlv=cont(dlv), dmu_direct=cont(dmu))
        elif dz is not None or dmu is not None:
            d = cont(dz if dz is not None else dmu)
            if dz is not None and dmu is not None:
                d = ops.axpy(cont(dmu), d.clone(), 1.0, True)
            st.encode_backward(tape, d)
        return (None, None) + tuple(G["pose_encoder." + n] if ctx.needs_input_grad[2 + i] else None for i, n in enumerate(names))


class _LatentHeadFn(torch.autograd.Function):
    """Linear -> BatchNorm1d -> act -> Linear [-> fc_mu / fc_logvar -> reparameterize] as ONE launch each way (ops.latent_head_fwd / _bwd).
    x: (B, K0), or (B, T, K0) with last_step (its last time step is read in place and the gradient lands in the last step of a zeroed
    tensor); cat (B, C) or None: the result is the left block of a (B, N2 + C) row whose right block is `cat`."""

    @staticmethod
    def forward(ctx, cfg, x, cat, *params):
        bn, training, slope, tail, last_step, eps, draw = cfg
        w1, b1, gamma, beta, w2, b2 = params[:6]
        xv = x[:, -1] if last_step else x
        B, N2 = xv.shape[0], w2.shape[0]
        C = 0 if cat is None else cat.shape[1]
        row = L.empty(B, N2 + C, like=x)
        if C:
            ops.copy2d(cat.contiguous(), row[:, N2:])
        tp = ops.latent_head_fwd(xv, w1, b1, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked, w2, b2, row[:, :N2],
                                 training=training, slope=slope, tail=params[6:10] if tail else None, eps=eps, draw=draw, bn_eps=bn.eps,
                                 momentum=bn.momentum)
        ctx.saved = (tp, params, tail, last_step, x, N2, C)
        ctx.set_materialize_grads(False)
        if tail:
            return row, tp.mu, tp.logvar
        return row

    @staticmethod
    def backward(ctx, drow, dmu=None, dlv=None):
        tp, params, tail, last_step, x, N2, C = ctx.saved
        w1, b1, gamma, beta, w2, b2 = params[:6]
        B = tp.dims[0]
        drow = ops.zeros(B, N2 + C, device=x.device) if drow is None else drow.contiguous()
        dx_full = dxv = None
        if ctx.needs_input_grad[1]:
            if last_step:
                dx_full = ops.zeros_like(x)
                dxv = dx_full[:, -1]
            else:
                dx_full = dxv = torch.empty_like(x)
        G = ops.latent_head_bwd(drow[:, :N2], tp, w1, gamma, beta, w2, tail=(params[6], params[8]) if tail else None,
                                dmu=None if dmu is None else dmu.contiguous(), dlv=None if dlv is None else dlv.contiguous(), dx=dxv)
        dcat = drow[:, N2:].contiguous() if (C and ctx.needs_input_grad[2]) else None
        order = ("w1", "b1", "gamma", "beta", "w2", "b2") + (("wmu", "bmu", "wlv", "blv") if tail else ())
        return (None, dx_full, dcat) + tuple(G[k] if ctx.needs_input_grad[3 + i] else None for i, k in enumerate(order))


# ------------------------------------------------------------------------------------------------------------------------ modules
def _head_params(seq, mu=None, logvar=None):
    ps = [seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias, seq[3].weight, seq[3].bias]
    if mu is not None:
        ps += [mu.weight, mu.bias, logvar.weight, logvar.bias]
    return ps


class ContextEncoder(nn.Module):
    """embedding_net.py:220-259.  forward(in_text (B, 34) int64, in_spec (B, samples)) -> (z, mu, logvar), z reparameterised in eval mode
    too; eps comes from `inject['c.eps']` or from the counter RNG `rng`.  Dropout of the text encoder: 0.3 in the TCN, 0.1 on the
    embedding (the reference's defaults, which ContextEncoder does not override); `tcn_dropout` / `emb_dropout` may be set to 0."""

    def __init__(self, args, n_frames, n_words, word_embed_size, word_embeddings):
        super().__init__()
        self.text_encoder = _TextEncoderParams(args, n_words, word_embed_size, word_embeddings, 0.3)
        self.audio_encoder = _WavEncoderParams()
        self.gru = GRU(32 + 32, hidden_size=256, num_layers=2, bidirectional=False, batch_first=True)
        # parameter containers: their forwards are never called
        self.out = nn.Sequential(nn.Linear(256, 128), nn.BatchNorm1d(128), nn.ReLU(inplace=True), nn.Linear(128, 32))
        self.fc_mu = nn.Linear(32, 32)
        self.fc_logvar = nn.Linear(32, 32)
        self.do_flatten_parameters = False
        self.n_layers = args.n_layers
        self.tcn_dropout, self.emb_dropout = 0.3, 0.1
        self.seed = 0
        self._rng = None

    def _front_names(self):
        seen, names = set(), []
        for n, p in self.named_parameters():
            if n.startswith(("text_encoder.", "audio_encoder.")) and id(p) not in seen:
                seen.add(id(p)); names.append(n)
        return names

    def rng(self, device):
        """The encoder's counter RNG on `device`, made on first use (forward's own): the one object forward advances and draws from."""
        if self._rng is None or self._rng.state.device != device:
            self._rng = DeviceRNG(self.seed, device)
        return self._rng

    def forward(self, in_text, in_spec, inject=None):
        need_cuda(in_text, "ContextEncoder: in_text", torch.int64); need_cuda(in_spec, "ContextEncoder: in_spec")
        if in_text.dim() != 2 or in_spec.dim() != 2 or in_spec.shape[0] != in_text.shape[0]:
            raise ValueError(f"ContextEncoder: in_text (B, T) and in_spec (B, samples) expected, got {tuple(in_text.shape)} and {tuple(in_spec.shape)}")
        B, T = in_text.shape
        if self.training and B == 1:
            raise ValueError("ContextEncoder: BatchNorm in train mode needs more than one clip")
        self.rng(in_spec.device)
        if inject is None:
            self._rng.advance()
        inject = dict(inject or {})
        if self.training and self.emb_dropout == 0 and "c.emb_drop" not in inject:
            inject["c.emb_drop"] = torch.ones(B, T, self.text_encoder.embedding.weight.shape[1], device=in_spec.device)
        elif self.training and self.emb_dropout not in (0, 0.1):
            raise NotImplementedError("ContextEncoder: the embedding dropout of the text-encoder stage is 0.1 (or off)")
        stages = _GeneratorStages(self.n_layers, self.tcn_dropout)
        stages._rng_obj = self._rng
        names = self._front_names()
        sd = dict(self.named_parameters())
        params = [sd[n] for n in names]
        save = self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        cfg = (stages, names, dict(self.named_buffers()), in_text.contiguous(), self.training, inject, save,
               not self.text_encoder.embedding.weight.requires_grad)
        feat = _ContextFrontFn.apply(cfg, in_spec.contiguous(), *params)
        output, _ = self.gru(feat)
        eps = inject.get("c.eps")
        draw = None if eps is not None else (self._rng.state, self._rng.site("c.eps"))
        hcfg = (self.out[1], self.training, 0.0, True, True, None if eps is None else eps.contiguous(), draw)
        z, mu, logvar = _LatentHeadFn.apply(hcfg, output, None, *_head_params(self.out, self.fc_mu, self.fc_logvar))
        return z, mu, logvar


class PoseDecoderGRU(nn.Module):
    """embedding_net.py:130-162.  forward(latent_code (B, 32), pre_poses (B, 4, pose_dim)) -> (B, gen_length, pose_dim).  Inter-layer GRU
    dropout 0.3 in train mode; parity tests queue {'g.gru.drop<l>': mask} in `gru._replay_draws`."""

    def __init__(self, gen_length, pose_dim):
        super().__init__()
        self.gen_length, self.pose_dim = gen_length, pose_dim
        self.in_size, self.hidden_size = 32 + 32, 300
        self.pre_pose_net = nn.Sequential(nn.Linear(pose_dim * 4, 32), nn.BatchNorm1d(32), nn.ReLU(), nn.Linear(32, 32))
        self.gru = GRU(self.in_size, hidden_size=self.hidden_size, num_layers=4, batch_first=True, bidirectional=True, dropout=0.3)
        # LeakyReLU(True) has negative_slope 1: the identity (out.1 holds no parameters)
        self.out = nn.Sequential(nn.Linear(self.hidden_size, self.hidden_size // 2), nn.LeakyReLU(True), nn.Linear(self.hidden_size // 2, pose_dim))

    def forward(self, latent_code, pre_poses):
        need_cuda(latent_code, "PoseDecoderGRU: latent_code"); need_cuda(pre_poses, "PoseDecoderGRU: pre_poses")
        B = pre_poses.shape[0]
        if self.training and B == 1:
            raise ValueError("PoseDecoderGRU: BatchNorm in train mode needs more than one clip")
        pre = pre_poses.reshape(B, -1).contiguous()
        if pre.shape[1] != self.pre_pose_net[0].in_features or tuple(latent_code.shape) != (B, 32):
            raise ValueError(f"PoseDecoderGRU: pre_poses {tuple(pre_poses.shape)} / latent_code {tuple(latent_code.shape)} do not match the network")
        hcfg = (self.pre_pose_net[1], self.training, 0.0, False, False, None, None)
        feat = _LatentHeadFn.apply(hcfg, pre, latent_code, *_head_params(self.pre_pose_net))          # (B, 64) = [pre_pose_feat | latent]
        output, _ = self.gru(RepeatRowsFn.apply(feat, self.gen_length))
        o = _SumHalvesFn.apply(output).view(B * self.gen_length, self.hidden_size)
        o = LinearFn.apply(LinearFn.apply(o, self.out[0].weight, self.out[0].bias), self.out[2].weight, self.out[2].bias)
        return o.view(B, self.gen_length, -1)

    def forward_constant(self, latent_code, pre_poses):
        """forward in eval mode for at most four clips WITHOUT materialising the repeated input: the GRU is told that its input is one row
        (rnn.GRU.forward_constant: layer 0 projects (B, 64) instead of (B * gen_length, 64) and its recurrence reads one gi row per clip);
        no tg_repeat_rows launch.  Same head, direction sum and output MLP as forward.  Raises ValueError where forward_constant does."""
        if self.training:
            raise ValueError("PoseDecoderGRU.forward_constant runs in eval mode only: call .eval() first")
        need_cuda(latent_code, "PoseDecoderGRU: latent_code"); need_cuda(pre_poses, "PoseDecoderGRU: pre_poses")
        B = pre_poses.shape[0]
        pre = pre_poses.reshape(B, -1).contiguous()
        if pre.shape[1] != self.pre_pose_net[0].in_features or tuple(latent_code.shape) != (B, 32):
            raise ValueError(f"PoseDecoderGRU: pre_poses {tuple(pre_poses.shape)} / latent_code {tuple(latent_code.shape)} do not match the network")
        with torch.no_grad():
            hcfg = (self.pre_pose_net[1], False, 0.0, False, False, None, None)
            feat = _LatentHeadFn.apply(hcfg, pre, latent_code, *_head_params(self.pre_pose_net))      # (B, 64) = [pre_pose_feat | latent]
            output, _ = self.gru.forward_constant(feat, self.gen_length)
            o = _SumHalvesFn.apply(output).view(B * self.gen_length, self.hidden_size)
            o = LinearFn.apply(LinearFn.apply(o, self.out[0].weight, self.out[0].bias), self.out[2].weight, self.out[2].bias)
        return o.view(B, self.gen_length, -1)


def embedding_forward(net, in_text, in_audio, pre_poses, poses, input_mode=None, variational_encoding=False):
    """EmbeddingNet.forward of the speech / random modes (embedding_net.py:276-308)."""
    if variational_encoding and poses is not None:
        _need_cuda_variational(poses, "EmbeddingNet: poses")
    if input_mode is None:
        assert net.mode is not None
        input_mode = net.mode
    inject = net._replay_draws.pop(0) if net._replay_draws else None
    if inject is not None and net.training:
        masks = {k: v for k, v in inject.items() if k.startswith("g.gru.drop")}
        if masks:
            net.decoder.gru._replay_draws.append(masks)
    context_feat = context_mu = context_logvar = None
    if net.context_encoder is not None and in_text is not None and in_audio is not None:
        context_feat, context_mu, context_logvar = net.context_encoder(in_text, in_audio.float(), inject=inject)
    poses_feat = pose_mu = pose_logvar = None
    if poses is not None:
        need_cuda(poses, "EmbeddingNet: poses")
        if net.training and poses.shape[0] == 1:
            raise ValueError("EmbeddingNet: BatchNorm in train mode needs more than one clip")
        enc = net.pose_encoder
        names = [n for n, _ in enc.named_parameters()]
        params = [p for _, p in enc.named_parameters()]
        save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        eps = draw = None
        if variational_encoding:
            # the flag reaches the pose encoder only (the context encoder reparameterises regardless), in train and in eval mode alike
            # (embedding_net.py:77-80); eps: injected under 'p.eps' or drawn by the launch from the net's RNG at the site of that name
            eps = None if inject is None else inject.get("p.eps")
            if eps is None:
                rng = getattr(net, "_pose_rng", None)
                if rng is None or rng.state.device != poses.device:
                    rng = DeviceRNG(getattr(net, "seed", 0), poses.device)
                    object.__setattr__(net, "_pose_rng", rng)
                rng.advance()
                draw = (rng.state, rng.site("p.eps"))
            else:
                eps = eps.contiguous()
        cfg = (names, dict(enc.named_buffers()), net.training, save, bool(variational_encoding), eps, draw)
        poses_feat, pose_mu, pose_logvar = _PoseEncoderFn.apply(cfg, poses.contiguous(), *params)     # variational_encoding=False: z = mu
    if input_mode == "random":
        input_mode = "speech" if random.random() > 0.5 else "pose"               # the host RNG, exactly as the reference draws it
    if input_mode == "speech":
        latent_feat = context_feat
    elif input_mode == "pose":
        latent_feat = poses_feat
    else:
        raise ValueError(f"input_mode {input_mode!r}")
    if latent_feat is None:
        raise ValueError(f"EmbeddingNet: input_mode {input_mode!r} needs its encoder's inputs")
    out_poses = net.decoder(latent_feat, pre_poses.float())
    return context_feat, context_mu, context_logvar, poses_feat, pose_mu, pose_logvar, out_poses


def embedding_synthesize(net, in_text, in_audio, pre_poses, inject=None, constant_input=False):
    """EmbeddingNet.synthesize: the 'speech' path of embedding_net.py:276-308 in eval mode, (B, n_frames, pose_dim).  The pose encoder is not
    run (in eval mode it has no side effect and 'speech' does not read its output).  Both GRUs are switched to rnn.GRU.few_row_eval: with
    B <= 4 each of their layers is one few-row recurrence launch (csrc/gru_vec.hip) instead of one launch per time step; larger batches
    stay on the per-step kernels.  ContextEncoder reparameterises in eval mode too: eps from inject['c.eps'] or the counter RNG, as forward.
    constant_input=True (opt-in, at most four clips): the decoder runs PoseDecoderGRU.forward_constant -- no repeated input, layer 0 of its GRU
    on the constant-input recurrence; the default keeps today's launches and bits."""
    if net.context_encoder is None:
        raise ValueError("EmbeddingNet.synthesize: mode='pose' has no context encoder")
    if net.training:
        raise RuntimeError("EmbeddingNet.synthesize runs in eval mode: call .eval() / .train(False) first")
    net.context_encoder.gru.few_row_eval = True
    net.decoder.gru.few_row_eval = True
    with torch.no_grad():
        latent, _, _ = net.context_encoder(in_text, in_audio.float(), inject=inject)
        if constant_input:
            return net.decoder.forward_constant(latent, pre_poses.float())
        return net.decoder(latent, pre_poses.float())


# ----------------------------------------------------------------------------------------------------------------------- training
class JointEmbedTrainer:
    """train_iter_embed with the device Adam (optim.ParamAdam): forward (both encoders), the summed per-clip L1 (L1MeanFn times B),
    backward, Adam on every parameter that received a gradient."""

    def __init__(self, net, lr=5e-4, betas=(0.5, 0.999), eps=1e-8):
        self.net = net
        self.adam = ParamAdam(net.parameters(), lr, betas, eps)
        self.step_dev = self.adam.step_dev
        self._bscale = {}                    # device constants by (value, device, dtype)

    def set_hparams(self, lr, betas, eps):
        self.adam.set_hparams(lr, betas, eps)

    def _const(self, value, dev, dtype=torch.float32):
        key = (float(value), dev, dtype)
        if key not in self._bscale:
            self._bscale[key] = torch.full((1,), float(value), device=dev, dtype=dtype)
        return self._bscale[key]

    def step(self, args, epoch, in_text, in_audio, target_data, mode=None, variational_encoding=False):
        """-> the recon loss as a device float [1]; with variational_encoding (loss, KLD) as ONE packed device buffer of two 8-byte slots
        (slot 0: the fp32 loss in its first four bytes, slot 1: the fp64 KLD) -- read with unpack_scalars, one copy to the host."""
        target = target_data.float().contiguous()
        B, dev = target.shape[0], target.device
        self.adam.zero_grad()
        pre_seq = target[:, 0:args.n_pre_poses]
        out = self.net(in_text, in_audio, pre_seq, target, mode, variational_encoding=variational_encoding)
        if not variational_encoding:
            loss = L1MeanFn.apply(out[6].contiguous(), target, self._const(B, dev))
            loss.backward()
            packed = loss.detach()
        else:
            packed = torch.empty(2, device=dev, dtype=torch.float64)
            loss = L1MeanFn.apply(out[6].contiguous(), target, self._const(B, dev), [packed[0:1].view(torch.float32)[0:1]])
            # train_joint_embed.py:30-40: the context latent's KL term when the NET's mode is 'speech', the pose latent's otherwise
            mu, logvar = (out[1], out[2]) if self.net.mode == "speech" else (out[4], out[5])
            if mu is None:
                raise ValueError(f"train_iter_embed: the KL term of a net with mode {self.net.mode!r} needs that encoder's inputs")
            kld = _KldFn.apply(mu, logvar, [packed[1:2]])
            # loss = loss_regression_weight * recon + KLD_weight * KLD: the two weights enter as the seeds of one backward pass
            torch.autograd.backward([loss, kld], [self._const(args.loss_regression_weight, dev),
                                                  self._const(embed_kld_weight(epoch, args.loss_kld_weight), dev, torch.float64)])
            packed = packed.detach()
        self.adam.step()
        return packed


def embed_kld_weight(epoch, loss_kld_weight):
    """train_joint_embed.py:37-40: 0 before epoch 10, then (epoch - 10) * loss_kld_weight, capped at 1."""
    return 0.0 if epoch < 10 else min(1.0, (epoch - 10) * loss_kld_weight)


def unpack_scalars(packed):
    """The (fp32 loss, fp64 KLD) pair of a packed two-slot device buffer: one copy to the host."""
    host = packed.cpu()
    return float(host[0:1].view(torch.float32)[0]), float(host[1])


class _KldFn(torch.autograd.Function):
    """KLD = -0.5 sum(1 + logvar - mu^2 - exp(logvar)) of a latent (fp64 device scalar, written into out[0]: a one-element list, as
    L1MeanFn's), value and gradient from ONE launch (ops.vae_kld); the backward scales the stored gradient by the incoming one (a device
    scalar: no host read)."""

    @staticmethod
    def forward(ctx, mu, logvar, out):
        kld, dmu, dlv = ops.vae_kld(mu.contiguous(), logvar.contiguous(), weight=1.0, kld=out[0])
        ctx.saved = (dmu, dlv)
        return kld

    @staticmethod
    def backward(ctx, g):
        dmu, dlv = ctx.saved
        g = g.float().contiguous().view(1)
        return ops.scale_by(dmu, g), ops.scale_by(dlv, g), None


def train_iter_embed(args, epoch, in_text, in_audio, target_data, net, optim, mode=None, *, variational_encoding=False):
    """The reference's signature and return dict (train_joint_embed.py:5-51).  variational_encoding is False on both of the reference's
    branches, so by default there is no KLD term; True (keyword only) is the reference with that literal flipped:
    loss = args.loss_regression_weight * recon + KLD_weight * KLD, KLD_weight = embed_kld_weight(epoch, args.loss_kld_weight), and the dict
    is {'loss': recon, 'KLD': KLD}, both unweighted as there.  One host read: the returned float (the packed pair with the KL term).
    The JointEmbedTrainer is kept on `optim` (optim.adopt: a plain torch.optim.Adam, whose hyper-parameters alone are used): every parameter
    of `net` that received a gradient is stepped (as Adam over net.parameters() does, which skips parameters without one)."""
    tr, g = adopt(optim, "_joint_embed_trainer", "train_iter_embed", lambda: JointEmbedTrainer(net), lambda t: t.net is net)
    tr.set_hparams(g["lr"], g["betas"], g["eps"])
    if not variational_encoding:
        return {"loss": tr.step(args, epoch, in_text, in_audio, target_data, mode).item()}
    loss, kld = unpack_scalars(tr.step(args, epoch, in_text, in_audio, target_data, mode, variational_encoding=True))
    return {"loss": loss, "KLD": kld}


# -------------------------------------------------------------------------------------------------------------------- checkpoints
def build_model(args, lang_model, pose_dim, device):
    """train.py:41-44 for model == 'joint_embedding': (EmbeddingNet(mode='random'), None, None)."""
    generator = EmbeddingNet(args, pose_dim, args.n_poses, lang_model.n_words, args.wordembed_dim, lang_model.word_embedding_weights,
                             mode="random").to(device)
    return generator, None, None


def load_checkpoint_and_model(checkpoint_path, _device="cpu"):
    """checkpoint.load_checkpoint_and_model for a 'joint_embedding' checkpoint: (args, generator in eval mode, loss_fn, lang_model,
    speaker_model, pose_dim).  The state dict loads strictly."""
    from .checkpoint import load_checkpoint
    ck = load_checkpoint(checkpoint_path, _device)
    args, lang_model, speaker_model, pose_dim = ck["args"], ck["lang_model"], ck["speaker_model"], ck["pose_dim"]
    if args.model != "joint_embedding":
        raise ValueError(f"joint_embed.load_checkpoint_and_model: the checkpoint holds model {args.model!r}; use checkpoint.load_checkpoint_and_model")
    generator, _, loss_fn = build_model(args, lang_model, pose_dim, _device)
    generator.load_state_dict(ck["gen_dict"], strict=True)
    generator.train(False)
    return args, generator, loss_fn, lang_model, speaker_model, pose_dim
