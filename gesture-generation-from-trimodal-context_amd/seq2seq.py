"""The Seq2Seq baseline (model/seq2seq_net.py, train_eval/train_seq2seq.py) on the HIP path: Bahdanau attention decoder, Seq2SeqNet and its
training step.

The classes keep the reference's constructor and forward signatures, attribute names and state_dict keys (state dicts load strictly both
ways).  All arithmetic runs in libtrimodal_hip.so: the attention step kernels of csrc/attn.hip, tg_gemm_nt / tg_gemm_tn, the BatchNorm
kernels, the general GRU recurrence (T = 1 with h0) and the loss / clip kernels of csrc/losses.hip; torch is plumbing (parameter containers,
copies into the concatenated inputs, the autograd bridge).  CPU tensors raise TypeError, shapes outside a kernel envelope raise ValueError:
there is no torch fallback.  Not implemented: discrete_representation=True.

In eval mode the decoder loop is row-local (BatchNorm on running statistics, no dropout) and runs as ONE launch, tg_seq2seq_decode_eval
(csrc/seq2seq_decode.hip), which also takes a per-row encoder length: Seq2SeqNet.synthesize() gives every row of a padded batch the result of
its own B = 1 run, as the reference synthesises.  FUSED_EVAL_DECODE = False keeps eval mode on the per-step path.
"""
import math

import torch
import torch.nn as nn

from . import layers as L
from . import ops
from .layers import need_cuda
from .ops import Win
from .optim import ParamAdam, adopt
from .rnn import GRU, EncoderRNN, _EmbedFn


# eval-mode decode through the one-launch kernel (csrc/seq2seq_decode.hip) where the shape is inside its envelope; False: the per-step path of
# _DecodeFn (benchmarks and parity tests compare the two).  Train mode never takes the kernel.
FUSED_EVAL_DECODE = True


class Attn(nn.Module):
    """Parameter container of the additive attention (seq2seq_net.py:59-89); `attn` is Linear(2H, H) over [hidden ; encoder output], `v` the
    score vector.  forward(hidden (B, H), encoder_outputs (T, B, H)) -> attention weights (B, 1, T), no gradient (the decoder's autograd
    function runs the differentiable form)."""

    def __init__(self, hidden_size):
        super().__init__()
        self.hidden_size = hidden_size
        self.attn = nn.Linear(self.hidden_size * 2, hidden_size)
        self.v = nn.Parameter(torch.rand(hidden_size))
        stdv = 1. / math.sqrt(self.v.size(0))
        self.v.data.normal_(mean=0, std=stdv)

    def forward(self, hidden, encoder_outputs):
        need_cuda(hidden, "Attn: hidden"); need_cuda(encoder_outputs, "Attn: encoder_outputs")
        H = self.hidden_size
        with torch.no_grad():
            enc = encoder_outputs.transpose(0, 1).contiguous()
            B, Te, _ = enc.shape
            _need_attn(B, Te, H)
            wa = self.attn.weight
            keys = ops.gemm_nt(Win.plain(enc.view(B * Te, H)), wa[:, H:], self.attn.bias, L.empty(B * Te, H, like=enc)).view(B, Te, H)
            q = ops.gemm_nt(Win.plain(hidden.contiguous()), wa[:, :H], None, L.empty(B, H, like=enc))
            w, _ = ops.attn_step_forward(q, keys, enc, self.v.detach(), L.empty(B, Te, like=enc), L.empty(B, H, like=enc))
        return w.unsqueeze(1)


def _need_attn(B, Te, H):
    if not ops.attn_step_supported(B, Te, H):
        raise ValueError(f"Seq2Seq attention: (B, Te, H) = {(B, Te, H)} is outside the HIP kernel envelope {ops.ATTN_ENVELOPE}; there is no torch fallback")
    if not ops.gru_seq_supported(B, 1, H, 1):
        raise ValueError(f"Seq2Seq decoder GRU: (B, T, H, D) = {(B, 1, H, 1)} is outside the HIP kernel envelope {ops.GRU_SEQ_ENVELOPE}")


_DEC_NAMES = ("attn.attn.weight", "attn.attn.bias", "attn.v", "pre_linear.0.weight", "pre_linear.0.bias", "pre_linear.1.weight", "pre_linear.1.bias",
              "out.weight", "out.bias")


class _DecodeFn(torch.autograd.Function):
    """The whole autoregressive decoder loop (seq2seq_net.py:241-252) behind one autograd node.

    forward: keys = enc W_e^T + b_a once, then per frame q = h_top W_h^T, the attention step (context written straight into the concatenated
    pre_linear input), Linear + BatchNorm + ReLU, the GRU stack with T = 1 from the previous state, Linear out.  Taped per step: the
    concatenated input, q, the attention weights, h_top, the pre-BatchNorm activations with their statistics, the GRU tape, the GRU output.
    backward: the loop reversed, carrying the state gradient and the feedback gradient of frames the model fed to itself; the gradients of
    W_h, pre_linear.0 and out are ONE tg_gemm_tn each over the steps stacked along the rows, after the loop; W_e, b_a and the encoder-output
    gradient come from the accumulated key gradient.  The decoder GRU's weight gradients accumulate step by step through
    layers.gru_seq_stack_bwd, which forms them from its own tape."""

    @staticmethod
    def forward(ctx, cfg, enc, h0, poses, z, spk, *params):
        dec, n_frames, n_pre, training, rng, injects, save = cfg
        gnames = tuple(dec.gru._names)
        P = dict(zip(_DEC_NAMES + gnames, params))
        H, nl = dec.hidden_size, dec.n_layers
        B, Te, _ = enc.shape
        Pd = poses.shape[2]
        Z = 0 if z is None else z.shape[1]
        S8 = 0 if spk is None else spk.shape[1]
        c0, Lin = Pd + Z, Pd + Z + H + S8
        S, Po = n_frames - 1, P["out.weight"].shape[0]
        assert Po == Pd or S == 1, "the decoder feeds its own output back: output_size must equal the pose width"
        wa = P["attn.attn.weight"]
        w_h, w_e = wa[:, :H].contiguous(), wa[:, H:].contiguous()
        keys = ops.gemm_nt(Win.plain(enc.view(B * Te, H)), w_e, P["attn.attn.bias"], L.empty(B * Te, H, like=enc)).view(B, Te, H)
        XIN, Q, WAT, HTOP = L.empty(S, B, Lin, like=enc), L.empty(S, B, H, like=enc), L.empty(S, B, Te, like=enc), L.empty(S, B, H, like=enc)
        PRE, ACT, Y, OUT = L.empty(S, B, H, like=enc), L.empty(S, B, H, like=enc), L.empty(S, B, H, like=enc), L.empty(S, B, Po, like=enc)
        if Z:
            XIN[:, :, Pd:c0] = z
        if S8:
            XIN[:, :, c0 + H:] = spk
        bn = dec.pre_linear[1]
        outputs = L.empty(B, n_frames, Po, like=enc)
        outputs[:, 0] = poses[:, 0, :Po]
        hidden, dec_in = h0, poses[:, 0]
        bn_states, tapes = [], []
        for s in range(S):
            t = s + 1
            XIN[s, :, :Pd] = dec_in
            HTOP[s] = hidden[nl - 1]
            ops.gemm_nt(Win.plain(HTOP[s]), w_h, None, Q[s])
            ops.attn_step_forward(Q[s], keys, enc, P["attn.v"], WAT[s], XIN[s][:, c0:c0 + H])
            ops.gemm_nt(Win.plain(XIN[s]), P["pre_linear.0.weight"], P["pre_linear.0.bias"], PRE[s])
            _, st = L.bn_fwd(PRE[s], P["pre_linear.1.weight"], P["pre_linear.1.bias"], bn.running_mean, bn.running_var, bn.num_batches_tracked,
                             training=training, act_slope=0.0, out=ACT[s])
            inject = injects[s] if injects is not None else None
            if rng is not None and inject is None:
                rng.advance()
            y, hidden, tape, _ = L.gru_seq_stack_fwd(ACT[s].view(B, 1, H), P, "", nl, H, 1, h0=hidden, p_drop=dec.dropout_p, training=training and nl > 1,
                                                     rng=rng, save=save, inject=inject)
            Y[s] = y.view(B, H)
            ops.gemm_nt(Win.plain(Y[s]), P["out.weight"], P["out.bias"], OUT[s])
            outputs[:, t] = OUT[s]
            dec_in = poses[:, t] if t < n_pre else OUT[s]
            bn_states.append(st); tapes.append(tape)
        if save:
            ctx.tape = (P, gnames, enc, keys, w_h, w_e, XIN, Q, WAT, HTOP, Y, bn_states, tapes, (B, Te, H, nl, Pd, Po, Z, S8, c0, Lin, S, n_pre))
        else:
            ctx.tape = None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(hidden, WAT)
        return outputs, hidden, WAT

    @staticmethod
    def backward(ctx, d_outputs, _d_hidden, _d_weights):
        if ctx.tape is None:
            raise NotImplementedError("Seq2Seq decoder: the forward ran without a tape (eval mode: gradients through BatchNorm on running "
                                      "statistics are not implemented)")
        P, gnames, enc, keys, w_h, w_e, XIN, Q, WAT, HTOP, Y, bn_states, tapes, dims = ctx.tape
        B, Te, H, nl, Pd, Po, Z, S8, c0, Lin, S, n_pre = dims
        names = _DEC_NAMES + gnames
        G = {n: ops.zeros_like(P[n]) for n in names}
        if d_outputs is None:
            return (None,) * 6 + tuple(G[n] for n in names)
        d_outputs = d_outputs.contiguous()
        DOUT, DPRE, DQ = L.empty(S, B, Po, like=enc), L.empty(S, B, H, like=enc), L.empty(S, B, H, like=enc)
        dkeys, denc, dv_rows = ops.zeros(B, Te, H, device=enc.device), ops.zeros(B, Te, H, device=enc.device), ops.zeros(B, H, device=enc.device)
        dz = ops.zeros(B, Z, device=enc.device) if Z else None
        dspk = ops.zeros(B, S8, device=enc.device) if S8 else None
        w_out_t, w_pre_t, w_h_t = L.transpose2d(P["out.weight"]), L.transpose2d(P["pre_linear.0.weight"]), L.transpose2d(w_h)
        dgamma, dbeta = G["pre_linear.1.weight"], G["pre_linear.1.bias"]
        dh, dfeed = None, None
        dy, dxin = L.empty(B, H, like=enc), L.empty(B, Lin, like=enc)
        for s in range(S - 1, -1, -1):
            t = s + 1
            DOUT[s] = d_outputs[:, t]
            if dfeed is not None:
                ops.axpy(dfeed, DOUT[s])
            ops.gemm_nt(Win.plain(DOUT[s]), w_out_t, None, dy)
            dx, dh = L.gru_seq_stack_bwd(dy.view(B, 1, H), dh, tapes[s], P, G, "", nl, need_dx=True, need_dh0=True)
            L.bn_bwd(dx.reshape(B, H), bn_states[s], P["pre_linear.1.weight"], P["pre_linear.1.bias"], dgamma, dbeta, out=DPRE[s])
            ops.gemm_nt(Win.plain(DPRE[s]), w_pre_t, None, dxin)
            ops.attn_step_backward(dxin[:, c0:c0 + H], Q[s], WAT[s], keys, enc, P["attn.v"], DQ[s], dkeys, denc, dv_rows)
            ops.gemm_nt(Win.plain(DQ[s]), w_h_t, None, dh[nl - 1], accumulate=True)
            if Z:
                ops.axpy(dxin[:, Pd:c0].contiguous(), dz)
            if S8:
                ops.axpy(dxin[:, c0 + H:].contiguous(), dspk)
            # the input of frame t was the model's own frame t - 1 when that frame is past the seed poses
            dfeed = dxin[:, :Pd].contiguous() if (t - 1 >= 1 and t - 1 >= n_pre) else None
        SB = S * B
        dwh, dwe = ops.zeros(H, H, device=enc.device), ops.zeros(H, H, device=enc.device)
        ops.gemm_tn(DOUT.view(SB, Po), Win.plain(Y.view(SB, H)), G["out.weight"], dbias=G["out.bias"])
        ops.gemm_tn(DPRE.view(SB, H), Win.plain(XIN.view(SB, Lin)), G["pre_linear.0.weight"], dbias=G["pre_linear.0.bias"])
        ops.gemm_tn(DQ.view(SB, H), Win.plain(HTOP.view(SB, H)), dwh)
        ops.gemm_tn(dkeys.view(B * Te, H), Win.plain(enc.view(B * Te, H)), dwe, dbias=G["attn.attn.bias"])
        G["attn.attn.weight"] = torch.cat((dwh, dwe), dim=1)
        ops.gemm_nt(Win.plain(dkeys.view(B * Te, H)), L.transpose2d(w_e), None, denc.view(B * Te, H), accumulate=True)
        ops.colsum(dv_rows, G["attn.v"], accumulate=True)
        ni = ctx.needs_input_grad
        return (None, denc if ni[1] else None, dh if ni[2] else None, None, dz if (Z and ni[4]) else None, dspk if (S8 and ni[5]) else None) + \
            tuple(G[n] if ni[6 + i] else None for i, n in enumerate(names))


class _FusedEvalDecodeFn(torch.autograd.Function):
    """The eval-mode loop as one launch.  Like the tape-less eval forward of _DecodeFn, it has a graph node only so that a backward through it
    raises instead of silently giving no gradients."""

    @staticmethod
    def forward(ctx, dec, n_frames, n_pre, enc_lengths, enc, h0, poses, z, spk, *params):
        P = dict(zip(_DEC_NAMES + tuple(dec.gru._names), params))
        B, Te, H = enc.shape
        wa, bn = P["attn.attn.weight"], dec.pre_linear[1]
        keys = ops.gemm_nt(Win.plain(enc.view(B * Te, H)), wa[:, H:], P["attn.attn.bias"], L.empty(B * Te, H, like=enc)).view(B, Te, H)
        gru = [tuple(P[f"{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(dec.n_layers)]
        outputs, h_n = L.empty(B, n_frames, dec.output_size, like=enc), L.empty(dec.n_layers, B, H, like=enc)
        wat = L.empty(n_frames - 1, B, Te, like=enc)
        ops.seq2seq_decode_eval(enc, keys, h0, poses, n_frames, n_pre, wa, P["attn.v"], P["pre_linear.0.weight"], P["pre_linear.0.bias"],
                                P["pre_linear.1.weight"], P["pre_linear.1.bias"], bn.running_mean, bn.running_var, bn.eps, gru, P["out.weight"],
                                P["out.bias"], outputs, h_n, wat, te_len=enc_lengths, z=z, spk=spk)
        ctx.mark_non_differentiable(h_n, wat)
        return outputs, h_n, wat

    @staticmethod
    def backward(ctx, *_grads):
        raise NotImplementedError("Seq2Seq decoder: the forward ran without a tape (eval mode: gradients through BatchNorm on running "
                                  "statistics are not implemented)")


class BahdanauAttnDecoderRNN(nn.Module):
    """seq2seq_net.py:92-187.  forward(motion_input (B, dim), last_hidden (n_layers, B, H), encoder_outputs (T, B, H), vid_indices=None) ->
    (output (B, output_size), hidden, attn_weights (B, 1, T)) runs ONE step without gradient (inference use; in train mode it advances the
    BatchNorm buffers, as the reference's step does); training goes through Seq2SeqNet.forward, whose autograd function owns the whole loop.  Train-mode inter-layer GRU dropout draws from the GRU's counter RNG;
    parity tests queue one dict of injected masks per decoded frame in `gru._replay_draws` (as rnn.GRU does per call)."""

    def __init__(self, input_size, hidden_size, output_size, n_layers=1, dropout_p=0.1, discrete_representation=False, speaker_model=None):
        super().__init__()
        if discrete_representation:
            raise NotImplementedError("BahdanauAttnDecoderRNN(discrete_representation=True) is not implemented on the HIP path")
        self.hidden_size, self.output_size, self.n_layers, self.dropout_p = hidden_size, output_size, n_layers, dropout_p
        self.discrete_representation, self.speaker_model = discrete_representation, speaker_model
        if self.speaker_model:
            self.speaker_embedding = nn.Embedding(speaker_model.n_words, 8)
        linear_input_size = input_size + hidden_size + (8 if self.speaker_model else 0)
        # parameter containers: their own forwards are never called
        self.pre_linear = nn.Sequential(nn.Linear(linear_input_size, hidden_size), nn.BatchNorm1d(hidden_size), nn.ReLU(inplace=True))
        self.attn = Attn(hidden_size)
        self.gru = GRU(hidden_size, hidden_size, n_layers, dropout=dropout_p)
        self.out = nn.Linear(hidden_size, output_size)
        self.do_flatten_parameters = False

    def freeze_attn(self):
        for param in self.attn.parameters():
            param.requires_grad = False

    def _params(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in _DEC_NAMES] + [getattr(self.gru, n) for n in self.gru._names]

    def decode(self, enc_bt, h0, poses, n_frames, n_pre, z=None, vid_indices=None, enc_lengths=None):
        """The loop of Seq2SeqNet.forward: enc_bt (B, Te, H), h0 (n_layers, B, H), poses (B, >= max(n_pre, 1), pose_dim) -> (outputs (B, n_frames,
        pose_dim), final hidden, attention weights (n_frames - 1, B, Te) without gradient).  enc_lengths (eval mode only): one encoder length
        per row; the row's softmax runs over its first enc_lengths[b] positions and the later weights are exact zeros.  None: all Te
        positions, padded ones included, as in training."""
        B, Te, H = enc_bt.shape
        _need_attn(B, Te, H)
        spk = None
        if self.speaker_model:
            assert vid_indices is not None
            spk = _EmbedFn.apply(self.speaker_embedding.weight, vid_indices.contiguous())
        if self.pre_linear[0].in_features != poses.shape[2] + (0 if z is None else z.shape[1]) + H + (8 if self.speaker_model else 0):
            raise ValueError("Seq2Seq decoder: pose / noise widths do not match pre_linear's input size")
        if not self.training:
            Z, S8 = 0 if z is None else z.shape[1], 0 if spk is None else spk.shape[1]
            if FUSED_EVAL_DECODE and ops.seq2seq_decode_supported(B, Te, H, self.n_layers, n_frames, n_pre, poses.shape[2], self.output_size, Z, S8):
                return _FusedEvalDecodeFn.apply(self, n_frames, n_pre, enc_lengths, enc_bt.contiguous(), h0.contiguous(), poses.contiguous(),
                                                None if z is None else z.contiguous(), spk, *self._params())
        if enc_lengths is not None and any(int(v) != Te for v in (enc_lengths.tolist() if isinstance(enc_lengths, torch.Tensor) else enc_lengths)):
            raise ValueError("Seq2Seq decoder: the per-step path has no per-row encoder lengths (they need eval mode, seq2seq.FUSED_EVAL_DECODE "
                             f"and a shape inside {ops.SEQ2SEQ_DECODE_ENVELOPE})")
        params = self._params()
        training = self.training
        S = n_frames - 1
        injects, rng = None, None
        if training and self.n_layers > 1:
            if self.gru._replay_draws:
                injects = [self.gru._replay_draws.pop(0) for _ in range(S)]
            elif self.dropout_p > 0:
                if self.gru._rng is None:
                    from .engine import DeviceRNG
                    self.gru._rng = DeviceRNG(self.gru.seed, enc_bt.device)
                rng = self.gru._rng
        # eval mode runs without a tape whatever the grad mode (the reference's eval forward works outside no_grad too); only a backward
        # through such a forward raises
        save = training and torch.is_grad_enabled() and (enc_bt.requires_grad or h0.requires_grad or any(p.requires_grad for p in params))
        cfg = (self, n_frames, n_pre, training, rng, injects, save)
        return _DecodeFn.apply(cfg, enc_bt.contiguous(), h0.contiguous(), poses.contiguous(), z, spk, *params)

    def decode_eval_static(self, enc_bt, h0, poses, n_frames, n_pre, te_len, outputs):
        """The eval-mode loop of decode() for a window on static buffers (synthesize.Seq2SeqWindowDecoder): te_len is a device int64 (B,)
        tensor handed to the kernel unread, outputs (B, n_frames, output_size) is written in place; no speaker, no noise, no attention
        weights.  The arithmetic is _FusedEvalDecodeFn's: the keys by the same GEMM entry, then tg_seq2seq_decode_eval.  Returns h_n."""
        B, Te, H = enc_bt.shape
        if self.training or self.speaker_model:
            raise ValueError("Seq2Seq decoder: decode_eval_static runs in eval mode, without a speaker model")
        if not ops.seq2seq_decode_supported(B, Te, H, self.n_layers, n_frames, n_pre, poses.shape[2], self.output_size, 0, 0):
            raise ValueError(f"Seq2Seq decoder: (B, Te, H, n_layers, n_frames, n_pre, Pd, Po) = "
                             f"{(B, Te, H, self.n_layers, n_frames, n_pre, poses.shape[2], self.output_size)} is outside the kernel envelope "
                             f"{ops.SEQ2SEQ_DECODE_ENVELOPE}")
        if self.pre_linear[0].in_features != poses.shape[2] + H:
            raise ValueError("Seq2Seq decoder: pose width does not match pre_linear's input size")
        P = dict(zip(_DEC_NAMES + tuple(self.gru._names), (p.detach() for p in self._params())))
        wa, bn = P["attn.attn.weight"], self.pre_linear[1]
        keys = ops.gemm_nt(Win.plain(enc_bt.view(B * Te, H)), wa[:, H:], P["attn.attn.bias"], L.empty(B * Te, H, like=enc_bt)).view(B, Te, H)
        gru = [tuple(P[f"{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(self.n_layers)]
        h_n = L.empty(self.n_layers, B, H, like=enc_bt)
        ops.seq2seq_decode_eval(enc_bt, keys, h0, poses, n_frames, n_pre, wa, P["attn.v"], P["pre_linear.0.weight"], P["pre_linear.0.bias"],
                                P["pre_linear.1.weight"], P["pre_linear.1.bias"], bn.running_mean, bn.running_var, bn.eps, gru, P["out.weight"],
                                P["out.bias"], outputs, h_n, None, te_len=te_len, te_len_as_is=True)
        return h_n

    def forward(self, motion_input, last_hidden, encoder_outputs, vid_indices=None):
        need_cuda(motion_input, "BahdanauAttnDecoderRNN: motion_input")
        with torch.no_grad():
            enc = encoder_outputs.transpose(0, 1).contiguous()
            out, hidden, w = self.decode(enc, last_hidden, motion_input.unsqueeze(1), 2, 1, None, vid_indices)
        return out[:, 1], hidden, w[0].unsqueeze(1)


class Generator(nn.Module):
    """seq2seq_net.py:190-214."""

    def __init__(self, args, motion_dim, discrete_representation=False, speaker_model=None):
        super().__init__()
        self.output_size = motion_dim
        self.n_layers = args.n_layers
        self.discrete_representation = discrete_representation
        self.decoder = BahdanauAttnDecoderRNN(input_size=motion_dim + args.GAN_noise_size, hidden_size=args.hidden_size,
                                              output_size=self.output_size, n_layers=self.n_layers, dropout_p=args.dropout_prob,
                                              discrete_representation=discrete_representation, speaker_model=speaker_model)

    def freeze_attn(self):
        self.decoder.freeze_attn()

    def forward(self, z, motion_input, last_hidden, encoder_output, vid_indices=None):
        input_with_noise_vec = motion_input if z is None else torch.cat([motion_input, z], dim=1)
        return self.decoder(input_with_noise_vec, last_hidden, encoder_output, vid_indices)


class Seq2SeqNet(nn.Module):
    """seq2seq_net.py:217-254.  forward(in_text (B, T) int64, in_lengths, poses (B, n_frames, pose_dim), vid_indices, z=None) -> outputs
    (B, n_frames, pose_dim): frame 0 is poses[:, 0], frames below n_pre_poses are fed from the target, later frames from the model's own
    output (gradient flows through that feedback).  The lengths need not be sorted."""

    def __init__(self, args, pose_dim, n_frames, n_words, word_embed_size, word_embeddings, speaker_model=None):
        super().__init__()
        self.encoder = EncoderRNN(n_words, word_embed_size, args.hidden_size, args.n_layers, dropout=args.dropout_prob,
                                  pre_trained_embedding=word_embeddings)
        self.decoder = Generator(args, pose_dim, speaker_model=speaker_model)
        self.n_frames = n_frames
        self.n_pre_poses = args.n_pre_poses

    def forward(self, in_text, in_lengths, poses, vid_indices, z=None):
        return self._run(in_text, in_lengths, poses, vid_indices, z, None)

    def _run(self, in_text, in_lengths, poses, vid_indices, z, enc_lengths):
        need_cuda(poses, "Seq2SeqNet: poses")
        need_cuda(in_text, "Seq2SeqNet: in_text", None)
        if poses.dim() != 3 or poses.shape[1] < max(self.n_pre_poses, 1) or poses.shape[2] != self.decoder.output_size:
            raise ValueError(f"Seq2SeqNet: poses must be (B, >= {max(self.n_pre_poses, 1)}, {self.decoder.output_size}), got {tuple(poses.shape)}")
        encoder_outputs, encoder_hidden = self.encoder(in_text.transpose(0, 1), in_lengths, None)
        decoder_hidden = encoder_hidden[:self.decoder.n_layers]
        outputs, _, _ = self.decoder.decoder.decode(encoder_outputs.transpose(0, 1), decoder_hidden, poses, self.n_frames, self.n_pre_poses, z,
                                                 vid_indices, enc_lengths)
        return outputs

    def synthesize(self, in_text, in_lengths, pre_poses):
        """The reference's synthesis call pose_decoder(in_text, words_lengths, pre_seq_partial, None) (scripts/synthesize.py:134-136) for a
        padded batch: in_text (B, T) int64 padded with 0, in_lengths one word count per row (any order), pre_poses (B, >= max(n_pre_poses, 1),
        pose_dim).  Eval arithmetic whatever the module's mode (the BatchNorm buffers do not move), no gradient; every row's attention runs over its own
        in_lengths[b] encoder positions, so row b equals the B = 1 run of that utterance."""
        was_training = self.training
        self.train(False)
        try:
            with torch.no_grad():
                return self._run(in_text, in_lengths, pre_poses, None, None, [int(v) for v in in_lengths])
        finally:
            self.train(was_training)


# ----------------------------------------------------------------------------------------------------------------------- training
class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, target, weights):
        scalars = L.empty(4, like=output)
        d = torch.empty_like(output)
        ops.seq2seq_loss(output, target, weights, scalars, d)
        ctx.d = d
        return scalars

    @staticmethod
    def backward(ctx, g):
        # the loss is the fourth scalar; the other three are reported, not differentiated
        return ops.scale_by(ctx.d.clone(), g[3:4].contiguous()), None, None


def custom_loss(output, target, args, epoch=None):
    """train_seq2seq.py:6-33 as a device scalar (differentiable with respect to output)."""
    w = (args.loss_regression_weight, args.loss_kld_weight, args.loss_reg_weight)
    return _LossFn.apply(output.contiguous(), target.contiguous(), w)[3]


class Seq2SeqTrainer:
    """train_iter_seq2seq with the device Adam (optim.ParamAdam): zero_grad, forward, custom_loss, backward, clip_grad_norm_(parameters, 5)
    by a device scale (no host read between the backward and the optimiser), Adam on every parameter that received a gradient."""

    def __init__(self, net, lr=1e-3, betas=(0.5, 0.999), eps=1e-8, max_norm=5.0):
        self.net, self.max_norm = net, max_norm
        self.adam = ParamAdam(net.parameters(), lr, betas, eps)
        self.step_dev = self.adam.step_dev
        dev = self.step_dev.device
        self.total = torch.zeros(1, device=dev, dtype=torch.float64)
        self.ws = torch.empty(256, device=dev, dtype=torch.float64)
        self.scale = torch.zeros(2, device=dev, dtype=torch.float32)

    def set_hparams(self, lr, betas, eps):
        self.adam.set_hparams(lr, betas, eps)

    def clip(self, grads):
        ops.zero_(self.total)
        for g in grads:
            ops.grad_sumsq(g, self.total, self.ws)
        ops.clip_scale(self.total, self.max_norm, self.scale)
        for g in grads:
            ops.scale_by(g, self.scale)

    def step(self, args, epoch, in_text, in_lengths, target_poses):
        self.adam.zero_grad()
        outputs = self.net(in_text, in_lengths, target_poses, None)
        loss = custom_loss(outputs, target_poses, args, epoch)
        loss.backward()
        self.clip(self.adam.live_grads())
        self.adam.step()
        return loss.detach()


def train_iter_seq2seq(args, epoch, in_text, in_lengths, target_poses, net, optim):
    """The reference's signature and return dict (train_seq2seq.py:36-51).  The Seq2SeqTrainer is kept on `optim` (optim.adopt: a plain
    torch.optim.Adam, whose hyper-parameters alone are used)."""
    tr, g = adopt(optim, "_seq2seq_trainer", "train_iter_seq2seq", lambda: Seq2SeqTrainer(net), lambda t: t.net is net)
    tr.set_hparams(g["lr"], g["betas"], g["eps"])
    return {"loss": tr.step(args, epoch, in_text, in_lengths, target_poses).item()}


def build_model(args, lang_model, speaker_model, pose_dim, device):
    """train.py:55-58 for model == 'seq2seq': (generator, None, L1Loss)."""
    generator = Seq2SeqNet(args, pose_dim, args.n_poses, lang_model.n_words, args.wordembed_dim, lang_model.word_embedding_weights,
                           speaker_model=speaker_model).to(device)
    return generator, None, torch.nn.L1Loss()
