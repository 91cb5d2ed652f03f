"""torch.nn.GRU-shaped modules on the general HIP recurrence (csrc/gru_seq.hip): per-row lengths, an initial state, the final state, one
direction or two.

`GRU` has torch.nn.GRU's constructor, parameter names, shapes and initialisation (state dicts load strictly both ways) and takes a padded
tensor or a PackedSequence; `EncoderRNN` is the Seq2Seq text encoder of the reference (model/seq2seq_net.py:14-56) on top of it.  All
arithmetic runs in libtrimodal_hip.so (layers.gru_seq_stack_fwd / gru_seq_stack_bwd); torch is plumbing -- parameter containers, the
packing / unpacking index shuffles and the autograd bridge.  Shapes outside the kernel envelope raise: there is no torch fallback.
"""
import torch
import torch.nn as nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from . import layers as L
from . import ops


class _GRUFn(torch.autograd.Function):
    """The stack's hand-written backward behind torch.autograd (as modules._Bridge, with the parameters as inputs so that their gradients
    reach any optimiser the ordinary way)."""

    @staticmethod
    def forward(ctx, cfg, x, hx, *params):
        names, n_layers, H, D, lengths, p_drop, training, rng, inject, save = cfg
        P = dict(zip(names, params))
        y, h_n, tape, _ = L.gru_seq_stack_fwd(x, P, "", n_layers, H, D, lengths=lengths, h0=hx, p_drop=p_drop, training=training, rng=rng,
                                              save=save, inject=inject)
        ctx.set_materialize_grads(False)
        ctx.tape, ctx.names, ctx.n_layers, ctx.P = tape, names, n_layers, P
        return y, h_n

    @staticmethod
    def backward(ctx, dy, dh_n):
        assert ctx.tape is not None, "GRU: the forward ran without saving its tape"
        G = {n: ops.zeros_like(ctx.P[n]) for n in ctx.names}
        dx, dh0 = L.gru_seq_stack_bwd(None if dy is None else dy.contiguous(), None if dh_n is None else dh_n.contiguous(), ctx.tape, ctx.P, G,
                                      "", ctx.n_layers, need_dx=ctx.needs_input_grad[1], need_dh0=ctx.needs_input_grad[2])
        return (None, dx, dh0) + tuple(G[n] if ctx.needs_input_grad[3 + i] else None for i, n in enumerate(ctx.names))


class GRU(nn.Module):
    """torch.nn.GRU on the HIP recurrence.  forward(input, hx=None) -> (output, h_n) for a padded tensor ((T, B, K), or (B, T, K) with
    batch_first) or a PackedSequence (sorted or not); float32 on the GPU.  Train-mode inter-layer dropout draws from the module's own
    counter RNG (`seed`); parity tests queue injected masks {f"g.gru.drop{l}": (B, T, D*H)} in `_replay_draws`."""

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=False, dropout=0.0, bidirectional=False, seed=0):
        super().__init__()
        if not bias:
            raise NotImplementedError("GRU(bias=False) is not implemented on the HIP path")
        self.input_size, self.hidden_size, self.num_layers = int(input_size), int(hidden_size), int(num_layers)
        self.bias, self.batch_first, self.dropout, self.bidirectional = True, bool(batch_first), float(dropout), bool(bidirectional)
        self.seed = int(seed)
        # torch's own module gives the names, shapes and default initialisation; only its parameters are kept
        proto = nn.GRU(input_size, hidden_size, num_layers, bias=True, batch_first=batch_first, dropout=dropout, bidirectional=bidirectional)
        self._names = []
        for name, p in proto.named_parameters():
            self.register_parameter(name, nn.Parameter(p.detach().clone()))
            self._names.append(name)
        self._rng = None
        self._replay_draws = []
        # opt-in: eval-mode forwards of at most four rows without a tape, lengths or hx run each layer's recurrence as ONE launch of the
        # few-row kernel (csrc/gru_vec.hip) instead of one launch per time step.  Off by default: every existing call keeps its kernel
        self.few_row_eval = False
        # opt-in: eval-mode forwards without a tape run each layer's recurrence as ONE launch of the row-local kernel (csrc/seq2seq_encode.hip:
        # a workgroup per (row, direction), per-row lengths and hx included) where the shape is inside its envelope.  Off by default
        self.row_local_eval = False

    def _row_local_takes(self, B, T, save):
        return self.row_local_eval and not self.training and not save and \
            ops.seq2seq_encode_supported(B, T, self.hidden_size, 2 if self.bidirectional else 1)

    def _row_local_forward(self, x, lengths, hx):
        """The stack in eval mode without a tape: per layer one grouped input projection (the GEMM entry of the per-step path) and one launch
        of the row-local recurrence.  lengths: None, a list / CPU tensor (validated and uploaded once) or a device int64 tensor, used as it
        is -- nothing is read back; the flag word the kernel sets for an entry outside [1, T] is kept in self._row_local_flag
        (ops.gru_seq_check)."""
        D, H = (2 if self.bidirectional else 1), self.hidden_size
        B, T, _ = x.shape
        sfxs = ("", "_reverse")[:D]
        ldev, flag = ops.gru_seq_lengths(lengths, B, T, x.device)
        self._row_local_flag = flag
        h_n = L.empty(self.num_layers * D, B, H, like=x)
        cur = x
        for l in range(self.num_layers):
            gi = L.empty(D, B, T, 3 * H, like=x)
            a_win = ops.Win.plain(cur.view(B * T, cur.shape[2]))
            ops.gemm_nt_group([dict(A=a_win, W=getattr(self, f"weight_ih_l{l}{s}"), bias=getattr(self, f"bias_ih_l{l}{s}"),
                                    out=gi[d].view(B * T, 3 * H)) for d, s in enumerate(sfxs)])
            y = L.empty(B, T, D * H, like=x)
            ops.seq2seq_encode_eval(gi, tuple(getattr(self, f"weight_hh_l{l}{s}").detach() for s in sfxs),
                                    tuple(getattr(self, f"bias_hh_l{l}{s}").detach() for s in sfxs), y, h_n[l * D:(l + 1) * D], lengths=ldev,
                                    h0=None if hx is None else hx[l * D:(l + 1) * D], flag=flag)
            cur = y
        return cur, h_n

    def _few_row_takes(self, B, lengths, hx, save):
        if not self.few_row_eval or self.training or save or lengths is not None or hx is not None or B > 4:
            return False
        H = self.hidden_size
        return ops.gru_vec_takes(B, H, None, None) if self.bidirectional else ops.gru_vec1_supported(B, H)

    def _few_row_forward(self, x, first_layer=0, h_n=None):
        """The stack for B <= 4 rows in eval mode: per layer one grouped input projection (the GEMM entry of the per-step path) and one
        recurrence launch carrying every direction.  h_n is read from y: the last step forward, the first step reverse.
        forward_constant enters at first_layer = 1 with layer 0's output as x and layer 0's rows of h_n filled in."""
        D, H = (2 if self.bidirectional else 1), self.hidden_size
        B, T, _ = x.shape
        sfxs = ("", "_reverse")[:D]
        if h_n is None:
            h_n = L.empty(self.num_layers * D, B, H, like=x)
        cur = x
        for l in range(first_layer, self.num_layers):
            gi = L.empty(D, B, T, 3 * H, like=x)
            a_win = ops.Win.plain(cur.view(B * T, cur.shape[2]))
            ops.gemm_nt_group([dict(A=a_win, W=getattr(self, f"weight_ih_l{l}{s}"), bias=getattr(self, f"bias_ih_l{l}{s}"),
                                    out=gi[d].view(B * T, 3 * H)) for d, s in enumerate(sfxs)])
            y = L.empty(B, T, D * H, like=x)
            whh = tuple(getattr(self, f"weight_hh_l{l}{s}").detach() for s in sfxs)
            bhh = tuple(getattr(self, f"bias_hh_l{l}{s}").detach() for s in sfxs)
            if D == 2:
                ops.gru_forward(gi, whh, bhh, y, None)
            else:
                ops.gru_forward_vec1(gi[0], whh[0], bhh[0], y)
            h_n[l * D].copy_(y[:, T - 1, :H])
            if D == 2:
                h_n[l * D + 1].copy_(y[:, 0, H:])
            cur = y
        return cur, h_n

    def forward_constant(self, x_row, T, hx=None):
        """The stack on an input that is the SAME row at every one of T steps: x_row (B, input_size) -> (y (B, T, D*H), h_n), batch-first
        whatever `batch_first` says.  Layer 0 projects the row ONCE per direction ((B, in) x (in, 3H), the GEMM entry of the other paths)
        and runs one constant-input few-row recurrence launch (ops.gru_forward_vec_const); layers 1 and above are the few_row_eval path.
        Eval mode, no hx, B <= 4 inside the few-row envelope -- anything else raises ValueError: the input is never repeated silently."""
        D, H = (2 if self.bidirectional else 1), self.hidden_size
        if self.training:
            raise ValueError("GRU.forward_constant runs in eval mode only (no dropout, no tape): call .eval() first")
        if hx is not None:
            raise ValueError("GRU.forward_constant takes no initial state")
        if not isinstance(x_row, torch.Tensor) or x_row.dim() != 2 or x_row.shape[1] != self.input_size:
            raise ValueError(f"GRU.forward_constant: x_row must be (B, {self.input_size}), got {tuple(getattr(x_row, 'shape', ()))}")
        B, T = x_row.shape[0], int(T)
        if not 1 <= B <= 4 or T < 1:
            raise ValueError(f"GRU.forward_constant: 1 <= B <= 4 rows and T >= 1 steps, got B = {B}, T = {T}")
        if not (x_row.is_cuda and x_row.dtype == torch.float32):
            raise TypeError(f"GRU.forward_constant: expected a CUDA float32 input, got {x_row.dtype} on {x_row.device}")
        if not ops.gru_vec_const_supported(B, H, D):
            raise ValueError(f"GRU.forward_constant: (B, H, D) = {(B, H, D)} is outside the few-row kernel envelope (1 <= B <= 4, 64 < H <= 320, "
                             "H % 4 == 0); there is no torch fallback")
        sfxs = ("", "_reverse")[:D]
        with torch.no_grad():
            x_row = x_row.contiguous()
            gi = L.empty(D, B, 3 * H, like=x_row)
            ops.gemm_nt_group([dict(A=ops.Win.plain(x_row), W=getattr(self, f"weight_ih_l0{s}"), bias=getattr(self, f"bias_ih_l0{s}"), out=gi[d])
                               for d, s in enumerate(sfxs)])
            y = L.empty(B, T, D * H, like=x_row)
            ops.gru_forward_vec_const(gi, tuple(getattr(self, f"weight_hh_l0{s}").detach() for s in sfxs),
                                      tuple(getattr(self, f"bias_hh_l0{s}").detach() for s in sfxs), y)
            h_n = L.empty(self.num_layers * D, B, H, like=x_row)
            h_n[0].copy_(y[:, T - 1, :H])
            if D == 2:
                h_n[1].copy_(y[:, 0, H:])
            if self.num_layers == 1:
                return y, h_n
            return self._few_row_forward(y, 1, h_n)

    def extra_repr(self):
        return (f"{self.input_size}, {self.hidden_size}, num_layers={self.num_layers}, batch_first={self.batch_first}, dropout={self.dropout}, "
                f"bidirectional={self.bidirectional}")

    def flatten_parameters(self):
        """No-op (the reference calls it under DataParallel)."""

    def run_batch_first(self, x, lengths=None, hx=None):
        """The stack on x (B, T, K) float32 contiguous on the GPU; lengths: None, a list / CPU tensor, or a device int64 tensor; hx
        (num_layers * D, B, H).  Returns (y (B, T, D*H) with zeros at t >= length, h_n)."""
        D, H = (2 if self.bidirectional else 1), self.hidden_size
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == self.input_size):
            raise TypeError(f"GRU: expected a CUDA float32 input with {self.input_size} features in 3 dimensions, got "
                            f"{getattr(x, 'dtype', None)} {getattr(x, 'device', None)} {tuple(getattr(x, 'shape', ()))}")
        B, T = x.shape[0], x.shape[1]
        if B < 1 or T < 1 or not ops.gru_seq_supported(B, T, H, D):
            raise ValueError(f"GRU: (B, T, H, D) = {(B, T, H, D)} is outside the HIP kernel envelope {ops.GRU_SEQ_ENVELOPE}; there is no torch fallback")
        if hx is not None:
            if tuple(hx.shape) != (self.num_layers * D, B, H):
                raise ValueError(f"GRU: hx must have shape {(self.num_layers * D, B, H)}, got {tuple(hx.shape)}")
            hx = hx.float().contiguous()
        params = [getattr(self, n) for n in self._names]
        training = self.training and self.num_layers > 1
        inject = self._replay_draws.pop(0) if (training and self._replay_draws) else None
        rng = None
        if training and self.dropout > 0 and inject is None:
            if self._rng is None:
                from .engine import DeviceRNG
                self._rng = DeviceRNG(self.seed, x.device)
            self._rng.advance()
            rng = self._rng
        save = torch.is_grad_enabled() and (x.requires_grad or (hx is not None and hx.requires_grad) or any(p.requires_grad for p in params))
        if self._few_row_takes(B, lengths, hx, save):
            with torch.no_grad():
                return self._few_row_forward(x.contiguous())
        if self._row_local_takes(B, T, save):
            with torch.no_grad():
                return self._row_local_forward(x.contiguous(), lengths, hx)
        cfg = (tuple(self._names), self.num_layers, H, D, lengths, self.dropout, training, rng, inject, save)
        return _GRUFn.apply(cfg, x.contiguous(), hx, *params)

    def forward(self, input, hx=None):
        if isinstance(input, PackedSequence):
            x, lens = pad_packed_sequence(input, batch_first=True)         # original batch order, as hx and h_n are
            y, h_n = self.run_batch_first(x.contiguous(), lens, hx)
            ys, ls = (y, lens) if input.sorted_indices is None else (y.index_select(0, input.sorted_indices), lens[input.sorted_indices.cpu()])
            data = pack_padded_sequence(ys, ls, batch_first=True, enforce_sorted=True).data
            return PackedSequence(data, input.batch_sizes, input.sorted_indices, input.unsorted_indices), h_n
        if input.dim() != 3:
            raise ValueError("GRU: unbatched (2-D) input is not implemented on the HIP path")
        x = input if self.batch_first else input.transpose(0, 1)
        y, h_n = self.run_batch_first(x.contiguous(), None, hx)
        return (y if self.batch_first else y.transpose(0, 1)), h_n


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, idx):
        out = torch.empty(*idx.shape, table.shape[1], device=table.device, dtype=torch.float32)
        ops.embed_gather(table, idx, out)
        ctx.idx, ctx.shape = idx, tuple(table.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        dtable = ops.zeros(*ctx.shape, device=dout.device)
        ops.embed_scatter_add(dout.contiguous(), ctx.idx, dtable)
        return dtable, None


class _SumHalvesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        o = torch.empty(*y.shape[:-1], y.shape[-1] // 2, device=y.device, dtype=torch.float32)
        return ops.add_halves(y, o)

    @staticmethod
    def backward(ctx, d_o):
        dy = torch.empty(*d_o.shape[:-1], 2 * d_o.shape[-1], device=d_o.device, dtype=torch.float32)
        return ops.dup_halves(d_o.contiguous(), dy)


class EncoderRNN(nn.Module):
    """The Seq2Seq text encoder (model/seq2seq_net.py:14-56): embedding -> packed bidirectional GRU -> the two directions summed.
    forward(input_seqs (T, B) int64, input_lengths, hidden=None) -> (outputs (max length, B, H), hidden (2 * n_layers, B, H)); the lengths
    need not be sorted."""

    def __init__(self, input_size, embed_size, hidden_size, n_layers=1, dropout=0.5, pre_trained_embedding=None):
        super().__init__()
        self.input_size, self.hidden_size, self.embed_size, self.n_layers, self.dropout = input_size, hidden_size, embed_size, n_layers, dropout
        if pre_trained_embedding is not None:
            assert pre_trained_embedding.shape[0] == input_size and pre_trained_embedding.shape[1] == embed_size
            self.embedding = nn.Embedding.from_pretrained(torch.as_tensor(pre_trained_embedding, dtype=torch.float32), freeze=False)
        else:
            self.embedding = nn.Embedding(input_size, embed_size)       # parameter container: its forward is never called
        self.gru = GRU(embed_size, hidden_size, n_layers, dropout=dropout, bidirectional=True)
        self.do_flatten_parameters = False

    @property
    def row_local_eval(self):
        """Opt-in (False by default: every call keeps its kernel): eval-mode forwards without a tape run each GRU layer as one GEMM entry plus
        ONE launch of the row-local recurrence (csrc/seq2seq_encode.hip) instead of one launch per time step, where the shape is inside
        ops.SEQ2SEQ_ENCODE_ENVELOPE.  With it, input_lengths may be a device int64 tensor: it is used as it is, nothing is read back, and
        the outputs keep all T steps of input_seqs (exact zeros behind every row's length)."""
        return self.gru.row_local_eval

    @row_local_eval.setter
    def row_local_eval(self, on):
        self.gru.row_local_eval = bool(on)

    def forward(self, input_seqs, input_lengths, hidden=None):
        if not (input_seqs.is_cuda and input_seqs.dtype == torch.int64 and input_seqs.dim() == 2):
            raise TypeError("EncoderRNN: input_seqs must be a CUDA int64 tensor of shape (T, B)")
        if self.row_local_eval and not self.training and isinstance(input_lengths, torch.Tensor) and input_lengths.is_cuda:
            lens, T = input_lengths, input_seqs.shape[0]                  # no host read: the kernel checks the entries (gru._row_local_flag)
        else:
            lens = [int(v) for v in (input_lengths.tolist() if isinstance(input_lengths, torch.Tensor) else input_lengths)]
            T = max(lens) if lens else 0
        if not 1 <= T <= input_seqs.shape[0]:
            raise ValueError(f"EncoderRNN: lengths up to {T} for {input_seqs.shape[0]} steps")
        idx = input_seqs[:T].t().contiguous()                            # (B, T): the kernels are batch-first
        embedded = _EmbedFn.apply(self.embedding.weight, idx)
        y, hidden = self.gru.run_batch_first(embedded, lens, hidden)
        return _SumHalvesFn.apply(y).transpose(0, 1), hidden
