"""The one-launch eval encoder recurrence (csrc/seq2seq_encode.hip, rnn.GRU.row_local_eval / EncoderRNN.row_local_eval) on the GPU.

Accuracy: the kernel and the per-step path (tg_gru_seq_forward) compute the same recurrence in fp32 with different summation orders, so the
gate is relative to the per-step path's own error against the same fp64 reference on the same inputs: err(new) <= 2 err(per-step) + 1.2e-7
(one fp32 epsilon: |h| < 1).  Everything else is bit-level."""
import numpy as np
import pytest
import torch

import gru_seq_ref as G

pytestmark = pytest.mark.gpu
EPS = 1.2e-7
NAN = float("nan")
CASES = {"one_step": (1, 1, [1]), "unsorted": (3, 5, [5, 1, 3]), "five_rows": (5, 34, [2, 34, 7, 1, 34])}


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def make(H, D, B, T, seed):
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(H)
    gi = rng.standard_normal((D, B, T, 3 * H)).astype(np.float32)
    whh = [rng.uniform(-s, s, (3 * H, H)).astype(np.float32) for _ in range(D)]
    bhh = [rng.uniform(-s, s, 3 * H).astype(np.float32) for _ in range(D)]
    h0 = rng.uniform(-0.9, 0.9, (D, B, H)).astype(np.float32)
    return gi, whh, bhh, h0


def reference(gi, whh, bhh, h0, lens):
    """fp64 cell loop of gru_seq_ref on the kernels' own gi: (y (B, T, D H), h_n (D, B, H))."""
    D, B, T, H3 = gi.shape
    eye, zero = np.eye(H3), np.zeros(H3)
    ys, hs = [], []
    for d in range(D):
        y, h = G.numpy_layer(gi[d].astype(np.float64), eye, whh[d].astype(np.float64), zero, bhh[d].astype(np.float64), lens,
                             None if h0 is None else h0[d].astype(np.float64), reverse=(d == 1))
        ys.append(y); hs.append(h)
    return np.concatenate(ys, axis=2), np.stack(hs)


def run(ops, dev, gi, whh, bhh, h0, lens, new, T=None, fill=None, flag=None):
    D, B, T_, H3 = gi.shape
    H = H3 // 3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    y = torch.full((B, T_, D * H), NAN if fill is None else fill, device=dev)
    hn = torch.full((D, B, H), NAN, device=dev)
    fn = ops.seq2seq_encode_eval if new else (lambda *a, **k: ops.gru_seq_forward(*a[:5], None, **k))
    fn(t(gi), [t(w) for w in whh], [t(b) for b in bhh], y, hn, lengths=lens, h0=None if h0 is None else t(h0), **({} if flag is None else {"flag": flag}))
    torch.cuda.synchronize()
    return y, hn


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("H", [8, 12, 200])
def test_accuracy_against_fp64_relative_to_the_per_step_path(pkg, dev, H, D, case):
    B, T, lens = CASES[case]
    gi, whh, bhh, h0 = make(H, D, B, T, 1000 * H + 10 * D + B)
    for h in (None, h0):
        ry, rh = reference(gi, whh, bhh, h, lens)
        err = {}
        for new in (False, True):
            y, hn = run(pkg.ops, dev, gi, whh, bhh, h, lens, new)
            assert not torch.isnan(y).any() and not torch.isnan(hn).any()
            err[new] = max(float(np.abs(y.cpu().numpy() - ry).max()), float(np.abs(hn.cpu().numpy() - rh).max()))
        print(f"H={H} D={D} {case} h0={'yes' if h is not None else 'no'}: per-step {err[False]:.3e}  one-launch {err[True]:.3e}")
        assert err[True] <= 2 * err[False] + EPS, (err, h is not None)


@pytest.mark.parametrize("H", [12, 200])
def test_bit_level_invariants(pkg, dev, H):
    """Zeros behind every length although the buffer held NaN; h_n is the y slice; a row of the batch is its own B = 1 run at T = len; two
    runs agree."""
    D = 2
    B, T, lens = CASES["five_rows"]
    gi, whh, bhh, h0 = make(H, D, B, T, 77 + H)
    y, hn = run(pkg.ops, dev, gi, whh, bhh, h0, lens, True)
    y2, hn2 = run(pkg.ops, dev, gi, whh, bhh, h0, torch.tensor(lens, dtype=torch.int64, device=dev), True)     # device lengths: the same launch
    assert np.array_equal(bits(y), bits(y2)) and np.array_equal(bits(hn), bits(hn2))
    for b, n in enumerate(lens):
        assert not bits(y[b, n:]).any(), b                                            # +0.0, bit for bit
        assert np.array_equal(bits(hn[0, b]), bits(y[b, n - 1, :H])) and np.array_equal(bits(hn[1, b]), bits(y[b, 0, H:])), b
        yb, hb = run(pkg.ops, dev, gi[:, b:b + 1, :n], whh, bhh, h0[:, b:b + 1], [n], True)
        assert np.array_equal(bits(yb[0]), bits(y[b, :n])) and np.array_equal(bits(hb[:, 0]), bits(hn[:, b])), b
    # without h0 too, at D = 1 (the forward direction alone equals the forward half of D = 2)
    y1, hn1 = run(pkg.ops, dev, gi[:1], whh[:1], bhh[:1], h0[:1], lens, True)
    assert np.array_equal(bits(y1), bits(y[..., :H])) and np.array_equal(bits(hn1[0]), bits(hn[0]))


def test_a_length_outside_1_T_skips_its_row_and_sets_the_flag(pkg, dev):
    """A refused input, reported through the flag word: the row's y is zero and its h_n is h0, the other rows are what they are without it."""
    H, D = 12, 2
    B, T, lens = CASES["unsorted"]
    gi, whh, bhh, h0 = make(H, D, B, T, 5)
    good_y, good_hn = run(pkg.ops, dev, gi, whh, bhh, h0, lens, True)
    for bad in (0, T + 1, -3):
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        dl = torch.tensor([lens[0], bad, lens[2]], dtype=torch.int64, device=dev)
        y, hn = run(pkg.ops, dev, gi, whh, bhh, h0, dl, True, flag=flag)
        assert int(flag.item()) == 1
        assert not bits(y[1]).any() and np.array_equal(bits(hn[:, 1]), bits(torch.from_numpy(h0[:, 1])))
        for b in (0, 2):
            assert np.array_equal(bits(y[b]), bits(good_y[b])) and np.array_equal(bits(hn[:, b]), bits(good_hn[:, b]))
        with pytest.raises(RuntimeError, match="outside"):
            pkg.ops.gru_seq_check(flag)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    run(pkg.ops, dev, gi, whh, bhh, h0, torch.tensor(lens, dtype=torch.int64, device=dev), True, flag=flag)
    assert int(flag.item()) == 0
    with pytest.raises(ValueError, match="lengths must lie"):
        run(pkg.ops, dev, gi, whh, bhh, h0, [5, 0, 3], True)                           # a host list is validated before the launch
    with pytest.raises(ValueError, match="envelope"):
        pkg.ops.seq2seq_encode_eval(torch.zeros(2, 1, 129, 24, device=dev), [None] * 2, [None] * 2, None, None)


@pytest.mark.parametrize("H,n_layers", [(12, 1), (200, 2)])
def test_encoder_rnn_row_local_eval(pkg, dev, H, n_layers):
    V, E, B, T = 50, 16, 4, 9
    lens = [3, 9, 1, 6]
    torch.manual_seed(3 + H)
    enc = pkg.EncoderRNN(V, E, H, n_layers, dropout=0.0).to(dev).eval()
    assert enc.row_local_eval is False and enc.gru.row_local_eval is False
    seqs = torch.randint(1, V, (T + 2, B), device=dev)
    ref = G.RefEncoder({k: v.detach().cpu() for k, v in enc.state_dict().items()}, n_layers)
    with torch.no_grad():
        ro, rh = ref(seqs.cpu(), lens)
        off_o, off_h = enc(seqs, lens)
        enc.row_local_eval = True
        assert enc.gru.row_local_eval is True
        on_o, on_h = enc(seqs, lens)
        dev_o, dev_h = enc(seqs, torch.tensor(lens, dtype=torch.int64, device=dev))         # used as it is: all T + 2 steps, zeros behind
    e_off = max(float((off_o.cpu().double() - ro).abs().max()), float((off_h.cpu().double() - rh).abs().max()))
    e_on = max(float((on_o.cpu().double() - ro).abs().max()), float((on_h.cpu().double() - rh).abs().max()))
    print(f"EncoderRNN H={H} layers={n_layers}: per-step {e_off:.3e}  row-local {e_on:.3e}")
    assert tuple(on_o.shape) == (max(lens), B, H) and e_on <= 2 * e_off + EPS, (e_on, e_off)
    assert tuple(dev_o.shape) == (T + 2, B, H) and np.array_equal(bits(dev_o[:max(lens)]), bits(on_o)) and not bits(dev_o[max(lens):]).any()
    assert np.array_equal(bits(dev_h), bits(on_h))
    for b, n in enumerate(lens):
        assert not bits(on_o[n:, b]).any()
    # a taped forward (eval mode, gradients enabled) and a training-mode forward ignore the flag
    taped_on = enc(seqs, lens)
    assert taped_on[0].requires_grad
    enc.row_local_eval = False
    taped_off = enc(seqs, lens)
    assert np.array_equal(bits(taped_on[0]), bits(taped_off[0])) and np.array_equal(bits(taped_on[1]), bits(taped_off[1]))
    enc.train()
    with torch.no_grad():
        tr_off = enc(seqs, lens)
        enc.row_local_eval = True
        tr_on = enc(seqs, lens)
    assert np.array_equal(bits(tr_on[0]), bits(tr_off[0])) and np.array_equal(bits(tr_on[1]), bits(tr_off[1]))
