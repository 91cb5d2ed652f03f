"""The resampling kernels on the GPU (csrc/resample.hip): tg_resample against the fp64 definition of tests/resample_ref.py under the forward
error bound of its summation -- derived, not measured -- and tg_resample_stream against tg_resample, bit for bit."""
import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.uint32)


_taps = {}


def taps_of(pkg, dev, sr):
    """(device table, L, M, K, the table as the device holds it): the package's fp64 table rounded once, within one fp32 ulp of the reference's."""
    if sr not in _taps:
        t, L, M, K = pkg.resample.device_taps(sr, dev)
        host = t.cpu().numpy()
        assert host.shape == (L, K) and np.array_equal(host.view(np.uint32), pkg.resample.tap_table(sr).astype(np.float32).view(np.uint32))
        ref = R.tap_table(sr)
        assert float(np.abs(host - ref).max()) <= 2.0 ** -24 * float(np.abs(ref).max())       # (half an ulp of the largest tap; all are below 1)
        assert pkg.resample.device_taps(sr, dev)[0] is t                                  # cached per (rate, device)
        _taps[sr] = (t, L, M, K, host)
    return _taps[sr]


def offline(pkg, dev, sr, rows):
    t, L, M, K, _ = taps_of(pkg, dev, sr)
    y, out_len = pkg.ops.resample(torch.from_numpy(np.concatenate(rows)).to(dev), [len(r) for r in rows], t, L, M, K)
    torch.cuda.synchronize()
    return [p.cpu().numpy() for p in torch.split(y, out_len)]


@pytest.mark.parametrize("sr", [48000, 44100, 8000, 11025])
def test_offline_against_fp64_under_the_forward_bound(pkg, syn, dev, sr):
    """Input lengths 1, K/2 - 1, K/2, K/2 + 1, M and 4099, three ragged rows per launch, white noise in [-1, 1] and rows of ones (on those the
    zeros outside the signal show: the head and the tail are partial sums of the taps).  Per element |y - ref| <= gamma_K sum_k |x_k tap_k|,
    gamma_K = K u / (1 - K u), u = 2^-24: the forward bound of a chain of K fp32 fused multiply-adds, whatever its order."""
    _, L, M, K, host_taps = taps_of(pkg, dev, sr)
    gamma = K * U24 / (1 - K * U24)
    lens = [1, K // 2 - 1, K // 2, K // 2 + 1, M, 4099]
    launches = [[noise(n, sr + n) for n in lens[:3]], [noise(n, sr + n) for n in lens[3:]],
                [np.ones(4099, np.float32), np.ones(K // 2 + 1, np.float32), noise(M, 5)]]
    worst = 0.0
    for rows in launches:
        got = offline(pkg, dev, sr, rows)
        for x, y in zip(rows, got):
            ref, mag = R.resample(x, host_taps, L, M, K)
            assert y.shape == ref.shape == (syn.resampled_length(len(x), L, M),) and y.dtype == np.float32
            err, bound = np.abs(y.astype(np.float64) - ref), gamma * mag
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (sr, len(x), float(err.max()), float(bound[err.argmax()]))
    print(f"{sr} Hz: worst error / bound {worst:.3f} (K = {K}, gamma_K = {gamma:.3e})")
    ones = offline(pkg, dev, sr, [np.ones(4099, np.float32)])[0]
    mid = ones[len(ones) // 2]
    assert abs(mid - 1.0) < 1e-4 and abs(ones[0] - 1.0) > 1e-3                            # unit gain inside, the edge sees the zeros in front


@pytest.mark.parametrize("sr", [48000, 44100])
def test_stream_is_bit_equal_to_offline(pkg, syn, dev, sr):
    """Three ragged rows and a fourth that stays idle.  Every row is pushed in chunks of 1, K - 2, K - 1, K, 1237 and max_chunk samples and, in
    between, not at all (length 0) -- the rows are at different places of that cycle --, then flushed in a call of its own while the others
    go on.  Every call's output rows start as NaN: a row that is not touched keeps them."""
    ops = pkg.ops
    t, L, M, K, _ = taps_of(pkg, dev, sr)
    B, max_chunk = 4, 2000
    sizes = [1, K - 2, 0, K - 1, K, 1237, max_chunk]
    rows = [noise(n, sr + 7 * n) for n in (2 * sum(sizes) + 33, sum(sizes) + K - 1, 3 * K + 1)]
    want = offline(pkg, dev, sr, rows)
    rs = ops.resample_state(B, t, L, M, K, max_chunk, dev)
    assert rs["out_stride"] == max(syn.resampled_length(max_chunk, L, M), syn.resampled_length(K // 2, L, M)) + 1
    nan = np.float32(np.nan).view(np.uint32)
    rs["carry"][3].fill_(float("nan")); rs["consumed"][3] = 12345; rs["produced"][3] = 678
    pos, made, flushed, pieces, step = [0, 0, 0], [0, 0, 0], [False] * 3, [[], [], []], 0
    out = torch.empty(B, rs["out_stride"], device=dev)
    while not all(flushed):
        n, flush = [0] * B, []
        for b in range(3):
            if pos[b] < len(rows[b]):
                n[b] = min(sizes[(step + 2 * b) % len(sizes)], len(rows[b]) - pos[b])
            elif not flushed[b]:
                flush.append(b)
        step += 1
        if not any(n) and not flush:
            continue                                                                     # (every row at a zero of its cycle: the library would refuse)
        stage = torch.zeros(B, max(max(n), 1))
        for b in range(3):
            stage[b, :n[b]] = torch.from_numpy(rows[b][pos[b]:pos[b] + n[b]])
        out.fill_(float("nan"))
        ops.resample_stream(rs, stage.to(dev) if any(n) else None, n, out, flush)
        host = out.cpu().numpy()
        for b in range(3):
            pos[b] += n[b]
            if b in flush:
                new, flushed[b] = syn.resampled_length(pos[b], L, M), True
            else:
                new = syn.resampled_ready(pos[b], L, M, K) if n[b] else made[b]
            pieces[b].append(host[b, :new - made[b]].copy())
            assert (host[b, new - made[b]:].view(np.uint32) == nan).all(), (step, b)         # nothing behind the row's new samples, nothing on an idle row
            made[b] = new
        assert (host[3].view(np.uint32) == nan).all()
    for b in range(3):
        got = np.concatenate(pieces[b])
        assert got.shape == want[b].shape and np.array_equal(bits(got), bits(want[b])), (sr, b)
    # the host's integers are the device's counters (read here, once, by the test only); the idle row kept every bit
    assert rs["consumed"].tolist() == [len(r) for r in rows] + [12345] and rs["produced"].tolist() == made + [678]
    assert (bits(rs["carry"][3]) == nan).all()
    for b in range(3):                                                                   # the carry is the signal's last K - 1 samples
        assert np.array_equal(bits(rs["carry"][b]), bits(rows[b][-(K - 1):]))


def test_a_chunk_shorter_than_the_carry_keeps_its_tail_and_single_samples_stream(pkg, syn, dev):
    """One row at 44.1 kHz pushed sample by sample for 2 K samples, then in one piece: the carry is rewritten from [carry | chunk] every time."""
    ops, sr = pkg.ops, 44100
    t, L, M, K, _ = taps_of(pkg, dev, sr)
    x = noise(2 * K + 500, 3)
    want = offline(pkg, dev, sr, [x])[0]
    rs = ops.resample_state(1, t, L, M, K, 500, dev)
    out, xd, got, made = torch.empty(1, rs["out_stride"], device=dev), torch.from_numpy(x).to(dev)[None], [], 0
    cuts = list(range(1, 2 * K + 1)) + [len(x)]
    for p, q in zip([0] + cuts, cuts):
        ops.resample_stream(rs, xd[:, p:q], [q - p], out)
        new = syn.resampled_ready(q, L, M, K)
        got.append(out[0, :new - made].clone()); made = new
    ops.resample_stream(rs, None, [0], out, flush=[0])
    got.append(out[0, :syn.resampled_length(len(x), L, M) - made].clone())
    assert np.array_equal(bits(torch.cat(got)), bits(want))
    assert rs["consumed"].tolist() == [len(x)] and rs["produced"].tolist() == [len(want)]


def test_refused_calls_launch_nothing(pkg, dev):
    ops = pkg.ops
    t, L, M, K, _ = taps_of(pkg, dev, 48000)
    rs = ops.resample_state(2, t, L, M, K, 100, dev)
    rs["carry"].fill_(3.0); rs["consumed"].fill_(500); rs["produced"].fill_(100)
    out = torch.full((2, rs["out_stride"]), 7.0, device=dev)
    chunk = torch.ones(2, 100, device=dev)
    with pytest.raises(ValueError, match="at most 100"):
        ops.resample_stream(rs, torch.ones(2, 101, device=dev), [101, 0], out)
    with pytest.raises(ValueError, match="flush"):
        ops.resample_stream(rs, chunk, [1, 1], out, flush=[2])
    with pytest.raises(ValueError, match="out"):
        ops.resample_stream(rs, chunk, [1, 1], out[:, :-1])
    with pytest.raises(RuntimeError, match="envelope"):
        ops.resample_stream(rs, None, [0, 0], out)                                        # no samples and no flush
    big = dict(rs, B=5, carry=torch.zeros(5, K - 1, device=dev), consumed=torch.zeros(5, dtype=torch.int64, device=dev),
               produced=torch.zeros(5, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="envelope"):
        ops.resample_stream(big, torch.ones(5, 4, device=dev), [4] * 5, torch.zeros(5, rs["out_stride"], device=dev))
    with pytest.raises(ValueError):
        ops.resample(torch.ones(10, device=dev), [4, 5], t, L, M, K)                      # the lengths do not add up to the buffer
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((rs["carry"] == 3.0).all())
    assert rs["consumed"].tolist() == [500, 500] and rs["produced"].tolist() == [100, 100]
