"""Device log-mel spectrogram (csrc/logmel.hip, melspec.extract_melspectrogram) against an fp64 numpy restatement of its definition.

librosa is not available here, so there is no reference-generated fixture for utils/data_utils.py:34-38; the oracle below restates
librosa.feature.melspectrogram(n_fft=1024, hop_length=512, power=2, n_mels=128) + power_to_db(ref=np.max) with a DENSE Slaney filterbank
and numpy.fft.rfft, independently of melspec.melspec_tables().

Gate on the fp32 output, computed per input, never fixed: e32 = the largest dB error of the SAME restatement evaluated in fp32 numpy (fp32
window, filterbank, complex64 rfft, fp32 log10) against its fp64 evaluation; the device may reach 8 x e32 (another butterfly order, another mel
summation order, the device log10)."""
import numpy as np
import pytest
import torch

from test_logmel_cpu import dense_slaney_filterbank

pytestmark = pytest.mark.gpu

SR = 16000


def oracle_logmel(y, pad_mode, dt):
    """(db, unclipped db) of one clip, every array and operation in dtype dt (np.float64: the oracle; np.float32: the yardstick of e32)."""
    y = np.asarray(y, dtype=dt)
    fb = dense_slaney_filterbank().astype(dt)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024, dtype=np.float64) / 1024)).astype(dt)
    ypad = np.pad(y, 512, mode=pad_mode)
    F = 1 + len(y) // 512
    frames = ypad[512 * np.arange(F)[:, None] + np.arange(1024)[None, :]] * win[None, :]
    spec = np.fft.rfft(frames, axis=1)
    assert spec.dtype == (np.complex128 if dt == np.float64 else np.complex64)
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(dt)
    mel = fb @ power.T                                                        # (128, F)
    amin = dt(1e-10)
    db = dt(10) * np.log10(np.maximum(mel, amin)) - dt(10) * np.log10(np.maximum(mel.max(), amin))
    assert db.dtype == dt
    return np.maximum(db, db.max() - dt(80)), db


def voiced(n, seed, gaps=False):
    """Harmonic, amplitude-modulated 'voiced' signal (f0 gliding around 120 Hz, 24 harmonics ~ 1 / h, 3 Hz envelope) + 1e-3 noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    phase = 2 * np.pi * (120 * t + 15 / (2 * np.pi * 0.7) * np.sin(2 * np.pi * 0.7 * t))
    y = sum(np.sin(h * phase + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 25))
    y = 0.2 * y * (0.55 + 0.45 * np.sin(2 * np.pi * 3 * t)) + 1e-3 * rng.standard_normal(n)
    if gaps:                                                                   # 1 s of exact zeros in the middle and at the end: the -80 dB floor and amin
        y[n // 2 - SR // 2:n // 2 + SR // 2] = 0
        y[n - SR:] = 0
    return y.astype(np.float32)


def impulse(n):
    y = np.zeros(n, np.float32)
    y[n // 3] = 1.0
    return y


N63 = int(6.3 * SR)                     # 100800: not a multiple of 512
CASES = {
    "voiced": lambda: voiced(N63, 1),
    "voiced_x512": lambda: voiced(197 * 512, 2),
    "voiced_gaps": lambda: voiced(N63, 3, gaps=True),
    "voiced_gaps_x512": lambda: voiced(200 * 512, 4, gaps=True),
    "impulse": lambda: impulse(N63),
    "impulse_x512": lambda: impulse(64 * 512),
}


def check_against_oracle(name, y, pad_mode, dev32):
    o64, raw64 = oracle_logmel(y, pad_mode, np.float64)
    o32, _ = oracle_logmel(y, pad_mode, np.float32)
    e32 = float(np.abs(o32.astype(np.float64) - o64).max())
    gate = 8 * e32
    err = float(np.abs(dev32.astype(np.float64) - o64).max())
    print(f"logmel {name} {pad_mode}: frames {o64.shape[1]} e32 {e32:.3e} dB gate {gate:.3e} dB device error {err:.3e} dB "
          f"floor share {float((o64 == -80).mean()):.3f}")
    assert dev32.shape == o64.shape and dev32.dtype == np.float32
    assert err <= gate, (name, pad_mode, err, gate)
    assert dev32.max() == 0.0 and o64.max() == 0.0
    deep = (o64 == -80.0) & (raw64 < -80.0 - gate)                           # on the oracle's floor by more than the gate: exactly max - 80
    assert (dev32[deep] == np.float32(-80.0)).all(), (name, pad_mode, int((dev32[deep] != -80).sum()))
    return o64, e32, err


def half_order(a):
    """fp16 array -> integers in which neighbouring fp16 values differ by 1 (and +0 == -0)."""
    b = a.view(np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7fff), b & 0x7fff)


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_logmel_matches_fp64_oracle_within_8_e32(pkg, dev, name, pad_mode):
    y = CASES[name]()
    d32 = pkg.extract_melspectrogram(y, pad_mode=pad_mode, dtype=torch.float32, device=dev)
    d16 = pkg.extract_melspectrogram(torch.from_numpy(y), pad_mode=pad_mode, device=dev)            # CPU tensor in, default fp16 out
    again = pkg.extract_melspectrogram(torch.from_numpy(y).to(dev), pad_mode=pad_mode, dtype=torch.float32)   # GPU tensor in
    assert d32.is_cuda and d16.dtype == torch.float16 and tuple(d32.shape) == (128, 1 + len(y) // 512)
    assert torch.equal(d32, again)                                                                  # two runs are bit-identical
    assert torch.equal(d16.view(torch.int16), d32.half().view(torch.int16))                         # the kernel's cast is the RNE cast
    o64, _, _ = check_against_oracle(name, y, pad_mode, d32.cpu().numpy())
    if "gaps" in name:
        assert (o64 == -80).mean() > 0.2
    # fp16 against the oracle's fp16 cast: one fp16 step at most, and rarely
    diff = np.abs(half_order(d16.cpu().numpy()) - half_order(o64.astype(np.float16)))
    share = float((diff != 0).mean())
    print(f"logmel {name} {pad_mode}: fp16 mismatches {share:.3e}, largest {int(diff.max())} step(s)")
    assert diff.max() <= 1
    if name == "voiced":
        assert share <= 1e-3, share


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
def test_all_zero_audio_gives_all_zeros(pkg, dev, pad_mode):
    for n in (N63, 4096):
        for dt in (torch.float32, torch.float16):
            out = pkg.extract_melspectrogram(np.zeros(n, np.float32), pad_mode=pad_mode, dtype=dt, device=dev)
            assert tuple(out.shape) == (128, 1 + n // 512) and (out == 0).all() and not torch.signbit(out).any()


def test_batch_has_a_maximum_per_clip_and_equals_single_calls(pkg, dev):
    """Five clips of very different loudness in one launch: each is referred to ITS OWN maximum, and equals its single call bit for bit."""
    L = 36267
    ys = np.stack([voiced(L, 10 + i) * s for i, s in enumerate((1e-4, 3e-2, 1.0, 30.0, 1e3))]).astype(np.float32)
    for pad_mode in ("reflect", "constant"):
        b32 = pkg.extract_melspectrogram(ys, pad_mode=pad_mode, dtype=torch.float32, device=dev)
        b16 = pkg.extract_melspectrogram(ys, pad_mode=pad_mode, device=dev)
        assert tuple(b32.shape) == (5, 128, 71) and torch.equal(b16.view(torch.int16), b32.half().view(torch.int16))
        assert torch.equal(b32, pkg.extract_melspectrogram(torch.from_numpy(ys).to(dev), pad_mode=pad_mode, dtype=torch.float32))
        for i in range(5):
            one = pkg.extract_melspectrogram(ys[i], pad_mode=pad_mode, dtype=torch.float32, device=dev)
            assert torch.equal(one, b32[i]), (pad_mode, i)
            check_against_oracle(f"batch[{i}]", ys[i], pad_mode, b32[i].cpu().numpy())
    # rows of a wider buffer (strided clips) through the thin wrapper
    wide = torch.zeros(5, L + 13, device=dev)
    wide[:, :L] = torch.from_numpy(ys).to(dev)
    F, _, ws_bytes = pkg.ops.logmel_query(5, L)
    out = torch.empty(5, 128, F, device=dev)
    pkg.ops.logmel(wide[:, :L], out, torch.empty(ws_bytes // 4, device=dev), pad_mode="constant")
    assert torch.equal(out, b32)


def test_short_clips_and_the_reflect_minimum(pkg, dev):
    y = voiced(513, 20)
    d = pkg.extract_melspectrogram(y, dtype=torch.float32, device=dev)
    check_against_oracle("len513", y, "reflect", d.cpu().numpy())
    with pytest.raises(ValueError, match="reflect"):
        pkg.extract_melspectrogram(y[:512], device=dev)
    d = pkg.extract_melspectrogram(y[:100], pad_mode="constant", dtype=torch.float32, device=dev)
    check_against_oracle("len100", y[:100], "constant", d.cpu().numpy())


def test_tables_must_exist_before_stream_capture(pkg, dev, monkeypatch):
    """The constant table is uploaded outside capture and cached per device; a first use inside a capture is an error, not an allocation
    from the graph's pool."""
    ms = pkg.melspec
    t = ms.device_tables(dev)
    assert ms.device_tables(dev) is t and t.dtype == torch.float32 and t.numel() == 5248
    monkeypatch.setattr(ms, "_DEVICE_TABLES", {})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        ms.device_tables(dev)
