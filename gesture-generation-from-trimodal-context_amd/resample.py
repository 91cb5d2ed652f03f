"""The resampler's definition: audio at an integer input_sr -> 16 kHz, the rate every synthesis path is defined for (the counterpart of
scripts/synthesize.py's `librosa.load(..., sr=16000, res_type='kaiser_fast')`, which hides the conversion in the reference).

Rational polyphase resampling: g = gcd(16000, input_sr), L = 16000 / g, M = input_sr / g.  Output sample n sits at input position n M / L,
integer part i_n = (n M) // L, phase p_n = (n M) % L, and

    y[n] = sum_{k = 0 .. K-1} x[i_n - K/2 + 1 + k] * tap[p_n][k]            (samples outside [0, n_in): exact zeros; ceil(n_in L / M) outputs)

The prototype is a Kaiser-windowed sinc with cut-off c = rolloff * min(1, L / M) relative to the input Nyquist and `zeros` zero crossings per
side, K = 2 ceil(zeros / c) taps per phase: tap[p][k] = c sinc(c d) w(d), d = p / L + K/2 - 1 - k the distance in input samples from sample
k of the span to the output's position, w(d) = I0(beta sqrt(1 - (d c / zeros)^2)) / I0(beta) inside |d| <= zeros / c and 0 outside.  The
defaults (zeros = 16, rolloff = 0.85, beta = 8.555504641634386) are the parameters resampy documents for 'kaiser_fast', written down from
memory: NO bit or dB parity with librosa / resampy is claimed (resampy interpolates a sampled prototype; this table is evaluated exactly
per phase).  The table is fp64 numpy (np.sinc, np.i0), rounded to fp32 once per (input_sr, device) and kept; the device arithmetic is
csrc/resample.hip's.  Integers and fp64 only on the host; the stream bookkeeping (resampled_length, resampled_ready) is in synthesize.py."""
import math

import numpy as np
import torch

TARGET_SR = 16000
ZEROS, ROLLOFF, BETA = 16, 0.85, 8.555504641634386
MIN_SR, MAX_SR, MAX_L, MAX_K = 8000, 192000, 640, 512         # the kernels' envelope (csrc/resample.hip)


def geometry(input_sr, zeros=ZEROS, rolloff=ROLLOFF):
    """(L, M, K, c) of input_sr -> 16 kHz.  ValueError naming the envelope for anything the kernels do not take: a rate that is not an integer
    in [8000, 192000], more than 640 phases (gcd(16000, input_sr) < 25) or more than 512 taps per phase."""
    if isinstance(input_sr, bool) or not isinstance(input_sr, (int, np.integer)):
        raise ValueError(f"resample: input_sr = {input_sr!r} is outside the envelope: an integer rate in [{MIN_SR}, {MAX_SR}] Hz")
    sr = int(input_sr)
    if not MIN_SR <= sr <= MAX_SR:
        raise ValueError(f"resample: input_sr = {sr} is outside the envelope {MIN_SR} <= input_sr <= {MAX_SR}")
    g = math.gcd(TARGET_SR, sr)
    L, M = TARGET_SR // g, sr // g
    c = rolloff * min(1.0, L / M)
    K = 2 * math.ceil(zeros / c)
    if L > MAX_L or K > MAX_K:
        raise ValueError(f"resample: input_sr = {sr} gives L = {L} phases of K = {K} taps, outside the envelope L <= {MAX_L}, K <= {MAX_K}")
    return L, M, K, c


def tap_table(input_sr, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """The (L, K) fp64 tap table of input_sr -> 16 kHz."""
    L, M, K, c = geometry(input_sr, zeros, rolloff)
    p = np.arange(L, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    d = (p + (K // 2 - 1 - k) * L).astype(np.float64) / L             # exact integers over L
    u = d * (c / zeros)                                               # the window's argument: |u| <= 1 inside the window
    w = np.where(np.abs(u) <= 1.0, np.i0(beta * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(beta), 0.0)
    return c * np.sinc(c * d) * w


_DEVICE_TAPS = {}


def device_taps(input_sr, device):
    """(taps, L, M, K): the table rounded to fp32 once, on `device`, uploaded once per (input_sr, device) and never written again.  Like
    ops.const_rowmax and melspec.device_tables it must exist before a stream capture starts: first use during a capture is refused."""
    key = (int(input_sr), str(torch.device(device)))
    hit = _DEVICE_TAPS.get(key)
    if hit is None:
        L, M, K, _ = geometry(input_sr)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("resample.device_taps: first use during stream capture; resample once (or call device_taps) before capturing")
        hit = _DEVICE_TAPS[key] = (torch.from_numpy(tap_table(input_sr).astype(np.float32)).to(device), L, M, K)
    return hit
