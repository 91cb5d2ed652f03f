"""The resampler's definition restated in plain fp64, independent of the package's table code (scalar loops, math.sin, a power series for I0):
rational polyphase resampling of audio at input_sr to 16 kHz by a Kaiser-windowed sinc.  Used by tests/test_resample_cpu.py and
tests/test_resample_gpu.py; brute force on purpose."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 16, 0.85, 8.555504641634386


def geometry(input_sr):
    g = math.gcd(16000, input_sr)
    L, M = 16000 // g, input_sr // g
    c = ROLLOFF * min(1.0, L / M)
    return L, M, 2 * math.ceil(ZEROS / c), c


def _i0(x):
    """Modified Bessel function I0 by its power series sum ((x/2)^2)^m / (m!)^2 (all terms positive; converges fast for x < 10)."""
    q, term, s, m = 0.25 * x * x, 1.0, 1.0, 0
    while term > 1e-18 * s:
        m += 1
        term *= q / (m * m)
        s += term
    return s


def tap_table(input_sr):
    """(L, K) fp64: tap[p][k] = c sinc(c d) kaiser(d), d = p / L + K/2 - 1 - k."""
    L, M, K, c = geometry(input_sr)
    tab = np.zeros((L, K), dtype=np.float64)
    half, i0b = ZEROS / c, _i0(BETA)
    for p in range(L):
        for k in range(K):
            d = (p + (K // 2 - 1 - k) * L) / L
            if abs(d) > half:
                continue
            a = math.pi * c * d
            s = 1.0 if a == 0.0 else math.sin(a) / a
            r = d / half
            tab[p, k] = c * s * _i0(BETA * math.sqrt(max(0.0, 1.0 - r * r))) / i0b
    return tab


def resampled_length(n_in, L, M):
    return sum(1 for n in range(n_in * L // M + 2) if n * M < n_in * L)           # outputs whose position n M / L lies before the end


def resampled_ready(p, L, M, K):
    """Outputs whose last tap (input sample i_n + K/2) is at or before input sample p - 1, by counting."""
    n = 0
    while (n * M) // L + K // 2 <= p - 1:
        n += 1
    return n


def resample(x, taps32, L, M, K):
    """y[n] = sum_k x[i_n - K/2 + 1 + k] taps32[p_n][k] in fp64, and bound[n] = sum_k |x . tap| (what the forward error bound of an fp32
    chain is a multiple of).  x: 1-D array; taps32: the (L, K) table as the device holds it (fp32 values)."""
    t = np.asarray(taps32, dtype=np.float64)
    n_in = len(x)
    n_out = -(-n_in * L // M)
    xp = np.concatenate([np.zeros(K), np.asarray(x, dtype=np.float64), np.zeros(K)])     # sample j of the signal is xp[K + j]: zeros outside
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for n in range(n_out):
        i, p = divmod(n * M, L)
        v = xp[K + i - K // 2 + 1:K + i + K // 2 + 1] * t[p]                             # the K products of output n
        y[n], mag[n] = v.sum(), np.abs(v).sum()
    return y, mag


def response(tab, n_fft=1 << 17):
    """(f, |H|): the prototype's fp64 magnitude response.  The interleaved prototype h[q], q = p + (K - 1 - k) L, is the filter at L times the
    input rate; f is relative to the INPUT Nyquist (1.0 = input_sr / 2), |H| is normalised by L (unit gain at DC for an ideal table)."""
    L, K = tab.shape
    h = np.zeros(L * K)
    for p in range(L):
        for k in range(K):
            h[p + (K - 1 - k) * L] = tab[p, k]
    n_fft = max(n_fft, 1 << int(math.ceil(math.log2(16 * L * K))))
    H = np.abs(np.fft.rfft(h, n_fft)) / L
    f = np.arange(len(H)) / n_fft * 2 * L                             # cycles per sample at rate L -> units of the input Nyquist
    return f, H
