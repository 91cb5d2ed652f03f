"""Log-mel spectrogram of raw audio on the device: utils/data_utils.py:34-38 extract_melspectrogram (librosa.feature.melspectrogram(n_fft=1024,
hop_length=512, power=2) with 128 Slaney mels, power_to_db(ref=np.max), the cast to fp16) as csrc/logmel.hip -- the input of the Speech2Gesture
generator (model/speech2gesture.py), for one utterance (synthesis) or a batch of equal-length clips (preprocessing).

The constant tables (window, twiddles, compressed mel filterbank) are formed here in fp64 numpy and rounded to fp32 once.
"""
import functools

import numpy as np
import torch

from . import ops

SR, N_FFT, HOP, N_MELS, F_MAX = 16000, 1024, 512, 128, 8000.0
MAX_TAPS = 24                       # non-zero bins of the widest filter (csrc/logmel.hip LM_TAPS)
PAD_MODES = {"reflect": 0, "constant": 1}


def _hz_to_mel(f):
    """Slaney scale: linear 200 / 3 Hz per mel below 1 kHz, logarithmic with step ln(6.4) / 27 above."""
    f = np.asarray(f, dtype=np.float64)
    lin = f * 3.0 / 200.0
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


@functools.lru_cache(maxsize=None)
def melspec_tables():
    """Host tables, fp64: dict of
      window  (1024,)    periodic Hann
      twiddle (512, 2)   (cos, -sin)(2 pi k / 1024)
      start   (128,)     first non-zero FFT bin of every mel filter (int64)
      count   (128,)     its number of non-zero bins (<= MAX_TAPS, never 0)
      weights (128, 24)  the filter's weights from bin `start` on, zero past `count`
    The filterbank is librosa's: 128 triangles over 130 points equally spaced in Slaney mels between 0 and 8 kHz, each scaled by
    2 / (f[i + 2] - f[i])."""
    n = np.arange(N_FFT, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)
    k = np.arange(N_FFT // 2, dtype=np.float64)
    twiddle = np.stack([np.cos(2.0 * np.pi * k / N_FFT), -np.sin(2.0 * np.pi * k / N_FFT)], axis=1)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(F_MAX), N_MELS + 2))
    bins = np.arange(N_FFT // 2 + 1, dtype=np.float64) * SR / N_FFT
    start, count, weights = np.zeros(N_MELS, np.int64), np.zeros(N_MELS, np.int64), np.zeros((N_MELS, MAX_TAPS), np.float64)
    for i in range(N_MELS):
        lower = (bins - pts[i]) / (pts[i + 1] - pts[i])
        upper = (pts[i + 2] - bins) / (pts[i + 2] - pts[i + 1])
        w = np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (pts[i + 2] - pts[i]))
        nz = np.nonzero(w)[0]
        assert len(nz) and nz[-1] - nz[0] + 1 <= MAX_TAPS, (i, nz)
        start[i], count[i] = nz[0], nz[-1] - nz[0] + 1
        weights[i, :count[i]] = w[nz[0]:nz[-1] + 1]
    tabs = dict(window=window, twiddle=twiddle, start=start, count=count, weights=weights)
    for v in tabs.values():
        v.setflags(write=False)
    return tabs


def _pack_tables():
    """The fp32 image tg_logmel reads (include/trimodal_hip.h): twiddles, window, weights [24][128], first bins."""
    t = melspec_tables()
    return np.concatenate([t["twiddle"].reshape(-1), t["window"], t["weights"].T.reshape(-1), t["start"].astype(np.float64)]).astype(np.float32)


_DEVICE_TABLES = {}


def device_tables(device):
    """The packed table on `device`, uploaded once and never written again.  Like ops.const_rowmax it must exist before a stream capture
    starts: a tensor created while capturing would live in the graph's private pool and be handed out again after the capture."""
    key = str(torch.device(device))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("melspec.device_tables: first use during stream capture; call extract_melspectrogram (or device_tables) once before capturing")
        t = _DEVICE_TABLES[key] = torch.from_numpy(_pack_tables()).to(device)
    return t


def n_frames(n_samples):
    """Frames of a clip of n_samples samples (center = True): 1 + n // 512."""
    return 1 + int(n_samples) // HOP


def extract_melspectrogram(y, sr=SR, pad_mode="reflect", dtype=torch.float16, device=None):
    """y: numpy array, CPU tensor or GPU tensor; (L,) or (N, L) clips of equal length, 16 kHz.  Returns a device tensor (128, F) or (N, 128, F),
    F = 1 + L // 512, of dtype fp16 (the reference's cast) or fp32.  pad_mode: 'reflect' (librosa < 0.10, the releases of the reference's time;
    needs L >= 513) or 'constant' (librosa >= 0.10)."""
    if sr != SR:
        raise ValueError(f"extract_melspectrogram: sr = {sr}; only {SR} Hz audio is supported (resample first)")
    if pad_mode not in PAD_MODES:
        raise ValueError(f"extract_melspectrogram: pad_mode {pad_mode!r}, expected one of {sorted(PAD_MODES)}")
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"extract_melspectrogram: dtype {dtype}, expected torch.float16 or torch.float32")
    if not isinstance(y, torch.Tensor):
        y = torch.from_numpy(np.ascontiguousarray(y))
    if device is None:
        device = y.device if y.is_cuda else torch.device("cuda", torch.cuda.current_device())
    y = y.to(device=device, dtype=torch.float32).contiguous()
    if y.dim() not in (1, 2):
        raise ValueError(f"extract_melspectrogram: audio of shape {tuple(y.shape)}, expected (L,) or (N, L)")
    single = y.dim() == 1
    y2 = y.view(1, -1) if single else y
    N, L = y2.shape
    if N < 1 or L < 1:
        raise ValueError(f"extract_melspectrogram: empty audio {tuple(y.shape)}")
    if pad_mode == "reflect" and L <= HOP:
        raise ValueError(f"extract_melspectrogram: reflect padding needs more than {HOP} samples, got {L} (pad_mode='constant' takes any length)")
    F, _, ws_bytes = ops.logmel_query(N, L)
    out = torch.empty(N, N_MELS, F, device=device, dtype=dtype)
    ws = torch.empty((ws_bytes + 3) // 4, device=device, dtype=torch.float32)
    ops.logmel(y2, out, ws, pad_mode=pad_mode, tables=device_tables(device))
    return out[0] if single else out
