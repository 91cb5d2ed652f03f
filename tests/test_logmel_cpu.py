"""Host side of the log-mel spectrogram and of Speech2Gesture synthesis (no GPU): the constant tables against their definitions, the window
arithmetic of scripts/synthesize.py:57-65,90, and the argument checks that come before any launch.

librosa is not available to these tests, so there is no reference-generated fixture: the definition (librosa.filters.mel with Slaney scale and
normalisation, periodic Hann, exp(-2 pi i k / 1024)) is restated below in fp64 numpy, independently of melspec.melspec_tables()."""
import argparse
import ctypes as C
import math

import numpy as np
import pytest
import torch


def dense_slaney_filterbank(sr=16000, n_fft=1024, n_mels=128, fmin=0.0, fmax=8000.0):
    """(n_mels, n_fft / 2 + 1) fp64, vectorised the way librosa.filters.mel lays it out (ramps / fdiff)."""
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def to_mel(hz):
        return min_log_mel + math.log(hz / min_log_hz) / logstep if hz >= min_log_hz else hz / f_sp
    mels = np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2)
    mel_f = np.where(mels >= min_log_mel, min_log_hz * np.exp(logstep * (mels - min_log_mel)), f_sp * mels)
    fftfreqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower, upper = -ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]


def test_compressed_filterbank_expands_to_the_dense_slaney_filterbank(pkg):
    t = pkg.melspec.melspec_tables()
    dense = np.zeros((128, 513))
    for i in range(128):
        dense[i, t["start"][i]:t["start"][i] + t["count"][i]] = t["weights"][i, :t["count"][i]]
    want = dense_slaney_filterbank()
    assert np.abs(dense - want).max() <= 1e-12
    assert (t["count"] >= 1).all() and ((want > 0).sum(axis=1) >= 1).all()                       # no filter is empty
    assert int((want > 0).sum()) == int(t["count"].sum()) == 1009 and int(t["count"].max()) == 24 == t["weights"].shape[1]
    assert (t["weights"][np.arange(24)[None, :] >= t["count"][:, None]] == 0).all()               # zero past the filter's last bin


def test_window_and_twiddles_are_the_fp64_formulas_rounded_once(pkg):
    ms = pkg.melspec
    t = ms.melspec_tables()
    n = np.arange(1024, dtype=np.float64)
    assert t["window"].dtype == np.float64 and np.array_equal(t["window"].astype(np.float32), (0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)).astype(np.float32))
    w = np.exp(-2j * np.pi * np.arange(512) / 1024)
    assert np.array_equal(t["twiddle"].astype(np.float32), np.stack([w.real, w.imag], axis=1).astype(np.float32))
    packed = ms._pack_tables()
    lib = pkg._lib.load()
    sizes = (C.c_int64 * 3)()
    assert lib.tg_logmel_query(256, 36267, C.cast(sizes, C.c_void_p)) == 0
    assert list(sizes) == [71, packed.size, 256 * 71 * 129 * 4] and packed.dtype == np.float32
    assert np.array_equal(packed[:1024].reshape(512, 2), t["twiddle"].astype(np.float32)) and np.array_equal(packed[1024:2048], t["window"].astype(np.float32))
    assert np.array_equal(packed[2048:5120].reshape(24, 128).T, t["weights"].astype(np.float32)) and np.array_equal(packed[5120:], t["start"].astype(np.float32))


def test_spectrogram_window_arithmetic_for_a_ten_second_clip(pkg):
    """synthesize.py:57-65,90 by hand for 10 s: stride 2 s, unit 34 / 15 s -> ceil((10 - 2.2667) / 2) + 1 = 5 windows; start of window i =
    floor(2 i / 10 * 128) -- the MEL count, as the reference has it -- = 0, 25, 51, 76, 102; slice length round(2.2667 * 31.25) = 71."""
    syn = pkg.synthesize
    assert syn.num_windows(10.0) == 5
    assert [syn.spec_window_start(i, 10.0) for i in range(5)] == [0, 25, 51, 76, 102]
    assert syn.spec_slice_length(34, 15) == 71 and pkg.melspec.n_frames(160000) == 313
    a = argparse.Namespace(n_poses=34, n_pre_poses=4, motion_resampling_framerate=15)
    assert syn.end_padding_samples(a, 160000) == 36266 - (160000 - 128000)                       # :96-102 for the last window


def test_short_utterance_is_refused_not_padded(pkg):
    """5 s: the third window starts at frame floor(4 / 5 * 128) = 102 of 157, 55 frames are left, the generator needs 70."""
    syn = pkg.synthesize
    a = argparse.Namespace(n_poses=34, n_pre_poses=4, motion_resampling_framerate=15, model="speech2gesture")
    with pytest.raises(ValueError, match=r"80000 samples.*100352 samples"):
        syn.generate_gestures(a, torch.nn.Linear(1, 1), None, np.zeros(80000, np.float32), None)
    with pytest.raises(ValueError, match="16000"):
        syn.generate_gestures(a, torch.nn.Linear(1, 1), None, np.zeros(200000, np.float32), None, audio_sr=22050)


def test_logmel_arguments_are_checked_before_any_launch(pkg):
    lib = pkg._lib.load()
    buf = (C.c_float * 8192)()
    p = C.cast(buf, C.c_void_p)
    good = dict(audio=p, stride=1024, N=1, L=1024, pad=0, tab=p, tabn=5248, ws=p, wsb=1 << 20, out=p, half=0)

    def run(**kw):
        a = dict(good, **kw)
        return lib.tg_logmel(a["audio"], a["stride"], a["N"], a["L"], a["pad"], a["tab"], a["tabn"], a["ws"], a["wsb"], a["out"], a["half"], None)
    assert run(L=512) != 0 and b"reflect padding needs at least 513 samples" in lib.tg_last_error()
    assert run(pad=2) != 0 and b"pad_mode" in lib.tg_last_error()
    assert run(L=0) != 0 and run(N=0) != 0 and run(N=-3) != 0 and run(audio=None) != 0 and run(out=None) != 0 and run(half=2) != 0
    assert run(tabn=5247) != 0 and run(wsb=3 * 129 * 4 - 1) != 0 and b"workspace" in lib.tg_last_error()
    assert run(N=2, stride=1000) != 0
    with pytest.raises(ValueError, match="16000"):
        pkg.extract_melspectrogram(np.zeros(2048, np.float32), sr=8000)
    with pytest.raises(ValueError, match="pad_mode"):
        pkg.extract_melspectrogram(np.zeros(2048, np.float32), pad_mode="edge")
