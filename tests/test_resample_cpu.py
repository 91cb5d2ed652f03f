"""Host side of the resampler (resample.py, synthesize.resampled_length / resampled_ready / resample_audio and the input_sr keyword), no GPU:
the integer bookkeeping against brute force, the tap table against the independent fp64 definition of tests/resample_ref.py and its
frequency response, the entries' envelope checks, and every refusal leaving host state as it was."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as R
import utterance_ref as U

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)
# What the fp64 response of the REFERENCE table (resample_ref.tap_table) shows over those rates, rounded toward the lenient side by 1 dB
# (DESIGN.md has the per-rate figures): worst pass-band deviation | |H| - 1 | below 0.5 c: -95.88 dB; worst stop-band level from min(1, L / M)
# on: -86.77 dB.
PASS_DEV_DB, STOP_DB = -94.8, -85.7


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def test_geometry_of_the_listed_rates_and_the_envelope(pkg):
    rs = pkg.resample
    want = {8000: (2, 1, 38), 11025: (640, 441, 38), 22050: (320, 441, 52), 24000: (2, 3, 58), 32000: (1, 2, 76), 44100: (160, 441, 104),
            48000: (1, 3, 114), 96000: (1, 6, 226), 192000: (1, 12, 452), 16000: (1, 1, 38)}
    for sr, lmk in want.items():
        assert rs.geometry(sr)[:3] == lmk == R.geometry(sr)[:3], sr
        assert lmk[0] <= 640 and lmk[2] <= 512 and lmk[2] % 2 == 0
    for bad in (7999, 192001, 0, -48000, 16001, 44101, 48000.0, "48000", None, True):      # 16001 and 44101: gcd 1, 16000 phases
        with pytest.raises(ValueError, match="envelope"):
            rs.geometry(bad)


@pytest.mark.parametrize("sr", [48000, 44100, 8000])                                     # 1/3, 160/441, 2/1
def test_length_and_ready_against_brute_force(syn, sr):
    L, M, K, _ = R.geometry(sr)
    for p in range(3 * K + 1):
        assert syn.resampled_length(p, L, M) == R.resampled_length(p, L, M), p
        assert syn.resampled_ready(p, L, M, K) == R.resampled_ready(p, L, M, K), p
        assert syn.resampled_ready(p, L, M, K) <= syn.resampled_length(p, L, M)
    rng = np.random.default_rng(sr)
    for _ in range(20):                                                                   # per-push increments sum to the total, flush included
        cuts = np.sort(rng.integers(0, 5000, size=rng.integers(1, 9)))
        total, done, made = int(cuts[-1]) + int(rng.integers(1, 700)), 0, 0
        for p in list(cuts) + [total]:
            inc = syn.resampled_ready(int(p), L, M, K) - made
            assert 0 <= inc <= syn.resampled_length(int(p) - done, L, M)                  # what one push can add: the ring's and chunk_buf's bound
            made, done = made + inc, int(p)
        flush = syn.resampled_length(total, L, M) - made
        assert 0 <= flush <= syn.resampled_length(K // 2, L, M) + 1 and made + flush == R.resampled_length(total, L, M)


@pytest.mark.parametrize("sr", RATES)
def test_tap_table_against_the_reference_and_its_frequency_response(pkg, sr):
    L, M, K, c = R.geometry(sr)
    tab = pkg.resample.tap_table(sr)
    ref = R.tap_table(sr)
    assert tab.shape == (L, K) and tab.dtype == np.float64
    assert float(np.abs(tab - ref).max()) <= 1e-14                                        # two evaluations of one fp64 formula, values below 1
    for name, t in (("reference", ref), ("package", tab), ("package, rounded to fp32", tab.astype(np.float32).astype(np.float64))):
        f, H = R.response(t)
        dev = 20 * np.log10(np.abs(H[f < 0.5 * c] - 1).max())
        stop = 20 * np.log10(H[f >= min(1.0, L / M)].max())
        print(f"{sr} Hz {name}: pass-band deviation {dev:.2f} dB, stop band {stop:.2f} dB")
        assert dev <= PASS_DEV_DB and stop <= STOP_DB, (sr, name, dev, stop)


def test_entries_refuse_calls_outside_their_envelope(pkg):
    lib = pkg._lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(B=1, max_out=4, L=1, M=3, K=114)
    for over in (dict(B=0), dict(max_out=0), dict(L=641), dict(L=0), dict(M=0), dict(K=0), dict(K=113), dict(K=514), dict(B=70000)):
        a = dict(ok, **over)
        assert lib.tg_resample(p, p, p, a["B"], a["max_out"], p, a["L"], a["M"], a["K"], p, None) != 0, over
        msg = lib.tg_last_error()
        assert b"tg_resample" in msg and b"envelope" in msg, (over, msg)
    assert lib.tg_resample(None, p, p, 1, 4, p, 1, 3, 114, p, None) != 0 and b"null" in lib.tg_last_error()
    ok = dict(n=(4, 0, 0, 0), flush=0, L=1, M=3, K=114, cs=4, os=3, B=1)
    for over in (dict(B=5), dict(B=0), dict(n=(0, 0, 0, 0)), dict(n=(4, 1, 0, 0)), dict(n=(-1, 0, 0, 0)), dict(flush=2), dict(flush=-1), dict(K=115),
                 dict(L=641), dict(cs=3), dict(os=2), dict(flush=1, os=20)):
        a = dict(ok, **over)
        rc = lib.tg_resample_stream(p, a["cs"], *a["n"], a["flush"], p, a["L"], a["M"], a["K"], p, p, p, p, a["os"], a["B"], None)
        assert rc != 0, over
        msg = lib.tg_last_error()
        assert b"tg_resample_stream" in msg and b"envelope" in msg, (over, msg)
    assert "tg_resample" in pkg._lib.SIGNATURES and "tg_resample_stream" in pkg._lib.SIGNATURES and pkg._lib.ABI_VERSION == 11


def test_refusals_leave_host_state_unchanged(pkg, syn):
    """Rate, audio_sr next to input_sr and (on a stream built without touching a model: the refusals come first) nothing constructed."""
    args, lang = U.make_args(), U.Lang()
    taps_before = dict(pkg.resample._DEVICE_TAPS)
    audio = np.zeros(100, np.float32)
    for call in (lambda: syn.resample_audio(audio, 44101), lambda: syn.resample_audio(audio, 7999), lambda: syn.resample_audio([audio], 48000.5),
                 lambda: syn.generate_gestures_batch(args, None, lang, [audio], [[]], input_sr=300000),
                 lambda: syn.generate_gestures(args, None, lang, audio, [], input_sr=1),
                 lambda: syn.UtteranceBatch(args, lang, [audio], [[]], "cpu", input_sr=44101),
                 lambda: syn.GestureStream(args, None, lang, input_sr=12345),
                 lambda: syn.StreamPool(args, None, lang, input_sr=250000),
                 lambda: syn.Seq2SeqGestureStream(U.make_args("seq2seq"), None, lang, input_sr=16001),
                 lambda: syn.Seq2SeqStreamPool(U.make_args("seq2seq"), None, lang, input_sr=16001)):
        with pytest.raises(ValueError, match="envelope"):
            call()
    for call in (lambda: syn.generate_gestures_batch(args, None, lang, [audio], [[]], audio_sr=48000, input_sr=48000),
                 lambda: syn.generate_gestures(args, None, lang, audio, [], audio_sr=8000, input_sr=44100),
                 lambda: syn.UtteranceBatch(args, lang, [audio], [[]], "cpu", audio_sr=22050, input_sr=22050),
                 lambda: syn.GestureStream(args, None, lang, audio_sr=48000, input_sr=48000),
                 lambda: syn.StreamPool(args, None, lang, audio_sr=48000, input_sr=16000)):
        with pytest.raises(ValueError, match="audio_sr must be 16000"):
            call()
    with pytest.raises(ValueError, match="empty signal"):
        syn.resample_audio([audio, np.zeros(0, np.float32)], 48000)
    assert pkg.resample._DEVICE_TAPS == taps_before and not audio.any()
    # the identity needs no device and launches nothing
    out = syn.resample_audio([audio + 1, audio[:7]], 16000)
    assert [o.shape for o in out] == [(100,), (7,)] and out[0].dtype == np.float32 and float(out[0].min()) == 1.0
    # a host-only stand-in for a stream: the oversize chunk of a resampling stream is refused against max_chunk in INPUT samples
    st = syn.GestureStream.__new__(syn.GestureStream)
    st.closed, st.B, st.max_chunk, st.pushed, st._rs_in, st._rs_out = False, 1, 480, 0, [0], [0]
    with pytest.raises(ValueError, match="max_chunk is 480"):
        st.push(np.zeros(481, np.float32))
    assert (st.pushed, st._rs_in, st._rs_out) == (0, [0], [0])
