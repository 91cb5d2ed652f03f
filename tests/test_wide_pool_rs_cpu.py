"""Host side of the wide stream pool at any sample rate (synthesize.WideResampledStreamPool, csrc/stream_pool_wide_rs.hip), no GPU: the
refusals the pool raises before it touches a device, the host's integer mirror of the device's resampler counters against brute force, the
numpy model of the entry against the resampler's definition, and the entry's envelope checks (argument validation precedes any launch)."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as RR
import stream_ref as R
import utterance_ref as U
import wide_pool_ref as WR
import wide_pool_rs_ref as M

S, A = R.S, R.A


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


@pytest.fixture
def host_pool(pkg, syn, monkeypatch):
    """A pool on the CPU: the tensor checks of the ops layer ask for device tensors, so they are lifted (as tests/test_abi_cpu.py lifts them)
    and the fused push is replaced by a recorder -- everything in front of the launch is the pool's own.  (resample.device_taps asks the
    runtime whether a capture is under way, which needs a device to answer: here none is.)"""
    import torch
    launches = []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(pkg.ops, "_f32", lambda t, name="tensor": t)
    monkeypatch.setattr(pkg.ops, "wide_pool_push_resampled",
                        lambda st, rs, packed, lay, words_live=0, flush_row=None: launches.append((dict(lay), words_live, flush_row)))

    def make(input_sr=44100, **kw):
        kw.setdefault("slots", 5)
        pool = syn.WideResampledStreamPool(U.make_args(), WR.HostGenerator(), U.Lang(), input_sr, **kw)
        pool.launches = launches
        return pool
    return make


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_construction_refusals(syn):
    for slots in (0, 129):
        with pytest.raises(ValueError, match=f"WideResampledStreamPool: 1 to 128 slots, got {slots}"):
            syn.WideResampledStreamPool(U.make_args(), None, U.Lang(), 44100, slots=slots)
    for model, why in (("joint_embedding", "window decoder holds four rows: use StreamPool"), ("seq2seq", "window decoder holds four rows: use Seq2SeqStreamPool"),
                       ("speech2gesture", "padded over the whole utterance")):
        with pytest.raises(ValueError, match="WideResampledStreamPool: .*" + why):
            syn.WideResampledStreamPool(U.make_args(model), None, U.Lang(), 44100)
    for rate in (7999, 192001, 44100.0, True, 16001):                            # (16001 Hz: 16000 phases)
        with pytest.raises(ValueError, match="outside the envelope"):
            syn.WideResampledStreamPool(U.make_args(), None, U.Lang(), rate)
    with pytest.raises(ValueError, match="audio_sr must be 16000"):
        syn.WideResampledStreamPool(U.make_args(), None, U.Lang(), 48000, audio_sr=48000)
    with pytest.raises(TypeError):
        syn.WideResampledStreamPool(U.make_args(), None, U.Lang())                # input_sr is required
    with pytest.raises(ValueError, match="WideResampledStreamPool.preview: a wide pool has no preview"):
        syn.WideResampledStreamPool.preview(object.__new__(syn.WideResampledStreamPool), 0)


def test_the_wide_pool_itself_still_refuses_another_rate(syn):
    with pytest.raises(ValueError, match="input_sr = 44100: the stream resampler takes its chunk lengths by value for four rows"):
        syn.WideStreamPool(U.make_args(), None, U.Lang(), input_sr=44100)
    with pytest.raises(ValueError, match="WideStreamPool.preview: a wide pool has no preview"):
        syn.WideStreamPool.preview(object.__new__(syn.WideStreamPool), 0)


def test_the_ring_is_sized_from_the_16k_count_and_no_dense_buffer_is_kept(syn, host_pool):
    pool = host_pool(44100, slots=6, max_chunk=441)
    L, M_, K, _ = RR.geometry(44100)
    assert pool.input_sr == 44100 and pool.state["R"] == A + 160 + 1 and pool.chunk_buf.numel() == 0
    assert pool.rs["stage"] is None and pool.rs["out_stride"] == 161 and tuple(pool.rs["carry"].shape) == (6, K - 1)
    assert pool.state["R"] >= M.min_ring(A, 441, L, M_, K, flush=False) and pool.state["R"] >= M.min_ring(A, 0, L, M_, K, flush=True)
    with pytest.raises(ValueError, match="a ring of"):
        host_pool(44100, max_chunk=441, ring=A + 160)
    same = host_pool(16000, slots=6, max_chunk=441)                              # the identity: WideStreamPool's own state
    assert same.input_sr is None and same.rs is None and same.state["R"] == A + 441


def test_a_refused_push_leaves_the_pool_as_it_was(syn, host_pool):
    pool = host_pool(44100, slots=6, max_chunk=100, word_ring=12)
    assert [pool.open() for _ in range(6)] == list(range(6))
    pool.push({0: np.ones(60, np.float32), 3: np.ones(100, np.float32)})         # (a tick that is taken: the state below is not the initial one)
    assert pool._rs_in == [60, 0, 0, 100, 0, 0] and len(pool.launches) == 1
    pool.open_slots[4] = False                                                   # (a closed slot, as close() leaves it)
    ok = np.zeros(10, np.float32)
    flood = [[f"w{i}", 0.3 + 0.01 * i, 0.305 + 0.01 * i] for i in range(13)]
    state = lambda: (list(pool.pushed), list(pool.next_window), list(pool._n_rec), list(pool.late_words), [list(l) for l in pool._live],
                     list(pool._rs_in), list(pool._rs_out), dict(pool._turn), [list(v) for v in pool._copied.values()],
                     [bytes(h.numpy()[:1024]) for h in pool._push_host], [bytes(d.numpy()[:1024]) for d in pool._push_dev], len(pool.launches))
    before = state()
    for chunks, why in (({4: ok}, "slot 4 is not open"), ({0: ok, 4: ok}, "slot 4 is not open"), ({0: ok, 6: ok}, "slot 6 is not open"), ({}, "non-empty"),
                        ({0: ok, 5: np.zeros(101, np.float32)}, "max_chunk = 100"), ({0: ok, 5: (ok, flood)}, "slot 5: .* word ring's capacity 12"),
                        ({0: np.zeros(10, np.float64)}, "must be float32")):
        with pytest.raises(ValueError, match=why):
            pool.push(chunks)
    with pytest.raises(ValueError, match="slot 4 is not open"):
        pool.close(4)
    with pytest.raises(ValueError, match="nothing was pushed"):
        pool.close(1)
    assert state() == before


# ------------------------------------------------------------------------------------------------------------------ the host's integers
@pytest.mark.parametrize("sr", [48000, 44100, 8000, 11025])
def test_the_host_mirror_against_brute_force(syn, host_pool, sr):
    """Random ragged ticks, short enough that no window completes (nothing but integers moves): per row `pushed` is resample_ref's count, by
    counting, of the final outputs of the cumulated input -- and, after the row's flush, of all of them.  Every tick is one launch."""
    L, M_, K, _ = RR.geometry(sr)
    rng = np.random.default_rng(sr)
    B, max_chunk = 7, 3 * K
    pool = host_pool(sr, slots=B, max_chunk=max_chunk)
    for _ in range(B):
        pool.open()
    total, flushed = [0] * B, [False] * B
    for t in range(24):
        n = [0 if flushed[b] else int(rng.choice([0, 0, 1, K // 2, K - 2, max_chunk, rng.integers(1, max_chunk + 1)])) for b in range(B)]
        if not any(n):
            continue
        got = pool.push({b: np.zeros(n[b], np.float32) for b in range(B) if n[b]})
        assert sorted(got) == [b for b in range(B) if n[b]] and all(v.shape[0] == 0 for v in got.values())
        lay, _, flush_row = pool.launches[-1]
        assert flush_row is None and lay["n_samples"] == sum(n) and lay["n_max"] == max(n)
        total = [a + b for a, b in zip(total, n)]
        if t % 5 == 4:                                                           # a row's input ends: the flush-only tick of close()
            b = int(rng.choice([r for r in range(B) if not flushed[r]]))
            add = pool._flush(b)
            pool.pushed[b] += add[b]
            flushed[b] = True
            lay, live, flush_row = pool.launches[-1]
            assert (flush_row, lay["n_samples"], lay["n_records"], live) == (b, 0, 0, 0) and [v for r, v in enumerate(add) if r != b] == [0] * (B - 1)
        want = [RR.resampled_length(total[b], L, M_) if flushed[b] else RR.resampled_ready(total[b], L, M_, K) for b in range(B)]
        assert pool.pushed == want == pool._rs_out and pool._rs_in == total, (t, pool.pushed, want)
    assert sum(flushed) >= 3 and max(pool.pushed) < A
    assert pool.next_window == [0] * B


def test_the_model_cuts_the_definition_at_the_host_counts():
    """tests/wide_pool_rs_ref.py on its own: ticks of a two-row state give, concatenated through a wrapping ring, resample_ref.resample of the
    whole signal; a records-only tick touches no resampler row; an idle row keeps its sentinels."""
    sr = 8000
    L, M_, K, _ = RR.geometry(sr)
    taps = RR.tap_table(sr).astype(np.float32)
    x = U.make_audio(150, 1)
    Rr = M.min_ring(10, 60, L, M_, K)
    st = M.new_state(3, Rr, 4, K, sentinel=True)
    for k in ("ring", "words", "carry"):
        st[k][0] = 0
    st["consumed"][2], st["produced"][2], st["written"][0] = 12345, 678, Rr - 7
    out, cuts = [], [0, 1, 20, 20, 80, 140, 150]
    for t, (p, q) in enumerate(zip(cuts, cuts[1:])):
        recs = [[(t, 1, 2)] if q == p else [], [], []]
        got, first = M.tick(st, [x[p:q], [], []], recs, 0 if q == 150 else None, L, M_, K, M.fp64_resampled(taps, L, M_, K))
        out += [st["ring"][0, (first[0] + r) % Rr] for r in range(got[0])]
    want = RR.resample(x, taps, L, M_, K)[0].astype(np.float32)
    assert np.array_equal(np.asarray(out, np.float32).view(np.uint32), want.view(np.uint32)) and len(want) == 300
    assert st["consumed"].tolist() == [150, 0, 12345] and st["produced"].tolist() == [300, 0, 678] and st["written"][0] == Rr - 7 + 300
    assert st["n_words"].tolist() == [1, 0, 0] and st["words"][0, 0].tolist() == [2, 1, 2]
    assert np.array_equal(st["carry"][0], x[-(K - 1):]) and np.isnan(st["ring"][1:]).all() and np.isnan(st["carry"][1:]).all()


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_the_entry_is_declared_and_refuses_calls_outside_its_envelope(pkg):
    lib = pkg._lib.load()
    assert "tg_wide_pool_push_resampled" in pkg._lib.SIGNATURES and pkg._lib.ABI_VERSION == 11
    assert len(pkg._lib.SIGNATURES["tg_wide_pool_push_resampled"]) == 25
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    L, M_, K = 160, 441, 104                                                    # 44.1 kHz
    need = lambda n, flush: -(-(n + (K // 2 if flush else 0)) * L // M_) + 1
    ok = dict(hdr=p, samples=p, s_len=4, recs=p, r_len=0, n_max=4, m_max=0, live=0, flush=-1, taps=p, L=L, M=M_, K=K, carry=p, consumed=p, produced=p,
              ring=p, B=1, R=A + need(4, False), W=16)

    def push(**over):
        a = dict(ok, **over)
        return lib.tg_wide_pool_push_resampled(a["hdr"], a["samples"], a["s_len"], a["recs"], a["r_len"], a["n_max"], a["m_max"], a["live"], a["flush"],
                                               a["taps"], a["L"], a["M"], a["K"], a["carry"], a["consumed"], a["produced"], a["ring"], p, p, p, a["B"],
                                               a["R"], A, a["W"], None)

    for over in (dict(B=0), dict(B=129, s_len=129 * 4), dict(flush=-2), dict(flush=1), dict(B=5, s_len=20, flush=5),
                 dict(L=641), dict(L=0), dict(M=0), dict(K=103), dict(K=514), dict(K=0),
                 dict(n_max=0, s_len=0),                                         # no samples, no records, no flush
                 dict(n_max=-1), dict(m_max=-1),
                 dict(R=A + need(4, False) - 1),                                 # the chunk's outputs would reach into the window
                 dict(flush=0),                                                  # a flush on a ring sized for the push alone: K/2 more input samples
                 dict(flush=0, R=A + need(4, True) - 1), dict(n_max=0, s_len=0, flush=0, R=A + need(0, True) - 1),
                 dict(B=128, n_max=9, s_len=1152), dict(R=(1 << 30) + 1),   # (9 samples: one more output than the ring was sized for)
                 dict(s_len=3), dict(B=2, s_len=9), dict(m_max=2, r_len=1), dict(B=3, m_max=2, r_len=7), dict(m_max=9, r_len=9, live=8),
                 dict(live=-1), dict(W=1025), dict(W=0)):
        assert push(**over) != 0, over
        msg = lib.tg_last_error()
        assert b"tg_wide_pool_push_resampled: outside the envelope" in msg, (over, msg)
    for over in (dict(hdr=None), dict(samples=None), dict(m_max=1, r_len=1, recs=None), dict(taps=None), dict(carry=None), dict(consumed=None),
                 dict(produced=None), dict(ring=None)):
        assert push(**over) != 0 and b"tg_wide_pool_push_resampled: null pointer" in lib.tg_last_error(), over
