"""The input_sr keyword of the synthesis entry points on the GPU.  Everything downstream of the resampler is the existing 16 kHz path, so the
yardstick is always that path fed synthesize.resample_audio's output: bit equality, no tolerance.  The streams resample chunk by chunk
(csrc/resample.hip's stream kernel, bit-equal to the offline one: tests/test_resample_gpu.py); their utterance lengths are chosen so that
stream_matches_offline holds for the RESAMPLED length (asserted here, on the host, before anything runs)."""
import numpy as np
import pytest
import torch

import stream_ref as R
import utterance_ref as U
from stream_pool_ref import bits
from test_s2g_synthesis_gpu import make_generator, s2g_args, utterance
from test_utterance_gpu import joint_embed, multimodal, seq2seq          # noqa: F401  (the small models of the on-device utterance tests)

pytestmark = pytest.mark.gpu
S, A, T, STRIDE, N_PRE = R.S, R.A, U.N_POSES, U.STRIDE, U.N_PRE
TWO_WINDOWS, ONE_WINDOW = 48000, 20001                                   # 16 kHz lengths (3 s; under one window)


@pytest.fixture(scope="module")
def syn(pkg):
    return pkg.synthesize


def audio_at(sr, n16, seed):
    """Noise at `sr` whose resampled length is exactly n16."""
    n = -(-n16 * sr // 16000)
    while -(-n * 16000 // sr) > n16:
        n -= 1
    assert -(-n * 16000 // sr) == n16
    return U.make_audio(n, seed)


def count_calls(pkg, monkeypatch):
    """Counts the library entries the ops layer calls, by name."""
    seen, real = {}, pkg.ops.call

    def counting(name, *a):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a)
    monkeypatch.setattr(pkg.ops, "call", counting)
    return seen


def test_offline_multimodal_equals_the_16k_call_on_the_resampled_audio(pkg, syn, dev, multimodal, monkeypatch):
    args, G, draws = multimodal
    audio = audio_at(48000, TWO_WINDOWS, 1)
    words = R.words_until(R.WORDS, TWO_WINDOWS / U.SR)
    kw = dict(vids=[3], _draws=[d[[0]] for d in draws], on_device=True)
    a16 = syn.resample_audio(audio, 48000)
    assert a16.shape == (TWO_WINDOWS,) and a16.dtype == np.float32 and syn.num_windows(len(a16) / U.SR) == 2
    want = syn.generate_gestures_batch(args, G, U.Lang(), [a16], [words], **kw)[0]
    seen = count_calls(pkg, monkeypatch)
    got = syn.generate_gestures_batch(args, G, U.Lang(), [audio], [words], input_sr=48000, **kw)[0]
    assert seen.get("tg_resample") == 1                                                    # one launch for the batch
    assert got.shape == want.shape == (2 * STRIDE + N_PRE, U.D) and np.array_equal(bits(got), bits(want))
    one = syn.generate_gestures(args, G, U.Lang(), audio, words, vid=3, _draws=kw["_draws"], on_device=True, input_sr=48000)
    assert np.array_equal(bits(one), bits(want))
    host = syn.generate_gestures_batch(args, G, U.Lang(), [audio], [words], vids=[3], _draws=kw["_draws"], input_sr=48000)[0]     # the host window loop
    assert np.array_equal(bits(host), bits(syn.generate_gestures_batch(args, G, U.Lang(), [a16], [words], vids=[3], _draws=kw["_draws"])[0]))
    dev16 = syn.resample_audio([audio], 48000, device=dev, return_device=True)[0]
    assert dev16.is_cuda and np.array_equal(bits(dev16), bits(a16))
    with pytest.raises(ValueError, match="audio_sr must be 16000"):
        syn.generate_gestures_batch(args, G, U.Lang(), [audio], [words], audio_sr=48000, input_sr=48000, **kw)


def test_offline_speech2gesture_equals_the_16k_call_on_the_resampled_audio(pkg, syn, dev):
    """Through the log-mel path.  6.3 s: the shortest utterance the generator takes is (128 + 70 - 2) * 512 samples, so three windows."""
    gen = make_generator(pkg, dev)
    a16_len = int(6.3 * 16000)
    audio = utterance(6.3, 2)
    x48 = np.interp(np.arange(3 * a16_len) / 3.0, np.arange(a16_len), audio).astype(np.float32)      # some 48 kHz signal of the same duration
    a16 = syn.resample_audio(x48, 48000)
    assert len(a16) == a16_len
    want = syn.generate_gestures_batch(s2g_args(), gen, None, [a16], None, on_device=True)[0]
    got = syn.generate_gestures_batch(s2g_args(), gen, None, [x48], None, on_device=True, input_sr=48000)[0]
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def test_gesture_stream_at_44100_in_441_sample_chunks(pkg, syn, dev, multimodal):
    args, G, draws = multimodal
    assert syn.stream_matches_offline(args, TWO_WINDOWS)
    audio = audio_at(44100, TWO_WINDOWS, 2)
    a16 = syn.resample_audio(audio, 44100, device=dev, return_device=True)
    dr = [d[[0]] for d in draws]
    want = syn.generate_gestures_batch(args, G, U.Lang(), [a16], [R.words_until(R.WORDS, TWO_WINDOWS / U.SR)], vids=[3], _draws=dr, on_device=True)[0]
    st = syn.GestureStream(args, G, U.Lang(), vids=[3], _draws=dr, max_chunk=441, input_sr=44100)
    assert st.state["R"] == A + 160 + 1 and st.chunk_buf.shape == (1, 161)
    pieces = []
    for p in range(0, len(audio), 441):
        q = min(p + 441, len(audio))
        pieces.append(st.push(audio[p:q], R.words_until(R.WORDS, q / 44100, p / 44100)))
        assert sum(x.shape[1] for x in pieces) == syn.complete_windows(st.pushed, S, A) * STRIDE
    assert st.pushed == st._rs_out[0] < TWO_WINDOWS and st._rs_in[0] == len(audio)         # the filter's delay: the last samples are not final yet
    pieces.append(st.close())
    got = torch.cat(pieces, dim=1)[0]
    assert st.pushed == TWO_WINDOWS and st.late_words == 0
    assert st.rs["consumed"].tolist() == [len(audio)] and st.rs["produced"].tolist() == [TWO_WINDOWS]
    assert tuple(got.shape) == want.shape and np.array_equal(bits(got), bits(want))


def test_stream_pool_at_48000_two_sessions_joining_at_different_times(pkg, syn, dev, multimodal):
    args, G, draws = multimodal
    n16 = [TWO_WINDOWS, ONE_WINDOW]
    assert all(syn.stream_matches_offline(args, n) for n in n16)
    audios = [audio_at(48000, n, 10 + b) for b, n in enumerate(n16)]
    words = [R.words_until(R.ROW_WORDS[b], n / U.SR) for b, n in enumerate(n16)]
    a16 = syn.resample_audio(audios, 48000, device=dev, return_device=True)
    want, want_j = syn.generate_gestures_batch(args, G, U.Lang(), a16, words, vids=[3, 9], _draws=[d[[0, 1]] for d in draws], on_device=True,
                                               fade_out=True, joints=True)
    pool = syn.StreamPool(args, G, U.Lang(), slots=2, _replay_draws=True, max_chunk=4800, input_sr=48000)
    got, got_j, pos, chunk = [[], []], [[], []], [0, 0], [4800, 3001]
    slot = [pool.open(vid=3, _draws=[d[0] for d in draws]), None]

    def piece(b):
        p, q = pos[b], min(pos[b] + chunk[b], len(audios[b]))
        pos[b] = q
        return audios[b][p:q], R.words_until(R.ROW_WORDS[b], q / 48000, p / 48000)

    step = 0
    while slot[0] is not None or slot[1] is not None or step < 6:
        if step == 5:                                                                     # the second session joins after 24 000 input samples of the first
            slot[1] = pool.open(vid=9, _draws=[d[1] for d in draws])
            assert pool._rs_in == [24000, 0]
        live = [b for b in range(2) if slot[b] is not None and pos[b] < len(audios[b])]
        if live:
            res = pool.push({slot[b]: piece(b) for b in live}, joints=True)
            for b in live:
                got[b].append(res[slot[b]][0].clone()); got_j[b].append(res[slot[b]][1].clone())
        for b in range(2):
            if slot[b] is not None and pos[b] >= len(audios[b]):
                f, j = pool.close(slot[b], fade_out=True, joints=True)
                got[b].append(f.clone()); got_j[b].append(j.clone())
                slot[b] = None
        step += 1
    assert pool.rs["consumed"].tolist() == [len(a) for a in audios] and pool.rs["produced"].tolist() == n16       # read once, by the test only
    for b in range(2):
        assert np.array_equal(bits(torch.cat(got[b])), bits(want[b])), b
        assert np.array_equal(bits(torch.cat(got_j[b])), bits(want_j[b])), b


def test_seq2seq_stream_and_pool_one_window(pkg, syn, dev, seq2seq):
    args, net = seq2seq
    assert syn.stream_matches_offline(args, ONE_WINDOW)
    audio = audio_at(48000, ONE_WINDOW, 3)
    words = R.words_until(R.WORDS, ONE_WINDOW / U.SR)
    net.encoder.row_local_eval = True
    try:
        want = syn.generate_gestures_batch(args, net, U.Lang(), syn.resample_audio([audio], 48000, device=dev, return_device=True), [words],
                                           on_device=True)[0]
    finally:
        net.encoder.row_local_eval = False
    cuts = list(range(0, len(audio), 6000)) + [len(audio)]
    st = syn.Seq2SeqGestureStream(args, net, U.Lang(), max_chunk=6000, input_sr=48000)
    pieces = [st.push(audio[p:q], R.words_until(R.WORDS, q / 48000, p / 48000)) for p, q in zip(cuts, cuts[1:])] + [st.close()]
    assert np.array_equal(bits(torch.cat(pieces, dim=1)[0]), bits(want))
    pool = syn.Seq2SeqStreamPool(args, net, U.Lang(), slots=1, max_chunk=6000, input_sr=48000)
    s = pool.open()
    pieces = [pool.push({s: (audio[p:q], R.words_until(R.WORDS, q / 48000, p / 48000))})[s] for p, q in zip(cuts, cuts[1:])] + [pool.close(s)]
    assert np.array_equal(bits(torch.cat(pieces)), bits(want))


@pytest.mark.parametrize("input_sr", [None, 16000])
def test_16k_streams_keep_their_bits_and_launch_no_resample_kernel(pkg, syn, dev, multimodal, monkeypatch, input_sr):
    args, G, draws = multimodal
    n, dr = R.LENGTHS["A_plus_1"], [d[[0]] for d in draws]
    audio = U.make_audio(n, 4)
    want = syn.generate_gestures_batch(args, G, U.Lang(), [audio], [[]], vids=[3], _draws=dr, on_device=True)[0]
    seen = count_calls(pkg, monkeypatch)
    st = syn.GestureStream(args, G, U.Lang(), vids=[3], _draws=dr, max_chunk=5000, input_sr=input_sr)
    assert st.rs is None and st.state["R"] == A + 5000 and st.chunk_buf.shape == (1, 5000)
    pieces = [st.push(audio[p:p + 5000]) for p in range(0, n, 5000)] + [st.close()]
    assert np.array_equal(bits(torch.cat(pieces, dim=1)[0]), bits(want))
    assert "tg_resample_stream" not in seen and "tg_resample" not in seen and seen["tg_stream_push"] == len(pieces) - 1


def test_a_refused_push_changes_nothing_on_host_or_device(pkg, syn, dev, multimodal):
    args, G, draws = multimodal
    st = syn.GestureStream(args, G, U.Lang(), vids=[3], _draws=[d[[0]] for d in draws], max_chunk=480, input_sr=48000, word_ring=4)
    st.push(U.make_audio(480, 5))

    def snapshot():
        dev_state = [t.clone() for t in (st.rs["carry"], st.rs["consumed"], st.rs["produced"], st.state["ring"], st.state["written"], st.state["n_words"],
                                         st.state["words"])]
        return dev_state, (st.pushed, list(st._rs_in), list(st._rs_out), st.next_window, st.late_words, list(st._n_rec))
    before = snapshot()
    assert before[1][:3] == (160 - 57 // 3, [480], [160 - 57 // 3])                       # (480 - K/2) / 3 outputs are final: K = 114
    for bad, why in ((np.zeros(481, np.float32), "max_chunk is 480"), (np.zeros(10, np.float64), "must be float32"),
                     (np.zeros((2, 10), np.float32), "expected")):
        with pytest.raises(ValueError, match=why):
            st.push(bad)
    with pytest.raises(ValueError, match="word ring's capacity"):
        st.push(U.make_audio(480, 6), R.WORDS)
    after = snapshot()
    assert after[1] == before[1] and all(torch.equal(a, b) for a, b in zip(after[0], before[0]))
    with pytest.raises(ValueError, match="a ring of"):
        syn.GestureStream(args, G, U.Lang(), max_chunk=480, input_sr=48000, ring=A + 160)
    pool = syn.StreamPool(args, G, U.Lang(), slots=2, max_chunk=480, input_sr=48000)
    s = pool.open()
    pool.push({s: U.make_audio(480, 7)})
    keep = [t.clone() for t in (pool.rs["carry"], pool.rs["consumed"], pool.rs["produced"], pool.state["written"])]
    with pytest.raises(ValueError, match="max_chunk = 480"):
        pool.push({s: np.zeros(481, np.float32)})
    assert all(torch.equal(a, b) for a, b in zip(keep, (pool.rs["carry"], pool.rs["consumed"], pool.rs["produced"], pool.state["written"])))
    s2 = pool.open()                                                                      # opening a slot resets ITS carry and counters only
    assert pool.rs["consumed"].tolist() == [480, 0] and torch.equal(pool.rs["carry"][0], keep[0][0]) and not bool(pool.rs["carry"][s2].any())
