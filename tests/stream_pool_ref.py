"""Shared pieces of tests/test_stream_pool_cpu.py and tests/test_stream_pool_gpu.py: a brute-force window schedule, a parameter-only stand-in
for a generator (a pool's host side can then be built without a device) and the sessions the GPU tests drive through a pool."""
import numpy as np
import torch

import stream_ref as R
import utterance_ref as U


def brute_rounds(pushed, next_window, S, A):
    """Round after round: the rows whose next window has all its samples run it, until no row has one."""
    nw, rounds = list(next_window), []
    while True:
        mask = [int(p >= w * S + A) for p, w in zip(pushed, nw)]
        if not any(mask):
            return rounds
        rounds.append(mask)
        nw = [w + a for w, a in zip(nw, mask)]


class HostGenerator(torch.nn.Module):
    """What WindowDecoder's constructor asks of a generator, on the CPU."""
    pose_dim = U.D

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


_audio = {}


def audio_of(n, b=0):
    if (n, b) not in _audio:
        _audio[n, b] = U.make_audio(n, 900 + 17 * b + n % 89)
    return _audio[n, b]


class Session:
    """One utterance on its way through a pool: `n` samples of row `b`'s audio and word list, pushed in pieces of `chunk` samples; every word goes
    with the piece that holds its start time.  frames / joints collect what push and close returned."""

    def __init__(self, n, b, chunk, words=None):
        self.n, self.b, self.chunk, self.pos, self.slot = n, b, chunk, 0, None
        self.audio, self.words = audio_of(n, b), R.ROW_WORDS[b] if words is None else words
        self.frames, self.joints = [], []

    @property
    def done(self):
        return self.pos >= self.n

    def offline_words(self):
        return R.words_until(self.words, self.n / U.SR)

    def piece(self):
        p, q = self.pos, min(self.pos + self.chunk, self.n)
        self.pos = q
        return self.audio[p:q], R.words_until(self.words, q / U.SR, p / U.SR)

    def take(self, res):
        f, j = res
        self.frames.append(f.clone()); self.joints.append(j.clone())

    def result(self):
        return torch.cat(self.frames), torch.cat(self.joints)


def push_all(pool, sessions):
    """One push with the next piece of every given session that still has audio."""
    sessions = [s for s in sessions if not s.done]
    res = pool.push({s.slot: s.piece() for s in sessions}, joints=True)
    for s in sessions:
        s.take(res[s.slot])
