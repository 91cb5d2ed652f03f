"""Host side of the Human3.6M feed (no GPU): the stored fixture is self-consistent, the module's window table equals the reference's starts,
the numpy restatements of both stages reproduce the reference within the bounds of tests/h36m_bounds.py, the C ABI declares and validates
the new entries, and bad inputs raise ValueError."""
import ctypes as C
import os

import numpy as np
import pytest

import h36m_bounds as HB
import h36m_inputs as HI
from conftest import ROOT


@pytest.fixture(scope="module")
def gold():
    return HB.load_gold()


@pytest.fixture(scope="module")
def positions():
    return HI.make_positions()


def test_fixture_is_self_consistent(gold):
    counts = dict(zip([a[2] for a in HI.ACTIONS], HI.window_counts()))
    assert (counts[67], counts[68], counts[77], counts[78]) == (0, 1, 1, 2)
    acts = HB.listed_actions(gold)
    assert {s for _, s, _, _ in acts} == {"S1", "S5", "S11"}                    # S2 is not a listed subject
    n_train = sum(HI.window_counts()[a] for a, *_ in acts)
    assert len(gold["train_win"]) == n_train == len(gold["poses"]) == len(gold["dir_vec"])
    assert len(gold["test_win"]) == sum(HI.window_counts()[a] for a, s, _, _ in acts if s == "S11") == len(gold["test_in_train"])
    assert np.array_equal(gold["train_win"][gold["test_in_train"]], gold["test_win"])
    for a, _, _, n in acts:
        assert gold[f"norm_{a}"].shape == (n, 10, 3) and gold[f"norm_{a}"].dtype == np.float32
    assert gold["poses"].dtype == np.float32 and gold["dir_vec"].dtype == np.float32 and gold["mean_dir_vec"].shape == (27,)
    large = gold["aug_rand"] < 0.2
    assert large.any() and not large.all() and np.array_equal(gold["aug_std"], np.where(large, 0.002 ** 0.5, 0.0001 ** 0.5))
    for k in range(len(gold["aug_index"])):
        HB.recorded_noise(gold, k)
    # the zero-length bone: exactly zero in the reference's normalised frames, its direction vector exactly minus the mean
    zero = [a for a, act in enumerate(HI.ACTIONS) if act[5]][0]
    x = gold[f"norm_{zero}"]
    assert (x[:, 3] == x[:, 2]).all()
    w = [i for i, (a, _) in enumerate(gold["train_win"]) if a == zero]
    assert w and np.array_equal(gold["dir_vec"][w][:, :, 6:9], np.broadcast_to((-gold["mean_dir_vec"][6:9]).astype(np.float32), (len(w), 34, 3)))


def test_window_table_equals_the_reference_starts(pkg, gold, positions):
    H = pkg.h36m
    assert [len(H.window_starts(n)) for n in (67, 68, 77, 78, 198)] == [0, 1, 1, 2, 14]
    for is_train, key in ((True, "train_win"), (False, "test_win")):
        actions, win_row0, arrays = H.window_table(positions, is_train)
        assert [s for s, *_ in actions] == [a[0] for a in HI.ACTIONS if a[0] in (H.TRAIN_SUBJECTS if is_train else H.TEST_SUBJECTS)]
        first_row = {(s, name): r for s, name, r, _ in actions}
        ref = [first_row[(HI.ACTIONS[a][0], HI.ACTIONS[a][1])] + f for a, f in gold[key]]
        assert win_row0.tolist() == ref and win_row0.dtype == np.int64
        assert sum(len(a) for a in arrays) == sum(n for *_, n in actions)
    assert H.TRAIN_SUBJECTS == ("S1", "S5", "S6", "S7", "S8", "S9", "S11") and H.TEST_SUBJECTS == ("S11",)


def test_normalize_restatement_matches_the_reference(pkg, gold, positions):
    for a, subject, name, n in HB.listed_actions(gold):
        mine = pkg.h36m.normalize_numpy(positions[subject][name])
        assert mine.shape == (n, 30) and mine.dtype == np.float32
        HB.assert_stage_a(mine, gold[f"norm_{a}"], positions[subject][name], f"{subject} {name}")


def test_samples_restatement_matches_the_reference(pkg, gold):
    H = pkg.h36m
    skel, win = HB.packed_reference(gold)
    poses, vec = H.samples_numpy(skel, win, gold["mean_dir_vec"])
    assert poses.dtype == np.float32 and vec.dtype == np.float32
    HB.assert_stage_b(poses, vec, gold["poses"], gold["dir_vec"], "augment=False")
    idx = gold["aug_index"]
    noise = np.stack([HB.recorded_noise(gold, k) for k in range(len(idx))])
    poses, vec = H.samples_numpy(skel, win[idx], gold["mean_dir_vec"], noise=noise)
    HB.assert_stage_b(poses, vec, gold["aug_poses"], gold["aug_dir_vec"], "recorded noise")


def test_header_declares_the_entries_and_validation_fires(pkg):
    header = open(os.path.join(ROOT, "include", "trimodal_hip.h")).read()
    for name in ("tg_h36m_normalize", "tg_h36m_samples"):
        assert name in pkg._lib.SIGNATURES
    assert "added under ABI 11" in header
    lib = pkg._lib.load()
    assert lib.tg_version() == 11
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    f = C.c_float
    assert lib.tg_h36m_normalize(p, 10, 27, p, None) != 0 and b"tg_h36m_normalize: n_joints" in lib.tg_last_error()
    assert lib.tg_h36m_normalize(p, 0, 32, p, None) != 0 and b"tg_h36m_normalize: rows" in lib.tg_last_error()
    assert lib.tg_h36m_normalize(None, 10, 32, p, None) != 0 and b"tg_h36m_normalize: NULL" in lib.tg_last_error()
    ok = dict(skel=p, rows=100, tab=p, tab_bytes=16, W=2, n=34, stride=2, mean=p, mean_bytes=216, noise=None, noise_bytes=0, st=None)

    def samples(**kw):
        a = dict(ok, **kw)
        return lib.tg_h36m_samples(a["skel"], a["rows"], a["tab"], a["tab_bytes"], a["W"], a["n"], a["stride"], a["mean"], a["mean_bytes"], a["noise"],
                                   a["noise_bytes"], a["st"], 1, 2, f(0.2), f(0.04), f(0.01), p, p, p, None)

    assert samples(tab_bytes=8) != 0 and b"tg_h36m_samples: window table" in lib.tg_last_error()
    assert samples(mean_bytes=208) != 0 and b"tg_h36m_samples: mean_dir_vec" in lib.tg_last_error()
    assert samples(stride=0) != 0 and b"frame_stride" in lib.tg_last_error()
    assert samples(noise=p, noise_bytes=2 * 34 * 30 * 8 - 8) != 0 and b"tg_h36m_samples: noise of" in lib.tg_last_error()
    assert samples(noise=p, noise_bytes=1 << 20, st=p) != 0 and b"both given" in lib.tg_last_error()
    assert samples(skel=None) != 0 and b"tg_h36m_samples: NULL" in lib.tg_last_error()
    assert samples(W=1, n=1, stride=1, rows=1, tab_bytes=1) != 0 and b"window table of 1 bytes" in lib.tg_last_error()


def test_bad_inputs_raise_value_error(pkg, positions):
    H = pkg.h36m
    mean = np.zeros(27)
    with pytest.raises(ValueError, match="J >= 28"):
        H.Human36M({"S1": {"a": np.zeros((80, 27, 3), dtype=np.float32)}}, mean, device="cpu")
    with pytest.raises(ValueError, match="float64"):
        H.Human36M({"S1": {"a": positions["S1"]["Eating"].astype(np.float64)}}, mean, device="cpu")
    with pytest.raises(ValueError, match="no action of the subjects"):
        H.Human36M({"S2": positions["S2"]}, mean, device="cpu")
    with pytest.raises(ValueError, match="no action of the subjects"):
        H.Human36M({"S1": positions["S1"]}, mean, is_train=False, device="cpu")     # S1 is not a test subject
    with pytest.raises(ValueError, match="27"):
        H.Human36M(positions, np.zeros(30), device="cpu")
    with pytest.raises(ValueError):
        H.normalize_numpy(np.zeros((4, 27, 3), dtype=np.float32))
