"""The Human3.6M feed on the device (csrc/h36m.hip) against the reference's results stored in tests/golden/g16_h36m.npz (made by
make_golden_h36m.py from the positions of tests/h36m_inputs.py) and, at shapes the fixture does not hold, against the fp64 numpy
restatement written in this file, independent of the package.  The bounds are those of tests/h36m_bounds.py; every element is compared.
The restatement performs the kernel's operations in the same order, so the same bounds hold against it (the two sides differ by libm only)."""
import math

import numpy as np
import pytest
import torch

import h36m_bounds as HB
import h36m_inputs as HI

pytestmark = pytest.mark.gpu

P_LARGE, STD_LARGE, STD_SMALL = 0.2, 0.002 ** 0.5, 0.0001 ** 0.5


@pytest.fixture(scope="module")
def gold():
    return HB.load_gold()


@pytest.fixture(scope="module")
def positions():
    return HI.make_positions()


@pytest.fixture(scope="module")
def packed(gold, dev):
    """The reference's normalised training actions packed on the device, the training windows' first rows, the mean."""
    skel, win = HB.packed_reference(gold)
    return torch.from_numpy(skel).to(dev), torch.from_numpy(win).to(dev), torch.from_numpy(gold["mean_dir_vec"]).to(dev)


def _samples(pkg, skel, win, mean, n_poses=34, stride=2, noise=None, rng=None, guard=False):
    W, dev = win.numel(), skel.device
    poses = torch.full((W + int(guard), n_poses, 30), 7.0, device=dev)
    vec = torch.full((W + int(guard), n_poses, 27), 7.0, device=dev)
    flag = torch.full((W + int(guard),), 7, device=dev, dtype=torch.int32)
    pkg.ops.h36m_samples(skel, win, n_poses, stride, mean, poses[:W], vec[:W], flag[:W], noise=noise, rng=rng)
    return poses, vec, flag


# ---------------------------------------------------------------------------------------------------------------- this file's restatement
def _normalize_ref(pos):
    """Human36M.normalize frame by frame: fp32 where numpy works on the fp32 array, Python floats (fp64) for the angle and the matrix."""
    g = pos[:, list(HI.TARGET_JOINTS)].copy()
    out = np.zeros((len(g), 10, 3), dtype=np.float32)
    for f in range(len(g)):
        d = g[f] - g[f, 2]
        d = np.stack([d[:, 0], -d[:, 2], d[:, 1]], axis=1)
        assert d.dtype == np.float32
        hip = d[1] - d[0]
        angle = math.pi - math.atan2(float(hip[2]), float(hip[0]))
        deg = angle * (180.0 / math.pi)
        if 180 > deg > 0:
            pass
        elif 180 < deg < 360:
            angle = angle - 360.0 * (math.pi / 180.0)
        a, c = math.cos(angle / 2.0), -math.sin(angle / 2.0)
        aa, cc, ac = a * a, c * c, a * c
        rot = np.array([[aa - cc, 0.0, 2.0 * (0.0 - ac)], [0.0, aa + cc, 0.0], [2.0 * (0.0 + ac), 0.0, aa - cc]])
        x = d.astype(np.float64)
        r = x[:, 0:1] * rot[0] + x[:, 1:2] * rot[1] + x[:, 2:3] * rot[2]
        out[f] = r[2:].astype(np.float32)
    return out.reshape(len(g), 30)


def _unit(d):
    n = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    return d / np.where(n == 0.0, 1.0, n)[..., None]


def _samples_ref(skel, win, mean, n_poses, stride, noise=None):
    poses, vec = [], []
    for w, r0 in enumerate(win):
        x = skel[r0 + stride * np.arange(n_poses)].reshape(n_poses, 10, 3)
        p = np.zeros((n_poses, 10, 3))
        for a, b, length in HI.BONES:
            p[:, b] = p[:, a] + length * _unit((x[:, b] - x[:, a]).astype(np.float64))
        if noise is not None:
            p = p + noise[w].reshape(n_poses, 10, 3)
        v = np.stack([_unit(p[:, b] - p[:, a]) for a, b, _ in HI.BONES], axis=1).reshape(n_poses, 27) - mean
        poses.append(p.astype(np.float32).reshape(n_poses, 30))
        vec.append(v.astype(np.float32))
    return np.stack(poses), np.stack(vec)


# ---------------------------------------------------------------------------------------------------------------- against the fixture
def test_stage_a_matches_the_reference(pkg, dev, gold, positions):
    acts = HB.listed_actions(gold)
    raw = np.concatenate([positions[s][name] for _, s, name, _ in acts])
    out = pkg.ops.h36m_normalize(torch.from_numpy(raw).to(dev)).cpu().numpy()
    r = 0
    for a, s, name, n in acts:
        HB.assert_stage_a(out[r:r + n], gold[f"norm_{a}"], positions[s][name], f"{s} {name}")
        r += n
    assert r == len(out)


def test_stage_b_matches_the_reference(pkg, dev, gold, packed):
    skel, win, mean = packed
    poses, vec, flag = _samples(pkg, skel, win, mean)
    assert (flag == 0).all()
    HB.assert_stage_b(poses.cpu().numpy(), vec.cpu().numpy(), gold["poses"].reshape(-1, 34, 30), gold["dir_vec"], "augment=False")
    zero = [a for a, act in enumerate(HI.ACTIONS) if act[5]][0]
    w = [i for i, (a, _) in enumerate(gold["train_win"]) if a == zero]
    expect = torch.from_numpy((-gold["mean_dir_vec"][6:9]).astype(np.float32)).to(dev)
    assert w and (vec[w][:, :, 6:9] == expect).all()                    # the zero-length bone: exact zeros, minus the mean
    assert (poses[w][:, :, 9:12] == poses[w][:, :, 6:9]).all()
    idx = gold["aug_index"]
    noise = np.stack([HB.recorded_noise(gold, k) for k in range(len(idx))]).reshape(len(idx), 34, 30)
    poses, vec, flag = _samples(pkg, skel, win[torch.from_numpy(idx).to(dev)], mean, noise=torch.from_numpy(noise).to(dev))
    assert (flag == 0).all()
    HB.assert_stage_b(poses.cpu().numpy(), vec.cpu().numpy(), gold["aug_poses"].reshape(-1, 34, 30), gold["aug_dir_vec"], "recorded noise")


def test_end_to_end_matches_the_reference(pkg, dev, gold, positions):
    H = pkg.h36m
    train = H.Human36M(positions, gold["mean_dir_vec"], is_train=True, device=dev)
    test = H.Human36M(positions, gold["mean_dir_vec"], is_train=False, device=dev)
    assert len(train) == len(gold["train_win"]) and len(test) == len(gold["test_win"])
    assert train.skel.shape == (sum(n for *_, n in HB.listed_actions(gold)), 30)
    poses, vec = train.build(check=True)
    assert poses.shape == (len(train), 34, 10, 3) and vec.shape == (len(train), 34, 27) and poses.dtype == vec.dtype == torch.float32
    vec = vec.cpu().numpy().astype(np.float64)
    for i, (a, f) in enumerate(gold["train_win"]):
        bound = HB.end_to_end_vec_bound(gold[f"norm_{a}"][f:f + 68:2])
        err = np.abs(vec[i] - gold["dir_vec"][i].astype(np.float64))
        assert (err <= bound).all(), (i, float(np.max(err / bound)))
    t_poses, t_vec = test.build()
    sel = torch.from_numpy(gold["test_in_train"]).to(dev)
    assert torch.equal(t_vec, train.build(sel)[1]) and torch.equal(t_poses, poses.index_select(0, sel))
    p, v = train[3]
    assert p.shape == (34, 10, 3) and v.shape == (34, 27) and p.is_cuda and torch.equal(p, poses[3]) and torch.equal(v, train.build([3])[1][0])
    with pytest.raises(IndexError):
        train[len(train)]
    train.build(torch.tensor([0, len(train)], device=dev))               # a device index outside the dataset: flagged, not read
    assert train.last_flag.tolist() == [0, -1]
    # a small normalisation batch gives the same buffer as one launch over everything
    assert torch.equal(H.Human36M(positions, gold["mean_dir_vec"], device=dev, batch_frames=100).skel, train.skel)


# ---------------------------------------------------------------------------------------------------------------- drawn noise
def test_drawn_noise_equals_given_noise(pkg, dev, packed):
    ops = pkg.ops
    skel, win, mean = packed
    W = 4096
    table = win[torch.arange(W, device=dev) % win.numel()].contiguous()
    state = ops.new_rng_state(1234, dev)
    ops.rng_advance(state)
    noise_site, select_site = 11, 12
    rng = (state, noise_site, select_site, P_LARGE, STD_LARGE, STD_SMALL)
    drawn = _samples(pkg, skel, table, mean, rng=rng)
    z = ops.normal(torch.empty(W * 34 * 30, device=dev), state, noise_site).view(W, 34, 30)
    mask = ops.dropout_mask(torch.empty(W, device=dev), P_LARGE, state, select_site)
    std = torch.where(mask == 0, torch.tensor(STD_LARGE, device=dev, dtype=torch.float32), torch.tensor(STD_SMALL, device=dev, dtype=torch.float32))
    given = _samples(pkg, skel, table, mean, noise=z.double() * std.double()[:, None, None])
    assert torch.equal(drawn[0], given[0]) and torch.equal(drawn[1], given[1]) and (drawn[2] == 0).all()
    share = float((mask == 0).float().mean())
    assert abs(share - P_LARGE) <= 5.0 * math.sqrt(P_LARGE * (1 - P_LARGE) / W), share
    # the draws do not depend on the length of the call: the first 5 slots of a shorter launch are the same values
    short = _samples(pkg, skel, table[:5].contiguous(), mean, rng=rng)
    assert torch.equal(short[0], drawn[0][:5]) and torch.equal(short[1], drawn[1][:5])
    again = _samples(pkg, skel, table, mean, rng=rng)                     # bitwise repeatable
    assert torch.equal(again[0], drawn[0]) and torch.equal(again[1], drawn[1])


def test_augmented_batches_differ(pkg, dev, gold, positions):
    ds = pkg.h36m.Human36M(positions, gold["mean_dir_vec"], augment=True, device=dev, seed=5)
    plain = pkg.h36m.Human36M(positions, gold["mean_dir_vec"], augment=False, device=dev)
    idx = [0, 1, 2, 3]
    a, b = ds.build(idx), ds.build(idx)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])    # the state advances between launches
    clean = plain.build(idx)
    d = (a[0] - clean[0]).abs()
    assert 0 < float(d.max()) < 8 * STD_LARGE                               # noise of the reference's size on the rebuilt joints
    assert torch.equal(ds.build(idx, noise=np.zeros((4, 34, 30)))[1], clean[1])
    batches = list(ds.batches(8, shuffle=False))
    assert len(batches) == len(ds) // 8 and not torch.equal(batches[0][1], plain.build(list(range(8)))[1])


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("rows,joints", [(1, 32), (63, 32), (64, 28), (65, 32), (4097, 32)])
def test_stage_a_row_counts(pkg, dev, rows, joints):
    rs = np.random.RandomState(rows)
    pos = np.concatenate([HI.make_action(rs, min(rows - r, 500), 360.0 * rs.rand(), 300.0, False, ()) for r in range(0, rows, 500)])[:, :joints]
    pos = np.ascontiguousarray(pos)
    out = torch.full((rows + 1, 30), 7.0, device=dev)
    pkg.ops.h36m_normalize(torch.from_numpy(pos).to(dev), out[:rows])
    assert (out[rows] == 7.0).all()                                       # the guard row after the output
    HB.assert_stage_a(out[:rows].cpu().numpy(), _normalize_ref(pos), pos, f"{rows} rows")


@pytest.mark.parametrize("n_poses,stride", [(34, 2), (1, 1), (130, 1), (34, 3)])
def test_stage_b_shapes(pkg, dev, gold, packed, n_poses, stride):
    skel, _, mean = packed
    F = skel.shape[0]
    span = (n_poses - 1) * stride
    win = np.array([0, 17, F - 1 - span, 5, 200], dtype=np.int64)         # the last possible window included
    noise = np.random.RandomState(n_poses).normal(0, 0.01, (len(win), n_poses, 30))
    ref = _samples_ref(skel.cpu().numpy(), win, gold["mean_dir_vec"], n_poses, stride, noise)
    poses, vec, flag = _samples(pkg, skel, torch.from_numpy(win).to(dev), mean, n_poses, stride, noise=torch.from_numpy(noise).to(dev), guard=True)
    assert flag.tolist() == [0] * len(win) + [7] and (poses[-1] == 7.0).all() and (vec[-1] == 7.0).all()
    HB.assert_stage_b(poses[:-1].cpu().numpy(), vec[:-1].cpu().numpy(), ref[0], ref[1], f"n_poses {n_poses}, stride {stride}")


def test_out_of_range_table_entries_are_flagged(pkg, dev, gold, packed):
    skel, _, mean = packed
    F = skel.shape[0]
    win = np.array([0, F - 67, 10, -1, F - 66, 1 << 62, 20, -(1 << 62)], dtype=np.int64)       # F - 67 is the last window that fits
    poses, vec, flag = _samples(pkg, skel, torch.from_numpy(win).to(dev), mean, guard=True)
    assert flag.tolist() == [0, 0, 0, -1, -1, -1, 0, -1, 7]
    good = [0, 1, 2, 6]
    ref = _samples_ref(skel.cpu().numpy(), win[good], gold["mean_dir_vec"], 34, 2)
    HB.assert_stage_b(poses[good].cpu().numpy(), vec[good].cpu().numpy(), ref[0], ref[1], "neighbours of bad entries")
    bad = [3, 4, 5, 7, 8]                                                 # nothing written for a flagged window, nor past the output
    assert (poses[bad] == 7.0).all() and (vec[bad] == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- the training loop
def test_train_autoencoder(pkg, dev, tmp_path):
    H, fgd = pkg.h36m, pkg.fgd
    args = pkg.config.load_config("gesture_autoencoder", epochs=3, batch_size=64, name="h36m_test", model_save_path=str(tmp_path))
    mean = np.squeeze(np.array(args.mean_dir_vec))
    data = H.synthetic_dataset(seed=3, actions_per_subject=2, n_frames=600)          # 54 windows per action: 324 training, 108 validation
    train = H.Human36M(data, mean, is_train=True, device=dev, seed=1)
    val = H.Human36M(data, mean, is_train=False, device=dev)
    assert len(train) == 324 and len(val) == 108
    # one epoch of shuffled batches: every sample at most once, the remainder dropped
    everything = train.build()[1]
    key = {everything[i, 0].cpu().numpy().tobytes(): i for i in range(len(train))}
    assert len(key) == len(train)
    seen = [key[v[0].cpu().numpy().tobytes()] for _, vec in train.batches(64, shuffle=True) for v in vec]
    assert len(seen) == 5 * 64 and len(set(seen)) == len(seen) and seen != sorted(seen)
    assert sum(len(v) for _, v in train.batches(64, shuffle=False, drop_last=False)) == 324
    lines = []
    torch.manual_seed(0)
    best, history = fgd.train_autoencoder(args, train, val, log=lines.append)
    assert [h["epoch"] for h in history] == [0, 1, 2] and all(np.isfinite(h["val_loss"]) and np.isfinite(h["train_loss"]) for h in history)
    assert history[2]["train_loss"] < history[0]["train_loss"], history
    assert best == min(((h["val_loss"], h["epoch"]) for h in history), key=lambda t: t[0])
    path = tmp_path / "h36m_test_checkpoint_best.bin"
    ckpt = pkg.checkpoint.load_checkpoint(str(path), dev)
    assert ckpt["epoch"] == best[1] and ckpt["pose_dim"] == 27 and set(ckpt) == {"args", "epoch", "pose_dim", "gen_dict"}
    evaluator = fgd.EmbeddingSpaceEvaluator(args, str(path), None, dev)
    # the stored weights give the validation loss logged for their epoch again (the same kernels on the same batches; rel 1e-6 leaves room
    # for a reduction that is ordered differently from run to run, a few fp32 ulps)
    again = fgd.evaluate_testset(val.batches(64, shuffle=False), evaluator.net)["loss"]
    assert again == pytest.approx(best[0], rel=1e-6)
    assert any("BEST VALIDATION LOSS: {:.3f}".format(best[0]) in line for line in lines) and any("samples/s" in line for line in lines)
