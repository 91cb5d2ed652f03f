"""Speech2Gesture baseline, host side: init_model builds both nets, their state_dict layout and parameter counts are the reference's
(tests/golden/golden_s2g_keys.json, from make_golden_s2g.py), the TF "SAME" padding rule, and the config."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLDEN, "golden_s2g_keys.json")) as f:
        return json.load(f)


def _nets(pkg):
    args = pkg.config.load_config("speech2gesture")
    return pkg.checkpoint.init_model(args, None, None, 27, "cpu")


def test_init_model_builds_speech2gesture(pkg):
    from importlib import import_module
    s2g = import_module(pkg.__name__ + ".speech2gesture")
    g, d, loss_fn = _nets(pkg)
    assert isinstance(g, s2g.Generator) and isinstance(d, s2g.Discriminator)
    assert type(loss_fn).__name__ == "L1Loss"


def test_state_dict_layout_matches_reference(pkg, ref_keys):
    g, d, _ = _nets(pkg)
    for mod, ref, n_keys, n_params in ((g, ref_keys["gen"], 179, 6_438_347), (d, ref_keys["dis"], 18, 172_993)):
        sd = mod.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == ref
        assert len(sd) == n_keys and sum(p.numel() for p in mod.parameters()) == n_params
    assert ref_keys["gen_params"] == 6_438_347 and ref_keys["dis_params"] == 172_993


def test_same_padding_of_every_layer(pkg):
    from importlib import import_module
    same_pad = import_module(pkg.__name__ + ".layers").same_pad
    # 2-D audio encoder: (rows, cols) per block, k3 s1 keeps the size, k4 s2 halves it (35 columns: total 3 -> 1 left, 2 right)
    H, W = 128, 70
    for k, s, out in ((3, 1, (128, 70)), (4, 2, (64, 35)), (3, 1, (64, 35)), (4, 2, (32, 18)), (3, 1, (32, 18)), (4, 2, (16, 9)), (3, 1, (16, 9))):
        (ho, pt, pb), (wo, pl, pr) = same_pad(H, k, s), same_pad(W, k, s)
        assert (ho, wo) == out
        if k == 3:
            assert (pt, pb, pl, pr) == (1, 1, 1, 1)
        H, W = ho, wo
    assert same_pad(35, 4, 2) == (18, 1, 2) and same_pad(70, 4, 2) == (35, 1, 1) and same_pad(128, 4, 2) == (64, 1, 1)
    # 1-D U-Net downsampling 34 -> 17 -> 9 -> 5 -> 3 -> 2
    L = 34
    for want in (17, 9, 5, 3, 2):
        lo, left, right = same_pad(L, 4, 2)
        assert lo == want and (left, right) == ((1, 2) if L % 2 else (1, 1)), (L, left, right)
        L = lo
    assert same_pad(34, 3, 1) == (34, 1, 1)
    # discriminator: 33 -> 17 (k4 s2) -> 9 ... on motion; k4 s1 on 8 frames pads 1 left, 2 right
    assert same_pad(8, 4, 1) == (8, 1, 2) and same_pad(32, 4, 2) == (16, 1, 1) and same_pad(16, 4, 2) == (8, 1, 1)


def test_speech2gesture_config_loads(pkg):
    a = pkg.config.load_config("speech2gesture")
    assert a.model == "speech2gesture" and a.n_poses == 34 and a.n_pre_poses == 4 and a.batch_size == 128
    assert a.learning_rate == 0.001 and a.loss_regression_weight == 100 and a.loss_gan_weight == 10.0
    assert np.asarray(a.mean_dir_vec).size == 27 and a.motion_resampling_framerate == 15


def test_spectrogram_length(pkg):
    from importlib import import_module
    s2g = import_module(pkg.__name__ + ".speech2gesture")
    assert s2g.spectrogram_length(34, 15) == 70


def test_conv2d_wrappers_refuse_mismatched_tensors(pkg):
    """ops.conv2d_fwd / _dgrad / _wgrad take the batch and channel counts from one tensor: a second tensor that disagrees must raise in
    Python (before the device checks, so CPU tensors show it) instead of letting the kernel read past its end."""
    import torch
    ops = pkg.ops
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = 2, 10, 12, 3, 5, 3, 2, 2, 1, 0, 5, 6
    kw_ = dict(stride=s, pad_top=pt, pad_left=pl)
    x, y, w = torch.zeros(B, H, W, Ci), torch.zeros(B, Ho, Wo, Co), torch.zeros(Co, Ci, kh, kw)
    # batch counts
    with pytest.raises(AssertionError):
        ops.conv2d_fwd(x, w, None, torch.zeros(B + 1, Ho, Wo, Co), **kw_)
    with pytest.raises(AssertionError):
        ops.conv2d_dgrad(torch.zeros(B + 1, Ho, Wo, Co), w, x, **kw_)
    with pytest.raises(AssertionError):
        ops.conv2d_dgrad(y, w, torch.zeros(B - 1, H, W, Ci), **kw_)
    with pytest.raises(AssertionError):
        ops.conv2d_wgrad(torch.zeros(B + 1, Ho, Wo, Co), x, w, **kw_)
    # channel counts and the weight gradient's shape
    with pytest.raises(AssertionError):
        ops.conv2d_fwd(x, w, torch.zeros(Co + 1), y, **kw_)
    for bad in ((Co + 1, Ci, kh, kw), (Co, Ci + 1, kh, kw), (Ci, Co, kh, kw), (Co, Ci, kh * kw)):
        with pytest.raises(AssertionError):
            ops.conv2d_wgrad(y, x, torch.zeros(bad), **kw_)
    with pytest.raises(AssertionError):
        ops.conv2d_dgrad(y, torch.zeros(Co, Ci + 1, kh, kw), x, **kw_)
    # spatial sizes: an output whose last window starts past the input, along either axis, and an empty one
    for Ho_, Wo_ in ((Ho + 2, Wo), (Ho, Wo + 1), (0, Wo)):
        y_ = torch.zeros(B, Ho_, Wo_, Co)
        with pytest.raises(ValueError, match="does not fit"):
            ops.conv2d_fwd(x, w, None, y_, **kw_)
        with pytest.raises(ValueError, match="does not fit"):
            ops.conv2d_dgrad(y_, w, x, **kw_)
        with pytest.raises(ValueError, match="does not fit"):
            ops.conv2d_wgrad(y_, x, w, **kw_)
    # the consistent call gets past all of these and stops at the device check
    with pytest.raises((TypeError, ValueError), match="CUDA"):
        ops.conv2d_fwd(x, w, None, y, **kw_)
    with pytest.raises((TypeError, ValueError), match="CUDA"):
        ops.conv2d_dgrad(y, w, x, **kw_)
    with pytest.raises((TypeError, ValueError), match="CUDA"):
        ops.conv2d_wgrad(y, x, w, **kw_)
