"""The shared conv reference (tests/conv2d_ref.py) checked where there is no GPU: against F.conv2d's own symmetric padding, against
layers.same_pad on the model's eight audio-encoder blocks, the magnitude yardstick against the reference, and every geometry of the
envelope table against c2_check's conditions and c2_wgrad_plan's split counts (so that a later edit cannot quietly take a case off the
split path)."""
import pytest
import torch
import torch.nn.functional as F

from tests.conv2d_ref import (GEOMS, SPECTROGRAM_GEOM, SPECTROGRAM_SPLIT_PLAN, SPLIT_PLANS, geom_ok, magnitudes, operands, ref_all, ref_conv,
                              rejected_variants, wgrad_plan)


@pytest.mark.parametrize("H,W,kh,kw,s,p", [(9, 7, 3, 3, 1, 1), (10, 8, 4, 4, 2, 1), (7, 9, 5, 3, 1, 0), (8, 8, 1, 1, 2, 0), (11, 6, 3, 3, 2, 1)])
def test_ref_conv_equals_symmetric_conv2d(H, W, kh, kw, s, p):
    B, Ci, Co = 2, 3, 4
    Ho, Wo = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    geom = (B, H, W, Ci, Co, kh, kw, s, p, p, Ho, Wo)
    assert geom_ok(geom)
    x, w, b, dy = operands(geom, "balanced", 1)
    want = F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=s, padding=(p, p)).permute(0, 2, 3, 1)
    assert torch.equal(ref_conv(x, w, b, geom), want)


# (H, W, k, stride, VALID): the eight ConvNormRelu blocks of the audio encoder
BLOCKS = [(128, 70, 3, 1, False), (128, 70, 4, 2, False), (64, 35, 3, 1, False), (64, 35, 4, 2, False), (32, 18, 3, 1, False),
          (32, 18, 4, 2, False), (16, 9, 3, 1, False), (16, 9, 3, 1, True)]


@pytest.mark.parametrize("H,W,k,s,valid", BLOCKS)
def test_ref_conv_equals_same_pad_geometry(pkg, H, W, k, s, valid):
    from importlib import import_module
    same_pad = import_module(pkg.__name__ + ".layers").same_pad
    B, Ci, Co = 1, 2, 3
    if valid:
        (Ho, pt, pb), (Wo, pl, pr) = ((H - k) // s + 1, 0, 0), ((W - k) // s + 1, 0, 0)
    else:
        (Ho, pt, pb), (Wo, pl, pr) = same_pad(H, k, s), same_pad(W, k, s)
    geom = (B, H, W, Ci, Co, k, k, s, pt, pl, Ho, Wo)
    assert geom_ok(geom)
    x, w, b, dy = operands(geom, "balanced", 2)
    want = F.conv2d(F.pad(x.permute(0, 3, 1, 2), [pl, pr, pt, pb]), w, b, stride=s).permute(0, 2, 3, 1)
    assert tuple(want.shape) == (B, Ho, Wo, Co) and torch.equal(ref_conv(x, w, b, geom), want)


ALL = dict(GEOMS, spectrogram=SPECTROGRAM_GEOM)


@pytest.mark.parametrize("name", [n for n in ALL if n != "split_cap256"])
def test_magnitudes_bound_the_reference(name):
    geom = ALL[name]
    x, w, b, dy = operands(geom, "spectrogram" if name == "spectrogram" else "decades", 3, half=name == "spectrogram")
    for r, m in zip(ref_all(x, w, b, dy, geom), magnitudes(x, w, b, dy, geom)):
        assert r.shape == m.shape and bool((m >= 0).all())
        assert bool((r.abs() <= m * (1 + 1e-12)).all())            # (the two sums round differently in fp64)


def test_uncovered_elements_have_zero_magnitude():
    """Where no product contributes the yardstick is exactly 0: the odd positions and the last column of k1_s2's dx, the last row and
    column of valid_s2_uncovered's, and the taps of k8_gt_input that only ever see padding."""
    geom = GEOMS["k1_s2"]
    _, mx, _ = magnitudes(*operands(geom, "decades", 4), geom)
    cover = torch.zeros(9, 10, dtype=torch.bool)
    cover[0::2, 0:9:2] = True
    assert bool((mx[:, ~cover] == 0).all()) and bool((mx[:, cover] > 0).all())
    geom = GEOMS["valid_s2_uncovered"]
    _, mx, _ = magnitudes(*operands(geom, "decades", 4), geom)
    assert bool((mx[:, 9] == 0).all()) and bool((mx[:, :, 11] == 0).all()) and bool((mx[:, :9, :11] > 0).all())
    geom = GEOMS["k8_gt_input"]
    _, _, mw = magnitudes(*operands(geom, "decades", 4), geom)
    live = torch.zeros(8, 8, dtype=torch.bool)
    live[2:7] = True                            # row taps i with 0 <= ho - 4 + i < 3 for some ho < 3; every column tap meets the image
    assert bool((mw[:, :, ~live] == 0).all()) and bool((mw[:, :, live] > 0).all())


@pytest.mark.parametrize("name", list(ALL))
def test_table_geometries_pass_c2_check_and_their_rejected_variants_do_not(name):
    geom = ALL[name]
    assert geom_ok(geom)
    B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo = geom
    fits = rejected_variants(geom)["Ho one larger than fits"][10] - 1
    assert Ho <= fits and geom_ok(geom[:10] + (fits, Wo))
    for what, bad in rejected_variants(geom).items():
        assert not geom_ok(bad), what


def test_wgrad_split_plans():
    for name, geom in GEOMS.items():
        assert wgrad_plan(geom) == SPLIT_PLANS[name], name
    assert wgrad_plan(SPECTROGRAM_GEOM) == SPECTROGRAM_SPLIT_PLAN
    # what the table is there to reach: a short last chunk that is no multiple of 8, the 256-split clamp, a two-split case
    assert SPLIT_PLANS["split_tail"][2] % 8 != 0 and SPLIT_PLANS["split_cap256"][0] < 256 < -(-9 * 95 * 80 // 256)
    assert SPLIT_PLANS["rect_k2x5_pads"][0] == 2
    # the audio encoder's widest weight gradient at B = 128 (block 1: 64 -> 64, k4 s2) stays on the split path
    assert wgrad_plan((128, 128, 70, 64, 64, 4, 4, 2, 1, 1, 64, 35))[0] > 1


def test_operands_are_seeded_and_already_rounded():
    geom = GEOMS["rect_k2x5_pads"]
    a, b = operands(geom, "decades", 5), operands(geom, "decades", 5)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(t.dtype == torch.float64 and torch.equal(t.float().double(), t) for t in a)
    x = operands(geom, "decades", 5, half=True)[0]
    assert torch.equal(x.half().double(), x)
    # six decades over the input channels, the other way over the weights' Ci axis
    sx, sw = a[0].abs().amax(dim=(0, 1, 2)), a[1].abs().amax(dim=(0, 2, 3))
    assert sx[-1] / sx[0] > 1e4 and sw[0] / sw[-1] > 1e2
    xs = operands(SPECTROGRAM_GEOM, "spectrogram", 5, half=True)[0]
    assert float(xs.min()) >= -80 and float(xs.max()) <= 0 and float(xs.mean().abs()) > float(xs.std())
