"""ops.tcn_fwd_fused (csrc/tcn_fused.hip): the text encoder's eight convs and its decoder as one clip-local launch, against a torch fp64
restatement of the block chain (model/tcn.py:16-46, multimodal_context_net.py:57-61) whose dropout masks are the ones ops.dropout_mask draws
for the same state and site.  Gate: the project's forward gate, 1e-5 normalised max error.  The op is called directly (the engine's own
dispatch starts at 8 192 rows); the kernel's envelope fixes T = 34, so T = 12 is asserted to be refused."""
import argparse

import pytest
import torch

pytestmark = pytest.mark.gpu

T, C, NB, E_OUT = 34, 300, 4, 32
GATE = 1e-5
SENTINEL = 12345.0
SITE = 77


def _nerr(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def net(pkg, dev):
    """Weight-normed conv weights (packed [8][C][2 C] + fp16 x 2 planes), biases, decoder: made once, never modified."""
    ops = pkg.ops
    g = torch.Generator(device="cpu").manual_seed(1234)
    vs = [(torch.randn(C, C, 2, generator=g) * 0.05).to(dev) for _ in range(2 * NB)]
    gs = [(torch.rand(C, 1, 1, generator=g) * 0.5 + 0.75).to(dev) for _ in range(2 * NB)]
    wps, _ = ops.weight_norm_fwd_batch(vs, gs, want_t=False)
    slab = (torch.randn(2 * NB * C + E_OUT * C + E_OUT, generator=g) * 0.1).to(dev)          # biases and decoder, 16-byte aligned pieces
    biases = [slab[j * C:(j + 1) * C] for j in range(2 * NB)]
    dec_w = slab[2 * NB * C:2 * NB * C + E_OUT * C].view(E_OUT, C)
    dec_b = slab[2 * NB * C + E_OUT * C:]
    w_pl = ops.split_planes(wps.view(2 * NB * C, 2 * C))
    assert w_pl.kind == "h2"
    return dict(wps=wps, w_pl=w_pl, biases=biases, dec_w=dec_w, dec_b=dec_b, state=ops.new_rng_state(99, dev))


def _ref(net, x0, masks):
    """fp64 chain: per block two causal dilated convs (tap 0 reads row t - d, tap 1 row t), each + ReLU + dropout, then relu(out + x)."""
    cur = x0.double()
    B = cur.shape[0]
    o0s, o1s, ys = [], [], []
    for i in range(NB):
        d, h = 2 ** i, cur
        for ci in range(2):
            j = 2 * i + ci
            W = net["wps"][j].double()
            hp = torch.cat([torch.zeros(B, d, C, dtype=torch.float64, device=h.device), h[:, :T - d]], 1)
            h = torch.relu(hp @ W[:, :C].T + h @ W[:, C:].T + net["biases"][j].double())
            if masks is not None:
                h = h * masks[j].double()
            (o0s, o1s)[ci].append(h)
        cur = torch.relu(h + cur)
        ys.append(cur)
    dec = cur @ net["dec_w"].double().T + net["dec_b"].double()
    return dict(o0=torch.stack(o0s), o1=torch.stack(o1s), y=torch.stack(ys), dec=dec)


def _masks(pkg, net, clips, p):
    if p == 0.0:
        return None
    return pkg.ops.dropout_mask(torch.empty(2 * NB, clips, T, C, device=net["dec_w"].device), p, net["state"], SITE)


def _fused(pkg, net, x0, p, save_rows, width=E_OUT, col0=0):
    ops = pkg.ops
    clips = x0.shape[0]
    tape = tuple(torch.full((NB, clips, T, C), SENTINEL, device=x0.device) for _ in range(3))
    wide = torch.full((clips, T, width), SENTINEL, device=x0.device)
    ops.tcn_fwd_fused(x0, net["w_pl"], net["biases"], net["dec_w"], net["dec_b"], wide[:, :, col0:col0 + E_OUT], p=p, state=net["state"], site=SITE,
                      save_rows=save_rows, tape=tape)
    torch.cuda.synchronize()
    return dict(o0=tape[0], o1=tape[1], y=tape[2], wide=wide, dec=wide[:, :, col0:col0 + E_OUT])


def _x0(dev, clips, seed=5):
    return torch.randn(clips, T, C, generator=torch.Generator(device="cpu").manual_seed(seed)).to(dev)


@pytest.fixture(scope="module")
def case3(pkg, dev, net):
    """3 clips (odd: the second workgroup holds a lone clip; also R + 1 clips), dropout 0.3, every clip taped."""
    x0 = _x0(dev, 3)
    masks = _masks(pkg, net, 3, 0.3)
    return dict(x0=x0, masks=masks, ref=_ref(net, x0, masks), got=_fused(pkg, net, x0, 0.3, (0, 3)))


def test_three_clips_with_dropout_match_fp64(case3):
    ref, got = case3["ref"], case3["got"]
    errs = {k: _nerr(got[k], ref[k]) for k in ("o0", "o1", "y", "dec")}
    print("normalised max errors:", errs)
    assert all(e <= GATE for e in errs.values()), errs
    # the taped conv outputs are zero exactly where the drawn mask is
    m = case3["masks"].view(NB, 2, 3, T, C)
    assert (got["o0"][m[:, 0] == 0] == 0).all() and (got["o1"][m[:, 1] == 0] == 0).all()
    assert 0.2 < (case3["masks"] == 0).float().mean().item() < 0.4


def test_sub_range_tape_and_decoder_columns_without_dropout(pkg, dev, net):
    """5 clips, clips 1..2 taped, p = 0: the taped tensors match on those clips, every other clip still holds the sentinel; the decoder columns
    land in columns 7 .. 38 of a 45-wide buffer and the neighbouring columns are untouched."""
    x0 = _x0(dev, 5, seed=6)
    ref = _ref(net, x0, None)
    got = _fused(pkg, net, x0, 0.0, (1, 2), width=45, col0=7)
    for k in ("o0", "o1", "y"):
        e = _nerr(got[k][:, 1:3], ref[k][:, 1:3])
        print(k, e)
        assert e <= GATE, (k, e)
        assert (got[k][:, 0] == SENTINEL).all() and (got[k][:, 3:] == SENTINEL).all(), k
    e = _nerr(got["dec"], ref["dec"])
    print("dec", e)
    assert e <= GATE
    assert (got["wide"][:, :, :7] == SENTINEL).all() and (got["wide"][:, :, 7 + E_OUT:] == SENTINEL).all()
    # nothing taped at all: the tape pointers may be absent
    out = torch.empty(5, T, E_OUT, device=dev)
    pkg.ops.tcn_fwd_fused(x0, net["w_pl"], net["biases"], net["dec_w"], net["dec_b"], out, p=0.0, save_rows=None, tape=None)
    assert torch.equal(out, got["dec"])


def test_row_magnitudes_and_zero_clip(pkg, dev, net):
    """Rows of one clip scaled by 10^0 .. 10^-6 alternating with their neighbours: every output row within 1e-5 of its OWN largest value.
    An all-zero clip gives exactly what the biases alone give."""
    x0 = _x0(dev, 3, seed=7)
    exps = torch.tensor([(t % 7) if t % 2 else 0 for t in range(T)], dtype=torch.float32, device=dev)       # 1, 1e-1, 1, 1e-3, 1, 1e-5, ...
    x0[0] *= (10.0 ** -exps)[:, None]
    x0[2] = 0.0
    ref = _ref(net, x0, None)
    got = _fused(pkg, net, x0, 0.0, (0, 3))
    worst = 0.0
    for k in ("o0", "o1", "y"):
        err = (got[k].double() - ref[k]).abs().amax(-1) / ref[k].abs().amax(-1).clamp_min(1e-300)
        worst = max(worst, err.max().item())
    derr = ((got["dec"].double() - ref["dec"]).abs().amax(-1) / ref["dec"].abs().amax(-1)).max().item()
    print("worst per-row normalised error:", worst, "decoder:", derr)
    assert worst <= GATE and derr <= GATE
    # the first conv of an all-zero clip is relu(bias), bit for bit
    b0 = torch.relu(net["biases"][0])
    assert torch.equal(got["o0"][0, 2], b0.expand(T, C))
    # and the clip's whole chain equals the chain of a lone all-zero clip (no leakage from its workgroup neighbour)
    lone = _fused(pkg, net, torch.zeros(1, T, C, device=dev), 0.0, (0, 1))
    assert torch.equal(lone["y"][:, 0], got["y"][:, 2]) and torch.equal(lone["dec"][0], got["dec"][2])


def test_agrees_with_the_unfused_chain(pkg, dev, net, case3):
    """The conv-by-conv path on the same inputs and RNG state (its masks regenerated from the same Philox elements): 2e-6 normalised."""
    ops, L = pkg.ops, pkg.layers
    x0, clips = case3["x0"], 3
    per = clips * T * C
    cur = x0
    outs = dict(o0=[], o1=[], y=[])
    for i in range(NB):
        d, h = 2 ** i, cur
        for ci in range(2):
            j = 2 * i + ci
            m = ops.Drop(net["state"], SITE, 0.3, (clips, T, C), index0=j * per).materialize()
            h = L.conv_fwd(h, net["wps"][j], net["biases"][j], 2, pad=d, dil=d, rows_out=T, act_slope=0.0, out_scale=m)
            outs[("o0", "o1")[ci]].append(h)
        cur = ops.add_relu(h, cur, torch.empty_like(cur))
        outs["y"].append(cur)
    dec = L.linear_fwd(cur.view(clips * T, C), net["dec_w"], net["dec_b"]).view(clips, T, E_OUT)
    errs = {k: _nerr(case3["got"][k], torch.stack(outs[k])) for k in outs}
    errs["dec"] = _nerr(case3["got"]["dec"], dec)
    print("against the unfused chain:", errs)
    assert all(e <= 2e-6 for e in errs.values()), errs


def test_predicate_states_the_envelope(pkg, dev, net, monkeypatch):
    ops = pkg.ops
    x0 = _x0(dev, 2)
    takes = lambda x, **kw: ops.tcn_fused_takes(x, kw.get("w_pl", net["w_pl"]), kw.get("ksize", 2), kw.get("nb", NB), net["dec_w"], net["biases"])
    assert takes(x0)
    assert not takes(torch.zeros(2, 12, C, device=dev))                                  # the envelope fixes T = 34
    assert not takes(torch.zeros(2, T, 1024, device=dev))                                # C above what the LDS layout holds
    assert not takes(torch.zeros(2 * T * C + 1, device=dev)[1:].view(2, T, C))           # misaligned embedding
    assert not takes(x0, ksize=3) and not takes(x0, nb=3) and not takes(x0, w_pl=None)
    ops.set_math_mode("bf16")
    try:
        assert not takes(x0)
    finally:
        ops.set_math_mode("f32")
    with pytest.raises(ValueError):
        ops.tcn_fwd_fused(torch.zeros(2, 12, C, device=dev), net["w_pl"], net["biases"], net["dec_w"], net["dec_b"], torch.empty(2, 12, E_OUT, device=dev))
    # a refused forward runs the conv-by-conv path: a small engine (below the stacked-forward size) never reaches the fused op
    a = argparse.Namespace(n_pre_poses=4, n_poses=T, input_context="both", hidden_size=300, n_layers=4, dropout_prob=0.3, freeze_wordembed=False)
    gen = pkg.PoseGenerator(a, 27, 64, C, None, pkg.Vocab.speakers(3)).to(dev)
    eng = gen.engine
    monkeypatch.setattr(ops, "tcn_fwd_fused", lambda *a_, **k_: (_ for _ in ()).throw(AssertionError("fused path taken")))
    P, _, _ = eng.views()
    in_data = torch.zeros(4, T, eng.in_size, device=dev)
    tp = {}
    eng._text_fwd(P, torch.randint(0, 64, (4, T), device=dev), in_data, tp, True, None, "g")
    torch.cuda.synchronize()
    assert len(tp["tcn"]) == NB and tp["text_x"].shape == (4, T, C)
    assert in_data[:, :, eng.c_text:eng.c_text + 32].abs().sum().item() > 0 and torch.isfinite(in_data).all()
