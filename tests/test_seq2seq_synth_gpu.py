"""Seq2Seq synthesis on the GPU: the one-launch eval decoder (csrc/seq2seq_decode.hip) against the fp64 chain of tests/seq2seq_synth_ref.py,
Seq2SeqNet in eval mode with the kernel on and off, generate_gestures / generate_gestures_batch, evaluate_testset and checkpoint loading
against the real reference (fixture g20).

Gates: the test runs the same chain in fp32 on the CPU, measures its error against fp64 and allows 4 x that, floored
at 1e-6 of the tensor's largest magnitude.  No gate is derived from the HIP result.  Every comparison prints its fraction of the gate."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import seq2seq_ref as R
import seq2seq_synth_ref as SR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
NAN = float("nan")
H_FIX, N_POSES, N_PRE = 12, 34, 4


def gate_of(ref64, ref32):
    e32 = float((ref32.double() - ref64).abs().max())
    return max(4.0 * e32, 1e-6 * float(ref64.abs().max()))


def check(name, got, ref64, ref32):
    g = gate_of(ref64, ref32)
    got = torch.as_tensor(got).detach().double().cpu()
    assert torch.isfinite(got).all(), name
    err = float((got - ref64).abs().max())
    print(f"{name}: error {err:.3e} gate {g:.3e} fraction {err / g:.3f}")
    assert err <= g, (name, err, g)


def check_to(name, got, target, ref64, ref32):
    """`got` against a stored result of the real reference, within the gate the chain gives (ref64 / ref32)."""
    g = gate_of(ref64, ref32)
    err = float((torch.as_tensor(got).detach().double().cpu() - torch.as_tensor(target).double()).abs().max())
    print(f"{name}: error {err:.3e} gate {g:.3e} fraction {err / g:.3f}")
    assert err <= g, (name, err, g)


# ------------------------------------------------------------------------------------------------------------------ the kernel
#        B, Te,  H, n_layers, n_frames, n_pre, Z, speaker
CASES = [(1, 1, 8, 1, 2, 1, 0, False), (2, 65, 12, 2, 6, 2, 0, False), (5, 7, 36, 4, 6, 0, 4, True), (3, 34, 200, 2, 34, 4, 0, False),
         (2, 128, 320, 4, 4, 2, 0, False)]
_cache = {}


def kernel_case(pkg, case):
    """State dict, inputs and the fp64 / fp32 chain results of one case, computed once (null and ragged lengths) and left unchanged."""
    if case in _cache:
        return _cache[case]
    B, Te, H, nl, nf, n_pre, Z, speaker = case
    torch.manual_seed(1000 + H + Te)
    args = SimpleNamespace(hidden_size=H, n_layers=nl, dropout_prob=0.0, n_pre_poses=n_pre, GAN_noise_size=Z)
    net = pkg.Seq2SeqNet(args, 27, nf, 12, 4, None, speaker_model=SimpleNamespace(n_words=5) if speaker else None)
    bn = net.decoder.decoder.pre_linear[1]
    with torch.no_grad():
        bn.running_mean.copy_(0.3 * torch.randn(H)); bn.running_var.copy_(0.5 + torch.rand(H))
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(7 + B + Te)
    enc, h0 = torch.randn(B, Te, H, generator=g), torch.randn(nl, B, H, generator=g)
    poses = torch.randn(B, max(n_pre, 1), 27, generator=g)
    z = torch.randn(B, Z, generator=g) if Z else None
    vid = torch.randint(0, 5, (B,), generator=g) if speaker else None
    ragged = [int(v) for v in torch.randint(1, Te + 1, (B,), generator=g)]
    ragged[0], ragged[-1] = 1, Te                                         # a row of length 1 and a full row (B = 1: Te = 1 is both)
    refs = {}
    for tag, lens in (("null", None), ("ragged", ragged)):
        for dt in (torch.float64, torch.float32):
            refs[tag, dt] = SR.decode(R.RefSeq2Seq(state, nl, nf, n_pre, dt), enc, h0, poses, nf, n_pre, lens, z, vid)
    _cache[case] = (net, state, enc, h0, poses, z, vid, ragged, refs)
    return _cache[case]


def run_kernel(pkg, dev, net, enc, h0, poses, nf, n_pre, lens, z, vid, rows=None):
    """ops.seq2seq_decode_eval on the module's parameters; outputs / h_n / weights sit between NaN guard rows."""
    dec = net.decoder.decoder
    if rows is not None:
        enc, h0, poses = enc[rows], h0[:, rows], poses[rows]
        z, vid, lens = None if z is None else z[rows], None if vid is None else vid[rows], None if lens is None else [lens[r] for r in rows]
    B, Te, H = enc.shape
    P = {k: v.detach().to(dev) for k, v in dec.state_dict().items()}
    encd = enc.to(dev).contiguous()
    keys = (encd.double() @ P["attn.attn.weight"][:, H:].double().t() + P["attn.attn.bias"].double()).float().contiguous()
    gru = [tuple(P[f"gru.{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(dec.n_layers)]
    spk = None if vid is None else P["speaker_embedding.weight"][vid.to(dev)].contiguous()
    out = torch.full((B + 2, nf, 27), NAN, device=dev)
    hn = torch.full((dec.n_layers, B + 2, H), NAN, device=dev)
    hn_in = torch.empty(dec.n_layers, B, H, device=dev)
    wat = torch.full((nf - 1, B, Te + 0), NAN, device=dev)
    pkg.ops.seq2seq_decode_eval(encd, keys, h0.to(dev).contiguous(), poses.to(dev).contiguous(), nf, n_pre, P["attn.attn.weight"], P["attn.v"],
                                P["pre_linear.0.weight"], P["pre_linear.0.bias"], P["pre_linear.1.weight"], P["pre_linear.1.bias"],
                                P["pre_linear.1.running_mean"], P["pre_linear.1.running_var"], 1e-5, gru, P["out.weight"], P["out.bias"],
                                out[1:B + 1], hn_in, wat, te_len=lens, z=None if z is None else z.to(dev).contiguous(), spk=spk)
    torch.cuda.synchronize()
    assert torch.isnan(out[0]).all() and torch.isnan(out[B + 1]).all()
    return out[1:B + 1].clone(), hn_in, wat, keys


@pytest.mark.parametrize("mode", ["null", "ragged"])
@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}_Te{c[1]}_H{c[2]}_L{c[3]}" for c in CASES])
def test_kernel_matches_the_fp64_chain(pkg, dev, case, mode):
    B, Te, H, nl, nf, n_pre, Z, speaker = case
    net, state, enc, h0, poses, z, vid, ragged, refs = kernel_case(pkg, case)
    lens = None if mode == "null" else ragged
    # the chain forms keys in its own dtype; the kernel's keys come from the fp64 product rounded once to fp32 (the product itself is gemm_nt's)
    out, hn, wat, _ = run_kernel(pkg, dev, net, enc, h0, poses, nf, n_pre, lens, z, vid)
    r64, r32 = refs[mode, torch.float64], refs[mode, torch.float32]
    check(f"outputs {case} {mode}", out, r64[0], r32[0])
    check(f"h_n {case} {mode}", hn, r64[1], r32[1])
    check(f"weights {case} {mode}", wat, r64[2], r32[2])
    assert torch.equal(out[:, 0].cpu(), poses[:, 0])                                      # frame 0 is seed pose 0
    assert float((wat.double().sum(2) - 1.0).abs().max()) <= 4 * 2.0 ** -23                # every row sums to 1 within a few ulps
    if lens is not None:
        for b, n in enumerate(lens):
            assert float(wat[:, b, n:].abs().max() if n < Te else 0.0) == 0.0               # exact zeros past the row's length
            assert float(wat[:, b, :n].min()) > 0.0


def test_rows_do_not_depend_on_the_batch_and_runs_are_bit_identical(pkg, dev):
    case = CASES[2]                                                                       # B = 5
    B, Te, H, nl, nf, n_pre, Z, speaker = case
    net, state, enc, h0, poses, z, vid, ragged, _ = kernel_case(pkg, case)
    for lens in (None, ragged):
        a = run_kernel(pkg, dev, net, enc, h0, poses, nf, n_pre, lens, z, vid)
        b = run_kernel(pkg, dev, net, enc, h0, poses, nf, n_pre, lens, z, vid)
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)
        for r in range(B):
            one = run_kernel(pkg, dev, net, enc, h0, poses, nf, n_pre, lens, z, vid, rows=[r])
            assert torch.equal(one[3][0], a[3][r])                                          # the same keys row went in
            assert torch.equal(one[0][0], a[0][r]) and torch.equal(one[1][:, 0], a[1][:, r]) and torch.equal(one[2][:, 0], a[2][:, r])


@pytest.mark.parametrize("dims", [dict(H=6), dict(Te=129), dict(nl=5)], ids=["H6", "Te129", "layers5"])
def test_shapes_outside_the_envelope_raise_and_launch_nothing(pkg, dev, dims):
    d = dict(B=2, Te=5, H=8, nl=1)
    d.update(dims)
    B, Te, H, nl = d["B"], d["Te"], d["H"], d["nl"]
    assert not pkg.ops.seq2seq_decode_supported(B, Te, H, nl, 3, 1, 27, 27)
    t = lambda *s: torch.zeros(*s, device=dev)
    out = torch.full((B, 3, 27), NAN, device=dev)
    with pytest.raises(ValueError, match="envelope"):
        pkg.ops.seq2seq_decode_eval(t(B, Te, H), t(B, Te, H), t(nl, B, H), t(B, 1, 27), 3, 1, t(H, 2 * H), t(H), t(H, 27 + H), t(H), t(H), t(H), t(H),
                                    t(H), 1e-5, [(t(3 * H, H), t(3 * H, H), t(3 * H), t(3 * H))] * nl, t(27, H), t(27), out, t(nl, B, H))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    with pytest.raises(ValueError, match="lengths"):                                      # a length outside [1, Te] never reaches the device
        pkg.ops.seq2seq_decode_eval(t(2, 5, 8), t(2, 5, 8), t(1, 2, 8), t(2, 1, 27), 3, 1, t(8, 16), t(8), t(8, 35), t(8), t(8), t(8), t(8), t(8), 1e-5,
                                    [(t(24, 8), t(24, 8), t(24), t(24))], t(27, 8), t(27), torch.full((2, 3, 27), NAN, device=dev), t(1, 2, 8), te_len=[0, 6])


# ------------------------------------------------------------------------------------------------------------------ modules and fixture
@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "g20_seq2seq_synth.npz"))
    return {k: z[k] for k in z.files}


def sub(c, prefix):
    return {k[len(prefix):]: v for k, v in c.items() if k.startswith(prefix)}


def fixture_args(fx):
    return SimpleNamespace(model="seq2seq", hidden_size=H_FIX, n_layers=2, dropout_prob=0.0, n_pre_poses=N_PRE, n_poses=N_POSES, GAN_noise_size=0,
                           z_type="none", motion_resampling_framerate=15, wordembed_dim=10, mean_dir_vec=fx["mean_dir_vec"].tolist())


def fixture_lang(pkg, fx):
    lang = pkg.Vocab("words")
    for w in fx["vocab_words"].tolist():
        lang.index_word(w)
    return lang


def fixture_net(pkg, dev, fx):
    lang = fixture_lang(pkg, fx)
    net = pkg.Seq2SeqNet(fixture_args(fx), 27, N_POSES, lang.n_words, 10, None)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sub(fx, "state/").items()}, strict=True)
    return net.to(dev).eval(), lang


def words_of(fx, name):
    return [[w, float(t[0]), float(t[1])] for w, t in zip(fx[name + "/words"].tolist(), fx[name + "/word_times"])]


def test_module_eval_fused_against_per_step_and_the_reference(pkg, dev, fx, monkeypatch):
    net, _ = fixture_net(pkg, dev, fx)
    state = sub(fx, "state/")
    text, lens, poses = torch.as_tensor(fx["eval/text0"]), fx["eval/lengths0"].tolist(), torch.as_tensor(fx["eval/target0"])
    r64 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE), text, lens, poses, per_row=False)
    r32 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE, torch.float32), text, lens, poses, per_row=False)
    fused = net(text.to(dev), lens, poses.to(dev), None)
    monkeypatch.setattr(pkg.seq2seq, "FUSED_EVAL_DECODE", False)
    steps = net(text.to(dev), lens, poses.to(dev), None)
    with pytest.raises(ValueError):                                                       # the per-step path has no row lengths
        net.synthesize(text.to(dev), lens, poses[:, :N_PRE].to(dev))
    monkeypatch.setattr(pkg.seq2seq, "FUSED_EVAL_DECODE", True)
    check("fused eval forward", fused, r64, r32)
    check("per-step eval forward", steps, r64, r32)
    assert float((fused - steps).detach().abs().max()) <= gate_of(r64, r32)
    check_to("fused against the reference's eval outputs", fused, fx["ckpt/eval_outputs"], r64, r32)
    # per-row lengths: every row equals its own B = 1 run
    syn = net.synthesize(text.to(dev), lens, poses[:, :N_PRE].to(dev))
    p64 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE), text, lens, poses, per_row=True)
    p32 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE, torch.float32), text, lens, poses, per_row=True)
    check("synthesize, per-row lengths", syn, p64, p32)
    for b, n in enumerate(lens):
        one = net.synthesize(text[b:b + 1, :n].to(dev), [n], poses[b:b + 1, :N_PRE].to(dev))
        assert float((one[0] - syn[b]).abs().max()) <= gate_of(p64[b], p32[b])
    assert not net.training and int(net.decoder.decoder.pre_linear[1].num_batches_tracked) == 7


def _ref_final(pkg, fx, name, dtype, lang):
    args = fixture_args(fx)
    ref = R.RefSeq2Seq(sub(fx, "state/"), 2, N_POSES, N_PRE, dtype)
    seed = fx[name + "/seed_seq"]
    stacked, wins = SR.generate_gestures(ref, int(fx[name + "/audio_len"]), words_of(fx, name), lang.get_word_index,
                                         seed_seq=seed if len(seed) else None)
    out = pkg.synthesize.seq2seq_smooth(stacked.astype(np.float64), len(wins), N_POSES, N_PRE)
    if bool(fx[name + "/fade_out"]):
        out = pkg.synthesize.fade_out_to_mean(out, pkg.synthesize.end_padding_samples(args, int(fx[name + "/audio_len"])), args)
    return torch.as_tensor(out)


def test_generate_gestures_single_and_batched_against_the_chain_and_the_reference(pkg, dev, fx):
    net, lang = fixture_net(pkg, dev, fx)
    args = fixture_args(fx)
    names = fx["cases"].tolist()
    singles, r64s, r32s = {}, {}, {}
    for name in names:
        seed = fx[name + "/seed_seq"]
        audio = np.zeros(int(fx[name + "/audio_len"]), np.float32)
        out = pkg.synthesize.generate_gestures(args, net, lang, audio, words_of(fx, name), seed_seq=seed if len(seed) else None,
                                               fade_out=bool(fx[name + "/fade_out"]))
        r64s[name], r32s[name] = _ref_final(pkg, fx, name, torch.float64, lang), _ref_final(pkg, fx, name, torch.float32, lang)
        assert out.shape == fx[name + "/final"].shape
        check(f"generate_gestures {name} against the chain", out, r64s[name], r32s[name])
        check_to(f"generate_gestures {name} against the reference", out, fx[name + "/final"], r64s[name], r32s[name])
        singles[name] = out
    # all utterances in lock-step (no fade-out in the batch API): unseeded ones get zero seeds, as a single run without seed does
    audios = [np.zeros(int(fx[n + "/audio_len"]), np.float32) for n in names]
    seeds = [fx[n + "/seed_seq"] if len(fx[n + "/seed_seq"]) else np.zeros((N_PRE, 27), np.float32) for n in names]
    outs = pkg.synthesize.generate_gestures_batch(args, net, lang, audios, [words_of(fx, n) for n in names], seed_seqs=seeds)
    for name, o in zip(names, outs):
        if bool(fx[name + "/fade_out"]):
            o = pkg.synthesize.fade_out_to_mean(o, pkg.synthesize.end_padding_samples(args, int(fx[name + "/audio_len"])), args)
        assert o.shape == singles[name].shape
        err, g = float(np.abs(o - singles[name]).max()), gate_of(r64s[name], r32s[name])
        print(f"batched {name}: differs from its single run by {err:.3e}, gate {g:.3e}")
        assert err <= g


def test_evaluate_testset_against_the_reference(pkg, dev, fx):
    net, _ = fixture_net(pkg, dev, fx)
    args = fixture_args(fx)
    loader = []
    for i in range(2):
        text, lens, target = torch.as_tensor(fx[f"eval/text{i}"]), torch.as_tensor(fx[f"eval/lengths{i}"]), torch.as_tensor(fx[f"eval/target{i}"])
        loader.append((text, lens, torch.zeros(3, N_POSES, dtype=torch.int64), torch.zeros(3, N_POSES, 30), target, torch.zeros(3, 8), torch.zeros(3, 1), {}))
    ret = pkg.eval_metrics.evaluate_testset(loader, net, torch.nn.L1Loss(), None, args)
    assert net.training and set(ret) == {"loss", "joint_mae"}
    # The metrics are means of |differences|: a mean moves by at most the largest change of an element.  Outputs move by at most their gate g;
    # a joint position is a chain of at most 4 bones of length <= 0.36 (1.5 g), a second difference of positions 4 x that (6 g).  The stored
    # values are fp32 means of the reference (2^-22 of the value).
    state, g = sub(fx, "state/"), 0.0
    for i in range(2):
        text, lens, target = torch.as_tensor(fx[f"eval/text{i}"]), fx[f"eval/lengths{i}"].tolist(), torch.as_tensor(fx[f"eval/target{i}"])
        r64 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE), text, lens, target, per_row=False)
        r32 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE, torch.float32), text, lens, target, per_row=False)
        g = max(g, gate_of(r64, r32))
    for k, got in (("loss", ret["loss"]), ("joint_mae", ret["joint_mae"]), ("accel", ret.accel)):
        want = float(fx["eval/" + k])
        bound = 6.0 * g + 2.0 ** -22 * abs(want)
        print(f"evaluate_testset {k}: {got:.9f} reference {want:.9f} difference {abs(got - want):.3e} bound {bound:.3e}")
        assert abs(got - want) <= bound


def test_load_checkpoint_and_model_reads_the_reference_checkpoint(pkg, dev, fx):
    args, gen, loss_fn, lang, spk, pose_dim = pkg.checkpoint.load_checkpoint_and_model(os.path.join(GOLDEN, "g20_seq2seq_checkpoint.bin"), dev)
    assert isinstance(gen, pkg.Seq2SeqNet) and not gen.training and isinstance(loss_fn, torch.nn.L1Loss) and pose_dim == 27 and spk is None
    assert args.model == "seq2seq" and lang.n_words == 4 + len(fx["vocab_words"])
    state = sub(fx, "state/")
    for k, v in gen.state_dict().items():
        assert torch.equal(v.cpu(), torch.as_tensor(state[k])), k
    text, lens, poses = torch.as_tensor(fx["eval/text0"]), fx["eval/lengths0"].tolist(), torch.as_tensor(fx["eval/target0"])
    r64 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE), text, lens, poses, per_row=False)
    r32 = SR.forward(R.RefSeq2Seq(state, 2, N_POSES, N_PRE, torch.float32), text, lens, poses, per_row=False)
    with torch.no_grad():
        out = gen(text.to(dev), lens, poses.to(dev), None)
    check_to("checkpoint eval outputs", out, fx["ckpt/eval_outputs"], r64, r32)
