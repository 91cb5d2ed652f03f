"""Checkpoint interop (utils/train_utils.py:147-183): a checkpoint written by the REAL reference
(tests/golden/g7_reference_checkpoint.bin, made by make_golden_variants.py) loads into the HIP-backed modules with
strict=True, and a checkpoint written here loads back -- and holds what the reference's own loading code reads."""
import json
import os
import subprocess
import sys

import torch

from conftest import GOLDEN, ROOT


def _ckpt(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".checkpoint")


def test_reference_checkpoint_loads_strict(pkg):
    ck = _ckpt(pkg)
    rep = json.load(open(os.path.join(GOLDEN, "golden_report_variants.json")))["checkpoint"]
    path = os.path.join(GOLDEN, "g7_reference_checkpoint.bin")
    raw = ck.load_checkpoint(path)
    assert sorted(raw) == ["args", "dis_dict", "epoch", "gen_dict", "lang_model", "pose_dim", "speaker_model"]
    assert isinstance(raw["lang_model"], pkg.Vocab) and isinstance(raw["speaker_model"], pkg.Vocab)   # model.vocab.Vocab mapped
    assert raw["lang_model"].n_words == rep["n_words"] and raw["speaker_model"].n_words == rep["n_speakers"]
    assert raw["lang_model"].get_word_index("fox") == raw["lang_model"].word2index["fox"] > 3
    assert raw["lang_model"].get_word_index("unseen") == pkg.Vocab.UNK_token
    args, gen, loss_fn, lang, spk, pose_dim = ck.load_checkpoint_and_model(path, "cpu")
    assert isinstance(gen, pkg.PoseGenerator) and not gen.training and pose_dim == 27 and loss_fn is None
    sd = gen.state_dict()
    assert len(sd) == rep["gen_keys"] and list(sd) == list(raw["gen_dict"])           # same keys, same order
    total = float(sum(v.double().abs().sum() for v in sd.values() if v.is_floating_point()))
    assert abs(total - rep["gen_abs_sum"]) < 1e-9 * rep["gen_abs_sum"]
    # the embedding came from lang_model.word_embedding_weights at construction and was then overwritten by gen_dict
    assert torch.equal(sd["text_encoder.embedding.weight"], raw["gen_dict"]["text_encoder.embedding.weight"])
    dis = pkg.ConvDiscriminator(27)
    dis.load_state_dict(raw["dis_dict"], strict=True)
    assert len(dis.state_dict()) == rep["dis_keys"]


def test_checkpoint_round_trip(pkg, tmp_path):
    ck = _ckpt(pkg)
    raw = ck.load_checkpoint(os.path.join(GOLDEN, "g7_reference_checkpoint.bin"))
    gen, dis, _ = ck.init_model(raw["args"], raw["lang_model"], raw["speaker_model"], raw["pose_dim"], "cpu")
    gen.load_state_dict(raw["gen_dict"]); dis.load_state_dict(raw["dis_dict"])
    out = str(tmp_path / "ours.bin")
    ck.save_checkpoint({"args": raw["args"], "epoch": 8, "lang_model": raw["lang_model"], "speaker_model": raw["speaker_model"],
                        "pose_dim": 27, "gen_dict": gen.state_dict(), "dis_dict": dis.state_dict()}, out)
    assert "model.vocab" not in sys.modules and pkg.Vocab.__module__.endswith(".vocab") and "model" != pkg.Vocab.__module__.split(".")[0]
    back = ck.load_checkpoint(out)
    assert back["epoch"] == 8 and isinstance(back["lang_model"], pkg.Vocab)
    assert back["lang_model"].word2index == raw["lang_model"].word2index
    for k, v in raw["gen_dict"].items():
        assert torch.equal(back["gen_dict"][k], v), k


def test_reference_reads_our_checkpoint(pkg, tmp_path):
    """A checkpoint saved by this package unpickles in a process that knows nothing but the reference's module path `model.vocab.Vocab`
    (a bare class: unpickling sets its attributes) and holds exactly what the reference's loading code reads: its Vocab attributes, and
    state dicts with the key / shape / dtype layout of the reference's PoseGenerator / ConvDiscriminator built from the checkpoint's own
    args (what load_state_dict(strict=True) checks).  That layout was recorded from the reference itself (tests/golden/
    make_golden_checkpoint_interop.py).  Separate process: neither this package nor its Vocab may be imported to read the file."""
    ck = _ckpt(pkg)
    ref = json.load(open(os.path.join(GOLDEN, "golden_checkpoint_interop.json")))
    raw = ck.load_checkpoint(os.path.join(GOLDEN, "g7_reference_checkpoint.bin"))
    gen, dis, _ = ck.init_model(raw["args"], raw["lang_model"], raw["speaker_model"], raw["pose_dim"], "cpu")
    gen.load_state_dict(raw["gen_dict"]); dis.load_state_dict(raw["dis_dict"])
    out = str(tmp_path / "ours.bin")
    ck.save_checkpoint({"args": raw["args"], "epoch": 9, "lang_model": raw["lang_model"], "speaker_model": raw["speaker_model"],
                        "pose_dim": 27, "gen_dict": gen.state_dict(), "dis_dict": dis.state_dict()}, out)
    code = f"""
import json, sys, types
sys.dont_write_bytecode = True
mod = types.ModuleType({ref["vocab_module"]!r})
Vocab = type({ref["vocab_class"]!r}, (), {{"__module__": {ref["vocab_module"]!r}}})
setattr(mod, {ref["vocab_class"]!r}, Vocab)
top = types.ModuleType({ref["vocab_module"]!r}.split(".")[0])
setattr(top, {ref["vocab_module"]!r}.split(".")[1], mod)
sys.modules[top.__name__], sys.modules[mod.__name__] = top, mod
import torch
c = torch.load({out!r}, map_location="cpu", weights_only=False)
assert type(c["lang_model"]) is Vocab and type(c["speaker_model"]) is Vocab, type(c["lang_model"])
assert not [m for m in sys.modules if "trimodal" in m], sorted(m for m in sys.modules if "trimodal" in m)
spec = lambda sd: [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]
a = c["args"]
print(json.dumps({{"epoch": c["epoch"], "pose_dim": c["pose_dim"], "args_type": type(a).__module__ + "." + type(a).__name__,
                  "args": sorted(vars(a)), "wordembed_dim": a.wordembed_dim,
                  "lang_attrs": sorted(vars(c["lang_model"])), "speaker_attrs": sorted(vars(c["speaker_model"])),
                  "word_embedding_shape": list(c["lang_model"].word_embedding_weights.shape),
                  "gen": spec(c["gen_dict"]), "dis": spec(c["dis_dict"])}}))
"""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["epoch"] == 9 and got["pose_dim"] == 27 and got["args_type"] == "argparse.Namespace"
    for k in ("args", "wordembed_dim", "lang_attrs", "speaker_attrs", "word_embedding_shape"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("gen", "dis"):          # strict=True: the same keys with the same shapes (order kept as well)
        assert len(got[k]) == len(ref[k]) and got[k] == ref[k], (k, [e for e in got[k] if e not in ref[k]], [e for e in ref[k] if e not in got[k]])
