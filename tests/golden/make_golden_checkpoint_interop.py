#!/usr/bin/env python3
"""What the REAL reference needs to read a checkpoint (build container only; imports the reference like make_golden.py):
the state_dict layout of its PoseGenerator / ConvDiscriminator built from the g7 checkpoint's own args and vocabularies (key, shape,
dtype, in order: what load_state_dict(strict=True) checks), and the attributes of its pickled Vocab objects (what its Vocab methods
read) -> golden_checkpoint_interop.json.  tests/test_checkpoint_cpu.py::test_reference_reads_our_checkpoint holds a checkpoint
written by this package against it.

    python tests/golden/make_golden_checkpoint_interop.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def spec(sd):
    return [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]


def main():
    _, mcn, vocab, _, _ = MG.import_reference()
    c = torch.load(os.path.join(HERE, "g7_reference_checkpoint.bin"), map_location="cpu", weights_only=False)
    assert type(c["lang_model"]) is vocab.Vocab and type(c["speaker_model"]) is vocab.Vocab
    a = c["args"]
    G = mcn.PoseGenerator(a, pose_dim=c["pose_dim"], n_words=c["lang_model"].n_words, word_embed_size=a.wordembed_dim,
                          word_embeddings=c["lang_model"].word_embedding_weights, z_obj=c["speaker_model"])
    D = mcn.ConvDiscriminator(c["pose_dim"])
    G.load_state_dict(c["gen_dict"], strict=True)
    D.load_state_dict(c["dis_dict"], strict=True)
    out = {"vocab_module": vocab.Vocab.__module__, "vocab_class": vocab.Vocab.__name__,
           "lang_attrs": sorted(vars(c["lang_model"])), "speaker_attrs": sorted(vars(c["speaker_model"])),
           "word_embedding_shape": list(c["lang_model"].word_embedding_weights.shape), "wordembed_dim": a.wordembed_dim,
           "args": sorted(vars(a)), "gen": spec(G.state_dict()), "dis": spec(D.state_dict())}
    with open(os.path.join(HERE, "golden_checkpoint_interop.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("gen", len(out["gen"]), "dis", len(out["dis"]), "vocab attrs", out["lang_attrs"])


if __name__ == "__main__":
    main()
