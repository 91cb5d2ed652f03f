#!/usr/bin/env python3
"""Golden values of the Frechet gesture distance (build container only): the exact oracle of tests/fgd_ref.py and the REAL reference's numbers.

For every case of tests/fgd_ref.py (seeded fp32 features) this records
  - the oracle: the symmetric formulation evaluated with mpmath at 60 digits from the fp32 rows (score, traces, ||d||^2, sum sqrt l, eigenvalues l);
  - the reference: /root/reference/scripts/model/embedding_space_evaluator.py, its own EmbeddingSpaceEvaluator.get_scores (the feature lists filled
    with the same rows; no network is involved in what get_scores does) and its calculate_frechet_distance on np.mean / np.cov of the rows,
    with the fp32 means it used.
Writes g17_fgd.npz and golden_report_fgd.json next to this file.  The fixture holds numbers only; the features themselves are regenerated from
their seeds by tests/fgd_ref.features (numpy keeps the legacy stream frozen) and the fixture carries their SHA-1 digests: the two largest cases alone
would be a megabyte.

Stand-ins, and why: `umap` is not installed and embedding_space_evaluator.py imports it at the top; only get_features_for_viz uses it, which is
not called here.  `fasttext` is not installed either and model/vocab.py, which the evaluator's module reaches through embedding_net.py, imports it
at the top; nothing called here touches a vocabulary.  Empty modules of those names stand in.

    python tests/golden/make_golden_fgd.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

REF = "/root/reference"


def import_reference():
    sys.path.insert(0, os.path.join(REF, "scripts"))
    for name in ("umap", "fasttext"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import model.embedding_space_evaluator as ese
    return ese


def main():
    import fgd_ref as FR
    ese = import_reference()
    warnings.filterwarnings("ignore")
    arrays, report = {}, {"cases": {}}
    for D, N, kind in FR.CASES:
        name = FR.case_name(D, N, kind)
        g, r = FR.features(D, N, kind)
        o = FR.oracle(g, r)
        ev = ese.EmbeddingSpaceEvaluator.__new__(ese.EmbeddingSpaceEvaluator)
        ev.generated_feat_list, ev.real_feat_list = [g], [r]
        ref_fd, ref_dist = ev.get_scores()
        mu_g, mu_r = np.mean(g, axis=0), np.mean(r, axis=0)
        try:
            ref_direct = float(np.real(ese.EmbeddingSpaceEvaluator.calculate_frechet_distance(mu_g, np.cov(g, rowvar=False), mu_r, np.cov(r, rowvar=False))))
        except ValueError:
            ref_direct = 1e10
        arrays[name + "/oracle"] = np.array([o["fgd"], o["tr1"], o["tr2"], o["d2"], o["sum_sqrt"]])
        arrays[name + "/lam"] = o["lam"]
        arrays[name + "/ref"] = np.array([float(np.real(ref_fd)), float(ref_dist), ref_direct])
        arrays[name + "/ref_mu_g"], arrays[name + "/ref_mu_r"] = mu_g.astype(np.float32), mu_r.astype(np.float32)
        arrays[name + "/sha1"] = np.array([FR.digest(g), FR.digest(r)])
        arrays[name + "/seed"] = np.array(FR.case_seed(D, N, kind))
        report["cases"][name] = {"oracle_fgd": o["fgd"], "reference_fgd": float(np.real(ref_fd)), "reference_feat_dist": float(ref_dist),
                                 "gate": FR.gate(D, o["lam"], o["tr1"], o["tr2"], o["d2"]), "restatement_fgd": FR.restate(g, r)[0]}
        print(name, report["cases"][name], flush=True)
    np.savez_compressed(os.path.join(HERE, "g17_fgd.npz"), **arrays)
    report["numpy"] = np.__version__
    with open(os.path.join(HERE, "golden_report_fgd.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
