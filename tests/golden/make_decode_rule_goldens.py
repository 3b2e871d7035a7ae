#!/usr/bin/env python3
"""Writes tests/golden/decode_rule_cases.json: seeded cases of the decoding constraints (skw_decode_rules: bias, repetition penalty, no-repeat n-gram) with the outcome of the
transform as tests/decode_rules_lib.py states it in numpy — sha256 of the transformed row's bytes, hash of its -inf set, its argmax — every case checked here against
transformers' SequenceBias / SuppressTokens / RepetitionPenalty / NoRepeatNGram logits processors bit for bit.  A fixture in which the two differ on any case is not written.
No logits in the file: history, raw row and bias pairs follow from the seed and the case's spec (decode_rules_lib.make_rule_case).  Needs transformers + torch; the fixture then
travels to where the GPU tests run, where k_dec_constrain is held to it.

    python tests/golden/make_decode_rule_goldens.py [cases per vocabulary]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import decode_rules_lib as dr  # noqa: E402
import logit_rules_lib as lr  # noqa: E402
from conftest import synth_model  # noqa: E402
from oracle_lib import OracleModel  # noqa: E402

VOCABS = [(51865, 80), (51864, 80), (51866, 128)]


def check_case(sp, NV, seed, spec):
    hist, raw, rules = dr.make_rule_case(seed, sp, NV, spec)
    x = dr.transform(hist, raw, rules, sp["eot"])
    y = dr.hf_transform(hist, raw, rules, sp["eot"])
    if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
        bad = np.flatnonzero(x.view(np.uint32) != y.view(np.uint32))
        raise SystemExit("numpy and transformers differ (vocab %d, seed %d, %r) at ids %s: %s vs %s — no fixture written" % (NV, seed, spec, bad[:8], x[bad[:8]], y[bad[:8]]))
    T = dr.text_tokens(hist, sp["eot"])
    return {"seed": int(seed), "spec": spec, "n_hist": len(hist), "m": len(T), "bias_hash": dr.bias_hash(rules["bias"]), "n_changed": int(np.sum(x.view(np.uint32) != raw.view(np.uint32))),
            "sha256": dr.row_hash(x), "mask_hash": lr.mask_hash(x), "argmax": int(np.argmax(x))}


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    out = {"about": "decoding-constraint cases: decode_rules_lib.transform == transformers %s logits processors on every case, bit for bit; history, raw logits and bias pairs = "
                    "decode_rules_lib.make_rule_case(seed, special, n_vocab, spec)" % __import__("transformers").__version__, "vocabs": []}
    for vi, (NV, mels) in enumerate(VOCABS):
        om = OracleModel(synth_model("micro", vocab=NV, mels=mels))
        assert om.hp.n_vocab == NV
        sp = lr.special_ids(om)
        cases = [check_case(sp, NV, 31000 + 1000 * vi + k, dr.spec_for(k + 7 * vi)) for k in range(n_cases)]
        out["vocabs"].append({"n_vocab": NV, "n_mels": mels, "special": sp, "cases": cases})
        cover = {key: sorted({str(c["spec"][key]) for c in cases}) for key in ("theta", "N", "m_kind", "n_bias")}
        print("vocab %d: %d cases agree with transformers; %d change the row; covered %s" % (NV, len(cases), sum(c["n_changed"] > 0 for c in cases), cover))
        om.close()
    with open(os.path.join(HERE, "decode_rule_cases.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
