"""Decoding constraints per clip (skw_decode_rules), the parts that need no GPU: the numpy transform against the transformers-checked fixture, the end-to-end checker
(tests/decode_rules_lib.py) against the oracle's own whisper_full, the binding's validation and struct, the node's parameter parsing, and the conditions under which the GPU
tests of tests/test_gpu_decode_rules.py show anything (asserted here on the checker alone, so that a GPU pass cannot be vacuous)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import context_ref_lib as cr
import decode_rules_lib as dr
import logit_rules_lib as lr
from conftest import ROOT

from decode_rules_lib import LOOP_IDS, RULE_SETS, fixture

_CACHE = {}


def checker(om, clip, name):
    """the checker's result for synth.clip(clip, 160000) under RULE_SETS[name] on the micro model: computed once, shared, never modified"""
    from streamkit_amd import synth
    if (clip, name) not in _CACHE:
        _CACHE[(clip, name)] = dr.full_with_rules(om, synth.clip(clip, 160000), (), cr.params_for(om), RULE_SETS[name])
    return _CACHE[(clip, name)]


# ---- (a) the transform in numpy is the fixture's (which transformers' processors agreed with, case by case)
def test_numpy_transform_equals_the_fixture():
    fx = fixture()
    n, seen = 0, dict(m=set(), N=set(), theta=set(), n_bias=set(), neg_inf_bias=0, zero=0, both_signs=0)
    assert [v["n_vocab"] for v in fx["vocabs"]] == [51865, 51864, 51866]
    for v in fx["vocabs"]:
        sp, NV = v["special"], v["n_vocab"]
        for c in v["cases"]:
            hist, raw, rules = dr.make_rule_case(c["seed"], sp, NV, c["spec"])
            assert len(hist) == c["n_hist"] and dr.bias_hash(rules["bias"]) == c["bias_hash"]
            x = dr.transform(hist, raw, rules, sp["eot"])
            assert dr.row_hash(x) == c["sha256"] and lr.mask_hash(x) == c["mask_hash"] and int(np.argmax(x)) == c["argmax"], (NV, c["seed"])
            T = dr.text_tokens(hist, sp["eot"])
            assert len(T) == c["m"]
            seen["m"].add(c["spec"]["m_kind"]); seen["N"].add(rules["N"]); seen["theta"].add(rules["theta"]); seen["n_bias"].add(len(rules["bias"]))
            seen["neg_inf_bias"] += any(np.isneginf(b) for _, b in rules["bias"])
            seen["zero"] += any(raw[t] == 0.0 for t in T); seen["both_signs"] += any(raw[t] < 0 for t in T) and any(raw[t] > 0 for t in T)
            n += 1
    assert n >= 300
    assert seen["m"] == set(dr.M_KINDS) and seen["N"] >= {0, 1, 2, 3, 5, 1000} and seen["theta"] >= {0.5, 1.0, 1.3, 4.0} and seen["n_bias"] >= {0, 1, 256}
    assert seen["neg_inf_bias"] > 20 and seen["zero"] > 20 and seen["both_signs"] > 20


def test_transform_on_hand_made_rows():
    """the contract's sentences one by one, on rows small enough to read"""
    eot = 100
    raw = np.array([2.0, -2.0, 0.0, -np.inf, 6.0, 1.0, 1.0, 1.0], np.float32)
    R = lambda **kw: dict(dict(theta=1.0, N=0, bias=[]), **kw)
    # a token seen three times is penalised once; negative values are multiplied, positive ones divided; 0 and -inf stay; timestamps / <|endoftext|> (>= eot) are not in T
    x = dr.transform([0, 0, 0, 1, 2, 3, 150, 100], raw, R(theta=2.0), eot)
    assert x.tolist()[:5] == [1.0, -4.0, 0.0, -np.inf, 6.0]
    # the penalty reads what the bias left: (2 + 2) / 2, not 2 / 2 + 2
    assert dr.transform([0], raw, R(theta=2.0, bias=[(0, 2.0)]), eot)[0] == 2.0
    # N = 1 bans every text token produced; N > m bans nothing; m == N - 1 bans nothing
    assert np.flatnonzero(np.isneginf(dr.transform([4, 150, 5], raw, R(N=1), eot))).tolist() == [3, 4, 5]
    assert np.array_equal(dr.transform([4, 5], raw, R(N=3), eot), raw)
    # the bigram (4, 5) was produced; after ... 4 the token 5 would repeat it — also when a timestamp pair stood between 4 and 5, and the ban ignores a bias on 5
    assert np.isneginf(dr.transform([4, 151, 151, 5, 6, 4], raw, R(N=2, bias=[(5, 30.0)]), eot)[5])
    assert np.array_equal(dr.transform([4, 5, 6, 7], raw, R(N=2), eot), raw)                    # no bigram starts with 7 yet
    # N = 3: (4, 5) -> 6 banned only behind the same two tokens
    assert np.isneginf(dr.transform([4, 5, 6, 4, 5], raw, R(N=3), eot)[6]) and not np.isneginf(dr.transform([4, 5, 6, 7, 5], raw, R(N=3), eot)[6])
    # None and the default record change nothing
    assert np.array_equal(dr.transform([4, 5, 4], raw, None, eot), raw) and np.array_equal(dr.transform([4, 5, 4], raw, dr.DEFAULT, eot), raw)


# ---- (b) the end-to-end checker with default rules is the oracle's whisper_full
@pytest.mark.parametrize("clip", [0, 3])
def test_checker_equals_oracle_full_with_default_rules(oracle_micro, clip):
    from streamkit_amd import synth
    om = oracle_micro
    ref = om.full(synth.clip(clip, 160000), cr.params_for(om))
    got = checker(om, clip, "plain")
    assert ref["fallback_requested"] == 0 and got["failed_passes"] == 0
    assert cr.token_bits(got["tokens"]) == cr.token_bits(ref["tokens"])
    assert [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in got["segments"]] == [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in ref["segments"]]
    dflt = dr.full_with_rules(om, synth.clip(clip, 160000), (), cr.params_for(om), dr.DEFAULT)
    assert cr.token_bits(dflt["tokens"]) == cr.token_bits(ref["tokens"]) and dflt["context"] == got["context"]
    assert tuple(t[0] for t in ref["tokens"] if t[0] < lr.special_ids(om)["eot"])[:3] == LOOP_IDS


# ---- (c) what makes the GPU end-to-end tests show something, on the checker alone
@pytest.mark.parametrize("clip", [0, 3])
def test_rule_sets_change_the_transcript_as_the_gpu_tests_assume(oracle_micro, clip):
    om = oracle_micro
    eot = lr.special_ids(om)["eot"]
    ids = {name: [t[0] for t in checker(om, clip, name)["tokens"]] for name in RULE_SETS}
    assert all(checker(om, clip, name)["failed_passes"] == 0 for name in RULE_SETS)              # no pass fails
    assert dr.repeats(ids["plain"], eot) <= 1
    assert dr.repeats(ids["bias"], eot) >= 20                                                     # the bias alone makes the model loop (seen: 28 of 31 text tokens)
    assert ids["bias_t"] != ids["bias"] and dr.repeats(ids["bias_t"], eot) < dr.repeats(ids["bias"], eot)       # (seen: 25 and 23)
    assert ids["bias_n2"] != ids["bias"] and dr.repeats(ids["bias_n2"], eot) < dr.repeats(ids["bias"], eot)     # (seen: 17)
    assert dr.repeated_bigrams(ids["bias"], eot) > 0 and dr.repeated_bigrams(ids["bias_n2"], eot) == 0
    assert all(ids["bias_t_n3"] != ids[k] for k in ("plain", "bias", "bias_t", "bias_n2"))


# ---- (d) the binding: validation without a device, and the struct
def test_binding_refuses_bad_records_naming_the_clip(built):
    from streamkit_amd import engine
    NV = 51865
    ok = engine.DecodeRules(repetition_penalty=1.1, no_repeat_ngram_size=3, bias={5: 1.5}, suppress=[7, 8])
    assert ok.n_bias == 3 and list(ok.bias_id[:3]) == [5, 7, 8] and ok.bias[0] == 1.5 and ok.bias[1] == float("-inf") and not ok.is_default()
    engine.rules_array([None, ok, engine.DecodeRules()], 3, NV, "clip")
    bad = [(dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
           (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(bias={NV: 1.0}), "token id"),
           (dict(bias={-1: 1.0}), "token id"), (dict(bias=[(3, 1.0), (3, 2.0)]), "twice"), (dict(bias={3: 1.0}, suppress=[3]), "twice"), (dict(bias={3: float("inf")}), "not finite"),
           (dict(bias={3: float("nan")}), "not finite")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=r"clip 2: .*" + what):
            engine.rules_array([None, ok, engine.DecodeRules(**kw)], 3, NV, "clip")
    r = engine.DecodeRules(); r.n_bias = 257
    with pytest.raises(ValueError, match="clip 0: n_bias 257"):
        engine.rules_array([r], 1, NV, "clip")
    with pytest.raises(ValueError, match="at most 256"):
        engine.DecodeRules(suppress=range(257))
    with pytest.raises(ValueError, match="2 rule records for 3 clips"):
        engine.rules_array([None, None], 3, NV, "clip")
    assert engine.DecodeRules(suppress=range(256)).n_bias == 256


def test_decode_rules_is_the_c_struct_field_for_field(built):
    from streamkit_amd import engine
    hdr = open(os.path.join(ROOT, "include", "skw_engine.h")).read()
    assert re.search(r"#define\s+SKW_BIAS_MAX\s+256\b", hdr) and engine.BIAS_MAX == 256
    body = re.search(r"typedef struct \{([^}]*)\} skw_decode_rules;", hdr).group(1)
    decl = [(t, n, a) for t, n, a in re.findall(r"(float|int32_t)\s+(\w+)(\[SKW_BIAS_MAX\])?;", body)]
    assert [n for _, n, _ in decl] == [n for n, _ in engine.DecodeRules._fields_]
    off = 0
    for (t, n, a), (fn, ft) in zip(decl, engine.DecodeRules._fields_):
        want = (C.c_float if t == "float" else C.c_int32)
        assert ft == (want * 256 if a else want) and getattr(engine.DecodeRules, fn).offset == off
        off += 4 * (256 if a else 1)
    assert C.sizeof(engine.DecodeRules) == off == 16 + 2048
    L = engine.lib()
    for sym in ("skw_full_batch_rules", "skw_decode_rules_default", "skw_debug_sample_rows_rules"):
        assert hasattr(L, sym), sym
    r = engine.DecodeRules(repetition_penalty=3.0, no_repeat_ngram_size=2, suppress=[1])
    L.skw_decode_rules_default(C.byref(r))
    assert r.is_default() and bytes(r) == bytes(engine.DecodeRules())
    assert C.sizeof(engine.FullParams) == 60                                       # the rules travel beside the parameter block, not in it


def test_full_batch_refuses_rules_with_trace_or_forced_before_touching_the_library():
    from streamkit_amd import engine
    ctx = engine.Context.__new__(engine.Context)                                   # (no device: the refusal comes first)
    for kw in (dict(trace=True), dict(forced=[[1]])):
        with pytest.raises(ValueError, match="rules cannot be combined with trace / forced"):
            ctx.full_batch([np.zeros(16, np.float32)], rules=[None], **kw)


# ---- (e) the node's parameters
def _node_rules(params, n_vocab=51865):
    from streamkit_amd import engine
    L = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libwhisper.so"))
    L.skw_whisper_plugin_parse_rules.argtypes = [C.c_char_p, C.c_int, C.POINTER(engine.DecodeRules), C.c_char_p, C.c_size_t]
    out, err = engine.DecodeRules(), C.create_string_buffer(512)
    if L.skw_whisper_plugin_parse_rules(json.dumps(params).encode(), n_vocab, C.byref(out), err, 512) != 0:
        raise ValueError(err.value.decode())
    return out


def test_node_parameters(built):
    from streamkit_amd import minihost
    props = minihost.Plugin().metadata["param_schema"]["properties"]
    assert props["repetition_penalty"]["type"] == "number" and props["repetition_penalty"]["default"] == 1.0
    assert props["no_repeat_ngram_size"]["type"] == "integer" and props["no_repeat_ngram_size"]["default"] == 0
    assert props["suppress_tokens"]["type"] == "array" and props["suppress_tokens"]["default"] == []
    assert props["logit_bias"]["type"] == "array" and props["logit_bias"]["default"] == []
    assert _node_rules({}).is_default() and _node_rules({"language": "de"}).is_default()
    assert _node_rules({"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "suppress_tokens": [], "logit_bias": []}).is_default()
    r = _node_rules({"repetition_penalty": 1.1, "no_repeat_ngram_size": 3, "suppress_tokens": [7, 9, 7], "logit_bias": [[5, 1.5], [9, 4.0], [0, -2.0]]})
    assert abs(r.repetition_penalty - 1.1) < 1e-6 and r.no_repeat_ngram_size == 3 and r.n_bias == 4
    assert dict(zip(r.bias_id[:4], r.bias[:4])) == {7: float("-inf"), 9: float("-inf"), 5: 1.5, 0: -2.0}      # an id under both keys stays suppressed
    bad = [({"repetition_penalty": 0}, "repetition_penalty"), ({"repetition_penalty": -2.0}, "repetition_penalty"), ({"repetition_penalty": "x"}, "repetition_penalty"),
           ({"no_repeat_ngram_size": -1}, "no_repeat_ngram_size"), ({"no_repeat_ngram_size": 1.5}, "no_repeat_ngram_size"), ({"suppress_tokens": 5}, "suppress_tokens"),
           ({"suppress_tokens": [1, -2]}, "suppress_tokens"), ({"suppress_tokens": [51865]}, "suppress_tokens"), ({"logit_bias": [[1]]}, "logit_bias"),
           ({"logit_bias": [[1, "a"]]}, "logit_bias"), ({"logit_bias": {"1": 2}}, "logit_bias"), ({"logit_bias": [[51865, 1.0]]}, "logit_bias"),
           ({"logit_bias": [[4, 1.0], [4, 2.0]]}, "logit_bias")]
    for params, key in bad:
        with pytest.raises(ValueError, match="Invalid config: .*" + key):
            _node_rules(params)
    assert _node_rules({"suppress_tokens": [51864]}).n_bias == 1
    with pytest.raises(ValueError, match="suppress_tokens: token id 51864 outside"):
        _node_rules({"suppress_tokens": [51864]}, n_vocab=51864)                   # the ids are checked against the loaded model's vocabulary
    assert _node_rules({"suppress_tokens": list(range(200)), "logit_bias": [[i, 1.0] for i in range(150, 256)]}).n_bias == 256      # 306 entries, 256 DISTINCT ids
    with pytest.raises(ValueError, match="at most 256 distinct"):
        _node_rules({"suppress_tokens": list(range(200)), "logit_bias": [[i, 1.0] for i in range(200, 257)]})
    # a bad value fails create_instance before any model is looked for, and the message names the key
    for params, key in bad[:2] + bad[3:4] + bad[5:6] + bad[8:9]:
        with pytest.raises(RuntimeError, match="Invalid config: .*" + key):
            minihost.Plugin().create_node(dict(params, model_path="/nonexistent/model.bin"))
