"""Decoding constraints per clip on the GPU (skw_full_batch_rules, k_dec_constrain): the kernel on its own against the transformers-checked fixture and the oracle's K11, the
engine end to end against the checker composed from the oracle (tests/decode_rules_lib.py), the launches a call without constraints does not make, the no-repeat property in
both precisions with the temperature ladder on, batch invariance, and the Whisper node.

Micro synthetic models; the conditions under which these tests show anything are asserted on the checker alone in tests/test_cpu_decode_rules.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import context_ref_lib as cr
import decode_rules_lib as dr
import logit_rules_lib as lr
from conftest import synth_model
from decode_rules_lib import LOOP_BIAS, RULE_SETS, fixture

pytestmark = pytest.mark.gpu
N_SAMPLES = 160000
_PCM = {}
_REF = {}


def clip(seed):
    if seed not in _PCM:
        from streamkit_amd import synth
        _PCM[seed] = synth.clip(seed, N_SAMPLES); _PCM[seed].setflags(write=False)
    return _PCM[seed]


def checker(om, seed, name, context=()):
    """computed once per (clip, rule set, context), shared, never modified"""
    key = (seed, name, tuple(context))
    if key not in _REF:
        _REF[key] = dr.full_with_rules(om, clip(seed), context, cr.params_for(om), RULE_SETS[name])
    return _REF[key]


def engine_params(ctx, **kw):
    p = ctx.default_params()
    p.temperature_inc = 0.0; p.no_speech_thold = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def same(a, b):
    return (cr.token_bits(a["tokens"]) == cr.token_bits(b["tokens"]) and a["segments"] == b["segments"] and a["n_windows"] == b["n_windows"]
            and a["lang_id"] == b["lang_id"] and a["fallback_requested"] == b["fallback_requested"])


@pytest.fixture(scope="module")
def gm(micro_model_path):
    from streamkit_amd import engine
    m = engine.Model(micro_model_path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ctx(gm):
    from streamkit_amd import engine
    c = engine.Context(gm, max_batch=8, max_samples=N_SAMPLES + 1024)
    yield c
    c.close()


# ---- 1. the kernel on its own: fixture cases through Context.sample_rows(rules=...), both sampler forms, 64 rows per launch
@pytest.mark.parametrize("vi", [0, 1, 2], ids=["v51865", "v51864", "v51866"])
def test_kernel_against_fixture_and_oracle(eng, vi):
    from oracle_lib import OracleModel
    v = fixture()["vocabs"][vi]
    sp, NV = v["special"], v["n_vocab"]
    path = synth_model("micro", vocab=NV, mels=v["n_mels"])
    om = OracleModel(path); m = eng.Model(path); ctx = eng.Context(m, max_batch=64)
    try:
        assert m.hp.n_vocab == NV and lr.special_ids(om) == sp
        rows = []
        for c in v["cases"]:
            hist, raw, rules = dr.make_rule_case(c["seed"], sp, NV, c["spec"])
            assert dr.row_hash(dr.transform(hist, raw, rules, sp["eot"])) == c["sha256"]      # the row the fixture (and transformers) saw
            rows.append((hist, raw, rules))
        rows += [(h, raw, None) for h, raw, _ in rows[1::3]][:28]                             # rows without a record, on inputs that have one elsewhere
        order = np.random.default_rng(5).permutation(len(rows))                               # the None rows land among the others
        rows = [rows[i] for i in order]
        assert len(rows) == 128
        n_changed = 0
        for b0 in (0, 64):
            batch = rows[b0:b0 + 64]
            hists = [h for h, _, _ in batch]; lg = np.stack([raw for _, raw, _ in batch])
            params, oparams = [], []
            for r in range(64):      # the per-row request rules vary too: the static mask with and without the non-speech list
                p = ctx.default_params(); p.suppress_nst = r % 2; params.append(p)
                po = om.default_params(); po.suppress_nst = r % 2; oparams.append(po)
            er = [dr.to_engine(rules) for _, _, rules in batch]
            assert len({bytes(x) for x in er if x is not None}) >= 32 and sum(x is None for x in er) >= 8      # the rows' records differ; some rows have none
            tk0, _, _ = ctx.sample_rows(hists, lg, params, form=0, rules=er)
            tk1, _, filt = ctx.sample_rows(hists, lg, params, form=1, want_filtered=True, rules=er)
            pk0, _, _ = ctx.sample_rows(hists, lg, params, form=0)
            pk1, _, pfilt = ctx.sample_rows(hists, lg, params, form=1, want_filtered=True)
            for r, (hist, raw, rules) in enumerate(batch):
                o = lr.oracle_process(om, oparams[r], hist, dr.transform(hist, raw, rules, sp["eot"]))
                assert o is not None
                assert np.array_equal(np.isneginf(filt[r]), np.isneginf(o[0])), (NV, b0, r)
                fin = ~np.isneginf(o[0])
                assert np.array_equal(filt[r][fin].view(np.uint32), o[0][fin].view(np.uint32)), (NV, b0, r)
                for f in ("id", "tid", "p", "plog", "pt", "ptsum"):
                    assert np.float32(tk0[f][r]) == np.float32(o[2][f]) and np.float32(tk1[f][r]) == np.float32(o[2][f]), (NV, b0, r, f, tk0[f][r], tk1[f][r], o[2][f])
                if rules is None:
                    assert tk0[r].tobytes() == pk0[r].tobytes() and tk1[r].tobytes() == pk1[r].tobytes() and filt[r].tobytes() == pfilt[r].tobytes(), (NV, b0, r)
                else:
                    n_changed += int(tk0["id"][r]) != int(pk0["id"][r])
        assert n_changed >= 20                                                                # the constraints decided something
    finally:
        ctx.close(); m.close(); om.close()


def test_engine_refuses_bad_records_naming_the_clip(eng, ctx):
    """the engine's own check (the binding's is tested without a device): records the binding would not let through, handed to the C entry point directly"""
    L = eng.lib()
    pcm = np.ascontiguousarray(clip(0)[:16000], np.float32)
    n = 3
    for field, value, what in (("repetition_penalty", 0.0, "repetition_penalty"), ("repetition_penalty", float("nan"), "repetition_penalty"), ("no_repeat_ngram_size", -2, "no_repeat_ngram_size"),
                               ("n_bias", 257, "n_bias"), ("n_bias", -1, "n_bias"), ("id", ctx.model.hp.n_vocab, "token id"), ("id", -1, "token id"), ("dup", 0, "twice"),
                               ("bias", float("inf"), "not finite"), ("bias", float("nan"), "not finite")):
        bad = eng.DecodeRules(bias={7: 1.0, 8: 2.0})
        if field == "id":
            bad.bias_id[1] = value
        elif field == "dup":
            bad.bias_id[1] = 7
        elif field == "bias":
            bad.bias[1] = value
        else:
            setattr(bad, field, value)
        ptrs = (C.c_void_p * n)(*[pcm.ctypes.data] * n); ns = (C.c_int32 * n)(*[pcm.size] * n); res = (eng.Result * n)()
        pp = (eng.FullParams * n)(*[ctx.default_params()] * n)
        rp = (C.c_void_p * n)(None, C.addressof(bad), None)
        assert L.skw_full_batch_rules(ctx.h, pp, ptrs, ns, n, 0, None, None, rp, res) != 0
        assert "clip 1" in ctx.last_error() and what in ctx.last_error(), (field, value, ctx.last_error())
    with pytest.raises(ValueError, match="clip 0: repetition_penalty"):
        ctx.full_batch([pcm], rules=[eng.DecodeRules(repetition_penalty=-1.0)])
    with pytest.raises(ValueError, match="row 1: .*twice"):
        ctx.sample_rows([[], []], np.zeros((2, ctx.model.hp.n_vocab), np.float32), [ctx.default_params()] * 2, rules=[None, eng.DecodeRules(bias=[(3, 1.0), (3, 1.0)])])


# ---- 2. end to end, exact precision
def test_engine_equals_checker_per_row(eng, ctx, oracle_micro):
    om = oracle_micro
    sp = lr.special_ids(om)
    c8 = cr.make_context(np.random.default_rng(11), sp, 8)
    rows = [(0, "plain", ()), (3, "bias", ()), (0, "bias_t", ()), (3, "bias_n2", ()), (0, "bias_t_n3", ()), (3, None, ()), (3, "bias_t", tuple(c8)), (0, "bias_n2", tuple(c8))]
    er = [None if name is None else (eng.DecodeRules() if name == "plain" else dr.to_engine(RULE_SETS[name])) for _, name, _ in rows]
    cxs = [eng.context_new(list(c)) for _, _, c in rows]
    clips = [clip(s) for s, _, _ in rows]
    got = ctx.full_batch(clips, engine_params(ctx), contexts=cxs, rules=er)
    for k, (seed, name, c) in enumerate(rows):
        ref = checker(om, seed, name or "plain", c)
        assert cr.token_bits(got[k]["tokens"]) == cr.token_bits(ref["tokens"]), (k, name)
        assert [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in got[k]["segments"]] == [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in ref["segments"]], (k, name)
        assert got[k]["n_windows"] == ref["n_windows"] and eng.context_ids(cxs[k]) == ref["context"], (k, name)
    ids = [[t[0] for t in g["tokens"]] for g in got]
    assert ids[1] != ids[5] and ids[2] != ids[1] and ids[3] != ids[1] and ids[4] not in (ids[0], ids[2])      # the rules did something (tests/test_cpu_decode_rules.py: on the checker)
    # the plain and the None row are the call without rules, bit for bit
    cxs2 = [eng.context_new(list(c)) for _, _, c in rows]
    base = ctx.full_batch(clips, engine_params(ctx), contexts=cxs2)
    for k in (0, 5):
        assert same(got[k], base[k]) and np.array_equal(cxs[k], cxs2[k]), k
    # ... and so is a call whose records are all default, whatever else it carries
    cxs3 = [eng.context_new(list(c)) for _, _, c in rows]
    dflt = ctx.full_batch(clips, engine_params(ctx), contexts=cxs3, rules=[eng.DecodeRules() if k % 2 else None for k in range(8)])
    assert all(same(a, b) for a, b in zip(dflt, base)) and all(np.array_equal(a, b) for a, b in zip(cxs3, cxs2))


# ---- 3. a call without constraints launches nothing new
def test_no_constraint_launches_by_default(eng, ctx):
    clips = [clip(0), clip(3)]
    ctx.profile(True)
    ctx.full_batch(clips, engine_params(ctx))
    assert ctx.profile_get()["k_dec_constrain"]["count"] == 0 and ctx.profile_get()["k_dec_sample"]["count"] > 0
    ctx.profile(True)
    ctx.full_batch(clips, engine_params(ctx), rules=[eng.DecodeRules(), None])
    assert ctx.profile_get()["k_dec_constrain"]["count"] == 0
    ctx.profile(True)
    a = ctx.full_batch(clips, engine_params(ctx), rules=[None, dr.to_engine(RULE_SETS["bias_n2"])])
    prof = ctx.profile_get()
    ctx.profile(False)
    assert prof["k_dec_constrain"]["count"] > 0 and prof["k_dec_constrain"]["count"] == prof["k_dec_sample"]["count"]
    b = ctx.full_batch(clips, engine_params(ctx), rules=[None, dr.to_engine(RULE_SETS["bias_n2"])])      # the captured step graph gives what the eager, profiled step gave
    assert all(same(x, y) for x, y in zip(a, b))


# ---- 4. the property, both precisions, temperature ladder on
@pytest.mark.parametrize("precision", ["exact", "f16_mfma"])
def test_no_bigram_repeats_under_the_rule_on_greedy_and_sampled_passes(eng, ctx, oracle_micro, precision):
    eot = lr.special_ids(oracle_micro)["eot"]
    clips = [clip(0), clip(3)]
    loop = dr.to_engine(RULE_SETS["bias"]); n2 = dr.to_engine(RULE_SETS["bias_n2"])
    ctx.set_precision(precision)
    try:
        # (a) whisper.cpp's default thresholds: whatever the ladder does, the window's pass result holds no bigram twice
        # (b) logprob_thold = 1: no pass can reach it (an average log-probability is <= 0), so every window goes down the whole ladder and its result is the pass SAMPLED at
        #     temperature 1.0 — the rule held on a drawn pass
        for forced in (False, True):
            p = ctx.default_params()
            assert p.temperature_inc > 0.0
            if forced:
                p.logprob_thold = 1.0; p.no_speech_thold = 1.0
            free = ctx.full_batch(clips, p, rules=[loop, loop])
            held = ctx.full_batch(clips, p, rules=[n2, n2])
            for k in range(2):
                assert free[k]["n_windows"] == 1 and held[k]["n_windows"] == 1                      # a 10 s clip is one window: the result's tokens are one pass's
                ids_f = [t[0] for t in free[k]["tokens"]]; ids_h = [t[0] for t in held[k]["tokens"]]
                assert dr.repeated_bigrams(ids_f, eot) > 0, (precision, forced, k)                  # the looping bias loops (also when drawn: +50 leaves three tokens any mass)
                assert len(dr.text_tokens(ids_h, eot)) >= 4 and dr.repeated_bigrams(ids_h, eot) == 0, (precision, forced, k, ids_h)
                if forced:
                    assert free[k]["fallback_requested"] >= 1 and held[k]["fallback_requested"] == 6, (free[k]["fallback_requested"], held[k]["fallback_requested"])
        if precision == "f16_mfma":      # all-default records are the call without rules, bit for bit, in this precision too
            p = ctx.default_params()
            a = ctx.full_batch(clips, p); b = ctx.full_batch(clips, p, rules=[eng.DecodeRules(), None])
            assert all(same(x, y) for x, y in zip(a, b))
    finally:
        ctx.set_precision("exact")


# ---- 5. a constrained clip alone == the same clip among seven others with other rules and parameters (exact)
def test_mixed_batch_invariance(eng, ctx):
    rules = [dr.to_engine(RULE_SETS["bias_t_n3"]), None, dr.to_engine(RULE_SETS["bias"]), eng.DecodeRules(no_repeat_ngram_size=1), dr.to_engine(RULE_SETS["bias_n2"]),
             eng.DecodeRules(repetition_penalty=4.0), eng.DecodeRules(suppress=[48931, 9388]), dr.to_engine(RULE_SETS["bias_t"])]
    params = [ctx.default_params() for _ in range(8)]                                              # the ladder is on: rows may be decoded again beside rows that are not
    params[1].suppress_nst = 0; params[2].audio_ctx = 512; params[3].no_timestamps = 1; params[5].temperature_inc = 0.0; params[6].max_tokens = 12
    params[4].logprob_thold = 1.0; params[4].no_speech_thold = 1.0                                 # this row goes down the whole ladder
    seeds = [0, 3, 0, 3, 3, 0, 3, 0]
    clips = [clip(s) for s in seeds]
    st = [eng.rng_state_new() for _ in range(8)]
    got = ctx.full_batch(clips, params, rng_states=st, rules=rules)
    assert got[4]["fallback_requested"] == 6
    for k in (0, 4, 6, 7):
        s1 = eng.rng_state_new()
        alone = ctx.full_batch([clips[k]], [params[k]], rng_states=[s1], rules=[rules[k]])[0]
        assert same(alone, got[k]) and np.array_equal(s1, st[k]), k
    assert not same(got[0], got[7])


# ---- 6. the node
def _node_segments(o):
    return [{"text": s["text"].decode().strip(), "start_time_ms": s["t0"] * 10, "end_time_ms": s["t1"] * 10, "confidence": None} for s in o["segments"] if s["text"].decode().strip()]


def _feed(node, pcm):
    for i in range(0, pcm.size, 960):
        assert node.process_audio(pcm[i:i + 960]) == 0, node.last_error()


def _feed_and_flush_together(nodes, pcms):
    import threading
    barrier = threading.Barrier(len(nodes)); rcs = [None] * len(nodes); errors = []

    def worker(k):
        try:
            _feed(nodes[k], pcms[k])
            barrier.wait(timeout=120)
            rcs[k] = nodes[k].flush()
        except Exception as e:      # noqa: BLE001
            errors.append((k, repr(e))); barrier.abort()

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(len(nodes))]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errors, errors
    return rcs


def test_node_instances_with_and_without_rules_share_a_batch(eng, ctx, micro_model_path):
    from streamkit_amd import minihost
    plugin = minihost.Plugin()
    pcm = clip(3)
    cfg = dict(model_path=micro_model_path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=300, max_batch=8)
    ruled = dict(no_repeat_ngram_size=2, logit_bias=[[i, b] for i, b in LOOP_BIAS])
    # what the engine gives for each alone (the node's parameters: English, both suppress_* rules, the ladder on)
    p = ctx.default_params(); p.lang_id = 0; p.suppress_blank = 1; p.suppress_nst = 1
    want_plain = ctx.full_batch([pcm], p)[0]
    want_ruled = ctx.full_batch([pcm], p, rules=[eng.DecodeRules(no_repeat_ngram_size=2, bias=LOOP_BIAS)])[0]
    assert _node_segments(want_plain) and _node_segments(want_ruled) and _node_segments(want_plain) != _node_segments(want_ruled)
    out = lambda nd, k0=0: [json.loads(o[2].decode()) for o in nd.outputs()][k0:]
    nodes = [plugin.create_node(dict(cfg, **ruled)), plugin.create_node(dict(cfg))]
    before = minihost.whisper_batch_stats()
    assert _feed_and_flush_together(nodes, [pcm, pcm]) == [0, 0], [n.last_error() for n in nodes]
    calls, jobs, _ = (a - b for a, b in zip(minihost.whisper_batch_stats(), before))
    assert (calls, jobs) == (1, 2)
    assert len(out(nodes[0])) == 1 and out(nodes[0])[0]["segments"] == _node_segments(want_ruled)
    assert len(out(nodes[1])) == 1 and out(nodes[1])[0]["segments"] == _node_segments(want_plain)
    # update_params switches the rule on for the next segment (the stream's clock ran on: texts and durations are compared)
    assert nodes[1].update_params(dict(cfg, **ruled)) == 0, nodes[1].last_error()
    _feed(nodes[1], pcm)
    assert nodes[1].flush() == 0, nodes[1].last_error()
    nxt = out(nodes[1], 1)
    assert len(nxt) == 1 and [s["text"] for s in nxt[0]["segments"]] == [s["text"] for s in _node_segments(want_ruled)]
    assert [s["end_time_ms"] - s["start_time_ms"] for s in nxt[0]["segments"]] == [s["end_time_ms"] - s["start_time_ms"] for s in _node_segments(want_ruled)]
    assert nodes[1].update_params(dict(cfg, suppress_tokens=[ctx.model.hp.n_vocab])) != 0 and "suppress_tokens" in nodes[1].last_error()
    for nd in nodes:
        nd.destroy()
    # mixed_batch: false cuts the batch where the rules differ
    nodes = [plugin.create_node(dict(cfg, mixed_batch=False, **ruled)), plugin.create_node(dict(cfg, mixed_batch=False))]
    before = minihost.whisper_batch_stats()
    assert _feed_and_flush_together(nodes, [pcm, pcm]) == [0, 0], [n.last_error() for n in nodes]
    calls, jobs, _ = (a - b for a, b in zip(minihost.whisper_batch_stats(), before))
    assert (calls, jobs) == (2, 2)
    assert out(nodes[0])[0]["segments"] == _node_segments(want_ruled) and out(nodes[1])[0]["segments"] == _node_segments(want_plain)
    for nd in nodes:
        nd.destroy()
    # a bad value fails create_instance, naming the key
    for bad, key in ((dict(repetition_penalty=0), "repetition_penalty"), (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(suppress_tokens=[ctx.model.hp.n_vocab]), "suppress_tokens"),
                     (dict(logit_bias=[[1, 2, 3]]), "logit_bias")):
        with pytest.raises(RuntimeError, match=key):
            plugin.create_node(dict(cfg, **bad))
