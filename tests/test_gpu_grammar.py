"""Grammar-constrained decoding on the GPU (skw_full_batch_grammar, k_dec_grammar; include/skw_grammar.h): the kernel on its own against the contract's restatement and the
oracle's K11, the engine end to end against the checker composed from the oracle (tests/grammar_lib.py), the property that a transcript decoded under a pattern matches it
(re.fullmatch; both precisions, greedy and drawn passes), what a call without a grammar does not do, batch invariance, refused records, and the Whisper node.

Micro synthetic models, 10 s clips; the conditions under which these tests show anything are asserted on the oracle alone in tests/test_cpu_grammar.py."""
import ctypes as C
import json
import re

import numpy as np
import pytest

import context_ref_lib as cr
import decode_rules_lib as dr
import grammar_lib as gl
import logit_rules_lib as lr
from conftest import synth_model

pytestmark = pytest.mark.gpu
_PCM = {}
_REF = {}
_GRAM = {}
NAMES = list(gl.TEST_PATTERNS)
RX = {k: re.compile(v.encode()) for k, v in gl.TEST_PATTERNS.items()}


def clip(seed):
    if seed not in _PCM:
        from streamkit_amd import synth
        _PCM[seed] = synth.clip(seed, gl.N_SAMPLES); _PCM[seed].setflags(write=False)
    return _PCM[seed]


def gram(name):
    """the test pattern `name` at the test penalty, compiled once (a dict; gl.to_engine makes the binding's Grammar)"""
    if name not in _GRAM:
        _GRAM[name] = gl.compile_py(gl.TEST_PATTERNS[name], penalty=gl.TEST_PENALTY)
    return _GRAM[name]


def checker(om, voc, seed, name, no_timestamps=1, context=(), rules=None, rules_key=None):
    """computed once per case, shared, never modified"""
    key = (seed, name, no_timestamps, tuple(context), rules_key)
    if key not in _REF:
        p = cr.params_for(om); p.no_timestamps = no_timestamps
        _REF[key] = gl.full_with_grammar(om, clip(seed), None if name is None else gram(name), voc, context, p, rules)
    return _REF[key]


def engine_params(ctx, **kw):
    p = ctx.default_params()
    p.temperature_inc = 0.0; p.no_speech_thold = 1.0; p.no_timestamps = 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def same(a, b):
    return (cr.token_bits(a["tokens"]) == cr.token_bits(b["tokens"]) and a["segments"] == b["segments"] and a["n_windows"] == b["n_windows"]
            and a["lang_id"] == b["lang_id"] and a["fallback_requested"] == b["fallback_requested"])


def equals_checker(got, ref):
    return (cr.token_bits(got["tokens"]) == cr.token_bits(ref["tokens"]) and got["n_windows"] == ref["n_windows"]
            and [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in got["segments"]] == [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in ref["segments"]])


def text_of(res):
    return b"".join(s["text"] for s in res["segments"])


@pytest.fixture(scope="module")
def gm(micro_model_path):
    from streamkit_amd import engine
    m = engine.Model(micro_model_path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ctx(gm):
    from streamkit_amd import engine
    c = engine.Context(gm, max_batch=16, max_samples=gl.N_SAMPLES + 1024)
    yield c
    c.close()


@pytest.fixture(scope="module")
def voc(oracle_micro):
    return gl.vocab_image(oracle_micro.token_bytes, lr.special_ids(oracle_micro)["eot"])


# ---- 1. the kernel on its own: constrain -> grammar -> sampler through Context.sample_rows(grammars=...), one launch each at 1, 3 and 64 rows
@pytest.mark.parametrize("vocab,mels", [(51865, 80), (51864, 80), (51866, 128)], ids=["v51865", "v51864", "v51866"])
def test_kernel_equals_the_contract_and_the_oracle(eng, vocab, mels):
    from oracle_lib import OracleModel
    path = synth_model("micro", vocab=vocab, mels=mels)
    om = OracleModel(path); m = eng.Model(path); ctx = eng.Context(m, max_batch=64)
    try:
        sp = lr.special_ids(om); eot, beg, NV = sp["eot"], sp["beg"], vocab
        voc = gl.vocab_image(om.token_bytes, eot)
        assert m.hp.n_vocab == NV
        ids_of = {}
        for t in range(eot):
            ids_of.setdefault(bytes(om.token_bytes(t)), t)
        spell = lambda s: [ids_of[bytes([c])] for c in s]
        words = [t for t in range(256, 4000) if bytes(om.token_bytes(t)).startswith(b" ") and bytes(om.token_bytes(t))[1:].isalpha()]
        ts = lambda k: [beg + k, beg + k]
        G = dict(digits=gl.compile_py(gl.TEST_PATTERNS["digits"], penalty=gl.TEST_PENALTY), yesno=gl.compile_py(gl.TEST_PATTERNS["yesno"], penalty=100.0),
                 words=gl.compile_py(gl.TEST_PATTERNS["words"], penalty=0.75), t1=gl.letters_table(1, 3.0), t2=gl.letters_table(2), t128=gl.letters_table(128, 50.0),
                 t129=gl.letters_table(129, 50.0), t4096=gl.letters_table(4096), c4096=gl.chain_table(4096, 12.5))
        assert [G[k]["accept"].size for k in ("t1", "t2", "t128", "t129", "t4096", "c4096")] == [1, 2, 128, 129, 4096, 4096]
        LONG = 223      # the longest history the hook (and the token loop: one slot is the decision's own) can hold: max_tok - 1
        r_mix = dict(theta=1.5, N=0, bias=[(words[0], 7.0), (ids_of[b"#"], -3.0), (eot, 2.0)])
        r_ng = dict(theta=2.0, N=2, bias=[(ids_of[b"4"], 10.0)])
        # (grammar, history, decode rules, active)
        specs = [("digits", [], None, 1), (None, words[:3], None, 1), ("t4096", words[:LONG], None, 1),
                 ("digits", spell(b"4"), None, 1), ("digits", ts(2) + spell(b"41") + ts(4) + spell(b"578"), None, 1), ("digits", spell(b"4a"), None, 1), ("digits", spell(b"41"), r_ng, 1),
                 ("yesno", [], None, 1), ("yesno", spell(b" ye"), None, 1), ("yesno", spell(b"maybe"), None, 1), ("yesno", spell(b"nope"), None, 1),
                 ("words", [], None, 1), ("words", words[:2], None, 1), ("words", words[:3], r_mix, 1), ("words", words[:4], None, 1),
                 ("t1", [], None, 1), ("t1", words[:1], None, 1), ("t2", [], None, 1), ("t2", words[:1], r_mix, 1), ("t128", [], None, 1), ("t128", words[:5], r_mix, 1),
                 ("t128", words[:LONG], None, 1), ("t129", [], None, 1), ("t129", words[:1], None, 1), ("t129", [beg] + words[:LONG - 3] + ts(9), None, 1),
                 ("t4096", [], None, 1), ("t4096", words[:1], None, 1), ("c4096", [], None, 1), ("c4096", spell(b"a"), None, 1), ("c4096", spell(b"a") * LONG, None, 1),
                 ("c4096", spell(b"ab"), None, 1), (None, [], None, 1), (None, spell(b"41"), r_ng, 1),
                 ("digits", spell(b"4"), None, 0), ("t4096", words[:LONG], None, 0), (None, words[:2], None, 0), ("words", words[:2], r_mix, 0)]
        rng = np.random.default_rng(vocab)
        rows = []
        k = 0
        while len(rows) < 64:      # the specs again on other logits until the launch is full
            g, h, r, a = specs[k % len(specs)]; k += 1
            x = (rng.standard_normal(NV) * 30.0).astype(np.float32)
            x[rng.integers(0, NV, 5)] = -np.inf
            rows.append((g, list(h), r, a, x))
        params = [ctx.default_params() for _ in range(64)]
        po = om.default_params()
        states = set(); n_changed = 0
        for n in (1, 3, 64):
            batch = rows[:n]
            hists = [h for _, h, _, _, _ in batch]; lg = np.stack([x for *_, x in batch])
            kw = dict(rules=[dr.to_engine(r) for _, _, r, _, _ in batch], grammars=[gl.to_engine(None if g is None else G[g]) for g, *_ in batch], active=[a for _, _, _, a, _ in batch])
            tk0, _, _ = ctx.sample_rows(hists, lg, params[:n], form=0, **kw)
            tk1, _, filt = ctx.sample_rows(hists, lg, params[:n], form=1, want_filtered=True, **kw)
            pk0, _, _ = ctx.sample_rows(hists, lg, params[:n], form=0, rules=kw["rules"])
            for r, (g, h, rules, active, x) in enumerate(batch):
                if not active:      # a finished row: no kernel touches its logits
                    assert np.array_equal(filt[r].view(np.uint32), x.view(np.uint32)), (vocab, n, r)
                    continue
                s, want = gl.apply(None if g is None else G[g], voc, eot, h, dr.transform(h, x, rules, eot))      # the stage order: rules' three, then the grammar
                states.add("none" if g is None else "dead" if s == gl.DEAD else "accept" if G[g]["accept"][s] else "open")
                o = lr.oracle_process(om, po, h, want)
                assert o is not None
                assert np.array_equal(np.isneginf(filt[r]), np.isneginf(o[0])), (vocab, n, r, g)
                fin = ~np.isneginf(o[0])
                assert np.array_equal(filt[r][fin].view(np.uint32), o[0][fin].view(np.uint32)), (vocab, n, r, g)
                for f in ("id", "tid", "p", "plog", "pt", "ptsum"):
                    assert np.float32(tk0[f][r]) == np.float32(o[2][f]) and np.float32(tk1[f][r]) == np.float32(o[2][f]), (vocab, n, r, g, f, tk0[f][r], tk1[f][r], o[2][f])
                if g is None or s == gl.DEAD:      # no grammar, or the walk left the language: the row is the one without a grammar, bit for bit
                    assert tk0[r].tobytes() == pk0[r].tobytes(), (vocab, n, r, g)
                elif n == 64:
                    n_changed += int(tk0["id"][r]) != int(pk0["id"][r])
        # the grammars decided something (on random logits the sampler's timestamp rules settle most rows for a timestamp whatever the text logits are: a handful is what to expect)
        assert states == {"none", "dead", "accept", "open"} and n_changed >= 5
    finally:
        ctx.close(); m.close(); om.close()


def test_engine_refuses_bad_records_naming_the_clip(eng, ctx):
    L = eng.lib()
    pcm = np.ascontiguousarray(clip(0)[:16000], np.float32)
    n = 3
    before = L.skw_debug_grammar_uploads(ctx.h)
    for field, value, what in (("n_states", 0, "n_states"), ("n_states", 4097, "n_states"), ("penalty", 0.0, "penalty"), ("penalty", float("nan"), "penalty"),
                               ("penalty", float("inf"), "penalty"), ("next", 3, "next[1][7]"), ("accept", 2, "accept[2]")):
        t = gl.chain_table(3)
        if field == "next":
            t["next"][1, 7] = value
        elif field == "accept":
            t["accept"][2] = value
        g = gl.to_engine(t)
        if field in ("n_states", "penalty"):
            setattr(g.rec, field, value)
        ptrs = (C.c_void_p * n)(*[pcm.ctypes.data] * n); ns = (C.c_int32 * n)(*[pcm.size] * n); res = (eng.Result * n)()
        pp = (eng.FullParams * n)(*[ctx.default_params()] * n)
        gp = (C.c_void_p * n)(None, C.addressof(g.rec), None)
        assert L.skw_full_batch_grammar(ctx.h, pp, ptrs, ns, n, 0, None, None, None, None, None, gp, res) != 0
        assert "clip 1" in ctx.last_error() and what in ctx.last_error(), (field, value, ctx.last_error())
    with pytest.raises(RuntimeError, match="row 1: grammar: penalty"):
        bad = gl.to_engine(gl.chain_table(3)); bad.rec.penalty = -1.0
        ctx.sample_rows([[], []], np.zeros((2, ctx.model.hp.n_vocab), np.float32), [ctx.default_params()] * 2, grammars=[None, bad])
    assert L.skw_debug_grammar_uploads(ctx.h) == before      # refused before anything was allocated or launched


# ---- 2. end to end, exact precision: three clips x three grammars in one call
def test_engine_equals_checker(eng, ctx, oracle_micro, voc):
    om = oracle_micro
    cases = [(s, n) for s in gl.TEST_SEEDS for n in NAMES]
    clips = [clip(s) for s, _ in cases]
    gs = [gl.to_engine(gram(n)) for _, n in cases]
    got = ctx.full_batch(clips, engine_params(ctx), grammars=gs)
    for k, (seed, name) in enumerate(cases):
        ref = checker(om, voc, seed, name)
        assert equals_checker(got[k], ref) and got[k]["fallback_requested"] == 0, (seed, name, text_of(got[k]))
        assert RX[name].fullmatch(text_of(got[k])), (seed, name, text_of(got[k]))
    plain = ctx.full_batch([clip(s) for s in gl.TEST_SEEDS], engine_params(ctx))
    assert all(text_of(a) != text_of(b) for a, b in zip(got[::3], plain))      # the grammar changed every transcript
    # the temperature ladder on, whisper.cpp's thresholds: no pass of these falls back (the CPU tier's checker shows average log-probabilities above -0.8 and at most 32 tokens),
    # so the result is still the checker's — through the step graphs of a call whose any_sampled flag may differ
    ladder = ctx.full_batch(clips, engine_params(ctx, temperature_inc=0.2, no_speech_thold=0.6), grammars=gs)
    for k, (seed, name) in enumerate(cases):
        assert equals_checker(ladder[k], checker(om, voc, seed, name)) and ladder[k]["fallback_requested"] == 0, (seed, name)


def test_engine_equals_checker_with_context_rules_and_word_timestamps(eng, ctx, oracle_micro, voc):
    om = oracle_micro
    sp = lr.special_ids(om)
    c8 = cr.make_context(np.random.default_rng(11), sp, 8)
    # behind a carried context
    cxs = [eng.context_new(list(c8)) for _ in NAMES]
    got = ctx.full_batch([clip(3)] * 3, engine_params(ctx), contexts=cxs, grammars=[gl.to_engine(gram(n)) for n in NAMES])
    for k, name in enumerate(NAMES):
        ref = checker(om, voc, 3, name, context=tuple(c8))
        assert equals_checker(got[k], ref) and eng.context_ids(cxs[k]) == ref["context"], name
        assert RX[name].fullmatch(text_of(got[k])), (name, text_of(got[k]))
    # with timestamps, a decode-rules record (its three stages run first) and word timestamps: timestamps are transparent to the match
    first = {n: [t[0] for t in checker(om, voc, 0, n, no_timestamps=0)["tokens"] if t[0] < sp["eot"]][0] for n in NAMES}
    rules = {n: dict(theta=1.3, N=2, bias=[(first[n], -gl.TEST_PENALTY / 4)]) for n in NAMES}      # pushes the plain run's first token down: the transcript changes, the match holds
    al = eng.align_params(top=1, hp=ctx.model.hp)
    got = ctx.full_batch([clip(0)] * 3, engine_params(ctx, no_timestamps=0), rules=[dr.to_engine(rules[n]) for n in NAMES], align=[al] * 3,
                         grammars=[gl.to_engine(gram(n)) for n in NAMES])
    for k, name in enumerate(NAMES):
        ref = checker(om, voc, 0, name, no_timestamps=0, rules=rules[name], rules_key=name)
        assert equals_checker(got[k], ref), (name, text_of(got[k]))
        # with timestamps the synthetic model closes a segment early and the clip takes several windows; the match restarts in each (the documented limit: a grammar is
        # per window), so it is every window's pass that matches — the passes are the checker's, whose tokens the engine's equal
        texts = [gl.transcript_bytes(om.token_bytes, ids, sp["eot"]) for ids in ref["passes"]]
        assert b"".join(texts) == text_of(got[k]) and got[k]["n_windows"] == len(texts) and all(RX[name].fullmatch(t) for t in texts), (name, texts)
        assert any(t[0] >= sp["beg"] for t in got[k]["tokens"]), name
        assert [t[0] for t in got[k]["tokens"]] != [t[0] for t in checker(om, voc, 0, name, no_timestamps=0)["tokens"]], name      # the rules did something too
        tt = got[k]["token_times"]
        assert len(tt) == len(got[k]["tokens"]) and all((a >= 0) == (t[0] < sp["eot"]) for (a, _), t in zip(tt, got[k]["tokens"])), name


# ---- 3. the property, both precisions, greedy and drawn passes
@pytest.mark.parametrize("precision", ["exact", "f16_mfma"])
def test_every_transcript_matches_its_pattern(eng, ctx, precision):
    cases = [(s, n) for s in gl.TEST_SEEDS for n in NAMES]
    clips = [clip(s) for s, _ in cases]
    gs = [gl.to_engine(gram(n)) for _, n in cases]
    ctx.set_precision(precision)
    try:
        for forced in (False, True):
            # forced: logprob_thold = 1 — no pass can reach it, so every window goes down the whole ladder (retries on moved slots) and its result is the pass DRAWN at
            # temperature 1.0: a token that does not fit keeps exp(-(penalty - spread)) of the mass, which is 0 in f32
            p = ctx.default_params(); p.no_timestamps = 1
            assert p.temperature_inc > 0.0
            if forced:
                p.logprob_thold = 1.0; p.no_speech_thold = 1.0
            st = [eng.rng_state_new() for _ in cases]
            got = ctx.full_batch(clips, p, rng_states=st, grammars=gs)
            for k, (seed, name) in enumerate(cases):
                assert got[k]["n_windows"] == 1 and got[k]["fallback_requested"] == (6 if forced else 0), (precision, forced, seed, name, got[k]["fallback_requested"])
                assert RX[name].fullmatch(text_of(got[k])), (precision, forced, seed, name, text_of(got[k]))
            if forced:      # a drawn pass beside others == the same clip alone (its generator continued the same way)
                for k in (2, 4):
                    s1 = eng.rng_state_new()
                    alone = ctx.full_batch([clips[k]], p, rng_states=[s1], grammars=[gs[k]])[0]
                    assert same(alone, got[k]) and np.array_equal(s1, st[k]), (precision, k)
    finally:
        ctx.set_precision("exact")


# ---- 4. nothing changes for callers without a grammar
def test_no_grammar_is_the_aligned_call_bit_for_bit(eng, gm):
    c = eng.Context(gm, max_batch=4, max_samples=gl.N_SAMPLES + 1024)
    try:
        L = eng.lib()
        clips = [clip(0), clip(3)]
        p = c.default_params()
        rules = [dr.to_engine(dr.RULE_SETS["bias_n2"]), None]
        al = [eng.align_params(top=1, hp=gm.hp), None]
        base = c.full_batch(clips, p, rules=rules, align=al)                                  # skw_full_batch_aligned
        c.profile(True)
        null_entries = c.full_batch(clips, p, rules=rules, align=al, grammars=[None, None])
        prof = c.profile_get()
        c.profile(False)
        assert prof["k_dec_grammar"]["count"] == 0 and prof["k_dec_sample"]["count"] > 0 and prof["k_dec_constrain"]["count"] > 0
        n = 2      # grammar == NULL, handed to the C entry point itself
        keep = [np.ascontiguousarray(x, np.float32) for x in clips]
        ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in keep]); ns = (C.c_int32 * n)(*[x.size for x in keep]); res = (eng.Result * n)()
        assert L.skw_full_batch_grammar(c.h, (eng.FullParams * n)(p, p), ptrs, ns, n, 0, None, None, None, None, None, None, res) == 0, c.last_error()
        null_array = [eng._result_to_dict(res[i]) for i in range(n)]
        for i in range(n):
            L.skw_result_free(C.byref(res[i]))
        plain = c.full_batch(clips, [p, p])
        assert all(same(a, b) and a["token_times"] == b["token_times"] for a, b in zip(null_entries, base)) and all(same(a, b) for a, b in zip(null_array, plain))
        assert L.skw_debug_grammar_uploads(c.h) == 0                                              # nothing was allocated for grammars: no vocabulary image, no table
        # with one: the kernel runs once per sampler launch, the eager profiled steps give what the step graphs give, and equal tables are one upload — across calls too
        g1 = gl.to_engine(gram("yesno")); g2 = gl.to_engine(gl.compile_py(gl.TEST_PATTERNS["yesno"], penalty=gl.TEST_PENALTY))
        pg = engine_params(c)
        c.profile(True)
        a = c.full_batch(clips, pg, grammars=[g1, g2])
        prof = c.profile_get()
        c.profile(False)
        assert prof["k_dec_grammar"]["count"] > 0 and prof["k_dec_grammar"]["count"] == prof["k_dec_sample"]["count"]
        assert L.skw_debug_grammar_uploads(c.h) == 2                                              # the vocabulary image and ONE table
        b = c.full_batch(clips, pg, grammars=[g2, g1])
        assert all(same(x, y) for x, y in zip(a, b)) and L.skw_debug_grammar_uploads(c.h) == 2
        for k in range(10):      # more tables than the cache keeps: the oldest leave, the results stay right
            c.full_batch(clips[:1], pg, grammars=[gl.to_engine(gl.letters_table(3 + k))])
        assert L.skw_debug_grammar_uploads(c.h) == 12
        again = c.full_batch(clips, pg, grammars=[g1, g2])
        assert all(same(x, y) for x, y in zip(a, again)) and L.skw_debug_grammar_uploads(c.h) == 13
    finally:
        c.close()


# ---- 5. a clip with a grammar decodes the same alone, beside clips without one, and beside clips with other grammars
def test_batch_invariance(eng, ctx):
    p = engine_params(ctx)
    g = {n: gl.to_engine(gram(n)) for n in NAMES}
    alone = ctx.full_batch([clip(3)], p, grammars=[g["words"]])[0]
    beside_none = ctx.full_batch([clip(0), clip(3), clip(5)], p, grammars=[None, g["words"], None])
    beside_others = ctx.full_batch([clip(0), clip(3), clip(5), clip(3)], p, grammars=[g["digits"], g["words"], g["yesno"], gl.to_engine(gl.letters_table(129))])
    assert same(alone, beside_none[1]) and same(alone, beside_others[1])
    plain = ctx.full_batch([clip(0), clip(5)], p)
    assert same(plain[0], beside_none[0]) and same(plain[1], beside_none[2])      # and the clips without one are the call's without any
    assert RX["words"].fullmatch(text_of(alone)) and RX["digits"].fullmatch(text_of(beside_others[0])) and not same(alone, beside_others[3])


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


def test_node_grammar_parameters(eng, ctx, micro_model_path):
    from streamkit_amd import minihost
    plugin = minihost.Plugin()
    pcm = clip(3)[:16000]      # 1 s: one window, so the whole transcript is one match (with timestamps on, a longer clip takes several windows and the match restarts in each)
    cfg = dict(model_path=micro_model_path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=300, max_batch=8)
    digits = dict(grammar=gl.TEST_PATTERNS["digits"], grammar_penalty=gl.TEST_PENALTY)
    choices = dict(grammar_choices=["yes", "no", "may.be"], grammar_penalty=gl.TEST_PENALTY, grammar_ignore_case=True)
    rx_choices = re.compile(rb" ?(yes|no|may\.be)[.!?]?", re.IGNORECASE)
    # what the engine gives for each alone (the node's parameters: English, both suppress_* rules, the ladder and timestamps on)
    p = ctx.default_params(); p.lang_id = 0; p.suppress_blank = 1; p.suppress_nst = 1
    want_plain = ctx.full_batch([pcm], p)[0]
    want_digits = ctx.full_batch([pcm], p, grammars=[eng.Grammar.compile(gl.TEST_PATTERNS["digits"], penalty=gl.TEST_PENALTY)])[0]
    want_choices = ctx.full_batch([pcm], p, grammars=[eng.Grammar.compile(r" ?(yes|no|may\.be)[.!?]?", ignore_case=True, penalty=gl.TEST_PENALTY)])[0]
    assert _node_segments(want_plain) and _node_segments(want_digits) and _node_segments(want_choices)
    joined = lambda segs: "".join(s["text"] for s in segs).encode()
    assert want_plain["n_windows"] == 1 and want_digits["n_windows"] == 1 and want_choices["n_windows"] == 1
    assert RX["digits"].fullmatch(joined(_node_segments(want_digits))), _node_segments(want_digits)
    assert rx_choices.fullmatch(joined(_node_segments(want_choices))), _node_segments(want_choices)
    assert not RX["digits"].fullmatch(joined(_node_segments(want_plain))) and not rx_choices.fullmatch(joined(_node_segments(want_plain)))
    out = lambda nd, k0=0: [json.loads(o[2].decode()) for o in nd.outputs()][k0:]
    # instances with and without grammars share one engine call
    nodes = [plugin.create_node(dict(cfg, **digits)), plugin.create_node(dict(cfg)), plugin.create_node(dict(cfg, **choices))]
    before = minihost.whisper_batch_stats()
    assert _feed_and_flush_together(nodes, [pcm, pcm, pcm]) == [0, 0, 0], [n.last_error() for n in nodes]
    calls, jobs, _ = (a - b for a, b in zip(minihost.whisper_batch_stats(), before))
    assert (calls, jobs) == (1, 3)
    for nd, want in zip(nodes, (want_digits, want_plain, want_choices)):
        assert len(out(nd)) == 1 and out(nd)[0]["segments"] == _node_segments(want)
    assert RX["digits"].fullmatch(joined(out(nodes[0])[0]["segments"])) and rx_choices.fullmatch(joined(out(nodes[2])[0]["segments"]))      # through the plugin ABI
    # update_params switches the grammar for the next segment (the stream's clock ran on: texts are compared)
    assert nodes[1].update_params(dict(cfg, **digits)) == 0, nodes[1].last_error()
    _feed(nodes[1], pcm)
    assert nodes[1].flush() == 0, nodes[1].last_error()
    nxt = out(nodes[1], 1)
    assert len(nxt) == 1 and [s["text"] for s in nxt[0]["segments"]] == [s["text"] for s in _node_segments(want_digits)]
    # ... and a bad one is refused with the compiler's message, the instance keeps what it had
    assert nodes[1].update_params(dict(cfg, grammar="[0-9")) != 0 and "grammar: unbalanced '['" in nodes[1].last_error()
    for nd in nodes:
        nd.destroy()
    for bad, what in ((dict(grammar="(yes|no"), "grammar: unbalanced '('"), (dict(grammar="yes", grammar_choices=["no"]), "cannot both"), (dict(grammar="a{2000}"), "repetition count"),
                      (dict(grammar_choices=["yes", 3]), "grammar_choices"), (dict(grammar="yes", grammar_penalty=0), "grammar_penalty"), (dict(grammar="yes", grammar_ignore_case=1), "grammar_ignore_case")):
        with pytest.raises(RuntimeError, match=re.escape(what)):
            plugin.create_node(dict(cfg, **bad))
