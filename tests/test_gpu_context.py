"""Initial prompts and carried context on the GPU (skw_full_batch_context): the exact precision against the checker composed from the oracle (tests/context_ref_lib.py), carried
calls, mixed batches, the refusals, the prompt pass's two cross-attention kernels, the f16_mfma precision under teacher forcing, and the Whisper node.

Tiny synthetic model; the checker's results are computed once per (clip, context) and shared."""
import ctypes as C
import json

import numpy as np
import pytest

import context_ref_lib as cr
import logit_rules_lib as lr
from conftest import quantized_model

pytestmark = pytest.mark.gpu
CLIPS = {"c5": (5, 9 * 16000), "c21": (21, 3 * 16000), "c13": (13, 47 * 16000 + 123)}
MAX_SAMPLES = 47 * 16000 + 1024
_REF = {}
_PCM = {}


def clip(name):
    if name not in _PCM:
        from streamkit_amd import synth
        seed, n = CLIPS[name]
        _PCM[name] = synth.clip(seed, n_samples=n); _PCM[name].setflags(write=False)
    return _PCM[name]


def context_of(om, n):
    """the seeded context of n tokens; the three shorter ones carry timestamp ids"""
    if n == 0:
        return []
    sp = lr.special_ids(om)
    c = cr.make_context(np.random.default_rng(100 + n), sp, n, with_timestamps=n != 300)
    if n == 1:
        c = [sp["beg"] + 75]
    assert n == 300 or any(t >= sp["beg"] for t in c)
    return c


def checker(om, name, context):
    key = (name, tuple(context))
    if key not in _REF:
        _REF[key] = cr.full_with_context(om, clip(name), context, cr.params_for(om))
    return _REF[key]


def engine_params(ctx, **kw):
    p = ctx.default_params()
    p.temperature_inc = 0.0; p.no_speech_thold = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def same(a, b):
    """two engine results, bit for bit"""
    return (cr.token_bits(a["tokens"]) == cr.token_bits(b["tokens"]) and a["segments"] == b["segments"] and a["n_windows"] == b["n_windows"]
            and a["lang_id"] == b["lang_id"] and a["fallback_requested"] == b["fallback_requested"])


def assert_equals_checker(got, ref, what):
    assert cr.token_bits(got["tokens"]) == cr.token_bits(ref["tokens"]), what
    assert [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in got["segments"]] == [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in ref["segments"]], what
    assert got["n_windows"] == ref["n_windows"], what


@pytest.fixture(scope="module")
def gm(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ctx(gm):
    from streamkit_amd import engine
    c = engine.Context(gm, max_batch=6, max_samples=MAX_SAMPLES)
    yield c
    c.close()


@pytest.mark.parametrize("n_ctx_tokens", [0, 1, 40, 300])
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_engine_equals_checker(eng, ctx, oracle_tiny, name, n_ctx_tokens):
    context = context_of(oracle_tiny, n_ctx_tokens)
    ref = checker(oracle_tiny, name, context)
    cx = eng.context_new(context)
    got = ctx.full_batch([clip(name)], engine_params(ctx), contexts=[cx])[0]
    assert_equals_checker(got, ref, (name, n_ctx_tokens))
    assert eng.context_ids(cx) == ref["context"]
    if n_ctx_tokens:      # the context did something (tests/test_cpu_context.py shows the same for the checker alone)
        assert [t[0] for t in got["tokens"]] != [t[0] for t in checker(oracle_tiny, name, [])["tokens"]]
    if n_ctx_tokens == 300:      # more than n_text_ctx / 2 handed in: the newest 224 were taken and are what comes back in front of the window's tokens
        assert ref["context"][:224] == context[-224:]


def test_two_calls_carried(eng, ctx, oracle_tiny):
    r1 = checker(oracle_tiny, "c5", context_of(oracle_tiny, 40))
    r2 = checker(oracle_tiny, "c21", r1["context"])
    cx = eng.context_new(context_of(oracle_tiny, 40))
    g1 = ctx.full_batch([clip("c5")], engine_params(ctx), contexts=[cx])[0]
    assert eng.context_ids(cx) == r1["context"]
    g2 = ctx.full_batch([clip("c21")], engine_params(ctx), contexts=[cx])[0]
    assert_equals_checker(g1, r1, "first call"); assert_equals_checker(g2, r2, "second call")
    assert eng.context_ids(cx) == r2["context"]
    assert [t[0] for t in g2["tokens"]] != [t[0] for t in checker(oracle_tiny, "c21", [])["tokens"]]


def _mixed_rows(eng, ctx, om):
    names = ["c5", "c21", "c13", "c21", "c5", "c21"]
    params = [engine_params(ctx), engine_params(ctx, lang_id=2), engine_params(ctx), engine_params(ctx, audio_ctx=256), engine_params(ctx, lang_id=7, suppress_nst=0), engine_params(ctx)]
    contexts = [None, context_of(om, 300), [], context_of(om, 40), context_of(om, 1), None]
    return names, params, contexts


def test_mixed_batch_equals_each_row_alone(eng, ctx, oracle_tiny):
    names, params, contexts = _mixed_rows(eng, ctx, oracle_tiny)
    mk = lambda: [None if c is None else eng.context_new(c) for c in contexts]
    cb = mk()
    batch = ctx.full_batch([clip(n) for n in names], params, contexts=cb)
    for i, n in enumerate(names):
        ca = mk()[i]
        alone = ctx.full_batch([clip(n)], [params[i]], contexts=[ca])[0]
        assert same(batch[i], alone), i
        assert (cb[i] is None and ca is None) or np.array_equal(cb[i], ca), i
    assert not same(batch[1], batch[5]) and not same(batch[0], batch[4])      # the rows' own contexts and languages told them apart


def test_null_context_is_the_mixed_call(eng, ctx, oracle_tiny):
    names, params, _ = _mixed_rows(eng, ctx, oracle_tiny)
    clips = [clip(n) for n in names]
    want = ctx.full_batch(clips, params)                                    # skw_full_batch_mixed
    got = ctx.full_batch(clips, params, contexts=[None] * len(names))      # NULL entries
    assert all(same(a, b) for a, b in zip(want, got))
    # a NULL array, through the C entry point itself
    n = len(names)
    keep = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
    res = (eng.Result * n)()
    rc = eng.lib().skw_full_batch_context(ctx.h, (eng.FullParams * n)(*params), (C.c_void_p * n)(*[k.ctypes.data for k in keep]), (C.c_int32 * n)(*[k.size for k in keep]), n, 0,
                                          None, None, res)
    assert rc == 0, ctx.last_error()
    got2 = [eng._result_to_dict(res[i]) for i in range(n)]
    for i in range(n):
        eng.lib().skw_result_free(C.byref(res[i]))
    assert all(same(a, b) for a, b in zip(want, got2))


def test_bad_contexts_are_refused_and_nothing_is_written(eng, ctx, oracle_tiny):
    good = eng.context_new(context_of(oracle_tiny, 40))
    for bad_words, needle in (([513, 1, 2], "clip 1"), ([-1], "clip 1"), ([2, 5, ctx.model.hp.n_vocab], "clip 1"), ([1, -3], "clip 1")):
        bad = np.zeros(eng.CONTEXT_WORDS, np.int32); bad[:len(bad_words)] = bad_words
        a, b = good.copy(), bad.copy()
        with pytest.raises(RuntimeError) as e:
            ctx.full_batch([clip("c21"), clip("c21")], engine_params(ctx), contexts=[a, b])
        assert needle in str(e.value) and "context" in str(e.value), str(e.value)
        assert np.array_equal(a, good) and np.array_equal(b, bad)
    # a clip too short to transcribe returns its context unchanged
    a = good.copy()
    r = ctx.full_batch([np.zeros(800, np.float32)], engine_params(ctx), contexts=[a])[0]
    assert r["n_windows"] == 0 and np.array_equal(a, good)


@pytest.mark.parametrize("quant", [None, "q8_0"])
def test_stepped_prompt_and_single_query_kernel_give_the_same_bits(eng, ctx, oracle_tiny, tiny_model_path, quant):
    if quant:
        m = eng.Model(quantized_model("tiny", quant)); c = eng.Context(m, max_batch=3, max_samples=MAX_SAMPLES)
        assert m.quant == 8
    else:
        m, c = None, ctx
    try:
        names = ["c21", "c5", "c21"]
        contexts = [context_of(oracle_tiny, 300), context_of(oracle_tiny, 40), context_of(oracle_tiny, 1)]
        params = [engine_params(c), engine_params(c), engine_params(c, audio_ctx=200)]
        runs = {}
        for mode, (pp, mq) in dict(default=(1, 1), single_query=(1, 0), stepped=(0, 1)).items():
            c.set_prompt_pass(pp); c.set_prompt_xattn_mq(mq)
            cx = [eng.context_new(x) for x in contexts]
            runs[mode] = (c.full_batch([clip(n) for n in names], params, contexts=cx), cx)
        c.set_prompt_pass(1); c.set_prompt_xattn_mq(1)
        for mode in ("single_query", "stepped"):
            assert all(same(a, b) for a, b in zip(runs["default"][0], runs[mode][0])), mode
            assert all(np.array_equal(a, b) for a, b in zip(runs["default"][1], runs[mode][1])), mode
        assert sum(len(r["tokens"]) for r in runs["default"][0]) > 0
    finally:
        if m is not None:
            c.close(); m.close()


def test_f16_mfma_with_contexts_stays_inside_the_parity_bounds(eng, ctx, oracle_tiny):
    from streamkit_amd.parity import bounds_for, teacher_forced_compare
    names = ["c5", "c21", "c13"]
    cx = [eng.context_new(context_of(oracle_tiny, n)) for n in (40, 300, 1)]
    before = [x.copy() for x in cx]
    tf = teacher_forced_compare(ctx, [clip(n) for n in names], engine_params(ctx), contexts=cx)
    eb, mb = bounds_for(ctx.model.hp)
    print("f16_mfma with contexts: %d decisions, %d differ, max logit err %.4f (bound %.2f), max margin at a disagreement %s (bound %.2f)"
          % (tf["steps_checked"], tf["argmax_disagreements"], tf["max_logit_err"], eb, tf["max_margin_at_disagreement"], mb))
    assert tf["logit_err_bound"] == eb and tf["margin_bound"] == mb
    assert tf["ok"], {k: tf[k] for k in ("argmax_disagreements", "max_margin_at_disagreement", "max_logit_err")}
    assert tf["steps_checked"] > 0 and all(np.array_equal(a, b) for a, b in zip(cx, before))
    # the exact run of the pair is the engine == checker run
    assert_equals_checker(tf["results_exact"][0], checker(oracle_tiny, "c5", context_of(oracle_tiny, 40)), "exact run under tracing")
    assert eng.context_ids(tf["contexts_exact"][0]) == checker(oracle_tiny, "c5", context_of(oracle_tiny, 40))["context"]


# ---- the Whisper node
SEG = 512 * 160      # two segments of 5.12 s: whole VAD frames, handed over by a flush each


def _context_calls():
    import os
    from streamkit_amd import minihost
    L = C.CDLL(os.path.join(minihost.ROOT, "streamkit_amd", "libwhisper.so"))
    L.skw_whisper_plugin_context_stats.argtypes = [C.POINTER(C.c_long)]; L.skw_whisper_plugin_context_stats.restype = None
    n = C.c_long(); L.skw_whisper_plugin_context_stats(C.byref(n))
    return n.value


def _node_transcripts(model_path, pcms, **params):
    from streamkit_amd import minihost
    node = minihost.Plugin().create_node(dict(model_path=model_path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=0, max_batch=2, **params))
    try:
        for pcm in pcms:
            for i in range(0, pcm.size, 960):
                assert node.process_audio(pcm[i:i + 960]) == 0, node.last_error()
            assert node.flush() == 0, node.last_error()
        out = [json.loads(payload.decode()) for (_, typ, payload) in node.outputs() if typ == 3]
        return [[s["text"] for s in o["segments"]] for o in out], node.logs()
    finally:
        node.destroy()


def _texts(result):
    return [t for t in (s["text"].decode().strip() for s in result["segments"]) if t]


def test_node_carries_context_and_prepends_the_prompt(eng, gm, tiny_model_path):
    from streamkit_amd import minihost, synth
    pcms = [synth.clip(5, n_samples=SEG), synth.clip(21, n_samples=SEG)]
    c = eng.Context(gm, max_batch=2, max_samples=31 * 16000 + 1024)
    try:
        p = c.default_params()      # the node's request: the defaults, language "en", both suppress_* rules on
        p.lang_id = 0; p.suppress_blank = 1; p.suppress_nst = 1
        # neither parameter: today's calls and today's transcripts
        calls0, ctx_calls0 = minihost.whisper_batch_stats(), _context_calls()
        got, _ = _node_transcripts(tiny_model_path, pcms)
        calls1 = minihost.whisper_batch_stats()
        rng = eng.rng_state_new()
        plain = [c.full_batch([x], p, rng_states=[rng])[0] for x in pcms]
        assert got == [_texts(r) for r in plain] and all(got)
        assert (calls1[0] - calls0[0], calls1[1] - calls0[1], calls1[2] - calls0[2]) == (2, 2, 0) and _context_calls() == ctx_calls0
        # carry_context: the instance's second segment decodes behind what its first left
        got, _ = _node_transcripts(tiny_model_path, pcms, carry_context=True)
        rng = eng.rng_state_new(); cx = eng.context_new()
        carried = [c.full_batch([x], p, rng_states=[rng], contexts=[cx])[0] for x in pcms]
        assert got == [_texts(r) for r in carried]
        assert _texts(carried[1]) != _texts(plain[1]) and _texts(carried[0]) == _texts(plain[0])
        assert _context_calls() == ctx_calls0 + 2
        # initial_prompt without carry: one prepended context per segment
        prompt = " " + gm.token_bytes(2100).decode().strip() + " " + gm.token_bytes(2200).decode().strip() + ", ok"
        ids = gm.tokenize(prompt)
        assert len(ids) >= 3
        got, _ = _node_transcripts(tiny_model_path, pcms, initial_prompt=prompt)
        rng = eng.rng_state_new()
        prompted = [c.full_batch([x], p, rng_states=[rng], contexts=[eng.context_new(ids)])[0] for x in pcms]
        assert got == [_texts(r) for r in prompted] and _texts(prompted[0]) != _texts(plain[0])
        # both: the prompt goes in FRONT of what is carried
        got, _ = _node_transcripts(tiny_model_path, pcms, initial_prompt=prompt, carry_context=True)
        rng = eng.rng_state_new(); cx = eng.context_new(ids)
        r1 = c.full_batch([pcms[0]], p, rng_states=[rng], contexts=[cx])[0]
        cx = eng.context_new(ids + eng.context_ids(cx))
        r2 = c.full_batch([pcms[1]], p, rng_states=[rng], contexts=[cx])[0]
        assert got == [_texts(r1), _texts(r2)]
        # a prompt longer than half the text context keeps its end, with a warning
        long_prompt = " ".join(gm.token_bytes(2000 + i).decode().strip() for i in range(300))
        lids = gm.tokenize(long_prompt)
        assert len(lids) > 224
        got, logs = _node_transcripts(tiny_model_path, pcms[:1], initial_prompt=long_prompt)
        rl = c.full_batch([pcms[0]], p, contexts=[eng.context_new(lids[-224:])])[0]
        assert got == [_texts(rl)] and any("initial_prompt" in ln and "224" in ln for ln in logs)
    finally:
        c.close()
