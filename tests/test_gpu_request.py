"""skw_full_batch_request against the entry points it stands behind (include/skw_engine.h): every legacy entry, called directly through ctypes, and the request with the same
fields set give identical bytes — tokens (floats as bit patterns), segments, text, counters, the generator states and contexts after the call, token times, trace records — and
the same launches per kernel class.  Both forms of the launch are exercised and told apart; what no entry offers is refused before anything runs.  Micro model, one context of
two rows, clips of 1 s and 2 s."""
import ctypes as C

import numpy as np
import pytest

from streamkit_amd import engine, synth

pytestmark = pytest.mark.gpu
N = 2
TEXT = [[300, 301, 302], [310, 311, 312]]      # forced alignment: 3 text tokens per clip


@pytest.fixture(scope="module")
def rig(micro_model_path):
    m = engine.Model(micro_model_path); ctx = engine.Context(m, max_batch=N, max_samples=16000 * 3)
    pcms = [synth.clip(3, 16000), synth.clip(5, 32000)]
    a = ctx.default_params(); a.lang_id = engine.lib().skw_model_lang_id(b"en"); a.suppress_blank = 1
    b = ctx.default_params(); b.lang_id = engine.lib().skw_model_lang_id(b"de"); b.suppress_blank = 0; b.temperature = 0.6      # (sampled from the first pass on: generators move)
    assert a.lang_id != b.lang_id and a.lang_id >= 0 and b.lang_id >= 0
    yield dict(m=m, ctx=ctx, h=ctx.h, pcms=pcms, a=a, b=b,
               pcm=engine._ptr_array(pcms, lambda c: c.ctypes.data), ns=(C.c_int32 * N)(*[c.size for c in pcms]),
               rules=[engine.DecodeRules(repetition_penalty=1.3, no_repeat_ngram_size=2), None], grammars=[None, engine.Grammar.compile("[a-z ,.]*", penalty=5.0)],
               align=[engine.align_params(top=1, hp=m.hp), engine.align_params(top=1, hp=m.hp)], text=[np.array(t, np.int32) for t in TEXT])
    ctx.close(); m.close()


class IO:
    """one call's arguments: the inputs shared, everything a call writes fresh — so that the legacy entry and the request start from identical bytes"""

    def __init__(self, rig, params, feats):
        self.rig = rig
        self.per_clip = isinstance(params, list)
        self.params = (engine.FullParams * N)(*params) if self.per_clip else params
        self.res = (engine.Result * N)()
        has = lambda k: k in feats
        self.rng = [engine.rng_state_new() for _ in range(N)] if has("rng") else None
        self.rng_p = engine._ptr_array(self.rng, lambda s: s.ctypes.data) if self.rng else None
        self.cx = [engine.context_new([300, 301, 302]), engine.context_new()] if has("context") else None
        self.cx_p = engine._ptr_array(self.cx, lambda x: x.ctypes.data) if self.cx else None
        self.rules_p = engine.rules_array(rig["rules"], N, rig["m"].hp.n_vocab, "clip")[1] if has("rules") else None
        self.align_p = engine._ptr_array(rig["align"] if has("text") else [rig["align"][0], None], C.addressof) if has("align") or has("text") else None
        self.times = (engine.TokenTimes * N)() if self.align_p is not None else None
        self.gram_p = engine.grammars_array(rig["grammars"], N, "clip") if has("grammar") else None
        self.text_p = engine._ptr_array(rig["text"], lambda t: t.ctypes.data) if has("text") else None
        self.n_text = (C.c_int32 * N)(*[t.size for t in rig["text"]]) if has("text") else None
        self.traces = (engine.Trace * N)() if has("traces") else None
        self.forced = feats.get("forced")
        self.forced_p = engine._ptr_array(self.forced, lambda f: f.ctypes.data) if self.forced else None
        self.n_forced = (C.c_int32 * N)(*[f.size for f in self.forced]) if self.forced else None

    def request(self, **over):
        r = self.rig
        rq = engine.FullRequest(size=C.sizeof(engine.FullRequest), params_per_clip=1 if self.per_clip else 0, params=self.params if self.per_clip else C.pointer(self.params),
                                pcm=r["pcm"], n_samples=r["ns"], n_clips=N, pcm_on_device=0, results=None if self.text_p is not None else self.res)
        for k, v in dict(rng_state=self.rng_p, context=self.cx_p, rules=self.rules_p, align=self.align_p, times=self.times, grammar=self.gram_p, text_tokens=self.text_p,
                         n_text=self.n_text, traces=self.traces, forced_ids=self.forced_p, n_forced=self.n_forced).items():
            if v is not None:
                setattr(rq, k, v)
        for k, v in over.items():
            setattr(rq, k, v)
        return rq

    def legacy_args(self, name):
        r = self.rig; p = self.params if self.per_clip else C.byref(self.params)
        head = [r["h"], p, r["pcm"], r["ns"], N, 0]
        tail = dict(skw_full_batch=[], skw_full_batch_rng=[self.rng_p], skw_full_batch_mixed=[self.rng_p], skw_full_batch_context=[self.rng_p, self.cx_p],
                    skw_full_batch_rules=[self.rng_p, self.cx_p, self.rules_p], skw_full_batch_aligned=[self.rng_p, self.cx_p, self.rules_p, self.align_p, self.times],
                    skw_full_batch_grammar=[self.rng_p, self.cx_p, self.rules_p, self.align_p, self.times, self.gram_p],
                    skw_full_batch_traced=[self.forced_p, self.n_forced, self.traces], skw_full_batch_traced_context=[self.forced_p, self.n_forced, self.traces, self.cx_p])[name] \
            if name != "skw_align_batch" else [self.text_p, self.n_text, self.align_p, self.times]
        return head + tail + ([] if name == "skw_align_batch" else [self.res])

    def state(self):
        """the bytes a refused call must leave alone"""
        return [s.tobytes() for s in self.rng or []] + [x.tobytes() for x in self.cx or []]

    def observe(self):
        """everything the call wrote, as bytes; releases what the library allocated"""
        L = engine.lib(); out = dict(state=self.state())
        if self.text_p is None:
            out["results"] = []
            for r in self.res:
                out["results"].append((r.n_segments, r.n_tokens, r.n_windows, r.n_decode_steps, r.fallback_requested, np.float32(r.min_margin).tobytes(), r.text_len, r.lang_id,
                                       C.string_at(r.tokens, r.n_tokens * C.sizeof(engine.Token)), C.string_at(r.segments, r.n_segments * C.sizeof(engine.Segment)),
                                       C.string_at(r.text, r.text_len)))
                L.skw_result_free(C.byref(r))
        if self.times is not None:
            out["times"] = [(t.n, C.string_at(t.t0, 8 * t.n), C.string_at(t.t1, 8 * t.n)) for t in self.times]
            for t in self.times:
                L.skw_token_times_free(C.byref(t))
        if self.traces is not None:
            out["traces"] = [(t.n, C.string_at(t.steps, t.n * engine.TRACE_DT.itemsize)) for t in self.traces]
            for t in self.traces:
                L.skw_trace_free(C.byref(t))
        return out


def counts(ctx):
    return {k: v["count"] for k, v in ctx.profile_get().items()}


def run(rig, call):
    """-> (what profile_get counted for this call alone, the return code)"""
    rig["ctx"].profile(True)
    rc = call()
    return counts(rig["ctx"]), rc


def both(rig, name, params, feats):
    """the legacy entry `name`, then the request with the same fields: -> (legacy observation, request observation), asserted equal with equal launch counts"""
    L = engine.lib()
    a = IO(rig, params, feats); ca, rc = run(rig, lambda: getattr(L, name)(*a.legacy_args(name)))
    assert rc == 0, rig["ctx"].last_error()
    oa = a.observe()
    b = IO(rig, params, feats); rq = b.request(); cb, rc = run(rig, lambda: L.skw_full_batch_request(rig["h"], C.byref(rq)))
    assert rc == 0, rig["ctx"].last_error()
    ob = b.observe()
    assert oa == ob, name
    assert ca == cb and sum(ca.values()) > 0, name
    return oa, ob, rq


ALL = ("rng", "context", "rules", "align", "grammar")
CASES = [("skw_full_batch", "b", ()), ("skw_full_batch_rng", "b", ("rng",)), ("skw_full_batch_mixed", "ab", ("rng",)), ("skw_full_batch_context", "ab", ALL[:2]),
         ("skw_full_batch_rules", "ab", ALL[:3]), ("skw_full_batch_aligned", "ab", ALL[:4]), ("skw_full_batch_grammar", "ab", ALL), ("skw_full_batch_traced", "a", ("traces",)),
         ("skw_align_batch", "ab", ("text",))]


@pytest.mark.parametrize("name,blocks,feats", CASES, ids=[c[0] for c in CASES])
def test_each_legacy_entry_is_the_request_with_its_fields_set(rig, name, blocks, feats):
    params = rig[blocks] if len(blocks) == 1 else [rig[k] for k in blocks]
    o, _, rq = both(rig, name, params, dict.fromkeys(feats))
    assert rq.params_per_clip == (1 if len(blocks) == 2 else 0)
    if "results" in o:
        assert all(r[1] > 0 for r in o["results"])      # every clip decoded something
    if "rng" in feats:
        fresh = engine.rng_state_new().tobytes()
        assert any(s != fresh for s in o["state"][:N])      # the generators moved: what comes back is not what went in
    if "context" in feats:
        assert o["state"][N:] != [engine.context_new([300, 301, 302]).tobytes(), engine.context_new().tobytes()]
    if "align" in feats:
        assert o["times"][0][0] == o["results"][0][1] and o["times"][1][0] == o["results"][1][1]
    if "text" in feats:
        assert [t[0] for t in o["times"]] == [3, 3] and "results" not in o
    if "traces" in feats:
        assert all(t[0] > 0 for t in o["traces"])


def test_a_teacher_forced_traced_call_with_a_carried_context(rig):
    free, _, _ = both(rig, "skw_full_batch_traced_context", rig["a"], dict(traces=None, context=None))
    ids = [np.ascontiguousarray(np.frombuffer(t[1], dtype=engine.TRACE_DT)["chosen_id"], dtype=np.int32) for t in free["traces"]]
    forced, _, _ = both(rig, "skw_full_batch_traced_context", rig["a"], dict(traces=None, context=None, forced=ids))
    assert forced == free      # the same precision fed its own decisions: the same run, contexts handed back included
    assert forced["state"] != [engine.context_new([300, 301, 302]).tobytes(), engine.context_new().tobytes()]


def test_the_two_forms_are_both_exercised_and_not_confused(rig):
    """uniform: every clip under params[0], whatever stands behind it; per clip: each under its own.  Equal blocks give equal results in both forms, through different kernels."""
    L = engine.lib(); ba = [rig["b"], rig["a"]]
    uni, _, rq_u = both(rig, "skw_full_batch_rng", rig["b"], dict(rng=None))
    eq, _, rq_e = both(rig, "skw_full_batch_mixed", [rig["b"], rig["b"]], dict(rng=None))
    mix, _, rq_m = both(rig, "skw_full_batch_mixed", ba, dict(rng=None))
    assert (rq_u.params_per_clip, rq_e.params_per_clip, rq_m.params_per_clip) == (0, 1, 1)
    assert eq == uni      # (an array whose entries are all equal gives exactly what skw_full_batch_rng gives)
    io = IO(rig, ba, dict(rng=None)); rq = io.request(params_per_clip=0)      # the array handed to the uniform form: only its first block counts
    assert L.skw_full_batch_request(rig["h"], C.byref(rq)) == 0, rig["ctx"].last_error()
    first = io.observe()
    assert first == uni and first != mix and mix["results"][0] == uni["results"][0] and mix["results"][1] != uni["results"][1]
    # the sampler's own two forms through the hook's request: the launcher picks another kernel
    NV = rig["m"].hp.n_vocab; lg = np.random.default_rng(7).standard_normal((N, NV)).astype(np.float32)
    k_uni = rig["ctx"].sample_rows([[], []], lg, params=rig["a"], extras=True)
    k_row = rig["ctx"].sample_rows([[], []], lg, params=[rig["a"], rig["a"]], extras=True)
    assert k_uni[3]["kernel"] != k_row[3]["kernel"] and k_row[3]["kernel"].endswith("true>") and k_uni[3]["kernel"].endswith("false>")
    assert k_uni[0].tobytes() == k_row[0].tobytes()


def test_the_sampler_hooks_are_the_request_with_their_fields_set(rig):
    L = engine.lib(); NV = rig["m"].hp.n_vocab; lg = np.random.default_rng(11).standard_normal((N, NV)).astype(np.float32)
    hist = np.array([[300, 301], [302, 0]], np.int32); nh = np.array([2, 1], np.int32)
    pp = (engine.FullParams * N)(rig["a"], rig["b"]); rules_p = engine.rules_array(rig["rules"], N, NV, "row")[1]
    out = []
    for use_request in (False, True):
        tok = np.zeros(N, engine._TOKEN_DT); tr = np.zeros(N, engine.TRACE_DT)
        if use_request:
            rq = engine.SampleRowsRequest(params_per_row=1, n_rows=N, params=pp, hist=hist.ctypes.data, hist_stride=2, form=0, n_hist=nh.ctypes.data, logits=lg.ctypes.data,
                                          tok_out=tok.ctypes.data, trace_out=tr.ctypes.data, rules=rules_p, trace=1)
            rc = L.skw_debug_sample_rows_request(rig["h"], C.byref(rq))
        else:
            rc = L.skw_debug_sample_rows_rules(rig["h"], pp, N, hist.ctypes.data, 2, nh.ctypes.data, lg.ctypes.data, 0, None, tok.ctypes.data, tr.ctypes.data, rules_p)
        assert rc == 0, rig["ctx"].last_error()
        out.append((tok.tobytes(), tr.tobytes()))
    assert out[0] == out[1] and out[0][0] != np.zeros(N, engine._TOKEN_DT).tobytes()


def _refused(rig, io, call):
    ctx = rig["ctx"]; before = io.state(); ctx.profile(True)
    L = engine.lib(); p = C.byref(rig["a"])      # one accepted call, so that the counters stand at something a launch would move
    res = (engine.Result * N)()
    assert L.skw_full_batch(rig["h"], p, rig["pcm"], rig["ns"], N, 0, res) == 0
    for r in res:
        L.skw_result_free(C.byref(r))
    c0 = counts(ctx); assert sum(c0.values()) > 0
    rc = call()
    assert rc != 0 and ctx.last_error() != ""
    assert io.state() == before and counts(ctx) == c0
    return rc, ctx.last_error()


REFUSED = [("traces", k) for k in ("params_per_clip", "rng", "rules", "align", "grammar")] + [("text", k) for k in ("rng", "context", "rules", "grammar", "traces")]


@pytest.mark.parametrize("base,extra", REFUSED, ids=["%s+%s" % c for c in REFUSED])
def test_combinations_no_entry_offers_are_refused_before_anything_runs(rig, base, extra):
    per_clip = base == "text" or extra == "params_per_clip"
    # (a traced call may carry contexts: they go in, so that there is a context to find untouched)
    io = IO(rig, [rig["a"], rig["b"]] if per_clip else rig["a"], dict.fromkeys([base, extra] + (["context"] if base == "traces" else [])))
    rq = io.request(results=io.res)
    rc, msg = _refused(rig, io, lambda: engine.lib().skw_full_batch_request(rig["h"], C.byref(rq)))
    assert rc == -3, msg
    assert all(t.n == 0 and not t.steps for t in io.traces or [])      # zeroed before the check: defined after the failed call


def test_forced_ids_need_their_lengths_and_the_traces(rig):
    ids = [np.array([1, 2, 3], np.int32)] * N
    for drop in ("n_forced", "traces"):
        io = IO(rig, rig["a"], dict(traces=None, forced=ids, context=None)); rq = io.request()
        setattr(rq, drop, None)
        rc, msg = _refused(rig, io, lambda: engine.lib().skw_full_batch_request(rig["h"], C.byref(rq)))
        assert rc == -3 and "forced_ids" in msg, msg


@pytest.mark.parametrize("size", [engine.FULL_REQUEST_MIN - 1, 0, C.sizeof(engine.FullRequest) + 8], ids=["one_below_min", "zero", "above_sizeof"])
def test_a_size_the_library_cannot_read_is_refused(rig, size):
    io = IO(rig, [rig["a"], rig["b"]], dict(rng=None, context=None)); rq = io.request(size=size)
    rc, msg = _refused(rig, io, lambda: engine.lib().skw_full_batch_request(rig["h"], C.byref(rq)))
    assert rc == -1 and "size %d" % size in msg, msg


def test_the_hook_refuses_the_ex_fields_with_rules(rig):
    NV = rig["m"].hp.n_vocab; lg = np.zeros((N, NV), np.float32); nh = np.zeros(N, np.int32); hist = np.zeros((N, 1), np.int32)
    io = IO(rig, rig["a"], dict(rng=None, context=None)); t = np.zeros(N, np.float32); tok = np.zeros(N, engine._TOKEN_DT)
    pp = (engine.FullParams * N)(rig["a"], rig["a"])
    rq = engine.SampleRowsRequest(params_per_row=1, n_rows=N, params=pp, hist=hist.ctypes.data, hist_stride=1, form=0, n_hist=nh.ctypes.data, logits=lg.ctypes.data,
                                  tok_out=tok.ctypes.data, rules=engine.rules_array(rig["rules"], N, NV, "row")[1], trace=1, temperature=t.ctypes.data)
    rc, msg = _refused(rig, io, lambda: engine.lib().skw_debug_sample_rows_request(rig["h"], C.byref(rq)))
    assert rc == -3 and "rules" in msg, msg
    assert tok.tobytes() == np.zeros(N, engine._TOKEN_DT).tobytes()
