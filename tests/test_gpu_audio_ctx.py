"""Per-clip audio context (skw_full_params.audio_ctx = K): every window of the clip is encoded and attended over K positions instead of n_audio_ctx.

The checker is the oracle as it stands, on a rewritten model file: M'(K) = the model with hparams.n_audio_ctx = K and the encoder's positional embedding cut to its first K rows
(tests/audio_ctx_lib.py).  In the exact precision the engine with audio_ctx = K on M equals the oracle on M'(K) bit for bit — conv stem, encoder output, cross K / V, logits,
tokens, log-probs, segment times, detected language.  The oracle is handed max_initial_ts x n_audio_ctx / K, so both sides ban the same timestamp ids (the helper asserts it).
K set: one key, under one tile, an exact 32-key block, ragged ends, one key short of full, full.  Micro model unless said; clips of 1.5 - 4 s; each case takes a second or two."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

from audio_ctx_lib import audio_ctx_model, scaled_max_initial_ts
from oracle_lib import OracleModel
from streamkit_amd import engine, minihost, synth
from streamkit_amd.parity import bounds_for, teacher_forced_compare

pytestmark = pytest.mark.gpu

KS = [1, 17, 32, 100, 129, 750, 1499, 1500]
NC = 1500
TOKS = [50258, 50259, 50359, 50364, 1234, 777]
_oracles = {}


def _oracle(path, K):
    """the oracle on M'(K) of the model file `path` (K = 0: the file itself), loaded once"""
    if (path, K) not in _oracles:
        _oracles[(path, K)] = OracleModel(audio_ctx_model(path, K) if 0 < K < NC else path)
    return _oracles[(path, K)]


def _params(ctx_or_oracle, **kw):
    p = ctx_or_oracle.default_params()
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _oracle_full(path, K, pcm, rng_state=None, **kw):
    om = _oracle(path, K); Ke = K if K > 0 else NC
    p = _params(om, **kw); p.max_initial_ts = scaled_max_initial_ts(p.max_initial_ts, NC, Ke)
    return om.full(pcm, p, rng_state=rng_state)


def _ids(r):
    return [t[0] for t in r["tokens"]]


def _same_as_oracle(g, o, what):
    assert _ids(g) == _ids(o), (what, _ids(g)[:12], _ids(o)[:12])
    assert [t[1] for t in g["tokens"]] == [t[1] for t in o["tokens"]], what
    assert [np.float32(t[3]).view(np.uint32) for t in g["tokens"]] == [np.float32(t[3]).view(np.uint32) for t in o["tokens"]], what      # plog, bit for bit
    assert [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in g["segments"]] == [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in o["segments"]], what
    assert g["n_windows"] == o["n_windows"] and g["lang_id"] == o["lang_id"] and g["fallback_requested"] == o["fallback_requested"], what


def _key(r):
    return ([tuple(np.float32(x).view(np.uint32) if isinstance(x, float) else x for x in t) for t in r["tokens"]], [(s["t0"], s["t1"], s["text"]) for s in r["segments"]],
            r["n_windows"], r["fallback_requested"], r["lang_id"], r["n_decode_steps"])


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def micro(eng, micro_model_path):
    m = eng.Model(micro_model_path); ctx = eng.Context(m, max_batch=8, max_samples=16000 * 36)
    yield micro_model_path, ctx
    ctx.close(); m.close()


# ------------------------------------------------------------------ 1. taps
@pytest.mark.parametrize("K", KS)
def test_taps_equal_the_oracle_on_the_rewritten_model(micro, K):
    path, ctx = micro; om = _oracle(path, K)
    ctx.set_precision("exact")
    pcm = synth.clip(7, 16000 * 3 + 777)
    mel, _ = om.log_mel(pcm)
    assert bits_equal(ctx.conv_stem(pcm, audio_ctx=K), om.conv_stem(mel)), "conv stem"
    enc_o, ck_o, cv_o = om.encode(mel)
    enc_g, ck_g, cv_g = ctx.encode(pcm, audio_ctx=K)
    assert enc_g.shape == (K, om.hp.n_audio_state)
    for name, a, b in (("enc_out", enc_g, enc_o), ("cross_k", ck_g, ck_o), ("cross_v", cv_g, cv_o)):
        assert bits_equal(a, b), name
    for n in (3, 6):      # skw_decode_logits follows the last encode's K
        assert bits_equal(ctx.decode_logits(TOKS[:n]), om.decoder(ck_o, cv_o).step(TOKS[:n], 0)), n
    # a later window of the same clip: seek > 0, the window runs out of audio inside its 2 K frames (or does not, for the small K)
    assert bits_equal(ctx.conv_stem(pcm, seek=100, audio_ctx=K), om.conv_stem(mel, 100)), "conv stem at seek 100"


# ------------------------------------------------------------------ 2. end to end
@pytest.mark.parametrize("K", KS)
def test_full_call_equals_the_oracle_on_the_rewritten_model(micro, K):
    path, ctx = micro
    ctx.set_precision("exact")
    pcm = synth.clip(9, 16000 * 4 - 321)
    g = ctx.full_batch([pcm], _params(ctx, audio_ctx=K))[0]
    _same_as_oracle(g, _oracle_full(path, K, pcm), K)
    assert len(g["tokens"]) > 0


def test_full_call_variants_equal_the_oracle(eng, micro):
    """language auto-detection (the row's K shapes the window it is detected from), no_timestamps, max_initial_ts switched off on both sides, and a 35 s clip at K = 750:
    two windows, the second with the first's text in its prompt"""
    path, ctx = micro
    ctx.set_precision("exact")
    pcm = synth.clip(12, 16000 * 3)
    for K, kw in ((100, {"lang_id": -1}), (129, {"no_timestamps": 1}), (17, {"max_initial_ts": 0.0}), (100, {"lang_id": -1, "no_timestamps": 1})):
        g = ctx.full_batch([pcm], _params(ctx, audio_ctx=K, **kw))[0]
        _same_as_oracle(g, _oracle_full(path, K, pcm, **kw), (K, kw))
    long = synth.clip(11, 16000 * 35)
    g = ctx.full_batch([long], _params(ctx, audio_ctx=750))[0]
    o = _oracle_full(path, 750, long)
    _same_as_oracle(g, o, "35 s at K = 750")
    assert o["n_windows"] == 2
    assert _ids(o) != _ids(_oracle_full(path, 0, long))      # the shorter context is heard: the transcript is not the full-context one


def test_quantised_file_equals_the_oracle(eng):
    """a q5_1 file (tiny) in the exact precision — ggml's q8 arithmetic — at K = 100"""
    from conftest import quantized_model
    path = quantized_model("tiny", "q5_1")
    pcm = synth.clip(14, 16000 * 2 + 5)
    m = eng.Model(path); ctx = eng.Context(m, max_batch=2, max_samples=16000 * 5)
    try:
        assert m.quant != 0
        res = ctx.full_batch([pcm, pcm], params=[_params(ctx, audio_ctx=100), _params(ctx, audio_ctx=0)])
        packed = ctx.full_batch([pcm, pcm], params=[_params(ctx, audio_ctx=17), _params(ctx, audio_ctx=100)])      # both short: 256 encoder rows per slot
        assert _key(packed[1]) == _key(res[0]) and _key(packed[0]) != _key(res[0])
    finally:
        ctx.close(); m.close()
    om = OracleModel(audio_ctx_model(path, 100)); om0 = OracleModel(path)
    assert om.quant != 0
    p = _params(om); p.max_initial_ts = scaled_max_initial_ts(1.0, NC, 100)
    _same_as_oracle(res[0], om.full(pcm, p), "q5_1 at K = 100")
    _same_as_oracle(res[1], om0.full(pcm), "q5_1 at full context beside it")
    om.close(); om0.close()


# ------------------------------------------------------------------ 3. mixed K in one call
MIX_K = [1500, 17, 100, 0, 750, 32, 129, 1]
MIX_SECS = [4.0, 1.5, 2.0, 3.5, 3.0, 1.7, 2.6, 2.2]


def test_mixed_audio_contexts_in_one_call(micro):
    """eight rows, eight audio contexts, different lengths: each row is its alone call and the oracle's transcript on M'(K)"""
    path, ctx = micro
    ctx.set_precision("exact")
    pcms = [synth.clip(20 + i, int(16000 * s)) for i, s in enumerate(MIX_SECS)]
    res = ctx.full_batch(pcms, params=[_params(ctx, audio_ctx=K) for K in MIX_K])
    for i, (K, pcm, g) in enumerate(zip(MIX_K, pcms, res)):
        _same_as_oracle(g, _oracle_full(path, K, pcm), (i, K))
        alone = ctx.full_batch([pcm], _params(ctx, audio_ctx=K))[0]
        assert _key(alone) == _key(g), (i, K)
    assert len({tuple(_ids(r)) for r in res}) == len(res)
    # only short rows: the encoder pass is packed to 256 rows per slot (in the call above a full-length row kept it at 1500), same transcripts
    short = [i for i, K in enumerate(MIX_K) if 0 < K < 256]
    again = ctx.full_batch([pcms[i] for i in short], params=[_params(ctx, audio_ctx=MIX_K[i]) for i in short])
    assert len(short) == 5 and [_key(r) for r in again] == [_key(res[i]) for i in short]


def test_short_context_row_goes_down_the_temperature_ladder_beside_a_long_one(eng):
    """A model whose greedy pass fails the default log-prob threshold (micro, gamma_text 8).  Row 1 (K = 100) retries its window at the next temperatures — its cross K / V move
    from slot 1 to slot 0 and its K must move with them — while row 0 (full context, a threshold it passes) advances to its second window in the slot beside it."""
    from conftest import _ensure_built
    path = "/tmp/skw_test_micro_gamma8.bin"
    if not os.path.exists(path):
        subprocess.check_call([_ensure_built(), path + ".tmp", "--size", "micro", "--gamma_text", "8"]); os.replace(path + ".tmp", path)
    pcms = [synth.clip(63, 16000 * 40), synth.clip(61, 16000 * 4), synth.clip(62, 16000 * 3)]
    sets = [dict(audio_ctx=0, logprob_thold=-5.0), dict(audio_ctx=100), dict(audio_ctx=17, temperature_inc=0.4)]
    m = eng.Model(path); ctx = eng.Context(m, max_batch=4, max_samples=16000 * 41)
    states = [eng.rng_state_new() for _ in pcms]
    try:
        res = ctx.full_batch(pcms, params=[_params(ctx, **kw) for kw in sets], rng_states=states)
    finally:
        ctx.close(); m.close()
    for i, (pcm, kw, g, st) in enumerate(zip(pcms, sets, res, states)):
        ost = eng.rng_state_new(); kw = dict(kw); K = kw.pop("audio_ctx")
        o = _oracle_full(path, K, pcm, rng_state=ost, **kw)
        _same_as_oracle(g, o, (i, K, kw))
        assert np.array_equal(st, ost), (i, "generator state after the call")
    assert res[0]["n_windows"] == 2 and res[0]["fallback_requested"] == 0 and res[1]["fallback_requested"] >= 1 and res[2]["fallback_requested"] >= 1


# ------------------------------------------------------------------ 4. stale keys
@pytest.mark.parametrize("precision", ["exact", "f16_mfma"])
def test_keys_of_an_earlier_longer_call_reach_nothing(eng, micro_model_path, precision):
    """one context: a full-length call on two loud 30 s clips, then K = 100 / K = 17 on other audio in the same slots == the same short call in a fresh context, bit for bit"""
    loud = [synth.clip(2, 16000 * 30), synth.clip(4, 16000 * 30)]
    pcms = [synth.clip(30, 16000 * 3), synth.clip(31, 16000 * 2)]
    m = eng.Model(micro_model_path)
    used = eng.Context(m, max_batch=2, max_samples=16000 * 31); fresh = eng.Context(m, max_batch=2, max_samples=16000 * 31)
    try:
        used.set_precision(precision); fresh.set_precision(precision)
        assert all(len(r["tokens"]) > 0 for r in used.full_batch(loud))
        ps = lambda c: [_params(c, audio_ctx=100), _params(c, audio_ctx=17)]      # noqa: E731
        a = used.full_batch(pcms, params=ps(used)); b = fresh.full_batch(pcms, params=ps(fresh))
        assert [_key(r) for r in a] == [_key(r) for r in b]
        ea = used.encode(pcms[0], audio_ctx=100); eb = fresh.encode(pcms[0], audio_ctx=100)
        assert all(bits_equal(x, y) for x, y in zip(ea, eb))
        assert bits_equal(used.decode_logits(TOKS), fresh.decode_logits(TOKS))
        assert all(np.isfinite(x).all() for x in ea)
    finally:
        used.close(); fresh.close(); m.close()


# ------------------------------------------------------------------ 5. f16_mfma
@pytest.mark.parametrize("size", ["tiny", "micro"])
def test_f16_mfma_is_held_to_the_exact_precision_at_the_same_k(eng, size):
    """streamkit_amd/parity.py, teacher forced, inside that file's bounds for the model shape, unchanged: at K < 1500 every contraction and every softmax is no longer than at 1500.
    The last case is the two-window clip at K = 750: its second window's prompt goes through the prompt pass's multi-query cross attention."""
    from conftest import synth_model
    m = eng.Model(synth_model(size)); ctx = eng.Context(m, max_batch=4, max_samples=16000 * 36)
    try:
        eb, mb = bounds_for(m.hp)
        clips = [synth.clip(40 + i, int(16000 * s)) for i, s in enumerate((4.0, 2.5, 1.5))]
        for K, cl in ((17, clips), (100, clips), (750, clips), (750, [synth.clip(11, 16000 * 35)])):
            tf = teacher_forced_compare(ctx, cl, _params(ctx, audio_ctx=K))
            print("%s K=%d: %d decisions, %d differ, max margin at a difference %s (bound %g), max logit error %.4f (bound %g)"
                  % (size, K, tf["steps_checked"], tf["argmax_disagreements"], tf["max_margin_at_disagreement"], mb, tf["max_logit_err"], eb))
            assert tf["logit_err_bound"] == eb and tf["margin_bound"] == mb
            assert tf["ok"] and tf["steps_checked"] > 0, (size, K, tf["max_logit_err"], tf["max_margin_at_disagreement"])
    finally:
        ctx.close(); m.close()


def test_f16_mfma_mixed_rows_equal_their_alone_calls(micro):
    """the precision's batch-composition contract (prompts of 3 tokens per row: no prompt pass comes near 256 rows): a mixed-K batch's rows are their alone calls, bit for bit"""
    path, ctx = micro
    ctx.set_precision("f16_mfma")
    try:
        pcms = [synth.clip(20 + i, int(16000 * s)) for i, s in enumerate(MIX_SECS)]
        res = ctx.full_batch(pcms, params=[_params(ctx, audio_ctx=K) for K in MIX_K])
        for i, (K, pcm, g) in enumerate(zip(MIX_K, pcms, res)):
            assert _key(ctx.full_batch([pcm], _params(ctx, audio_ctx=K))[0]) == _key(g), (i, K)
            assert len(g["tokens"]) > 0
    finally:
        ctx.set_precision("exact")


# ------------------------------------------------------------------ 6. 0 and n_audio_ctx are today's call
@pytest.mark.parametrize("precision", ["exact", "f16_mfma"])
def test_zero_and_the_models_own_context_are_the_plain_call(micro, precision):
    path, ctx = micro
    ctx.set_precision(precision)
    try:
        pcms = [synth.clip(50, 16000 * 4), synth.clip(51, 16000 * 33)]
        plain = [_key(r) for r in ctx.full_batch(pcms)]
        for K in (0, NC):
            assert [_key(r) for r in ctx.full_batch(pcms, _params(ctx, audio_ctx=K))] == plain, K
            assert [_key(r) for r in ctx.full_batch(pcms, params=[_params(ctx, audio_ctx=K), _params(ctx, audio_ctx=NC - K)])] == plain, K
        tap = ctx.encode(pcms[0]); x0 = ctx.conv_stem(pcms[0]); lg = ctx.decode_logits(TOKS)
        for K in (0, NC):
            assert bits_equal(ctx.conv_stem(pcms[0], audio_ctx=K), x0), K
            assert all(bits_equal(a, b) for a, b in zip(ctx.encode(pcms[0], audio_ctx=K), tap)), K
            assert bits_equal(ctx.decode_logits(TOKS), lg), K
        if precision == "exact":
            _same_as_oracle(ctx.full_batch([pcms[0]], _params(ctx, audio_ctx=NC))[0], _oracle(path, 0).full(pcms[0]), "K = n_audio_ctx")
    finally:
        ctx.set_precision("exact")


# ------------------------------------------------------------------ 7. refusals
def test_out_of_range_values_are_refused_naming_the_clip(micro):
    path, ctx = micro
    ctx.set_precision("exact")
    pcm = synth.clip(3, 16000 * 2)
    with pytest.raises(RuntimeError, match=r"clip 1: audio_ctx 1501 outside \[0, 1500\]"):
        ctx.full_batch([pcm] * 3, params=[_params(ctx), _params(ctx, audio_ctx=NC + 1), _params(ctx, audio_ctx=17)])
    with pytest.raises(RuntimeError, match=r"clip 2: audio_ctx -1 outside \[0, 1500\]"):
        ctx.full_batch([pcm] * 3, params=[_params(ctx), _params(ctx, audio_ctx=NC), _params(ctx, audio_ctx=-1)])
    with pytest.raises(RuntimeError, match=r"clip 0: audio_ctx -5 outside"):
        ctx.full_batch([pcm], _params(ctx, audio_ctx=-5))
    with pytest.raises(RuntimeError, match=r"audio_ctx 1501 outside"):
        ctx.encode(pcm, audio_ctx=NC + 1)
    ok = ctx.full_batch([pcm] * 2, params=[_params(ctx), _params(ctx, audio_ctx=17)])      # the context is usable afterwards
    assert len(ok) == 2 and len(ok[0]["tokens"]) > 0


def _node_segments(o):
    return [{"text": s["text"].decode().strip(), "start_time_ms": s["t0"] * 10, "end_time_ms": s["t1"] * 10, "confidence": None} for s in o["segments"] if s["text"].decode().strip()]


def _feed_and_flush_together(nodes, pcms):
    """one thread per instance: feed the clip (no cut: vad_mode always, shorter than a segment), meet at the barrier, flush — the tails queue together"""
    barrier = threading.Barrier(len(nodes)); rcs = [None] * len(nodes); errors = []

    def worker(k):
        try:
            for i in range(0, pcms[k].size, 960):
                assert nodes[k].process_audio(pcms[k][i:i + 960]) == 0, nodes[k].last_error()
            barrier.wait(timeout=120)
            rcs[k] = nodes[k].flush()
        except Exception as e:      # noqa: BLE001
            errors.append((k, repr(e))); barrier.abort()

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(len(nodes))]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errors, errors
    return rcs


def test_node_refusal_stays_with_its_request(micro_model_path):
    plugin = minihost.Plugin(); path = micro_model_path
    pcm = synth.clip(33, 16000 * 3)
    sets = [{"audio_ctx": 100}, {"audio_ctx": NC + 1}, {"audio_ctx": "auto"}, {"audio_ctx": -3}]
    nodes = [plugin.create_node(dict(st, model_path=path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=200, max_batch=8)) for st in sets]
    rcs = _feed_and_flush_together(nodes, [pcm] * len(nodes))
    for k, st in enumerate(sets):
        if st["audio_ctx"] in (NC + 1, -3):
            assert rcs[k] != 0 and "audio_ctx %d outside" % st["audio_ctx"] in nodes[k].last_error() and not nodes[k].outputs(), (k, rcs[k], nodes[k].last_error())
        else:
            assert rcs[k] == 0, (k, nodes[k].last_error())
            K = 100 if st["audio_ctx"] == 100 else engine.audio_ctx_for_samples(pcm.size, NC)
            segs = _node_segments(_oracle_full(path, K, pcm, suppress_nst=1))
            got = [json.loads(o[2].decode()) for o in nodes[k].outputs()]
            assert segs and len(got) == 1 and got[0]["segments"] == segs, k
    for nd in nodes:
        nd.destroy()


# ------------------------------------------------------------------ 8. the node on "auto"
def test_node_auto_batches_segments_of_different_lengths_in_one_call(eng, micro_model_path):
    """Four instances on audio_ctx "auto" whose segments of 1, 2, 4 and 9 s arrive together: one engine call, each transcript the oracle's on M'(K) with K from the exported rule;
    then update_params switches one instance to a fixed K and its next segment uses it."""
    plugin = minihost.Plugin(); path = micro_model_path
    secs = [1, 2, 4, 9]
    pcms = [synth.clip(70 + i, 16000 * s) for i, s in enumerate(secs)]
    cfg = dict(model_path=path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=300, max_batch=8, audio_ctx="auto")
    nodes = [plugin.create_node(dict(cfg)) for _ in secs]
    assert all(n is not None for n in nodes)
    before = minihost.whisper_batch_stats()
    rcs = _feed_and_flush_together(nodes, pcms)
    calls, jobs, mixed = (a - b for a, b in zip(minihost.whisper_batch_stats(), before))
    assert rcs == [0] * 4, [n.last_error() for n in nodes]
    assert (calls, jobs, mixed) == (1, 4, 1), (calls, jobs, mixed)
    ks = [eng.audio_ctx_for_samples(p.size, NC) for p in pcms]
    assert ks == [96, 128, 256, 480]
    for k, (K, pcm) in enumerate(zip(ks, pcms)):
        segs = _node_segments(_oracle_full(path, K, pcm, suppress_nst=1))
        got = [json.loads(o[2].decode()) for o in nodes[k].outputs()]
        assert segs and len(got) == 1 and got[0]["segments"] == segs, (k, K)
    # a fixed K from the next segment on
    assert nodes[2].update_params(dict(cfg, audio_ctx=64)) == 0, nodes[2].last_error()
    n_before = len(nodes[2].outputs())
    nxt = synth.clip(75, 16000 * 3)
    for i in range(0, nxt.size, 960):
        assert nodes[2].process_audio(nxt[i:i + 960]) == 0, nodes[2].last_error()
    assert nodes[2].flush() == 0, nodes[2].last_error()
    got = [json.loads(o[2].decode()) for o in nodes[2].outputs()][n_before:]
    o64 = _oracle_full(path, 64, nxt, suppress_nst=1)
    assert _ids(o64) != _ids(_oracle_full(path, eng.audio_ctx_for_samples(nxt.size, NC), nxt, suppress_nst=1))      # "auto" would have given another transcript
    segs = _node_segments(o64)
    assert segs and len(got) == 1 and [dict(s, start_time_ms=0, end_time_ms=0) for s in got[0]["segments"]] == [dict(s, start_time_ms=0, end_time_ms=0) for s in segs]
    assert [s["end_time_ms"] - s["start_time_ms"] for s in got[0]["segments"]] == [s["end_time_ms"] - s["start_time_ms"] for s in segs]      # (the stream's clock ran on: times are offset)
    for nd in nodes:
        nd.destroy()
    with pytest.raises(RuntimeError):      # a string other than "auto" is a configuration error
        plugin.create_node(dict(cfg, audio_ctx="sometimes"))
