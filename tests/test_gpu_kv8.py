"""cross_kv = q8_0 on the GPU (include/skw_kv8.h; tests/kv8_ref_lib.py has the numpy restatement, the derived bound and the cases; tests/test_cpu_kv8_cases.py shows on the CPU
that an off-by-one in the key count cannot pass them).

Kernel by kernel, through the public launchers (skw_debug_kv8_quantize / skw_debug_attn_kv8): k_kv8_quantize's image equals numpy byte for byte, k_dec_cross_attn_kv8's raw scores
equal the contract's bit for bit, its outputs lie inside the bound in every output form, rows it must leave alone keep the sentinel, and a row's bits do not depend on its
neighbours.  Then the engine and the node: the teacher-forced comparison of the q8_0 leg against the exact precision under the measured bounds (streamkit_amd/parity.py), the
toggle leaving nothing behind, the exact precision ignoring the flag, and a transcript through the mini-host.  Every f16 pad position of K and V is a NaN."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref_lib as kv  # noqa: E402
from streamkit_amd import minihost, synth  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = kv.cases()
SENTINEL = 0x5A5A
SENT16 = np.array([SENTINEL], np.uint16).view(np.float16).astype(np.float32).view(np.uint32)[0]
SENT32 = np.uint32(SENTINEL | (SENTINEL << 16))
WORST = {}
_PREPARED = {}


@pytest.fixture(scope="module")
def ctx(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path); c = engine.Context(m, max_batch=1, max_samples=16000)
    c.set_precision("f16_mfma")
    yield c
    c.close(); m.close()


def _prepared(case):
    if case.name not in _PREPARED:
        _PREPARED.clear()                                                  # one case's arrays at a time
        _PREPARED[case.name] = case.prepared()
    return _PREPARED[case.name]


def _launch(ctx, case, rows=None, **flags):
    """the case's launch (rows: only these query rows, with their flags), every pad a NaN; a launch the device refused or faulted on ends the session"""
    Q, K, V, _, _ = _prepared(case)
    kw = {k: case.kw.get(k) for k in ("active", "seq", "count")}
    if rows is not None:
        Q = Q[rows]; kw = {k: (None if v is None else [v[r] for r in rows]) for k, v in kw.items()}
        if kw["seq"] is None:
            kw["seq"] = list(rows)                                         # a row's sequence is its own index unless the case maps it
    try:
        return ctx.attn_kv8(case.H, case.n_ctx, Q, K, V, case.fill_from(), k_pad=kv.K_PAD, v_pad=kv.V_PAD, slot_k=case.slot_k() if case.vark else None, sentinel=SENTINEL,
                            **kw, **flags)
    except RuntimeError as e:
        pytest.exit("%s %r: %s" % (case.name, flags, e), returncode=3)


def _check(case, form, got, sentinel):
    """finite, inside the bound, and every row the kernel must leave alone still the sentinel, bit for bit"""
    _, _, _, _, refs = _prepared(case)
    written = np.zeros(len(case.rows), bool); worst = 0.0
    for rs, s, n, h, sl, sc, Vh, ref, bound in refs:
        worst = max(worst, float(kv.ratio(got[rs, sl], ref, bound).max())); written[rs] = True
    WORST[form] = max(WORST.get(form, 0.0), worst)
    print("%s %s: error / bound %.3f" % (case.name, form, worst))
    assert (got[~written].view(np.uint32) == sentinel).all(), "%s %s: a row the kernel must leave alone was written" % (case.name, form)
    assert worst <= 1.0, "%s %s: %.3f of the bound" % (case.name, form, worst)


def test_numpy_offsets_equal_the_exported_layout_functions():
    """kv8_ref_lib.image_offsets against skw_layout_kv8_* (one ctypes call per byte: one small geometry with two heads, a ragged Tpad and more than one record)"""
    from streamkit_amd import engine
    L = engine.lib(); H, n_ctx, T = 2, 100, 96; Tpad = 128; d = H * 64
    kq, kd, vq, vd = kv.image_offsets(H, n_ctx, T)
    for k in range(T):
        assert [L.skw_layout_kv8_kq_off(0, H, Tpad, k, f) for f in range(d)] == list(kq[k]) and [L.skw_layout_kv8_vq_off(0, H, Tpad, f, k) for f in range(d)] == list(vq[k])
        assert [L.skw_layout_kv8_kd_off(0, H, Tpad, k, 32 * b) for b in range(2 * H)] == list(kd[k])
    for j in range(T // 32):
        assert [L.skw_layout_kv8_vd_off(0, H, Tpad, f, 32 * j) for f in range(d)] == list(vd[j])
    assert engine.kv8_slot_bytes(H, Tpad) == H * (Tpad // 32) * kv.REC


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_quantise_kernel_equals_numpy_byte_for_byte(ctx, case):
    """every case, every slot: qs and scales of K and V^T, NaN pads without a trace, nothing written behind the last record of the slot's count"""
    _, K, V, _, _ = _prepared(case)
    counts = case.slot_k()
    try:
        img = ctx.kv8_quantize(case.H, case.n_ctx, K, V, case.fill_from(), k_pad=kv.K_PAD, v_pad=kv.V_PAD, slot_k=counts if case.vark else None)
    except RuntimeError as e:                                              # a launch the device refused or faulted on: nothing more runs on it in this session
        pytest.exit("%s quantise: %s" % (case.name, e), returncode=3)
    for s, n in enumerate(counts):
        T = (n + 31) // 32 * 32
        kq, kd, vq, vd = kv.quantize_slot(K[s], V[s], n)
        gkq, gkd, gvq, gvd = kv.unpack_image(img[s], case.H, case.n_ctx, T)
        assert np.array_equal(gkq, kq) and np.array_equal(gvq, vq), "%s slot %d: qs differ" % (case.name, s)
        assert np.array_equal(gkd.view(np.uint32), kd.view(np.uint32)) and np.array_equal(gvd.view(np.uint32), vd.view(np.uint32)), "%s slot %d: scales differ" % (case.name, s)
        if n % 32:
            assert not gkq[n:].any() and not gkd[n:].any() and not gvq[n:].any(), "%s slot %d: a NaN pad left a trace" % (case.name, s)
        # records of blocks wholly past the count are not written: per head, everything behind the written records is still the fill byte
        per_head = img[s].reshape(case.H, -1)
        assert (per_head[:, T // 32 * kv.REC:] == 0xEE).all() and not (per_head[:, :T // 32 * kv.REC] == 0xEE).all(axis=1).any(), "%s slot %d" % (case.name, s)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_raw_scores_equal_the_contract_bit_for_bit(ctx, case):
    got = _launch(ctx, case, raw=1)
    _, _, _, _, refs = _prepared(case)
    assert got.shape == (len(case.rows), case.H, case.n_ctx)
    seen = np.zeros(got.shape, bool)
    for rs, s, n, h, sl, sc, Vh, ref, bound in refs:
        assert np.array_equal(got[rs, h, :n].view(np.uint32), sc.view(np.uint32)), "%s slot %d, %d keys, head %d" % (case.name, s, n, h)
        seen[rs, h, :n] = True
    assert np.isnan(got[~seen]).all(), "%s: a score was written for a key past the row's count or for an inactive row" % case.name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_outputs_inside_the_bound_in_every_form(ctx, case):
    one = _launch(ctx, case); _check(case, "rows", one, SENT16)
    assert np.array_equal(one.view(np.uint32), _launch(ctx, case, ofrag=1).view(np.uint32)), "the fragment-order output differs from the rows"
    f32 = _launch(ctx, case, f32_out=1); _check(case, "f32_out", f32, SENT32)
    live = [r for r in range(len(case.rows)) if case.live[r]]
    assert np.array_equal(f32[live].astype(np.float16).view(np.uint16), one[live].astype(np.float16).view(np.uint16)), "the f16 rows are not the rounded f32 rows"


@pytest.mark.parametrize("case", [c for c in CASES if len(c.rows) > 1], ids=lambda c: c.name)
def test_a_rows_bits_do_not_depend_on_its_neighbours(ctx, case):
    among = _launch(ctx, case)
    for r in [r for r in range(len(case.rows)) if case.live[r]][:3]:
        alone = _launch(ctx, case, rows=[r])
        assert np.array_equal(alone[0].view(np.uint32), among[r].view(np.uint32)), "%s row %d" % (case.name, r)


def test_report_the_largest_error_over_bound_per_form():
    print("\nq8 cross attention, largest error / bound per output form: " + "   ".join("%s %.3f" % kv_ for kv_ in sorted(WORST.items())))
    assert max(WORST.values(), default=0.0) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the engine
def _params(c, **kw):
    p = c.default_params()
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _key(r):
    return ([tuple(np.float32(x).view(np.uint32) if isinstance(x, float) else x for x in t) for t in r["tokens"]], [(s["t0"], s["t1"], s["text"]) for s in r["segments"]],
            r["n_windows"], r["fallback_requested"], r["lang_id"], r["n_decode_steps"])


def engine_batch(c):
    """a mixed audio_ctx batch: a short clip at K = 100, one at the full context that fails its greedy pass and goes down the temperature ladder, and a 35 s clip at K = 750 whose
    second window decodes behind a prompt"""
    clips = [synth.clip(40, 16000 * 4), synth.clip(41, int(16000 * 2.5)), synth.clip(11, 16000 * 35)]
    return clips, [_params(c, audio_ctx=100), _params(c, audio_ctx=0, logprob_thold=-0.05, temperature_inc=0.4), _params(c, audio_ctx=750)]


def traced_runs(c):
    """The same three settings as calls of their own: a traced call takes ONE parameter block (engine.full_batch), so the teacher-forced comparison sees the mix one audio_ctx at
    a time, each over a batch of several clips — short clips at K = 100, the full context with a temperature pass, and K = 750 with a 35 s clip (a prompt) beside a short one."""
    short = [synth.clip(40 + i, int(16000 * s)) for i, s in enumerate((4.0, 2.5, 1.5))]
    return [("K100", short, _params(c, audio_ctx=100)), ("full_sampled", short[:2], _params(c, audio_ctx=0, logprob_thold=-0.05, temperature_inc=0.4)),
            ("K750_prompt", [synth.clip(11, 16000 * 35), short[0]], _params(c, audio_ctx=750)),
            # the two compositions that set parity.py's KV8_SMALL_MODEL_* bounds: few keys average the least of the 8-bit rounding away (logit error), four full windows make the
            # most decisions (margin at a disagreement)
            ("K17", short, _params(c, audio_ctx=17)), ("four_30s", [synth.clip(i, 480000) for i in range(4)], c.default_params())]


@pytest.fixture(scope="module")
def big(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path); c = engine.Context(m, max_batch=4, max_samples=16000 * 36)
    yield c
    c.close(); m.close()


def test_q8_leg_is_held_to_the_exact_precision_under_the_measured_bounds(big):
    from streamkit_amd.parity import bounds_for, teacher_forced_compare
    sampled = steps = windows = 0
    for name, clips, params in traced_runs(big):
        tf = teacher_forced_compare(big, clips, params, cross_kv="q8_0")
        print("%s, q8_0 leg against exact: %d decisions (%d in temperature passes), %d differ, largest margin at a disagreement %s, largest logit error %.4f; bounds %s"
              % (name, tf["steps_checked"], tf["sampled_steps"], tf["argmax_disagreements"], tf["max_margin_at_disagreement"], tf["max_logit_err"], bounds_for(big.model.hp, "q8_0")))
        sampled += tf["sampled_steps"]; steps += tf["steps_checked"]; windows = max(windows, tf["results_exact"][0]["n_windows"])
        assert big.get_cross_kv() == "f16" and big.get_precision() == "exact"                                       # both restored
        assert tf["ok"], (name, {k: tf[k] for k in ("argmax_disagreements", "max_margin_at_disagreement", "max_logit_err", "logit_err_bound", "margin_bound")})
    assert sampled > 0 and windows >= 2 and steps > 100                                                             # a temperature pass and a prompt did happen


def test_the_toggle_leaves_nothing_behind(big):
    """f16_mfma results with cross_kv f16 are bit-identical before and after the context has run with q8_0 (step graphs are keyed by the flag), and q8_0 did change something"""
    clips, params = engine_batch(big)
    big.set_precision("f16_mfma")
    try:
        before = [_key(r) for r in big.full_batch(clips, params)]
        big.set_cross_kv("q8_0")
        q8 = big.full_batch(clips, params)
        assert [_key(r) for r in big.full_batch(clips, params)] == [_key(r) for r in q8]      # and q8_0 repeats itself
        big.set_cross_kv("f16")
        assert [_key(r) for r in big.full_batch(clips, params)] == before
        assert [_key(r) for r in q8] != before, "cross_kv q8_0 changed no bit of any log-probability: the q8 kernels did not run"
    finally:
        big.set_cross_kv("f16"); big.set_precision("exact")


def test_the_exact_precision_ignores_the_flag(big):
    clips, params = engine_batch(big)
    assert big.get_precision() == "exact"
    before = [_key(r) for r in big.full_batch(clips, params)]
    big.set_cross_kv("q8_0")
    try:
        assert [_key(r) for r in big.full_batch(clips, params)] == before
    finally:
        big.set_cross_kv("f16")
    with pytest.raises(KeyError):
        big.set_cross_kv("q4_0")


def test_node_with_cross_kv_q8_0_transcribes_and_f16_gets_its_own_context():
    from conftest import synth_model
    plugin = minihost.Plugin()
    path = synth_model("tiny", seed=4321)      # a model file no other test loads: what the context cache says below is about these three instances alone
    cfg = dict(model_path=path, vad_mode="always", flush_tail=True, precision="f16_mfma", max_batch=2, gpu_device=0)
    pcm = synth.clip(6, 16000 * 5)

    def transcript(node):
        for i in range(0, pcm.size, 960):
            assert node.process_audio(pcm[i:i + 960]) == 0, node.last_error()
        assert node.flush() == 0, node.last_error()
        return [json.loads(o[2].decode()) for o in node.outputs()]

    a = plugin.create_node(dict(cfg, cross_kv="q8_0"))
    b = plugin.create_node(dict(cfg, cross_kv="f16"))
    assert any("CACHE MISS" in l for l in a.logs()) and any("CACHE MISS" in l for l in b.logs()), "cross_kv is not part of the context cache's key"
    ta, tb = transcript(a), transcript(b)
    assert len(ta) == 1 and ta[0]["segments"] and len(tb) == 1 and tb[0]["segments"]
    c = plugin.create_node(dict(cfg, cross_kv="q8_0"))
    assert any("CACHE HIT" in l for l in c.logs())
    for n in (a, b, c):
        n.destroy()
    with pytest.raises(RuntimeError, match="Invalid config: cross_kv \"q8_0\" needs precision \"f16_mfma\""):
        plugin.create_node(dict(cfg, precision="exact", cross_kv="q8_0"))
