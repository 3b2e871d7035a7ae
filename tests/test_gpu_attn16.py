"""The f16_mfma attention kernels, each on its own against a float64 softmax(scale Q K^T) V under a derived bound (tests/attn_ref_lib.py has the reference, the bound, the operands
and the case list; tests/test_cpu_attn_cases.py shows on the CPU that an off-by-one in the key count cannot pass these cases).

What runs, through the public launchers (skw_debug_attn16, skw_hooks.hip): k_attn_encoder16 in its encoder, prompt-pass (XP) and per-clip (VARK) forms, k_dec_cross_attn16<3,3> and
<3,3,true>, the two-phase k_dec_cross_attn<24,4,3,true> and the FASTV form of k_dec_attn — at the real strides (n_ctx 1500, Tpad 1504) with key counts on either side of every block
edge, H = 4 (a cross-attention workgroup's third head slot is invalid) and H = 6 (the self attention's four-head block is ragged), inactive rows, rows mapped to another sequence.
Every K / V position a kernel must not use is poisoned: NaN in K; NaN in V where the kernel promises to replace it, 1000.0 where it relies on p = 0.

Per launch and per form the largest error / bound seen is printed (pytest -s); DESIGN.md section 3 is where the per-form maxima belong.  The numpy emulation of the kernels'
arithmetic reaches 0.26 of the bound on these cases (tests/test_cpu_attn_cases.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref_lib as ar  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ar.cases()
SENTINEL = 0x5A5A
SENTINEL_F32 = np.array([SENTINEL], np.uint16).view(np.float16).astype(np.float32)[0]
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
    """operands and, per (slot, key count, head), the reference and the bound of the rows the kernel writes: computed once per case, shared by its launches, never modified"""
    if case.name not in _PREPARED:
        _PREPARED.clear()                                                  # one case's arrays at a time
        Q, K, V, _ = case.operands()
        groups = {}
        for r, (s, n) in enumerate(case.rows):
            if case.live[r]:
                groups.setdefault((s, n), []).append(r)
        refs = []
        for (s, n), rs in groups.items():
            for h in range(case.H):
                sl = slice(h * 64, h * 64 + 64)
                ref, bound, _ = ar.reference(Q[rs, sl], K[s, :n, sl], V[s, :n, sl], case.scale)
                refs.append(([case.out_row[r] for r in rs], sl, ref, bound))
        for a in (Q, K, V):
            a.setflags(write=False)
        _PREPARED[case.name] = (Q, K, V, refs)
    return _PREPARED[case.name]


def _launch(ctx, case, form, **flags):
    Q, K, V, _ = _prepared(case)
    k_pad, v_pad = case.pads()
    kw = {k: v for k, v in case.kw.items() if k in ("slot_k", "out_rows", "row0", "nq", "slot", "active", "seq", "count")}
    if case.form == "encoder":                                             # its queries are the slots' own rows
        Qe = np.zeros(K.shape, np.float16); at = 0
        for s, (_, counts) in enumerate(case.slots):
            Qe[s, :counts[0]] = Q[at:at + counts[0]]; Qe[s, counts[0]:] = np.float16(np.nan); at += counts[0]
        Q = Qe
    elif case.form == "prefill":                                           # the pass's rows: each sequence's queries at its row0, NaN between them
        Qp = np.full((case.n_out, Q.shape[1]), np.nan, np.float16)
        Qp[case.out_row] = Q; Q = Qp
    try:
        got = ctx.attn16(form, case.H, case.n_ctx, Q, K, V, case.fill_from(), k_pad=k_pad, v_pad=v_pad, sentinel=SENTINEL, **kw, **flags)
    except RuntimeError as e:                                              # a launch the device refused or faulted on: nothing more runs on it in this session
        pytest.exit("%s %s %r: %s" % (case.name, form, flags, e), returncode=3)
    assert got.shape == (case.n_out, case.H * 64)
    return got


def _check(case, form, got):
    """finite, under the bound, and every row the kernel must leave alone still the sentinel, bit for bit"""
    _, _, _, refs = _prepared(case)
    written = np.zeros(case.n_out, bool); worst = 0.0
    for rows, sl, ref, bound in refs:
        g = got[rows, sl].astype(np.float64)
        assert np.isfinite(g).all(), "%s %s: non-finite output" % (case.name, form)
        worst = max(worst, float((np.abs(g - ref) / bound).max()))
        written[rows] = True
    WORST[form] = max(WORST.get(form, 0.0), worst)
    print("%s %s: error / bound %.3f" % (case.name, form, worst))
    assert (got[~written].view(np.uint32) == SENTINEL_F32.view(np.uint32)).all(), "%s %s: a row the kernel must leave alone was written" % (case.name, form)
    assert worst <= 1.0, "%s %s: %.3f of the bound" % (case.name, form, worst)


def _within(case, a, b, factor):
    _, _, _, refs = _prepared(case)
    for rows, sl, _, bound in refs:
        assert (np.abs(a[rows, sl].astype(np.float64) - b[rows, sl]) <= factor * bound).all()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", [c for c in CASES if c.form == "cross"], ids=lambda c: c.name)
def test_decode_cross_attention(ctx, case):
    one = _launch(ctx, case, "cross16"); _check(case, "cross16", one)
    assert _same_bits(one, _launch(ctx, case, "cross16", ofrag=1)), "the fragment-order output differs from the rows"
    two = _launch(ctx, case, "cross2p"); _check(case, "cross2p", two)
    _within(case, one, two, 2.0)


@pytest.mark.parametrize("case", [c for c in CASES if c.form == "self"], ids=lambda c: c.name)
def test_decode_self_attention_fastv(ctx, case):
    got = _launch(ctx, case, "self"); _check(case, "self", got)
    assert _same_bits(got, _launch(ctx, case, "self", ofrag=1)), "the fragment-order output differs from the rows"


@pytest.mark.parametrize("case", [c for c in CASES if c.form == "encoder"], ids=lambda c: c.name)
def test_encoder_attention(ctx, case):
    _check(case, "encoder", _launch(ctx, case, "encoder"))


@pytest.mark.parametrize("case", [c for c in CASES if c.form == "prefill"], ids=lambda c: c.name)
def test_prompt_pass_cross_attention(ctx, case):
    rows = _launch(ctx, case, "prefill", frag=0); _check(case, "prefill", rows)
    frag = _launch(ctx, case, "prefill", frag=1); _check(case, "prefill", frag)
    _within(case, rows, frag, 1.0)
    assert _same_bits(rows, _launch(ctx, case, "prefill", frag=0, ofrag=1)) and _same_bits(frag, _launch(ctx, case, "prefill", frag=1, ofrag=1)), \
        "the fragment-order output differs from the rows"


def test_report_the_largest_error_over_bound_per_form():
    print("\nf16 attention kernels, largest error / bound per form: " + "   ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    assert max(WORST.values(), default=0.0) <= 1.0
