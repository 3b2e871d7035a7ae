"""The exact precision's attention kernels, each on its own against the numpy restatement of the contract, bit for bit (tests/attn_exact_ref_lib.py has the restatement, the operands
and the case list; tests/test_cpu_attn_exact_cases.py pins the restatement to the oracle's arithmetic and shows that no row's expectation depends on a summation order, so no row is
skipped here and nothing is a tolerance).

What runs, through the public launchers: k_attn_encoder (with and without per-slot key counts) and k_attn_encoder_v3<94, 72> through skw_attn_encoder — which of the two ran is
reported by the hook and asserted — and k_dec_attn<7> (fastv = 0) through skw_dec_self_attn (skw_debug_attn_exact); k_dec_cross_attn<24, 4, 3> and k_xattn_prefill_exact through
skw_debug_xattn_exact.  Every launch in both output forms (f16 rows, raw f32).  Every K / V position a kernel must not use is poisoned (NaN; 1000.0 in V where the kernel multiplies
it by p = 0) and the output starts as a sentinel that must survive wherever no row may be written.

Of the 1500-key encoder cases the first two and the last two 64-query tiles and 64 seeded rows of every (slot, head) are compared bit for bit (the restatement's CPU time is what
bounds it); every other row must be finite and within attn_ref_lib's derived bound of float64.

The last test prints, per kernel and output form, launches / outputs compared / mismatches (pytest -s); profiles/attn_exact/README.md is where a run's table belongs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_exact_ref_lib as ax  # noqa: E402
import attn_ref_lib as ar  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = ax.cases()
KERNELS = ("k_attn_encoder", "k_attn_encoder_v3", "k_dec_attn<7>", "k_dec_cross_attn<24,4,3>", "k_xattn_prefill_exact")
COVER = {}                                # (kernel, "f16" | "f32") -> [launches, outputs compared bit for bit, mismatches]
_PREPARED = {}                            # case name -> operands, expectations, the float64 reference of the rows without a bit-exact one: computed once, never modified


@pytest.fixture(scope="module")
def ctx(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path); c = engine.Context(m, max_batch=1, max_samples=16000)
    yield c
    c.close(); m.close()


def _prepared(case):
    if case.name not in _PREPARED:
        Q, K, V = case.operands()
        recs = ax.expected(case, (Q, K, V))
        loose = []
        for g in case.groups:
            rest = np.flatnonzero(~g.exact)
            for h in range(case.H if rest.size else 0):
                sl = slice(h * 64, h * 64 + 64)
                ref, bound, _ = ar.reference(Q[g.qrows[rest], sl], K[g.slot, :g.n, sl], V[g.slot, :g.n, sl], float(case.scale))
                loose.append((g.orows[rest], sl, ref, bound))
        for a in (Q, K, V):
            a.setflags(write=False)
        _PREPARED[case.name] = (Q, K, V, recs, loose)
    return _PREPARED[case.name]


def _check(case, kernel, f32_out, got):
    """got: uint16 (f16 bits, natural order) or uint32 (f32 bits) [n_out][H*64]: every expected output bit for bit, every row no query owns still the sentinel"""
    _, _, _, recs, loose = _prepared(case)
    assert got.shape == (case.n_out, case.H * 64) and got.dtype == (np.uint32 if f32_out else np.uint16)
    cov = COVER.setdefault((kernel, "f32" if f32_out else "f16"), [0, 0, 0])
    cov[0] += 1
    sent = np.uint32(ax.SENTINEL * 0x10001) if f32_out else np.uint16(ax.SENTINEL)
    assert (got[~case.written()] == sent).all(), "%s %s: a row the kernel must leave alone was written" % (case.name, kernel)
    first = None
    for rec in recs:
        g, h = rec["group"], rec["head"]
        want = rec["out32"].view(np.uint32) if f32_out else ax.stored_f16(rec["out32"])
        have = got[g.orows[rec["rows"]], h * 64:h * 64 + 64]
        bad = np.argwhere(have != want)
        cov[1] += want.size; cov[2] += len(bad)
        if len(bad) and first is None:
            i, c = bad[0]
            first = "%d outputs differ in slot %d (%d keys) head %d, first at query %d channel %d: kernel %x, contract %x" % (len(bad), g.slot, g.n, h, rec["rows"][i], c, have[i, c], want[i, c])
    assert first is None, "%s %s %s: %s" % (case.name, kernel, "f32" if f32_out else "f16", first)
    for orows, sl, ref, bound in loose:
        v = got[orows, sl].view(np.float32 if f32_out else np.float16).astype(np.float64)
        assert np.isfinite(v).all() and (np.abs(v - ref) <= bound).all(), "%s %s: a row outside the bit-exact subset is %.3f of the float64 bound" % (
            case.name, kernel, float((np.abs(v - ref) / bound).max()))


def _launch_attn(ctx, case, form, f32_out, raw=False, **kw):
    Q, K, V, _, _ = _prepared(case)
    k_pad, v_pad = case.pads()
    q = case.q_bits(Q)
    try:
        return ctx.attn_exact(form, case.H, case.n_ctx, q.reshape(K.shape) if form == "encoder" else q, K, V, case.fill_from, f32_out=f32_out, raw=raw, k_pad=k_pad, v_pad=v_pad,
                              sentinel=ax.SENTINEL, **kw)
    except RuntimeError as e:                                              # a launch the device refused or faulted on: nothing more runs on it in this session
        pytest.exit("%s %s f32_out %d: %s" % (case.name, form, f32_out, e), returncode=3)


def _raw_is_kperm(case, got, raw):
    """the f16 rows as the kernel leaves them are the un-permuted ones in kperm order"""
    assert np.array_equal(raw[:, ax.kperm(np.arange(case.H * 64))], got), "%s: the raw f16 rows are not the kperm image of the un-permuted ones" % case.name


@pytest.mark.parametrize("case", [c for c in CASES if c.kernel in ("enc3", "encv3")], ids=lambda c: c.name)
def test_encoder_attention(ctx, case):
    want_kernel = "k_attn_encoder_v3" if case.kernel == "encv3" else "k_attn_encoder"
    kw = dict(slot_k=case.launch["slot_k"], out_rows=case.launch["out_rows"])
    got = {}
    for f32_out in (False, True):
        got[f32_out], kernel = _launch_attn(ctx, case, "encoder", f32_out, **kw)
        assert kernel == want_kernel, "%s: the launcher chose %s" % (case.name, kernel)
        _check(case, kernel, f32_out, got[f32_out])
    if case.kernel == "enc3":
        _raw_is_kperm(case, got[False], _launch_attn(ctx, case, "encoder", False, raw=True, **kw)[0])


@pytest.mark.parametrize("case", [c for c in CASES if c.kernel == "self"], ids=lambda c: c.name)
def test_decoder_self_attention(ctx, case):
    kw = {k: case.launch[k] for k in ("pos", "active", "seq")}
    got = {}
    for f32_out in (False, True):
        got[f32_out], _ = _launch_attn(ctx, case, "self", f32_out, **kw)
        _check(case, "k_dec_attn<7>", f32_out, got[f32_out])
    _raw_is_kperm(case, got[False], _launch_attn(ctx, case, "self", False, raw=True, **kw)[0])


@pytest.mark.parametrize("case", [c for c in CASES if c.kernel == "cross"], ids=lambda c: c.name)
def test_decoder_cross_attention_single_and_multi_query(ctx, case):
    Q, K, V, _, _ = _prepared(case)
    L = case.launch
    d = case.H * 64
    for mq, kernel in ((0, "k_dec_cross_attn<24,4,3>"), (1, "k_xattn_prefill_exact")):
        for f32_out in (False, True):
            try:
                raw = ctx.xattn_exact(mq, case.H, case.n_ctx, case.q_bits(Q), K, V, case.fill_from, L["row0"], L["nq"], L["slot"], slot_k=L["slot_k"], f32_out=f32_out,
                                      k_pad=ax.F16_NAN, v_pad=ax.F16_NAN, sentinel=ax.SENTINEL)
            except RuntimeError as e:                                      # a launch the device refused or faulted on: nothing more runs on it in this session
                pytest.exit("%s mq %d f32_out %d: %s" % (case.name, mq, f32_out, e), returncode=3)
            got = np.ascontiguousarray(raw).view(np.uint32) if f32_out else raw[:, ax.kperm(np.arange(d))]
            _check(case, kernel, f32_out, got)


def test_every_kernel_was_compared_in_both_output_forms():
    print("\nexact attention kernels against the contract, launches / outputs compared bit for bit / mismatches:")
    for k in KERNELS:
        print("  %-26s %s" % (k, "   ".join("%s %d / %d / %d" % ((f,) + tuple(COVER.get((k, f), (0, 0, 0)))) for f in ("f16", "f32"))))
    missing = [(k, f) for k in KERNELS for f in ("f16", "f32") if COVER.get((k, f), [0, 0, 0])[1] == 0]
    assert not missing, "never compared: %s" % missing
    assert sum(c[2] for c in COVER.values()) == 0
