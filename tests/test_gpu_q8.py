"""The ggml-arithmetic kernels for quantised files (skw_kernels_q8.hip), each on its own against the numpy restatement of tests/q8_ref_lib.py — bit for bit: that is the
project's contract for this path, not a tolerance.  tests/test_cpu_q8_cases.py shows on the CPU that the reference equals the scalar restatement and the oracle, and that these
cases tell a wrong per-block form, a scale from the neighbouring block, a dropped m * s term or a single sum in place of the four runs from the right arithmetic.

What runs, through the engine's own path (skw_debug_gemm_q8: the model loader's repack, skw_q8_quantize, skw_gemm_q8 with its dispatch): k_gemm_q8_small<UB 6 | 8>,
k_gemm_q8<TW 2 | 4> and k_gemm_q8_lds, each in all three per-block forms, at the shapes of q8_ref_lib.cases(); the six epilogues at one shape per class; k_q8_quantize and the
in-kernel quantiser of k_dec_attn against quantize_rows (and that launch's f32 rows against the attention contract's restatement).  The launch reports the kernel the dispatcher picked (the function the launcher itself branches on), every output buffer
starts as a sentinel with a margin past M and N that must come back untouched, and the closing test asserts that every kernel ran in every form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_ref_lib as q8  # noqa: E402
import attn_exact_ref_lib as ax  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = q8.cases()
EPI_CASES = q8.epi_cases()
SENT8 = 0x5A
MARGIN_ROWS, MARGIN_COLS = 3, 8
COVER = {}                                 # (kernel id, form) -> [cases, outputs compared]
_REF = {}


@pytest.fixture(scope="module")
def ctx(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path); c = engine.Context(m, max_batch=1, max_samples=16000)
    yield c
    c.close(); m.close()


def _sentinel(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, SENT8, np.uint8).view(dtype)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _prepared(case, kind):
    """operands and the reference sums: computed once per (case, kind), shared by the tests that need them, never modified"""
    key = (case.M, case.N, case.K, bool(getattr(case, "order", False)), kind)
    if key not in _REF:
        if len(_REF) >= 4:
            _REF.clear()
        blocks, A = q8.operands(case, kind)
        S = q8.mul_mat(kind, blocks, case.N, case.K, A, 4 if case.segmented else 1)
        A.setflags(write=False); S.setflags(write=False)
        _REF[key] = (blocks, A, S)
    return _REF[key]


def _launch(ctx, what, kind, blocks, N, K, A, segmented, epi, C_buf, **kw):
    try:
        return ctx.gemm_q8(q8.TYPES[kind], blocks, N, K, A, segmented, epi, C_buf, **kw)
    except RuntimeError as e:                                              # a launch the device refused or faulted on: nothing more runs on it in this session
        pytest.exit("%s %s: %s" % (what, kind, e), returncode=3)


def _plain_f32(ctx, case, kind):
    blocks, A, S = _prepared(case, kind)
    ldc = case.N + MARGIN_COLS
    kid, C, _, _ = _launch(ctx, q8.case_id(case), kind, blocks, case.N, case.K, A, case.segmented, q8.EPI_F32, _sentinel((case.M + MARGIN_ROWS) * ldc, np.float32), ldc=ldc)
    return kid, C.reshape(case.M + MARGIN_ROWS, ldc)


def _first_mismatch(case, kind, got, want):
    """count and the first (m, n) with the reference's partial sum of each block run there"""
    bad = got.view(np.uint32) != want.view(np.uint32)
    m, n = (int(v) for v in np.argwhere(bad)[0])
    blocks, A, _ = _prepared(case, kind)
    nb = case.K // 32; bb = q8.BLOCK_BYTES[kind]; nseg = 4 if case.segmented else 1; bps = nb // nseg
    row = np.frombuffer(blocks, np.uint8).reshape(case.N, nb, bb)[n]
    runs = [float(q8.mul_mat(kind, row[s * bps:(s + 1) * bps].tobytes(), 1, bps * 32, A[m:m + 1, s * bps * 32:(s + 1) * bps * 32])[0, 0]) for s in range(nseg)]
    return "%d of %d outputs differ; first (m, n) = (%d, %d): got %r (0x%08x), want %r (0x%08x); the reference's block runs there: %s" % (
        bad.sum(), bad.size, m, n, float(got[m, n]), got.view(np.uint32)[m, n], float(want[m, n]), want.view(np.uint32)[m, n], runs)


@pytest.mark.parametrize("case,kind", [(c, k) for c in CASES for k in c.kinds], ids=lambda v: v if isinstance(v, str) else q8.case_id(v))
def test_gemm_bits_equal_the_reference(ctx, case, kind):
    _, _, S = _prepared(case, kind)
    kid, C = _plain_f32(ctx, case, kind)
    assert kid == case.kernel, "%s: the dispatcher picked %s, the case is there for %s" % (q8.case_id(case), q8.KERNEL_NAMES[kid], q8.KERNEL_NAMES[case.kernel])
    assert (_raw(C[case.M:]) == SENT8).all() and (_raw(C[:, case.N:]) == SENT8).all(), "%s %s: the margin past M / N was written" % (q8.case_id(case), kind)
    got = np.ascontiguousarray(C[:case.M, :case.N])
    assert np.array_equal(got.view(np.uint32), S.view(np.uint32)), "%s %s (%s): %s" % (q8.case_id(case), kind, q8.KERNEL_NAMES[kid], _first_mismatch(case, kind, got, S))
    n = COVER.setdefault((kid, q8.FORM[kind]), [0, 0]); n[0] += 1; n[1] += S.size


@pytest.mark.parametrize("case,kind", [(c, k) for c in CASES if c.kernel == q8.K_LDS for k in c.kinds], ids=lambda v: v if isinstance(v, str) else q8.case_id(v))
def test_staged_cases_without_the_lds_kernel(ctx, eng, case, kind):
    """SKW_Q8_LDS=0: every staged shape runs on k_gemm_q8<4> and returns the same bytes"""
    _, _, S = _prepared(case, kind)
    kid1, C1 = _plain_f32(ctx, case, kind)
    with eng.switch("Q8_LDS", 0):
        kid0, C0 = _plain_f32(ctx, case, kind)
    assert (kid1, kid0) == (q8.K_LDS, q8.K_TW4)
    assert np.array_equal(_raw(C0), _raw(C1)), "%s %s: the register-fed kernel's bytes differ from the staged kernel's" % (q8.case_id(case), kind)
    assert np.array_equal(np.ascontiguousarray(C0[:case.M, :case.N]).view(np.uint32), S.view(np.uint32))
    n = COVER.setdefault((kid0, q8.FORM[kind]), [0, 0]); n[0] += 1; n[1] += S.size


@pytest.mark.parametrize("e,kind", [(e, k) for e in EPI_CASES for k in q8.EPI_KINDS], ids=lambda v: v if isinstance(v, str) else v.name)
def test_epilogues(ctx, e, kind):
    """the raw bytes of every output buffer, margins and untouched cache rows included, equal the numpy epilogue applied to the reference sums"""
    blocks, A, S = _prepared(e, kind)
    rng = np.random.default_rng(e.M + e.N + e.epi)
    bias = (rng.standard_normal(e.N) * 0.5).astype(np.float32) if e.bias else None
    kw = dict(bias=bias); ref_kw = dict(bias=bias)
    if e.epi in (q8.EPI_F32, q8.EPI_GELU_F32, q8.EPI_F16_PLAIN):
        ldc = e.N + MARGIN_COLS
        bufs = [_sentinel((e.M + MARGIN_ROWS) * ldc, np.float16 if e.epi == q8.EPI_F16_PLAIN else np.float32)]
        if e.epi == q8.EPI_F16_PLAIN:
            bufs[0] = bufs[0].view(np.uint16); kw.update(scale=e.scale, has_scale=1)
        kw.update(ldc=ldc)
        if e.res:                                                          # the residual aliases the output, as the engine calls it
            res = rng.standard_normal((e.M, e.N)).astype(np.float32)
            bufs[0].reshape(e.M + MARGIN_ROWS, ldc)[:e.M, :e.N] = res
            kw.update(res_alias=True); ref_kw.update(res=res)
        if e.epi == q8.EPI_GELU_F32:
            ref_kw.update(gelu=lambda v: ctx.math(4, v))                   # the device's GELU: tests/test_gpu_math.py holds it to the contract
    elif e.epi in (q8.EPI_HEADS_F16, q8.EPI_VT_F16):
        bufs = [_sentinel((e.M // e.n_ctx) * e.H * e.Tpad * 64 + 192, np.uint16)]
        kw.update(n_ctx=e.n_ctx, H=e.H, Tpad=e.Tpad)
        if e.epi == q8.EPI_HEADS_F16:
            kw.update(scale=e.scale, has_scale=1)
    else:                                                                  # EPI_DEC_QKV: q rows, and the K / V cache rows at each row's own position
        d = e.N // 3; n_text_ctx = 16; ldc = d + MARGIN_COLS
        bufs = [_sentinel((e.M + MARGIN_ROWS) * ldc, np.uint16), _sentinel((e.M + 1) * n_text_ctx * d, np.uint16), _sentinel((e.M + 1) * n_text_ctx * d, np.uint16)]
        pos = np.array([0, 3, 15, 7, 1], np.int32); assert pos.size == e.M and len(set(pos.tolist())) == e.M
        kw.update(ldc=ldc, ldc2=n_text_ctx * d, pos=pos, n_ctx=d, scale=e.scale, has_scale=1, C2_buf=bufs[1], C3_buf=bufs[2])
    ref_kw.update({k: v for k, v in kw.items() if k in ("ldc", "ldc2", "pos", "n_ctx", "H", "Tpad", "scale", "has_scale")})
    want = q8.epilogue(e.epi, S, bufs, **ref_kw)
    kid, C, C2, C3 = _launch(ctx, e.name, kind, blocks, e.N, e.K, A, e.segmented, e.epi, bufs[0], **kw)
    assert kid == e.kernel
    for name, g, w, b in zip(("C", "C2", "C3"), (C, C2, C3), want, bufs):
        assert not np.array_equal(_raw(w), _raw(b))
        bad = np.flatnonzero(g.view(w.dtype) != w) if w.dtype != np.float32 else np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s %s: %d elements of %s differ, first at flat index %d" % (e.name, kind, bad.size, name, bad[0])


def _quantiser_rows(M, K, variant):
    A = q8.activations(M * 131 + K, M, K).copy()
    if variant == "tiny":
        A[0, :32] *= np.float32(1e-30) / np.abs(A[0, :32]).max()
    elif variant == "huge":
        A[0, :32] *= np.float32(1e30) / np.abs(A[0, :32]).max()
    elif M >= 5:                                                           # "edges": the edge rows sit in the last three rows; the two extreme blocks go into rows 0 and 1
        A[0, 32:64] *= np.float32(1e-30) / np.abs(A[0, 32:64]).max()
        A[1, :32] *= np.float32(1e30) / np.abs(A[1, :32]).max()
    assert np.isfinite(A).all()
    amax = np.abs(A.reshape(M, K // 32, 32)).max(axis=2)
    assert ((amax == 0) | (amax >= 127 * np.finfo(np.float32).tiny)).all()      # below that ggml leaves the result undefined
    return A


@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("M,K,variant", [(1, 32, "edges"), (1, 32, "tiny"), (1, 32, "huge"), (5, 96, "edges"), (300, 384, "edges")])
def test_row_quantiser_equals_quantize_rows(ctx, M, K, variant, pad):
    A = _quantiser_rows(M, K, variant)
    x = np.full((M, K + pad), 3e38, np.float32); x[:, :K] = A              # what lies between the rows (ldx > K) must reach nothing
    try:
        q, dT, sT = ctx.q8_quantize(x, K)
    except RuntimeError as e:
        pytest.exit("k_q8_quantize %dx%d: %s" % (M, K, e), returncode=3)
    wq, wd, ws = q8.quantize_rows(A)
    assert np.abs(wq).max() <= 127
    assert np.array_equal(q, wq.reshape(M, K).astype(np.int8)), "q differs in %d values" % (q != wq.reshape(M, K)).sum()
    assert np.array_equal(dT.T.copy().view(np.uint32), wd.view(np.uint32)) and np.array_equal(sT.T.copy().view(np.uint32), ws.view(np.uint32))
    if variant == "huge" or M >= 5:
        assert np.isinf(wd).any()                                          # d past the f16 range rounds to infinity in both
    if variant == "tiny" or M >= 5:
        assert ((wd == 0) & (np.abs(wq).max(axis=2) == 127)).any()         # d below the f16 range rounds to zero while the block's q are full scale


@pytest.mark.parametrize("H", [4, 6])
def test_attention_q8_output_equals_quantize_rows_of_its_f32_output(ctx, H):
    """k_dec_attn's in-kernel quantiser (q8_half_wave_block: wave shuffles, fmaxf) against quantize_rows applied to what the same launch leaves with f32_out — and those f32 rows
    against the contract's restatement (tests/attn_exact_ref_lib.py), bit for bit"""
    d = H * 64; n_text_ctx = 448
    pos = np.array([0, 1, 63, 64, 447, 30, 100], np.int32); rows = pos.size
    active = np.array([1, 1, 1, 1, 1, 0, 1], np.int32)                     # row 5 is finished: its outputs stay as they were
    seq = np.array([0, 1, 2, 3, 4, 5, 2], np.int32)                        # row 6 reads sequence 2's cache (which holds 101 positions for it)
    rng = np.random.default_rng(H)
    Q = (rng.standard_normal((rows, d)) * 0.3).astype(np.float16)
    K = rng.standard_normal((rows, n_text_ctx, d)).astype(np.float16)
    V = (rng.standard_normal((rows, n_text_ctx, d)) * np.exp2(rng.integers(-2, 3, (rows, 1, H)).repeat(64, axis=2).astype(np.float64))).astype(np.float16)
    filled = np.zeros(rows, np.int64)
    for b in range(rows):
        if active[b]:
            filled[seq[b]] = max(filled[seq[b]], pos[b] + 1)
    for s in range(rows):                                                  # what no live row may use is NaN
        K[s, filled[s]:] = np.nan; V[s, filled[s]:] = np.nan
    try:
        out, q, dT, sT = ctx.self_attn_q8(H, n_text_ctx, Q, K, V, pos, active=active, seq=seq, sentinel=SENT8)
    except RuntimeError as e:
        pytest.exit("skw_dec_self_attn H = %d: %s" % (H, e), returncode=3)
    live = np.flatnonzero(active); dead = np.flatnonzero(active == 0)
    assert np.isfinite(out[live]).all() and np.abs(out[live]).max() > 0.01
    for b in live:
        for h in range(H):
            sl = slice(h * 64, h * 64 + 64)
            r = ax.attend(Q[b:b + 1, sl], K[seq[b], :pos[b] + 1, sl], V[seq[b], :pos[b] + 1, sl])
            assert not ax.order_dependent_rows(r["e"])                         # (a condition on the seeded operands: the row has one expectation)
            assert np.array_equal(out[b:b + 1, sl].view(np.uint32), r["out32"].view(np.uint32)), "row %d head %d: k_dec_attn's f32 output is not the contract's" % (b, h)
    wq, wd, ws = q8.quantize_rows(out[live])
    assert np.array_equal(q[live], wq.reshape(live.size, d).astype(np.int8))
    assert np.array_equal(dT[:, live].T.copy().view(np.uint32), wd.view(np.uint32)) and np.array_equal(sT[:, live].T.copy().view(np.uint32), ws.view(np.uint32))
    for a in (out[dead], q[dead], dT[:, dead], sT[:, dead]):
        assert (_raw(a) == SENT8).all(), "an inactive row's output was written"


def test_every_kernel_ran_in_every_form():
    print("\nq8 GEMM kernels compared bit for bit (cases / outputs), per-block form 1 | 2 | 3:")
    for kid, name in enumerate(q8.KERNEL_NAMES):
        print("  %-20s %s" % (name, "   ".join("%d / %d" % tuple(COVER.get((kid, f), (0, 0))) for f in (1, 2, 3))))
    missing = [(q8.KERNEL_NAMES[k], f) for k in range(5) for f in (1, 2, 3) if COVER.get((k, f), [0, 0])[0] == 0]
    assert not missing, "never compared: %s" % missing
