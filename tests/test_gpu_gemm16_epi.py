"""The f16_mfma GEMM kernels (skw_kernels_f16.hip), each on its own with every epilogue it has, against the numpy restatement of tests/gemm16_ref_lib.py — bit for bit, except
GELU, whose hardware exp2 / reciprocal no CPU restates: there every output must be the float64 value's exact f16 or one of the two f16 values adjacent to it, and at most 1 % of a
case's outputs may be the farther of the two (gemm16_ref_lib.gelu_verdict).  tests/test_cpu_gemm16_cases.py shows on the CPU that the cases cover every launch of the engine and tell
the named wrong epilogues (scale before bias, rounding before the scale, bias by memory position, pad keys not zeroed, pos of row 0, a short LayerNorm mean, one K chain) from the right.

What runs, through the public launchers (skw_debug_gemm16_epi: the dispatch is part of what is tested, and the launch reports the kernel the launcher itself picked): k_gemm16w and
k_gemm16 — both against the reference, not against each other — k_gemm16_small with its weights as rows and as the fragment-order image, k_gemm16_small_lnA in its four register
forms, k_gemm16_vocab and the small kernel forced in its place.  Every output buffer starts as a sentinel with margins past M, N, the clips and the caches, and every byte a launch
may not write must still hold it.  The closing test prints the number of bitwise and GELU cases and the GELU shares."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm16_ref_lib as g  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = g.cases()
COUNT = {"bitwise": 0, "gelu": 0, "outputs": 0}
SHARES = {}                                 # GELU case id -> share of outputs that are not the nearest f16, per run
_PREP = {}


@pytest.fixture(scope="module")
def ctx(tiny_model_path, eng):
    m = eng.Model(tiny_model_path); c = eng.Context(m, max_batch=1, max_samples=16000)
    c.set_precision("f16_mfma")
    yield c
    c.close(); m.close()


def _prep(c):
    if c not in _PREP:
        if len(_PREP) >= 2:
            _PREP.clear()
        _PREP[c] = g.Prepared(c)
    return _PREP[c]


def _launch(ctx, what, **kw):
    try:
        return ctx.gemm16_epi(**kw)
    except RuntimeError as e:                                              # a launch the device refused or faulted on: nothing more runs on it in this session
        pytest.exit("%s: %s" % (what, e), returncode=3)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(c, run, p, got, want, masks, pre):
    what = "%s %s" % (g.case_id(c), g.run_id(run))
    for name, gb, wb, mk in zip(("C", "C2", "C3"), got, want, masks):
        gb = gb.view(wb.dtype)
        untouched = _bits(gb)[~mk] == _bits(wb)[~mk]
        assert untouched.all(), "%s: %d elements of %s outside the launch's outputs were written, first at flat index %d" % (what, (~untouched).sum(), name, np.flatnonzero(~mk)[~untouched][0])
        if pre is None:
            bad = np.flatnonzero(_bits(gb) != _bits(wb))
            assert bad.size == 0, "%s: %d of %d elements of %s differ, first at flat index %d: got 0x%x, want 0x%x" % (
                what, bad.size, int(mk.sum()), name, bad[0], int(_bits(gb)[bad[0]]), int(_bits(wb)[bad[0]]))
    if pre is None:
        COUNT["bitwise"] += 1; COUNT["outputs"] += sum(int(m.sum()) for m in masks)
        return
    off, x16, pe = pre
    out = got[0].view(want[0].dtype)[off]
    ok, far = g.gelu_verdict(out if pe is not None else out.view(np.float16), x16, pe)
    share = float(far.mean())
    SHARES.setdefault(g.case_id(c), {})[g.run_id(run)] = share
    print("%s: %d GELU outputs, not the nearest f16: %d (%.4f %%), outside the two adjacent f16 values: %d" % (what, far.size, int(far.sum()), 100 * share, int((~ok).sum())))
    assert ok.all(), "%s: %d outputs are neither of the two f16 values adjacent to float64 GELU, first at (m, n) = %s" % (what, (~ok).sum(), np.argwhere(~ok)[0])
    assert share <= g.GELU_CAP, "%s: %.3f %% of the outputs are not the nearest f16" % (what, 100 * share)
    COUNT["gelu"] += 1; COUNT["outputs"] += far.size


def _run_case(ctx, c, run):
    p = _prep(c)
    launcher, wf, forced, split = run
    rc, kid, C, C2, C3 = _launch(ctx, g.case_id(c), **p.launch_kwargs(run))
    if c.refuse:
        assert rc == -2 and kid == -1, "%s (%s): the launcher must refuse, returned %d and kernel %s" % (g.case_id(c), c.refuse, rc, g.kernel_name(kid))
        assert np.array_equal(C.view(np.uint8), p.bufs[0].view(np.uint8))
        return
    assert rc == 0, "%s %s: the launcher refused a geometry the engine uses (%s)" % (g.case_id(c), g.run_id(run), ctx.last_error())
    if c.family == "big":
        assert (kid == g.K_W) == (launcher == g.L_W) and kid in (g.K_W, g.K_LDS_256, g.K_LDS_128)
    else:
        want_k = g.K_SMALL_64 if forced else c.kernel
        assert kid == want_k, "%s: the dispatcher picked %s, the case is there for %s" % (g.case_id(c), g.kernel_name(kid), g.kernel_name(want_k))
    want, masks, pre = g.expected(p, g.accumulator(p, split))
    _check(c, run, p, [b for b in (C, C2, C3) if b is not None], want, masks, pre)
    return C


def _params(family):
    return [pytest.param(c, r, id="%s-%s" % (c.name, g.run_id(r))) for c in CASES if c.family == family for r in g.runs(c)]


@pytest.mark.parametrize("c,run", _params("big"))
def test_big_kernels_epilogues(ctx, c, run):
    """k_gemm16w and k_gemm16: epi_value, epi_chunk_offset and the staged write-out at one tile, ragged rows, ragged row and feature tiles with an odd number of K steps, M < 128,
    and the per-clip layouts (heads, V^T with its zeroed pad keys, ROWPAD, conv2's overlapping rows, the fragment-order cross K / V^T) at two clip geometries"""
    _run_case(ctx, c, run)


@pytest.mark.parametrize("c,run", _params("small"))
def test_small_kernel_epilogues(ctx, c, run):
    """k_gemm16_small / gemm16_small_finish: the residual that aliases C, the scalar path of an odd ldc, A as a fragment-order image with NaN pad rows, c_frag, EPI_DEC_QKV
    appending at pos[m]; and the refusal of a fragment-order weight image whose N is no multiple of 16"""
    _run_case(ctx, c, run)


@pytest.mark.parametrize("c,run", _params("lna"))
def test_lnA_kernel(ctx, c, run):
    """k_gemm16_small_lnA: every output bit-identical to the restatement (f64 one-pass statistics in the kernel's order of additions, the variance clamp, two float32 fmas, one f16
    rounding; then the small kernel's sums and epilogues).  No instruction is exempted: the bitwise assertion stands as written."""
    _run_case(ctx, c, run)


@pytest.mark.parametrize("c,run", _params("vocab"))
def test_vocab_kernel(ctx, c, run):
    """k_gemm16_vocab (one chain over the whole K) and k_gemm16_small forced in its place (four K quarters): ragged last strip, odd ldc, the RD 12 / 20 / 4 rings, both LDS forms"""
    _run_case(ctx, c, run)


def test_fc1_image_feeds_fc2_like_its_rows(ctx):
    """the fragment-order hand-over: fc1's c_frag image, as the GPU wrote it, fed as fc2's a_frag operand gives the bytes of the same product fed from fc1's rows — and both equal
    the reference computed from those rows"""
    fc1 = next(c for c in CASES if c.name == "gelu-5x1536x384"); fc1f = next(c for c in CASES if c.name == "gelu-5x1536x384-cfrag")
    run = (g.L_SMALL, True, False, 4)
    rows = _run_case(ctx, fc1, run).view(np.uint16); img = _run_case(ctx, fc1f, run).view(np.uint16)
    M, N = fc1.M, fc1.N; p1 = _prep(fc1)
    H = np.ascontiguousarray(rows.reshape(-1, p1.ldc)[:M, :N])                                         # fc1's output rows, in memory (kperm) order: fc2's K axis
    m, pp = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    assert np.array_equal(img[g.afrag_off(m, pp, N)], H), "the image and the rows of one fc1 product hold different values"
    _, W2 = g.gemm_operands(77, 1, 384, N)
    rng = np.random.default_rng(78); bias = rng.standard_normal(384).astype(np.float32); res = (rng.standard_normal((M, 384)) * 4).astype(np.float32)
    ldc = 384 + g.MARGIN_COLS
    buf = np.full((M + g.MARGIN_ROWS) * ldc * 4, g.SENT8, np.uint8).view(np.float32).copy(); buf.reshape(-1, ldc)[:M, :384] = res
    kw = dict(launcher=g.L_SMALL, N=384, K=N, epi=g.EPI_F32, W=W2, C_buf=buf, M=M, use_wf=True, bias=bias, res_alias=True, ldc=ldc)
    rc_r, kid_r, C_r, _, _ = _launch(ctx, "fc2 from rows", A=H, lda=N, **kw)
    rc_f, kid_f, C_f, _, _ = _launch(ctx, "fc2 from the image", A=img[:16 * N], a_frag=True, **kw)
    assert (rc_r, rc_f) == (0, 0) and kid_r == kid_f == g.K_SMALL_16
    assert np.array_equal(C_r.view(np.uint32), C_f.view(np.uint32))
    want = buf.copy(); want.reshape(-1, ldc)[:M, :384] = (g.ol.gemm_f16mfma(H, W2, 4) + bias[None, :]) + res
    assert np.array_equal(C_r.view(np.uint32), want.view(np.uint32))
    COUNT["bitwise"] += 2; COUNT["outputs"] += 2 * M * 384


def test_entry_checks_indices_on_the_host_before_launching(ctx):
    """geometries whose epilogue would leave a buffer are answered with -1 and a message, and nothing is launched: a kperm'ed output whose width is no multiple of 32 (its bias index
    would pass N), an output buffer one row short, a cache position past the cache"""
    M, N, K = g.BAD_KPERM_WIDTH
    x, gain, b, _ = g.ln_rows(1, M, K); _, W = g.gemm_operands(1, 1, N, K)
    buf = np.full(M * N, 0x5A5A, np.uint16)
    with pytest.raises(RuntimeError, match="N % 32"):
        ctx.gemm16_epi(launcher=g.L_LNA, N=N, K=K, epi=g.EPI_GELU_F16_KPERM, W=W, C_buf=buf, ln=(x, gain, b), bias=np.zeros(N, np.float32), ldc=N)
    c = next(c for c in CASES if c.name == "f32-bias-128x256x64"); p = _prep(c); kw = p.launch_kwargs((g.L_LDS, False, False, 1))
    kw["C_buf"] = p.bufs[0][:(c.M - 1) * p.ldc]
    with pytest.raises(RuntimeError, match="C too small"):
        ctx.gemm16_epi(**kw)
    c = next(c for c in CASES if c.name == "qkv-5x1152x384" and c.family == "small"); p = _prep(c); kw = p.launch_kwargs((g.L_SMALL, False, False, 4))
    kw["pos"] = p.pos.copy(); kw["pos"][-1] = 10 * g.N_TEXT_CTX
    with pytest.raises(RuntimeError, match="cache position"):
        ctx.gemm16_epi(**kw)


def test_case_counts_and_gelu_shares():
    print("\nf16 GEMM launches held to the reference: %d bitwise, %d GELU (faithful rounding, at most %.0f %% not nearest); %d outputs compared" % (
        COUNT["bitwise"], COUNT["gelu"], 100 * g.GELU_CAP, COUNT["outputs"]))
    for cid in sorted(SHARES):
        print("  %-48s %s" % (cid, "   ".join("%s %.4f %%" % (r, 100 * s) for r, s in sorted(SHARES[cid].items()))))
    n_runs = sum(len(g.runs(c)) for c in CASES if not c.refuse)
    assert COUNT["bitwise"] + COUNT["gelu"] == n_runs + 4, "a case did not run"                 # (+ 4: the hand-over test runs fc1 twice and fc2 twice more)
    assert COUNT["gelu"] == sum(len(g.runs(c)) for c in CASES if g.is_gelu(c)) + 2
