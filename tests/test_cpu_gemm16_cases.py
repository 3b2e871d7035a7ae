"""CPU tier of the f16 GEMM epilogue tests: tests/gemm16_ref_lib.py is the description of what the kernels must return, and the cases of tests/test_gpu_gemm16_epi.py can tell a
wrong kernel from a right one — conditions on the layouts, the case list and the operands, checked with the reference alone:
  * the layout functions are bijections onto the ranges they claim;
  * the case list covers every (kernel family, epilogue, flags) combination skw_engine.hip launches in f16_mfma (gemm16_ref_lib.ENGINE_LAUNCHES, enumerated by hand);
  * each named wrong variant — scale before bias, f16 rounding before the scale, bias indexed by memory position under kperm, pad keys not zeroed, pos[m] taken from row 0, a
    LayerNorm mean that leaves out the last 128 values, one K chain instead of four quarters — changes at least one output bit of every bitwise case it applies to;
  * the LayerNorm restatement lies within one f16 ulp of a float64 LayerNorm on every row, so it is not the copy of a bug;
  * the reference side of the GELU condition uses up at most half of the cap;
  * every case's reference output is finite and inside f16's range."""
import numpy as np
import pytest

import gemm16_ref_lib as g

CASES = g.cases()
LIVE = [c for c in CASES if not c.refuse]
TEETH_ROWS = 16           # the conditions are per element: on the bigger cases they are looked for in the first rows and the last ones
_PREP = {}


def _prep(c):
    if c not in _PREP:
        if len(_PREP) >= 4:
            _PREP.clear()
        _PREP[c] = g.Prepared(c)
    return _PREP[c]


def _rows(c):
    if c.epi == g.EPI_VT_F16 or c.M <= TEETH_ROWS + 4:                       # (V^T: the pad keys belong to whole clips)
        return None
    return np.concatenate([np.arange(TEETH_ROWS), np.arange(c.M - 4, c.M)])


def _split(c):
    return 4 if c.family in ("small", "lna") else 1


def test_layouts_are_bijections_onto_the_ranges_they_claim():
    k = np.arange(4096)
    assert np.array_equal(np.sort(g.kperm(k)), k) and np.array_equal(g.inv_kperm(g.kperm(k)), k) and np.array_equal(g.kperm(k) & ~31, k & ~31)
    assert g.kperm(np.array([0, 1, 2, 3, 4, 31])).tolist() == [0, 8, 16, 24, 1, 31]                 # the 8 values with k % 4 == q are contiguous at [8q, 8q + 8)
    for B, H, Tpad in [(2, 2, 160), (3, 6, 320), (1, 1, 32)]:
        size = B * H * Tpad * 64; want = np.arange(size)
        b, i, n = np.meshgrid(np.arange(B), np.arange(Tpad), np.arange(64 * H), indexing="ij")
        assert np.array_equal(np.sort(g.heads_off(b, i, n, H, Tpad).ravel()), want)
        assert np.array_equal(np.sort(g.vt_off(b, n, i, H, Tpad).ravel()), want)
        assert np.array_equal(np.sort(g.kfrag_off(b, H, Tpad, i, n).ravel()), want)
        assert np.array_equal(np.sort(g.vtfrag_off(b, H, Tpad, n, i).ravel()), want)
        # both fragment orders permute 16-byte chunks of the row layouts: eight consecutive features (K) / memory positions (V^T) stay together
        t = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
        assert (np.diff(g.kfrag_off(b, H, Tpad, i, n).reshape(-1, 8), axis=1) == 1).all() and (np.diff(g.vtfrag_off(t(b), H, Tpad, t(n), t(i)).reshape(-1, 8), axis=1) == 1).all()
    for M16, K in [(16, 128), (48, 1536), (80, 384)]:
        m, p = np.meshgrid(np.arange(M16), np.arange(K), indexing="ij")
        assert np.array_equal(np.sort(g.afrag_off(m, p, K).ravel()), np.arange(M16 * K))
        assert (g.afrag_off(m, p, K) // (16 * K) == m // 16).all()                                   # a row tile's k-blocks are consecutive KiB
    for T, B in [(150, 2), (300, 3)]:
        r = g.rowpad(np.arange(B * T), T)
        pads = np.concatenate([np.arange(B) * (T + 2), np.arange(B) * (T + 2) + T + 1])
        assert np.array_equal(np.sort(np.concatenate([r, pads])), np.arange(B * (T + 2)))
    img = g.afrag_image(np.arange(5 * 128, dtype=np.uint16).reshape(5, 128))
    assert img.size == 16 * 128 and (img == g.F16_NAN).sum() == 11 * 128


def test_case_list_covers_every_launch_of_the_engine():
    have = {g.launch_key(c) for c in LIVE}
    missing = g.ENGINE_LAUNCHES - have
    assert not missing, "launched by the engine, held by no case: %s" % sorted(missing)
    assert len({g.case_id(c) for c in CASES}) == len(CASES)
    ran = {}
    for c in LIVE:
        for r in g.runs(c):
            ran.setdefault(g.K_SMALL_64 if r[2] else c.kernel if c.kernel is not None else r[0], []).append(c)
    for k in (g.L_W, g.L_LDS, g.K_SMALL_16, g.K_SMALL_64, g.K_LNA_6_1, g.K_LNA_6_4, g.K_LNA_12_1, g.K_LNA_12_2, g.K_VOCAB + 412, g.K_VOCAB + 220, g.K_VOCAB + 404):
        assert k in ran, k
    for c in LIVE:                                                                                   # arithmetic facts the case table claims
        assert c.M * c.N * c.K <= 5e8
        if c.family == "big":
            assert c.K % 64 == 0 and c.N % 32 == 0 and ((g.L_W in c.launchers) == (c.M >= 128))
        else:
            assert c.K % 128 == 0
        if c.family == "lna":
            nkw = c.K // 128; nt4 = c.N >= 2048
            assert c.kernel == {(True, False): g.K_LNA_6_1, (True, True): g.K_LNA_6_4, (False, False): g.K_LNA_12_1, (False, True): g.K_LNA_12_2}[(nkw <= 6, nt4)] and nkw <= 12
    assert 2080 // 16 == 130 and 130 % 4 and 2080 % 32 == 0 and g.BAD_KPERM_WIDTH[1] % 32 == 16 and 333 % 128 and 416 % 128 and (192 // 64) % 2 == 1 and 390 % 4 and 391 % 4 and 8201 % 16 and 8201 % 2


@pytest.mark.parametrize("variant", g.VARIANTS)
def test_every_wrong_variant_is_seen_by_every_bitwise_case_it_applies_to(variant):
    hit = 0
    for c in LIVE:
        if not g.applicable(c, variant):
            continue
        p = _prep(c); rows = _rows(c); split = _split(c)
        acc = g.accumulator(p, split, rows=rows) if rows is not None else g.accumulator(p, split)
        good = g.expected(p, acc, rows=rows)[0]
        if variant == "split1":
            wrong = g.expected(p, g.accumulator(p, 1, rows=rows) if rows is not None else g.accumulator(p, 1), rows=rows)[0]
        elif variant == "ln_mean_short":
            wrong = g.expected(p, g.accumulator(p, split, rows=rows if rows is not None else np.arange(c.M), variant=variant), rows=rows)[0]
        else:
            wrong = g.expected(p, acc, rows=rows, variant=variant)[0]
        n = sum(int((a.view(np.uint8) != b.view(np.uint8)).sum()) for a, b in zip(good, wrong))
        assert n > 0, "%s: '%s' returns the same bytes — the case pins nothing about it" % (g.case_id(c), variant)
        hit += 1
    assert hit >= 2, "no case to tell '%s' by" % variant
    if variant == "split1":
        seen = []
        for c in g.split1_candidates(CASES):
            p = _prep(c)
            good = g.expected(p, g.accumulator(p, 4))[0]; wrong = g.expected(p, g.accumulator(p, 1))[0]
            seen.append(sum(int((a != b).sum()) for a, b in zip(good, wrong)))
        print("k_gemm16_small_lnA, f16 outputs that one K chain instead of four quarters changes, per case:", seen)
        assert max(seen) > 0


@pytest.mark.parametrize("c", [c for c in CASES if c.family == "lna"], ids=g.case_id)
def test_layernorm_restatement_is_within_one_f16_ulp_of_float64(c):
    x, gain, bias, (loud, const) = g.ln_rows(g._seed(c), c.M, c.K)
    got, md, var_raw = g.layernorm_operand(x, gain, bias)
    xd = x.astype(np.float64)
    mean = xd.mean(axis=1, keepdims=True); var = ((xd - mean) ** 2).mean(axis=1, keepdims=True)
    ref = (xd - mean) / np.sqrt(var + 1e-5) * gain.astype(np.float64) + bias.astype(np.float64)
    g16 = got.view(np.float16)
    assert np.isfinite(g16).all()
    ulp = np.maximum(np.exp2(np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -30))) - 10), 2.0 ** -24)      # the f16 spacing in the binade of the float64 value
    # What float32 itself costs: the kernel forms (x - mean) rstd as fma(x, sa, sb) with sb = -f32(mean) rstd, so an output near zero on a row whose mean is far from zero is the
    # difference of two numbers of size |mean| rstd, each carrying a float32 rounding (2^-24 relative; two of them: 2^-23).  That absolute term — from the number format, whatever the
    # order of evaluation — is allowed on top of the f16 ulp; on rows with mean 0 it is a thousandth of an ulp, on the constant row (|mean| rstd ~ 1000) it is all there is.
    # The second fma, t gain + bias, adds one float32 rounding of its own where the two terms cancel.
    t = (xd - mean) / np.sqrt(var + 1e-5)
    f32_term = 2.0 ** -23 * (np.abs(xd) + np.abs(mean)) / np.sqrt(var + 1e-5) * np.abs(gain.astype(np.float64)) + 2.0 ** -24 * (np.abs(t * gain) + np.abs(bias.astype(np.float64)))
    err = (np.abs(g16.astype(np.float64) - ref) - f32_term) / ulp
    assert err.max() <= 1.0, "row %d: %.3f f16 ulp" % (int(np.argmax(err.max(axis=1))), err.max())
    plain = np.abs(mean[:, 0]) < 1e-3 * np.sqrt(var[:, 0]) + 1e-6                                    # rows with mean 0: the float32 term is a hundredth of an ulp, and the result is
    assert plain.any() and err[plain].max() <= 0.5                                                   # the correctly rounded f16 of the float64 value
    assert np.allclose(md, mean[:, 0], rtol=0, atol=1e-9 * np.abs(xd).max())
    far = np.abs(mean[:, 0]) > 20 * np.sqrt(var[:, 0])
    assert far.any()
    if c.M >= 4:
        assert var[const, 0] < 1e-20 and np.abs(var_raw[const]) < 1e-12 and np.abs(xd[loud]).max() == 500.0
        assert np.abs(g16[const].astype(np.float64) - bias.astype(np.float64)).max() < 2e-3             # a constant row normalises to (nearly) its bias


def test_variance_clamp_is_reached():
    """a constant row whose f64 sum of squares is rounded: E[x^2] - mean^2 comes out below zero for some K, and the clamp makes the row's rstd that of variance 0"""
    neg = 0
    for K in (128, 384, 512, 768, 1024, 1536):
        for v in (3.1415927, 0.1, 7.3, 1e3 + 0.1):
            x = np.full((1, K), v, np.float32)
            A, md, var_raw = g.layernorm_operand(x, np.ones(K, np.float32), np.zeros(K, np.float32))
            neg += int(var_raw[0] < 0)
            assert np.abs(A.view(np.float16).astype(np.float64)).max() <= 1e-2
    assert neg > 0


def test_fmaf_is_correctly_rounded():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32); b = rng.standard_normal(4000).astype(np.float32); c = (rng.standard_normal(4000) * np.exp2(rng.integers(-30, 4, 4000))).astype(np.float32)
    # products that land exactly on, and a hair off, a float32 midpoint: a b = 1 + 2^-24 exactly; c pushes the sum off the tie by less than a float64 ulp
    a[:4] = np.float32(1 + 2.0 ** -12); b[:4] = np.float32(1 - 2.0 ** -12 + 2.0 ** -23); c[:4] = np.array([0, 2.0 ** -80, -2.0 ** -80, 2.0 ** -60], np.float32)
    got = g.fmaf(a, b, c)
    for i in list(range(8)) + list(range(8, 4000, 97)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact)); cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, i


GELU_CASES = [c for c in LIVE if g.is_gelu(c)]


@pytest.mark.parametrize("c", GELU_CASES, ids=g.case_id)
def test_gelu_reference_side_stays_inside_half_the_cap(c):
    """gelu16's formula in float32 with a correctly rounded exp2 and reciprocal, on the case's own pre-activations: faithful everywhere, and at most 0.5 % not nearest"""
    p = _prep(c)
    _, _, (off, x16, pe) = g.expected(p, g.accumulator(p, _split(c)))
    ok, far = g.gelu_verdict(g.gelu16_f32(x16), x16)
    share = float(far.mean())
    print("%s: %d pre-activations in [%.1f, %.1f], |x| < 4 for %.0f %%; float32 formula not nearest: %.4f %%" % (g.case_id(c), x16.size, x16.min(), x16.max(), 100 * (np.abs(x16) < 4).mean(),
                                                                                                              100 * share))
    assert ok.all() and share <= g.GELU_REF_CAP
    assert (np.abs(x16) < 4).mean() > 0.5, "most pre-activations must lie where GELU is not the identity or zero"


@pytest.mark.parametrize("c", LIVE, ids=g.case_id)
def test_reference_outputs_are_finite_and_inside_f16_range(c):
    p = _prep(c); rows = _rows(c)
    acc = g.accumulator(p, _split(c), rows=rows) if rows is not None else g.accumulator(p, _split(c))
    bufs, masks, pre = g.expected(p, acc, rows=rows)
    assert np.isfinite(acc).all()
    n_rows = c.M if rows is None else len(rows)
    written = sum(int(m.sum()) for m in masks)
    pads = (c.M // c.n_ctx) * c.N * (c.Tpad - c.n_ctx) if c.epi == g.EPI_VT_F16 else 0
    assert written == n_rows * c.N + pads, "every output element is written exactly once"
    for b, m, b0 in zip(bufs, masks, p.bufs):
        v = b[m].view(np.float16).astype(np.float32) if b.dtype == np.uint16 else b[m]
        assert np.isfinite(v).all() and np.abs(v).max() < 65504 and np.abs(v).max() > 0
        assert np.array_equal(b[~m].view(np.uint8), b0[~m].view(np.uint8))
        if c.res != "alias":
            assert (b0.view(np.uint8) == g.SENT8).all()
        assert (~m).sum() >= 64, "a margin of sentinel elements around the outputs"
