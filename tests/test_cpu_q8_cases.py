"""CPU tier of the q8 kernel tests: the numpy reference of tests/q8_ref_lib.py is the description (it equals the scalar restatement and the oracle's C bit for bit, single sum and
four runs), and the cases of tests/test_gpu_q8.py can tell a wrong kernel from a right one — conditions on the operands, checked with the reference alone:
  * the four-run sum differs from the single sum in some output bits wherever a run holds more than one block;
  * without the m * s term, or with a block's dw, dy or sy taken from the neighbouring block, bits change;
  * on the order cases the per-block forms (sumi dw) dy and (dw dy) sumi differ in at least 64 outputs for each of q4_0, q5_0 and q8_0 (with plain normal operands they differ
    in none for q4_0: dw dy is a product of two f16 values, and sumi dw is exact while sumi stays under about 2^13);
and the shapes are what the case table says they are there for (arithmetic facts about M, N, K; the dispatcher is not restated)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import q8_ref_lib as q8

CASES = q8.cases()
TEETH_ROWS = 64           # the conditions are per row: on the big cases they are looked for in the first rows and the edge rows


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _case(M, N, K):
    return next(c for c in CASES if (c.M, c.N, c.K) == (M, N, K))


def _oracle(kind, blocks, N, K, A, nseg):
    out = np.full((A.shape[0], N), np.nan, np.float32)
    buf = (C.c_uint8 * len(blocks)).from_buffer_copy(blocks)
    A = np.ascontiguousarray(A, np.float32)
    assert oracle_lib.lib().skwo_debug_linear_q8_seg(q8.TYPES[kind], buf, N, K, A.ctypes.data, A.shape[0], nseg, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("nseg", [1, 4])
@pytest.mark.parametrize("kind", q8.KINDS)
def test_vectorised_reference_equals_the_scalar_restatement(kind, nseg):
    """shapes small enough for the scalar loops: a few rows of the order case (saturated blocks), the bps 3 case with its edge rows, and an odd block count for the single sum"""
    shapes = [(_case(5, 104, 384), slice(None)), (_case(200, 136, 128), slice(0, 6))]
    if nseg == 1:
        shapes.append((_case(70, 136, 96), slice(64, 70)))
    for case, rows in shapes:
        blocks, A = q8.operands(case, kind)
        A = np.ascontiguousarray(A[rows])
        want = q8.np_q8_mul_mat_seg(kind, blocks, case.N, case.K, A, nseg)
        got = q8.mul_mat(kind, blocks, case.N, case.K, A, nseg)
        assert np.array_equal(_bits(got), _bits(want)), q8.case_id(case)


def test_quantize_rows_edges():
    """the zero block (d = 0, id = 0), ties away from zero, and s from the unrounded d"""
    A = np.zeros((2, 64), np.float32)
    A[0, :32] = np.linspace(-127, 127, 32, dtype=np.float32) * 0.5
    A[1, 32:] = 3.0
    q, d, s = q8.quantize_rows(A)
    assert np.array_equal(q[0, 0], np.sign(A[0, :32] * 2) * np.floor(np.abs(A[0, :32] * 2) + 0.5)) and (q[0, 1] == 0).all() and d[0, 1] == 0 and s[0, 1] == 0
    assert (q[1, 1] == 127).all() and d[1, 1] == np.float32(np.float16(np.float32(3.0) / np.float32(127)))
    assert s[1, 1] == np.float32(np.float16(np.float32(127 * 32) * (np.float32(3.0) / np.float32(127))))


SMALL = [c for c in CASES if c.M * c.N * c.K <= 37 * 136 * 1536 and c.cls != "vocabulary"]


@pytest.mark.parametrize("kind", q8.KINDS)
@pytest.mark.parametrize("case", SMALL, ids=q8.case_id)
def test_oracle_equals_the_reference_single_sum_and_four_runs(case, kind):
    assert (37, 136, 1536) in [(c.M, c.N, c.K) for c in SMALL] and sum(c.order for c in SMALL) == 2
    blocks, A = q8.operands(case, kind)
    for nseg in (1, 4):
        if (case.K // 32) % nseg:
            continue
        got = _oracle(kind, blocks, case.N, case.K, A, nseg)
        want = q8.mul_mat(kind, blocks, case.N, case.K, A, nseg)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), "%s %s nseg %d: %d outputs differ, first (m, n) = %s" % (q8.case_id(case), kind, nseg, bad.sum(), np.argwhere(bad)[0])


@pytest.mark.parametrize("case", CASES, ids=q8.case_id)
def test_operands_tell_wrong_arithmetic_from_right(case):
    for kind in case.kinds:
        blocks, A = q8.operands(case, kind)
        if case.M > TEETH_ROWS + 8:
            A = np.ascontiguousarray(np.concatenate([A[:TEETH_ROWS], A[-8:]]))
        N, K, nb = case.N, case.K, case.K // 32
        nseg = 4 if case.segmented else 1
        ref = q8.mul_mat(kind, blocks, N, K, A, nseg)
        differs = lambda **kw: int((_bits(q8.mul_mat(kind, blocks, N, K, A, kw.pop("nseg", nseg), **kw)) != _bits(ref)).sum())
        if case.segmented and nb // 4 >= 2:
            assert differs(nseg=1) > 0, "%s: the four-run sum equals the single sum" % kind
        if nb > 1:
            assert differs(shift="dw") > 0 and differs(shift="dy") > 0, "%s: a scale from the neighbouring block goes unseen" % kind
        if q8.FORM[kind] == 3:
            assert differs(drop_ms=True) > 0, "%s: the m * s term goes unseen" % kind
            if nb > 1:
                assert differs(shift="sy") > 0, "%s: sy from the neighbouring block goes unseen" % kind


@pytest.mark.parametrize("case", [c for c in CASES if c.order], ids=q8.case_id)
def test_order_cases_pin_the_order_of_multiplications(case):
    for kind in ("q4_0", "q5_0", "q8_0"):
        blocks, A = q8.operands(case, kind)
        nseg = 4 if case.segmented else 1
        f1 = q8.mul_mat(kind, blocks, case.N, case.K, A, nseg, form=1); f2 = q8.mul_mat(kind, blocks, case.N, case.K, A, nseg, form=2)
        n = int((_bits(f1) != _bits(f2)).sum())
        print("%s %s: forms 1 and 2 differ in %d of %d outputs" % (q8.case_id(case), kind, n, f1.size))
        assert n >= 64


def test_plain_operands_do_not_pin_the_order_for_q4_0():
    """why the order block exists: without it (the model-level tests' kind of operands) a q4_0 kernel running form 2 returns form 1's bits"""
    case = _case(70, 136, 96)
    blocks, A = q8.operands(case, "q4_0")
    A = A[:case.M - 3]                                                         # (without the edge rows)
    assert np.array_equal(_bits(q8.mul_mat("q4_0", blocks, case.N, case.K, A, form=1)), _bits(q8.mul_mat("q4_0", blocks, case.N, case.K, A, form=2)))


def test_every_case_carries_the_quantiser_edges():
    for case in CASES:
        _, A = q8.operands(case, case.kinds[0])
        zero, zblock, ties = q8.edge_rows(case.M, case.K // 32)
        assert A.shape == (case.M, case.K) and A.dtype == np.float32 and np.isfinite(A).all()
        if case.M >= 3:
            assert None not in (zero, zblock, ties) and len({zero, zblock, ties}) == 3
        if zero is not None:
            assert not A[zero].any()
        if zblock is not None:
            assert not A[zblock, -32:].any() and (case.K == 32 or A[zblock, :32].any())
        t = min(1, case.K // 32 - 1); x = A[ties, t * 32:(t + 1) * 32]
        v = x * (np.float32(1) / (np.abs(x).max() / np.float32(127)))
        assert (np.abs(v - np.trunc(v)) == 0.5).sum() == 31 and q8.quantize_rows(x[None, :])[2][0, 0] != 0
        if case.K > 32:
            assert np.array_equal(A[ties, :32], np.linspace(-127, 127, 32, dtype=np.float32) * 0.5)


def test_case_list_reaches_what_its_table_claims():
    by = {(c.M, c.N, c.K): c for c in CASES}
    assert len(by) == len(CASES) == 20
    for c in CASES:
        assert c.K % 32 == 0 and (c.kinds == tuple(q8.KINDS) or c.cls == "vocabulary")
        if c.segmented:                                                        # four runs of bps blocks; UB 6 holds bps <= 6 in one round, UB 8 takes the longer ones
            assert c.K % 128 == 0 and c.M <= 4096 and ((c.K // 128 <= 6) == (c.kernel == q8.K_SMALL6))
        elif c.kernel == q8.K_TW2:
            assert c.M < 1024
        elif c.kernel == q8.K_TW4:
            assert c.M >= 1024 and (c.N % 128 or c.K % 64 or c.M % 4)
        else:
            assert c.kernel == q8.K_LDS and c.M >= 1024 and c.N % 128 == 0 and c.K % 64 == 0 and c.M % 4 == 0
    bps = lambda c: c.K // 128
    assert bps(by[1, 16, 128]) == 1 and by[1, 16, 128].M == 1
    assert bps(by[5, 104, 384]) == 3 and 104 % 16 != 0 and 6 % 3 == 0
    assert bps(by[17, 384, 768]) == 6 and 16 < 17 < 32
    assert bps(by[200, 136, 128]) == 1 and by[200, 136, 128].order and 136 % 16 != 0
    assert by[300, 384, 384].M >= 256 and 300 % 16 != 0
    assert bps(by[64, 384, 1024]) == 8
    assert bps(by[37, 136, 1536]) == 12 and 8 < 12 < 16 and 37 % 16 != 0
    assert bps(by[16, 128, 3072]) == 24 == 3 * 8
    v = by[9, 51865, 384]
    assert v.N % 2 == 1 and (v.N + 63) // 64 * 64 == 51904 and v.kinds == ("q4_0", "q5_1") and bps(v) == 3
    assert by[1, 64, 32].K // 32 == 1
    assert 70 % 64 and 136 % 64 and (96 // 32) % 2 == 1 and 70 > 64 and 136 > 128
    assert by[200, 136, 96].order
    assert by[1023, 384, 384].M == 1024 - 1
    assert 1026 % 4 and 192 % 128 and 96 % 64
    assert 200 % 128 and 1500 % 4 == 0 and 384 % 64 == 0                       # not staged for its ragged feature tile alone
    stages = {k: k[2] // 64 for k in by if by[k].kernel == q8.K_LDS}
    assert stages[1024, 128, 64] == 1 and 1024 % 128 == 0
    assert stages[1028, 256, 192] == 3 and 1028 % 128 == 4
    assert stages[1500, 384, 384] == 6 and stages[1500, 1536, 384] == 6 and stages[1500, 384, 1536] == 24 and 1500 % 128 not in (0, 4)
    assert any(s % 2 for s in stages.values()) and any(s % 2 == 0 for s in stages.values())
    for c in CASES:                                                            # the order block needs its 32 features and a fourth of the rows
        assert not c.order or (c.N >= q8.ORDER_FEATURES and c.M >= 64)


def test_epilogue_cases_cover_the_engine_calls_and_write_each_output_once():
    ecs = q8.epi_cases()
    assert {(e.name.split("-")[0], e.epi) for e in ecs} == (
        {(k, e) for k in ("plain", "staged") for e in (q8.EPI_F32, q8.EPI_GELU_F32, q8.EPI_HEADS_F16, q8.EPI_VT_F16, q8.EPI_F16_PLAIN)} |
        {("segmented", e) for e in (q8.EPI_DEC_QKV, q8.EPI_F32, q8.EPI_GELU_F32, q8.EPI_F16_PLAIN)})
    rng = np.random.default_rng(3)
    for e in ecs:
        if e.M > 512:
            continue                                                           # (the same code at the plain case's size)
        S = (rng.standard_normal((e.M, e.N)) + 3.0).astype(np.float32)
        if e.epi in (q8.EPI_F32, q8.EPI_GELU_F32):
            bufs = [np.full(e.M * (e.N + 8), np.nan, np.float32)]; kw = dict(ldc=e.N + 8, gelu=lambda v: v)
        elif e.epi == q8.EPI_F16_PLAIN:
            bufs = [np.zeros(e.M * (e.N + 8), np.uint16)]; kw = dict(ldc=e.N + 8, scale=0.5, has_scale=1)
        elif e.epi == q8.EPI_DEC_QKV:
            d = e.N // 3; bufs = [np.zeros(e.M * d, np.uint16), np.zeros(e.M * 8 * d, np.uint16), np.zeros(e.M * 8 * d, np.uint16)]
            kw = dict(ldc=d, ldc2=8 * d, pos=np.arange(e.M) % 8, scale=0.5)
        else:
            bufs = [np.zeros((e.M // e.n_ctx) * e.H * e.Tpad * 64, np.uint16)]; kw = dict(n_ctx=e.n_ctx, H=e.H, Tpad=e.Tpad)
        out = q8.epilogue(e.epi, S, bufs, **kw)
        changed = sum(int((o.view(np.uint8) != b.view(np.uint8)).reshape(o.size, -1).any(axis=1).sum()) for o, b in zip(out, bufs))
        assert changed == e.M * e.N, e.name
