"""ggml's quantised mul_mat (include/skw_ggml_quant.h (a)) restated in numpy, the operands and the case list the q8 kernel tests run (tests/test_gpu_q8.py; tests/test_cpu_q8_cases.py
shows on the CPU that the reference and the cases have teeth).  No GPU, and none of the C code: the block layouts, the activation quantiser and the three per-block forms are
written out again here.

    unpack(kind, blocks, N, K)            int weights [N][K/32][32], d and m [N][K/32]
    quantize_rows(A)                      q [M][K/32][32] int32, d and s [M][K/32] rounded to f16 (roundf = half away from zero, taken in float64 where it is exact)
    mul_mat(kind, blocks, N, K, A, nseg)  the integer block dots as float32 matmuls (exact: |sumi| <= 32 * 127 * 128 < 2^24), the float32 update of skw_ggml_block_dot as
                                          separate numpy operations (numpy fuses nothing), block-ascending; nseg contiguous runs from zero, added in ascending order
    np_q8_mul_mat                         the same in scalar loops: slow, and obviously the description (moved here from test_cpu_oracle.py, unchanged)
    epilogue(...)                         what skw_gemm_q8's six epilogues (epi_store, skw_dev_common.h) leave in their output buffers, in numpy float32, f16 by numpy's RNE cast
    cases(), operands(case, kind)         the shapes of the dispatcher's five kernels and their seeded operands
"""
import collections
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from quantize_ggml import quantize_blocks, TYPES  # noqa: E402,F401

KINDS = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]
BLOCK_BYTES = {"q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "q8_0": 34}
FORM = {"q4_0": 1, "q5_0": 2, "q8_0": 2, "q4_1": 3, "q5_1": 3}            # skw_ggml_dot_form
# what launch_gemm_q8 reports (skw_gemm_q8_kernel, skw_kernels.h)
K_SMALL6, K_SMALL8, K_TW2, K_TW4, K_LDS = range(5)
KERNEL_NAMES = ["k_gemm_q8_small<6>", "k_gemm_q8_small<8>", "k_gemm_q8<2>", "k_gemm_q8<4>", "k_gemm_q8_lds"]
EPI_F32, EPI_HEADS_F16, EPI_VT_F16, EPI_F16_PLAIN, EPI_DEC_QKV, EPI_GELU_F32 = 0, 4, 5, 6, 8, 9      # SkwEpi


def np_q8_mul_mat(kind, blocks, n_out, n_in, A):
    """ggml's quantised mul_mat restated step by step in numpy float32 scalars (include/skw_ggml_quant.h (a)), independent of the C code."""
    f1 = np.float32
    bb = {"q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "q8_0": 34}[kind]
    nb = n_in // 32
    raw = np.frombuffer(blocks, np.uint8).reshape(n_out * nb, bb)
    qw = np.zeros((n_out * nb, 32), np.int32); dw = np.zeros(n_out * nb, np.float32); mw = np.zeros(n_out * nb, np.float32)
    for i, b in enumerate(raw):
        o = 0
        dw[i] = np.frombuffer(b[o:o + 2].tobytes(), np.float16)[0]; o += 2
        if kind in ("q4_1", "q5_1"):
            mw[i] = np.frombuffer(b[o:o + 2].tobytes(), np.float16)[0]; o += 2
        qh = 0
        if kind in ("q5_0", "q5_1"):
            qh = struct.unpack("<I", b[o:o + 4].tobytes())[0]; o += 4
        qs = b[o:]
        if kind == "q8_0":
            qw[i] = qs.view(np.int8)
            continue
        for j in range(16):
            x0, x1 = int(qs[j]) & 15, int(qs[j]) >> 4
            if kind in ("q5_0", "q5_1"):
                x0 |= ((qh >> j) & 1) << 4; x1 |= ((qh >> (j + 16)) & 1) << 4
            off = 8 if kind == "q4_0" else 16 if kind == "q5_0" else 0
            qw[i, j], qw[i, j + 16] = x0 - off, x1 - off
    rows = A.shape[0]
    out = np.zeros((rows, n_out), np.float32)
    for r in range(rows):
        qa = np.zeros((nb, 32), np.int32); da = np.zeros(nb, np.float32); sa = np.zeros(nb, np.float32)
        for b in range(nb):
            x = A[r, b * 32:(b + 1) * 32]
            amax = f1(np.abs(x).max()); d = f1(amax / f1(127)); idv = f1(f1(1) / d) if d != 0 else f1(0)
            v = (x * idv).astype(np.float32).astype(np.float64)
            q = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)          # roundf: half away from zero (exact in f64)
            qa[b] = q; da[b] = f1(np.float16(d)); sa[b] = f1(np.float16(f1(f1(int(q.sum())) * d)))
        for n in range(n_out):
            sumf = f1(0)
            for b in range(nb):
                i = n * nb + b; sumi = int((qw[i] * qa[b]).sum())
                if kind == "q4_0":
                    t = f1(f1(f1(sumi) * dw[i]) * da[b])
                else:
                    t = f1(f1(dw[i] * da[b]) * f1(sumi))
                    if kind in ("q4_1", "q5_1"):
                        t = f1(t + f1(mw[i] * sa[b]))
                sumf = f1(sumf + t)
            out[r, n] = sumf
    return out


def np_q8_mul_mat_seg(kind, blocks, n_out, n_in, A, nseg):
    """the scalar form over nseg contiguous runs of blocks: each run is a mul_mat of its own columns from zero (blocks never straddle a run), the runs added in ascending order"""
    nb = n_in // 32; bps = nb // nseg; bb = BLOCK_BYTES[kind]
    assert nb % nseg == 0
    raw = np.frombuffer(blocks, np.uint8).reshape(n_out, nb, bb)
    total = None
    for s in range(nseg):
        part = np_q8_mul_mat(kind, np.ascontiguousarray(raw[:, s * bps:(s + 1) * bps]).tobytes(), n_out, bps * 32, np.ascontiguousarray(A[:, s * bps * 32:(s + 1) * bps * 32]))
        total = part if total is None else (total + part).astype(np.float32)
    return total


def unpack(kind, blocks, N, K):
    """blocks of `kind` -> int32 weights [N][K/32][32] in the integer dot's common form (q4_0: nibble - 8, q5_0: 5-bit - 16, q4_1 / q5_1 unsigned, q8_0 as stored), d and m float32
    [N][K/32] (m = 0 for the symmetric kinds).  Element j < 16 is the low nibble of qs[j] (+ bit j of qh), element j + 16 the high nibble (+ bit j + 16)."""
    nb = K // 32; bb = BLOCK_BYTES[kind]
    raw = np.frombuffer(blocks, np.uint8).reshape(N * nb, bb)
    o = 2
    d = np.ascontiguousarray(raw[:, 0:2]).view(np.float16)[:, 0].astype(np.float32)
    m = np.zeros(N * nb, np.float32)
    if kind in ("q4_1", "q5_1"):
        m = np.ascontiguousarray(raw[:, o:o + 2]).view(np.float16)[:, 0].astype(np.float32); o += 2
    qh = None
    if kind in ("q5_0", "q5_1"):
        qh = np.ascontiguousarray(raw[:, o:o + 4]).view("<u4")[:, 0]; o += 4
    qs = raw[:, o:]
    if kind == "q8_0":
        q = qs.view(np.int8).astype(np.int32)
    else:
        lo = (qs & 15).astype(np.int32); hi = (qs >> 4).astype(np.int32)
        if qh is not None:
            j = np.arange(16, dtype=np.uint32)
            lo |= (((qh[:, None] >> j) & 1) << 4).astype(np.int32); hi |= (((qh[:, None] >> (j + 16)) & 1) << 4).astype(np.int32)
        q = np.concatenate([lo, hi], axis=1) - (8 if kind == "q4_0" else 16 if kind == "q5_0" else 0)
    return q.reshape(N, nb, 32), d.reshape(N, nb), m.reshape(N, nb)


def quantize_rows(A):
    """quantize_row_q8_0 / q8_1 of every 32-block of every row: amax / 127, id = 1 / d (0 for a zero block), roundf(x id); d and s = d_unrounded * sum(q) rounded to f16.
    A [M][K] float32 -> q int32 [M][K/32][32], d, s float32 [M][K/32]."""
    A = np.ascontiguousarray(A, np.float32); M, K = A.shape
    x = A.reshape(M, K // 32, 32)
    amax = np.abs(x).max(axis=2)
    d = (amax / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)
    v = (x * idv[:, :, None]).astype(np.float32).astype(np.float64)
    q = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)                      # roundf: half away from zero (exact in f64)
    s = (q.sum(axis=2).astype(np.float32) * d).astype(np.float32)
    with np.errstate(over="ignore"):
        return q, d.astype(np.float16).astype(np.float32), s.astype(np.float16).astype(np.float32)


def mul_mat(kind, blocks, N, K, A, nseg=1, form=None, drop_ms=False, shift=None):
    """out [M][N] float32 = ggml's mul_mat of A [M][K] with the N x K / 32 blocks, the block sum cut into nseg contiguous runs.
    The last three arguments build WRONG variants, for the tests that show a case can tell them apart: form = another kind's per-block form (1 or 2), drop_ms = without the
    m * s term, shift = "dw" | "dy" | "sy": that factor of block b taken from block b + 1 (the last block: from block 0)."""
    qw, dw, mw = unpack(kind, blocks, N, K)
    qa, da, sa = quantize_rows(A)
    nb = K // 32; M = A.shape[0]; bps = nb // nseg
    assert nb % nseg == 0
    form = form or FORM[kind]
    qwf = qw.astype(np.float32); qaf = qa.astype(np.float32)
    if shift == "dw": dw = np.roll(dw, -1, axis=1)
    if shift == "dy": da = np.roll(da, -1, axis=1)
    if shift == "sy": sa = np.roll(sa, -1, axis=1)
    total = None
    for sg in range(nseg):
        sumf = np.zeros((M, N), np.float32)
        for b in range(sg * bps, (sg + 1) * bps):
            sumi = qaf[:, b, :] @ qwf[:, b, :].T                                       # integers below 2^24: exact in float32 whatever the order
            if form == 1:
                t = (sumi * dw[None, :, b]) * da[:, b, None]
            else:
                t = (dw[None, :, b] * da[:, b, None]) * sumi
                if form == 3 and not drop_ms:
                    t = t + mw[None, :, b] * sa[:, b, None]
            sumf = sumf + t
        total = sumf if total is None else total + sumf
    assert total.dtype == np.float32
    return total


_KPERM = None


def kperm(k):
    """position in memory of logical index k (skw_kperm, through the engine library's host-side layout helper, as tests/test_cpu_layouts.py reads it)"""
    global _KPERM
    if _KPERM is None:
        import ctypes as C
        from streamkit_amd import engine
        L = engine.lib(); L.skw_layout_kperm.restype = C.c_int; L.skw_layout_kperm.argtypes = [C.c_int]
        _KPERM = np.array([L.skw_layout_kperm(i) for i in range(32)], np.int64)
    k = np.asarray(k, np.int64)
    return (k & ~31) | _KPERM[k & 31]


def _f16_bits(v):
    with np.errstate(over="ignore"):
        return v.astype(np.float16).view(np.uint16)


def epilogue(epi, S, bufs, ldc=0, bias=None, res=None, scale=1.0, has_scale=0, n_ctx=0, H=0, Tpad=0, pos=None, ldc2=0, gelu=None):
    """What the kernel's epilogue leaves in its output buffers, applied to the reference sums S [M][N] in the kernel's order of operations (epi_store).
    bufs: the flat output buffers as they are before the launch (float32 for EPI_F32 / EPI_GELU_F32, uint16 otherwise; three for EPI_DEC_QKV); copies are returned.
    gelu: the function the GPU test passes in (the device's own table-driven GELU, held to the contract elsewhere); EPI_GELU_F32 only."""
    M, N = S.shape; out = [b.copy() for b in bufs]
    m = np.arange(M, dtype=np.int64)[:, None]; n = np.arange(N, dtype=np.int64)[None, :]
    v = S.astype(np.float32)
    if epi == EPI_VT_F16:
        if bias is not None: v = v + bias[None, :]
        b, key, h, c = m // n_ctx, m % n_ctx, n >> 6, n & 63
        out[0][((b * H + h) * 64 + c) * Tpad + kperm(key)] = _f16_bits(v)
        return out
    if bias is not None: v = v + bias[None, :]
    if epi == EPI_F32:
        if res is not None: v = v + res
        out[0][m * ldc + n] = v
    elif epi == EPI_GELU_F32:
        out[0][m * ldc + n] = gelu(np.ascontiguousarray(v)).reshape(M, N)
    elif epi == EPI_F16_PLAIN:
        if has_scale: v = v * np.float32(scale)
        out[0][m * ldc + n] = _f16_bits(v)
    elif epi == EPI_HEADS_F16:
        if has_scale: v = v * np.float32(scale)
        b, i, h, d = m // n_ctx, m % n_ctx, n >> 6, n & 63
        out[0][((b * H + h) * Tpad + i) * 64 + kperm(d)] = _f16_bits(v)
    elif epi == EPI_DEC_QKV:
        d = N // 3
        v = v.copy(); v[:, :2 * d] = v[:, :2 * d] * np.float32(scale)
        hb = _f16_bits(v); po = np.asarray(pos, np.int64)[:, None] * d; nd = n[:, :d]
        out[0][m * ldc + nd] = hb[:, :d]
        out[1][m * ldc2 + po + nd] = hb[:, d:2 * d]
        out[2][m * ldc2 + po + nd] = hb[:, 2 * d:]
    else:
        raise ValueError(epi)
    assert v.dtype == np.float32
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "cls kernel M N K segmented kinds order why")


def _c(cls, kernel, M, N, K, why, kinds=None, order=False):
    return Case(cls, kernel, M, N, K, 1 if kernel in (K_SMALL6, K_SMALL8) else 0, tuple(kinds or KINDS), order, why)


def cases():
    return [
        _c("segmented", K_SMALL6, 1, 16, 128, "bps 1"),
        _c("segmented", K_SMALL6, 5, 104, 384, "bps 3, N % 16 != 0"),
        _c("segmented", K_SMALL6, 17, 384, 768, "bps 6 = UB, ragged second row tile"),
        _c("segmented", K_SMALL6, 200, 136, 128, "order block", order=True),
        _c("segmented", K_SMALL6, 300, 384, 384, "prompt-pass row counts"),
        _c("segmented", K_SMALL8, 64, 384, 1024, "one full round"),
        _c("segmented", K_SMALL8, 37, 136, 1536, "bps 12: second round clamped and broken off"),
        _c("segmented", K_SMALL8, 16, 128, 3072, "three rounds"),
        _c("vocabulary", K_SMALL6, 9, 51865, 384, "odd N, n_pad 51904", kinds=("q4_0", "q5_1")),
        _c("plain", K_TW2, 1, 64, 32, "one block"),
        _c("plain", K_TW2, 70, 136, 96, "ragged tiles, odd block count"),
        _c("plain", K_TW2, 200, 136, 96, "order block", order=True),
        _c("plain", K_TW2, 1023, 384, 384, "the last M below the switch"),
        _c("plain4", K_TW4, 1026, 192, 96, "M % 4, N % 128 and K % 64 all non-zero"),
        _c("plain4", K_TW4, 1500, 200, 384, "ragged feature tile"),
        _c("staged", K_LDS, 1024, 128, 64, "one stage"),
        _c("staged", K_LDS, 1028, 256, 192, "three stages; last row tile holds 4 rows"),
        _c("staged", K_LDS, 1500, 384, 384, "tiny's Q/K/V/O"),
        _c("staged", K_LDS, 1500, 1536, 384, "FC1"),
        _c("staged", K_LDS, 1500, 384, 1536, "FC2, 24 stages"),
    ]


def case_id(c):
    return "%s-%dx%dx%d" % (c.cls, c.M, c.N, c.K)


# the epilogue cases: one shape per class, every epilogue the engine uses with the class (run_encoder and the q8 branch of the decode step, skw_engine.hip), for q4_0 and q5_1
EpiCase = collections.namedtuple("EpiCase", "name kernel M N K segmented epi n_ctx H Tpad bias res scale")
EPI_KINDS = ("q4_0", "q5_1")


def epi_cases():
    out = []
    for name, kernel, M, N, K, n_ctx, Tpad in (("plain", K_TW2, 200, 128, 96, 100, 128), ("staged", K_LDS, 3000, 384, 384, 1500, 1504)):
        H = N // 64
        out += [EpiCase(name + "-f32-bias-res", kernel, M, N, K, 0, EPI_F32, 0, 0, 0, True, True, 0.0),
                EpiCase(name + "-gelu", kernel, M, N, K, 0, EPI_GELU_F32, 0, 0, 0, True, False, 0.0),
                EpiCase(name + "-heads", kernel, M, N, K, 0, EPI_HEADS_F16, n_ctx, H, Tpad, True, False, 0.353553),
                EpiCase(name + "-vt", kernel, M, N, K, 0, EPI_VT_F16, n_ctx, H, Tpad, True, False, 0.0),
                EpiCase(name + "-f16", kernel, M, N, K, 0, EPI_F16_PLAIN, 0, 0, 0, False, False, 0.353553)]
    out += [EpiCase("segmented-qkv", K_SMALL6, 5, 384, 128, 1, EPI_DEC_QKV, 128, 0, 0, True, False, 0.353553),
            EpiCase("segmented-f32-bias-res", K_SMALL6, 5, 128, 384, 1, EPI_F32, 0, 0, 0, True, True, 0.0),
            EpiCase("segmented-gelu", K_SMALL6, 5, 128, 384, 1, EPI_GELU_F32, 0, 0, 0, True, False, 0.0),
            EpiCase("segmented-f16", K_SMALL6, 5, 128, 384, 1, EPI_F16_PLAIN, 0, 0, 0, True, False, 0.353553)]
    return out


def edge_rows(M, nb):
    """which rows of a case carry the quantiser's edges: (all-zero row, row with one zero block, row whose first block lands on roundf ties); None where M has no room — one row
    takes the ties and, with more than one block, a zero block as well"""
    if M >= 3:
        return M - 1, M - 2, M - 3           # the last rows: in the ragged tail of the last row tile where the case has one
    if M == 2:
        return None, 1, 0
    return None, (0 if nb > 1 else None), 0


def activations(seed, M, K, order_pattern=None):
    """rows scaled by 2^-1 .. 2^3 with a few channels x 30 (as tests/test_gpu_mfma_model._gemm_operands), the edge rows, and on the order cases every fourth row the pattern"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)) * np.exp2(rng.integers(-1, 4, (M, 1)).astype(np.float64))
    A[:, rng.integers(0, K, max(1, K // 100))] *= 30.0
    A = A.astype(np.float32)
    if order_pattern is not None:
        rows = np.arange(0, M, 4)
        A[rows] = (order_pattern[None, :] * 3.0 * (1.0 + 0.02 * rng.random((len(rows), K)))).astype(np.float32)
    zero, zblock, ties = edge_rows(M, K // 32)
    nb = K // 32
    if zero is not None: A[zero] = 0.0
    if zblock is not None: A[zblock, (nb - 1) * 32:] = 0.0       # the last block (the first is the tie row's when both fall on one row)
    if ties is not None:
        A[ties, :32] = np.linspace(-127, 127, 32, dtype=np.float32) * 0.5      # amax 63.5 -> d = 0.5, id = 2 exactly (the block test_cpu_oracle.py uses; symmetric: its q sum to 0)
        t = min(1, nb - 1)                                                      # and a block where x id IS n + 0.5 for 31 of 32 values, not symmetric: roundf's ties, s != 0
        A[ties, t * 32:(t + 1) * 32] = TIE_BLOCK
    return A


TIE_BLOCK = np.array([63.5] + [(2 * n + 1) / 4.0 for n in range(-20, 11)], np.float32)


ORDER_FEATURES = 32


def weights(seed, N, K, order_pattern=None):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, K)) * 0.04).astype(np.float32)
    if order_pattern is not None:            # the order block: 32 features follow the activations' sign pattern, away from zero, so that their integer dots saturate
        f = np.arange(ORDER_FEATURES) * (N // ORDER_FEATURES)
        W[f] = (order_pattern[None, :] * 0.04 * (1.0 + rng.random((ORDER_FEATURES, K)))).astype(np.float32)
    return W


def _seed(M, N, K):
    return (M * 1000003 + N * 10007 + K) % (2 ** 31)


_WCACHE = {}


def operands(case, kind):
    """(blocks, A): the case's weights quantised as `kind`, and its activation rows.  The float weights are drawn once per shape and shared by the kinds."""
    M, N, K = case.M, case.N, case.K; s = _seed(M, N, K)
    pat = None
    if getattr(case, "order", False):
        pat = np.where(np.random.default_rng(s + 2).random(K) < 0.5, -1.0, 1.0)
    key = (N, K, s, pat is not None)
    if key not in _WCACHE:
        if N * K > 4 << 20: _WCACHE.clear()
        _WCACHE[key] = weights(s + 1, N, K, pat)
    W = _WCACHE[key]
    return quantize_blocks(W.reshape(-1, 32), kind), activations(s, M, K, pat)
