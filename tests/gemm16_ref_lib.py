"""What the f16_mfma GEMM kernels (skw_kernels_f16.hip) must return, restated in numpy: the reference of tests/test_gpu_gemm16_epi.py (the kernels, bit for bit) and of
tests/test_cpu_gemm16_cases.py (the cases themselves: that they cover the engine's launches and tell the named wrong epilogues from the right one).

  * accumulator: oracle_lib.gemm_f16mfma — oracle/'s integer restatement of v_mfma_f32_16x16x32_f16 chained over ascending 32-k blocks; split 1 for k_gemm16w, k_gemm16 and
    k_gemm16_vocab, split 4 for k_gemm16_small and k_gemm16_small_lnA (their four waves take a K quarter each and the quarters meet as ((q0 + q1) + q2) + q3);
  * epilogues: bias, scale, residual and the f16 rounding are single IEEE operations, written here as numpy float32 operations in the kernels' order;
  * layouts: skw_kperm, the per-head and V^T layouts, ROWPAD and the three fragment orders (skw_kfrag_off, skw_vtfrag_off, skw_afrag_off), restated from their definitions in
    skw_kernels.h;
  * the LayerNorm operand of k_gemm16_small_lnA in the kernel's own order of f64 additions (layernorm_operand);
  * GELU: gelu16 uses the hardware's exp2 and reciprocal approximations, so its outputs are held to faithful rounding of the float64 formula and a cap on the share of outputs
    that are not the nearest f16 (gelu_verdict), not to bits.
Every case is data (cases()); prepare(case) draws its operands from a seed and lays down the sentinel buffers; expected(...) returns the buffers after a correct launch together
with the mask of the elements a launch may write — everything else must still hold the sentinel."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as ol  # noqa: E402

EPI_F32, EPI_F16_KPERM, EPI_GELU_F16_KPERM, EPI_CONV2, EPI_HEADS_F16, EPI_VT_F16, EPI_F16_PLAIN, EPI_GELU_F16_KPERM_ROWPAD, EPI_DEC_QKV = 0, 1, 2, 3, 4, 5, 6, 7, 8
EPI_NAME = {EPI_F32: "f32", EPI_F16_KPERM: "f16kperm", EPI_GELU_F16_KPERM: "gelu", EPI_CONV2: "conv2", EPI_HEADS_F16: "heads", EPI_VT_F16: "vt", EPI_F16_PLAIN: "f16",
            EPI_GELU_F16_KPERM_ROWPAD: "gelurowpad", EPI_DEC_QKV: "qkv"}
GELU_EPIS = (EPI_GELU_F16_KPERM, EPI_GELU_F16_KPERM_ROWPAD, EPI_CONV2)
KPERM_EPIS = (EPI_F16_KPERM, EPI_GELU_F16_KPERM, EPI_GELU_F16_KPERM_ROWPAD, EPI_HEADS_F16)
# launchers of skw_debug_gemm16_epi and the kernel ids they report (SkwGemm16Kernel, skw_kernels.h)
L_W, L_LDS, L_SMALL, L_LNA = 0, 1, 2, 3
K_W, K_LDS_256, K_LDS_128, K_SMALL_16, K_SMALL_64, K_LNA_6_1, K_LNA_6_4, K_LNA_12_1, K_LNA_12_2, K_VOCAB = 0, 1, 2, 10, 11, 20, 21, 22, 23, 1000
KERNEL_NAME = {K_W: "k_gemm16w", K_LDS_256: "k_gemm16<256>", K_LDS_128: "k_gemm16<128>", K_SMALL_16: "k_gemm16_small<16 rows>", K_SMALL_64: "k_gemm16_small<64 rows>",
               K_LNA_6_1: "k_gemm16_small_lnA<NKW 6, NT 1>", K_LNA_6_4: "k_gemm16_small_lnA<NKW 6, NT 4>", K_LNA_12_1: "k_gemm16_small_lnA<NKW 12, NT 1>",
               K_LNA_12_2: "k_gemm16_small_lnA<NKW 12, NT 2>"}
SCALE = np.float32(0.353553)          # the engine's KQscale at d_head 64: not a power of two, so "round, then scale" and "scale, then round" give different bits
SENT8 = 0x5A
F16_NAN = 0x7E00
GELU_CAP = 0.01                       # share of a case's GELU outputs that may be the farther of the two adjacent f16 values (a condition, not a measurement)
GELU_REF_CAP = 0.005                  # the same share for gelu16's formula in float32 with correctly rounded exp2 and reciprocal: what the reference side alone uses up

f32 = np.float32


def kernel_name(k):
    return KERNEL_NAME.get(k, "k_gemm16_vocab<MT %d, RD %d>" % ((k - K_VOCAB) // 100, (k - K_VOCAB) % 100) if k >= K_VOCAB else "none")


# ---------------------------------------------------------------------------------------------------------------- layouts (skw_kernels.h)
def kperm(k):
    """memory position of logical index k: inside each aligned block of 32 the 8 values with k % 4 == q are contiguous at [8q, 8q + 8)"""
    k = np.asarray(k)
    return (k & ~31) | ((k & 3) << 3) | ((k >> 2) & 7)


def inv_kperm(p):
    p = np.asarray(p)
    return (p & ~31) | ((p & 7) << 2) | ((p >> 3) & 3)


def rowpad(m, T):
    """conv1's output rows: one pad row on each side of a clip's T rows"""
    m = np.asarray(m)
    return (m // T) * (T + 2) + m % T + 1


def heads_off(b, i, n, H, Tpad):
    """EPI_HEADS_F16: C[(b H + h) Tpad + i][kperm(d)], n = 64 h + d"""
    return ((b * H + (n >> 6)) * Tpad + i) * 64 + kperm(n & 63)


def vt_off(b, feat, key, H, Tpad):
    """EPI_VT_F16: C[(b H + h) 64 + c][kperm(key)], row stride Tpad, feat = 64 h + c"""
    return ((b * H + (feat >> 6)) * 64 + (feat & 63)) * Tpad + kperm(key)


def kfrag_off(slot, H, Tpad, key, feat):
    """skw_kfrag_off for the 8-half chunk that holds feature `feat`, plus the place inside the chunk"""
    h, c, r = feat >> 6, (feat >> 3) & 7, key & 15
    i = 4 * (r & 3) + (r >> 2)
    return ((slot * H + h) * (Tpad >> 4) + (key >> 4)) * 1024 + (c >> 2) * 512 + (i + 16 * (c & 3)) * 8 + (feat & 7)


def vtfrag_off(slot, H, Tpad, feat, pos):
    """skw_vtfrag_off for the chunk that holds memory position `pos` (= kperm(key)) of channel `feat`, plus the place inside the chunk"""
    h, ch = feat >> 6, feat & 63
    return ((slot * H + h) * (Tpad >> 5) + (pos >> 5)) * 2048 + (ch >> 4) * 512 + ((ch & 15) + 16 * ((pos >> 3) & 3)) * 8 + (pos & 7)


def afrag_off(m, p, K):
    """skw_afrag_off: memory position p of row m in the fragment-order activation image, K halves per row"""
    return ((m >> 4) * (K >> 5) + (p >> 5)) * 512 + ((m & 15) + 16 * ((p >> 3) & 3)) * 8 + (p & 7)


def afrag_image(rows, fill=F16_NAN):
    """the fragment-order image of rows [M][K] (u16); the pad rows M .. ceil16(M) hold `fill`"""
    M, K = rows.shape
    img = np.full(((M + 15) & ~15) * K, fill, np.uint16)
    m, p = np.meshgrid(np.arange(M), np.arange(K), indexing="ij")
    img[afrag_off(m, p, K)] = rows
    return img


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def fmaf(a, b, c):
    """float32 fma(a, b, c), correctly rounded, through float64.  The product of two float32 values has at most 48 significant bits, so p = a * b is EXACT in float64.  t = p + c
    is one float64 rounding; rounding t again to float32 can differ from rounding the exact sum only when t sits exactly on the midpoint of two float32 values while the exact sum
    does not (the float64 rounding moved it there, or off by less than half a float64 ulp).  TwoSum gives that lost part e = (p + c) - t exactly, and on such a midpoint the sign of
    e says which neighbour the exact sum is nearer to.  (Results in float32's subnormal range are not handled: no case produces one.)"""
    a, b, c = np.broadcast_arrays(np.atleast_1d(np.asarray(a, np.float64)), np.asarray(b, np.float64), np.asarray(c, np.float64))
    p = a * b
    t = p + c
    bb = t - p
    e = (p - (t - bb)) + (c - bb)
    r = t.astype(np.float32)
    tie = ((np.ascontiguousarray(t).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (e != 0) & np.isfinite(t)
    if tie.any():
        tt, rr, ee = t[tie], r[tie], e[tie]
        other = np.nextafter(rr, np.where(rr.astype(np.float64) < tt, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        lo, hi = np.minimum(rr, other), np.maximum(rr, other)
        r[tie] = np.where(ee > 0, hi, lo)
    return r


def layernorm_operand(x, gain, bias, variant=None):
    """the A operand k_gemm16_small_lnA builds from x [M][K] f32: f16(fma(fma(x, sa, sb), gain, bias)) with the row statistics in the kernel's own order.  Wave w holds k-blocks
    [w nkw, (w + 1) nkw) of 32; lane (r16, g) of it the eight values at 32 (w nkw + j) + 8 g + 4 h + e and adds them in f64 in ascending j, then h, then e (s2 += x x, exact in
    f64 before the addition); lanes combine (g0 + g1) + (g2 + g3) (two xor shuffles), waves (w0 + w1) + (w2 + w3) (LDS).  md = s1 / K, var = max(s2 / K - md md, 0),
    rstd = 1 / sqrtf(f32(var) + 1e-5f), sa = rstd, sb = -f32(md) rstd.  -> (A u16 [M][K], mean f64 [M], var f64 [M] before the clamp)
    variant "ln_mean_short": the sums leave out the last 128 values of a row (a K tail that is not summed)."""
    x = np.ascontiguousarray(x, np.float32); M, K = x.shape
    assert K % 128 == 0
    nkw = K // 128
    xd = x.astype(np.float64).reshape(M, 4, nkw, 4, 8)                     # [m][w][j][g][h e]
    if variant == "ln_mean_short":
        xd = xd.copy(); xd.reshape(M, K)[:, K - 128:] = 0.0
    s1 = np.zeros((M, 4, 4)); s2 = np.zeros((M, 4, 4))
    for j in range(nkw):
        for he in range(8):
            v = xd[:, :, j, :, he]
            s1 = s1 + v; s2 = s2 + v * v
    s1 = (s1[:, :, 0] + s1[:, :, 1]) + (s1[:, :, 2] + s1[:, :, 3]); s2 = (s2[:, :, 0] + s2[:, :, 1]) + (s2[:, :, 2] + s2[:, :, 3])
    s1 = (s1[:, 0] + s1[:, 1]) + (s1[:, 2] + s1[:, 3]); s2 = (s2[:, 0] + s2[:, 1]) + (s2[:, 2] + s2[:, 3])
    md = s1 / float(K); var_raw = s2 / float(K) - md * md
    var = np.maximum(var_raw, 0.0)
    rstd = f32(1.0) / np.sqrt(var.astype(np.float32) + f32(1e-5))          # numpy's float32 sqrt and division are correctly rounded, as the device's are here
    sa = rstd; sb = -(md.astype(np.float32)) * rstd
    y = fmaf(fmaf(x, sa[:, None], sb[:, None]), np.asarray(gain, np.float32)[None, :], np.asarray(bias, np.float32)[None, :])
    with np.errstate(over="ignore"):                                        # (the wrong-variant statistics of a far-mean row can leave f16's range)
        return y.astype(np.float16).view(np.uint16), md, var_raw


def gelu64(x):
    """ggml's tanh form in float64"""
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)))


def gelu16_f32(x):
    """gelu16's own formula (skw_kernels_f16.hip) in float32 with a correctly rounded exp2 and reciprocal in place of the hardware's approximations -> f16"""
    x = np.asarray(x, np.float32)
    c2 = f32(f32(f32(-2.88539008177792681472) * f32(0.79788456080286535588)) * f32(0.044715)); c1 = f32(f32(-2.88539008177792681472) * f32(0.79788456080286535588))
    z = x * fmaf(x * x, c2, c1)
    with np.errstate(over="ignore"):
        e = np.exp2(z.astype(np.float64)).astype(np.float32)
        r = (1.0 / (f32(1.0) + e).astype(np.float64)).astype(np.float32)
    return (x * r).astype(np.float16)


def gelu_verdict(got, x16, pe=None):
    """got: the kernel's outputs (f16 values; with pe, EPI_CONV2's f32 outputs pe + f32(f16 gelu)); x16: the pre-activations f32(f16(acc + bias)).
    -> (ok [..] bool: the output is the exact f16 value of float64 GELU(x) or one of the two f16 values adjacent to it — in f16's subnormal range, within 2^-24 of it;
        far [..] bool: it is not the nearest f16)"""
    ref = gelu64(x16)
    near = ref.astype(np.float16)
    n64 = near.astype(np.float64)
    other = np.where(n64 < ref, np.nextafter(near, np.float16(np.inf)), np.where(n64 > ref, np.nextafter(near, np.float16(-np.inf)), near)).astype(np.float16)
    if pe is None:
        g = np.asarray(got, np.float16).astype(np.float64)
        is_near = g == n64; is_other = g == other.astype(np.float64)
        sub = (np.abs(ref) < 2.0 ** -14) & (np.abs(g - ref) <= 2.0 ** -24)
    else:
        g = np.asarray(got, np.float32); pe = np.asarray(pe, np.float32)
        is_near = g == pe + near.astype(np.float32); is_other = g == pe + other.astype(np.float32)
        sub = np.zeros(g.shape, bool)
    return is_near | is_other | sub, ~is_near


# ---------------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "family name launchers M N K epi bias res scale n_ctx Tpad frag conv a_frag c_frag wf ldc kernel refuse why")


def _c(family, name, launchers, M, N, K, epi, bias=True, res=None, scale=False, n_ctx=0, Tpad=0, frag=False, conv=False, a_frag=False, c_frag=False, wf=(False,), ldc=0,
       kernel=None, refuse=None, why=""):
    return Case(family, name, tuple(launchers), M, N, K, epi, bias, res, scale, n_ctx, Tpad, frag, conv, a_frag, c_frag, tuple(wf), ldc, kernel, refuse, why)


BIG_SHAPES = [(128, 256, 64, "one tile, one K step"), (200, 384, 256, "ragged rows"), (333, 416, 192, "ragged row and feature tiles, odd number of K steps"),
              (64, 384, 128, "M < 128: k_gemm16 only")]
CLIP_GEOMS = [(150, 160, 2, 128, 128), (300, 320, 3, 384, 256)]      # n_ctx, Tpad, clips, N, K


def cases():
    out = []
    for M, N, K, why in BIG_SHAPES:
        ls = (L_W, L_LDS) if M >= 128 else (L_LDS,)
        s = "%dx%dx%d" % (M, N, K)
        out += [_c("big", "f32-nobias-" + s, ls, M, N, K, EPI_F32, bias=False, why=why), _c("big", "f32-bias-" + s, ls, M, N, K, EPI_F32, why=why),
                _c("big", "f32-bias-res-" + s, ls, M, N, K, EPI_F32, res="separate", why=why), _c("big", "f32-bias-resalias-" + s, ls, M, N, K, EPI_F32, res="alias", why=why),
                _c("big", "f16kperm-" + s, ls, M, N, K, EPI_F16_KPERM, scale=True, why=why), _c("big", "gelu-" + s, ls, M, N, K, EPI_GELU_F16_KPERM, why=why),
                _c("big", "f16-" + s, ls, M, N, K, EPI_F16_PLAIN, scale=True, why=why)]
    for gi, (n_ctx, Tpad, B, N, K) in enumerate(CLIP_GEOMS):
        M = n_ctx * B; s = "%dx%d-%dx%dx%d" % (n_ctx, Tpad, M, N, K); g = dict(n_ctx=n_ctx, Tpad=Tpad)
        out += [_c("big", "heads-" + s, (L_W, L_LDS), M, N, K, EPI_HEADS_F16, scale=bool(gi), why="the engine's Q / K call (no scale) | scaled", **g),
                _c("big", "vt-" + s, (L_W, L_LDS), M, N, K, EPI_VT_F16, why="pad keys n_ctx .. Tpad are +0", **g),
                _c("big", "gelurowpad-" + s, (L_W, L_LDS), M, N, K, EPI_GELU_F16_KPERM_ROWPAD, why="conv1: the pad rows keep the sentinel", **g),
                _c("big", "conv2-" + s, (L_W, L_LDS), M, N, K, EPI_CONV2, conv=True, why="overlapping A rows (lda < K) per clip, positional embedding", **g),
                _c("big", "f16-frag-" + s, (L_W, L_LDS), M, N, K, EPI_F16_PLAIN, scale=True, frag=True, why="fragment-order cross K", **g),
                _c("big", "vt-frag-" + s, (L_W, L_LDS), M, N, K, EPI_VT_F16, frag=True, why="fragment-order cross V^T", **g)]
    both = (True, False)
    sm = lambda M, N, K: "%dx%dx%d" % (M, N, K)
    for M, N, K, k, why in [(5, 384, 384, K_SMALL_16, "one ragged row tile"), (37, 768, 1536, K_SMALL_16, "12 k-blocks per wave: one full ring"),
                            (64, 2048, 128, K_SMALL_64, "the 64-row form, one k-block per wave"), (70, 2304, 384, K_SMALL_64, "two row blocks, the second ragged")]:
        out.append(_c("small", "f32-bias-resalias-" + sm(M, N, K), (L_SMALL,), M, N, K, EPI_F32, res="alias", wf=both, kernel=k, why=why))
    out.append(_c("small", "f32-bias-resalias-9x390x256-ldc391", (L_SMALL,), 9, 390, 256, EPI_F32, res="alias", ldc=391, kernel=K_SMALL_16,
                  why="ragged 4-column groups, odd ldc: the scalar path"))
    for M, N, K in [(5, 384, 384), (37, 768, 1536)]:
        out.append(_c("small", "f32-afrag-" + sm(M, N, K), (L_SMALL,), M, N, K, EPI_F32, res="alias", a_frag=True, wf=both, kernel=K_SMALL_16,
                      why="A as the fragment-order image, NaN pad rows"))
    out += [_c("small", "f16-5x384x384", (L_SMALL,), 5, 384, 384, EPI_F16_PLAIN, scale=True, wf=both, kernel=K_SMALL_16),
            _c("small", "f16-64x2304x768", (L_SMALL,), 64, 2304, 768, EPI_F16_PLAIN, scale=True, wf=both, kernel=K_SMALL_64)]
    for M, N, K, k in [(5, 1536, 384, K_SMALL_16), (37, 3072, 768, K_SMALL_64)]:
        for cf in (False, True):
            out.append(_c("small", "gelu-%s%s" % (sm(M, N, K), "-cfrag" if cf else ""), (L_SMALL,), M, N, K, EPI_GELU_F16_KPERM, c_frag=cf, wf=both, kernel=k, why="fc1 as rows | as fc2's A image"))
    for M, N, K, k in [(5, 1152, 384, K_SMALL_16), (37, 2304, 768, K_SMALL_64)]:
        out.append(_c("small", "qkv-" + sm(M, N, K), (L_SMALL,), M, N, K, EPI_DEC_QKV, scale=True, n_ctx=N // 3, wf=both, kernel=k, why="K / V appended at pos[m]"))
    out.append(_c("small", "refuse-wf-ragged-9x390x256", (L_SMALL,), 9, 390, 256, EPI_F32, ldc=391, wf=(True,), refuse="an image of a weight with N % 16 != 0"))
    for M, N, K, k, why in [(5, 384, 128, K_LNA_6_1, "one k-block per wave"), (16, 384, 384, K_LNA_6_1, "a full row tile"), (37, 768, 768, K_LNA_6_1, "NKW 6 full"),
                            (5, 1024, 1024, K_LNA_12_1, "8 of 12 k-blocks"), (37, 384, 1536, K_LNA_12_1, "NKW 12 full")]:
        out.append(_c("lna", "f16-" + sm(M, N, K), (L_LNA,), M, N, K, EPI_F16_PLAIN, scale=True, wf=both, kernel=k, why=why))
    for M, N, K, k, why in [(5, 2048, 512, K_LNA_6_4, "NT 4"),
                            (37, 2080, 768, K_LNA_6_4, "130 strips: the last NT group holds two of four (2064 is no width of a kperm'ed output: see BAD_KPERM_WIDTH)"),
                            (16, 4096, 1024, K_LNA_12_2, "NT 2")]:
        for cf in (False, True):
            out.append(_c("lna", "gelu-%s%s" % (sm(M, N, K), "-cfrag" if cf else ""), (L_LNA,), M, N, K, EPI_GELU_F16_KPERM, c_frag=cf, wf=both, kernel=k, why=why))
    for M, N, K, k in [(5, 1152, 384, K_LNA_6_1), (37, 2304, 768, K_LNA_6_4), (16, 3072, 1024, K_LNA_12_2)]:
        out.append(_c("lna", "qkv-" + sm(M, N, K), (L_LNA,), M, N, K, EPI_DEC_QKV, scale=True, n_ctx=N // 3, wf=both, kernel=k))
    out += [_c("lna", "refuse-K1664", (L_LNA,), 5, 384, 1664, EPI_F16_PLAIN, scale=True, refuse="13 k-blocks per wave: more than the registers hold"),
            _c("lna", "refuse-res", (L_LNA,), 5, 384, 384, EPI_F16_PLAIN, scale=True, res="separate", refuse="a residual")]
    for M, N, K, ldc, mt, rd, why in [(9, 8201, 384, 8201, 4, 12, "ragged strip, odd ldc, RD 12, 64-row LDS form"), (37, 8200, 1280, 8200, 2, 20, "RD 20, 32-row form"),
                                      (64, 8208, 256, 8208, 4, 4, "RD 4")]:
        for b in (True, False):
            out.append(_c("vocab", "f32-%s-%s" % ("bias" if b else "nobias", sm(M, N, K)), (L_SMALL,), M, N, K, EPI_F32, bias=b, ldc=ldc, kernel=K_VOCAB + 100 * mt + rd, why=why))
    return out


# N = 2064 = 64 x 32 + 16 with a kperm'ed output: memory positions 2048 .. 2063 of a row would hold logical features up to 2079 >= N (kperm permutes inside aligned blocks of 32),
# so the epilogue's bias index leaves the bias vector.  No product of the engine has such a width; skw_debug_gemm16_epi refuses it on the host (-1), before anything is launched.
BAD_KPERM_WIDTH = (37, 2064, 768)


def case_id(c):
    return "%s-%s" % (c.family, c.name)


def runs(c):
    """the launches of a case: (launcher, weights from the fragment-order image, force k_gemm16_small, split of the accumulator)"""
    if c.family == "big":
        return [(l, l == L_W, False, 1) for l in c.launchers]
    if c.family == "vocab":
        return [(L_SMALL, False, False, 1), (L_SMALL, False, True, 4)]
    return [(c.launchers[0], wf, False, 4) for wf in c.wf]


def run_id(r):
    return {L_W: "k_gemm16w", L_LDS: "k_gemm16", L_SMALL: "small", L_LNA: "lnA"}[r[0]] + ("-wf" if r[1] and r[0] >= L_SMALL else "") + ("-forced" if r[2] else "")


def is_gelu(c):
    return c.epi in GELU_EPIS


# ---------------------------------------------------------------------------------------------------------------- operands
def _seed(c):
    return (c.M * 1000003 + c.N * 10007 + c.K * 31 + (7 if c.family == "lna" else 0)) % (2 ** 31)


def gemm_operands(seed, M, N, K):
    """as tests/test_gpu_mfma_model._gemm_operands: rows scaled by 2^-1 .. 2^3, a few loud channels"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)) * np.exp2(rng.integers(-1, 4, (M, 1)).astype(np.float64))
    A[:, rng.integers(0, K, max(1, K // 100))] *= 30.0
    W = rng.standard_normal((N, K)) * 0.04
    return A.astype(np.float16).view(np.uint16), W.astype(np.float16).view(np.uint16)


def ln_rows(seed, M, K):
    """LayerNorm inputs: rows with mean 0, rows with |mean| ~ 30 std, one row with a single loud channel, one constant row (the variance clamp)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K)) * np.exp2(rng.integers(-1, 3, (M, 1)).astype(np.float64))
    x -= x.mean(axis=1, keepdims=True)
    far = np.arange(M) % 2 == 1
    x[far] += 30.0 * x[far].std(axis=1, keepdims=True) * rng.choice([-1.0, 1.0], (int(far.sum()), 1))
    x = x.astype(np.float32)
    loud, const = (2, 3) if M >= 4 else (None, None)
    if loud is not None:
        x[loud, int(rng.integers(0, K))] = 500.0
        x[const] = np.float32(3.1415927)                                    # 24 significant bits: the f64 sum of K squares is rounded, so E[x^2] - mean^2 is not exactly 0
    gain = (1.0 + rng.uniform(-0.5, 0.5, K)).astype(np.float32); bias = rng.uniform(-0.5, 0.5, K).astype(np.float32)
    return x, gain, bias, (loud, const)


def positions(M, n_text_ctx):
    """distinct cache positions per row, with 0 and the last position among them"""
    assert M <= n_text_ctx
    pos = (np.arange(M) * 5 + 3) % n_text_ctx
    pos[0] = 0; pos[-1] = n_text_ctx - 1
    if M > 2:
        taken = {0, n_text_ctx - 1}
        for i in range(1, M - 1):
            while int(pos[i]) in taken:
                pos[i] = (pos[i] + 1) % n_text_ctx
            taken.add(int(pos[i]))
    assert len(set(pos.tolist())) == M
    return pos.astype(np.int32)


N_TEXT_CTX = 40
MARGIN_ROWS, MARGIN_COLS = 3, 8


def _sentinel(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, SENT8, np.uint8).view(dtype)


class Prepared:
    """a case's operands, launch arguments and sentinel buffers; nothing here is modified after construction"""
    def __init__(self, c):
        self.c = c
        M, N, K = c.M, c.N, c.K
        rng = np.random.default_rng(_seed(c) + 1)
        self.ln = None; self.loud_const = (None, None)
        if c.family == "lna":
            x, g, b, self.loud_const = ln_rows(_seed(c), M, K)
            self.ln = (x, g, b)
            _, self.W = gemm_operands(_seed(c), 1, N, K)
            self.rows = None
        elif c.conv:                                                        # conv2: a clip's rows overlap — row i starts lda = K / 2 halves after row i - 1
            self.lda = K // 2; self.rpb = c.n_ctx; self.stride = (c.n_ctx + 1) * self.lda + 64
            B = M // c.n_ctx
            flat, self.W = gemm_operands(_seed(c), 1, N, K)
            buf = (rng.standard_normal(B * self.stride) * np.exp2(rng.integers(-1, 3, B * self.stride).astype(np.float64))).astype(np.float16).view(np.uint16)
            self.A_buf = buf
            m = np.arange(M)
            start = (m // self.rpb) * self.stride + (m % self.rpb) * self.lda
            self.rows = buf[start[:, None] + np.arange(K)[None, :]]
        else:
            self.rows, self.W = gemm_operands(_seed(c), M, N, K)
        self.bias = rng.standard_normal(N).astype(np.float32) if c.bias else None
        self.res = (rng.standard_normal((M, N)) * 4.0).astype(np.float32) if c.res else None
        self.pe = (rng.standard_normal((c.n_ctx, N)) * 0.5).astype(np.float32) if c.epi == EPI_CONV2 else None
        self.scale = SCALE if c.scale else np.float32(1.0)
        self.pos = positions(M, N_TEXT_CTX) if c.epi == EPI_DEC_QKV else None
        self.H = N // 64 if (c.epi in (EPI_HEADS_F16, EPI_VT_F16) or c.frag) else 0
        # ---- output buffers: the sentinel, with margins past M, N, the clips and the caches
        B = M // c.n_ctx if (c.n_ctx and c.epi != EPI_DEC_QKV) else 0
        self.ldc = c.ldc or N + MARGIN_COLS
        self.ldc2 = 0
        if c.epi in (EPI_HEADS_F16, EPI_VT_F16) or c.frag:
            bufs = [_sentinel(B * self.H * c.Tpad * 64 + 192, np.uint16)]; self.ldc = 0
        elif c.epi == EPI_GELU_F16_KPERM_ROWPAD:
            bufs = [_sentinel((B * (c.n_ctx + 2) + MARGIN_ROWS) * self.ldc, np.uint16)]
        elif c.epi == EPI_DEC_QKV:
            d = N // 3; self.ldc = d + MARGIN_COLS; self.ldc2 = N_TEXT_CTX * d + 64
            bufs = [_sentinel((M + MARGIN_ROWS) * self.ldc, np.uint16), _sentinel((M + 1) * self.ldc2, np.uint16), _sentinel((M + 1) * self.ldc2, np.uint16)]
        elif c.c_frag:
            bufs = [_sentinel(((M + 15) & ~15) * N + 512, np.uint16)]; self.ldc = N
        else:
            bufs = [_sentinel((M + MARGIN_ROWS) * self.ldc, np.float32 if c.epi in (EPI_F32, EPI_CONV2) else np.uint16)]
        if c.res == "alias":
            bufs[0].reshape(M + MARGIN_ROWS, self.ldc)[:M, :N] = self.res
        self.bufs = bufs
        for a in [self.W, self.bias, self.res, self.pe, self.rows] + bufs + list(self.ln or ()):
            if a is not None:
                a.setflags(write=False)
        self._A16 = None

    def a_rows(self, variant=None):
        """the A operand as rows [M][K] of f16 bits in the kernel's k order (the lnA family: the LayerNorm restatement)"""
        if self.ln is None:
            return self.rows
        if variant == "ln_mean_short":
            return layernorm_operand(*self.ln, variant=variant)[0]
        if self._A16 is None:
            self._A16 = layernorm_operand(*self.ln)[0]
        return self._A16

    def launch_kwargs(self, run):
        """arguments of Context.gemm16_epi for one run of the case"""
        c = self.c; launcher, wf, forced, _ = run
        kw = dict(launcher=launcher, N=c.N, K=c.K, epi=c.epi, W=self.W, C_buf=self.bufs[0], M=c.M, use_wf=wf, bias=self.bias, scale=float(self.scale), has_scale=1 if c.scale else 0,
                  n_ctx=c.n_ctx, H=self.H, Tpad=c.Tpad, frag=c.frag, c_frag=c.c_frag, pos=self.pos, force_small=forced, ldc=self.ldc, ldc2=self.ldc2)
        if c.res == "alias":
            kw.update(res_alias=True)
        elif c.res:
            kw.update(res=self.res)
        if self.ln is not None:
            kw.update(ln=self.ln)
        elif c.conv:
            kw.update(A=self.A_buf, lda=self.lda, a_rows_per_batch=self.rpb, a_batch_stride=self.stride)
        elif c.a_frag:
            kw.update(A=afrag_image(self.rows), a_frag=True)
        else:
            kw.update(A=self.rows, lda=c.K)
        if c.epi == EPI_CONV2:
            kw.update(pe=self.pe)
        if c.epi == EPI_DEC_QKV:
            kw.update(C2_buf=self.bufs[1], C3_buf=self.bufs[2])
        return kw


_ACC = collections.OrderedDict()


def accumulator(prep, split, rows=None, variant=None):
    """the matrix cores' sums for the case (rows: a subset of its rows), cached per (case, split) for the full row set"""
    A = prep.a_rows(variant)
    if rows is not None or variant is not None:
        return ol.gemm_f16mfma(A if rows is None else np.ascontiguousarray(A[rows]), prep.W, split)
    c = prep.c
    key = (c.family == "lna", _seed(c), c.M, c.N, c.K, c.conv, split)
    if key not in _ACC:
        while len(_ACC) >= 3:
            _ACC.popitem(last=False)
        acc = ol.gemm_f16mfma(A, prep.W, split); acc.setflags(write=False)
        _ACC[key] = acc
    return _ACC[key]


VARIANTS = ("scale_before_bias", "round_before_scale", "bias_by_position", "pads_not_zeroed", "pos_row0", "ln_mean_short", "split1")


def applicable(c, variant):
    """does the named wrong variant change what a correct kernel would compute for this case at all?"""
    if c.refuse or is_gelu(c):
        return False
    if variant == "scale_before_bias":
        return c.scale and c.bias and c.epi in (EPI_F16_KPERM, EPI_F16_PLAIN, EPI_HEADS_F16, EPI_DEC_QKV)
    if variant == "round_before_scale":
        return c.scale and c.epi in (EPI_F16_KPERM, EPI_F16_PLAIN, EPI_HEADS_F16, EPI_DEC_QKV)
    if variant == "bias_by_position":
        return c.bias and c.epi in KPERM_EPIS
    if variant == "pads_not_zeroed":
        return c.epi == EPI_VT_F16
    if variant == "pos_row0":
        return c.epi == EPI_DEC_QKV
    if variant == "ln_mean_short":
        return c.family == "lna"
    if variant == "split1":                                                 # (an f16 output hides most of the f32 sums' last bits: the f32 cases pin the split; see split1_visible_f16)
        return c.family == "small" and c.epi == EPI_F32 and c.K >= 256
    raise KeyError(variant)


def split1_candidates(cs):
    """the f16-output cases of the K-split kernels: one chain instead of four quarters changes an f16 output only where the f32 sums straddle an f16 rounding boundary, so a single
    case need not show it — but k_gemm16_small_lnA has no f32 epilogue, so at least one of its cases must"""
    return [c for c in cs if c.family == "lna" and not c.refuse and not is_gelu(c) and c.K >= 256]


def expected(prep, acc, rows=None, variant=None):
    """-> (bufs, masks, pre): the output buffers after a correct launch (bit patterns; for the GELU epilogues the written elements hold the NEAREST f16 of float64 GELU and are
    judged by gelu_verdict, not by equality), per buffer the mask of the elements a launch may write, and for the GELU epilogues (pre-activations f32(f16(acc + bias)) per written
    element of buffer 0, pe per element or None).  acc: accumulator(prep, split, rows); rows: the subset of the case's rows acc holds (None: all).  variant: one of VARIANTS."""
    c = prep.c; M, N = c.M, c.N
    m_idx = np.arange(M) if rows is None else np.asarray(rows)
    acc = np.asarray(acc, np.float32); assert acc.shape == (len(m_idx), N)
    bufs = [b.copy() for b in prep.bufs]; masks = [np.zeros(b.shape, bool) for b in bufs]
    n = np.arange(N)
    mm, nn = np.meshgrid(m_idx, n, indexing="ij")
    bias = prep.bias if prep.bias is not None else None
    if bias is not None and variant == "bias_by_position":
        bias = bias[kperm(n)]
    scale = prep.scale
    pre = None

    def put(k, off, val):
        assert off.min() >= 0 and off.max() < bufs[k].size and np.unique(off).size == off.size, "an output element outside its buffer or written twice"
        bufs[k][off.reshape(-1)] = val.reshape(-1); masks[k][off.reshape(-1)] = True

    def scaled16(v):                                                        # f16((v + bias) * scale), the multiply skipped when the launch has no scale
        if variant == "scale_before_bias":
            t = v * scale + bias
        else:
            t = v + bias[None, :] if bias is not None else v
            if variant == "round_before_scale":
                t = t.astype(np.float16).astype(np.float32)
            if c.scale:
                t = t * scale
        with np.errstate(over="ignore"):
            return t.astype(np.float16).view(np.uint16)

    if c.epi == EPI_F32:
        v = acc + bias[None, :] if bias is not None else acc
        if prep.res is not None:
            v = v + prep.res[m_idx]
        put(0, mm * prep.ldc + nn, v)
    elif c.epi in (EPI_F16_PLAIN, EPI_F16_KPERM, EPI_HEADS_F16):
        o = scaled16(acc)
        if c.epi == EPI_HEADS_F16:
            off = heads_off(mm // c.n_ctx, mm % c.n_ctx, nn, prep.H, c.Tpad)
        elif c.frag:
            off = kfrag_off(mm // c.n_ctx, prep.H, c.Tpad, mm % c.n_ctx, nn)
        else:
            off = mm * prep.ldc + (kperm(nn) if c.epi == EPI_F16_KPERM else nn)
        put(0, off, o)
    elif c.epi == EPI_VT_F16:
        v = acc + bias[None, :] if bias is not None else acc
        o = v.astype(np.float16).view(np.uint16)
        b, key = mm // c.n_ctx, mm % c.n_ctx
        offf = (lambda b_, f_, k_: vtfrag_off(b_, prep.H, c.Tpad, f_, kperm(k_))) if c.frag else (lambda b_, f_, k_: vt_off(b_, f_, k_, prep.H, c.Tpad))
        put(0, offf(b, nn, key), o)
        if rows is None:                                                    # pad keys n_ctx .. Tpad of every clip: +0 (the kernel computes them on a copy of the clip's last row)
            B = M // c.n_ctx
            bb, ff, kk = np.meshgrid(np.arange(B), n, np.arange(c.n_ctx, c.Tpad), indexing="ij")
            padv = np.zeros(bb.shape, np.uint16)
            if variant == "pads_not_zeroed":
                padv = np.broadcast_to(o.reshape(B, c.n_ctx, N)[:, -1, :, None], bb.shape).copy()
            put(0, offf(bb, ff, kk), padv)
    elif c.epi == EPI_DEC_QKV:
        d = N // 3
        if variant == "scale_before_bias":
            t = np.where(nn < 2 * d, acc * scale, acc) + (bias[None, :] if bias is not None else 0)
        else:
            t = acc + bias[None, :] if bias is not None else acc
            if variant == "round_before_scale":
                t = t.astype(np.float16).astype(np.float32)
            t = np.where(nn < 2 * d, t * scale, t)
        o = t.astype(np.float32).astype(np.float16).view(np.uint16)
        pos = prep.pos.astype(np.int64)
        if variant == "pos_row0":
            pos = np.full_like(pos, pos[0])
        po = (m_idx * prep.ldc2 + pos[m_idx] * d)[:, None]
        put(0, mm[:, :d] * prep.ldc + nn[:, :d], o[:, :d])
        put(1, po + (nn[:, d:2 * d] - d), o[:, d:2 * d])
        put(2, po + (nn[:, 2 * d:] - 2 * d), o[:, 2 * d:])
    else:                                                                   # the GELU epilogues
        v = acc + bias[None, :] if bias is not None else acc
        x16 = v.astype(np.float16).astype(np.float32)
        near = gelu64(x16).astype(np.float16)
        if c.epi == EPI_CONV2:
            pe = prep.pe[mm % c.n_ctx, nn]
            off = mm * prep.ldc + nn
            put(0, off, pe + near.astype(np.float32))
        else:
            pe = None
            p = kperm(nn)
            if c.epi == EPI_GELU_F16_KPERM_ROWPAD:
                off = rowpad(mm, c.n_ctx) * prep.ldc + p
            elif c.c_frag:
                off = afrag_off(mm, p, N)
            else:
                off = mm * prep.ldc + p
            put(0, off, near.view(np.uint16))
        pre = (off, x16, pe)
    return bufs, masks, pre


# ---------------------------------------------------------------------------------------------------------------- what the engine launches in f16_mfma
# Every (launcher family, epilogue, flags) skw_engine.hip launches in the f16_mfma precision, enumerated by hand from its call sites (run_conv, run_encoder, the decoder step with
# its prompt pass): tests/test_cpu_gemm16_cases.py asserts that cases() covers each.  Flags: res (alias: the residual is C), scale, frag, conv (batch-strided overlapping A rows),
# a_frag, c_frag.
ENGINE_LAUNCHES = {
    ("big", EPI_GELU_F16_KPERM_ROWPAD, ""),            # conv1
    ("big", EPI_CONV2, "conv"),                         # conv2
    ("big", EPI_HEADS_F16, ""),                         # encoder Q, K
    ("big", EPI_VT_F16, ""),                            # encoder V^T, cross V^T (rows)
    ("big", EPI_VT_F16, "frag"),                        # cross V^T (fragment order)
    ("big", EPI_F32, "res-alias"),                      # O projection, FC2; the prompt pass's O / cross O / FC2
    ("big", EPI_GELU_F16_KPERM, ""),                    # FC1; the prompt pass's FC1
    ("big", EPI_F16_PLAIN, "scale"),                    # cross K (rows); the prompt pass's cross query
    ("big", EPI_F16_PLAIN, "scale,frag"),               # cross K (fragment order)
    ("small", EPI_DEC_QKV, "scale"),                    # layer 0's QKV (its LayerNorm is the embedding kernel's); every layer with the fold off
    ("small", EPI_F32, "res-alias"),                    # O, cross O, FC2 from rows
    ("small", EPI_F32, "res-alias,a_frag"),             # the same from the attention kernels' / FC1's fragment-order image
    ("small", EPI_F16_PLAIN, "scale"),                  # cross query (fold off)
    ("small", EPI_GELU_F16_KPERM, ""),                  # FC1 (fold off)
    ("small", EPI_GELU_F16_KPERM, "c_frag"),
    ("lna", EPI_DEC_QKV, "scale"),
    ("lna", EPI_F16_PLAIN, "scale"),
    ("lna", EPI_GELU_F16_KPERM, ""),
    ("lna", EPI_GELU_F16_KPERM, "c_frag"),
    ("vocab", EPI_F32, ""),                             # logits
}


def launch_key(c):
    flags = [f for f, on in (("res-alias", c.res == "alias"), ("res", c.res == "separate"), ("scale", c.scale), ("frag", c.frag), ("conv", c.conv), ("a_frag", c.a_frag),
                             ("c_frag", c.c_frag)) if on]
    return (c.family, c.epi, ",".join(flags))
