"""The decode cross attention over q8_0 cross K / V (include/skw_kv8.h) restated in numpy: the quantiser, the bit-exact scores, the float64 reference with its bound, an
emulation of the kernel's arithmetic and the case list (no GPU, none of the C code).  Shared by tests/test_cpu_kv8_cases.py and tests/test_gpu_kv8.py.

(a) quantize_slot   K rows and V^T rows through q8_ref_lib.quantize_rows; a key at or past the count is zero for the quantiser BY INDEX (its value is never looked at)
(b) scores          s = (0 + (dk0 dq0) f32(i0)) + (dk1 dq1) f32(i1), every operation a separate float32 numpy operation (numpy fuses nothing); the integer dots in int64
(c) reference       float64 softmax over the contract's scores, times V^ = d qs in float64
(d) THE BOUND.  The kernel's scores ARE the contract's (held bit for bit), so the reference takes them as they are and owes nothing for K's or q's quantisation, nor for V's:
    V^ is exact in the kernel too (int8 widened to f16 exactly, the f16 scale applied in f32).  What is left is attn_ref_lib.reference's account, term by term:
      1. every probability is rounded to f16 once: relative 2^-11 on the numerator              -> 2^-11 sum_k p_k |v^_kc|
      2. the normaliser is the sum of those rounded values: relative 2^-11 on the denominator   -> 2^-11 sum_k p_k |v^_kc|
      3. the output is rounded to f16 once                                                      -> 2^-11 sum_k p_k |v^_kc|
      4. one spare unit of 2^-11 for everything done in f32: the exp2 argument (|s - m| log2 e in one fma: |s - m| 2^-24, under 2^-17 for |s - m| < 128), v_exp_f32 (1 ulp),
         the rescales when the maximum grows (2^-24 each, at most 12 per wave), the MFMA's f32 accumulation of 32 exact products per block (32 x 2^-24), the final combine
         and division (a few 2^-24) — and, new here, ONE f32 rounding per block for o = fma(dv, blocksum, o): 47 blocks x 2^-24 = 2^-18.4.  Together below 2^-15 of
         sum_k p_k |v^_kc|: far inside the unit of 2^-11 = 8192 x 2^-24.
      5. a probability below 2^-14 is an f16 subnormal: absolute error 2^-25 against a normaliser >= 1 (the largest p of the row is exactly 1 in its wave, and a wave's share
         only shrinks in the combine)                                                           -> 2^-24 sum_k |v^_kc|
    |got - ref| <= 2^-9 sum_k p_k |v^_kc| + 2^-24 sum_k |v^_kc|     — attn_ref_lib's bound over V^; derived, not fitted.
(e) emulate         the kernel's arithmetic: four waves taking every fourth 32-key block, running maximum, f16 probabilities, per-block f32 sums scaled by dv in one fma
(f) cases()         on attn_ref_lib's operand generator and its loud keys; the >= 2 % mass of every loud key is asserted again HERE on the contract's softmax (q8 rounding of
                    q[62] = 1/16 and of the loud rows moves it by a few per cent of itself; the assertion is the same, not a looser one)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref_lib as ar  # noqa: E402
from q8_ref_lib import quantize_rows  # noqa: E402

F = np.float32
KEY_COUNTS = [1, 31, 32, 33, 129, 1500]
N_CTX = 1500
K_PAD = V_PAD = 0x7E00      # NaN in every f16 pad position of K and V


def quantize_slot(K, V, count):
    """K, V [n >= count][d] float16 -> kq int32 [T][d], kd f32 [T][d / 32], vq int32 [T][d], vd f32 [T / 32][d] for the T = 32 ceil(count / 32) keys of the written blocks"""
    d = K.shape[1]; T = (count + 31) // 32 * 32
    Kp = np.zeros((T, d), F); Kp[:count] = np.asarray(K[:count], F)
    Vp = np.zeros((T, d), F); Vp[:count] = np.asarray(V[:count], F)
    q, kd, _ = quantize_rows(Kp)
    qv, dv, _ = quantize_rows(np.ascontiguousarray(Vp.T))
    return q.reshape(T, d), kd, np.ascontiguousarray(qv.reshape(d, T).T), np.ascontiguousarray(dv.T)


REC, SCALES = 4352, 4096      # bytes per (slot, head, 32-key block) record; the scales' offset inside it


def image_offsets(H, n_ctx, T):
    """include/skw_kv8.h's offset functions restated on whole arrays, for keys [0, T) of slot 0 -> byte offsets kq [T][d], kd [T][2 H], vq [T][d], vd [T / 32][d]
    (tests/test_gpu_kv8.py holds them to the exported skw_layout_kv8_* functions on one case, then unpacks every case and slot with them)"""
    d = H * 64; nb = ((n_ctx + 31) // 32 * 32) // 32
    key = np.arange(T, dtype=np.int64)[:, None]; f = np.arange(d, dtype=np.int64)[None, :]
    rec = ((f >> 6) * nb + (key >> 5)) * REC
    dd = f & 63; r = key & 15; i = 4 * (r & 3) + (r >> 2); kl = key & 31
    kq = rec + ((key >> 4) & 1) * 1024 + (i + 16 * ((dd >> 3) & 3)) * 16 + (dd >> 5) * 8 + (dd & 7)
    kd = (rec + SCALES + (16 * (kl & 3) + (kl >> 2)) * 4 + ((f >> 5) & 1) * 2)[:, ::32]
    c = dd; ct = c >> 4
    vq = rec + 2048 + (ct >> 1) * 1024 + ((c & 15) + 16 * (kl & 3)) * 16 + (ct & 1) * 8 + (kl >> 2)
    vd = (rec + SCALES + (16 * ((c >> 2) & 3) + 8 + 2 * ct + ((c >> 1) & 1)) * 4 + (c & 1) * 2)[::32]
    return kq, kd, vq, vd


def unpack_image(img, H, n_ctx, T):
    """one slot's image (uint8) -> K qs int8 [T][d], K scales f32 [T][2 H], V qs int8 [T][d], V scales f32 [T / 32][d]"""
    img = np.ascontiguousarray(img, np.uint8).ravel()
    kq, kd, vq, vd = image_offsets(H, n_ctx, T)
    f16 = lambda o: (img[o].astype(np.uint16) | (img[o + 1].astype(np.uint16) << 8)).view(np.float16).astype(F)      # noqa: E731
    return img[kq].view(np.int8), f16(kd), img[vq].view(np.int8), f16(vd)


def quantize_query(q):
    """q [R][64] float16 -> qq int32 [R][2][32], dq f32 [R][2]"""
    qq, dq, _ = quantize_rows(np.asarray(q, F).reshape(-1, 64))
    return qq, dq


def scores(q, kq, kd, h, count):
    """the contract's scores of queries q [R][64] (one head's) over keys [0, count) of head h -> f32 [R][count], bit for bit"""
    qq, dq = quantize_query(q)
    i0 = qq[:, 0].astype(np.int64) @ kq[:count, h * 64:h * 64 + 32].astype(np.int64).T
    i1 = qq[:, 1].astype(np.int64) @ kq[:count, h * 64 + 32:h * 64 + 64].astype(np.int64).T
    assert np.abs(i0).max(initial=0) < 2 ** 24 and np.abs(i1).max(initial=0) < 2 ** 24
    dd0 = (kd[None, :count, 2 * h] * dq[:, 0:1]).astype(F); t0 = (dd0 * i0.astype(F)).astype(F); s = (F(0) + t0).astype(F)
    dd1 = (kd[None, :count, 2 * h + 1] * dq[:, 1:2]).astype(F); t1 = (dd1 * i1.astype(F)).astype(F)
    return (s + t1).astype(F)


def vhat(vq, vd, h, count):
    """V^ = d qs of head h, float64 [count][64] (exact)"""
    return (vq[:, h * 64:h * 64 + 64].astype(np.float64) * np.repeat(vd[:, h * 64:h * 64 + 64].astype(np.float64), 32, axis=0))[:count]


def reference(s, Vh):
    """float64 softmax(s) V^ and the bound: attn_ref_lib.reference on scores given as they are (q = 1, K = s: its q K^T is s).  -> (out [R][64], bound, p [R][n])"""
    outs, bounds, ps = [], [], []
    for r in range(s.shape[0]):
        o, b, p = ar.reference(np.ones((1, 1)), s[r].astype(np.float64)[:, None], Vh, 1.0)
        outs.append(o[0]); bounds.append(b[0]); ps.append(p[0])
    return np.array(outs), np.array(bounds), np.array(ps)


def off_by_one(s, Vh):
    """attn_ref_lib.reference_off_by_one on the contract's scores: the last key dropped / one more key that repeats the last key's score with a zero V row -> (less, more) [R][64]"""
    less, more = [], []
    for r in range(s.shape[0]):
        a, b = ar.reference_off_by_one(np.ones((1, 1)), s[r].astype(np.float64)[:, None], Vh, 1.0)
        less.append(a[0]); more.append(b[0])
    return np.array(less), np.array(more)


def ratio(got, ref, bound):
    """|got - ref| / bound; where the bound is zero (a channel whose V^ is zero throughout) only an exact zero passes"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r[~np.isfinite(np.asarray(got, np.float64))] = np.inf
    return r


def emulate(s, vq, vd, h, count):
    """the kernel's arithmetic on its (bit-exact) scores s [R][count]: -> float64 [R][64] of the f16 outputs"""
    R = s.shape[0]; nb = (count + 31) // 32; c1 = ar.LOG2E
    vqh = vq[:, h * 64:h * 64 + 64].astype(F); vdh = vd[:, h * 64:h * 64 + 64].astype(F)
    sp = np.full((R, nb * 32), -np.inf, F); sp[:, :count] = s
    ms, ls, os_ = [], [], []
    for part in range(4):
        m = np.full(R, -np.inf, F); l = np.zeros(R, F); o = np.zeros((R, 64), F)
        for j in range(part, nb, 4):
            sb = sp[:, 32 * j:32 * j + 32]
            mn = np.maximum(m, sb.max(axis=1))
            with np.errstate(invalid="ignore"):
                a = np.where(np.isneginf(m), F(0), np.exp2((m - mn) * c1)).astype(F)
            p = np.exp2((sb * c1 - (mn * c1)[:, None]).astype(F)).astype(F).astype(np.float16).astype(F)
            l = (l * a + p.sum(axis=1, dtype=F)).astype(F)
            bsum = (p @ vqh[32 * j:32 * j + 32]).astype(F)
            o = ((o * a[:, None]).astype(F).astype(np.float64) + vdh[j][None, :].astype(np.float64) * bsum.astype(np.float64)).astype(F)
            m = mn
        ms.append(m); ls.append(l); os_.append(o)
    M = np.max(ms, axis=0)
    num = np.zeros((R, 64), F); den = np.zeros(R, F)
    for m, l, o in zip(ms, ls, os_):
        a = np.exp2((m - M) * c1).astype(F)
        num = (num + o * a[:, None]).astype(F); den = (den + l * a).astype(F)
    return (num / den[:, None]).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- the cases
class Case(ar.Case):
    """attn_ref_lib.Case (form "cross") plus: the quantiser's key count per slot, and on the larger cases an all-zero K block (d = 0) and an all-zero V^T block (d = 0)"""
    def __init__(self, name, H, n_ctx, profile, slots, rows, zero_blocks=False, **kw):
        super().__init__(name, "cross", H, n_ctx, profile, slots, rows, **kw)
        self.zero_blocks = zero_blocks

    def slot_k(self):
        return [max(c) for _, c in self.slots]

    def operands(self):
        Q, K, V, loud = super().operands()
        if self.zero_blocks:      # quiet key 2: its first K block; channel 5 of every head: the V^T block of keys 32 .. 63
            for s in range(K.shape[0]):
                assert 2 not in loud[s]
                for h in range(self.H):
                    K[s, 2, h * 64:h * 64 + 32] = 0; V[s, 32:64, h * 64 + 5] = 0
        return Q, K, V, loud

    def prepared(self):
        """-> Q, K, V and per live (slot, key count, head): (rows, channel slice, scores, V^, reference, bound); every loud key a row sees holds >= 2 % of its contract softmax"""
        Q, K, V, loud = self.operands()
        quant = [quantize_slot(K[s], V[s], n) for s, n in enumerate(self.slot_k())]
        groups = {}
        for r, (s, n) in enumerate(self.rows):
            if self.live[r]:
                groups.setdefault((s, n), []).append(r)
        refs = []
        for (s, n), rs in groups.items():
            kq, kd, vq, vd = quant[s]
            for h in range(self.H):
                sl = slice(h * 64, h * 64 + 64)
                sc = scores(Q[rs, sl], kq, kd, h, n); Vh = vhat(vq, vd, h, n)
                ref, bound, p = reference(sc, Vh)
                vis = loud[s][loud[s] < n]
                assert p[:, vis].min() >= ar.MIN_MASS, "%s slot %d, %d keys, head %d: a loud key holds %.4f of the contract's softmax mass" % (self.name, s, n, h, p[:, vis].min())
                refs.append((rs, s, n, h, sl, sc, Vh, ref, bound))
        for a in (Q, K, V):
            a.setflags(write=False)
        return Q, K, V, quant, refs


def cases():
    out = []
    act = [1, 0, 1, 1, 1]; seq = [0, 1, 2, 3, 2]      # row 1 inactive, row 4 on row 2's sequence
    # the key counts as n_ctx: the full-length instantiation (nkeys null), H = 1, 2, 4 — a ragged grid of three heads per workgroup
    for i, (H, n) in enumerate(((1, 1), (2, 31), (4, 32), (1, 33), (2, 129), (4, 1500), (1, 1500))):
        prof = ar.PROFILES[i % 6]
        out.append(Case("kv8_full_H%d_n%d_%s" % (H, n, prof), H, n, prof, [(n, [n])] * 4, [(s, n) for s in seq], zero_blocks=n >= 129, active=act, seq=seq,
                        live=[bool(a) for a in act]))
    # the same counts per row below n_ctx = 1500 (VARK); the fourth of each group is the inactive row's, row 4 attends over row 1's sequence with its own count
    groups = [[1, 33, 129, 100, 1500], [31, 1500, 32, 17, 1], [32, 129, 1500, 40, 33], [33, 31, 1, 500, 129]]
    act = [1, 1, 1, 0, 1]; seq = [0, 1, 2, 3, 1]
    for i, g in enumerate(groups):
        H = (1, 2, 4, 2)[i]; prof = ar.PROFILES[(i + 2) % 6]
        counts = [[g[0]], [g[1], g[4]], [g[2]], [g[3]]]
        out.append(Case("kv8_vark_H%d_k%d_%s" % (H, g[0], prof), H, N_CTX, prof, [(N_CTX, c) for c in counts], [(seq[r], g[r]) for r in range(5)], vark=True,
                        active=act, seq=seq, count=g, live=[bool(a) for a in act]))
    out.append(Case("kv8_vark_H4_one_k129_random", 4, N_CTX, "random", [(N_CTX, [129])], [(0, 129)], zero_blocks=True, vark=True, count=[129]))
    return out
