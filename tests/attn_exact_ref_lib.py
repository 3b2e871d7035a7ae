"""The exact precision's attention kernels against the contract, bit for bit: the numpy restatement, the operands and the case list (plain numpy, no GPU).

Shared by tests/test_cpu_attn_exact_cases.py (the restatement equals the oracle's arithmetic, the cases have teeth, no row's expectation depends on a summation order) and
tests/test_gpu_attn_exact.py (every exact-precision attention kernel equals the restatement in every output bit).  tests/test_gpu_q8.py holds k_dec_attn's f32 rows to it as well.

THE CONTRACT (include/skw_math.h; softmax_row2 and gemm_chain of oracle/skw_oracle.c), for query rows q over keys K, V of one head (64 channels, every operand f16-valued):
  1. s[q][j] = the d-ascending chain acc = fmaf(K[j][d], q[d], acc) from 0, d = 0 .. 63
  2. the encoder only: s = s * kq_scale, one f32 multiply, kq_scale = f32(1 / sqrt(64)); the decoder forms take pre-scaled q / k and multiply by nothing
  3. m = max_j s        4. e_j = skw_expf(s_j - m)        5. sum = the f64 sum of e_j, inv = (float)(1.0 / sum)        6. p_j = f16(e_j * inv)
  7. out[c] = the key-ascending chain acc = fmaf(p_j, V[j][c], acc) from 0        8. stored as f16 (kperm order in memory) or as the raw f32
Products of two f16 values are exact in f32, so a * b + c rounded once is the same whichever factor comes first; gemm16_ref_lib.fmaf is that operation.

THE f64 ROW SUM.  The kernels add it per lane, per wave and in four parts, not key by key as the oracle does; the contract calls an f64 sum of f32 terms order-insensitive.  That is
checkable: with S the exact sum (math.fsum), any order of n non-negative terms lands in [S (1 - n 2^-53), S (1 + n 2^-53)]; a row is ORDER-DEPENDENT when (float)(1.0 / x) is not one
f32 value over that interval, and such a row has no bit-exact expectation.  About 6e-6 of random rows are; the condition on this file is that NO row of any case is (asserted by the
CPU test; SEED_BUMP is where a case gets another seed if one turns up), so the GPU test never skips a row.

THE OPERANDS.  Seeded f16 values, scores of unit spread.  Up to four keys per slot are LOUD: 40 to 100 times an ordinary key, all along one direction per (slot, head), never the
last key of a key count in use nor the one after it.  Each head of each query row is turned so that the loud keys score far below the row's other keys — their s - max falls below skw_expf's clamp (-86)
and below exp's underflow (-104), which the single-pass encoder kernel evaluates without that clamp, while the rest of the row is an ordinary softmax in which the LAST key carries a
probability that is not zero (a dropped last key must show in every (slot, key count), single-query ones included: the CPU tier asserts it) — except in every eighth row of a
larger group, where a loud key takes all the mass and every other key is what falls under the clamp.  V carries a power-of-two scale per (slot, head).  What a kernel must not use is poisoned by the test hooks:
NaN in K and in every query row no sequence owns; in V NaN where the kernel promises to replace or not to read it, 1000.0 where it relies on p = 0 (the encoder kernels without
per-slot key counts multiply the pad keys' V by p = 0: NaN there would be the test's fault).

THE CASES are the smallest geometries that cross every edge — see each builder below."""
import math
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm16_ref_lib import fmaf, inv_kperm, kperm  # noqa: E402,F401

KQ_SCALE = np.float32(1.0) / np.sqrt(np.float32(64.0))
F16_NAN, F16_1000 = 0x7E00, 0x63D0
SENTINEL = 0x5A5A
N_TEXT_CTX = 448
LOUD = (40.0, 60.0, 80.0, 100.0)      # the loud keys' lengths, in units of an ordinary key's
# One query row per encoder slot is scaled by 2^-13: its elements lie below 2^-11, where multiplying by kq_scale = 2^-3 and rounding to f16 lands among the subnormals and loses
# bits.  In f32 the power of two commutes with every rounding of the chain (what k_attn_encoder_v3 relies on when it folds the scale into q); in f16 it does not, and only such a
# row can tell a kernel that scales q before it is stored as f16 from one that scales the score.
QUIET = 2.0 ** -13
SEED_BUMP = {}                            # case name -> added to its seed: set where a seed produced an order-dependent row (none did)


# ---------------------------------------------------------------------------------------------------------------- skw_expf
def _exp_poly(x):
    """the reduction and the polynomial of skw_expf (include/skw_math.h) -> (y, n): exp(x) = y 2^n"""
    n = np.rint(x * np.float32(1.44269504088896341))
    r = fmaf(n, np.float32(-0.693359375), x)
    r = fmaf(n, np.float32(2.12194440e-4), r)
    p = np.float32(1.9875691500e-4)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = fmaf(p, r, np.float32(c))
    y = fmaf(p, r * r, r) + np.float32(1.0)
    return y.reshape(x.shape), n


def skw_expf(x):
    """skw_expf for x <= 0 (or -inf): 0 below -86, else the polynomial scaled through the exponent bits"""
    x = np.asarray(x, np.float32)
    ok = x >= np.float32(-86.0)
    y, n = _exp_poly(np.where(ok, x, np.float32(0.0)))
    scale = ((n.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)
    return np.where(ok, y * scale, np.float32(0.0)).astype(np.float32)


def expf_unclamped(x):
    """expf_nonpos_x2_softmax of skw_kernels_attn_enc.hip for finite x <= 0: the same polynomial, ldexp instead of the clamp — below -86 a subnormal, some e < 2^-124, or 0"""
    x = np.asarray(x, np.float32)
    y, n = _exp_poly(x)
    return np.ldexp(y, n.astype(np.int32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the restatement
VARIANTS = ("q_scaled_f16", "p_f32", "div", "sum_f32", "key_desc", "d_desc")      # the named wrong kernels `attend` evaluates itself; "fewer", "more" and "pad_times_zero" are the caller's


def scores(q, K, scale=None, variant=None):
    """steps 1 and 2 -> s f32 [R][n]"""
    q = np.asarray(q, np.float32); K = np.asarray(K, np.float32)
    if variant == "q_scaled_f16":
        q = (q * scale).astype(np.float16).astype(np.float32); scale = None
    elif variant == "q_scaled_f32":
        q = q * scale; scale = None
    s = np.zeros((q.shape[0], K.shape[0]), np.float32)
    with np.errstate(invalid="ignore"):
        for d in (range(63, -1, -1) if variant == "d_desc" else range(64)):
            s = fmaf(K[None, :, d], q[:, d, None], s)
        if scale is not None:
            s = s * np.float32(scale)
    return s


def softmax(s, variant=None, exp=skw_expf):
    """steps 3 to 6 -> dict m, tot, inv, e, p (f32 [R][n], f16-valued)"""
    m = s.max(axis=1)
    with np.errstate(invalid="ignore"):
        e = exp(s - m[:, None])
    if variant == "sum_f32":
        tot = np.cumsum(e, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    else:
        tot = np.cumsum(e.astype(np.float64), axis=1)[:, -1]                   # (accumulate is sequential: the oracle's key-ascending sum)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = (1.0 / tot).astype(np.float32)
        p = (e.astype(np.float64) / tot[:, None]).astype(np.float32) if variant == "div" else e * inv[:, None]
    if variant != "p_f32":
        p = p.astype(np.float16).astype(np.float32)
    return dict(m=m, tot=tot, inv=inv, e=e, p=p)


def pv(p, V, variant=None):
    """step 7 -> out32 [R][64]"""
    V = np.asarray(V, np.float32); n = V.shape[0]
    out = np.zeros((p.shape[0], 64), np.float32)
    with np.errstate(invalid="ignore"):
        for j in (range(n - 1, -1, -1) if variant == "key_desc" else range(n)):
            out = fmaf(p[:, j, None], V[None, j, :], out)
    return out


def attend(q, K, V, scale=None, variant=None, exp=skw_expf, n_valid=None):
    """The contract for query rows q [R][64] over keys K, V [n][64].  scale: None (the decoder forms) or kq_scale.  n_valid: keys from there on are masked to -inf after the score
    chain, as a kernel that walks whole 32-key blocks masks its pad keys (their p = 0 then MULTIPLIES V in the P.V chain).  variant: None, one of VARIANTS, or "q_scaled_f32" (q times
    kq_scale in f32 before the chain: what k_attn_encoder_v3 does, claimed bit-identical).  -> dict s, m, tot, inv, e, p, out32 [R][64]"""
    s = scores(q, K, scale, variant)
    if n_valid is not None:
        s[:, n_valid:] = -np.inf
    r = softmax(s, variant, exp)
    r["s"] = s; r["out32"] = pv(r["p"], V, variant)
    return r


def order_dependent_rows(e):
    """the rows of e [R][n] (f32, >= 0) whose (float)(1.0 / sum) depends on the order of the f64 sum (see the file's head)"""
    n = e.shape[1]; bad = []
    for r in range(e.shape[0]):
        S = math.fsum(e[r].astype(np.float64).tolist())
        lo, hi = np.nextafter(S * (1.0 - n * 2.0 ** -53), 0.0), np.nextafter(S * (1.0 + n * 2.0 ** -53), np.inf)
        if np.float32(1.0 / lo) != np.float32(1.0 / hi):
            bad.append(r)
    return bad


# ---------------------------------------------------------------------------------------------------------------- the cases
class Group:
    """query rows that share a (slot, key count): qrows index the case's flat Q, orows the output buffer; exact[i]: row i has a bit-exact expectation (all, but for the 1500-key
    encoder cases, whose other rows are held to float64 under attn_ref_lib's bound)"""
    def __init__(self, slot, n, qrows, orows, exact=None):
        self.slot, self.n = slot, n
        self.qrows, self.orows = np.asarray(qrows, np.int64), np.asarray(orows, np.int64)
        self.exact = np.ones(self.qrows.size, bool) if exact is None else exact


class Case:
    """One set of operands and the launches over it.  kernel: "enc3" (k_attn_encoder), "encv3" (k_attn_encoder_v3), "self" (k_dec_attn<7>), "cross" (k_dec_cross_attn<24,4,3> and
    k_xattn_prefill_exact).  q_rows: rows of the flat Q (the encoder's is [slot][n_ctx]); fill_from[slot]: keys below it are the operands', from there on the pads."""
    def __init__(self, name, kernel, H, n_ctx, n_slots, q_rows, n_out, groups, fill_from, vark, launch):
        self.name, self.kernel, self.H, self.n_ctx, self.n_slots, self.q_rows, self.n_out = name, kernel, H, n_ctx, n_slots, q_rows, n_out
        self.groups, self.fill_from, self.vark, self.launch = groups, list(fill_from), vark, launch
        self.scale = KQ_SCALE if kernel in ("enc3", "encv3") else None
        self.seed = zlib.crc32(name.encode()) + SEED_BUMP.get(name, 0)

    def pads(self):
        """(k_pad, v_pad): NaN in K; in V NaN where the kernel replaces the pad keys or never reads them, 1000.0 where it multiplies them by p = 0"""
        return F16_NAN, (F16_1000 if self.kernel in ("enc3", "encv3") and not self.vark else F16_NAN)

    def operands(self):
        """-> Q [q_rows][H*64], K, V [n_slots][n_ctx][H*64] float16, natural order"""
        rng = np.random.default_rng(self.seed)
        d = self.H * 64
        Q = (rng.standard_normal((self.q_rows, d)) * (2.0 if self.scale is not None else 0.25)).astype(np.float16)      # (scores of unit spread either way: the encoder's q is unscaled, 2.0 * 0.5 * 8 * kq_scale)
        K = (rng.standard_normal((self.n_slots, self.n_ctx, d)) * 0.5).astype(np.float16)
        vs = np.exp2(rng.integers(-2, 3, (self.n_slots, 1, self.H)).astype(np.float64)).repeat(64, axis=2)
        V = (rng.standard_normal((self.n_slots, self.n_ctx, d)) * vs).astype(np.float16)
        # the loud keys: per slot up to four keys, never a group's last one or the next, along ONE direction u per (slot, head) with growing lengths, so that a query sees them all on the same side
        u = rng.standard_normal((self.n_slots, d)) * 0.5
        for s in range(self.n_slots):
            cand = np.setdiff1d(np.arange(self.fill_from[s]), [g.n - 1 + i for g in self.groups if g.slot == s for i in (0, 1)])      # (nor the key just past one: a row on a longer cache)
            for i, k in enumerate(rng.choice(cand, size=min(len(LOUD), cand.size, self.fill_from[s] // 2), replace=False)):
                K[s, k] = (u[s] * LOUD[i]).astype(np.float16)
        # ... and which side: a head of a query row is turned round (q -> -q) where needed, so that the loud keys score far BELOW the rest (their s - max is what falls under the
        # clamp; the row's other keys keep an ordinary softmax, and its last key a probability that is not zero) — but far ABOVE for every eighth row of a group of eight or more
        # (row 5, 13, ..: one loud key takes all the mass and every other key of the row is what falls under the clamp)
        for g in self.groups:
            for i, r in enumerate(g.qrows):
                above = g.qrows.size >= 8 and i % 8 == 5
                for h in range(self.H):
                    sl = slice(h * 64, h * 64 + 64)
                    if (float(Q[r, sl].astype(np.float64) @ u[g.slot, sl]) > 0) != above:
                        Q[r, sl] = -Q[r, sl]
        for g in self.groups if self.scale is not None else ():             # the encoder's last query of every slot is QUIET: q 2^-3 would be an f16 subnormal (see QUIET)
            Q[g.qrows[-1]] = (Q[g.qrows[-1]].astype(np.float32) * np.float32(QUIET)).astype(np.float16)
        return Q, K, V

    def q_bits(self, Q):
        """Q as the hooks take it: uint16, every row no group owns poisoned"""
        owned = np.zeros(self.q_rows, bool)
        for g in self.groups:
            owned[g.qrows] = True
        b = Q.view(np.uint16).copy(); b[~owned] = F16_NAN
        return b

    def written(self):
        w = np.zeros(self.n_out, bool)
        for g in self.groups:
            w[g.orows] = True
        return w

    def kv(self, K, V, slot, head, n_total):
        """keys 0 .. n_total of (slot, head) as the kernel finds them: the operands below fill_from, the pads from there on (also past n_ctx) -> K, V float32 [n_total][64]"""
        sl = slice(head * 64, head * 64 + 64)
        kp, vp = (np.array([b], np.uint16).view(np.float16)[0] for b in self.pads())
        k = np.full((n_total, 64), kp, np.float32); v = np.full((n_total, 64), vp, np.float32)
        f = min(self.fill_from[slot], n_total)
        k[:f] = K[slot, :f, sl]; v[:f] = V[slot, :f, sl]
        return k, v


def _enc_case(name, kernel, H, n_ctx, slot_k, out_rows=0, exact_rows=None):
    vark = not isinstance(slot_k, int)                                       # slot_k: the slots' key counts, or the number of full-length slots
    counts = list(slot_k) if vark else [n_ctx] * slot_k
    S = len(counts)
    stride = out_rows if out_rows else n_ctx
    groups = []
    for s, n in enumerate(counts):
        ex = None
        if exact_rows is not None:
            ex = np.zeros(n, bool); ex[exact_rows(n, zlib.crc32(("%s/%d" % (name, s)).encode()))] = True
        groups.append(Group(s, n, s * n_ctx + np.arange(n), s * stride + np.arange(n), ex))
    return Case(name, kernel, H, n_ctx, S, S * n_ctx, S * stride, groups, counts, vark, dict(slot_k=counts if vark else None, out_rows=out_rows))


ENC3_N_CTX = [1, 31, 32, 33, 127, 128, 129, 160]
# per context length three slots' key counts: every set has a slot that ends inside a 32-key block (its pad keys' V must be replaced); together they put a slot on either side of
# the 32-key block edges 32 and 128 / 96 and of the 128-query tile edge, and one slot of a single key next to longer ones
ENC3_SLOT_K = {1: [1, 1, 1], 31: [31, 1, 17], 32: [32, 31, 1], 33: [33, 32, 1], 127: [127, 96, 97], 128: [128, 127, 1], 129: [129, 128, 33], 160: [129, 1, 160]}


def _enc3_cases():
    """k_attn_encoder: Tpad = ceil32(n_ctx); 3 slots; H 1 and 3; without per-slot counts (the pad keys n_ctx .. Tpad masked, V there finite) and with them (out_rows > slot_k in every
    set: the rows at and past a slot's count keep the sentinel; at n_ctx 160 also out_rows = 192 > n_ctx)"""
    out = []
    for n_ctx in ENC3_N_CTX:
        for H in (1, 3):
            out.append(_enc_case("enc3_n%d_H%d" % (n_ctx, H), "enc3", H, n_ctx, 3))
            out.append(_enc_case("enc3_n%d_H%d_slotk" % (n_ctx, H), "enc3", H, n_ctx, ENC3_SLOT_K[n_ctx], out_rows=192 if (n_ctx == 160 and H == 3) else 0))
    return out


def v3_exact_rows(n, seed):
    """the rows of a 1500-key slot held bit for bit: the first two and the last two 64-query tiles and 64 seeded rows between them"""
    tiles = (n + 63) // 64
    mid = np.random.default_rng(seed).choice(np.arange(128, (tiles - 2) * 64), size=64, replace=False)
    return np.concatenate([np.arange(128), np.sort(mid), np.arange((tiles - 2) * 64, n)])


def _encv3_cases():
    """k_attn_encoder_v3<94, 72>: Tpad 1504 and fewer than 16 pad keys is the only geometry the launcher sends there — 1489 (15 pad keys, the most), 1500 (Whisper's), 1504 (none)"""
    return [_enc_case("encv3_n%d_H2" % n_ctx, "encv3", 2, n_ctx, 2, exact_rows=v3_exact_rows) for n_ctx in (1489, 1500, 1504)]


SELF_POS = [0, 1, 62, 63, 64, 127, 128, 447]


SELF_SHARED = 128                         # rows 10 .. 137 read sequence 7's full cache at pos 447, each with its own q: rows enough for a last-bit change of a probability to show


def _self_cases():
    """k_dec_attn<7>, fastv = 0: one row per pos (n_kv = pos + 1: one key, either side of the 64-key pass and of the 128 prefetched V rows, the whole cache), row 8 inactive (its
    cache holds nothing but NaN), row 9 reads sequence 5's cache (filled to 128) at pos 100, rows 10 .. 137 sequence 7's.  H 4 (one full four-head block) and 6 (the second block is
    ragged)."""
    out = []
    pos = SELF_POS + [30, 100] + [447] * SELF_SHARED; active = [1] * 8 + [0, 1] + [1] * SELF_SHARED; seq = list(range(9)) + [5] + [7] * SELF_SHARED
    R = len(pos)
    for H in (4, 6):
        filled = [0] * 10
        for b in range(R):
            if active[b]:
                filled[seq[b]] = max(filled[seq[b]], pos[b] + 1)
        groups = [Group(seq[b], pos[b] + 1, [b], [b]) for b in range(10) if active[b]] + [Group(7, 448, np.arange(10, R), np.arange(10, R))]
        out.append(Case("self_H%d" % H, "self", H, N_TEXT_CTX, 10, R, R, groups, filled, True, dict(pos=pos, active=active, seq=seq)))
    return out


CROSS_N_CTX = [1, 33, 64, 65, 257, 1500]      # 1, 1, 1, 2, 5, 24 tiles of 64 keys over four waves: at 1, 2 and 5 some waves have no tile and only zero-fill
CROSS_SLOT_K = {1: [1, 1, 1], 33: [31, 32, 33], 64: [63, 64, 33], 65: [65, 64, 1], 257: [255, 256, 257], 1500: [1473, 321, 1500]}      # either side of a 32- and of a 64-key edge
CROSS_NQ, CROSS_GAP = (17, 1, 48), 3      # three sequences, unowned rows between them; 17 and 48 queries: either side of a workgroup's 16
CROSS_SLOTS = [(2, 0, 1), (0, 2, 1), (1, 2, 0), (2, 1, 0), (1, 0, 2)]      # the sequences' slots, never in ascending order; taken in turn, so each slot count meets each sequence length


def _cross_cases():
    """k_dec_cross_attn<24, 4, 3> (mq = 0) and k_xattn_prefill_exact (mq = 1) through skw_debug_xattn_exact.  H 1 (one workgroup with two invalid head slots) and 4 (the first
    workgroup's third head slot is valid, the second has two invalid ones)."""
    out = []
    row0 = []; at = CROSS_GAP
    for n in CROSS_NQ:
        row0.append(at); at += n + CROSS_GAP
    rows = at
    for n_ctx in CROSS_N_CTX:
        for H in (1, 4):
            for vark in (False, True):
                counts = CROSS_SLOT_K[n_ctx] if vark else [n_ctx] * 3
                slot = CROSS_SLOTS[len(out) % len(CROSS_SLOTS)]
                groups = [Group(slot[i], counts[slot[i]], np.arange(row0[i], row0[i] + CROSS_NQ[i]), np.arange(row0[i], row0[i] + CROSS_NQ[i])) for i in range(3)]
                out.append(Case("cross_n%d_H%d%s" % (n_ctx, H, "_slotk" if vark else ""), "cross", H, n_ctx, 3, rows, rows, groups, counts, vark,
                                dict(row0=row0, nq=list(CROSS_NQ), slot=list(slot), slot_k=counts if vark else None)))
    return out


def cases():
    return _enc3_cases() + _encv3_cases() + _self_cases() + _cross_cases()


# ---------------------------------------------------------------------------------------------------------------- expectations
def expected(case, ops=None, keep=False):
    """The restatement over every (group, head) of a case, on the rows with a bit-exact expectation -> list of dict(group, head, rows (indices into the group), out32 [rows][64])
    (keep: s, m, tot, inv, e, p as well)"""
    Q, K, V = ops if ops is not None else case.operands()
    recs = []
    for g in case.groups:
        rows = np.flatnonzero(g.exact)
        for h in range(case.H):
            sl = slice(h * 64, h * 64 + 64)
            r = attend(Q[g.qrows[rows], sl], K[g.slot, :g.n, sl], V[g.slot, :g.n, sl], case.scale)
            rec = dict(group=g, head=h, rows=rows, out32=r["out32"])
            if keep:
                rec.update({k: r[k] for k in ("s", "m", "tot", "inv", "e", "p")})
            recs.append(rec)
    return recs


def stored_f16(out32):
    """step 8, the f16 form: the bits of the row in natural order (the hooks un-permute kperm)"""
    return np.asarray(out32, np.float32).astype(np.float16).view(np.uint16)
