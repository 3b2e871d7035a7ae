"""The f16_mfma attention kernels against a float64 softmax(scale Q K^T) V: the reference, the error bound, the operand generator and the case list (plain numpy, no GPU).

Shared by tests/test_cpu_attn_cases.py (the cases have teeth, the bound is sane) and tests/test_gpu_attn16.py (every launcher under the bound).

THE BOUND.  The kernels round every probability to f16 once (relative 2^-11; absolute 2^-25 where the value is an f16 subnormal), normalise by the sum of those rounded values and
round the output to f16 once: three units of 2^-11 on sum_k p_k |v_kc|.  One more unit covers the f32 accumulation, the exp2 argument and the division:
    |got - ref| <= 2^-9 sum_k p_k |v_kc| + 2^-24 sum_k |v_kc|
It is derived, not fitted; a kernel over it is a finding.

THE OPERANDS.  With random scores an off-by-one in the key count (one pad key in the denominator, the last real key dropped) moves the output by a fraction of this bound once there
are a few hundred keys.  So every case makes some keys LOUD: the last real key of every key count in use and the keys on either side of the 32- and 64-key block boundaries below it
(key 0 too in the descending profile, which wants the first block to hold the maximum).  Each loud key must carry >= 2 % of every query's softmax mass (asserted on the reference),
so there can be at most 50 of them; the generator keeps LOUD_CAP = 24 per slot — at key counts past ~380 those nearest the last key, where a miscounted loop goes wrong.  Two head
dimensions are reserved for it: q[63] = 1 and q[62] = 1/16 in every query, K[key][63] = A and K[key][62] = 16 delta in the loud keys only, whose other dimensions are zero: a loud
key's score is A + delta for every query.  A puts 80 % of the worst query's mass on the loud keys together; delta (0 .. 0.3) orders them in the ascending / descending profiles.
Channel 0 of every head holds |v|, so that sum_k p_k v_k0 = sum_k p_k |v_k0| there and a change of the normaliser by a factor (1 + w) shows as w / 2^-9 bounds."""
import numpy as np

LOUD_CAP = 24
MIN_MASS = 0.02
PROFILES = ["random", "ascending", "descending", "flat", "peaked", "loud"]
LOG2E = np.float32(1.44269504088896340736)


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16)


def loud_keys(counts, profile="random", cap=LOUD_CAP):
    """The loud keys of a slot whose rows use the key counts `counts`: per count n the key n - 1 and the keys 32 j - 1, 32 j below it, nearest first, cap // len(counts) of them."""
    counts = sorted(set(int(n) for n in counts))
    per = max(1, cap // len(counts))
    out = set()
    for n in counts:
        mine = [n - 1]
        for b in range(((n - 1) // 32) * 32, 0, -32):      # every 64-key boundary is a 32-key boundary
            for k in (b, b - 1):
                if k < n - 1 and k not in mine:
                    mine.append(k)
        mine = mine[:per]
        if profile == "descending" and n > 1 and 0 not in mine:
            mine[-1 if len(mine) == per and len(mine) > 1 else len(mine):] = [0]
        out.update(mine)
    return np.array(sorted(out), np.int64)


def reference(q, K, V, scale):
    """float64 softmax(scale q K^T) V and the bound, for queries q [R][64] over keys K, V [n][64] (f16-valued).  n == 0: zeros.  -> (out [R][64], bound [R][64], p [R][n])"""
    q = np.asarray(q, np.float64); K = np.asarray(K, np.float64); V = np.asarray(V, np.float64)
    if K.shape[0] == 0:
        z = np.zeros((q.shape[0], V.shape[1])); return z, z.copy(), np.zeros((q.shape[0], 0))
    s = scale * (q @ K.T)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p @ V, 2.0 ** -9 * (p @ np.abs(V)) + 2.0 ** -24 * np.abs(V).sum(axis=0)[None, :], p


def reference_off_by_one(q, K, V, scale):
    """The two miscounts: the last key dropped, and one more key counted that repeats the last key's K row with a zero V row.  -> (out over n - 1 keys, out over n + 1 keys)"""
    q = np.asarray(q, np.float64); K = np.asarray(K, np.float64); V = np.asarray(V, np.float64)
    s = scale * (q @ K.T)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    num = e @ V; den = e.sum(axis=1, keepdims=True); el = e[:, -1:]
    less = (num - el * V[-1][None, :]) / (den - el) if K.shape[0] > 1 else np.zeros_like(num)
    return less, num / (den + el)


def emulate(q, K, V, scale, block):
    """The kernels' arithmetic in numpy: f32 scores, a running maximum per `block` keys with a rescale of the accumulators when it grows, probabilities exp2((s - m) scale log2 e)
    rounded to f16, their f32 sum as the normaliser, f32 accumulation of p v, one f16 rounding of the output."""
    q = np.asarray(q, np.float32); K = np.asarray(K, np.float32); V = np.asarray(V, np.float32)
    R, n = q.shape[0], K.shape[0]
    c1 = np.float32(scale) * LOG2E
    m = np.full(R, -np.inf, np.float32); l = np.zeros(R, np.float32); o = np.zeros((R, V.shape[1]), np.float32)
    for k0 in range(0, n, block):
        s = (q @ K[k0:k0 + block].T).astype(np.float32)
        mn = np.maximum(m, s.max(axis=1))
        with np.errstate(invalid="ignore"):
            a = np.where(np.isneginf(m), np.float32(0), np.exp2((m - mn) * c1)).astype(np.float32)
        p = np.exp2(s * c1 - (mn * c1)[:, None]).astype(np.float32).astype(np.float16).astype(np.float32)
        l = (l * a + p.sum(axis=1, dtype=np.float32)).astype(np.float32)
        o = (o * a[:, None] + (p @ V[k0:k0 + block]).astype(np.float32)).astype(np.float32)
        m = mn
    return (o / l[:, None]).astype(np.float16).astype(np.float64)


def make_operands(seed, profile, H, scale, slots, rows):
    """Operands of one launch.  slots: per slot (n_store, [key counts in use]); rows: per query row (slot, key count).  -> Q [R][H*64], K, V [S][n_store][H*64] float16 (keys
    past a slot's largest count are zero: the debug entry poisons them), loud[slot] the loud keys.  Asserts on the reference that every loud key a row sees has >= 2 % of its mass."""
    rng = np.random.default_rng(seed)
    R, S, n_store = len(rows), len(slots), slots[0][0]
    assert all(s[0] == n_store for s in slots) and profile in PROFILES
    Q = np.zeros((R, H, 64)); K = np.zeros((S, n_store, H, 64)); V = np.zeros((S, n_store, H, 64))
    inv = 1.0 / scale                                                     # the encoder form scales inside the kernel: its K carries 1 / scale
    Q[:, :, :62] = 0.0 if profile == "flat" else rng.standard_normal((R, H, 62)) * {"ascending": 0.05, "descending": 0.05, "loud": 0.05, "peaked": 0.1}.get(profile, 1.0)
    if profile in ("ascending", "descending", "loud"):
        Q[:, :, 0] = 1.0
    Q[:, :, 62] = 1.0 / 16; Q[:, :, 63] = 1.0
    loud = []
    for s, (_, counts) in enumerate(slots):
        n = max(counts); lk = loud_keys(counts, profile); loud.append(lk)
        k = rng.standard_normal((n, H, 62)) * (2.0 / np.sqrt(62.0))
        if profile == "ascending":
            k[:, :, 0] = 0.02 * np.arange(n)[:, None]
        elif profile == "descending":
            k[:, :, 0] = 0.02 * (n - 1 - np.arange(n))[:, None]
        elif profile == "loud":
            k[:, :, 0] = 60.0 * rng.choice([-1.0, 1.0], (n, H))
        K[s, :n, :, :62] = k * inv
        K[s, lk, :, :] = 0.0
        v = rng.standard_normal((n, H, 64)) * np.exp2(rng.integers(-2, 3, (n, 1, 1)).astype(np.float64))
        v[lk] = rng.standard_normal((lk.size, H, 64)) * 4.0
        v[:, :, 0] = np.abs(v[:, :, 0])
        V[s, :n] = v
    Q = f16(Q); K = f16(K); V = f16(V)
    # the loud keys' score A + delta, from the f16-valued operands: 80 % of the mass of the query with the heaviest quiet keys (peaked: 2^24.1 .. 2^24.6 above the loudest quiet key)
    for s, (_, counts) in enumerate(slots):
        n = max(counts); lk = loud[s]; quiet = np.setdiff1d(np.arange(n), lk)
        mine = [r for r, (rs, _) in enumerate(rows) if rs == s]
        delta = np.zeros(lk.size)
        if profile in ("ascending", "descending") and lk.size > 1:
            delta = 0.3 * np.arange(lk.size) / (lk.size - 1)
            if profile == "descending":
                delta = delta[::-1]
        for h in range(H):
            if quiet.size and mine:
                sc = scale * (Q[mine, h].astype(np.float64) @ K[s, quiet, h].astype(np.float64).T)
                top = sc.max()
                A = top + np.log(2.0) * rng.uniform(24.1, 24.6) if profile == "peaked" else (top + np.log(np.exp(sc - top).sum(axis=1)).max()) + np.log(4.0 / lk.size)
            else:
                A = 1.0
            K[s, lk, h, 63] = np.float16(A * inv)
            K[s, lk, h, 62] = f16(16.0 * delta * inv)
    groups = {}
    for r, (s, n) in enumerate(rows):
        groups.setdefault((s, n), []).append(r)
    for (s, n), rs in groups.items():
        vis = loud[s][loud[s] < n]
        for h in range(H):
            _, _, p = reference(Q[rs, h], K[s, :n, h], V[s, :n, h], scale)
            assert p[:, vis].min() >= MIN_MASS, "slot %d, %d keys, head %d: a loud key holds %.4f of the softmax mass" % (s, n, h, p[:, vis].min())
    return Q.reshape(R, H * 64), K.reshape(S, n_store, H * 64), V.reshape(S, n_store, H * 64), loud


# ---------------------------------------------------------------------------------------------------------------- the cases
KEY_COUNTS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 750, 1499, 1500]
QUERY_COUNTS = [1, 31, 32, 33, 127, 128, 129, 240]
SELF_POS = [0, 1, 63, 64, 65, 127, 128, 129, 447]
N_CTX, N_TEXT_CTX = 1500, 448


class Case:
    """One launch: `form` and the launcher's arguments, the rows' (slot, key count) as the reference sees them, and which output rows must keep the sentinel."""
    def __init__(self, name, form, H, n_ctx, profile, slots, rows, **kw):
        self.name, self.form, self.H, self.n_ctx, self.profile, self.slots, self.rows = name, form, H, n_ctx, profile, slots, rows
        self.scale = 0.125 if form == "encoder" else 1.0
        self.block = 64 if form in ("encoder", "prefill", "self") else 32
        self.vark = kw.pop("vark", False)
        self.kw = kw                                                      # launcher arguments beyond the operands
        self.live = kw.pop("live", [True] * len(rows))                    # rows the kernel writes
        self.out_row = kw.pop("out_row", list(range(len(rows))))          # output row of each query row
        self.n_out = kw.pop("n_out", len(rows))
        self.seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))

    def operands(self):
        return make_operands(self.seed, self.profile, self.H, self.scale, self.slots, self.rows)

    def fill_from(self):
        return [max(c) for _, c in self.slots]

    def pads(self):
        """NaN in K always; in V where the kernel promises to replace it (the per-clip key counts, the self-attention cache), 1000.0 where it relies on p = 0"""
        return 0x7E00, (0x7E00 if self.vark or self.form == "self" else 0x63D0)


def _decode_cases():
    out = []
    groups = [[1, 33, 96, 100, 750], [31, 64, 97, 17, 1499], [32, 65, 127, 500, 1500], [63, 128, 129, 40, 1]]      # the fourth of each is the inactive row's
    i = 0
    for H in (4, 6):
        for g in groups:
            prof = PROFILES[i % 6]; i += 1
            act = [1, 1, 1, 0, 1]; seq = [0, 1, 2, 3, 1]                    # row 4 attends over row 1's sequence, with its own key count
            counts = [[g[0]], [g[1], g[4]], [g[2]], [g[3]]]
            out.append(Case("cross_H%d_k%d_%s" % (H, g[0], prof), "cross", H, N_CTX, prof, [(N_CTX, c) for c in counts], [(seq[r], g[r]) for r in range(5)], vark=True,
                            active=act, seq=seq, count=g, live=[bool(a) for a in act]))
        for n in (97, 1500) if H == 4 else (96, 750):                      # one row, no flags, no sequence map
            prof = PROFILES[i % 6]; i += 1
            out.append(Case("cross_H%d_one_k%d_%s" % (H, n, prof), "cross", H, N_CTX, prof, [(N_CTX, [n])], [(0, n)], vark=True, count=[n]))
    for H, n_ctx in ((4, 96), (6, 100), (4, 1500), (6, 1500)):             # the full-length instantiations: nkeys null
        prof = PROFILES[i % 6]; i += 1
        act = [1, 0, 1, 1, 1]; seq = [0, 1, 2, 3, 2]
        out.append(Case("cross_full_H%d_n%d_%s" % (H, n_ctx, prof), "cross", H, n_ctx, prof, [(n_ctx, [n_ctx])] * 4, [(s, n_ctx) for s in seq], active=act, seq=seq,
                        live=[bool(a) for a in act]))
    out.append(Case("cross_full_H6_one_n1500_ascending", "cross", 6, 1500, "ascending", [(1500, [1500])], [(0, 1500)]))
    return out


def _self_cases():
    out = []
    groups = [(4, [0, 64, 127, 5, 447]), (6, [1, 63, 128, 300, 129]), (4, [65, 447, 0, 9, 129]), (6, [447, 127, 64, 2, 65]), (4, [128, 1, 63, 70, 0])]
    for i, (H, g) in enumerate(groups):
        prof = PROFILES[(i + 2) % 6]
        act = [1, 1, 1, 0, 1]; seq = [0, 1, 2, 3, 1]
        counts = [[g[0] + 1], [g[1] + 1, g[4] + 1], [g[2] + 1], [g[3] + 1]]
        out.append(Case("self_H%d_p%d_%s" % (H, g[0], prof), "self", H, N_TEXT_CTX, prof, [(N_TEXT_CTX, c) for c in counts], [(seq[r], g[r] + 1) for r in range(5)],
                        active=act, seq=seq, count=g, live=[bool(a) for a in act]))
    out.append(Case("self_H6_one_p447_ascending", "self", 6, N_TEXT_CTX, "ascending", [(N_TEXT_CTX, [448])], [(0, 448)], count=[447]))
    out.append(Case("self_H4_one_p0_random", "self", 4, N_TEXT_CTX, "random", [(N_TEXT_CTX, [1])], [(0, 1)], count=[0]))
    return out


def _encoder_case(name, H, n_ctx, prof, slot_k, out_rows, vark):
    per = out_rows if (vark and out_rows) else n_ctx
    rows, out_row = [], []
    for s, n in enumerate(slot_k):
        rows += [(s, n)] * n; out_row += [s * per + i for i in range(n)]
    return Case(name, "encoder", H, n_ctx, prof, [(n_ctx, [n]) for n in slot_k], rows, vark=vark, out_row=out_row, n_out=len(slot_k) * per,
                **({"slot_k": list(slot_k), "out_rows": out_rows} if vark else {}))


def _encoder_cases():
    out = []
    sets = [(4, [1, 31, 32, 33, 63, 64, 65, 96], 256), (6, [97, 127, 128, 129, 240], 256), (6, [17, 100, 256], 256), (4, [750, 1500], 0), (6, [1499], 0), (4, [129, 1, 240], 0)]
    for i, (H, sk, orows) in enumerate(sets):
        prof = PROFILES[(i + 1) % 6]
        out.append(_encoder_case("enc_H%d_k%d_%s" % (H, sk[0], prof), H, N_CTX, prof, sk, orows, True))
    for i, (H, n_ctx, B) in enumerate(((4, 96, 2), (6, 100, 2), (6, 1500, 1), (4, 1500, 1))):
        prof = PROFILES[(i + 3) % 6]
        out.append(_encoder_case("enc_full_H%d_n%d_%s" % (H, n_ctx, prof), H, n_ctx, prof, [n_ctx] * B, 0, False))
    return out


def _prefill_cases():
    out = []
    sets = [(4, (1, 129, 31), (33, 1499)), (6, (32, 240, 33), (750, 65)), (4, (127, 128, 240), (1, 1500)), (6, (129, 31, 1), (96, 97)), (4, (33, 32, 128), (63, 64)),
            (6, (240, 127, 129), (31, 32)), (4, (31, 33, 1), (127, 128)), (6, (128, 1, 32), (129, 100))]
    full = [(4, (33, 129, 1), 96), (6, (240, 31, 128), 100), (6, (127, 32, 129), 1500), (4, (1, 240, 33), 1500)]
    for i, (H, nq, sk) in enumerate(sets + full):
        prof = PROFILES[(i + 4) % 6]
        vark = i < len(sets)
        n_ctx = N_CTX if vark else sk
        keys = sk if vark else (n_ctx, n_ctx)
        slot = [0, 0, 1]                                                  # two sequences share window slot 0, the third has slot 1
        row0 = [3, 3 + nq[0] + 2, 3 + nq[0] + 2 + nq[1] + 5]              # gaps between the sequences' rows: they keep the sentinel
        total = row0[2] + nq[2] + 4
        rows, out_row = [], []
        for j in range(3):
            rows += [(slot[j], keys[slot[j]])] * nq[j]; out_row += list(range(row0[j], row0[j] + nq[j]))
        out.append(Case("xp%s_H%d_q%d_%s" % ("" if vark else "_full", H, nq[0], prof), "prefill", H, n_ctx, prof, [(n_ctx, [keys[0]]), (n_ctx, [keys[1]])], rows, vark=vark,
                        out_row=out_row, n_out=total, row0=row0, nq=list(nq), slot=slot, **({"slot_k": list(sk)} if vark else {})))
    return out


def cases():
    return _decode_cases() + _self_cases() + _encoder_cases() + _prefill_cases()


def check_rows(case, Q, K, V, got, pick=None):
    """got [n_out][H*64] against the reference under the bound.  -> the largest error / bound over the rows the kernel writes (asserts nothing)"""
    H = case.H; worst = 0.0
    groups = {}
    for r, (s, n) in enumerate(case.rows):
        if case.live[r]:
            groups.setdefault((s, n), []).append(r)
    for (s, n), rs in groups.items():
        for h in range(H):
            sl = slice(h * 64, h * 64 + 64)
            ref, bound, _ = reference(Q[rs, sl], K[s, :n, sl], V[s, :n, sl], case.scale)
            g = got[[case.out_row[r] for r in rs], sl].astype(np.float64)
            with np.errstate(invalid="ignore"):
                ratio = np.abs(g - ref) / bound
            ratio[~np.isfinite(g)] = np.inf
            worst = max(worst, float(ratio.max()))
    return worst
