"""The sampler's temperature draws and greedy near-ties: seeded cases, generator states and an INDEPENDENT reference (numpy) of the generator and of the draw.
Test infrastructure only (tests/test_cpu_sampler_draw.py, tests/test_gpu_sampler_draw.py).  Nothing here is stored: every case is regenerated from its seed.

Generator.  std::mt19937(seed) is init_genrand(seed), which is what numpy.random.RandomState(seed) holds; the reference for its outputs is numpy.random.MT19937 with the state
set, random_raw(2) — numpy's C, independent of oracle/skw_oracle.c and of the kernel.  u = std::generate_canonical<double, 53>: (lo + hi * 2^32) / 2^64 in doubles, 1.0 clamped
to nextafter(1, 0) (libstdc++).  untemper() inverts the output tempering, so a state can be made to emit two chosen words next — as long as both come before the twist
(index <= 622).

Draw.  draw_ref(): libstdc++'s discrete_distribution on f32 weights — the sequential f64 sum (np.cumsum, never np.sum: pairwise), q = p / sum, the sequential partial sums with
the last forced to 1.0, lower_bound.  tests/test_cpu_oracle.py pins it against libstdc++ itself on weight_family()'s rows.

Rows.  A row = a decoder history (logit_rules_lib.make_case's kinds) + raw logits + a temperature + a generator state.  Sampled rows are designed in the divided space
(design * T is the raw row), so a family keeps its shape at every temperature; greedy rows (temperature 0) carry the near-ties.  Rows whose u is aimed at a place of the
row's own cumulative distribution take the oracle's probs for it (aim()): the aim is part of the input, the expected index is always the reference's."""
from fractions import Fraction

import numpy as np

import logit_rules_lib as lr

F32 = np.float32
TEMPS = [F32(0.2), F32(0.4), F32(0.2) + F32(0.2) + F32(0.2), F32(0.8), F32(1.0), F32(0.05), F32(4.0)]      # the third: the ladder's accumulated 0.6
STATE_IDX = [0, 1, 622, 623, 624]      # 623: the draw's second word comes after the twist; 624: both do
CRAFTED_U = {                          # name -> (low word, high word)
    "zero": (0, 0),
    "2^-64": (1, 0),
    "half": (0, 0x80000000),
    "after_half": (0x800, 0x80000000),             # 2^63 + 2^11: the next double after 0.5, times 2^64
    "1-2^-53": (0xFFFFF800, 0xFFFFFFFF),           # 2^64 - 2^11
    "ones": (0xFFFFFFFF, 0xFFFFFFFF),              # 2^64 - 1 rounds to 2^64: u == 1.0, clamped
}
GAPS = {"0": None, "1ulp": None, "5e-5": F32(5e-5), "below_1e-4": np.nextafter(F32(1e-4), F32(0)), "1e-4": F32(1e-4), "above_1e-4": np.nextafter(F32(1e-4), F32(1)),
        "2e-4": F32(2e-4)}
PLACEMENTS = ["same_thread", "same_wave", "other_wave", "ends", "text_stripes", "text_vs_ts", "two_ts"]


# ---------------------------------------------------------------- generator
def mt_state(seed, idx):
    """std::mt19937(seed) as uint32[625] (mt + index), the index moved to idx"""
    key = np.random.RandomState(seed).get_state()[1]
    st = np.empty(625, np.uint32); st[:624] = key; st[624] = idx
    return st


def untemper(y):
    y = int(y) & 0xFFFFFFFF
    y ^= y >> 18
    y ^= (y << 15) & 0xEFC60000
    x = y
    for _ in range(5):
        x = y ^ ((x << 7) & 0x9D2C5680)
    y = x & 0xFFFFFFFF
    x = y
    for _ in range(3):
        x = y ^ (x >> 11)
    return x & 0xFFFFFFFF


def crafted_state(seed, idx, lo, hi):
    """a state whose next two outputs are lo, hi (both words before the twist)"""
    assert 0 <= idx <= 622
    st = mt_state(seed, idx)
    st[idx] = untemper(lo); st[idx + 1] = untemper(hi)
    return st


def canonical(lo, hi):
    cs = 0.0 + float(int(lo)) * 1.0
    cs = cs + float(int(hi)) * 4294967296.0
    u = cs / 18446744073709551616.0
    return float(np.nextafter(1.0, 0.0)) if u >= 1.0 else u


def generator_ref(state):
    """-> (u, state after the draw) by numpy.random.MT19937"""
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": np.array(state[:624], dtype=np.uint32), "pos": int(state[624])}}
    lo, hi = (int(x) for x in bg.random_raw(2))
    after = np.empty(625, np.uint32); after[:624] = bg.state["state"]["key"]; after[624] = bg.state["state"]["pos"]
    return canonical(lo, hi), after


def words_for(t):
    """the two words whose canonical value is the largest one <= the double t (t in [0, 1))"""
    n = int(Fraction(float(t)) * (1 << 64))
    n = min(max(n, 0), (1 << 64) - 1)
    while canonical(n & 0xFFFFFFFF, n >> 32) > t:      # (the sum of the two words rounds to nearest: step down past a round-up)
        n -= 1 << max(0, n.bit_length() - 53)
    return n & 0xFFFFFFFF, n >> 32


# ---------------------------------------------------------------- draw
def draw_ref(p32, u):
    p64 = np.asarray(p32, dtype=np.float32).astype(np.float64)
    s = np.cumsum(p64)[-1]
    q = p64 / s
    cp = np.cumsum(q); cp[-1] = 1.0
    return int(np.searchsorted(cp, u, "left")), s, cp


def weight_family(name, n, rng):
    """f32 weights as the sampler's probs row would hold them (exp of a design row minus its maximum, rounded to f32; zeros where a token is suppressed)"""
    if name == "flat":
        return np.ones(n, F32)
    if name.startswith("spike@"):
        z = rng.standard_normal(n)
        lg = z - z.max() - 40.0; lg[min(int(name[6:]), n - 1)] = 0.0      # 40 above the noise's largest: e^-40 = 4.2e-18 < 2^-53, no noise term after the spike can move the sum
        return np.exp(lg).astype(F32)
    if name.startswith("spike2@"):      # the same with an equal spike on the last element: u = 0.75 makes the second chain cross everything between them
        z = rng.standard_normal(n)
        lg = z - z.max() - 40.0; lg[min(int(name[7:]), n - 1)] = 0.0; lg[n - 1] = 0.0
        return np.exp(lg).astype(F32)
    if name == "half_ulp_tie":      # sum = 1 + 2^-52 (odd) after two elements, then blocks of exactly half an ulp of it: every addition is a tie that round-to-even moves UP — the
        w = np.full(n, 2.0 ** -53, F32); w[0] = 1.0      # skip bound is strict (<), a block AT the bound still moves the sum
        if n > 1:
            w[1] = 2.0 ** -52
        w[2:min(n, 64)] = 0.0
        return w
    if name == "staircase":
        return np.exp(-80.0 * np.arange(n) / max(n, 2)).astype(F32)
    if name == "two_spikes":
        w = np.zeros(n, F32); w[[max(n // 2 - 1, 0), n // 2]] = 0.5 if n > 1 else 1.0
        return w
    if name == "subnormal":
        lg = rng.standard_normal(n) - 5.0
        k = rng.random(n) < 0.5; lg[k] = -rng.uniform(88.0, 103.0, int(k.sum())); lg[int(rng.integers(0, n))] = 0.0
        return np.exp(lg).astype(F32)
    raise KeyError(name)


WEIGHT_FAMILIES = ["flat", "spike@0", "spike@63", "spike@64", "spike@4095", "spike@4096", "spike@30000", "spike@999999", "spike2@0", "spike2@64", "spike2@4096", "staircase", "two_spikes", "subnormal", "half_ulp_tie"]
LOW_TAIL_AT = [63, 64, 4095, 4096, 8191, 8192]


def family_us(name, w):
    """the u values a weight row is drawn at: {label: u}"""
    n = len(w)
    _, _, cp = draw_ref(w, 0.0)
    us = {"zero": 0.0, "2^-64": 2.0 ** -64, "half": 0.5, "after_half": 0.5 + 2.0 ** -53, "1-2^-53": 1.0 - 2.0 ** -53}
    for k in range(1, 8):
        us["spread%d" % k] = k / 8.0 + 1e-3
    if name.startswith("spike2@"):
        us["between"] = 0.75
    if name.startswith("spike@"):
        s = min(int(name[6:]), n - 1)
        for k in LOW_TAIL_AT:
            if k < s:
                us["low@%d" % k] = float(cp[k]); us["low@%d-" % k] = float(np.nextafter(cp[k], 0.0)); us["low@%d+" % k] = float(np.nextafter(cp[k], 1.0))
        us["spike"] = float(cp[s]) - 0.25
        if s < n - 1:
            us["after"] = float(cp[s]) + (1.0 - float(cp[s])) * 0.5; us["after_end"] = 1.0 - 2.0 ** -53
    return us


# ---------------------------------------------------------------- rows
def _hist(sp, NV, kind, seed):
    return lr.make_case(np.random.default_rng(seed), sp, NV, kind)[0]


def _row(name, family, hist, design, T, **kw):
    T = F32(T)
    raw = np.asarray(design, dtype=F32) * T if T > 0 else np.asarray(design, dtype=F32)
    c = dict(name=name, family=family, hist=list(hist), raw=raw.astype(F32), temperature=T, state=None, aim=None, u_name=None, gap=None, placement=None, higher_wins=None)
    c.update(kw)
    return c


def _bg(rng, NV, beg, text=-12.0, ts=-30.0):
    d = rng.standard_normal(NV).astype(F32) + F32(text)
    d[beg:] += F32(ts - text)
    return d


def placement_ids(pl, NV, beg):
    """(a, b, c): the two tied / near-tied ids in ascending order and a third for the triple tie; the history kind that leaves them admissible"""
    return {"same_thread": ((1000, 1512, 2024), "after_pair"),                  # 512 apart: one thread's slots 1, 2, 3
            "same_wave": ((2000, 2001, 2010), "after_pair"),                    # one stripe, lanes of wave 7
            "other_wave": ((2000, 2100, 2300), "after_pair"),                   # thread 464 (wave 7) / 52 (wave 0) / 252 (wave 3)
            "ends": ((0, NV - 1, NV - 2), "text"),
            "text_stripes": ((5000, 40000, 48000), "after_pair"),               # stripes 9, 78, 93
            "text_vs_ts": ((49000, beg + 1300, beg + 1301), "text"),            # below 49 152 = 96 * 512: a text stripe's entry against an index-ruled one
            "two_ts": ((NV - 300, NV - 5, NV - 3), "text")}[pl]


def greedy_cases(sp, NV, gaps=None, placements=None):
    beg = sp["beg"]; out = []
    for gi, gap in enumerate(gaps or list(GAPS)):
        for pi, pl in enumerate(placements or PLACEMENTS):
            ids, kind = placement_ids(pl, NV, beg)
            for higher_wins in (False, True):
                seed = 7000 + 100 * gi + 10 * pi + int(higher_wins)
                rng = np.random.default_rng(seed)
                d = _bg(rng, NV, beg)
                if gap == "1ulp":
                    lo_v, hi_v = F32(0.015625), np.nextafter(F32(0.015625), F32(1.0))      # one ulp of the logit (1.9e-9) is far below one of the probability: they round together
                elif gap == "0":
                    lo_v = hi_v = F32(8.0)
                else:
                    lo_v, hi_v = F32(0.0), GAPS[gap]      # against 0 the difference IS the gap, exactly
                a, b = (ids[0], ids[1])
                d[b if higher_wins else a] = hi_v; d[a if higher_wins else b] = lo_v
                out.append(_row("tie/%s/%s/%d" % (gap, pl, higher_wins), "near_tie", _hist(sp, NV, kind, 400 + pi), d, 0.0, gap=gap, placement=pl, higher_wins=higher_wins))
            if gap == "0":
                rng = np.random.default_rng(7900 + pi)
                d = _bg(rng, NV, beg); d[list(ids)] = F32(8.0)
                out.append(_row("tie3/%s" % pl, "triple_tie", _hist(sp, NV, kind, 400 + pi), d, 0.0, gap="0", placement=pl))
    return out


def _temps(k):
    return TEMPS[k % len(TEMPS)]


def sampled_cases(om, po, reduced=False):
    """the draw rows, each with its generator state; rows with an aim still need aim()"""
    sp = lr.special_ids(om); NV = om.hp.n_vocab; beg = sp["beg"]
    out = []; n = [0]

    def add(name, family, hist, design, T=None, u=None, aim=None, idx=None):
        k = n[0]; n[0] += 1
        T = _temps(k) if T is None else T
        c = _row(name, family, hist, design, T, aim=aim, u_name=u)
        if u is not None:
            c["state"] = crafted_state(1000 + k, [0, 1, 622][k % 3] if idx is None else idx, *CRAFTED_U[u])
        elif aim is None:
            c["state"] = mt_state(2000 + k, STATE_IDX[k % 5] if idx is None else idx)
        c["state_seed"] = 3000 + k; c["state_idx"] = [0, 1, 622][k % 3]
        out.append(c)

    h_pair = _hist(sp, NV, "after_pair", 11); h_text = _hist(sp, NV, "text", 12)
    # flat: every admissible logit equal — nothing is skippable
    flat = np.zeros(NV, F32)
    for u in CRAFTED_U:
        add("flat/" + u, "flat", h_pair, flat, u=u)
    for k in range(1 if reduced else 5):
        add("flat/natural%d" % k, "flat", h_pair, flat)
    # flat over the timestamps alone (the mass rule removes the text): u just below 1 — the sequential partial sums of n equal terms end a little below or above 1, and the
    # definition's cp_{n-1} = 1.0 decides; the history sets n
    for k in range(2 if reduced else 6):
        add("flat_ts/%d" % k, "flat_ts", _hist(sp, NV, "text", 12 + k), flat, u="1-2^-53" if k % 2 == 0 else "ones")
    # spike: one logit 40 above the noise's largest
    for s in ([64, 4096, NV - 1] if reduced else [0, 63, 64, 4095, 4096, 30000, NV - 1]):
        rng = np.random.default_rng(5000 + s)
        z = rng.standard_normal(NV)
        d = (z - z.max() - 40.0).astype(F32); d[s] = F32(0.0)
        h = h_text if s >= beg else h_pair
        for k in LOW_TAIL_AT:
            if k < s and not (reduced and k not in (63, 4096)):
                add("spike@%d/low@%d" % (s, k), "spike", h, d, T=[TEMPS[4], TEMPS[3], TEMPS[2]][k % 3], aim=("cp", k))
        add("spike@%d/spike" % s, "spike", h, d, u="half")
        if s < NV - 1:
            add("spike@%d/after" % s, "spike", h, d, T=TEMPS[4], aim=("after", s))
            add("spike@%d/last" % s, "spike", h, d, u="1-2^-53")
    # staircase
    stair = (-80.0 * np.arange(NV) / NV).astype(F32)
    for k in range(1 if reduced else 4):
        add("staircase/%d" % k, "staircase", h_pair, stair)
    if not reduced:
        add("staircase/ones", "staircase", h_pair, stair, u="ones"); add("staircase/zero", "staircase", h_pair, stair, u="zero")
    # two equal spikes, everything else -inf in the raw row: q is exactly 0.5 twice
    for a, b, h in ([(4095, 4096, h_pair)] if reduced else [(4095, 4096, h_pair), (63, 64, h_pair), (NV - 2, NV - 1, h_text)]):
        d = np.full(NV, -np.inf, F32); d[[a, b]] = F32(1.0)
        for u in ("half", "after_half"):
            add("two_spikes@%d/%s" % (a, u), "two_spikes", h, d, u=u)
    if not reduced:
        # f32 probabilities below the normal range: logits 88 .. 103 below the maximum, mixed with normal ones
        for k in range(3):
            rng = np.random.default_rng(5100 + k)
            d = (rng.standard_normal(NV) - 5.0).astype(F32); m = rng.random(NV) < 0.5
            d[m] = -rng.uniform(88.0, 103.0, int(m.sum())).astype(F32); d[int(rng.integers(0, beg))] = F32(0.0)
            add("subnormal/%d" % k, "subnormal", h_pair, d, T=TEMPS[4] if k == 0 else None)
        add("subnormal/zero", "subnormal", h_pair, d, u="zero"); add("subnormal/2^-64", "subnormal", h_pair, d, u="2^-64")
        # the rules under temperature: make_case's own rows (N(0, 3) plus peaks on rule boundaries), divided by every temperature
        for ki, kind in enumerate(("initial", "after_lone_ts", "after_pair")):
            for ti, T in enumerate(TEMPS):
                h, raw = lr.make_case(np.random.default_rng(6000 + 10 * ki + ti), sp, NV, kind)
                c = _row("rules/%s/T%d" % (kind, ti), "rules", h, raw, 0.0); c["temperature"] = T      # (make_case's row is the RAW one)
                k = n[0]; n[0] += 1
                c["state"] = mt_state(2000 + k, STATE_IDX[k % 5]); out.append(c)
        # the timestamp mass within a few ulps of max_text after the division (D-d): one text logit against one timestamp
        for du in (-2, -1, 0, 1, 2):
            rng = np.random.default_rng(6100 + du)
            d = _bg(rng, NV, beg, ts=-40.0)
            x = F32(3.0); t = x
            for _ in range(abs(du)):
                t = np.nextafter(t, F32(9.0) if du > 0 else F32(-9.0))
            d[49000] = x; d[beg + 1300] = t
            c = _row("mass/%+d" % du, "mass_edge", h_text, d, 0.0); c["temperature"] = TEMPS[2]
            k = n[0]; n[0] += 1
            c["state"] = mt_state(2000 + k, STATE_IDX[k % 5]); out.append(c)
        # every family at every temperature, each on a generator of its own seed (the index cycles through STATE_IDX): the division ahead of the filters and the natural u
        designs = [("flat", "flat", h_pair, flat), ("staircase", "staircase", h_pair, stair), ("subnormal", "subnormal", h_pair, d)]
        for s in (0, 63, 64, 4095, 4096, 30000):
            z = np.random.default_rng(5200 + s).standard_normal(NV)
            ds = (z - z.max() - 8.0).astype(F32); ds[s] = F32(0.0)      # a spike the tail is still drawn from: 8 above the noise's largest, about 0.7 of the mass
            designs.append(("spike8@%d" % s, "spike", h_pair, ds))
        z = np.random.default_rng(5300).standard_normal(NV)
        designs.append(("noise_text", "rules", h_text, (z * 2.0).astype(F32)))
        designs.append(("noise_lone", "rules", _hist(sp, NV, "after_lone_ts", 13), (z * 2.0).astype(F32)))
        for name, fam, h, dd in designs:
            for ti, T in enumerate(TEMPS):
                add("%s/T%d" % (name, ti), fam, h, dd, T=T)
    # a single admissible token
    d = np.full(NV, -np.inf, F32); d[777] = F32(2.5)
    add("single/sampled", "single", h_pair, d)
    return out


def single_greedy(sp, NV):
    d = np.full(NV, -np.inf, F32); d[777] = F32(2.5)
    return _row("single/greedy", "single", _hist(sp, NV, "after_pair", 11), d, 0.0)


def oracle_canonical(state):
    """-> (u, state after) by the oracle's restatement (skwo_debug_mt_canonical)"""
    import ctypes as C
    from oracle_lib import lib
    L = lib(); L.skwo_debug_mt_canonical.restype = C.c_double; L.skwo_debug_mt_canonical.argtypes = [C.c_void_p]
    st = np.array(state, dtype=np.uint32)
    return L.skwo_debug_mt_canonical(st.ctypes.data), st


def last_element_decides(p32, u):
    """True when only the definition's cp_{n-1} = 1.0 makes the last element the hit (the running sum itself ends below u)"""
    p64 = np.asarray(p32, dtype=F32).astype(np.float64)
    return bool(np.cumsum(p64 / np.cumsum(p64)[-1])[-1] < u)


def oracle_sample(om, po, case, state=None):
    """skwo_debug_sample_logits on one row -> dict(filtered, logprobs, probs, tok, no_speech_prob, state)"""
    import ctypes as C
    from oracle_lib import lib, Params, Token
    L = lib()
    L.skwo_debug_sample_logits.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(Token), C.POINTER(C.c_float)]
    NV = om.hp.n_vocab
    h = np.ascontiguousarray(case["hist"], dtype=np.int32); raw = np.ascontiguousarray(case["raw"], dtype=F32)
    st = np.array(case["state"] if state is None else state, dtype=np.uint32)
    filt = np.empty(NV, F32); lp = np.empty(NV, F32); probs = np.empty(NV, F32); tk = Token(); nsp = C.c_float()
    rc = L.skwo_debug_sample_logits(om.h, C.byref(po), h.ctypes.data, h.size, raw.ctypes.data, C.c_float(float(case["temperature"])), st.ctypes.data, filt.ctypes.data, lp.ctypes.data,
                                    probs.ctypes.data, C.byref(tk), C.byref(nsp))
    if rc != 0:
        raise RuntimeError("skwo_debug_sample_logits rc=%d (%s)" % (rc, case["name"]))
    return dict(filtered=filt, logprobs=lp, probs=probs, tok=dict(id=tk.id, tid=tk.tid, p=tk.p, plog=tk.plog, pt=tk.pt, ptsum=tk.ptsum, margin=tk.margin),
                no_speech_prob=nsp.value, state=st)


def aim(om, po, case):
    """Gives a row with an aim its generator state: u from the cumulative distribution of the oracle's own probs for the row.  ("cp", k): the largest canonical value
    <= cp[k] — a hit in the low tail, where cp is tiny; ("after", s): half way through the mass that follows index s."""
    if case["aim"] is None or case["state"] is not None:
        return case
    probs = oracle_sample(om, po, case, state=mt_state(0, 0))["probs"]
    _, _, cp = draw_ref(probs, 0.0)
    kind, k = case["aim"]
    t = float(cp[k]) if kind == "cp" else float(cp[k]) + 0.5 * (1.0 - float(cp[k]))
    case["state"] = crafted_state(case["state_seed"], case["state_idx"], *words_for(min(t, 1.0 - 2.0 ** -53)))
    return case


def all_cases(om, po, reduced=False):
    """-> (greedy rows, sampled rows), every sampled row with its generator state; greedy rows get a state too (it must come back untouched)"""
    sp = lr.special_ids(om); NV = om.hp.n_vocab
    if reduced:
        g = greedy_cases(sp, NV, gaps=["1ulp", "2e-4"]) + [c for c in greedy_cases(sp, NV, gaps=["0"], placements=["text_vs_ts", "ends"])]
    else:
        g = greedy_cases(sp, NV)
    g.append(single_greedy(sp, NV))
    for i, c in enumerate(g):
        c["state"] = mt_state(9000 + i, STATE_IDX[i % 5])
    s = [aim(om, po, c) for c in sampled_cases(om, po, reduced)]
    return g, s


def launches(greedy, sampled, rows=64):
    """the launches of the GPU test: all-greedy ones, then mixed ones — every fourth row of a sampled launch is a greedy row again (the mixed-batch ladder's launch)"""
    out = [greedy[i:i + rows] for i in range(0, len(greedy), rows)]
    mixed = []; gi = 0
    for i, c in enumerate(sampled):
        mixed.append(c)
        if i % 3 == 2:
            mixed.append(greedy[gi % len(greedy)]); gi += 7
    out += [mixed[i:i + rows] for i in range(0, len(mixed), rows)]
    return out
