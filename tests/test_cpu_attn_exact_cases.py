"""CPU tier: the numpy restatement tests/test_gpu_attn_exact.py holds the exact-precision attention kernels to IS the contract, and its cases have teeth (tests/attn_exact_ref_lib.py;
no GPU).

  * the numpy skw_expf equals the oracle's on a seeded sweep of non-positive arguments with the edges in it;
  * fed the oracle's own l0.q / l0.k / l0.v, the restatement reproduces the oracle's row maxima, reciprocals, f32 attention output and its stored form, bit for bit;
  * no row of any case has an expectation that depends on the order of the f64 row sum (so the GPU test skips no row);
  * the single-pass encoder kernel's exponential without the -86 clamp gives the same probabilities and reciprocal on every case — and cases exist in which it is evaluated
    between -104 and -86, where it is NOT zero; scaling q by 2^-3 in f32 before the chain (what that kernel does) gives the same score bits;
  * each named wrong kernel, applied to the restatement, changes output bits: a key count of n - 1 in every (slot, key count) of every case, in the f32 and in the f16 output form,
    and n + 1 in every (slot, key count, head); the others counted per case and asserted per kernel and per-slot-count mode (a one-key slot cannot show an order)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_exact_ref_lib as ax  # noqa: E402
import oracle_lib  # noqa: E402

CASES = ax.cases()
SUB = 8                                   # query rows per (group, head) the wrong kernels are evaluated on: the first, the last and seeded ones between
_HITS = {}                                # (wrong kernel, kernel, vark) -> [cases in which it changed a bit, cases it applies to]
_UNCLAMPED = {"below_86": 0, "nonzero": 0}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_numpy_expf_equals_the_oracles(oracle_tiny):
    rng = np.random.default_rng(86)
    f = np.float32
    edges = [f(0), f(-0.0), f(-86), np.nextafter(f(-86), f(0)), np.nextafter(f(-86), f(-100)), f(-104), f(-1e4), f(-87.3), f(-1e-30), f(-88.72283)]
    x = np.concatenate([np.array(edges, f), -rng.uniform(0, 110, 200000).astype(f), -np.exp(rng.uniform(-40, 5, 50000)).astype(f)])
    got, want = ax.skw_expf(x), oracle_tiny.math(0, x)
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d differ" % ((_bits(got) != _bits(want)).sum(), x.size)
    assert got[0] == 1 and got[2] > 0 and got[4] == 0 and got[5] == 0 and got[6] == 0
    un = ax.expf_unclamped(x)
    hi = x >= f(-86)
    assert np.array_equal(_bits(un[hi]), _bits(got[hi])) and (un[~hi] < 2.0 ** -124).all() and (un[(x < -86) & (x > -103)] > 0).all()


def test_restatement_reproduces_the_oracles_attention_taps(oracle_tiny):
    """layer 0 of the tiny model's encoder on a seeded clip: 2 heads, the first and the last 32 query rows against all 1500 keys"""
    from streamkit_amd import synth
    hp = oracle_tiny.hp
    n_ctx, d, nh = hp.n_audio_ctx, hp.n_audio_state, hp.n_audio_head
    mel, _ = oracle_tiny.log_mel(synth.clip(5, 16000 * 12))
    oracle_lib.debug_enable(True)
    try:
        oracle_tiny.encode(mel, cross=False)
        tap = {k: oracle_lib.debug_get("l0." + k).copy() for k in ("q", "k", "v", "rmax", "rinv", "att32", "att")}
    finally:
        oracle_lib.debug_enable(False)
    q, k, v, a32, att = (tap[n].reshape(n_ctx, d) for n in ("q", "k", "v", "att32", "att"))
    rmax, rinv = tap["rmax"].reshape(nh, n_ctx), tap["rinv"].reshape(nh, n_ctx)
    for a in (q, k, v):
        assert np.array_equal(a.astype(np.float16).astype(np.float32), a)          # f16-valued, as the contract takes them
    rows = np.r_[0:32, n_ctx - 32:n_ctx]
    for h in (0, nh - 1):
        sl = slice(h * 64, h * 64 + 64)
        r = ax.attend(q[rows, sl], k[:, sl], v[:, sl], ax.KQ_SCALE)
        assert np.array_equal(_bits(r["m"]), _bits(rmax[h, rows])), "row maxima, head %d" % h
        assert np.array_equal(_bits(r["inv"]), _bits(rinv[h, rows])), "reciprocals, head %d" % h
        assert np.array_equal(_bits(r["out32"]), _bits(a32[rows, sl])), "f32 output, head %d" % h
        stored = r["out32"] if oracle_tiny.quant else r["out32"].astype(np.float16).astype(np.float32)
        assert np.array_equal(_bits(stored), _bits(att[rows, sl])), "stored output, head %d" % h


def test_the_kernel_level_hook_is_exported_and_bound(built):
    from streamkit_amd import engine
    assert hasattr(engine.lib(), "skw_debug_attn_exact") and set(engine.Context.ATTN_EXACT_FORMS) == {"encoder", "self"}
    assert engine.Context.ATTN_ENC_KERNELS == {0: "k_attn_encoder", 1: "k_attn_encoder_v3"}


def test_the_case_list_reaches_every_edge_the_kernels_have():
    by = {k: [c for c in CASES if c.kernel == k] for k in ("enc3", "encv3", "self", "cross")}
    assert len(set(c.name for c in CASES)) == len(CASES)
    assert sorted(set(c.n_ctx for c in by["enc3"])) == ax.ENC3_N_CTX and set(c.H for c in by["enc3"]) == {1, 3} and all(c.n_slots == 3 for c in by["enc3"])
    for n in ax.ENC3_N_CTX:
        assert {c.vark for c in by["enc3"] if c.n_ctx == n} == {False, True}
    sk = set(g.n for c in by["enc3"] if c.vark for g in c.groups)
    assert {1, 31, 32, 33, 96, 97, 127, 128, 129, 160} <= sk
    assert all(any(g.n % 32 for g in c.groups) for c in by["enc3"] + by["cross"] if c.vark)          # a pad key inside the last walked block, in every per-slot-count case
    assert any(c.vark and min(g.n for g in c.groups) == 1 and max(g.n for g in c.groups) > 128 for c in by["enc3"])
    assert all(any(g.n < c.n_out // c.n_slots for g in c.groups) for c in by["enc3"] if c.vark and c.n_ctx > 1) and any(c.launch["out_rows"] > c.n_ctx for c in by["enc3"])
    assert sorted(c.n_ctx for c in by["encv3"]) == [1489, 1500, 1504] and all(c.H == 2 and c.n_slots == 2 and not c.vark for c in by["encv3"])
    for c in by["encv3"]:
        for g in c.groups:
            ex = np.flatnonzero(g.exact); tiles = (g.n + 63) // 64
            assert set(range(128)) <= set(ex) and set(range((tiles - 2) * 64, g.n)) <= set(ex) and ex.size == 128 + 64 + g.n - (tiles - 2) * 64
    assert set(c.H for c in by["self"]) == {4, 6}
    for c in by["self"]:
        assert set(ax.SELF_POS) <= set(g.n - 1 for g in c.groups) and c.launch["active"].count(0) == 1 and c.launch["seq"][:10] != list(range(10)) and max(g.qrows.size for g in c.groups) == ax.SELF_SHARED and c.n_ctx == 448
    assert sorted(set(c.n_ctx for c in by["cross"])) == ax.CROSS_N_CTX and set(c.H for c in by["cross"]) == {1, 4}
    assert sorted(set((c.n_ctx + 63) // 64 for c in by["cross"])) == [1, 2, 5, 24]
    ck = set(g.n for c in by["cross"] if c.vark for g in c.groups)
    assert {31, 32, 33, 63, 64, 65, 255, 256, 257} <= ck and any((n + 63) // 64 == 6 for n in ck)          # 6 tiles over four waves: parts of 2, the last wave empty


def _sub_rows(rows, seed):
    if rows.size <= SUB:
        return np.arange(rows.size)
    mid = np.random.default_rng(seed).choice(np.arange(1, rows.size - 1), size=SUB - 2, replace=False)
    return np.unique(np.r_[0, mid, rows.size - 1])


def _hit(wrong, case, changed):
    h = _HITS.setdefault((wrong, case.kernel, case.vark), [0, 0])
    h[0] += bool(changed); h[1] += 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_rows_are_order_independent_unclamped_exp_agrees_and_wrong_kernels_show(case):
    ops = case.operands()
    Q, K, V = ops
    recs = ax.expected(case, ops, keep=True)
    changed = {w: False for w in ax.VARIANTS + ("fewer", "more")}
    nan_pad = []
    fewer32 = {id(g): False for g in case.groups}; fewer16 = dict(fewer32)
    for rec in recs:
        g, h = rec["group"], rec["head"]
        assert np.isfinite(rec["out32"]).all()
        assert not ax.order_dependent_rows(rec["e"]), "%s slot %d head %d: rows %s have no bit-exact expectation; give the case another seed (SEED_BUMP)" % (
            case.name, g.slot, h, ax.order_dependent_rows(rec["e"]))
        # the exponential without the clamp: same e where it matters, so the same sum, reciprocal and probabilities — hence the same P.V chain
        arg = rec["s"] - rec["m"][:, None]
        e2 = ax.expf_unclamped(arg)
        tot2 = np.cumsum(e2.astype(np.float64), axis=1)[:, -1]
        inv2 = (1.0 / tot2).astype(np.float32)
        assert np.array_equal(_bits(inv2), _bits(rec["inv"])) and np.array_equal(_bits((e2 * inv2[:, None]).astype(np.float16).astype(np.float32)), _bits(rec["p"]))
        if case.kernel == "encv3":
            _UNCLAMPED["below_86"] += int((arg < -86).sum()); _UNCLAMPED["nonzero"] += int(((arg < -86) & (e2 > 0)).sum())
        sl = slice(h * 64, h * 64 + 64)
        k1, v1 = case.kv(K, V, g.slot, h, g.n + 1)
        # the wrong kernels that change nothing but the softmax: every row's probabilities, then the P.V chain of (a few of) the rows whose probabilities moved
        for w in ("p_f32", "div", "sum_f32"):
            moved = np.flatnonzero((_bits(ax.softmax(rec["s"], w)["p"]) != _bits(rec["p"])).any(axis=1))[:4]
            if moved.size and not changed[w]:
                changed[w] |= not np.array_equal(_bits(ax.pv(ax.softmax(rec["s"][moved], w)["p"], v1[:g.n])), _bits(rec["out32"][moved]))
        # those that change a chain: a few rows, the slot's last (the encoder's quiet one) among them
        sub = _sub_rows(rec["rows"], case.seed + h)
        q = Q[g.qrows[rec["rows"][sub]], sl]
        want = rec["out32"][sub]
        for w in ("q_scaled_f16", "key_desc", "d_desc"):
            if w == "q_scaled_f16" and case.scale is None:
                continue
            changed[w] |= not np.array_equal(_bits(ax.attend(q, k1[:g.n], v1[:g.n], case.scale, variant=w)["out32"]), _bits(want))
        # a miscounted key loop must show in EVERY (slot, key count) — single-query groups and the counts on either side of a block edge are where it would hide.  One key fewer:
        # the scores are the same chains, so the softmax over n - 1 keys of every row, then the P.V chain of (a few of) the rows whose last key carried a probability
        if g.n > 1:
            seen = np.flatnonzero(rec["p"][:, g.n - 1] > 0)[:4]
            if seen.size:
                less = ax.pv(ax.softmax(rec["s"][seen, :g.n - 1])["p"], v1[:g.n - 1])
                fewer32[id(g)] |= not np.array_equal(_bits(less), _bits(rec["out32"][seen]))
                fewer16[id(g)] |= not np.array_equal(ax.stored_f16(less), ax.stored_f16(rec["out32"][seen]))
        # one key more (the poisoned one): every (group, head)
        assert not np.array_equal(_bits(ax.attend(q, k1, v1, case.scale)["out32"]), _bits(want)), "%s slot %d (%d keys) head %d: one key more changes nothing" % (case.name, g.slot, g.n, h)
        changed["more"] = True
        if case.scale is not None:          # 2^-3 in f32 commutes with every rounding of the chain: k_attn_encoder_v3's folded scale is the contract's bits
            assert np.array_equal(_bits(ax.attend(q, k1[:g.n], v1[:g.n], case.scale, variant="q_scaled_f32")["out32"]), _bits(want))
        if case.vark and case.kernel in ("enc3", "cross") and g.n % 32:
            # pad keys of the last walked block masked and MULTIPLIED by p = 0 instead of replaced: their V is NaN, so NaN must come out
            nb = (g.n + 31) & ~31
            kb, vb = case.kv(K, V, g.slot, h, nb)
            nan_pad.append(bool(np.isnan(ax.attend(q, kb, vb, case.scale, n_valid=g.n)["out32"]).all()))
    blind = [(g.slot, g.n) for g in case.groups if g.n > 1 and not (fewer32[id(g)] and fewer16[id(g)])]
    assert not blind, "%s: dropping the last key changes no compared bit (f32 and f16 form) for (slot, keys) %s" % (case.name, blind)
    changed["fewer"] = any(fewer32.values())
    for w, c in changed.items():
        if not (w == "q_scaled_f16" and case.scale is None):
            _hit(w, case, c)
    if case.vark and case.kernel in ("enc3", "cross"):
        assert nan_pad and all(nan_pad), "%s: pad V times p = 0 did not show" % case.name
        _hit("pad_times_zero", case, True)
    print("%s: wrong kernels that changed a bit: %s" % (case.name, " ".join(w for w, c in changed.items() if c) or "none"))


def test_every_wrong_kernel_shows_on_every_kernel_and_the_unclamped_exponential_was_exercised():
    """(after the parametrised test: it tallies what that one saw)"""
    assert _HITS, "nothing was tallied: run the file as a whole"
    print("\nwrong kernel x kernel x per-slot counts: cases with a changed bit / cases")
    for key in sorted(_HITS):
        print("  %-16s %-6s %-6s %d / %d" % (key[0], key[1], "slot_k" if key[2] else "full", _HITS[key][0], _HITS[key][1]))
    assert all(h[0] > 0 for h in _HITS.values()), [k for k, h in _HITS.items() if not h[0]]
    kernels = {(k, v) for (_, k, v) in _HITS}
    for w in ax.VARIANTS + ("fewer", "more"):
        assert {(k, v) for (ww, k, v) in _HITS if ww == w} == {kv for kv in kernels if not (w == "q_scaled_f16" and kv[0] in ("self", "cross"))}, w
    assert {(k, v) for (w, k, v) in _HITS if w == "pad_times_zero"} == {("enc3", True), ("cross", True)}
    print("single-pass encoder cases: %d arguments below -86, %d of them with a non-zero unclamped exponential" % (_UNCLAMPED["below_86"], _UNCLAMPED["nonzero"]))
    assert _UNCLAMPED["below_86"] > 0 and _UNCLAMPED["nonzero"] > 0
