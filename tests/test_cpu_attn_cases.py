"""CPU tier: the operands tests/test_gpu_attn16.py feeds the f16 attention kernels have teeth, and the bound it holds them to is sane (tests/attn_ref_lib.py; no GPU).

For every case of the generator, in every (row, head):
  * the reference over one key fewer differs from the reference by more than 4 bounds somewhere — a kernel that drops the last real key cannot pass;
  * so does the reference over one key more (the last key's K row again, with a zero V row) — a kernel that counts a pad key in the denominator cannot pass;
  * a numpy emulation of the kernels' arithmetic (f32 scores, blockwise running maximum, f16 probabilities, f32 accumulation, f16 output) stays under the bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref_lib as ar  # noqa: E402

CASES = ar.cases()


def test_the_case_list_reaches_every_edge_the_kernels_have():
    by = {f: [c for c in CASES if c.form == f] for f in ("cross", "self", "encoder", "prefill")}
    for f in ("cross", "encoder", "prefill"):
        vark = set(n for c in by[f] if c.vark for _, n in c.rows)
        assert set(ar.KEY_COUNTS) <= vark, (f, sorted(set(ar.KEY_COUNTS) - vark))
        assert set(c.n_ctx for c in by[f] if not c.vark) == {96, 100, 1500}, f
    live_cross = set(n for c in by["cross"] if c.vark for (_, n), l in zip(c.rows, c.live) if l)
    assert set(ar.KEY_COUNTS) <= live_cross
    assert set(ar.SELF_POS) <= set(n - 1 for c in by["self"] for (_, n), l in zip(c.rows, c.live) if l)
    assert set(ar.QUERY_COUNTS) <= set(q for c in by["prefill"] for q in c.kw["nq"])
    assert set(ar.QUERY_COUNTS) <= set(n for c in by["encoder"] if c.vark for n in c.kw["slot_k"])
    assert any(c.kw.get("out_rows") == 256 and c.kw["slot_k"] == [17, 100, 256] for c in by["encoder"])
    for f in by:
        assert set(c.H for c in by[f]) == {4, 6}, f
        assert set(c.profile for c in by[f]) == set(ar.PROFILES), f
    for f in ("cross", "self"):
        assert set(len(c.rows) for c in by[f]) == {1, 5}
        assert all(len(set(n for _, n in c.rows)) == 5 for c in by[f] if len(c.rows) == 5 and (c.vark or f == "self"))
        assert all(c.live.count(False) == 1 and c.kw["seq"] != list(range(5)) for c in by[f] if len(c.rows) == 5)
    assert len(set(c.name for c in CASES)) == len(CASES)


def test_loud_keys_sit_on_the_block_boundaries():
    assert list(ar.loud_keys([1])) == [0]
    assert list(ar.loud_keys([33])) == [31, 32]
    assert list(ar.loud_keys([65])) == [31, 32, 63, 64]
    assert list(ar.loud_keys([129])) == [31, 32, 63, 64, 95, 96, 127, 128]
    lk = ar.loud_keys([1500])
    assert lk.size == ar.LOUD_CAP and lk[-1] == 1499 and {1471, 1472, 1407, 1408} <= set(lk) and ar.MIN_MASS * lk.size < 1
    assert 0 in ar.loud_keys([1500], "descending") and ar.loud_keys([1500], "descending").size == ar.LOUD_CAP
    assert {99, 95, 96, 749, 735, 736} <= set(ar.loud_keys([100, 750]))


def test_profiles_do_what_they_are_for():
    """ascending: every 32-key block of every row raises the running maximum; peaked: every quiet probability is an f16 subnormal or zero; loud: scores reach +-60."""
    for prof, n in (("ascending", 1500), ("ascending", 129), ("peaked", 750), ("loud", 750), ("flat", 97), ("descending", 1500)):
        Q, K, V, loud = ar.make_operands(7, prof, 4, 1.0, [(n, [n])], [(0, n), (0, n)])
        s = Q[:, :64].astype(np.float64) @ K[0, :, :64].astype(np.float64).T
        if prof == "ascending":
            bm = np.array([s[:, b:b + 32].max(axis=1) for b in range(0, n, 32)])
            assert (np.diff(bm, axis=0) > 0).all()
        elif prof == "descending":
            assert (s[:, :32].max(axis=1) == s.max(axis=1)).all()
        elif prof == "peaked":
            quiet = np.setdiff1d(np.arange(n), loud[0])
            rel = np.exp2((s[:, quiet] - s.max(axis=1, keepdims=True)) * np.log2(np.e))
            assert (rel < 2.0 ** -24).all() and (rel.astype(np.float16) == 0).any() and (rel.astype(np.float16) > 0).any()
        elif prof == "loud":
            assert s.min() < -55 and s.max() > 55
        elif prof == "flat":
            assert (Q[:, :62] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cases_have_teeth_and_the_emulated_kernel_is_under_the_bound(case):
    Q, K, V, _ = case.operands()
    groups = {}
    for r, (s, n) in enumerate(case.rows):
        groups.setdefault((s, n), []).append(r)
    worst = 0.0
    for (s, n), rs in groups.items():
        for h in range(case.H):
            sl = slice(h * 64, h * 64 + 64)
            q, k, v = Q[rs, sl], K[s, :n, sl], V[s, :n, sl]
            ref, bound, _ = ar.reference(q, k, v, case.scale)
            less, more = ar.reference_off_by_one(q, k, v, case.scale)
            assert ((np.abs(less - ref) > 4 * bound).any(axis=1)).all(), "dropping the last of %d keys hides under the bound (slot %d head %d)" % (n, s, h)
            assert ((np.abs(more - ref) > 4 * bound).any(axis=1)).all(), "one pad key past %d keys hides under the bound (slot %d head %d)" % (n, s, h)
            worst = max(worst, float((np.abs(ar.emulate(q, k, v, case.scale, case.block) - ref) / bound).max()))
    print("%s: emulated kernel at %.3f of the bound" % (case.name, worst))
    assert worst < 1.0
