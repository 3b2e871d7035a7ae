"""The sampler's draw on the CPU: the oracle's hook (skwo_debug_sample_logits) against numpy's generator and a numpy restatement of libstdc++'s draw on every row of
tests/sampler_draw_lib.py; include/skw_draw.h's serial walks — what one lane of block_discrete_draw runs, block skipping included — against the plain sequential
definition (tests/cpp/draw_main.cpp, staged as the kernel stages a row); and the case set itself: it visits what it claims, and the skip logic is exercised."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sampler_draw_lib as sd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_LIST = [51864, 51865, 51866, 4096, 4097, 64, 65, 1]


@pytest.fixture(scope="module")
def cases(oracle_tiny):
    om = oracle_tiny
    return sd.all_cases(om, om.default_params())


@pytest.fixture(scope="module")
def draw_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("draw") / "draw_main"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-misleading-indentation", "-ffp-contract=off", "-O2", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(HERE, "cpp", "draw_main.cpp")])
    return str(exe)


def run_draw_main(exe, records):
    """records: [(weights f32, u)] -> [dict] in order"""
    buf = [struct.pack("<i", len(records))]
    for w, u in records:
        w = np.ascontiguousarray(w, dtype=np.float32)
        buf.append(struct.pack("<i", w.size) + struct.pack("<d", u) + w.tobytes())
    out = subprocess.check_output([exe], input=b"".join(buf)).decode().split("\n")
    res = []
    for line in out[:len(records)]:
        f = line.split()
        res.append(dict(idx=int(f[0]), sum=f[1], skip1=int(f[2]), blocks=int(f[3]), skip2=int(f[4]), reached2=int(f[5]), ref_idx=int(f[6]), ref_sum=f[7]))
    assert len(res) == len(records)
    return res


@pytest.fixture(scope="module")
def family_runs(draw_exe):
    """every weight family at every n, every u of the family: (family, n, label, u, weights, draw_main's line)"""
    recs, meta = [], []
    for fi, fam in enumerate(sd.WEIGHT_FAMILIES):
        for n in N_LIST:
            w = sd.weight_family(fam, n, np.random.default_rng(100 * fi + n % 97))
            for label, u in sd.family_us(fam, w).items():
                recs.append((w, u)); meta.append((fam, n, label, u, w))
    return [m + (r,) for m, r in zip(meta, run_draw_main(draw_exe, recs))]


def test_untemper_inverts_the_tempering():
    rng = np.random.default_rng(1)
    for y in [0, 1, 0x80000000, 0xFFFFFFFF, 0x800, 0xFFFFF800] + [int(x) for x in rng.integers(0, 1 << 32, 200)]:
        st = sd.crafted_state(5, 17, y, y ^ 0x5A5A5A5A)
        bg = np.random.MT19937(); bg.state = {"bit_generator": "MT19937", "state": {"key": st[:624].copy(), "pos": 17}}
        assert [int(x) for x in bg.random_raw(2)] == [y, y ^ 0x5A5A5A5A]
    bg = np.random.MT19937(); st = sd.mt_state(0, 624); bg.state = {"bit_generator": "MT19937", "state": {"key": st[:624].copy(), "pos": 624}}
    assert [int(x) for x in bg.random_raw(2)] == [2357136044, 2546248239]      # std::mt19937(0)'s first two outputs


def test_oracle_generator_equals_numpys(cases):
    """(a) state after the draw and u, for every state of the case set and every crafted u at every index it can sit at"""
    greedy, sampled = cases
    states = [(c["name"], c["state"]) for c in sampled]
    for seed in (0, 1, 12345):
        states += [("seed%d@%d" % (seed, i), sd.mt_state(seed, i)) for i in sd.STATE_IDX]
    for name, (lo, hi) in sd.CRAFTED_U.items():
        states += [("%s@%d" % (name, i), sd.crafted_state(77, i, lo, hi)) for i in (0, 1, 622)]
    for name, st in states:
        u_ref, after_ref = sd.generator_ref(st)
        u, after = sd.oracle_canonical(st)
        assert u == u_ref and 0.0 <= u < 1.0, (name, u, u_ref)
        assert np.array_equal(after, after_ref), name
    want = {"zero": 0.0, "2^-64": 2.0 ** -64, "half": 0.5, "after_half": float(np.nextafter(0.5, 1.0)), "1-2^-53": 1.0 - 2.0 ** -53, "ones": 1.0 - 2.0 ** -53}
    for name, (lo, hi) in sd.CRAFTED_U.items():
        assert sd.oracle_canonical(sd.crafted_state(3, 622, lo, hi))[0] == want[name], name


def test_oracle_draw_equals_the_numpy_reference(cases, oracle_tiny):
    """(b) on the hook's own probs; the state the hook returns is numpy's; a greedy row leaves its generator alone and equals skwo_debug_process_logits"""
    import logit_rules_lib as lr
    om = oracle_tiny; po = om.default_params()
    greedy, sampled = cases
    n = 0
    for c in sampled:
        o = sd.oracle_sample(om, po, c)
        u, after = sd.generator_ref(c["state"])
        i, _, _ = sd.draw_ref(o["probs"], u)
        assert o["tok"]["id"] == i, (c["name"], o["tok"]["id"], i, u)
        assert np.array_equal(o["state"], after), c["name"]
        assert np.float32(o["tok"]["p"]) == o["probs"][i] and (np.float32(o["tok"]["plog"]) == o["logprobs"][i]) and np.isposinf(o["tok"]["margin"])
        n += 1
    for c in greedy:
        o = sd.oracle_sample(om, po, c)
        assert np.array_equal(o["state"], c["state"]), c["name"]
        ref = lr.oracle_process(om, po, c["hist"], c["raw"])
        assert ref[2] == o["tok"] and np.array_equal(ref[0].view(np.uint32), o["filtered"].view(np.uint32)), c["name"]
        n += 1
    assert n == len(greedy) + len(sampled)
    bad = c["state"].copy(); bad[624] = 625
    c2 = dict(c); c2["state"] = bad
    with pytest.raises(RuntimeError, match="rc=-2"):
        sd.oracle_sample(om, po, c2)


def test_serial_walks_equal_the_sequential_definition(family_runs):
    """(c) same index and same bits of sum, every family, every n, every u — and both agree with the numpy reference"""
    assert {(f, n) for f, n, *_ in family_runs} == {(f, n) for f in sd.WEIGHT_FAMILIES for n in N_LIST}
    for fam, n, label, u, w, r in family_runs:
        assert r["idx"] == r["ref_idx"] and r["sum"] == r["ref_sum"], (fam, n, label, r)
        i, s, _ = sd.draw_ref(w, u)
        assert r["ref_idx"] == i and int(r["ref_sum"], 16) == int(np.float64(s).view(np.uint64)), (fam, n, label, r, i)
        assert r["blocks"] == (n + 63) // 64
        if fam == "half_ulp_tie" and n > 64:      # the ties moved the sum: a walk that skipped blocks AT the bound would have left it at 1 + 2^-52
            assert float(s) > 1.0 + 2.0 ** -52 and r["skip1"] == 0


def test_skip_logic_is_exercised(family_runs):
    """(d) properties of the INPUTS under the reference rule (a block is skipped iff its largest element is below half an ulp of the running sum):
    flat rows skip nothing; after a spike 40 above the noise's largest no noise term can move a sum >= 1 (e^-40 < 2^-53), so the first chain skips every block behind the
    spike's — at least 90 % of the row for a spike in the first 4 097 elements of 51 864+; a second equal spike on the last element keeps the second chain going (u = 0.75)
    across the same blocks: at least 90 % there too (a lone spike ends the second chain at the spike: nothing left to skip); a hit in the low tail before a spike sees
    cp ~ 1e-17, whose half-ulp no probability is below: nothing skipped before the hit."""
    seen = {"flat": 0, "spike1": 0, "spike2": 0, "low": 0}
    for fam, n, label, u, w, r in family_runs:
        if fam == "flat":
            assert r["skip1"] == 0 and r["skip2"] == 0, (n, label, r); seen["flat"] += 1
        if fam.startswith("spike@"):
            s = min(int(fam[6:]), n - 1)
            behind = r["blocks"] - (s // 64 + 1)
            assert r["skip1"] == behind, (fam, n, label, r)
            if n >= 51864 and s <= 4096:
                assert r["skip1"] >= 0.9 * r["blocks"], (fam, n, r); seen["spike1"] += 1
            if label.startswith("low@"):
                assert r["skip2"] == 0 and r["idx"] <= s, (fam, n, label, r); seen["low"] += 1      # ("+": the element after cp[k], which may be the spike)
        if fam.startswith("spike2@") and n >= 51864 and label == "between":
            assert r["idx"] == n - 1 and r["reached2"] == r["blocks"]
            assert r["skip1"] >= 0.9 * r["blocks"] and r["skip2"] >= 0.9 * r["blocks"], (fam, n, r); seen["spike2"] += 1
    assert seen["flat"] >= 8 * 12 and seen["spike1"] >= 3 * 5 * 12 and seen["spike2"] == 9 and seen["low"] >= 50, seen
    print("\nskip counts at n = 51865 (family / u: first chain skipped, second chain skipped / reached, of blocks):")
    for fam, n, label, u, w, r in family_runs:
        if n == 51865 and label in ("half", "between", "low@4095", "1-2^-53"):
            print("  %-12s %-9s %4d  %4d / %4d  of %d" % (fam, label, r["skip1"], r["skip2"], r["reached2"], r["blocks"]))


def test_last_element_rule_and_zero_u_are_reached(family_runs, cases, oracle_tiny):
    """what the deliberately wrong builds must trip over exists in the inputs: hits that only cp_{n-1} = 1.0 produces, and u == 0 on a row whose first token is suppressed"""
    assert sum(1 for fam, n, label, u, w, r in family_runs if r["idx"] == n - 1 and n > 1 and sd.last_element_decides(w, u)) >= 5
    om = oracle_tiny; po = om.default_params()
    last = zero = 0
    for c in cases[1]:
        o = sd.oracle_sample(om, po, c)
        u, _ = sd.generator_ref(c["state"])
        if o["tok"]["id"] == om.hp.n_vocab - 1 and sd.last_element_decides(o["probs"], u):
            last += 1
        if u == 0.0 and np.isneginf(o["filtered"][0]):      # token 0 suppressed: all three implementations return index 0: p = 0, plog = -inf
            assert o["tok"]["id"] == 0 and o["tok"]["p"] == 0.0 and np.isneginf(o["tok"]["plog"])
            zero += 1
    assert last >= 1 and zero >= 1, (last, zero)


def test_case_set_visits_what_it_claims(cases, oracle_tiny):
    """(e) every gap, placement, orientation, state index, crafted u, temperature and family; the near-tie ids are admissible and ARE the two largest; the mass rule fires in
    some near-tie rows and not in others; rows on both sides of the fast-path gate"""
    om = oracle_tiny; po = om.default_params()
    greedy, sampled = cases
    assert {(c["gap"], c["placement"], c["higher_wins"]) for c in greedy if c["family"] == "near_tie"} == {(g, p, h) for g in sd.GAPS for p in sd.PLACEMENTS for h in (False, True)}
    assert {c["placement"] for c in greedy if c["family"] == "triple_tie"} == set(sd.PLACEMENTS)
    assert {int(c["state"][624]) for c in sampled} == set(sd.STATE_IDX) and {int(c["state"][624]) for c in greedy} == set(sd.STATE_IDX)
    assert {c["u_name"] for c in sampled if c["u_name"]} == set(sd.CRAFTED_U)
    assert {float(c["temperature"]) for c in sampled} == {float(t) for t in sd.TEMPS}
    assert {c["family"] for c in sampled} == {"flat", "flat_ts", "spike", "staircase", "two_spikes", "subnormal", "rules", "mass_edge", "single"}
    fired = {True: 0, False: 0}; side = {True: 0, False: 0}; together = 0
    for c in greedy:
        o = sd.oracle_sample(om, po, c)
        fin = o["filtered"][~np.isneginf(o["filtered"])]
        if c["family"] == "single":
            assert fin.size == 1 and np.isposinf(o["tok"]["margin"]); continue
        srt = np.sort(fin)[::-1]
        mass = bool(np.all(np.isneginf(o["filtered"][:lr_beg(om)])))
        fired[mass] += 1
        if not mass:      # the two (three) placed logits are the row's largest, and their difference is the gap the case names
            gap = np.float32(srt[0] - srt[1])
            want = {"0": np.float32(0), "1ulp": np.float32(np.nextafter(np.float32(0.015625), np.float32(1)) - np.float32(0.015625))}.get(c["gap"], sd.GAPS[c["gap"]])
            assert gap == want and np.float32(o["tok"]["margin"]) == want, (c["name"], gap, want)
            side[bool(gap > np.float32(1e-4))] += 1
            if c["family"] == "triple_tie":
                assert srt[2] == srt[0]
            ids = np.flatnonzero(o["filtered"] >= srt[1])
            pr = o["probs"][ids]
            if c["higher_wins"] and pr[0] == pr[-1] and c["gap"] != "0":
                together += 1      # the larger logit sits at the higher index and the probabilities round together: "first index" decides against logit order
                assert o["tok"]["id"] == int(ids[0])
    assert fired[True] >= 7 and fired[False] >= 60 and side[True] >= 20 and side[False] >= 40 and together >= 4, (fired, side, together)
    print("\nnear-tie rows: mass rule fired in %d, not in %d; gap above the gate in %d, at or below in %d; probabilities rounded together against logit order in %d"
          % (fired[True], fired[False], side[True], side[False], together))
    lo = [c for c in sampled if c["aim"] and c["aim"][0] == "cp"]
    assert {c["aim"][1] for c in lo} == set(sd.LOW_TAIL_AT)
    n_launch = sd.launches(greedy, sampled)
    assert all(len(b) <= 64 for b in n_launch) and sum(len(b) for b in n_launch) >= len(greedy) + len(sampled)


def lr_beg(om):
    import logit_rules_lib as lr
    return lr.special_ids(om)["beg"]
