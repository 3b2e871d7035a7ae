"""The q8_0 cross K / V contract without a GPU: include/skw_kv8.h's evaluator, compiled into tests/cpp/kv8_main.cpp and run as a program of its own (plain and under the host
sanitizers), equals the numpy quantiser and scores of tests/kv8_ref_lib.py bit for bit; the numpy emulation of the kernel's arithmetic lies inside the derived bound on every
case, and both off-by-one variants of the key count lie outside it — the cases tests/test_gpu_kv8.py runs have teeth.  The node's cross_kv parameter is parsed before any device
is touched."""
import os
import subprocess

import numpy as np
import pytest

import align_ref_lib as al
import kv8_ref_lib as kv
from streamkit_amd import minihost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
CASES = kv.cases()
_EXE = {}


def driver(tmp_path_factory, sanitize=False):
    """tests/cpp/kv8_main.cpp, built the way align_ref_lib.driver builds align_main.cpp"""
    if sanitize not in _EXE:
        exe = tmp_path_factory.mktemp("kv8") / ("kv8_san" if sanitize else "kv8")
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-misleading-indentation", "-ffp-contract=off"] + flags +
                              ["-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "kv8_main.cpp")])
        _EXE[sanitize] = str(exe)
    return _EXE[sanitize]


def _bits16(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16).astype(np.int32).ravel()


def _record(H, n_ctx, count, q, K, V, poison):
    """one slot; rows at or past `count` hold NaN bit patterns when `poison` (the quantiser decides by the count, never by the value)"""
    K = np.array(K, np.float16); V = np.array(V, np.float16)
    if poison:
        K[count:] = np.float16(np.nan); V[count:] = np.float16(np.nan)
    return np.concatenate([np.array([H, n_ctx, count, q.shape[0]], np.int32), _bits16(q), _bits16(K), _bits16(V)])


def _parse(o, H, count, n_q):
    d = H * 64; T = (count + 31) // 32 * 32; k = 0
    def take(n, shape):
        nonlocal k
        a = o[k:k + n].reshape(shape); k += n
        return a
    kq = take(T * d, (T, d)); kd = take(T * 2 * H, (T, 2 * H)); vq = take(T * d, (T, d)); vd = take(T // 32 * d, (T // 32, d))
    sc = take(n_q * H * count, (n_q, H, count)).view(np.float32)
    stray = int(o[k]); assert k + 1 == o.size
    return kq, kd.astype(np.uint16).view(np.float16).astype(np.float32), vq, vd.astype(np.uint16).view(np.float16).astype(np.float32), sc, stray


def _slots_of(case, limit=2):
    """(slot, its quantiser count, the live rows on it) for the first `limit` slots that live rows use"""
    out = []
    for s, n in enumerate(case.slot_k()):
        rows = [r for r, (rs, _) in enumerate(case.rows) if rs == s and case.live[r]]
        if rows and len(out) < limit:
            out.append((s, n, rows))
    return out


@SANITIZE
def test_evaluator_equals_numpy_bit_for_bit(tmp_path_factory, sanitize):
    """the quantiser (every qs, every scale, pads by the count with NaNs behind it, nothing written outside the records) and the score chain, on every case's operands"""
    todo = [c for c in CASES if not sanitize or c.n_ctx <= 129 or c.H == 1]      # the sanitised build runs ~20x slower: the small cases and one of 1500 keys
    recs, want = [], []
    for c in todo:
        Q, K, V, _ = c.operands()
        for s, n, rows in _slots_of(c):
            recs.append(_record(c.H, c.n_ctx, n, Q[rows], K[s], V[s], poison=True)); want.append((c, s, n, Q[rows]))
    assert len(recs) >= 8
    outs = al.run(driver(tmp_path_factory, sanitize), recs)
    for (c, s, n, q), o in zip(want, outs):
        _, K, V, _ = c.operands()
        kq, kd, vq, vd = kv.quantize_slot(K[s], V[s], n)
        gkq, gkd, gvq, gvd, gsc, stray = _parse(o, c.H, n, q.shape[0])
        assert stray == 0, c.name
        assert np.array_equal(gkq, kq) and np.array_equal(gvq, vq), c.name
        assert np.array_equal(gkd.view(np.uint32), kd.view(np.uint32)) and np.array_equal(gvd.view(np.uint32), vd.view(np.uint32)), c.name
        if n % 32:
            assert not gkq[n:].any() and not gkd[n:].any() and not gvq[n:].any(), "%s: a pad key left a trace" % c.name
        for h in range(c.H):
            sc = kv.scores(q[:, h * 64:h * 64 + 64], kq, kd, h, n)
            assert np.array_equal(gsc[:, h].view(np.uint32), sc.view(np.uint32)), "%s head %d: scores differ from the contract's" % (c.name, h)


def test_zero_blocks_are_zero():
    """the cases that ask for them do hold an all-zero K block and an all-zero V^T block: d = 0 and qs = 0"""
    n = 0
    for c in CASES:
        if c.zero_blocks:
            _, K, V, _ = c.operands()
            kq, kd, vq, vd = kv.quantize_slot(K[0], V[0], c.slot_k()[0])
            for h in range(c.H):
                assert kd[2, 2 * h] == 0 and not kq[2, h * 64:h * 64 + 32].any() and kd[2, 2 * h + 1] != 0
                assert vd[1, h * 64 + 5] == 0 and not vq[32:64, h * 64 + 5].any() and vd[0, h * 64 + 5] != 0
            n += 1
    assert n >= 3


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_emulation_inside_and_off_by_one_outside_the_bound(case):
    _, _, _, quant, refs = case.prepared()
    worst = 0.0
    for rs, s, n, h, sl, sc, Vh, ref, bound in refs:
        em = kv.emulate(sc, quant[s][2], quant[s][3], h, n)
        worst = max(worst, float(kv.ratio(em, ref, bound).max()))
        if n > 1:      # a last key to miscount
            less, more = kv.off_by_one(sc, Vh)
            for name, wrong in (("one key short", less), ("one key over", more)):
                assert (kv.ratio(wrong, ref, bound).max(axis=1) > 1.0).all(), "%s slot %d, %d keys, head %d: %s passes" % (case.name, s, n, h, name)
    print("%s: emulation at %.3f of the bound" % (case.name, worst))
    assert worst <= 1.0


def test_case_list_covers_what_the_kernel_can_get_wrong():
    full = [c for c in CASES if not c.vark]; vark = [c for c in CASES if c.vark]
    assert {c.n_ctx for c in full} == set(kv.KEY_COUNTS) and {c.H for c in full} == {1, 2, 4}
    assert {n for c in vark for _, n in c.rows} >= set(kv.KEY_COUNTS) and {c.H for c in vark} == {1, 2, 4} and all(c.n_ctx == kv.N_CTX for c in vark)
    assert all(len(c.rows) <= 8 for c in CASES)
    assert any(not all(c.live) for c in full) and any(not all(c.live) for c in vark)
    assert any(c.kw.get("seq") and sorted(c.kw["seq"]) != list(range(len(c.rows))) for c in CASES)


def test_plugin_parses_cross_kv_before_touching_the_gpu(built):
    p = minihost.Plugin()
    assert p.metadata["param_schema"]["properties"]["cross_kv"]["default"] == "f16"
    with pytest.raises(RuntimeError, match="Invalid config: cross_kv \"q8_0\" needs precision \"f16_mfma\""):
        p.create_node({"cross_kv": "q8_0"})                                   # the default precision is exact
    with pytest.raises(RuntimeError, match="Invalid config: cross_kv \"q8_0\" needs precision \"f16_mfma\""):
        p.create_node({"cross_kv": "q8_0", "precision": "exact"})
    with pytest.raises(RuntimeError, match="Invalid config: cross_kv must be"):
        p.create_node({"cross_kv": "q4_0", "precision": "f16_mfma"})
    with pytest.raises(RuntimeError, match="Invalid config: invalid type for `cross_kv`"):
        p.create_node({"cross_kv": 8})
    # accepted: the configuration parses, and what fails afterwards is the model file that is not there (or, without a GPU, the device) — never the configuration
    with pytest.raises(RuntimeError) as e:
        p.create_node({"cross_kv": "q8_0", "precision": "f16_mfma", "model_path": "/nonexistent/model.bin"})
    assert "Invalid config" not in str(e.value)
