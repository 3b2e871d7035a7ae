"""The exact precision's multi-query prompt cross attention (k_xattn_prefill_exact) against the single-query kernel it stands in for (k_dec_cross_attn<24, 4, 3>), byte for byte,
through the kernel-level tap skw_debug_xattn_exact: mq = 1 against mq = 0 on the same operands, for both output forms (f16 kperm rows, f32 rows).

Operands are seeded f16 values; a few K rows are scaled up so that the scores of some rows spread past exp's underflow.  Every K / V position past a slot's key count, V^T's pad keys
and every query row outside the sequences hold the NaN pattern 0x7E00; the output buffer starts as a sentinel that must survive wherever no row may be written.

Shapes: the smallest that cross every tile edge — 16 queries per workgroup (nq 1, 15, 16, 17, 33, 223), 32-key P.V blocks and 64-key score tiles (n_ctx 1, 33, 64, 65, 257, 1500),
the four-part f64 sum at tile counts that are no multiple of 4 (1, 2, 5, 24 tiles), per-slot key counts on either side of a block edge, sequences in non-monotone slot order with a
gap of unowned rows between them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
POISON = 0x7E00
GAP = 3
SETS = {"a": dict(nq=(17, 1, 223), slot=(2, 0, 1), counts=(1, 200, None)),
        "b": dict(nq=(16, 33, 15), slot=(1, 2, 0), counts=(31, 32, None))}
_OPS = {}


@pytest.fixture(scope="module")
def ctx(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path); c = engine.Context(m, max_batch=1, max_samples=16000)
    yield c
    c.close(); m.close()


def _operands(H, n_ctx, rows):
    """seeded once per geometry, shared by the launches that use it, never modified"""
    key = (H, n_ctx, rows)
    if key not in _OPS:
        rng = np.random.default_rng(1000 * H + n_ctx)
        d = H * 64
        Q = (rng.standard_normal((rows, d)) * 0.5).astype(np.float16)
        K = (rng.standard_normal((3, n_ctx, d)) * 0.5).astype(np.float16)
        V = rng.standard_normal((3, n_ctx, d)).astype(np.float16)
        for s in range(3):      # a few keys with +-large scores: s - max falls below exp's underflow (-104) in some rows
            for k in rng.integers(0, n_ctx, size=min(4, n_ctx)):
                K[s, k] = (K[s, k].astype(np.float32) * 40.0).astype(np.float16)
        for a in (Q, K, V):
            a.setflags(write=False)
        _OPS[key] = (Q, K, V)
    return _OPS[key]


@pytest.mark.parametrize("f32_out", [False, True])
@pytest.mark.parametrize("with_slot_k", [False, True])
@pytest.mark.parametrize("which", sorted(SETS))
@pytest.mark.parametrize("n_ctx", [1, 33, 64, 65, 257, 1500])
@pytest.mark.parametrize("H", [1, 6])
def test_mq_equals_single_query_bytes(ctx, H, n_ctx, which, with_slot_k, f32_out):
    S = SETS[which]
    nq, slot = np.array(S["nq"], np.int32), np.array(S["slot"], np.int32)
    row0 = np.zeros(3, np.int32); at = GAP
    for i in range(3):
        row0[i] = at; at += int(nq[i]) + GAP
    rows = at
    Q0, K, V = _operands(H, n_ctx, rows)
    owned = np.zeros(rows, bool)
    for i in range(3):
        owned[row0[i]:row0[i] + nq[i]] = True
    Q = Q0.view(np.uint16).copy(); Q[~owned] = POISON
    slot_k = np.array([min(n_ctx, c if c else n_ctx) for c in S["counts"]], np.int32) if with_slot_k else None
    fill_from = slot_k if with_slot_k else np.full(3, n_ctx, np.int32)
    try:
        one = ctx.xattn_exact(0, H, n_ctx, Q, K, V, fill_from, row0, nq, slot, slot_k=slot_k, f32_out=f32_out, k_pad=POISON, v_pad=POISON, sentinel=SENTINEL)
        many = ctx.xattn_exact(1, H, n_ctx, Q, K, V, fill_from, row0, nq, slot, slot_k=slot_k, f32_out=f32_out, k_pad=POISON, v_pad=POISON, sentinel=SENTINEL)
    except RuntimeError as e:      # a launch the device refused or faulted on: nothing more runs on it in this session
        pytest.exit("H %d n_ctx %d %s: %s" % (H, n_ctx, which, e), returncode=3)
    assert np.all(one[~owned] == SENTINEL) and np.all(many[~owned] == SENTINEL), "a row outside every sequence was written"
    vals = many[owned].view(np.float32) if f32_out else many[owned].view(np.float16)
    assert np.all(np.isfinite(vals.astype(np.float32))), "a poisoned position reached an output"
    assert not np.all(many[owned] == SENTINEL)
    bad = np.argwhere(one != many)
    assert bad.size == 0, "%d halves differ, first at row %d col %d: single %04x multi %04x" % (len(bad), bad[0][0], bad[0][1], one[tuple(bad[0])], many[tuple(bad[0])])
