"""The three word-timestamp kernels (streamkit_amd/csrc/skw_kernels_align.hip) against the evaluator of include/skw_align.h, BIT FOR BIT, through the kernel-level hooks
skw_debug_align_qk / _reduce / _dtw.  The evaluator is tests/cpp/align_main.cpp, compiled here and run on the CPU (tests/test_cpu_align.py holds it to transformers).

Shapes are the smallest that cross every edge: a DTW row per thread up to 225 rows and a packed trace word every 16 keys (63, 64, 65), problems of one row or one key, the largest
problem (225 x 1500), five ragged problems in one launch; the reduce kernel's 250-column tiles and reflected margins (K 1, 3, 4, 7, 63, 64, 65, 1500), a zero-variance column, heads
arriving in two launches; the weights kernel's 64-key lane stride (40, 64, 96, 1500 keys at a 1500-key stride), 3 to 226 rows, both stored layouts of the cross K."""
import numpy as np
import pytest

import align_ref_lib as al

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope="module")
def ctx(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path); c = engine.Context(m, max_batch=1, max_samples=16000)
    yield c
    c.close(); m.close()


# ---- k_align_dtw
DTW_SHAPES = [(1, 1), (1, 7), (2, 1), (3, 64), (17, 63), (64, 65), (65, 64), (225, 750), (225, 1500)]


def _dtw_case(tmp_path_factory, N, K, kind):
    key = ("dtw", N, K, kind)
    if key not in _CACHE:
        x = al.dtw_matrix(7000 + 2 * (31 * N + K) + (kind == "grid"), N, K, kind)      # (odd seeds: the coarse grid, ties everywhere)
        ref = al.parse_dtw(al.run(al.driver(tmp_path_factory), [al.rec_dtw(x, 300)])[0], N)
        x.setflags(write=False)
        _CACHE[key] = (x, ref)
    return _CACHE[key]


@pytest.mark.parametrize("kind", ["grid", "normal"])
@pytest.mark.parametrize("N,K", DTW_SHAPES)
def test_dtw_equals_evaluator(ctx, tmp_path_factory, N, K, kind):
    x, ref = _dtw_case(tmp_path_factory, N, K, kind)
    jump, t0, t1 = ctx.align_dtw([x], seek_cs=[300])
    assert np.array_equal(jump, ref["jump"]) and np.array_equal(t0, ref["t0"]) and np.array_equal(t1, ref["t1"])
    assert jump[0] == 0 and np.all(np.diff(jump) >= 0) and jump[-1] <= K - 1


@pytest.mark.parametrize("kind", ["grid", "normal"])
def test_dtw_five_ragged_problems_in_one_launch(ctx, tmp_path_factory, kind):
    shapes = [(17, 63), (1, 1), (225, 750), (64, 65), (3, 64)]
    cases = [_dtw_case(tmp_path_factory, N, K, kind) for N, K in shapes]
    jump, t0, t1 = ctx.align_dtw([x for x, _ in cases], seek_cs=[300] * 5)
    for name, got in (("jump", jump), ("t0", t0), ("t1", t1)):
        assert np.array_equal(got, np.concatenate([r[name] for _, r in cases])), name


# ---- k_align_reduce
RED_T = (2, 3, 17, 65, 225)


def _reduce_case(tmp_path_factory, H, K):
    """five sequences of RED_T rows in one capture of stride K + 3 (the kernel must not read past its crop); sequence 1 is cropped to fewer keys where K allows; sequence 2 has a
    zero-variance column in every head"""
    key = ("red", H, K)
    if key not in _CACHE:
        rows, stride = sum(RED_T), K + 3
        P = al.weights_like(8000 + 10 * K + H, H, rows, stride)
        kw = [K, max(1, K - 5), K, K, K]
        r0 = np.concatenate([[0], np.cumsum(RED_T)])
        P[:, r0[2]:r0[3], min(5, K - 1)] = P[:, r0[2]:r0[2] + 1, min(5, K - 1)]
        split = H // 2                                                                     # the heads arrive as two layers (H = 1: one)
        recs = [al.rec_reduce(P[:, r0[i]:r0[i + 1]], kw[i], split=split if split else None) for i in range(5)]
        want = np.concatenate([o.view(np.float32) for o in al.run(al.driver(tmp_path_factory), recs)])
        P.setflags(write=False)
        _CACHE[key] = (P, kw, split, want, (sum(RED_T[i] * kw[i] for i in range(2)), RED_T[2], kw[2], min(5, K - 1)))
    return _CACHE[key]


@pytest.mark.parametrize("K", [1, 3, 4, 7, 63, 64, 65, 1500])
@pytest.mark.parametrize("H", [1, 2, 6])
def test_reduce_equals_evaluator(ctx, tmp_path_factory, H, K):
    P, kw, split, want, (zoff, zn, zkw, zcol) = _reduce_case(tmp_path_factory, H, K)
    layers = [P[:split], P[split:]] if split else [P]
    got = ctx.align_reduce(layers, RED_T, kw)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    z = got[zoff:zoff + zn * zkw].reshape(zn, zkw)
    if zkw <= 3:                                                                           # unfiltered: the zero-variance column itself comes out as (minus) zero
        assert np.all(z[:, zcol] == 0)
    assert np.all(np.isfinite(got))


# ---- k_align_qk
QK_N = (3, 16, 17, 226)
QK_KEYS = (40, 64, 96, 0)       # 0: all n_ctx = 1500 keys
QK_SLOT = (2, 0, 1, 1)
QK_H, QK_CTX, QK_GAP = 6, 1500, 2


def _qk_operands():
    if "qk" not in _CACHE:
        rng = np.random.default_rng(8800)
        d = QK_H * 64
        qrow0, at = [], QK_GAP
        for n in QK_N:
            qrow0.append(at); at += n + QK_GAP
        Q = (rng.standard_normal((at, d)) * 0.6).astype(np.float16)
        K = (rng.standard_normal((3, QK_CTX, d)) * 0.6).astype(np.float16)
        for s in range(3):      # a few loud keys: the other weights of those rows fall far down the exponential, some below its cut at -86
            for k in rng.integers(0, 40, size=2).tolist() + rng.integers(0, QK_CTX, size=3).tolist():
                K[s, k] = (K[s, k].astype(np.float32) * 12.0).astype(np.float16)
        Q.setflags(write=False); K.setflags(write=False)
        _CACHE["qk"] = (Q, K, np.array(qrow0, np.int32))
    return _CACHE["qk"]


def _qk_ref(tmp_path_factory, h):
    """the evaluator's weights of head h for every sequence: list of f32 [n][n_keys]"""
    key = ("qkref", h)
    if key not in _CACHE:
        Q, K, qrow0 = _qk_operands()
        recs, shapes = [], []
        for i, n in enumerate(QK_N):
            nk = QK_KEYS[i] or QK_CTX
            recs.append(al.rec_weights(Q[qrow0[i]:qrow0[i] + n, 64 * h:64 * h + 64], K[QK_SLOT[i], :nk, 64 * h:64 * h + 64])); shapes.append((n, nk))
        _CACHE[key] = [o.view(np.float32).reshape(s) for o, s in zip(al.run(al.driver(tmp_path_factory), recs), shapes)]
    return _CACHE[key]


@pytest.mark.parametrize("frag", [False, True], ids=["rows", "frag"])
@pytest.mark.parametrize("head_mask", [0b100010, 0b111111], ids=["2heads", "6heads"])
def test_qk_equals_evaluator_and_tracks_float64(ctx, tmp_path_factory, head_mask, frag):
    Q, K, qrow0 = _qk_operands()
    sentinel = np.float32(-7.0)
    P = ctx.align_qk(QK_H, QK_CTX, Q, K, head_mask, qrow0, QK_N, QK_SLOT, QK_KEYS, frag=frag, sentinel=sentinel)
    heads = [h for h in range(QK_H) if head_mask >> h & 1]
    assert P.shape == (len(heads), sum(QK_N), QK_CTX)
    r0 = np.concatenate([[0], np.cumsum(QK_N)])
    cut = 0
    for hl, h in enumerate(heads):
        for i, ref in enumerate(_qk_ref(tmp_path_factory, h)):
            n, nk = ref.shape
            got = P[hl, r0[i]:r0[i + 1]]
            assert np.array_equal(got[:, :nk].view(np.uint32), ref.view(np.uint32)), (h, i)
            assert np.all(got[:, nk:] == sentinel), "keys past the sequence's count were written"
            q, k = Q[qrow0[i]:qrow0[i] + n, 64 * h:64 * h + 64], K[QK_SLOT[i], :nk, 64 * h:64 * h + 64]
            f64 = al.softmax_f64(q, k)
            smax = float((np.abs(q.astype(np.float64)) @ np.abs(k.astype(np.float64)).T).max())
            excess = np.max(np.abs(got[:, :nk].astype(np.float64) - f64) - (al.qk_bound(nk, smax) * f64 + al.QK_ABS))
            assert excess <= 0, (h, i, excess)
            cut += int((got[:, :nk] == 0).sum())
    assert cut > 0      # the exponential's cut was reached somewhere
