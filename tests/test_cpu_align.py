"""The word-timestamp contract without a GPU: include/skw_align.h's evaluator and streamkit_amd/csrc/skw_words.h, compiled into tests/cpp/align_main.cpp and run as a program of its
own, plain and under the host sanitizers.  The evaluator is held to transformers' own functions through tests/golden/align_cases.json (DTW paths, the median filter, the f32
normalisation), to the contract's formulas in torch double, and to short statements of the word rule and the record check."""
import numpy as np
import pytest

import align_ref_lib as al

SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
EPS = 2.0 ** -24      # half an f32 ulp, relative


# ---- DTW: path for path against transformers' _dynamic_time_warping
@SANITIZE
def test_dtw_equals_transformers_path_for_path(tmp_path_factory, sanitize):
    cases = al.load_fixture()["dtw"]
    assert len(cases) >= 60 and sum(c["kind"] == "grid" for c in cases) >= 25 and sum(c["kind"] == "normal" for c in cases) >= 25
    xs = [al.dtw_matrix(c["seed"], c["N"], c["K"], c["kind"]) for c in cases]
    for c, x in zip(cases, xs):
        assert al.digest(x) == c["digest"], "seeded input %d is not the one the fixture was written for" % c["seed"]
    outs = al.run(al.driver(tmp_path_factory, sanitize), [al.rec_dtw(x, 100 * n) for n, x in enumerate(xs)])
    ties = 0
    for n, (c, x, o) in enumerate(zip(cases, xs, outs)):
        got = al.parse_dtw(o, c["N"])
        assert al.moves(got["path_i"], got["path_j"]) == c["moves"], c
        assert (got["path_i"][0], got["path_j"][0]) == (0, 0) and (got["path_i"][-1], got["path_j"][-1]) == (c["N"] - 1, c["K"] - 1)
        assert list(got["jump"]) == c["jumps"], c
        assert list(got["t0"]) == [100 * n + 2 * j for j in c["jumps"]] and list(got["t1"]) == list(got["t0"][1:]) + [got["t0"][-1]]
        ties += c["kind"] == "grid" and len(np.unique(x)) < x.size
    assert ties >= 20      # the grid cases do repeat values: the tie rule was exercised


# ---- step 4 alone against _median_filter, bit for bit (selection: nothing to round)
@SANITIZE
def test_median_filter_equals_transformers(tmp_path_factory, sanitize):
    cases = al.load_fixture()["median"]
    assert {c["K"] for c in cases} >= {1, 3, 4, 7}
    zs = [al.dtw_matrix(c["seed"], c["N"], c["K"], c["kind"]) for c in cases]
    for c, z in zip(cases, zs):
        assert al.digest(z) == c["digest"]
    for c, o in zip(cases, al.run(al.driver(tmp_path_factory, sanitize), [al.rec_median(z) for z in zs])):
        assert list(o) == c["out_bits"], c["seed"]


# ---- steps 3-5 against transformers' f32 normalisation (tiny cases): the same quantity up to f32 rounding of its mean / std
def test_steps_3_to_5_track_transformers_f32(tmp_path_factory):
    """transformers normalises in f32; the contract in f64 rounded once.  Per element |dz| <= (|z| + |mean| / std) * c * N * eps for the f32 sums of N terms (c = 4 covers the
    mean, the deviations' squares and the square root); the median selects among such values (their order may swap only inside that error) and the head mean adds H more roundings."""
    cases = al.load_fixture()["normalise"]
    Ps = [al.weights_exact(c["seed"], c["H"], c["N"], c["K"]) for c in cases]
    for c, P in zip(cases, Ps):
        assert al.digest(P[None]) == c["digest"]
    for c, P, o in zip(cases, Ps, al.run(al.driver(tmp_path_factory), [al.rec_reduce(P, P.shape[2]) for P in Ps])):
        want = np.array(c["neg_matrix_bits"], np.int32).view(np.float32).reshape(c["N"], c["K"])
        got = o.view(np.float32).reshape(c["N"], c["K"])
        ratio = float(np.max(np.abs(P.mean(axis=1)) / P.std(axis=1)))
        bound = (np.sqrt(c["N"]) + ratio) * 4 * c["N"] * 2 * EPS + c["H"] * 2 * EPS * np.sqrt(c["N"])      # |z| <= sqrt(N) for any column of N values
        assert np.max(np.abs(got - want)) <= bound, (c["seed"], float(np.max(np.abs(got - want))), bound)


# ---- steps 3-5 against the contract's formulas in torch double
STEP345 = [(1, 2, 1), (2, 2, 3), (2, 3, 4), (6, 2, 7), (1, 17, 7), (2, 40, 120), (6, 33, 65), (3, 226, 96), (6, 64, 750), (2, 12, 1500)]


@SANITIZE
def test_steps_3_to_5_equal_torch_double(tmp_path_factory, sanitize):
    """every value within 1 f32 ulp of the double evaluation, at most 0.1 % not identical (a sequential f64 sum and torch's pairwise one differ in the last place of a double,
    which moves an f32 rounding only when the value sits on a rounding boundary)"""
    Ps = [al.weights_like(4000 + n, H, N, K) for n, (H, N, K) in enumerate(STEP345)]
    assert {K for _, _, K in STEP345} >= {1, 3, 4, 7} and any(N == 2 for _, N, _ in STEP345)
    recs = [al.rec_reduce(P, P.shape[2]) for P in Ps] + [al.rec_reduce(Ps[6], 40), al.rec_reduce(Ps[6], 65, split=2), al.rec_reduce(Ps[5], 120, width=3)]
    wants = [al.steps345_double(P, P.shape[2]) for P in Ps] + [al.steps345_double(Ps[6], 40), al.steps345_double(Ps[6], 65), al.steps345_double(Ps[5], 120, width=3)]
    outs = al.run(al.driver(tmp_path_factory, sanitize), recs)
    total = differ = 0
    for o, w in zip(outs, wants):
        got = o.view(np.float32).reshape(w.shape)
        d = al.ulp_diff(got, w)
        assert d.max() <= 1, int(d.max())
        total += d.size; differ += int((d != 0).sum())
    print("steps 3-5: %d of %d values not identical to torch double" % (differ, total))
    assert total > 100000 and differ <= total // 1000
    # heads accumulated by two calls (two layers) are the heads accumulated by one
    assert np.array_equal(outs[6], outs[len(Ps) + 1])


def test_zero_variance_column_is_zero(tmp_path_factory):
    P = al.weights_like(4100, 2, 9, 12, zero_var_col=5)
    P[1, :, 5] = P[1, 0, 5]
    got = al.run(al.driver(tmp_path_factory), [al.rec_reduce(P, 12, width=1)])[0].view(np.float32).reshape(9, 12)
    assert np.all(got[:, 5] == 0) and np.all(np.isfinite(got)) and np.any(got[:, 4] != 0)


# ---- step 1 against float64 softmax, and the crop rule
def qk_inputs(seed, rows, n_keys):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, 64)) * 0.7).astype(np.float16), (rng.standard_normal((n_keys, 64)) * 0.7).astype(np.float16)


@SANITIZE
def test_weights_within_derived_bound_of_float64_softmax(tmp_path_factory, sanitize):
    shapes = [(3, 40), (2, 64), (2, 96), (2, 1500), (1, 1)]
    ins = [qk_inputs(4200 + n, r, k) for n, (r, k) in enumerate(shapes)]
    for (q, K), o in zip(ins, al.run(al.driver(tmp_path_factory, sanitize), [al.rec_weights(q, K) for q, K in ins])):
        P = o.view(np.float32).reshape(q.shape[0], K.shape[0]).astype(np.float64)
        ref = al.softmax_f64(q, K)
        smax = float((np.abs(q.astype(np.float64)) @ np.abs(K.astype(np.float64)).T).max())
        excess = np.max(np.abs(P - ref) - (al.qk_bound(K.shape[0], smax) * ref + al.QK_ABS))
        assert excess <= 0, excess
        assert np.all(np.abs(P.sum(-1) - 1) < 1e-5)


def test_crop_rule_and_top_heads(tmp_path_factory):
    kw = [(3000, 0, 1500, 1500), (3000, 0, 96, 96), (500, 0, 1500, 250), (4000, 2800, 1500, 600), (3001, 3000, 1500, 1), (3001, 2998, 64, 1), (7000, 1000, 1500, 1500), (205, 0, 128, 102)]
    tops = [(4, 6, 2), (2, 2, 1), (32, 20, 16), (6, 8, 9), (4, 32, 1)]
    outs = al.run(al.driver(tmp_path_factory), [np.array([5, a, b, c], np.int32) for a, b, c, _ in kw] + [np.array([6, a, b, c], np.int32) for a, b, c in tops])
    assert [int(o[0]) for o in outs[:len(kw)]] == [w for _, _, _, w in kw]
    for (L, H, n), o in zip(tops, outs[len(kw):]):
        m = o[:32].view(np.uint32)
        want = [((1 << H) - 1 if L - min(n, L) <= l < L else 0) for l in range(32)]
        assert [int(v) for v in m] == want and int(o[32]) == min(n, L) * H


# ---- the word rule on hand-written token lists
@SANITIZE
def test_word_rule(tmp_path_factory, sanitize):
    ni = "你".encode()      # one character, three bytes
    lists = [
        ([(b" Hello", 10), (b" wor", 20), (b"ld", 26), (b"!", 30)], 40, [(0, 1, 10, 20, b"Hello"), (1, 4, 20, 40, b"world!")]),
        ([(b"And", 0), (b" so", 8)], 8, [(0, 1, 0, 8, b"And"), (1, 2, 8, 8, b"so")]),                                              # first token starts a word without a space
        ([(b" a", 4), (b" " + ni[:2], 6), (ni[2:], 8), (b" b", 12)], 20, [(0, 3, 4, 12, b"a " + ni), (3, 4, 12, 20, b"b")]),       # a split character: its pieces stay together,
        ([(b" x", 2), (ni[:1], 4), (b" y", 6), (ni[1:], 7), (b" z", 9)], 11, [(0, 5, 2, 11, b"x" + ni[:1] + b" y" + ni[1:] + b" z")]),      # bytes that never become valid keep the word open
        ([(b" ", 1), (b" ", 2), (b" end", 5)], 9, [(2, 3, 5, 9, b"end")]),                                                         # words that trim to nothing are skipped
        ([(b" late", 30), (b" early", 20)], 10, [(0, 1, 30, 30, b"late"), (1, 2, 20, 20, b"early")]),                              # end >= start
        ([], 5, []),
        ([(b"", 3), (b" w", 4)], 6, [(1, 2, 4, 6, b"w")]),
    ]
    outs = al.run(al.driver(tmp_path_factory, sanitize), [al.rec_words(t, e) for t, e, _ in lists])
    for (_, _, want), o in zip(lists, outs):
        assert al.parse_words(o) == want


# ---- record validation
@SANITIZE
def test_record_validation(tmp_path_factory, sanitize):
    L, H, clip = 4, 6, 3
    cases = [((1, 7, [0, 0, 0x3f, 0x3f]), None), ((0, 0, []), None), ((0, 2, [0xffffffff] * 32), None), ((1, 1, [1]), None), ((1, 15, [0, 0, 0, 0x20]), None),
             ((1, 7, []), "clip 3: alignment asked for with an empty head mask"),
             ((1, 7, [0, 0, 0, 0x40]), "clip 3: alignment head 6 of layer 3 outside the model's 6 heads"),
             ((1, 7, [1, 0, 0, 0, 1]), "clip 3: alignment head in layer 4 outside the model's 4 decoder layers"),
             ((1, 6, [1]), "clip 3: alignment median_width 6 is not an odd number in [1, 15]"),
             ((1, 0, [1]), "clip 3: alignment median_width 0 is not an odd number in [1, 15]"),
             ((1, -7, [1]), "clip 3: alignment median_width -7 is not an odd number in [1, 15]"),
             ((1, 17, [1]), "clip 3: alignment median_width 17 is not an odd number in [1, 15]")]
    outs = al.run(al.driver(tmp_path_factory, sanitize), [al.rec_params(L, H, clip, e, w, m) for (e, w, m), _ in cases])
    for (_, want), o in zip(cases, outs):
        assert al.parse_params(o) == ((1, "") if want is None else (0, want))
