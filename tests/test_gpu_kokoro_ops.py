"""The Kokoro synthesiser's HIP kernels (streamkit_amd/csrc/skw_tts.hip), operator by operator at Kokoro-82M's widths, BIT FOR BIT against the CPU checker's operator
(oracle/skw_kokoro_oracle.cpp; both through include/skw_kokoro_ops.h), on the case tables of tests/kokoro_ops_lib.py — which tests/test_cpu_kokoro_ops.py holds to float64 and
to the edges they claim.  Every kernel variant is forced in turn (skw_tts_debug_conv_mode / _conv_tile / _lstm_mode) and the launch counters prove that the forced variant is
what ran.  Then the whole network at production width against the checker, with no spectrum rows masked, and again under every forced variant.
The hooks' outputs are arena buffers that start as NaNs before every call (allocation poisoning is switched on for this module): an element a kernel leaves unwritten shows."""
import contextlib
import os

import numpy as np
import pytest

import kokoro_lib
import kokoro_ops_lib as K
from streamkit_amd.tts import TILES as TILE_COUNTER, launch_counts
from test_gpu_kokoro import TOL_GEN, TOL_WAVE, _rel, _wrap_mask

pytestmark = pytest.mark.gpu
CONV_COUNTERS = ("conv", "t12", "t14", "t18", "t28")


@pytest.fixture(scope="module")
def eng():
    tts = kokoro_lib.Tts(kokoro_lib.synth_kokoro_dir("micro"))
    tts.L.skw_tts_debug_alloc_poison(1)
    yield tts
    tts.L.skw_tts_debug_alloc_poison(1 if os.environ.get("SKW_TEST_ALLOC_POISON") == "1" else 0)
    tts.close()


@contextlib.contextmanager
def forced(L, conv_mode=0, tile=(0, 0), lstm_mode=0):
    """the switches set for the block and back to automatic after it; yields a function returning the launch counters since the block began"""
    assert L.skw_tts_debug_conv_tile(*tile) == 0
    L.skw_tts_debug_conv_mode(conv_mode); L.skw_tts_debug_lstm_mode(lstm_mode); launch_counts(L, reset=True)
    try:
        yield lambda: launch_counts(L)
    finally:
        L.skw_tts_debug_conv_mode(0); L.skw_tts_debug_lstm_mode(0); L.skw_tts_debug_conv_tile(0, 0)


def _only(counts, which, n=None):
    """of the convolution kernels, only `which` ran (n times)"""
    return all((counts[c] == 0) for c in CONV_COUNTERS if c != which) and (counts[which] == n if n is not None else counts[which] > 0)


def test_switches_refuse_what_they_do_not_know(eng):
    L = eng.L
    for pair in ((2, 4), (1, 1), (3, 8), (0, 8), (1, 0)):
        assert L.skw_tts_debug_conv_tile(*pair) == -1
    assert L.skw_tts_debug_conv_tile(0, 0) == 0
    x, w, b = K.conv_inputs("short_input")
    assert eng.ops().f["conv"](eng.h, x.ctypes.data, 2, 16, w.ctypes.data, 16, 11, None, 1, 5, 2, None, 0) == -2      # no output row at this padding


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name", sorted(K.CONV))
def test_conv_every_kernel_bit_for_bit(eng, name, bias):
    x, w, b = K.conv_inputs(name); Ci, Co, Kk, stride, dil, pad, T = K.CONV[name]; b = b if bias else None
    want = K.checker("conv", name, bias); ops = eng.ops()
    with forced(eng.L, conv_mode=1) as counts:
        got = ops.conv(x, w, b, stride, dil, pad)
        assert _only(counts(), "conv", 1)
    assert K.same_bits(got, want), (name, "untiled", _rel(got, want))
    for tile in K.TILES:
        with forced(eng.L, conv_mode=2, tile=tile) as counts:
            got = ops.conv(x, w, b, stride, dil, pad)
            assert _only(counts(), TILE_COUNTER[tile], 1), (tile, counts())
        assert K.same_bits(got, want), (name, tile, int(np.isnan(got).sum()), _rel(np.nan_to_num(got), want))
    with forced(eng.L) as counts:      # the automatic choice, recorded
        got = ops.conv(x, w, b, stride, dil, pad); c = counts()
    assert K.same_bits(got, want) and sum(c[k] for k in CONV_COUNTERS) == 1
    print("conv %s: automatic choice %s" % (name, [k for k in CONV_COUNTERS if c[k]][0]))
    To = want.shape[0]
    with forced(eng.L, conv_mode=0, tile=(2, 8)) as counts:      # a forced tile replaces the tile only: a launch that would be untiled stays untiled
        got = ops.conv(x, w, b, stride, dil, pad)
        assert _only(counts(), "t28" if (To >= 32 and Kk * Ci >= 32) else "conv", 1)
    assert K.same_bits(got, want)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name", sorted(K.CONVTR))
def test_convtr_direct_and_per_phase_bit_for_bit(eng, name, bias):
    x, w, b = K.convtr_inputs(name); Ci, Co, Kk, stride, pad, out_pad, dw, T = K.CONVTR[name]; b = b if bias else None
    want = K.checker("convtr", name, bias); ops = eng.ops()
    if dw:
        with forced(eng.L) as counts:
            got = ops.convtr(x, w, b, stride, pad, out_pad, True); c = counts()
        assert not np.isnan(got).any() and K.same_bits(got, want) and c["convtr_direct"] == c["convtr_phased"] == 0
        return
    with forced(eng.L, conv_mode=1) as counts:
        direct = ops.convtr(x, w, b, stride, pad, out_pad, False); c = counts()
    assert c["convtr_direct"] == 1 and c["convtr_phased"] == 0 and sum(c[k] for k in CONV_COUNTERS) == 0
    assert not np.isnan(direct).any(axis=1).any() and K.same_bits(direct, want), (name, "direct")
    for mode, tile in [(0, (0, 0))] + [(2, t) for t in K.TILES]:
        with forced(eng.L, conv_mode=mode, tile=tile) as counts:
            got = ops.convtr(x, w, b, stride, pad, out_pad, False); c = counts()
        assert c["convtr_direct"] == 0 and c["convtr_phased"] == 1 and c["convtr_phase_launches"] == stride == sum(c[k] for k in CONV_COUNTERS), c
        if mode == 2:
            assert _only(c, TILE_COUNTER[tile], stride)
        assert not np.isnan(got).any(axis=1).any(), (name, tile, np.nonzero(np.isnan(got).any(axis=1))[0][:8])      # every output row of every phase was written
        assert K.same_bits(got, direct) and K.same_bits(got, want), (name, mode, tile)


@pytest.mark.parametrize("name", sorted(K.LSTM))
def test_lstm_both_kernels_bit_for_bit(eng, name):
    x, ws = K.lstm_inputs(name); In, H, T = K.LSTM[name]; want = K.checker("lstm", name); ops = eng.ops()
    with forced(eng.L, lstm_mode=1) as counts:
        got = ops.lstm_bi(x, ws); c = counts()
    assert (c["lstm"], c["lstm_mw"]) == (1, 0) and K.same_bits(got, want), (name, 1)
    with forced(eng.L, lstm_mode=2) as counts:
        got = ops.lstm_bi(x, ws); c = counts()
    if H % 32 == 0:
        assert (c["lstm"], c["lstm_mw"], c["lstm_mw_max_wg"]) == (0, 1, H // 32), c
    else:
        assert (c["lstm"], c["lstm_mw"]) == (1, 0), c      # the multi-workgroup kernel splits H in 32s: anything else falls back
    assert K.same_bits(got, want), (name, 2, int(np.isnan(got).sum()))
    assert eng.L.skw_tts_debug_lstm_error(eng.h) == 0


def test_lstm_epoch_wrap(eng):
    """k_tts_lstm_mw tags every exchanged h with {20-bit launch epoch, step}: at 2^20 launches (a server's life) the epoch wraps to 1 and the exchange words are cleared, so that
    tags of the engine's first launches cannot match again.  Four launches across the wrap, each against the checker; the engine's own words and error flag stay as they were."""
    x, ws = K.lstm_inputs("H256_T9"); want = K.checker("lstm", "H256_T9"); ops = eng.ops(); L = eng.L
    ids = np.array([0, 20, 17, 24, 27, 9, 31, 44, 5, 0], np.int32)
    with forced(L, lstm_mode=2) as counts:
        y0, _ = eng.generate(None, 3, 1.0, ids=ids)      # the engine's own launches first: they leave low-epoch tags in the engine's own words
        assert counts()["lstm_mw"] > 0
        L.skw_tts_debug_lstm_epoch(eng.h, 0xFFFFD)
        seen = []
        for _ in range(4):
            got = ops.lstm_bi(x, ws); seen.append(L.skw_tts_debug_lstm_epoch_get(eng.h))
            assert K.same_bits(got, want), seen
        assert seen == [0xFFFFE, 0xFFFFF, 1, 2] and L.skw_tts_debug_lstm_error(eng.h) == 0
        y1, _ = eng.generate(None, 3, 1.0, ids=ids)      # the engine after the wrap: epochs it has used before, on words the wrap cleared
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32)) and L.skw_tts_debug_lstm_error(eng.h) == 0


def test_layernorm_and_ada_ln_bit_for_bit(eng):
    ops = eng.ops()
    for Cn in K.LN_WIDTHS:
        x, g, b, gb = K.ln_inputs(Cn)
        for eps in K.LN_EPS:
            assert K.same_bits(ops.layernorm(x, g, b, eps), K.checker("layernorm", Cn, eps)), (Cn, eps)
        assert K.same_bits(ops.ada_ln(x, gb), K.checker("ada_ln", Cn)), Cn      # (AdaLayerNorm's eps is the contract's 1e-5: the operator takes none)


def test_ada_in_act_bit_for_bit(eng):
    ops = eng.ops()
    for T, Cn in K.ADA_IN:
        x, gb, act = K.ada_in_inputs(T, Cn)
        got = ops.ada_in_act(x, gb, act)
        assert K.same_bits(got, K.checker("ada_in_act", (T, Cn))), (T, Cn, act, int(np.isnan(got).sum()))


def test_attention_bit_for_bit(eng):
    ops = eng.ops()
    for name, (heads, T, qs) in K.ATTN.items():
        q, k, v = K.attn_inputs(name)
        got = ops.attention(q, k, v, heads)
        assert K.same_bits(got, K.checker("attention", name)), (name, int(np.isnan(got).sum()))


# ------------------------------------------------------------------ the whole network at production width
STAGES = ((5, "bert"), (6, "d_en"), (7, "t_en"), (1, "f0"), (2, "en"), (3, "dec"))


def test_kokoro_82m_matches_the_checker_and_every_variant_agrees():
    """Kokoro-82M's widths against the checker on two short utterances (tests/kokoro_ops_lib.py FIXTURES; tests/test_cpu_kokoro_ops.py shows that their source phases cannot wrap
    on an ulp, so NO spectrum row is masked here): durations exact, everything through the decoder bit-identical, source / spectrum / waveform within the stage tests' tolerances.
    Then the longer one under every forced convolution tile, untiled, and both LSTM kernels: all nine taps and the waveform bit-identical to the automatic run."""
    d = kokoro_lib.synth_kokoro_dir("kokoro82m")
    tts = kokoro_lib.Tts(d); orc = kokoro_lib.OracleTts(d); tts.taps(True); L = tts.L
    try:
        for name, (ids, speed) in K.FIXTURES.items():
            ids = np.asarray(ids, np.int32)
            with forced(L) as counts:
                y, _ = tts.generate(None, 50, speed, ids=ids); auto = counts()
            r = orc.synth(None, 50, speed, ids=ids)
            assert np.array_equal(tts.tap(0).astype(np.int32), r["dur"]) and y.size == r["y"].size == 600 * int(r["dur"].sum())
            for what, stage in STAGES:
                assert np.array_equal(tts.tap(what).view(np.uint32), r[stage].ravel().view(np.uint32)), (name, stage, _rel(tts.tap(what), r[stage].ravel()))
            har, post = tts.tap(8).reshape(-1, 22), tts.tap(4).reshape(-1, 22)
            keep, wraps = _wrap_mask(har, r["har"])
            e = {"source": _rel(har[:, :11], r["har"][:, :11]), "spec": _rel(post, r["post"]), "wave": _rel(y, r["y"])}
            print("kokoro82m %s: %d tokens -> %d frames in %.2f ms; %d wraps; rel rms err %s; automatic launches %s"
                  % (name, ids.size, y.size // 600, tts.last_ms(), wraps, {a: "%.2g" % b for a, b in e.items()}, {k: v for k, v in auto.items() if v}))
            assert wraps == 0 and keep.all()
            assert e["source"] < TOL_GEN and e["spec"] < TOL_GEN and e["wave"] < TOL_WAVE, e
            if ids.size >= 8:      # the automatic choice at 8 tokens and up: k_tts_lstm_mw, eight workgroups per direction at H = 256
                assert auto["lstm"] == 0 and auto["lstm_mw"] > 0 and auto["lstm_mw_max_wg"] == 8, auto
        base = [y] + [tts.tap(k) for k in range(9)]
        variants = [("untiled", dict(conv_mode=1))] + [("tile %d,%d" % t, dict(conv_mode=2, tile=t)) for t in K.TILES] + [("lstm 1", dict(lstm_mode=1)), ("lstm 2", dict(lstm_mode=2))]
        for label, kw in variants:
            with forced(L, **kw) as counts:
                yv, _ = tts.generate(None, 50, speed, ids=ids); c = counts()
            if "tile" in kw:
                assert _only(c, TILE_COUNTER[kw["tile"]]) and c["convtr_direct"] == 0 and c["convtr_phased"] == 2, (label, c)
            elif kw.get("conv_mode") == 1:
                assert _only(c, "conv") and c["convtr_direct"] == 2 and c["convtr_phased"] == 0, (label, c)
            elif kw["lstm_mode"] == 1:
                assert c["lstm"] > 0 and c["lstm_mw"] == 0, (label, c)
            else:
                assert c["lstm"] == 0 and c["lstm_mw"] > 0 and c["lstm_mw_max_wg"] == 8, (label, c)
            for k, (a, b) in enumerate(zip([yv] + [tts.tap(k) for k in range(9)], base)):
                assert a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, k)
        assert L.skw_tts_debug_lstm_error(tts.h) == 0
    finally:
        tts.close()
