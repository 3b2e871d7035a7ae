"""The CPU checker's Kokoro operators (oracle/skw_kokoro_oracle.cpp through include/skw_kokoro_ops.h) against plain float64 references, and the case tables of
tests/kokoro_ops_lib.py against the edges they claim to reach.  No GPU: tests/test_gpu_kokoro_ops.py then holds the HIP kernels to the checker bit for bit, on the same cases."""
import numpy as np
import pytest

import kokoro_lib
import kokoro_ops_lib as K

U = 2.0 ** -24      # unit roundoff of f32


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


# ------------------------------------------------------------------ a. the checker against float64
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name", sorted(K.CONV))
def test_checker_conv_within_the_chain_bound(built, name, bias):
    """one f32 fma chain of n terms from 0, the bias added after: |got - ref| <= (n + 2) 2^-24 sum |w||x| per output (n roundings of the chain, one of the bias add, one of slack
    for the reference's own float64 rounding; the standard first-order bound gamma_n sum |w||x| with n 2^-24 << 1)"""
    x, w, b = K.conv_inputs(name); Ci, Co, Kk, stride, dil, pad, T = K.CONV[name]
    got = K.checker("conv", name, bias); ref, mag = K.ref_conv(x, w, b if bias else None, stride, dil, pad)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref); bound = (Kk * Ci + 2) * U * mag
    print("checker conv %s bias=%d: worst error / bound %.3f" % (name, bias, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name", sorted(K.CONVTR))
def test_checker_convtr_within_the_chain_bound(built, name, bias):
    x, w, b = K.convtr_inputs(name); Ci, Co, Kk, stride, pad, out_pad, dw, T = K.CONVTR[name]
    got = K.checker("convtr", name, bias); ref, mag = K.ref_convtr(x, w, b if bias else None, stride, pad, out_pad, dw)
    n = -(-Kk // stride) * (1 if dw else Ci)      # the taps that reach one output, times the channels each walks
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (np.abs(got.astype(np.float64) - ref) <= (n + 2) * U * mag).all()


def _held(op, errs):
    """no bound follows from the contract for these (skw_expf, recurrences, f32 statistics of f64 sums): the checker's distance from float64 was measured on every case of the
    table (K.MEASURED, profiles/kokoro_ops/README.md) and is held at 4 x that"""
    worst = max(errs.values()); print("checker %s vs float64: worst max|got - ref| / max|ref| = %.3e (%s); recorded %.3e" % (op, worst, max(errs, key=errs.get), K.MEASURED[op]))
    assert worst <= 4.0 * K.MEASURED[op], errs


def test_checker_layernorm_and_ada_ln_against_float64(built):
    e_ln, e_ada = {}, {}
    for Cn in K.LN_WIDTHS:
        x, g, b, gb = K.ln_inputs(Cn)
        for eps in K.LN_EPS:
            e_ln[(Cn, eps)] = _rel(K.checker("layernorm", Cn, eps), K.ref_layernorm(x, g, b, eps))
        e_ada[Cn] = _rel(K.checker("ada_ln", Cn), K.ref_ada(x, gb, 1))
    _held("layernorm", e_ln); _held("ada_ln", e_ada)


def test_checker_ada_in_act_against_float64(built):
    errs = {}
    for T, Cn in K.ADA_IN:
        x, gb, act = K.ada_in_inputs(T, Cn)
        errs[(T, Cn)] = _rel(K.checker("ada_in_act", (T, Cn)), K.ref_act(K.ref_ada(x, gb, 0), act))
    _held("ada_in_act", errs)


def test_checker_attention_against_float64(built):
    errs = {}
    for name, (heads, T, qs) in K.ATTN.items():
        q, k, v = K.attn_inputs(name); got = K.checker("attention", name)
        errs[name] = _rel(got, K.ref_attention(q, k, v, heads))
        if qs > 1.0:      # the spread case: part of every row's probabilities underflows to exactly 0
            s = (q[:, :64].astype(np.float64) @ k[:, :64].astype(np.float64).T) * 0.125
            assert s.max() - s.min() > 100.0 and (s.max(axis=1) - s.min(axis=1) > 104.0).any()
    _held("attention", errs)


def test_checker_lstm_against_float64(built):
    errs = {}
    for name in K.LSTM:
        x, ws = K.lstm_inputs(name)
        errs[name] = _rel(K.checker("lstm", name), K.ref_lstm_bi(x, ws))
    _held("lstm", errs)


# ------------------------------------------------------------------ b. the tables reach the edges they claim (computed from the shapes)
def test_case_tables_reach_their_edges():
    for mt, nt in K.TILES:
        reached = {}
        for name in K.CONV:
            for edge, hit in K.conv_edges(name, mt, nt).items():
                reached[edge] = reached.get(edge, False) or hit
        need = ["ragged_rows", "ragged_kgroups", "ragged_k", "tap_straddles_slab", "scalar_stores"] + (["dead_second_mtile"] if mt == 2 else [])
        assert all(reached[e] for e in need), ((mt, nt), reached)
    # the production decoder chain is what it is said to be: Ktot 3270, nk4 818, 103 chunks, the last 2/8 full with a half-empty last k-group
    Ci, Co, Kk = K.CONV["decoder_input"][:3]; Ktot = Ci * Kk; nk4 = (Ktot + 3) // 4
    assert (Ktot, nk4, (nk4 + 7) // 8, nk4 % 8, Ktot % 4) == (3270, 818, 103, 2, 2)
    assert any(c[1] % 4 for c in K.CONV.values())
    lanes = lambda Cn: {(Cn - l + 255) // 256 for l in range(256)}      # elements per lane of the 256-lane sum
    assert any(len(lanes(Cn)) > 1 and max(lanes(Cn)) > 1 for Cn in K.LN_WIDTHS) and any(Cn <= 256 for Cn in K.LN_WIDTHS)
    Ts = sorted({T for T, _ in K.ADA_IN})
    for edge in (16, 512, 8 * 512):
        assert any(T < edge for T in Ts) and any(T > edge for T in Ts) and (edge in Ts or edge == 8 * 512)
    assert any((T + 511) // 512 == 9 for T in Ts)
    At = sorted({T for _, T, _ in K.ATTN.values()})
    assert any(T < 256 for T in At) and 256 in At and any(T > 256 for T in At) and {h for h, _, _ in K.ATTN.values()} == {2, 12}
    Hs = {H for _, H, _ in K.LSTM.values()}
    assert 256 in Hs and any(H % 32 for H in Hs) and any((H // 32) % 2 == 1 and H // 32 > 1 for H in Hs if H % 32 == 0)
    assert {T for _, H, T in K.LSTM.values() if H == 256} >= {1, 2, 9, 40}
    # norm inputs hold the row f32 statistics fail on
    x = K.ln_inputs(768)[0]
    assert abs(float(x[1].mean()) - 100.0) < 0.01 and 0.005 < float(x[1].astype(np.float64).std()) < 0.02
    x = K.ada_in_inputs(513, 65)[0]
    assert abs(float(x[:, 0].mean()) - 100.0) < 0.01 and 0.005 < float(x[:, 0].astype(np.float64).std()) < 0.02


# ------------------------------------------------------------------ c. the fixture utterances of the production-width test cannot wrap on an ulp
def test_fixture_utterances_cannot_wrap(built):
    """The source's STFT phase is a network input, and a bin with re < 0 and im near 0 sits at +-pi: its phase can come out on the other side when the two backends' platform
    sin / atan2 differ by an ulp.  tests/test_gpu_kokoro_ops.py compares the whole spectrum and waveform of these utterances with NO rows masked; this is what makes that fair.
    im is a float64 sum over the frame's 20 windowed source samples, identical arithmetic on both sides: it differs only as far as the source samples do.  A source sample is
    tanh of a 9-term chain over sines the platform's sin produced: sines an f32 ulp apart (7.5e-9 at |sine| <= 0.1) move it by about two ulps of 1.0 at most, and the Hann
    weights times |sin| sum to under 10, so |im| can move by about 2 x 10 x 2^-24 = 1.2e-6.  Every bin with re < 0 must keep |im| >= 8 x 10 x 2^-24 = 4.8e-6, four times that.
    Two families are exempt because their im does not follow the source's roundings like that: bins 0 and N/2, whose im is exactly +0 (asserted: the phase is exactly 0 or +pi),
    and row 0, whose frame is symmetric under the reflection pad, so that every im is the rounding residue of a sum that is 0 (the phase there flips only if a source sample
    itself differs; the no-rows-masked comparison on the GPU would show it).
    The bound first proposed for this test, |im| >= 1e-4 x the largest magnitude, cannot be met by any utterance: the source's low-energy bins sit under it by chance (16 and 74
    bins at these two utterances, 11 to 123 at the twelve others tried: profiles/kokoro_ops/README.md), and half of row 0 always.  The ids were picked among those for the largest
    margin: 7.2e-5 and 6.1e-6."""
    d = kokoro_lib.synth_kokoro_dir("kokoro82m"); orc = kokoro_lib.OracleTts(d)
    for name, (ids, speed) in K.FIXTURES.items():
        r = orc.synth(None, 50, speed, ids=np.asarray(ids, np.int32))
        har = r["har"]; mag, ph = har[:, :11].astype(np.float64), har[:, 11:].astype(np.float64)
        assert np.isin(har[:, [11, 21]], np.float32([0.0, np.pi])).all()
        re, im = (mag * np.cos(ph))[1:, 1:10], (mag * np.sin(ph))[1:, 1:10]
        floor = 8 * 10 * U; worst = float(np.abs(im[re < 0]).min())
        issue = int(((re < 0) & (np.abs(im) < 1e-4 * mag.max())).sum())
        print("fixture %s: %d tokens -> %d frames; smallest |im| at re < 0: %.3e (floor %.3e, largest magnitude %.3f); %d bins under 1e-4 x the largest magnitude"
              % (name, len(ids), r["F"], worst, floor, mag.max(), issue))
        assert worst >= floor
        assert len(ids) == (3 if name == "three" else 9) and (name == "three" or len(ids) >= 8)
