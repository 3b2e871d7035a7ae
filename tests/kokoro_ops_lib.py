"""Case tables and float64 references for the Kokoro operators, one at a time (include/skw_kokoro_ops.h): what tests/test_cpu_kokoro_ops.py holds the CPU checker's operators to,
and what tests/test_gpu_kokoro_ops.py runs through the product's kernels and compares with the checker bit for bit.  Every input is seeded by the case's name; the checker's
result for a case is computed once per process and shared (checker())."""
import ctypes as C
import functools
import os
import zlib

import numpy as np

from streamkit_amd.tts import KokoroOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [(1, 2), (1, 4), (1, 8), (2, 8)]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def checker_ops():
    return KokoroOps(C.CDLL(os.path.join(ROOT, "oracle", "libskw_oracle.so")), "skwo_kokoro_op_", None)


# ------------------------------------------------------------------ the tables (shapes: the smallest at which the named path exists)
# conv: name -> (Ci, Co, K, stride, dil, pad, T)
CONV = {
    "decoder_input": (1090, 1024, 3, 1, 1, 1, 70),      # the production decoder chain: Ktot 3270, nk4 818 (half-empty last k-group), 103 chunks (the last 2/8 full)
    "odd_widths": (33, 72, 7, 1, 3, 9, 200),            # Co16 = 80: the second MT tile of the last wave is dead
    "conv_post": (128, 22, 7, 1, 1, 3, 130),            # scalar stores (Co % 4 != 0); one row past a 128-row tile
    "f0n_conv": (1, 1, 3, 2, 1, 1, 75),                 # stride 2, the narrowest width
    "linear_5": (768, 2048, 1, 1, 1, 0, 5),             # ALBERT FFN, a few tokens
    "linear_302": (768, 2048, 1, 1, 1, 0, 302),         # ... and a long text
    "short_input": (16, 16, 11, 1, 5, 25, 2),           # almost every tap is padding
}
# convtr: name -> (Ci, Co, K, stride, pad, out_pad, depthwise, T)
CONVTR = {}
for _T in (1, 2, 37):
    CONVTR["up0_T%d" % _T] = (512, 256, 20, 10, 5, 0, False, _T)      # the production first up-sampling
    CONVTR["up1_T%d" % _T] = (96, 40, 12, 6, 3, 0, False, _T)         # the second up-sampling's geometry
for _T in (1, 33):
    CONVTR["pool_T%d" % _T] = (200, 200, 3, 2, 1, 1, True, _T)        # the AdainResBlk1d depthwise `pool`
# lstm: name -> (In, H, T)
LSTM = {"H256_T1": (640, 256, 1), "H256_T2": (640, 256, 2), "H256_T9": (640, 256, 9), "H256_T40": (640, 256, 40),
        "H96_T9": (96, 96, 9),      # three workgroups per direction: an odd block count
        "H32_T9": (32, 32, 9),
        "H48_T9": (48, 48, 9)}      # not a multiple of 32: only k_tts_lstm can run it
LN_WIDTHS = (64, 256, 257, 512, 768, 1090)
LN_EPS = (1e-5, 1e-12)
# ada_in_act: (T, C): both sides of the 16-row unroll, the 512-row chunk, and 9 chunks (the unrolled 8 plus one)
ADA_IN = [(T, Cn) for T in (1, 15, 16, 17, 511, 512, 513) for Cn in (1, 65)] + [(4441, 200)]
# attention: name -> (heads, T, q scale)
ATTN = {"h12_T1": (12, 1, 1.0), "h12_T3": (12, 3, 1.0), "h12_T257": (12, 257, 1.0), "h2_T255": (2, 255, 1.0), "h2_T256": (2, 256, 1.0), "h2_T510": (2, 510, 1.0),
        "h2_T256_spread": (2, 256, 20.0)}      # scores over +-60: part of every row underflows to 0


# ------------------------------------------------------------------ seeded inputs
@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    Ci, Co, K, stride, dil, pad, T = CONV[name]; r = _rng("conv." + name)
    x = r.standard_normal((T, Ci)).astype(np.float32)
    w = (r.uniform(-1, 1, (Co, Ci, K)) / np.sqrt(Ci * K)).astype(np.float32)
    b = r.standard_normal(Co).astype(np.float32)
    return x, w, b


@functools.lru_cache(maxsize=None)
def convtr_inputs(name):
    Ci, Co, K, stride, pad, out_pad, dw, T = CONVTR[name]; r = _rng("convtr." + name)
    x = r.standard_normal((T, Ci)).astype(np.float32)
    w = (r.uniform(-1, 1, (Ci, 1 if dw else Co, K)) / np.sqrt(1 if dw else Ci)).astype(np.float32)
    b = r.standard_normal(Co).astype(np.float32)
    return x, w, b


@functools.lru_cache(maxsize=None)
def lstm_inputs(name):
    In, H, T = LSTM[name]; r = _rng("lstm." + name); a = 1.0 / np.sqrt(H)      # uniform in +-1 / sqrt(H), torch's own initialisation: the gates do not saturate
    ws = []
    for _ in range(2):
        ws += [r.uniform(-a, a, (4 * H, In)).astype(np.float32), r.uniform(-a, a, (4 * H, H)).astype(np.float32), r.uniform(-a, a, 4 * H).astype(np.float32), r.uniform(-a, a, 4 * H).astype(np.float32)]
    return r.standard_normal((T, In)).astype(np.float32), tuple(ws)


def _norm_rows(r, n_rows, n):
    """rows (or channels) of a norm's input: unit normal, mean 100 with standard deviation 0.01 (f32 statistics fail there, the contract's f64 statistics do not), mixed scales"""
    x = r.standard_normal((n_rows, n))
    if n_rows > 1:
        x[1] = 100.0 + 0.01 * r.standard_normal(n)
    if n_rows > 2:
        x[2] *= np.exp(r.uniform(-6, 6, n))
    return x


@functools.lru_cache(maxsize=None)
def ln_inputs(Cn):
    r = _rng("ln.%d" % Cn)
    return _norm_rows(r, 3, Cn).astype(np.float32), r.standard_normal(Cn).astype(np.float32), r.standard_normal(Cn).astype(np.float32), (0.5 * r.standard_normal(2 * Cn)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ada_in_inputs(T, Cn):
    r = _rng("ada_in.%d.%d" % (T, Cn))
    x = _norm_rows(r, Cn + 1, T)[[1] + list(range(2, Cn + 1))] if Cn > 1 else _norm_rows(r, 2, T)[1:]      # channel 0: mean 100, standard deviation 0.01
    return np.ascontiguousarray(x.T).astype(np.float32), (0.5 * r.standard_normal(2 * Cn)).astype(np.float32), ("leaky02", "gelu")[(T + Cn) % 2]


@functools.lru_cache(maxsize=None)
def attn_inputs(name):
    heads, T, qs = ATTN[name]; r = _rng("attn." + name)
    return tuple((s * r.standard_normal((T, 64 * heads))).astype(np.float32) for s in (qs, 1.0, 1.0))


# ------------------------------------------------------------------ float64 references
def im2col(x, K, stride, dil, pad):
    T, Ci = x.shape; To = (T + 2 * pad - dil * (K - 1) - 1) // stride + 1
    cols = np.zeros((To, K * Ci), np.float64)
    for tap in range(K):
        tt = np.arange(To) * stride + tap * dil - pad; ok = (tt >= 0) & (tt < T)
        cols[ok, tap * Ci:(tap + 1) * Ci] = x[tt[ok]]
    return cols


def ref_conv(x, w, bias, stride, dil, pad):
    """-> (float64 result, sum |w||x| per output: the scale of the f32 chain's error bound)"""
    Co, Ci, K = w.shape; cols = im2col(x.astype(np.float64), K, stride, dil, pad)
    wm = w.astype(np.float64).transpose(2, 1, 0).reshape(K * Ci, Co)      # k = tap * Ci + ci
    y = cols @ wm; mag = np.abs(cols) @ np.abs(wm)
    if bias is not None:
        y = y + bias.astype(np.float64); mag = mag + np.abs(bias.astype(np.float64))
    return y, mag


def ref_convtr(x, w, bias, stride, pad, out_pad, depthwise):
    T, Ci = x.shape; K = w.shape[2]; Co = Ci if depthwise else w.shape[1]; To = (T - 1) * stride - 2 * pad + K + out_pad
    y = np.zeros((To, Co)); mag = np.zeros((To, Co)); xd, wd = x.astype(np.float64), w.astype(np.float64)
    for tap in range(K):
        u = np.arange(T) * stride + tap - pad; ok = (u >= 0) & (u < To)
        if depthwise:
            y[u[ok]] += xd[ok] * wd[:, 0, tap]; mag[u[ok]] += np.abs(xd[ok] * wd[:, 0, tap])
        else:
            y[u[ok]] += xd[ok] @ wd[:, :, tap]; mag[u[ok]] += np.abs(xd[ok]) @ np.abs(wd[:, :, tap])
    if bias is not None:
        y = y + bias.astype(np.float64); mag = mag + np.abs(bias.astype(np.float64))
    return y, mag


def ref_norm(x, axis, eps):
    """two-pass mean / variance in float64"""
    xd = x.astype(np.float64); m = xd.mean(axis=axis, keepdims=True); v = ((xd - m) ** 2).mean(axis=axis, keepdims=True)
    return (xd - m) / np.sqrt(v + float(np.float32(eps)))


def ref_act(v, act):
    if act == "gelu":
        return 0.5 * v * (1.0 + np.tanh(0.79788456080286535588 * (v + float(np.float32(0.044715)) * v ** 3)))
    return np.where(v > 0, v, v * float(np.float32({"leaky02": 0.2, "leaky01": 0.1, "leaky001": 0.01}[act])))


def ref_layernorm(x, gamma, beta, eps):
    return ref_norm(x, 1, eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def ref_ada(x, gb, axis):
    Cn = x.shape[1]; g = gb.astype(np.float64)
    return ref_norm(x, axis, 1e-5) * (1.0 + g[:Cn]) + g[Cn:]


def ref_attention(q, k, v, heads):
    T = q.shape[0]; out = np.zeros((T, 64 * heads))
    for h in range(heads):
        sl = slice(64 * h, 64 * h + 64); s = (q[:, sl].astype(np.float64) @ k[:, sl].astype(np.float64).T) * 0.125
        p = np.exp(s - s.max(axis=1, keepdims=True)); p /= p.sum(axis=1, keepdims=True)
        out[:, sl] = p @ v[:, sl].astype(np.float64)
    return out


def ref_lstm_bi(x, ws):
    T = x.shape[0]; H = ws[1].shape[1]; out = np.zeros((T, 2 * H)); sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    for d in range(2):
        wih, whh, bih, bhh = (a.astype(np.float64) for a in ws[4 * d:4 * d + 4]); h = np.zeros(H); c = np.zeros(H)
        for s in range(T):
            t = T - 1 - s if d else s
            a = wih @ x[t].astype(np.float64) + bih + whh @ h + bhh
            c = sig(a[H:2 * H]) * c + sig(a[:H]) * np.tanh(a[2 * H:3 * H]); h = sig(a[3 * H:]) * np.tanh(c)
            out[t, d * H:(d + 1) * H] = h
    return out


# ------------------------------------------------------------------ the checker's result per case, computed once
@functools.lru_cache(maxsize=None)
def checker(op, key, *extra):
    o = checker_ops()
    if op == "conv":
        x, w, b = conv_inputs(key); Ci, Co, K, stride, dil, pad, T = CONV[key]
        return o.conv(x, w, b if extra[0] else None, stride, dil, pad)
    if op == "convtr":
        x, w, b = convtr_inputs(key); Ci, Co, K, stride, pad, out_pad, dw, T = CONVTR[key]
        return o.convtr(x, w, b if extra[0] else None, stride, pad, out_pad, dw)
    if op == "lstm":
        x, ws = lstm_inputs(key)
        return o.lstm_bi(x, ws)
    if op == "layernorm":
        x, g, b, gb = ln_inputs(key)
        return o.layernorm(x, g, b, extra[0])
    if op == "ada_ln":
        x, g, b, gb = ln_inputs(key)
        return o.ada_ln(x, gb)
    if op == "ada_in_act":
        x, gb, act = ada_in_inputs(*key)
        return o.ada_in_act(x, gb, act)
    if op == "attention":
        q, k, v = attn_inputs(key)
        return o.attention(q, k, v, ATTN[key][0])
    raise KeyError(op)


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ which edges a conv case reaches under a tile (computed from the shapes)
def conv_edges(name, mt, nt):
    Ci, Co, K, stride, dil, pad, T = CONV[name]
    To = (T + 2 * pad - dil * (K - 1) - 1) // stride + 1; Ktot = K * Ci; nk4 = (Ktot + 3) // 4; Co16 = (Co + 15) // 16 * 16
    # a 32-wide slab of k holds a tap boundary that is not its own edge: the gather's tap / ci split changes inside the slab
    straddle = any((tap * Ci) % 32 != 0 and tap * Ci < Ktot for tap in range(1, K))
    return {"ragged_rows": To % (16 * nt) != 0, "ragged_kgroups": nk4 % 8 != 0, "ragged_k": Ktot % 4 != 0, "tap_straddles_slab": straddle,
            "dead_second_mtile": mt == 2 and Co16 % 32 != 0, "scalar_stores": Co % 4 != 0}


# ------------------------------------------------------------------ the fixture utterances of the production-width test (kokoro82m, speaker 50)
FIXTURES = {"three": ([0, 20, 0], 3.0), "nine": ([0, 14, 4, 18, 17, 52, 54, 1, 0], 2.0)}

# checker vs float64, worst over the table, as measured by tests/test_cpu_kokoro_ops.py (profiles/kokoro_ops/README.md): max |got - ref| / max |ref| per case.
# The tests assert 4 x these: the margin covers other seeds of the same distribution; the GPU kernels are not in that loop (they are held to the checker bit for bit).
MEASURED = {"layernorm": 1.25e-4, "ada_ln": 1.07e-4, "ada_in_act": 1.97e-4, "attention": 3.92e-6, "lstm": 1.51e-6}
