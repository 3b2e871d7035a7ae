"""ctypes binding of libskw_tts.so (include/skw_tts.h: the calls a Rust host binds in place of sherpa-onnx's, kokoro/src/ffi.rs:119-137) and the seeded Kokoro model
directory tools/make_synth_kokoro.py writes.  Product-side access only: the CPU checkers live under tests/ and oracle/."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, STYLE, MAX_TOKENS, MAX_FRAMES = 11, 128, 510, 3000


def synth_kokoro_dir(size="micro", seed=1234):
    path = "/tmp/skw_kokoro_%s_%d" % (size, seed)
    if not os.path.exists(os.path.join(path, "voices.bin")):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_synth_kokoro.py"), path + ".tmp", "--seed", str(seed), "--size", size])
        if os.path.exists(path):
            import shutil; shutil.rmtree(path)
        os.replace(path + ".tmp", path)
    return path


class _Cfg(C.Structure):
    _fields_ = [("model", C.c_char_p), ("voices", C.c_char_p), ("tokens", C.c_char_p), ("lexicon", C.c_char_p), ("length_scale", C.c_float), ("gpu_device", C.c_int32)]


class _Audio(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_float)), ("n", C.c_int32), ("sample_rate", C.c_int32)]


def tts_lib():
    L = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libskw_tts.so"))
    L.skw_tts_create.restype = C.c_void_p; L.skw_tts_create.argtypes = [C.POINTER(_Cfg), C.c_char_p, C.c_size_t]
    L.skw_tts_destroy.argtypes = [C.c_void_p]
    L.skw_tts_generate.restype = C.POINTER(_Audio); L.skw_tts_generate.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_float]
    L.skw_tts_destroy_audio.argtypes = [C.POINTER(_Audio)]
    L.skw_tts_last_error.restype = C.c_char_p; L.skw_tts_last_error.argtypes = [C.c_void_p]
    L.skw_tts_num_speakers.argtypes = [C.c_void_p]; L.skw_tts_sample_rate.argtypes = [C.c_void_p]
    L.skw_tts_tokenize.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32]
    L.skw_tts_debug_get.restype = C.c_long; L.skw_tts_debug_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
    L.skw_tts_last_ms.restype = C.c_float; L.skw_tts_last_ms.argtypes = [C.c_void_p]
    L.skw_tts_generate_ids.restype = C.POINTER(_Audio); L.skw_tts_generate_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float]
    L.skw_tts_debug_enable.argtypes = [C.c_void_p, C.c_int]; L.skw_tts_debug_conv_mode.argtypes = [C.c_int]; L.skw_tts_debug_lstm_mode.argtypes = [C.c_int]
    L.skw_tts_debug_conv_tile.argtypes = [C.c_int, C.c_int]; L.skw_tts_debug_launch_counts.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.skw_tts_debug_lstm_epoch.argtypes = [C.c_void_p, C.c_uint]; L.skw_tts_debug_lstm_epoch_get.argtypes = [C.c_void_p]; L.skw_tts_debug_lstm_epoch_get.restype = C.c_uint
    L.skw_tts_debug_lstm_error.argtypes = [C.c_void_p]
    return L


COUNTERS = ("conv", "t12", "t14", "t18", "t28", "convtr_direct", "convtr_phased", "convtr_phase_launches", "lstm", "lstm_mw", "lstm_mw_max_wg")
TILES = {(1, 2): "t12", (1, 4): "t14", (1, 8): "t18", (2, 8): "t28"}
ACTS = {"leaky02": 0, "leaky01": 1, "leaky001": 2, "gelu": 3}


def launch_counts(L, reset=False):
    """skw_tts_debug_launch_counts as a dict keyed by COUNTERS"""
    v = (C.c_long * len(COUNTERS))()
    n = L.skw_tts_debug_launch_counts(v, len(COUNTERS), 1 if reset else 0)
    assert n == len(COUNTERS), n
    return dict(zip(COUNTERS, [int(x) for x in v]))


class KokoroOps:
    """One Kokoro operator at a time, from numpy arrays (include/skw_kokoro_ops.h): the product's skw_tts_debug_op_* (prefix, an engine handle) and the checker's skwo_kokoro_op_*
    (its own prefix, no handle) have the same seven signatures.  Activations are [T][C] float32."""

    def __init__(self, lib, prefix, handle=None):
        self.h = handle; P, F, I, L_ = C.c_void_p, C.c_float, C.c_int, C.c_long
        sig = {"conv": [P, P, I, I, P, I, I, P, I, I, I, P, L_], "convtr": [P, P, I, P, I, I, I, P, I, I, I, I, P, L_], "layernorm": [P, P, I, I, P, P, F, P, L_],
               "ada_ln": [P, P, I, I, P, P, L_], "ada_in_act": [P, P, I, I, P, I, P, L_], "attention": [P, P, P, P, I, I, P, L_], "lstm_bi": [P, P, I, I, I, P, P, L_]}
        self.f = {}
        for name, args in sig.items():
            f = getattr(lib, prefix + name); f.restype = L_; f.argtypes = args; self.f[name] = f

    @staticmethod
    def _a(x):
        return None if x is None else np.ascontiguousarray(x, np.float32)

    def _run(self, name, n_out, shape, *args):
        out = np.full(n_out, np.nan, np.float32); keep = [self._a(a) if isinstance(a, np.ndarray) else a for a in args]
        n = self.f[name](self.h, *[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep], out.ctypes.data, out.size)
        if n != n_out:
            raise RuntimeError("%s: returned %d, expected %d elements" % (name, n, n_out))
        return out.reshape(shape)

    def conv(self, x, w, bias, stride=1, dil=1, pad=0):
        (T, Ci), (Co, Ci2, K) = x.shape, w.shape; assert Ci == Ci2
        To = (T + 2 * pad - dil * (K - 1) - 1) // stride + 1
        return self._run("conv", To * Co, (To, Co), self._a(x), T, Ci, self._a(w), Co, K, self._a(bias), stride, dil, pad)

    def convtr(self, x, w, bias, stride, pad, out_pad=0, depthwise=False):
        T, Ci = x.shape; K = w.shape[2]; Co = Ci if depthwise else w.shape[1]; assert w.shape[0] == Ci
        To = (T - 1) * stride - 2 * pad + K + out_pad
        return self._run("convtr", To * Co, (To, Co), self._a(x), T, self._a(w), Ci, Co, K, self._a(bias), stride, pad, out_pad, 1 if depthwise else 0)

    def layernorm(self, x, gamma, beta, eps):
        T, Cn = x.shape
        return self._run("layernorm", T * Cn, (T, Cn), self._a(x), T, Cn, self._a(gamma), self._a(beta), float(eps))

    def ada_ln(self, x, gb):
        T, Cn = x.shape; assert gb.size == 2 * Cn
        return self._run("ada_ln", T * Cn, (T, Cn), self._a(x), T, Cn, self._a(gb))

    def ada_in_act(self, x, gb, act):
        T, Cn = x.shape; assert gb.size == 2 * Cn
        return self._run("ada_in_act", T * Cn, (T, Cn), self._a(x), T, Cn, self._a(gb), ACTS[act])

    def attention(self, q, k, v, heads):
        T, Cn = q.shape; assert Cn == 64 * heads and k.shape == q.shape == v.shape
        return self._run("attention", T * Cn, (T, Cn), self._a(q), self._a(k), self._a(v), T, heads)

    def lstm_bi(self, x, ws):
        """ws: 8 arrays, per direction weight_ih [4H][In], weight_hh [4H][H], bias_ih [4H], bias_hh [4H]"""
        T, In = x.shape; H = ws[1].shape[1]; keep = [self._a(w) for w in ws]
        ptrs = (C.c_void_p * 8)(*[w.ctypes.data for w in keep])
        return self._run("lstm_bi", T * 2 * H, (T, 2 * H), self._a(x), T, In, H, ptrs)


class Tts:
    """The product: libskw_tts.so through its C ABI (the calls a Rust host binds in place of sherpa-onnx's)."""

    def __init__(self, model_dir, device=0):
        self.L = tts_lib()
        d = model_dir
        cfg = _Cfg((d + "/model.onnx").encode(), (d + "/voices.bin").encode(), (d + "/tokens.txt").encode(), (d + "/lexicon-us-en.txt," + d + "/lexicon-zh.txt").encode(), 1.0, device)
        err = C.create_string_buffer(512)
        self.h = self.L.skw_tts_create(C.byref(cfg), err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())

    def tokenize(self, text):
        ids = np.zeros(MAX_TOKENS, np.int32)
        n = self.L.skw_tts_tokenize(self.h, text.encode(), ids.ctypes.data, ids.size)
        return ids[:n].copy()

    def generate(self, text, sid=0, speed=1.0, ids=None):
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            a = self.L.skw_tts_generate_ids(self.h, ids.ctypes.data, ids.size, sid, speed)
        else:
            a = self.L.skw_tts_generate(self.h, text.encode(), sid, speed)
        if not a:
            raise RuntimeError(self.L.skw_tts_last_error(self.h).decode())
        y = np.ctypeslib.as_array(a.contents.samples, shape=(a.contents.n,)).copy(); rate = a.contents.sample_rate
        self.L.skw_tts_destroy_audio(a)
        return y, rate

    def taps(self, on=True):
        self.L.skw_tts_debug_enable(self.h, 1 if on else 0)

    def tap(self, what):
        n = self.L.skw_tts_debug_get(self.h, what, None, 0)
        out = np.zeros(n, np.float32); self.L.skw_tts_debug_get(self.h, what, out.ctypes.data, n)
        return out

    def ops(self):
        """the product's operator hooks on this engine's stream and arena"""
        return KokoroOps(self.L, "skw_tts_debug_op_", self.h)

    def last_ms(self):
        return self.L.skw_tts_last_ms(self.h)

    def close(self):
        if self.h:
            self.L.skw_tts_destroy(self.h); self.h = None
