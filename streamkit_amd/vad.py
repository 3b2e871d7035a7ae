"""ctypes binding of the Silero VAD gate (include/skw_vad.h, include/skw_vad_batch.h).

CpuVad: libskw_vad.so, one stream, in the libm arithmetic (the plugin's default gate) or in the contract arithmetic of
include/skw_silero_net.h.  GpuVad: the HIP kernels of libskw_engine.so, contract arithmetic, many streams per call.  Both carry a
stream's state as the same 320 floats (context[64], h[128], c[128]), so a stream may move between them at any frame.
There is no fallback: GpuVad without the compiled library or without a HIP device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CPU_LIB_PATH = os.path.join(_HERE, "libskw_vad.so")
ARITH_LIBM, ARITH_CONTRACT = 0, 1
STATE_FLOATS = 320
TAP_SHAPES = (("mag", 516), ("c1", 512), ("c2", 128), ("c3", 64), ("c4", 128), ("gin", 512))
_CPU = None
_GPU = None


def cpu_lib():
    global _CPU
    if _CPU is None:
        L = C.CDLL(CPU_LIB_PATH)
        L.skw_vad_create_ex.restype = C.c_void_p
        L.skw_vad_create_ex.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
        L.skw_vad_process_chunk.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.skw_vad_process_chunks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.skw_vad_reset.argtypes = [C.c_void_p]
        L.skw_vad_get_state_ex.argtypes = [C.c_void_p, C.c_void_p]
        L.skw_vad_set_state_ex.argtypes = [C.c_void_p, C.c_void_p]
        L.skw_vad_debug_feed_forward.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        L.skw_vad_free.argtypes = [C.c_void_p]
        _CPU = L
    return _CPU


def gpu_lib():
    global _GPU
    if _GPU is None:
        from . import engine
        L = engine.lib()
        L.skw_vad_gpu_create.restype = C.c_void_p
        L.skw_vad_gpu_create.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
        L.skw_vad_gpu_process.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_vad_gpu_last_error.restype = C.c_char_p
        L.skw_vad_gpu_last_error.argtypes = [C.c_void_p]
        L.skw_vad_gpu_last_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.skw_vad_gpu_free.argtypes = [C.c_void_p]
        L.skw_vad_gpu_debug_feed_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.skw_vad_gpu_debug_alloc_poison.argtypes = [C.c_int]
        _GPU = L
    return _GPU


def _frames(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    if a.size % 512:
        raise ValueError("frames must be a multiple of 512 samples")
    return a


class CpuVad:
    """One stream on the CPU.  arithmetic: ARITH_LIBM (what skw_vad_create gives) or ARITH_CONTRACT."""

    def __init__(self, path, arithmetic=ARITH_CONTRACT):
        err = C.create_string_buffer(512)
        self._h = cpu_lib().skw_vad_create_ex(os.fsencode(path), arithmetic, err, 512)
        if not self._h:
            raise RuntimeError(err.value.decode(errors="replace"))

    def process_chunk(self, frame):
        f = _frames(frame)
        assert f.size == 512
        p = C.c_float()
        assert cpu_lib().skw_vad_process_chunk(self._h, f.ctypes.data, C.byref(p)) == 0
        return np.float32(p.value)

    def process_chunks(self, frames):
        f = _frames(frames)
        out = np.zeros(f.size // 512, np.float32)
        assert cpu_lib().skw_vad_process_chunks(self._h, f.ctypes.data, out.size, out.ctypes.data) == 0
        return out

    def get_state(self):
        s = np.zeros(STATE_FLOATS, np.float32)
        cpu_lib().skw_vad_get_state_ex(self._h, s.ctypes.data)
        return s

    def set_state(self, s):
        s = np.ascontiguousarray(s, np.float32)
        assert s.size == STATE_FLOATS
        cpu_lib().skw_vad_set_state_ex(self._h, s.ctypes.data)

    def reset(self):
        cpu_lib().skw_vad_reset(self._h)

    def feed_forward_taps(self, frame):
        """Contract arithmetic, from the carried context, state untouched: dict of the six stages of TAP_SHAPES."""
        f = _frames(frame)
        assert f.size == 512
        out = {k: np.zeros(n, np.float32) for k, n in TAP_SHAPES}
        assert cpu_lib().skw_vad_debug_feed_forward(self._h, f.ctypes.data, *[out[k].ctypes.data for k, _ in TAP_SHAPES]) == 0
        return out

    def close(self):
        if self._h:
            cpu_lib().skw_vad_free(self._h)
            self._h = None

    __del__ = close


class GpuVad:
    """The gate on one GPU device; process() takes any number of streams and is safe to call from many threads."""

    def __init__(self, path, device=0):
        err = C.create_string_buffer(512)
        self._h = gpu_lib().skw_vad_gpu_create(os.fsencode(path), device, err, 512)
        if not self._h:
            raise RuntimeError(err.value.decode(errors="replace"))

    def process(self, frames, states):
        """frames: one array of n_s * 512 samples per stream (n_s may be 0); states: one 320-float array per stream, updated in place.
        Returns the list of probability arrays."""
        S = len(frames)
        fr = [_frames(f) for f in frames]
        for s in states:
            assert s.dtype == np.float32 and s.size == STATE_FLOATS and s.flags.c_contiguous
        n = np.array([f.size // 512 for f in fr], np.int32)
        probs = [np.zeros(int(k), np.float32) for k in n]
        fp = (C.c_void_p * S)(*[f.ctypes.data if f.size else None for f in fr])
        sp = (C.c_void_p * S)(*[s.ctypes.data for s in states])
        pp = (C.c_void_p * S)(*[p.ctypes.data if p.size else None for p in probs])
        if gpu_lib().skw_vad_gpu_process(self._h, S, fp, n.ctypes.data, sp, pp) != 0:
            raise RuntimeError(gpu_lib().skw_vad_gpu_last_error(self._h).decode(errors="replace"))
        return probs

    def last_timing(self):
        """(host-to-device, kernels, device-to-host) milliseconds of the last process() call, by device events."""
        t = np.zeros(3, np.float32)
        gpu_lib().skw_vad_gpu_last_timing(self._h, t.ctypes.data)
        return tuple(float(x) for x in t)

    def feed_forward_taps(self, frames, state):
        f = _frames(frames)
        n = f.size // 512
        st = np.ascontiguousarray(state, np.float32)
        out = {k: np.zeros((n, m), np.float32) for k, m in TAP_SHAPES}
        if gpu_lib().skw_vad_gpu_debug_feed_forward(self._h, f.ctypes.data, n, st.ctypes.data, *[out[k].ctypes.data for k, _ in TAP_SHAPES]) != 0:
            raise RuntimeError(gpu_lib().skw_vad_gpu_last_error(self._h).decode(errors="replace"))
        return out

    def close(self):
        if self._h:
            gpu_lib().skw_vad_gpu_free(self._h)
            self._h = None

    __del__ = close


def set_alloc_poison(on):
    """Tests: every work buffer of every GpuVad starts each call as NaNs."""
    gpu_lib().skw_vad_gpu_debug_alloc_poison(1 if on else 0)
