"""Per-clip audio context (skw_full_params.audio_ctx), the checker's side.

The oracle has no audio_ctx parameter and needs none: it uses hparams.n_audio_ctx only for tensor extents and for the precision behind max_initial_ts, and its window
logic runs on WHISPER_CHUNK_SIZE.  So the engine with audio_ctx = K on a model file M must equal, bit for bit in the exact precision, the oracle on M'(K):
M with hparams.n_audio_ctx rewritten to K and encoder.positional_embedding cut to its first K rows (a prefix of the tensor's data).  The oracle is then handed
max_initial_ts x n_audio_ctx / K, so that both sides ban the same timestamp ids (the engine keeps the model's 0.02 s precision).
"""
import math
import os
import struct

import numpy as np

from ggml_reader import _BLOCK

WHISPER_CHUNK_SIZE = 30


def write_audio_ctx_model(src, dst, K):
    """M'(K): `src` with hparams.n_audio_ctx = K and the encoder's positional embedding cut to its first K rows.  Every other byte is copied.  Returns n_audio_ctx of src."""
    f = open(src, "rb"); o = open(dst, "wb")
    o.write(f.read(4))
    hp = list(struct.unpack("<11i", f.read(44))); nc = hp[1]
    assert 1 <= K <= nc, (K, nc)
    hp[1] = K; o.write(struct.pack("<11i", *hp))
    n_mel, n_fft = struct.unpack("<2i", f.read(8)); o.write(struct.pack("<2i", n_mel, n_fft)); o.write(f.read(4 * n_mel * n_fft))
    nv, = struct.unpack("<i", f.read(4)); o.write(struct.pack("<i", nv))
    for _ in range(nv):
        ln, = struct.unpack("<I", f.read(4)); o.write(struct.pack("<I", ln)); o.write(f.read(ln))
    cut = 0
    while True:
        h = f.read(12)
        if len(h) < 12:
            break
        nd, ln, tt = struct.unpack("<3i", h)
        ne = list(struct.unpack("<%di" % nd, f.read(4 * nd))); name = f.read(ln); cnt = int(np.prod(ne))
        raw = f.read(cnt // 32 * _BLOCK[tt]) if tt in _BLOCK else f.read(cnt * (4 if tt == 0 else 2))
        if name == b"encoder.positional_embedding":
            assert tt in (0, 1) and nd == 2 and ne[1] == nc, (tt, ne)      # [n_audio_ctx][n_state], ne[0] = n_state runs fastest: the first K rows are a prefix
            ne[1] = K; raw = raw[:K * ne[0] * (4 if tt == 0 else 2)]; cut += 1
        o.write(struct.pack("<3i", nd, ln, tt)); o.write(struct.pack("<%di" % nd, *ne)); o.write(name); o.write(raw)
    o.close()
    assert cut == 1, "encoder.positional_embedding not found"
    return nc


def audio_ctx_model(src, K):
    """path of M'(K) for the model file `src` (written once beside it)"""
    dst = src[:-4] + "_actx%d.bin" % K
    if not os.path.exists(dst):
        write_audio_ctx_model(src, dst + ".tmp", K)
        os.replace(dst + ".tmp", dst)
    return dst


def tid0(max_initial_ts, n_audio_ctx):
    """the last timestamp id a window's first token may take (whisper_process_logits): round(max_initial_ts / (30 / n_audio_ctx)) in f32, as both implementations compute it"""
    precision = np.float32(WHISPER_CHUNK_SIZE) / np.float32(n_audio_ctx)
    q = np.float32(max_initial_ts) / precision
    return int(math.floor(float(q) + 0.5)) if q >= 0 else -int(math.floor(-float(q) + 0.5))      # roundf: halves away from zero


def scaled_max_initial_ts(max_initial_ts, n_audio_ctx, K):
    """what the oracle on M'(K) is given so that it bans the timestamp ids the engine bans on M with audio_ctx = K; asserts the two integers agree"""
    scaled = float(np.float32(max_initial_ts) * np.float32(n_audio_ctx) / np.float32(K))
    if max_initial_ts > 0:
        a, b = tid0(max_initial_ts, n_audio_ctx), tid0(scaled, K)
        assert a == b, "max_initial_ts %g: the engine bans ids above %d, the oracle on M'(%d) above %d" % (max_initial_ts, a, K, b)
    return scaled
