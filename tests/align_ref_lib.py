"""Word-timestamp contract (include/skw_align.h): the driver's record format (tests/cpp/align_main.cpp), seeded inputs, numpy / torch-double restatements of the steps, and the
loader of tests/golden/align_cases.json.  Shared by tests/test_cpu_align.py, tests/test_gpu_align_kernels.py and tests/golden/make_align_goldens.py; computes nothing on import."""
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "align_cases.json")
_EXE = {}


# ---- the driver ----
def driver(tmp_path_factory, sanitize=False):
    if sanitize not in _EXE:
        exe = tmp_path_factory.mktemp("align") / ("align_san" if sanitize else "align")
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-misleading-indentation", "-ffp-contract=off"] + flags +
                              ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "streamkit_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "align_main.cpp")])
        _EXE[sanitize] = str(exe)
    return _EXE[sanitize]


def run(exe, records):
    """records: int32 arrays (kind first) -> one int32 array per record"""
    blob = np.concatenate([np.array([len(records)], np.int32)] + [np.ascontiguousarray(r, dtype=np.int32).ravel() for r in records]).tobytes()
    out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-2000:]
    w = np.frombuffer(out.stdout, np.int32)
    res, k = [], 0
    for _ in records:
        n = int(w[k]); res.append(w[k + 1:k + 1 + n]); k += 1 + n
    assert k == w.size
    return res


def _i(*v):
    return np.array(v, np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).ravel()


def rec_dtw(x, seek_cs=0):
    return np.concatenate([_i(0, x.shape[0], x.shape[1], seek_cs), bits(x)])


def parse_dtw(o, N):
    n = int(o[0])
    return dict(path_i=o[1:1 + n], path_j=o[1 + n:1 + 2 * n], jump=o[1 + 2 * n:1 + 2 * n + N], t0=o[1 + 2 * n + N:1 + 2 * n + 2 * N], t1=o[1 + 2 * n + 2 * N:1 + 2 * n + 3 * N])


def rec_reduce(P, Kw, width=7, split=None):
    H, N, K = P.shape
    return np.concatenate([_i(1, H, H if split is None else split, N, K, Kw, width), bits(P)])


def rec_words(toks, t_eot):
    """toks: [(bytes, t0)]"""
    return np.concatenate([_i(2, len(toks), t_eot)] + [np.concatenate([_i(t0, len(b)), np.frombuffer(b, np.uint8).astype(np.int32)]) for b, t0 in toks])


def rec_words2(toks):
    """toks: [(bytes, t0, t1, first)] — the node's call of the word rule"""
    return np.concatenate([_i(8, len(toks))] + [np.concatenate([_i(t0, t1, int(first), len(b)), np.frombuffer(b, np.uint8).astype(np.int32)]) for b, t0, t1, first in toks])


def parse_words(o):
    out, k = [], 1
    for _ in range(int(o[0])):
        n = int(o[k + 4])
        out.append((int(o[k]), int(o[k + 1]), int(o[k + 2]), int(o[k + 3]), bytes(o[k + 5:k + 5 + n].astype(np.uint8))))
        k += 5 + n
    assert k == o.size
    return out


def rec_params(n_layer, n_head, clip, enabled, width, mask):
    m = np.zeros(32, np.uint32); m[:len(mask)] = mask
    return np.concatenate([_i(3, n_layer, n_head, clip, enabled, width), m.view(np.int32)])


def parse_params(o):
    return int(o[0]), bytes(o[2:2 + int(o[1])].astype(np.uint8)).decode()


def rec_weights(q, K):
    """q [rows][64], K [n_keys][64] float16"""
    return np.concatenate([_i(4, q.shape[0], K.shape[0]), q.view(np.uint16).astype(np.int32).ravel(), K.view(np.uint16).astype(np.int32).ravel()])


def rec_median(z, width=7):
    return np.concatenate([_i(7, z.shape[0], z.shape[1], width), bits(z)])


# ---- seeded inputs ----
def dtw_matrix(seed, N, K, kind):
    """grid: multiples of 1/1024 with |x| <= 8 (every DTW sum of a path is exact in f32; odd seeds use multiples of 1/8, so ties are everywhere); normal: ordinary f32 values
    of no special form — a sum of three uniform 24-bit integers scaled to (-3, 3), bell-shaped.  Integer draws and exact float64 arithmetic only: the fixture pins these inputs by
    a digest, so nothing here may depend on a libm"""
    rng = np.random.default_rng(seed)
    if kind == "grid":
        return (rng.integers(-8, 9, size=(N, K)) * 128 / 1024 if seed % 2 else rng.integers(-8 * 1024, 8 * 1024 + 1, size=(N, K)) / 1024).astype(np.float32)
    return ((rng.integers(0, 1 << 24, size=(N, K)) + rng.integers(0, 1 << 24, size=(N, K)) + rng.integers(0, 1 << 24, size=(N, K))) / float(1 << 23) - 3.0).astype(np.float32)


def weights_like(seed, H, N, K, zero_var_col=None):
    """attention-like rows: softmax of scaled normals over K keys, f32"""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((H, N, K)) * 2.0
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    P = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    if zero_var_col is not None:
        P[:, :, zero_var_col] = P[:, :1, zero_var_col]
    return P


def weights_exact(seed, H, N, K):
    """positive f32 weights from integer draws alone (k / 2^26, k < 2^20): the inputs the fixture pins by a digest"""
    return (np.random.default_rng(seed).integers(1, 1 << 20, size=(H, N, K)) / float(1 << 26)).astype(np.float32)


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


# ---- restatements ----
def dtw_f32(x):
    """transformers' _dynamic_time_warping with every add in f32 -> (text_indices, time_indices)"""
    N, K = x.shape
    cost = np.full((N + 1, K + 1), np.inf, np.float32); trace = np.zeros((N + 1, K + 1), np.int8)
    cost[0, 0] = 0
    for j in range(1, K + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1]) + c
            trace[i, j] = t
    trace[0, :] = 2; trace[:, 0] = 1
    i, j, ti, tj = N, K, [], []
    while i > 0 or j > 0:
        ti.append(i - 1); tj.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1; j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti[::-1]), np.array(tj[::-1])


def jumps(ti, tj):
    return tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)]


def moves(ti, tj):
    """a path as a string: the step into each point after the first (d, u: row + 1, l: key + 1)"""
    return "".join("d" if a and b else ("u" if a else "l") for a, b in zip(np.diff(ti), np.diff(tj)))


def steps345_double(P, Kw, width=7):
    """steps 2-5 with torch in double, rounded where the contract rounds: z to f32 after the normalisation, the head mean to f32 -> f32 [N][Kw]"""
    import torch
    import torch.nn.functional as F
    w = torch.from_numpy(np.ascontiguousarray(P[:, :, :Kw])).double()
    mean = w.mean(dim=-2, keepdim=True)
    var = ((w - mean) ** 2).mean(dim=-2, keepdim=True)
    z = torch.where(var == 0, torch.zeros_like(w), (w - mean) / var.sqrt()).float()
    half = width // 2
    if Kw > half:
        z = F.pad(z, (half, half, 0, 0), mode="reflect").unfold(-1, width, 1).sort()[0][..., half]
    return (-(z.double().mean(dim=0).float())).numpy()


def softmax_f64(q, K):
    """q [rows][64], K [n_keys][64] float16 -> float64 [rows][n_keys]"""
    s = q.astype(np.float64) @ K.astype(np.float64).T
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


EPS = 2.0 ** -24       # half an f32 ulp, relative
QK_ABS = 2.0 ** -124   # skw_expf returns 0 below -86 (e^-86 = 4.5e-38 < 2^-124): what a weight may lose to that cut, absolutely


def qk_bound(n_keys, smax):
    """Step 1 against softmax in float64: |P - ref| <= rel * ref + QK_ABS, rel derived from the chain, not fitted.  smax = max over (row, key) of sum_c |q_c k_c|.
    A score is 64 f32 fmas, each rounding at most eps times the running magnitude (<= smax): |ds| <= 64 eps smax; s - m carries that error at both ends and one more rounding
    (<= eps * 2 smax).  An error d in an exponent multiplies the exponential by e^d; numerator and denominator (a weighted mean of such factors) each move by at most that.
    skw_expf is Cephes' expf (its reduction and polynomial), documented peak relative error 1.7e-7 < 4 eps, again in numerator and denominator; the f64 sum of n_keys terms and
    the division add n_keys * 2^-52; the final rounding to f32 eps.  Factors (1 + a)(1 + b) <= e^(a + b)."""
    ds = 2 * 64 * EPS * smax + 2 * EPS * smax
    return float(np.expm1(2 * ds + 8 * EPS + n_keys * 2.0 ** -52 + EPS))


def ulp_diff(a, b):
    """distance in f32 representable values (monotone integer image of the floats)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)
