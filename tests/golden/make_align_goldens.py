"""Writes tests/golden/align_cases.json: seeded inputs (regenerated from their seeds by tests/align_ref_lib.py, pinned here by a digest) with what transformers' own
functions give for them — _dynamic_time_warping's path, _median_filter's output, and the normalise / filter / head-mean of _extract_token_timestamps (f32, as transformers runs
it).  Run once where transformers is installed:  python tests/golden/make_align_goldens.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import align_ref_lib as al  # noqa: E402
import transformers  # noqa: E402
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter  # noqa: E402


def main():
    rng = np.random.default_rng(20240607)
    dtw = []
    shapes = [(1, 1), (1, 7), (2, 1), (5, 1), (3, 2), (7, 7), (40, 120), (40, 3), (17, 63)]
    for n in range(60):
        N, K = shapes[n] if n < len(shapes) else (int(rng.integers(1, 41)), int(rng.integers(1, 121)))
        kind = "grid" if n % 2 == 0 or n < 4 else "normal"
        seed = 9000 + n
        x = al.dtw_matrix(seed, N, K, kind)
        ti, tj = _dynamic_time_warping(x.astype(np.float64))            # as _extract_token_timestamps calls it: a double matrix, f32 cost table
        fi, fj = al.dtw_f32(x)
        assert np.array_equal(ti, fi) and np.array_equal(tj, fj), ("the pure-f32 restatement leaves transformers' path", n)
        dtw.append(dict(seed=seed, N=N, K=K, kind=kind, digest=al.digest(x), moves=al.moves(ti, tj), jumps=[int(v) for v in al.jumps(ti, tj)]))
    med = []
    for n, (N, K) in enumerate([(2, 1), (3, 3), (3, 4), (4, 7), (5, 8), (6, 33), (9, 120)]):
        seed = 9500 + n
        z = al.dtw_matrix(seed, N, K, "normal" if n % 2 else "grid")
        out = _median_filter(torch.from_numpy(z)[None, None], 7)[0, 0].numpy()
        med.append(dict(seed=seed, N=N, K=K, kind="normal" if n % 2 else "grid", digest=al.digest(z), out_bits=[int(v) for v in out.view(np.int32).ravel()]))
    norm = []
    for n, (H, N, K) in enumerate([(1, 2, 4), (2, 5, 9), (6, 7, 3), (3, 12, 16)]):
        seed = 9700 + n
        w = torch.from_numpy(al.weights_exact(seed, H, N, K))[None]      # (batch, heads, tokens, keys), the lines of _extract_token_timestamps
        std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
        mean = torch.mean(w, dim=-2, keepdim=True)
        assert bool((std > 0).all())
        m = _median_filter((w - mean) / std, 7).mean(dim=1)[0]
        norm.append(dict(seed=seed, H=H, N=N, K=K, digest=al.digest(w.numpy()), neg_matrix_bits=[int(v) for v in (-m).numpy().view(np.int32).ravel()]))
    out = dict(note="written by tests/golden/make_align_goldens.py", transformers=transformers.__version__, dtw=dtw, median=med, normalise=norm)
    with open(al.FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(al.FIXTURE, os.path.getsize(al.FIXTURE), "bytes")
    assert os.path.getsize(al.FIXTURE) <= 200 * 1024


if __name__ == "__main__":
    main()
