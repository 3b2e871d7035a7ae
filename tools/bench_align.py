#!/usr/bin/env python3
"""Word timestamps through the engine (skw_full_batch_aligned): what the alignment phase costs.

(1) The benchmark batch — Whisper-small, 64 clips of 30 s, both precisions — with alignment off and with every clip aligned on the top half of the decoder layers,
    alternated repetition by repetition in one process: wall, decode ms, windows and tokens per configuration (medians; the alignment phase runs after a window's decode
    timing ends, so it shows in wall_ms), and the three alignment kernels' time per launch from the per-kernel-class profile (classes 10-12; one extra, eager call).
(2) The long-form batch of tools/bench_longform.py (32 clips of 95 s, f16_mfma) off / on.

Prints one JSON object.
usage: python tools/bench_align.py [--clips 64] [--size small] [--reps 3] [--long-clips 32] [--long-s 95] [--no-longform] [--precisions exact,f16_mfma]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(ctx, pcms, p, align):
    t0 = time.perf_counter(); res = ctx.full_batch(pcms, [p] * len(pcms), align=align); wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    timed = sum(1 for r in res for a, _ in r["token_times"] if a >= 0)
    return dict(wall_ms=wall, total_ms=t["total_ms"], decode_ms=t["decode_ms"], encode_ms=t["encode_ms"], windows=t["n_windows"], tokens=t["n_tokens"], timed_tokens=timed)


def alternate(ctx, pcms, p, configs, reps):
    """the configurations alternated repetition by repetition after one warm-up each; medians of the timed figures, the counts of the last repetition"""
    for al in configs.values():
        run(ctx, pcms, p, al)
    acc = {k: [] for k in configs}
    for _ in range(reps):
        for k, al in configs.items():
            acc[k].append(run(ctx, pcms, p, al))
    out = {}
    for k, rs in acc.items():
        out[k] = dict(rs[-1], **{f: round(statistics.median(r[f] for r in rs), 2) for f in ("wall_ms", "total_ms", "decode_ms", "encode_ms")}, wall_ms_all=[round(r["wall_ms"], 2) for r in rs])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64); ap.add_argument("--size", default="small"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long-clips", type=int, default=32); ap.add_argument("--long-s", type=float, default=95.0); ap.add_argument("--no-longform", action="store_true")
    ap.add_argument("--precisions", default="exact,f16_mfma")
    a = ap.parse_args()
    import torch  # noqa: F401  (libamdhip64 first, as bench.py does)
    from streamkit_amd import engine, synth
    from conftest import synth_model
    m = engine.Model(synth_model(a.size))
    top = max(1, m.hp.n_text_layer // 2)
    out = {"what": "%d x 30 s, Whisper-%s: alignment off vs on (every head of the top %d decoder layers)" % (a.clips, a.size, top), "reps": a.reps, "precisions": {}}
    pcms = [synth.clip(c, 480000) for c in range(a.clips)]
    ctx = engine.Context(m, max_batch=a.clips, max_samples=480000)
    p = ctx.default_params(); p.suppress_nst = 1
    ap_on = engine.align_params(top=top, hp=m.hp)
    for prec in a.precisions.split(","):
        ctx.set_precision(prec)
        rec = alternate(ctx, pcms, p, {"align_off": [None] * a.clips, "align_on": [ap_on] * a.clips}, a.reps)
        ctx.profile(True); run(ctx, pcms, p, [ap_on] * a.clips); prof = ctx.profile_get(); ctx.profile(False)
        rec["kernels"] = {k: dict(launches=prof[k]["count"], ms=round(prof[k]["ms"], 3), us_per_launch=round(1e3 * prof[k]["ms"] / max(1, prof[k]["count"]), 2))
                          for k in ("k_align_qk", "k_align_reduce", "k_align_dtw")}
        out["precisions"][prec] = rec
    ctx.close()
    if not a.no_longform:
        n = int(16000 * a.long_s)
        lp = [synth.clip(200 + c, n) for c in range(a.long_clips)]
        ctx = engine.Context(m, max_batch=a.long_clips, max_samples=n + 16)
        ctx.set_precision("f16_mfma")
        out["longform"] = dict(what="%d x %g s, f16_mfma: alignment off vs on" % (a.long_clips, a.long_s),
                               **alternate(ctx, lp, p, {"align_off": [None] * a.long_clips, "align_on": [ap_on] * a.long_clips}, max(1, a.reps - 1)))
        ctx.close()
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
