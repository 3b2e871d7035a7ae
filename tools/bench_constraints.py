#!/usr/bin/env python3
"""Decoding constraints through the engine (skw_full_batch_rules): what the constraint kernel costs and what the rules change.

(1) The benchmark batch — Whisper-small, 64 clips of 30 s, both precisions — with the rules off and with repetition_penalty 1.1 + no_repeat_ngram_size 3 on every clip,
    alternated repetition by repetition in one process: wall, decode ms, decode steps, tokens and fallback passes per configuration (medians), and k_dec_constrain's time per
    launch from the per-kernel-class profile (one extra, eager call).
(2) The long-form batch of tools/bench_longform.py (32 clips of 95 s, f16_mfma) with and without no_repeat_ngram_size 3: windows, fallback_requested and wall.

Prints one JSON object.
usage: python tools/bench_constraints.py [--clips 64] [--size small] [--reps 3] [--long-clips 32] [--long-s 95] [--no-longform]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(ctx, pcms, p, rules):
    t0 = time.perf_counter(); res = ctx.full_batch(pcms, p, rules=rules); wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    return dict(wall_ms=wall, decode_ms=t["decode_ms"], encode_ms=t["encode_ms"], decode_steps=t["n_decode_steps"], windows=t["n_windows"], tokens=t["n_tokens"],
                result_windows=sum(r["n_windows"] for r in res), fallback_requested=sum(r["fallback_requested"] for r in res))


def alternate(ctx, pcms, p, configs, reps):
    """the configurations alternated repetition by repetition after one warm-up each (step graphs captured); medians of the timed figures, the counts of the last repetition"""
    for rules in configs.values():
        run(ctx, pcms, p, rules)
    acc = {k: [] for k in configs}
    for _ in range(reps):
        for k, rules in configs.items():
            acc[k].append(run(ctx, pcms, p, rules))
    out = {}
    for k, rs in acc.items():
        out[k] = dict(rs[-1], wall_ms=round(statistics.median(r["wall_ms"] for r in rs), 2), decode_ms=round(statistics.median(r["decode_ms"] for r in rs), 2),
                      encode_ms=round(statistics.median(r["encode_ms"] for r in rs), 2), wall_ms_all=[round(r["wall_ms"], 2) for r in rs], decode_ms_all=[round(r["decode_ms"], 2) for r in rs])
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
    out = {"what": "%d x 30 s, Whisper-%s: rules off vs repetition_penalty 1.1 + no_repeat_ngram_size 3" % (a.clips, a.size), "reps": a.reps, "precisions": {}}
    m = engine.Model(synth_model(a.size))
    pcms = [synth.clip(c, 480000) for c in range(a.clips)]
    ctx = engine.Context(m, max_batch=a.clips, max_samples=480000)
    p = ctx.default_params(); p.suppress_nst = 1
    on = [engine.DecodeRules(repetition_penalty=1.1, no_repeat_ngram_size=3) for _ in range(a.clips)]
    for prec in a.precisions.split(","):
        ctx.set_precision(prec)
        rec = alternate(ctx, pcms, p, {"rules_off": None, "penalty_1.1_ngram_3": on}, a.reps)
        ctx.profile(True); run(ctx, pcms, p, on); prof = ctx.profile_get(); ctx.profile(False)
        k, s = prof["k_dec_constrain"], prof["k_dec_sample"]
        rec["k_dec_constrain"] = dict(launches=k["count"], ms=round(k["ms"], 3), us_per_launch=round(1e3 * k["ms"] / max(1, k["count"]), 2),
                                      k_dec_sample_us_per_launch=round(1e3 * s["ms"] / max(1, s["count"]), 2), note="HIP events around eager launches, one row group")
        out["precisions"][prec] = rec
    ctx.close()
    if not a.no_longform:
        n = int(16000 * a.long_s)
        lp = [synth.clip(200 + c, n) for c in range(a.long_clips)]
        ctx = engine.Context(m, max_batch=a.long_clips, max_samples=n + 16)
        ctx.set_precision("f16_mfma")
        n3 = [engine.DecodeRules(no_repeat_ngram_size=3) for _ in range(a.long_clips)]
        out["longform"] = dict(what="%d x %g s, f16_mfma: rules off vs no_repeat_ngram_size 3" % (a.long_clips, a.long_s),
                               **alternate(ctx, lp, p, {"rules_off": None, "ngram_3": n3}, max(1, a.reps - 1)))
        ctx.close()
    m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
