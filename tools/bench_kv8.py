#!/usr/bin/env python3
"""cross_kv f16 against q8_0 on one MI355X, in one process, the two alternating (include/skw_kv8.h; DESIGN.md section 3, "8-bit cross K/V").

What it measures, on the benchmark model (Whisper-small geometry, seeded weights) in the f16_mfma precision:
  * the decode step's cross-attention launch through the kernel's own clock (skw_ctx_kernel_clock: first wave in to last wave out) in the timed configuration — step graphs —
    at 64 live rows x 1500 keys: median over the launches with every row live, f16 and q8_0;
  * the same on a short-clip batch with audio_ctx "auto" (all launches: mean time per live row);
  * the quantise kernel: the "other" class of the per-class event profile with the flag on minus the same class with it off (one eager, profiled call each), per 64-slot batch;
  * the batch's wall time (host clock around a call that ends synchronised) and the engine's own decode_ms, f16 / q8_0 alternating, `--reps` rounds after a warm-up of each;
  * the teacher-forced comparison of the q8_0 leg against the EXACT precision on the benchmark batch (streamkit_amd/parity.py): decisions, disagreements, largest exact-mode
    margin at a disagreement, largest logit error — the figures parity.py's KV8_* bounds are set from.
No GPU: fails.  One JSON document on stdout (and --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="small")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-parity", action="store_true", help="skip the teacher-forced comparison (the exact leg is the slowest part)")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv8: no GPU (a measurement path does not fall back)")
    from streamkit_amd import engine, synth
    from streamkit_amd.parity import teacher_forced_compare

    tool = os.path.join(ROOT, "tools", "make_synth_model")
    if not os.path.exists(tool):
        subprocess.check_call(["gcc", "-O2", "-o", tool, tool + ".c", "-lm"])
    path = "/tmp/skw_bench_%s_seed1234_v3.bin" % args.size
    if not os.path.exists(path):
        subprocess.check_call([tool, path + ".tmp", "--size", args.size, "--seed", "1234"]); os.replace(path + ".tmp", path)
    model = engine.Model(path, device=0); hp = model.hp
    B = args.clips; n_samples = 480000
    ctx = engine.Context(model, max_batch=B, max_samples=n_samples)
    ctx.set_precision("f16_mfma")
    base = ctx.default_params(); base.suppress_nst = 1

    long_clips = [synth.clip(c, n_samples) for c in range(B)]
    secs = [2 + (7 * c) % 9 for c in range(B)]                               # 2 .. 10 s
    short_clips = [synth.clip(1000 + c, 16000 * s) for c, s in enumerate(secs)]
    short_params = []
    for c in short_clips:
        p = ctx.default_params(); p.suppress_nst = 1; p.audio_ctx = engine.audio_ctx_for_samples(c.size, hp.n_audio_ctx); short_params.append(p)

    def call(clips, params):
        t0 = time.perf_counter()
        res = ctx.full_batch(clips, params)                                   # returns with the stream drained
        return 1000.0 * (time.perf_counter() - t0), ctx.timing(), res

    def clock(clips, params, full_rows):
        """the launches of one call (after one that captured the graphs): per-launch us over the launches with `full_rows` live rows, and us per live row over all"""
        ctx.kernel_clock(True)
        try:
            ctx.full_batch(clips, params); ctx.full_batch(clips, params)
            g = ctx.kernel_clock_get(); rec = ctx.kernel_clock_records(); keys = ctx.kernel_clock_keys()
        finally:
            ctx.kernel_clock(False)
        us = rec[:, 1] - rec[:, 0]; full = us[rec[:, 2] == full_rows]
        return dict(launches=int(g["launches"]), launches_all_rows_live=int(full.size), us_median_all_rows_live=float(np.median(full)) if full.size else None,
                    us_min_all_rows_live=float(full.min()) if full.size else None, us_max_all_rows_live=float(full.max()) if full.size else None,
                    us_per_live_row=float(g["sum_us"] / g["sum_live_rows"]) if g["sum_live_rows"] else None, keys_walked=float(keys))

    def profiled(clips, params):
        ctx.profile(True)
        try:
            ctx.full_batch(clips, params)
            return ctx.profile_get()
        finally:
            ctx.profile(False)

    out = dict(model=args.size, clips=B, n_audio_ctx=hp.n_audio_ctx, precision="f16_mfma", reps=args.reps)
    kinds = ("f16", "q8_0")
    for name, clips, params in (("benchmark_batch", long_clips, base), ("short_clips_audio_ctx_auto", short_clips, short_params)):
        sec = {k: dict(wall_ms=[], decode_ms=[], encode_ms=[]) for k in kinds}
        for k in kinds:                                                       # warm-up: every shape, both flags (graphs are keyed by the flag)
            ctx.set_cross_kv(k); call(clips, params)
        for _ in range(args.reps):
            for k in kinds:
                ctx.set_cross_kv(k)
                wall, t, res = call(clips, params)
                sec[k]["wall_ms"].append(round(wall, 2)); sec[k]["decode_ms"].append(round(t["decode_ms"], 2)); sec[k]["encode_ms"].append(round(t["encode_ms"], 2))
                sec[k]["decode_steps"] = t["n_decode_steps"]; sec[k]["tokens"] = sum(len(r["tokens"]) for r in res)
        for k in kinds:
            ctx.set_cross_kv(k)
            sec[k]["cross_attention_clock"] = clock(clips, params, B)
            pr = profiled(clips, params)
            sec[k]["profile_other_ms"] = pr["other"]["ms"]; sec[k]["profile_cross_attn"] = pr["k_dec_cross_attn"]
            for f in ("wall_ms", "decode_ms", "encode_ms"):
                sec[k][f + "_median"] = statistics.median(sec[k][f])
        sec["quantise_ms_per_call"] = round(sec["q8_0"]["profile_other_ms"] - sec["f16"]["profile_other_ms"], 3)
        a, b = sec["f16"]["cross_attention_clock"], sec["q8_0"]["cross_attention_clock"]
        key = "us_median_all_rows_live" if a["us_median_all_rows_live"] and b["us_median_all_rows_live"] else "us_per_live_row"
        sec["launch_ratio_q8_over_f16"] = round(b[key] / a[key], 4); sec["launch_ratio_of"] = key
        sec["wall_ratio_q8_over_f16"] = round(sec["q8_0"]["wall_ms_median"] / sec["f16"]["wall_ms_median"], 4)
        sec["decode_ratio_q8_over_f16"] = round(sec["q8_0"]["decode_ms_median"] / sec["f16"]["decode_ms_median"], 4)
        out[name] = sec
    ctx.set_cross_kv("f16")
    if not args.no_parity:
        for name, kv in (("teacher_forced_f16_vs_exact", "f16"), ("teacher_forced_q8_0_vs_exact", "q8_0")):
            tf = teacher_forced_compare(ctx, long_clips, base, cross_kv=kv, logit_err_bound=float("inf"), margin_bound=float("inf"))
            out[name] = {k: tf[k] for k in ("steps_checked", "argmax_disagreements", "disagreements_on_exact_runner_up", "max_margin_at_disagreement", "max_logit_err")}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    ctx.close(); model.close()


if __name__ == "__main__":
    main()
