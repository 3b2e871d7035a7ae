#!/usr/bin/env python3
"""Short segments through the engine at different audio contexts (skw_full_params.audio_ctx): N clips of a few seconds in one batch, with audio_ctx 0 (the model's 1500
positions), a fixed value, and "auto" (skw_audio_ctx_for_samples per clip).  Per setting: wall time of the call, the engine's encode_ms / decode_ms, and — from the in-kernel
launch clock of the decode step's cross attention — time per launch next to its algorithmic bytes, 4 B x (keys walked by the launch's live rows) x n_text_state.
usage: python tools/bench_audio_ctx.py [--clips 64] [--clip-s 4 | 1-9] [--size small] [--precision f16_mfma] [--fixed 256] [--reps 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64); ap.add_argument("--size", default="small"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clip-s", default="4", help="clip length in seconds: one number, or lo-hi for lengths spread evenly over the batch (e.g. 1-9)")
    ap.add_argument("--precision", default="f16_mfma", choices=["exact", "f16_mfma"]); ap.add_argument("--fixed", type=int, default=256)
    a = ap.parse_args()
    import torch  # noqa: F401  (libamdhip64 first, as bench.py does)
    from streamkit_amd import engine, synth
    from conftest import synth_model
    lo, hi = (float(x) for x in (a.clip_s.split("-") if "-" in a.clip_s else (a.clip_s, a.clip_s)))
    pcms = [synth.clip(c, int(16000 * (lo + (hi - lo) * (c * 7 % a.clips) / max(1, a.clips - 1)))) for c in range(a.clips)]
    m = engine.Model(synth_model(a.size)); ctx = engine.Context(m, max_batch=a.clips, max_samples=max(p.size for p in pcms) + 16000)
    ctx.set_precision(a.precision)
    nc, dt = m.hp.n_audio_ctx, m.hp.n_text_state
    out = {"what": "engine batch of %d clips of %s s, %s, %s" % (a.clips, a.clip_s, a.size, a.precision), "audio_s": round(sum(p.size for p in pcms) / 16000.0, 1), "settings": {}}
    for name in ("0", str(a.fixed), "auto"):
        ks = [engine.audio_ctx_for_samples(p.size, nc) if name == "auto" else int(name) for p in pcms]
        params = []
        for k in ks:
            p = ctx.default_params(); p.audio_ctx = k; params.append(p)
        call = (lambda: ctx.full_batch(pcms, params=params)) if name == "auto" else (lambda: ctx.full_batch(pcms, params[0]))
        call()                                                        # warm-up: step graphs captured, workspace touched
        walls, enc, dec = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); res = call(); walls.append((time.perf_counter() - t0) * 1e3)
            t = ctx.timing(); enc.append(t["encode_ms"]); dec.append(t["decode_ms"])
        rec = {"audio_ctx": sorted(set(ks)), "wall_ms": [round(x, 2) for x in walls], "encode_ms": [round(x, 2) for x in enc], "decode_ms": [round(x, 2) for x in dec],
               "decode_steps": t["n_decode_steps"], "row_steps": t["n_row_steps"], "tokens": sum(len(r["tokens"]) for r in res)}
        if a.precision == "f16_mfma":
            ctx.kernel_clock(True); call(); kc = ctx.kernel_clock_get(); keys = ctx.kernel_clock_keys(); ctx.kernel_clock(False)
            if kc["launches"]:
                by = 4.0 * keys * dt
                rec["cross_attention"] = {"launches": kc["launches"], "us_per_launch": round(kc["sum_us"] / kc["launches"], 2), "min_us": round(kc["min_us"], 2), "max_us": round(kc["max_us"], 2),
                                          "live_rows_per_launch": round(kc["sum_live_rows"] / kc["launches"], 1), "keys_per_live_row": round(keys / max(1.0, kc["sum_live_rows"]), 1),
                                          "algorithmic_MB_per_launch": round(by / kc["launches"] / 1e6, 2), "algorithmic_GB_per_s": round(by / (kc["sum_us"] * 1e-6) / 1e9, 1)}
        out["settings"][name] = rec
    ctx.close(); m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
