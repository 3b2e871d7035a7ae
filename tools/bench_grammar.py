#!/usr/bin/env python3
"""Grammar-constrained decoding through the engine (skw_full_batch_grammar): what k_dec_grammar costs.

Whisper-small, 64 rows, f16_mfma (the benchmark's model and precision; --secs of audio per clip, 10 by default: the decode step does not depend on it).  Three configurations,
alternated repetition by repetition in one process after a warm-up each (step graphs captured):
  no_grammar     the call as it is without
  small_table    a ~10-state grammar on every row: ( [a-z]{3,8})+ — every word of the synthetic vocabulary that starts with a space fits, so the transcripts go on for as many
                 steps as without and the per-step figures compare
  table_4096     a 4096-state table on every row that lets the same words through (the state counts bytes), so its walks touch rows all over the 2 MiB table
Reported per configuration: wall, decode ms, decode steps, decode ms per step (medians).  From one extra eager, profiled call each: k_dec_grammar's time per launch (both of its
kernels; HIP events, one row group) next to the launch's algorithmic bytes — two passes over rows x n_vocab f32, plus the table — and k_dec_sample's for scale.

Prints one JSON object.
usage: python tools/bench_grammar.py [--clips 64] [--size small] [--reps 3] [--secs 10] [--precision f16_mfma]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def letters_table(engine, n, penalty):
    """n states over lowercase letters and the space; the state counts bytes, every state but the start accepts"""
    nxt = np.full((n, 256), engine.GRAMMAR_DEAD, np.uint16)
    for k in range(n):
        nxt[k, [ord(" ")] + list(range(ord("a"), ord("z") + 1))] = (k % (n - 1)) + 1
    acc = np.ones(n, np.uint8); acc[0] = 0
    return engine.Grammar.from_tables(nxt, acc, penalty)


def run(ctx, pcms, p, grammars):
    t0 = time.perf_counter(); res = ctx.full_batch(pcms, p, grammars=grammars); wall = (time.perf_counter() - t0) * 1e3
    t = ctx.timing()
    return dict(wall_ms=wall, decode_ms=t["decode_ms"], decode_steps=t["n_decode_steps"], tokens=t["n_tokens"], fallback_requested=sum(r["fallback_requested"] for r in res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64); ap.add_argument("--size", default="small"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--secs", type=float, default=10.0); ap.add_argument("--precision", default="f16_mfma"); ap.add_argument("--penalty", type=float, default=100.0)
    a = ap.parse_args()
    import torch  # noqa: F401  (libamdhip64 first, as bench.py does)
    from streamkit_amd import engine, synth
    from conftest import synth_model
    m = engine.Model(synth_model(a.size))
    n = int(16000 * a.secs)
    pcms = [synth.clip(c, n) for c in range(a.clips)]
    ctx = engine.Context(m, max_batch=a.clips, max_samples=n + 16)
    ctx.set_precision(a.precision)
    p = ctx.default_params(); p.suppress_nst = 1
    small = engine.Grammar.compile(r"( [a-z]{3,8})+", penalty=a.penalty)
    big = letters_table(engine, 4096, a.penalty)
    configs = {"no_grammar": None, "small_table": [small] * a.clips, "table_4096": [big] * a.clips}
    out = {"what": "%d x %g s, Whisper-%s, %s: no grammar vs a %d-state and a 4096-state table on every row" % (a.clips, a.secs, a.size, a.precision, small.n_states),
           "reps": a.reps, "configs": {}}
    for g in configs.values():
        run(ctx, pcms, p, g)
    acc = {k: [] for k in configs}
    for _ in range(a.reps):
        for k, g in configs.items():
            acc[k].append(run(ctx, pcms, p, g))
    NV = m.hp.n_vocab
    for k, rs in acc.items():
        rec = dict(rs[-1], wall_ms=round(statistics.median(r["wall_ms"] for r in rs), 2), decode_ms=round(statistics.median(r["decode_ms"] for r in rs), 2),
                   decode_ms_all=[round(r["decode_ms"], 2) for r in rs])
        rec["decode_ms_per_step"] = round(rec["decode_ms"] / max(1, rec["decode_steps"]), 4)
        if configs[k] is not None:
            ctx.profile(True); run(ctx, pcms, p, configs[k]); prof = ctx.profile_get(); ctx.profile(False)
            kg, ks = prof["k_dec_grammar"], prof["k_dec_sample"]
            table_bytes = configs[k][0].n_states * 513
            us = 1e3 * kg["ms"] / max(1, kg["count"])
            rec["k_dec_grammar"] = dict(launches=kg["count"], us_per_launch=round(us, 2), k_dec_sample_us_per_launch=round(1e3 * ks["ms"] / max(1, ks["count"]), 2),
                                        n_states=configs[k][0].n_states, algorithmic_bytes=8 * a.clips * NV + table_bytes,
                                        algorithmic_gb_per_s=round((8 * a.clips * NV + table_bytes) / (us * 1e-6) / 1e9, 1) if us > 0 else None,
                                        note="both kernels of the stage; HIP events around eager launches, one row group; rows that finished return at once")
        out["configs"][k] = rec
    ctx.close(); m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
