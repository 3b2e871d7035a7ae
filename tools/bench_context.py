#!/usr/bin/env python3
"""Carried context through the engine (skw_full_batch_context): N clips of a few seconds in one batch, each behind a context of up to 224 tokens, against the same clips with no
context; and, in the exact precision, the prompt pass's two cross-attention kernels — the 16-queries-per-workgroup one (skw_debug_set_prompt_xattn_mq 1, the default) and the
single-query one on every prompt row (0) — alternated in one process, repetition by repetition, so that both see the same clocks and the same neighbours.

Per setting: wall time of the call and the engine's decode_ms, for the whole call and for a call cut after the second token (max_tokens = 1): its decode_ms is the prompt pass plus
two decode steps, which is how the prompt pass is timed without a profiler.  --sweep: the same cut call with contexts of n tokens (n + 3 prompt rows per clip on a multilingual
model), for the selection constant SKW_XATTN_MQ_MIN_NQ.
usage: python tools/bench_context.py [--clips 64] [--clip-s 10] [--size small] [--tokens 224] [--reps 5] [--sweep 1,5,13,29,61,125,221]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64); ap.add_argument("--size", default="small"); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clip-s", type=float, default=10.0); ap.add_argument("--tokens", type=int, default=224); ap.add_argument("--sweep", default="1,5,13,29,61,125,221")
    ap.add_argument("--precisions", default="exact,f16_mfma")
    a = ap.parse_args()
    import torch  # noqa: F401  (libamdhip64 first, as bench.py does)
    from streamkit_amd import engine, synth
    from conftest import synth_model
    pcms = [synth.clip(c, int(16000 * a.clip_s)) for c in range(a.clips)]
    m = engine.Model(synth_model(a.size)); ctx = engine.Context(m, max_batch=a.clips, max_samples=pcms[0].size + 16000)
    rng = np.random.default_rng(7)
    make = lambda n: [engine.context_new(rng.integers(0, 2000, size=n).tolist()) for _ in range(a.clips)]

    def run(contexts, max_tokens):
        p = ctx.default_params(); p.temperature_inc = 0.0; p.max_tokens = max_tokens
        cx = None if contexts is None else [x.copy() for x in contexts]
        t0 = time.perf_counter(); res = ctx.full_batch(pcms, p, contexts=cx); wall = (time.perf_counter() - t0) * 1e3
        t = ctx.timing()
        return dict(wall_ms=wall, decode_ms=t["decode_ms"], encode_ms=t["encode_ms"], tokens=sum(len(r["tokens"]) for r in res), ids=[[k[0] for k in r["tokens"]] for r in res])

    def ab(contexts, max_tokens, modes):
        """the modes alternated repetition by repetition; medians, and whether every mode produced the same tokens"""
        for mq in modes:
            ctx.set_prompt_xattn_mq(mq); run(contexts, max_tokens)            # warm-up: step graphs captured, workspace touched
        acc = {mq: [] for mq in modes}
        for _ in range(a.reps):
            for mq in modes:
                ctx.set_prompt_xattn_mq(mq); acc[mq].append(run(contexts, max_tokens))
        ctx.set_prompt_xattn_mq(1)
        med = lambda rs, k: round(statistics.median(r[k] for r in rs), 2)
        out = {("mq" if mq else "single_query"): dict(wall_ms=med(rs, "wall_ms"), decode_ms=med(rs, "decode_ms"), decode_ms_all=[round(r["decode_ms"], 2) for r in rs], tokens=rs[0]["tokens"])
               for mq, rs in acc.items()}
        out["same_tokens"] = all(rs[0]["ids"] == acc[modes[0]][0]["ids"] for rs in acc.values())
        return out

    out = {"what": "%d clips of %g s, %s, contexts of %d tokens" % (a.clips, a.clip_s, a.size, a.tokens), "reps": a.reps, "precisions": {}}
    full = make(a.tokens)
    for prec in a.precisions.split(","):
        ctx.set_precision(prec)
        modes = [0, 1] if prec == "exact" else [1]                            # (f16_mfma has its own multi-query prompt kernel: the switch does not reach it)
        rec = {"context_prompt_pass": ab(full, 1, modes), "context_whole_call": ab(full, 0, modes),
               "no_context_prompt_pass": ab(None, 1, modes), "no_context_whole_call": ab(None, 0, modes)}
        if prec == "exact" and a.sweep:
            rec["sweep_prompt_pass"] = {str(n + 3): ab(make(n), 1, modes) for n in (int(x) for x in a.sweep.split(","))}
        out["precisions"][prec] = rec
    ctx.close(); m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
