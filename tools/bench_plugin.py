#!/usr/bin/env python3
"""BASELINE config 2 through the drop-in boundary: N concurrent plugin instances (libwhisper.so, StreamKit native ABI v2), each fed one
30 s clip in 960-sample RawAudio packets from host memory and flushed, the way N oneshot HTTP requests would drive the reference node.
Informational: the bench.py headline times the engine with PCM resident in HBM; this adds packet feeding, the 512-sample
framing, batch formation across instances, H2D copies and JSON building.   usage: python tools/bench_plugin.py [--clips 64] [--size small]
--param-sets K deals K different parameter blocks over the instances (K = 1: all alike; the sets differ in `language` first — en, de, es, fr — then in
suppress_non_speech_tokens, then in suppress_blank) and --mixed-batch 0|1 sets the node's `mixed_batch`: with 1 (the default) the K groups share GPU batches
(skw_full_batch_mixed), with 0 the scheduler cuts a batch at the first job whose parameters differ.  Prints wall time (best and every repetition), x real time and the
node's batch counters over the timed repetitions (engine calls, jobs, calls that carried different parameter blocks).  --tree DIR drives another checkout's build
(the parent commit in a side directory) with the same loop, for alternated A/Bs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64); ap.add_argument("--size", default="small"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch-window-ms", type=float, default=40.0); ap.add_argument("--packet", type=int, default=960)
    ap.add_argument("--precision", default="f16_mfma", choices=["exact", "f16_mfma"])
    ap.add_argument("--param-sets", type=int, default=1, help="1..16 different parameter blocks dealt over the instances")
    ap.add_argument("--mixed-batch", type=int, default=1, choices=[0, 1], help="the node's mixed_batch parameter")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose built libraries and bindings are driven (default: this one).  For A/Bs against another commit built in a "
                                                 "side directory: same loop, same inputs; a build without the batch counters prints null for them and ignores mixed_batch")
    a = ap.parse_args()
    assert 1 <= a.param_sets <= 16 and a.reps >= 1
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree); sys.path.insert(0, os.path.join(tree, "tests"))
    import torch  # noqa: F401  (libamdhip64 first, as bench.py does)
    from streamkit_amd import minihost
    from conftest import synth_model
    from streamkit_amd import synth
    assert os.path.abspath(minihost.ROOT) == tree, (minihost.ROOT, tree)
    batch_stats = getattr(minihost, "whisper_batch_stats", None)
    path = synth_model(a.size)
    plug = minihost.Plugin()
    pcms = [synth.clip(c) for c in range(a.clips)]
    params = {"model_path": path, "vad_mode": "always", "flush_tail": True, "max_batch": a.clips, "batch_window_ms": a.batch_window_ms, "precision": a.precision,
              "mixed_batch": bool(a.mixed_batch)}
    langs = ["en", "de", "es", "fr"]
    sets = [{"language": langs[k % 4], "suppress_non_speech_tokens": not (k // 4) & 1, "suppress_blank": not (k // 8) & 1} for k in range(a.param_sets)]
    best = None; walls = []; stats0 = None
    for rep in range(a.reps + 1):
        if rep == 1 and batch_stats: stats0 = batch_stats()
        nodes = [plug.create_node(dict(params, **sets[i % len(sets)])) for i in range(a.clips)]      # model load is cached per path (first create pays it; excluded, as in the reference)
        ms = C.c_double(minihost.run_oneshot(nodes, pcms, a.packet))
        outs = [n.outputs() for n in nodes]
        assert all(len(o) == 1 and o[0][1] == 3 for o in outs), [len(o) for o in outs]
        for n in nodes: n.destroy()
        if rep > 0: best = ms.value if best is None else min(best, ms.value); walls.append(round(ms.value, 2))     # rep 0 = warm-up
    audio_s = sum(p.size for p in pcms) / 16000.0
    n_seg = sum(len(json.loads(o[0][2].decode())["segments"]) for o in outs)
    print(json.dumps({"what": "plugin-level Oneshot batch (host PCM -> Transcription JSON), %d instances" % a.clips, "value": round(audio_s / (best * 1e-3), 1), "unit": "x real-time",
                      "wall_ms": round(best, 2), "packet_samples": a.packet, "batch_window_ms": a.batch_window_ms, "segments": n_seg, "model": a.size, "precision": a.precision,
                      "wall_ms_reps": walls, "param_sets": a.param_sets, "mixed_batch": a.mixed_batch,
                      "batch_stats": dict(zip(("engine_calls", "jobs", "mixed_calls"), [x - y for x, y in zip(batch_stats(), stats0)])) if batch_stats else None,
                      "tree": os.path.relpath(tree, ROOT)}))


if __name__ == "__main__":
    main()
