#!/usr/bin/env python3
"""S streams x F frames through the Silero gate: (a) the libm gate and (b) the CPU contract evaluator on 1 and 16 threads (one
stream per task), (c) skw_vad_gpu_process.  One JSON line per row.  GPU rows report device time by events after a warm-up, with
the PCIe copies apart from the kernels, and the wall time of the call.

usage: bench_vad.py [--streams 64] [--frames 937] [--model PATH] [--reps 5] [--cpu-streams N] [--no-cpu] [--no-gpu]
(--cpu-streams: the CPU rows time only the first N streams and scale, default 16: the CPU gate takes ~1 ms per frame)
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--frames", type=int, default=937)
    ap.add_argument("--model", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-streams", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    a = ap.parse_args()
    import make_synth_silero
    import silero_lib
    from streamkit_amd import vad
    path = a.model
    if path is None:
        path = "/tmp/skw_bench_silero_random.onnx"
        with open(path, "wb") as f:
            f.write(make_synth_silero.build(1234, random_lstm=True)[0])
    S, F = a.streams, a.frames
    audio = [silero_lib.speechlike(F, seed=i) for i in range(S)]
    total = S * F
    base = {"streams": S, "frames_per_stream": F, "audio_seconds": total * 0.032}

    def row(name, seconds, **kw):
        r = dict(base, row=name, seconds=seconds, frames_per_second=total / seconds, us_per_frame=seconds / total * 1e6, x_realtime=total * 0.032 / seconds)
        r.update(kw)
        print(json.dumps(r), flush=True)

    if not a.no_cpu:
        n = min(S, a.cpu_streams)
        for arith, name in ((vad.ARITH_LIBM, "cpu_libm"), (vad.ARITH_CONTRACT, "cpu_contract")):
            for threads in (1, 16):
                gates = [vad.CpuVad(path, arith) for _ in range(n)]
                gates[0].process_chunks(audio[0][:8 * 512]); gates[0].reset()
                t0 = time.perf_counter()
                with ThreadPoolExecutor(threads) as ex:      # ctypes releases the GIL inside the call
                    list(ex.map(lambda i: gates[i].process_chunks(audio[i]), range(n)))
                dt = (time.perf_counter() - t0) * S / n
                row("%s_%dt" % (name, threads), dt, threads=threads, timed_streams=n, scaled=n != S)
    if not a.no_gpu:
        g = vad.GpuVad(path, 0)
        for _ in range(2):
            g.process(audio, [np.zeros(320, np.float32) for _ in range(S)])
        walls, tim = [], []
        for _ in range(a.reps):
            st = [np.zeros(320, np.float32) for _ in range(S)]
            t0 = time.perf_counter()
            g.process(audio, st)
            walls.append(time.perf_counter() - t0); tim.append(g.last_timing())
        k = int(np.argsort(walls)[len(walls) // 2])
        h2d, ker, d2h = tim[k]
        row("gpu", walls[k], h2d_ms=h2d, kernels_ms=ker, d2h_ms=d2h, wall_ms_all=[round(w * 1e3, 3) for w in walls], kernels_ms_all=[round(t[1], 3) for t in tim],
            kernels_us_per_stream_step=ker * 1e3 / F)
        g.close()


if __name__ == "__main__":
    main()
