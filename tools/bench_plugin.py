#!/usr/bin/env python3
"""BASELINE config 2 through the drop-in boundary: N concurrent plugin instances (libwhisper.so, StreamKit native ABI v2), each fed one
30 s clip in 960-sample RawAudio packets from host memory and flushed, the way N oneshot HTTP requests would drive the reference node.
Informational: the bench.py headline times the engine with PCM resident in HBM; this adds packet feeding, the 512-sample
framing, batch formation across instances, H2D copies and JSON building.   usage: python tools/bench_plugin.py [--clips 64] [--size small]
--param-sets K deals K different parameter blocks over the instances (K = 1: all alike; the sets differ in `language` first — en, de, es, fr — then in
suppress_non_speech_tokens, then in suppress_blank) and --mixed-batch 0|1 sets the node's `mixed_batch`: with 1 (the default) the K groups share GPU batches
(skw_full_batch_mixed), with 0 the scheduler cuts a batch at the first job whose parameters differ.  Prints wall time (best and every repetition), x real time and the
node's batch counters over the timed repetitions (engine calls, jobs, calls that carried different parameter blocks).  --tree DIR drives another checkout's build
(the parent commit in a side directory) with the same loop, for alternated A/Bs.
--vad-mode silero|energy|auto|always (default always: the gate switched off, the run the earlier figures were taken with) puts the node's VAD gate into the measurement.
With a gate the clips are multiplied by the on/off pattern of tests/silero_lib.speechlike, so that the gate opens and closes, and the line also carries the share of frames
judged speech (by the libm gate on the CPU, outside the timed region), the number of segments cut and the audio seconds that reached Whisper: the gate decides how much work
Whisper gets.  --vad-model names the Silero file (default: the seeded engineered file of tools/make_synth_silero.py, written by THIS checkout's tool also when --tree points
elsewhere); --vad-device cpu|gpu and --vad-batch-frames N are sent only when given, so that a tree that predates them can be driven."""
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
    ap.add_argument("--vad-mode", default="always", choices=["always", "energy", "silero", "auto"])
    ap.add_argument("--vad-model", default=None, help="Silero .onnx file (default: the seeded file of tools/make_synth_silero.py)")
    ap.add_argument("--vad-device", default=None, choices=["cpu", "gpu"], help="the node's vad_device (not sent when absent)")
    ap.add_argument("--vad-batch-frames", type=int, default=None, help="the node's vad_batch_frames (not sent when absent)")
    ap.add_argument("--audio-ctx", default=None, help="the node's audio_ctx: 0, an integer 1..n_audio_ctx, or auto (not sent when absent)")
    ap.add_argument("--clip-s", default="30", help="clip length in seconds: one number, or lo-hi for lengths spread evenly over the instances (e.g. 1-9)")
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
    lo, hi = (float(x) for x in (a.clip_s.split("-") if "-" in a.clip_s else (a.clip_s, a.clip_s)))
    pcms = [synth.clip(c, int(16000 * (lo + (hi - lo) * (c * 7 % a.clips) / max(1, a.clips - 1)))) for c in range(a.clips)]
    gate = None
    if a.vad_mode != "always":
        pattern = ((20, 0.0), (60, 1.0), (30, 0.0), (40, 1.0), (50, 0.0))                    # frames on / off, as tests/silero_lib.speechlike
        env = np.concatenate([np.full(n * 512, v, np.float32) for n, v in pattern])
        pcms = [p * np.resize(env, p.size) for p in pcms]
        gate = {"vad_mode": a.vad_mode, "min_silence_duration_ms": 320, "emit_vad_events": True}
        if a.vad_mode in ("silero", "auto"):
            vad_model = a.vad_model
            if vad_model is None:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import make_synth_silero
                vad_model = "/tmp/skw_bench_plugin_silero.onnx"
                with open(vad_model, "wb") as f:
                    f.write(make_synth_silero.build(1234)[0])
            gate["vad_model_path"] = vad_model
        if a.vad_device is not None: gate["vad_device"] = a.vad_device
        if a.vad_batch_frames is not None: gate["vad_batch_frames"] = a.vad_batch_frames
    params = {"model_path": path, "vad_mode": "always", "flush_tail": True, "max_batch": a.clips, "batch_window_ms": a.batch_window_ms, "precision": a.precision,
              "mixed_batch": bool(a.mixed_batch)}
    if gate: params.update(gate)
    if a.audio_ctx is not None: params["audio_ctx"] = "auto" if a.audio_ctx == "auto" else int(a.audio_ctx)
    langs = ["en", "de", "es", "fr"]
    sets = [{"language": langs[k % 4], "suppress_non_speech_tokens": not (k // 4) & 1, "suppress_blank": not (k // 8) & 1} for k in range(a.param_sets)]
    best = None; walls = []; stats0 = None
    for rep in range(a.reps + 1):
        if rep == 1 and batch_stats: stats0 = batch_stats()
        nodes = [plug.create_node(dict(params, **sets[i % len(sets)])) for i in range(a.clips)]      # model load is cached per path (first create pays it; excluded, as in the reference)
        ms = C.c_double(minihost.run_oneshot(nodes, pcms, a.packet))
        outs = [n.outputs() for n in nodes]
        assert all(o[0][1] == 3 for o in outs if o) and (gate or all(len(o) == 1 for o in outs)), [len(o) for o in outs]
        n_cut = sum(sum(1 for t in n.telemetry() if t[0] == "vad.speech_end") for n in nodes) if gate else len(nodes)
        for n in nodes: n.destroy()
        if rep > 0: best = ms.value if best is None else min(best, ms.value); walls.append(round(ms.value, 2))     # rep 0 = warm-up
    audio_s = sum(p.size for p in pcms) / 16000.0
    n_seg = sum(len(json.loads(x[2].decode())["segments"]) for o in outs for x in o)
    gate_report = None
    if gate:
        gate_report = {"vad_mode": a.vad_mode, "vad_device": a.vad_device, "vad_batch_frames": a.vad_batch_frames, "segments_cut": n_cut, "transcription_packets": sum(len(o) for o in outs)}
        if "vad_model_path" in gate:       # the libm gate of the driven tree's libskw_vad.so over every clip, 16 threads, outside the timed region
            from concurrent.futures import ThreadPoolExecutor
            L = C.CDLL(os.path.join(tree, "streamkit_amd", "libskw_vad.so"))
            L.skw_vad_create.restype = C.c_void_p; L.skw_vad_create.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
            L.skw_vad_process_chunk.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]; L.skw_vad_free.argtypes = [C.c_void_p]
            def speech_frames(p):
                h = L.skw_vad_create(gate["vad_model_path"].encode(), None, 0); pr = C.c_float(); k = 0
                for i in range(p.size // 512):
                    L.skw_vad_process_chunk(h, p[i * 512:].ctypes.data, C.byref(pr)); k += pr.value >= 0.5
                L.skw_vad_free(h); return k
            with ThreadPoolExecutor(16) as ex: n_speech = sum(ex.map(speech_frames, [np.ascontiguousarray(p) for p in pcms]))
            n_frames = sum(p.size // 512 for p in pcms)
            gate_report.update(speech_frame_share=round(n_speech / n_frames, 4), transcribed_audio_s=round(n_speech * 0.032, 1))
    print(json.dumps({"what": "plugin-level Oneshot batch (host PCM -> Transcription JSON), %d instances" % a.clips, "value": round(audio_s / (best * 1e-3), 1), "unit": "x real-time",
                      "wall_ms": round(best, 2), "packet_samples": a.packet, "batch_window_ms": a.batch_window_ms, "segments": n_seg, "model": a.size, "precision": a.precision,
                      "wall_ms_reps": walls, "param_sets": a.param_sets, "mixed_batch": a.mixed_batch, "audio_ctx": a.audio_ctx, "clip_s": a.clip_s,
                      "batch_stats": dict(zip(("engine_calls", "jobs", "mixed_calls"), [x - y for x, y in zip(batch_stats(), stats0)])) if batch_stats else None,
                      "gate": gate_report, "tree": os.path.relpath(tree, ROOT)}))


if __name__ == "__main__":
    main()
