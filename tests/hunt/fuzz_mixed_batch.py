"""The Whisper node under arrival timings (mixed batches as a scheduler forms them): the fourteen differently configured instances of test_gpu_plugin.py's threaded stress test
(same seed, same clips and parameters, one f16_mfma engine beside the exact one, an instance dropped and re-created mid-way), run [rounds] times with seeded arrival delays drawn from
0 / 5 / 50 / 200 ms.  Every exact instance against the oracle's transcript for its audio and parameters, every f16_mfma instance against the packets the same configuration emits alone
(whole JSON).  Prints, per round, the node's batch counters (engine calls, jobs, mixed calls), every error string and every differing instance with what differs.
usage: python tests/hunt/fuzz_mixed_batch.py [rounds=10] [seed=100]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import synth_model
from oracle_lib import OracleModel
from streamkit_amd import engine as eng, synth
path = synth_model("tiny"); om = OracleModel(path)
rng = np.random.default_rng(33); jobs = []; cfgs = []
for i in range(14):
    pcm = synth.clip(40 + i, int(16000 * rng.choice([4, 9, 17, 30])))
    bw = int(rng.choice([0, 2, 20])); mb = int(rng.choice([1, 4, 64]))
    sb = bool(rng.integers(0, 2)); nst = bool(rng.integers(0, 2)); lang = str(rng.choice(["en", "de", "auto"]))
    jobs.append(dict(pcm=pcm, sb=int(sb), nst=int(nst), lang={"en": 0, "de": 2, "auto": -1}[lang], f16=(i % 5 == 4)))
    cfgs.append(({"model_path": path, "vad_mode": "always", "flush_tail": True, "batch_window_ms": bw, "max_batch": mb, "suppress_blank": sb, "suppress_non_speech_tokens": nst,
                  "language": lang, "precision": "f16_mfma" if i % 5 == 4 else "exact"}, int(rng.choice([480, 960, 1920, 4000])), float(rng.uniform(0, 0.05))))
def P(x, j):
    p = x.default_params(); p.suppress_blank = j["sb"]; p.suppress_nst = j["nst"]; p.lang_id = j["lang"]; return p
def key(r):
    return ([(t[0], t[1], np.float32(t[3]).view(np.uint32)) for t in r["tokens"]], [(s["t0"], s["t1"], s["text"]) for s in r["segments"]], r["n_windows"], r["lang_id"], r["fallback_requested"])
t0 = time.time()
want = [key(om.full(j["pcm"], P(om, j))) for j in jobs]
print("oracle done %.0f s; jobs:" % (time.time() - t0),
      [(k, j["pcm"].size // 16000, j["sb"], j["nst"], j["lang"], j["f16"], len(want[k][0]), want[k][2], want[k][4]) for k, j in enumerate(jobs)], flush=True)

import json, threading
from streamkit_amd import minihost
plugin = minihost.Plugin()
def feed(node, pcm, packet):
    for i in range(0, pcm.size, packet):
        assert node.process_audio(pcm[i:i + packet]) == 0, node.last_error()
def alone(cfg, pcm):
    node = plugin.create_node(cfg); feed(node, pcm, 960); assert node.flush() == 0
    out = [json.loads(bytes(o[2]).decode()) for o in node.outputs()]; node.destroy(); return out
def want_json(k):
    segs = [{"text": s[2].decode().strip(), "start_time_ms": s[0] * 10, "end_time_ms": s[1] * 10, "confidence": None} for s in want[k][1] if s[2].decode().strip()]
    return segs
ref_f16 = {k: alone(cfgs[k][0], jobs[k]["pcm"]) for k in range(14) if jobs[k]["f16"]}
total_bad = 0
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 10; SEED = int(sys.argv[2]) if len(sys.argv) > 2 else 100
for variant in range(ROUNDS):
    vr = np.random.default_rng(SEED + variant)
    delays = [float(vr.uniform(0, [0.0, 0.005, 0.05, 0.2][variant % 4])) for _ in range(14)]
    results = [None] * 14; errors = []
    s0 = minihost.whisper_batch_stats()
    def worker(k):
        try:
            cfg, packet, _ = cfgs[k]
            time.sleep(delays[k])
            if k % 7 == 3:
                tmp = plugin.create_node(cfg); feed(tmp, jobs[k]["pcm"][:16000], packet); tmp.destroy()
            node = plugin.create_node(cfg); feed(node, jobs[k]["pcm"], packet); rc = node.flush()
            if rc != 0: errors.append((k, "flush", node.last_error()))
            results[k] = [json.loads(bytes(o[2]).decode()) for o in node.outputs()]; node.destroy()
        except Exception as e:
            errors.append((k, repr(e)))
    ths = [threading.Thread(target=worker, args=(k,)) for k in range(14)]
    [t.start() for t in ths]; [t.join() for t in ths]
    s1 = minihost.whisper_batch_stats(); bad = []
    for k in range(14):
        got = results[k]
        if got is None: bad.append((k, "no result")); continue
        if not jobs[k]["f16"]:
            segs = want_json(k)
            if len(got) != (1 if segs else 0): bad.append((k, "exact: packets", len(got)))
            elif segs and got[0]["segments"] != segs: bad.append((k, "exact: segments differ from the oracle", [s["text"][:12] for s in got[0]["segments"]][:3], [s["text"][:12] for s in segs][:3]))
            elif segs and got[0]["language"] != cfgs[k][0]["language"]: bad.append((k, "exact: language"))
        else:
            ref = ref_f16[k]
            if len(got) != len(ref): bad.append((k, "f16: packets", len(got), len(ref)))
            else:
                for a, b in zip(got, ref):
                    if a != b: bad.append((k, "f16: differs from alone", "n segments", len(a["segments"]), len(b["segments"]),
                                           "first start", a["segments"][0]["start_time_ms"], b["segments"][0]["start_time_ms"],
                                           "same text" if a["text"] == b["text"] else "text differs"))
    total_bad += len(bad) + len(errors)
    print("variant", variant, "stats (calls, jobs, mixed)", tuple(x - y for x, y in zip(s1, s0)), "errors", errors, "bad", bad, flush=True)
print("plugin-level hunt: %d findings" % total_bad, flush=True)
