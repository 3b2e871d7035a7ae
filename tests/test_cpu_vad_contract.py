"""The Silero gate's contract arithmetic (include/skw_silero_net.h) on the CPU: how far it lies from the existing libm gate, and
that its C ABI (skw_vad_create_ex, skw_vad_process_chunks, the 320-float state block) behaves."""
import ctypes as C

import numpy as np
import pytest

import silero_lib
import vad_contract_lib as vcl
from streamkit_amd import vad

# Bounds: 4 x the largest difference measured between the contract evaluator and the libm gate (the reference for these numbers)
# over the inputs of test_contract_stays_close_to_the_libm_gate — 3 model files x 6 streams x 1000 frames.  Measured maxima:
#   |dp| 3.58e-7   |dh| 1.07e-6   |dc| 8.58e-6
# The last-bit differences of expf / tanhf / fma-vs-mul-add vary with the input; the factor 4 covers streams outside the
# measured set, and a real mistake (a wrong coefficient, a swapped gate, a shifted tap) is orders of magnitude larger.  |dc| is
# the largest because c is not bounded by 1: on the random-LSTM file it reaches 13, where one ulp is 9.5e-7.
BOUND_P, BOUND_H, BOUND_C = 4 * 3.58e-7, 4 * 1.07e-6, 4 * 8.58e-6
N_STREAMS, N_FRAMES = 6, 1000


@pytest.mark.parametrize("kind", vcl.MODEL_KINDS)
def test_contract_stays_close_to_the_libm_gate(built, kind):
    path = vcl.model_path(kind)
    max_p = max_h = max_c = 0.0
    near = flips = mid = speech = 0
    for seed in range(N_STREAMS):
        x = vcl.stream(seed, N_FRAMES)
        a, b = vad.CpuVad(path, vad.ARITH_LIBM), vad.CpuVad(path, vad.ARITH_CONTRACT)
        for i in range(N_FRAMES):
            pa, pb = a.process_chunk(x[i * 512:(i + 1) * 512]), b.process_chunk(x[i * 512:(i + 1) * 512])
            sa, sb = a.get_state(), b.get_state()
            assert np.array_equal(sa[:64], sb[:64])
            max_p = max(max_p, abs(float(pa) - float(pb)))
            max_h = max(max_h, float(np.abs(sa[64:192] - sb[64:192]).max()))
            max_c = max(max_c, float(np.abs(sa[192:] - sb[192:]).max()))
            mid += 0.1 < pa < 0.9
            speech += pa >= 0.5
            if abs(float(pa) - 0.5) <= BOUND_P:
                near += 1                                      # excluded from the decision comparison
            elif (pa >= 0.5) != (pb >= 0.5):
                flips += 1
        a.close(); b.close()
    total = N_STREAMS * N_FRAMES
    print("\n[%s] contract vs libm over %d frames: max|dp| %.3g  max|dh| %.3g  max|dc| %.3g;  %d frames with 0.1 < p < 0.9, %d judged speech, %d within %.3g of the threshold"
          % (kind, total, max_p, max_h, max_c, mid, speech, near, BOUND_P))
    assert max_p <= BOUND_P and max_h <= BOUND_H and max_c <= BOUND_C
    assert flips == 0, "a decision at threshold 0.5 differs away from the threshold"
    assert near <= total // 100, "more than 1 % of the frames lie within the bound of the threshold: choose other seeds"
    assert mid >= total // 10 and 0 < speech < total, "the streams do not exercise the middle of the range"


def test_contract_sigmoid_and_tanh_error():
    """The absolute error include/skw_silero_net.h states for its tanh (2.5e-7) and what follows for the sigmoid, against float64."""
    L = vad.cpu_lib()
    L.skw_vad_debug_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    rng = np.random.default_rng(5)
    v = np.concatenate([np.linspace(-20, 20, 400001), rng.normal(0, 1e-3, 100000), rng.normal(0, 1, 200000), [0.0, -0.0, 1e-30, -1e-30, 50.0, -50.0, 1e30, -1e30, np.inf, -np.inf]]).astype(np.float32)
    out = np.zeros_like(v)
    L.skw_vad_debug_math(1, v.ctypes.data, out.ctypes.data, v.size)
    err_t = np.abs(out.astype(np.float64) - np.tanh(v.astype(np.float64))).max()
    assert np.array_equal(np.signbit(out), np.signbit(v)) and np.abs(out).max() <= 1.0
    L.skw_vad_debug_math(0, v.ctypes.data, out.ctypes.data, v.size)
    with np.errstate(over="ignore"):
        err_s = np.abs(out.astype(np.float64) - 1.0 / (1.0 + np.exp(-v.astype(np.float64)))).max()
    print("\ncontract tanh max abs error %.3g, sigmoid %.3g" % (err_t, err_s))
    assert err_t < 2.5e-7 and err_s < 2.5e-7


@pytest.mark.parametrize("kind", vcl.MODEL_KINDS)
@pytest.mark.parametrize("arith", [vad.ARITH_LIBM, vad.ARITH_CONTRACT])
def test_process_chunks_is_n_calls_of_process_chunk(built, kind, arith):
    path = vcl.model_path(kind)
    x = vcl.stream(11, 150)
    one, many = vad.CpuVad(path, arith), vad.CpuVad(path, arith)
    p1 = np.array([one.process_chunk(x[i * 512:(i + 1) * 512]) for i in range(150)], np.float32)
    rng = np.random.default_rng(3)
    pm, pos = [], 0
    while pos < 150:
        n = min(150 - pos, int(rng.integers(0, 40)))
        pm.append(many.process_chunks(x[pos * 512:(pos + n) * 512])); pos += n
    assert np.array_equal(vcl.bits(p1), vcl.bits(np.concatenate(pm)))
    assert np.array_equal(vcl.bits(one.get_state()), vcl.bits(many.get_state()))
    assert np.array_equal(one.get_state()[:64], x[150 * 512 - 64:150 * 512])


@pytest.mark.parametrize("arith", [vad.ARITH_LIBM, vad.ARITH_CONTRACT])
def test_state_round_trip_and_reset(built, arith):
    path = vcl.model_path("random_lstm")
    x = vcl.stream(12, 90)
    a = vad.CpuVad(path, arith)
    a.process_chunks(x[:40 * 512])
    s = a.get_state()
    assert s.shape == (320,) and np.abs(s[64:]).max() > 0
    rest = a.process_chunks(x[40 * 512:])
    end = a.get_state()
    b = vad.CpuVad(path, arith)
    b.process_chunks(x[:7 * 512])                       # some other history, overwritten by set_state
    b.set_state(s)
    assert np.array_equal(vcl.bits(b.get_state()), vcl.bits(s))
    assert np.array_equal(vcl.bits(b.process_chunks(x[40 * 512:])), vcl.bits(rest)) and np.array_equal(vcl.bits(b.get_state()), vcl.bits(end))
    b.reset()
    assert not b.get_state().any()
    fresh = vad.CpuVad(path, arith)
    assert np.array_equal(vcl.bits(b.process_chunks(x[:20 * 512])), vcl.bits(fresh.process_chunks(x[:20 * 512])))


def test_default_arithmetic_is_the_libm_gate(built):
    """skw_vad_create and skw_vad_create_ex(LIBM) are the gate tests/test_cpu_silero.py pins; the old 256-float state call agrees with the new block"""
    path = vcl.model_path("cell")
    x = vcl.stream(13, 60)
    old = silero_lib.ProductVad(path)
    new = vad.CpuVad(path, vad.ARITH_LIBM)
    po = np.array([old.process_chunk(x[i * 512:(i + 1) * 512]) for i in range(60)], np.float32)
    assert np.array_equal(vcl.bits(po), vcl.bits(new.process_chunks(x)))
    assert np.array_equal(vcl.bits(old.state().reshape(-1)), vcl.bits(new.get_state()[64:]))
    old.close()


def test_feed_forward_taps_are_the_evaluators_own(built):
    """gin + W_hh.h through the cell reproduces process_chunk: the taps are what the evaluator computes, not a second implementation"""
    path = vcl.model_path("random_lstm")
    x = vcl.stream(14, 30)
    a = vad.CpuVad(path, vad.ARITH_CONTRACT)
    a.process_chunks(x[:29 * 512])
    t = a.feed_forward_taps(x[29 * 512:])
    assert all(np.isfinite(v).all() for v in t.values()) and t["mag"].min() >= 0 and t["c4"].min() >= 0
    before = a.get_state()
    t2 = a.feed_forward_taps(x[29 * 512:])
    assert np.array_equal(vcl.bits(a.get_state()), vcl.bits(before)) and all(np.array_equal(vcl.bits(t[k]), vcl.bits(t2[k])) for k in t)
    assert t["c4"].max() > 0 and np.abs(t["gin"]).max() > 0


def test_create_ex_errors(built, tmp_path):
    with pytest.raises(RuntimeError, match=r"Failed to load VAD model from '/nonexistent/silero.onnx': cannot open file"):
        vad.CpuVad("/nonexistent/silero.onnx")
    with pytest.raises(RuntimeError, match="unknown arithmetic 7"):
        vad.CpuVad(vcl.model_path("cell"), 7)
    bad = tmp_path / "bad.onnx"
    data = open(vcl.model_path("cell"), "rb").read()
    bad.write_bytes(data[:len(data) // 2])
    with pytest.raises(RuntimeError, match="Failed to load VAD model from"):
        vad.CpuVad(str(bad))


# ------------------------------------------------------------------ the segmenter with vad_batch_frames (skw::Segmenter through mh_segment_run)
from streamkit_amd import minihost  # noqa: E402
import oracle_lib  # noqa: E402

BATCHES = [1, 7, 64, 1000]


random_packets = vcl.random_packets


def script_probs(rng, n):
    """stretches of speech and silence of random lengths, probabilities on both sides of 0.5, some long enough for a max_duration cut at 5 s"""
    p = []
    while len(p) < n:
        p += list(rng.uniform(0.55, 1.0, int(rng.integers(3, 260)))) + list(rng.uniform(0.0, 0.45, int(rng.integers(1, 60))))
    return np.array(p[:n], np.float32)


def what(events):
    """everything but the packet an event was handed over in (the one thing vad_batch_frames may change)"""
    return [tuple(e[k] for k in ("kind", "start_ms", "end_ms", "samples", "reason", "silence_ms", "counter", "extra")) for e in events]


def test_segmenter_scripted_gate_is_independent_of_batch_frames_and_packets(built):
    rng = np.random.default_rng(31)
    n_frames = 2500
    probs = script_probs(rng, n_frames)
    audio = rng.normal(0, 0.1, n_frames * 512 + 300).astype(np.float32)
    kw = dict(script=probs, min_silence_ms=300, max_secs=5.0, flush=2)
    ref = minihost.segment_run(audio, [960] * (audio.size // 960 + 1), batch_frames=1, **kw)
    cuts = [e for e in ref if e["kind"] == "cut"]
    assert len(cuts) >= 10 and {e["reason"] for e in cuts} == {0, 1} and ref[-1]["kind"] == "end"
    # the cuts are the ones the oracle's state machine makes of the same probabilities
    want = oracle_lib.segment_sim(probs, 0.5, 300, 5.0, max_cuts=1024)
    assert [(e["start_ms"], e["end_ms"], e["samples"], e["reason"], e["silence_ms"]) for e in cuts] == [tuple(c[:5]) for c in want]
    assert ref[-1]["start_ms"] == n_frames * 32 and ref[-1]["end_ms"] == 0 and ref[-1]["samples"] == 0           # flush drained: every frame consumed, none pending, none judged
    for N in BATCHES:
        for trial in range(3):
            got = minihost.segment_run(audio, random_packets(rng, audio.size), batch_frames=N, **kw)
            assert what(got) == what(ref), (N, trial)


def test_segmenter_without_flush_holds_back_less_than_one_batch(built):
    rng = np.random.default_rng(32)
    probs = script_probs(rng, 700)
    audio = rng.normal(0, 0.1, 700 * 512).astype(np.float32)
    ref = what(minihost.segment_run(audio, [960] * 400, batch_frames=1, script=probs, min_silence_ms=300, flush=0))
    for N in (7, 64):
        got = minihost.segment_run(audio, [960] * 400, batch_frames=N, script=probs, min_silence_ms=300, flush=0)
        end = got[-1]
        assert end["end_ms"] == 700 % N and end["start_ms"] == (700 - 700 % N) * 32          # pending frames < N, the clock stands at the last consumed frame
        assert what(got)[:-1] == ref[:len(got) - 1]                                          # a prefix of the N = 1 run: nothing differs, the rest is still held back
    # N = 1 hands every cut over in the packet that completes the deciding frame; N = 64 at most 63 frames later
    a = minihost.segment_run(audio, [512] * 700, batch_frames=1, script=probs, min_silence_ms=300, flush=1)
    b = minihost.segment_run(audio, [512] * 700, batch_frames=64, script=probs, min_silence_ms=300, flush=1)
    assert what(a) == what(b)
    late = [y["packet"] - x["packet"] for x, y in zip(a, b) if x["kind"] == "cut"]
    assert min(late) >= 0 and max(late) <= 63 and max(late) > 0


@pytest.mark.parametrize("kind", ["cell", "random_lstm"])
def test_segmenter_contract_gate_is_independent_of_batch_frames_and_packets(built, kind):
    rng = np.random.default_rng(33)
    path = vcl.model_path(kind)
    audio = np.concatenate([vcl.stream(80, 400), vcl.stream(81, 300)[:300 * 512 - 77]])
    kw = dict(silero_path=path, min_silence_ms=200, max_secs=4.0, flush=2)
    ref = minihost.segment_run(audio, [960] * (audio.size // 960 + 1), batch_frames=1, **kw)
    assert sum(e["kind"] == "cut" for e in ref) >= 3
    # ground truth: the CPU contract evaluator's probabilities through the oracle's state machine
    g = vad.CpuVad(path, vad.ARITH_CONTRACT)
    probs = g.process_chunks(audio[:audio.size // 512 * 512])
    want = oracle_lib.segment_sim(probs, 0.5, 200, 4.0, max_cuts=1024)
    assert [(e["start_ms"], e["end_ms"], e["samples"], e["reason"], e["silence_ms"]) for e in ref if e["kind"] == "cut"] == [tuple(c[:5]) for c in want]
    starts = [e for e in ref if e["kind"] == "start"]
    assert all(np.uint32(e["extra"]) == vcl.bits(probs[e["start_ms"] // 32:e["start_ms"] // 32 + 1])[0] for e in starts)
    for N in BATCHES:
        got = minihost.segment_run(audio, random_packets(rng, audio.size), batch_frames=N, **kw)
        assert what(got) == what(ref), N


@pytest.mark.parametrize("swap", [dict(swap_threshold=0.8), dict(swap_gate=True), dict(swap_gate=True, swap_threshold=0.3), dict(swap_batch_frames=5)])
def test_update_in_mid_stream_judges_pending_frames_by_the_old_gate_and_threshold(built, swap):
    rng = np.random.default_rng(34)
    n_frames = 1200
    probs, probs2 = script_probs(rng, n_frames), script_probs(rng, n_frames)
    audio = rng.normal(0, 0.1, n_frames * 512).astype(np.float32)
    at = 512 * 611 + 200                                 # 611 complete frames and 200 samples have arrived when the update comes
    kw = dict(script=probs, min_silence_ms=300, max_secs=5.0, flush=2, swap_at_sample=at, swap_script=probs2 if swap.get("swap_gate") else None, **swap)
    ref = minihost.segment_run(audio, [960] * 1000, batch_frames=1, **kw)
    # what must come out, from the rule alone: frames 0..610 by the old gate against 0.5, the rest by the gate and threshold in force afterwards
    t2 = swap.get("swap_threshold", 0.5)
    after = probs2[:n_frames - 611] if swap.get("swap_gate") else probs[611:]
    decisions = np.concatenate([probs[:611] >= 0.5, after >= np.float32(t2)]).astype(np.float32)
    want = oracle_lib.segment_sim(decisions, 0.5, 300, 5.0, max_cuts=1024)
    assert [(e["start_ms"], e["end_ms"], e["samples"], e["reason"], e["silence_ms"]) for e in ref if e["kind"] == "cut"] == [tuple(c[:5]) for c in want]
    for N in (7, 64, 1000):
        for trial in range(2):
            got = minihost.segment_run(audio, random_packets(rng, audio.size), batch_frames=N, **kw)
            assert what(got) == what(ref), (N, trial, swap)


@pytest.mark.parametrize("gate", ["script", "contract"])
def test_refused_cut_keeps_queue_and_gate_state_consistent(built, gate):
    """on_cut returning false ends push at once (an engine error in the node).  Frames already evaluated keep their probabilities, so the gate is asked for
    every frame exactly once and the stream goes on as in the N = 1 run with the same refusal."""
    rng = np.random.default_rng(35)
    if gate == "script":
        n_frames = 900
        audio = rng.normal(0, 0.1, n_frames * 512).astype(np.float32)
        kw = dict(script=script_probs(rng, n_frames), min_silence_ms=300, max_secs=5.0, flush=2)
    else:
        audio = vcl.stream(82, 500)
        kw = dict(silero_path=vcl.model_path("random_lstm"), min_silence_ms=200, max_secs=4.0, flush=2)
    clean = minihost.segment_run(audio, [960] * 1000, batch_frames=1, **kw)
    ref = minihost.segment_run(audio, [960] * 1000, batch_frames=1, abort_cut=1, **kw)
    assert [e["kind"] for e in ref].count("refused_cut") == 1
    # as in the reference (`?` leaves process() before the clock advances, lib.rs:464-493) the frame whose cut was refused does not advance the clock: 32 ms behind from there on
    assert ref[-1]["start_ms"] == clean[-1]["start_ms"] - 32 == audio.size // 512 * 32 - 32
    # the gate was asked for every frame exactly once, in order: the segments that start afterwards start on the same frames with the same probabilities
    assert [e["extra"] for e in ref if e["kind"] == "start"] == [e["extra"] for e in clean if e["kind"] == "start"]
    assert ref[-1]["end_ms"] == 0 and ref[-1]["samples"] == 0                       # nothing pending, nothing judged and unconsumed
    for N in (7, 64, 1000):
        got = minihost.segment_run(audio, random_packets(rng, audio.size), batch_frames=N, abort_cut=1, **kw)
        assert what(got) == what(ref), N


def test_node_schema_lists_the_new_keys_and_refuses_unknown_values(built):
    p = minihost.Plugin()
    props = p.metadata["param_schema"]["properties"]
    assert props["vad_device"]["default"] == "cpu" and props["vad_device"]["type"] == "string"
    assert props["vad_batch_frames"]["default"] == 1 and props["vad_batch_frames"]["minimum"] == 1 and props["vad_batch_frames"]["type"] == "integer"
    with pytest.raises(RuntimeError, match=r'Invalid config: vad_device must be "cpu" or "gpu"'):
        p.create_node({"vad_device": "npu"})
    with pytest.raises(RuntimeError, match="Invalid config: invalid type for `vad_device`, expected a string"):
        p.create_node({"vad_device": 1})
    for bad in (0, -3, 2.5, 100000):
        with pytest.raises(RuntimeError, match="Invalid config: vad_batch_frames must be an integer between 1 and 65536"):
            p.create_node({"vad_batch_frames": bad})
    with pytest.raises(RuntimeError, match="Invalid config: invalid type for `vad_batch_frames`, expected a number"):
        p.create_node({"vad_batch_frames": "many"})


def test_libraries_export_every_symbol_of_skw_vad_batch_h(built):
    import os
    from test_cpu_abi import _declared_functions
    from conftest import ROOT
    names = _declared_functions("skw_vad_batch.h")
    cpu = [n for n in names if not n.startswith("skw_vad_gpu_")]
    gpu = [n for n in names if n.startswith("skw_vad_gpu_")]
    assert "skw_vad_create_ex" in cpu and "skw_vad_process_chunks" in cpu and "skw_vad_gpu_process" in gpu and len(cpu) >= 7 and len(gpu) >= 7
    L = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libskw_vad.so"))
    for n in cpu:
        assert hasattr(L, n), "libskw_vad.so lacks %s" % n
    E = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libskw_engine.so"))
    for n in gpu:
        assert hasattr(E, n), "libskw_engine.so lacks %s" % n
