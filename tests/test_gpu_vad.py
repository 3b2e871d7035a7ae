"""The Silero gate on the GPU (skw_vad_gpu_process, streamkit_amd/csrc/skw_vad_gpu.hip) against the CPU contract evaluator: bit for bit,
no tolerance, because both evaluate the chains include/skw_silero_net.h states."""
import threading

import numpy as np
import pytest

import vad_contract_lib as vcl
from streamkit_amd import vad

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 63, 64, 65, 937]


def cpu_run(path, frames, state):
    """the CPU contract evaluator from a given 320-float state: (probabilities, new state)"""
    v = vad.CpuVad(path, vad.ARITH_CONTRACT)
    v.set_state(state)
    p = v.process_chunks(frames)
    s = v.get_state()
    v.close()
    return p, s


def make_streams(S, seed, nonzero_state, path):
    """S streams of unequal lengths (LENGTHS first, then seeded ones), each with its carried state"""
    rng = np.random.default_rng(seed)
    lens = (LENGTHS + [int(n) for n in rng.integers(0, 200, max(0, S - len(LENGTHS)))])[:S] if S >= len(LENGTHS) else {1: [65], 3: [0, 937, 64]}[S]
    frames, states = [], []
    for i, n in enumerate(lens):
        x = vcl.stream(seed * 100 + i, n + 12)
        st = np.zeros(320, np.float32)
        if nonzero_state:                       # a state some earlier audio really left behind
            _, st = cpu_run(path, x[:12 * 512], st)
        frames.append(x[12 * 512:]); states.append(st)
    return frames, states


@pytest.fixture(scope="module", params=vcl.MODEL_KINDS)
def model(request, built):
    path = vcl.model_path(request.param)
    g = vad.GpuVad(path, 0)
    yield path, g
    g.close()


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("nonzero_state", [False, True])
@pytest.mark.parametrize("S", [1, 3, 64])
def test_gpu_equals_cpu_contract_bit_for_bit(model, S, nonzero_state, poison):
    """poison: the test-only switch skw_vad_gpu_debug_alloc_poison fills every work buffer of the gate with NaNs before each call (SKW_TEST_ALLOC_POISON's
    mechanism lives in the engine's workspace allocator and does not reach these buffers)"""
    path, g = model
    frames, states = make_streams(S, 7 + S, nonzero_state, path)
    want = [cpu_run(path, f, s) for f, s in zip(frames, states)]
    vad.set_alloc_poison(poison)
    try:
        got_states = [s.copy() for s in states]
        probs = g.process(frames, got_states)
    finally:
        vad.set_alloc_poison(False)
    for i, ((wp, ws), gp, gs) in enumerate(zip(want, probs, got_states)):
        assert gp.shape == wp.shape
        assert np.array_equal(vcl.bits(gp), vcl.bits(wp)), "stream %d (%d frames): probabilities differ, first at frame %d" % (i, wp.size, int(np.argmax(vcl.bits(gp) != vcl.bits(wp))))
        assert np.array_equal(vcl.bits(gs), vcl.bits(ws)), "stream %d (%d frames): state differs" % (i, wp.size)
        if wp.size == 0:
            assert np.array_equal(vcl.bits(gs), vcl.bits(states[i]))


def test_call_cutting_does_not_change_anything(model):
    """the same streams in one call and cut into calls of random lengths (other streams idle or present in between)"""
    path, g = model
    rng = np.random.default_rng(21)
    frames = [vcl.stream(300 + i, n) for i, n in enumerate([937, 130, 64])]
    one_states = [np.zeros(320, np.float32) for _ in frames]
    one = g.process(frames, one_states)
    states = [np.zeros(320, np.float32) for _ in frames]
    pos = [0] * len(frames)
    parts = [[] for _ in frames]
    while any(p < f.size // 512 for p, f in zip(pos, frames)):
        n = [min(f.size // 512 - p, int(rng.integers(0, 90))) for p, f in zip(pos, frames)]
        out = g.process([f[p * 512:(p + k) * 512] for f, p, k in zip(frames, pos, n)], states)
        for i, o in enumerate(out):
            parts[i].append(o); pos[i] += n[i]
    for i in range(len(frames)):
        assert np.array_equal(vcl.bits(np.concatenate(parts[i])), vcl.bits(one[i]))
        assert np.array_equal(vcl.bits(states[i]), vcl.bits(one_states[i]))


def test_stream_alternates_between_cpu_and_gpu(model):
    path, g = model
    x = vcl.stream(41, 400)
    want, want_state = cpu_run(path, x, np.zeros(320, np.float32))
    rng = np.random.default_rng(4)
    state, pos, parts, on_gpu = np.zeros(320, np.float32), 0, [], True
    while pos < 400:
        n = min(400 - pos, int(rng.integers(1, 70)))
        chunk = x[pos * 512:(pos + n) * 512]
        if on_gpu:
            parts.append(g.process([chunk], [state])[0])
        else:
            p, state = cpu_run(path, chunk, state)
            parts.append(p)
        pos += n; on_gpu = not on_gpu
    assert np.array_equal(vcl.bits(np.concatenate(parts)), vcl.bits(want)) and np.array_equal(vcl.bits(state), vcl.bits(want_state))


def test_feed_forward_taps_equal_the_contracts(model):
    """STFT magnitudes, each conv block and b_ih + W_ih.x for 300 consecutive frames from a carried context"""
    path, g = model
    x = vcl.stream(51, 310)
    _, st = cpu_run(path, x[:10 * 512], np.zeros(320, np.float32))
    got = g.feed_forward_taps(x[10 * 512:], st)
    v = vad.CpuVad(path, vad.ARITH_CONTRACT)
    v.set_state(st)
    for i in range(300):
        fr = x[(10 + i) * 512:(11 + i) * 512]
        want = v.feed_forward_taps(fr)
        for k, _ in vad.TAP_SHAPES:
            assert np.array_equal(vcl.bits(got[k][i]), vcl.bits(want[k])), "frame %d, stage %s: %d of %d elements differ" % (i, k, int((vcl.bits(got[k][i]) != vcl.bits(want[k])).sum()), want[k].size)
        v.process_chunk(fr)                     # advances the context
    v.close()


def test_more_frames_than_one_feed_forward_chunk(model):
    """20 000 frames in one call cross the 8192-frame chunks the intermediates are kept for; spot-checked against the CPU on whole streams"""
    path, g = model
    base = vcl.stream(61, 2500)
    frames = [np.roll(base, 512 * 37 * i) for i in range(8)]
    states = [np.zeros(320, np.float32) for _ in frames]
    probs = g.process(frames, states)
    for i in (0, 3, 7):                         # streams 3 and 7 straddle a chunk boundary (frames 7500..10000, 17500..20000)
        wp, ws = cpu_run(path, frames[i], np.zeros(320, np.float32))
        assert np.array_equal(vcl.bits(probs[i]), vcl.bits(wp)) and np.array_equal(vcl.bits(states[i]), vcl.bits(ws))


def test_many_threads_share_one_gate(model):
    path, g = model
    inputs = [vcl.stream(500 + i, 40 + 9 * i) for i in range(12)]
    want = [cpu_run(path, x, np.zeros(320, np.float32)) for x in inputs]
    got, errors = [None] * len(inputs), []

    def work(i):
        try:
            st, parts = np.zeros(320, np.float32), []
            for a in range(0, inputs[i].size // 512, 16):
                parts.append(g.process([inputs[i][a * 512:(a + 16) * 512]], [st])[0])
            got[i] = (np.concatenate(parts), st)
        except Exception as e:                  # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(len(inputs))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for (wp, ws), (gp, gs) in zip(want, got):
        assert np.array_equal(vcl.bits(gp), vcl.bits(wp)) and np.array_equal(vcl.bits(gs), vcl.bits(ws))


def test_create_destroy_does_not_grow_device_memory(built):
    import torch
    path = vcl.model_path("cell")
    x = vcl.stream(71, 300)

    def cycle():
        g = vad.GpuVad(path, 0)
        g.process([x, x[:64 * 512]], [np.zeros(320, np.float32), np.zeros(320, np.float32)])
        g.close()
    for _ in range(3):
        cycle()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < (8 << 20), "device memory shrank by %d bytes over 20 create / destroy cycles" % (free0 - free1)


def test_error_paths(built, tmp_path):
    with pytest.raises(RuntimeError, match=r"Failed to load VAD model from '/nonexistent/silero.onnx': cannot open file"):
        vad.GpuVad("/nonexistent/silero.onnx", 0)
    bad = tmp_path / "bad.onnx"
    data = open(vcl.model_path("cell"), "rb").read()
    bad.write_bytes(data[:len(data) // 2])
    with pytest.raises(RuntimeError, match=r"Failed to load VAD model from '.*bad.onnx': "):
        vad.GpuVad(str(bad), 0)
    with pytest.raises(RuntimeError, match=r"device 99 out of range \(\d+ HIP devices?\)"):
        vad.GpuVad(vcl.model_path("cell"), 99)
    with pytest.raises(RuntimeError, match="out of range"):
        vad.GpuVad(vcl.model_path("cell"), -1)
    g = vad.GpuVad(vcl.model_path("cell"), 0)
    assert g.process([], []) == []
    lib = vad.gpu_lib()
    import ctypes as C
    n = np.array([-1], np.int32)
    st = np.zeros(320, np.float32)
    sp = (C.c_void_p * 1)(st.ctypes.data); fp = (C.c_void_p * 1)(None); pp = (C.c_void_p * 1)(None)
    assert lib.skw_vad_gpu_process(g._h, 1, fp, n.ctypes.data, sp, pp) != 0 and b"stream 0" in lib.skw_vad_gpu_last_error(g._h)
    n[0] = 3                                    # frames announced, no pointer
    assert lib.skw_vad_gpu_process(g._h, 1, fp, n.ctypes.data, sp, pp) != 0
    x = vcl.stream(1, 5)                        # the object still works after refused calls
    assert g.process([x], [st])[0].shape == (5,)
    g.close()


# ------------------------------------------------------------------ the node: vad_device and vad_batch_frames
import json  # noqa: E402

import oracle_lib  # noqa: E402
from oracle_lib import OracleModel  # noqa: E402
from streamkit_amd import minihost  # noqa: E402


@pytest.fixture(scope="module")
def plugin():
    return minihost.Plugin()


def _expected_transcription(om, pcm_segment, start_ms, language="en"):
    """What lib.rs:648-695 builds from whisper.cpp's segments, computed from the oracle's full() (as tests/test_gpu_plugin.py does)."""
    po = om.default_params(); po.suppress_nst = 1
    r = om.full(pcm_segment, po)
    segs = []
    for s in r["segments"]:
        text = s["text"].decode().strip()
        if text:
            segs.append({"text": text, "start_time_ms": start_ms + s["t0"] * 10, "end_time_ms": start_ms + s["t1"] * 10, "confidence": None})
    return {"text": " ".join(s["text"] for s in segs), "segments": segs, "language": language, "metadata": None} if segs else None


def node_pcm():
    """~19 s: three stretches the engineered gate opens on, pauses between them"""
    import silero_lib
    return silero_lib.speechlike(600, seed=2, pattern=((20, 0.0), (150, 0.25), (40, 0.0), (100, 0.2), (45, 0.0), (170, 0.22), (75, 0.0)))


def run_node(plugin, cfg, pcm, packets, update=None):
    """update = (sample position, params): update_params is called when exactly that many samples have been fed"""
    node = plugin.create_node(cfg); pos = 0
    for n in packets:
        n = min(n, pcm.size - pos)
        if update and pos <= update[0] < pos + n:
            head = update[0] - pos
            assert node.process_audio(pcm[pos:pos + head]) == 0, node.last_error()
            assert node.update_params(update[1]) == 0, node.last_error()
            pos += head; n -= head; update = None
        assert node.process_audio(pcm[pos:pos + n]) == 0, node.last_error()
        pos += n
    assert pos == pcm.size and node.flush() == 0, node.last_error()
    out = ([(o[0], o[1], bytes(o[2])) for o in node.outputs()], node.telemetry(), node.logs())
    node.destroy()
    return out


def test_node_gpu_gate_equals_ground_truth_for_every_batch_size_and_packet_cutting(plugin, tiny_model_path):
    om = OracleModel(tiny_model_path)
    vad_path = vcl.model_path("cell")
    pcm = node_pcm()
    base = {"model_path": tiny_model_path, "vad_mode": "silero", "vad_model_path": vad_path, "vad_device": "gpu", "min_silence_duration_ms": 320, "emit_vad_events": True}
    # ground truth: CPU contract evaluator + the oracle's state machine + the oracle's transcription of the cut samples
    prob = vad.CpuVad(vad_path, vad.ARITH_CONTRACT).process_chunks(pcm)
    cuts = oracle_lib.segment_sim(prob, 0.5, 320, 30.0)
    assert len(cuts) == 3 and all(c[3] == 1 for c in cuts)
    speech_frames = np.flatnonzero(prob >= 0.5)
    ref = run_node(plugin, dict(base, vad_batch_frames=1), pcm, [960] * 400)
    assert len(ref[0]) == 3
    pos = 0
    for (start_ms, end_ms, n_samples, _, _, _), out in zip(cuts, ref[0]):
        idx = speech_frames[pos:pos + n_samples // 512]; pos += n_samples // 512
        seg = np.concatenate([pcm[i * 512:(i + 1) * 512] for i in idx])
        assert idx[0] * 32 == start_ms
        assert json.loads(out[2].decode()) == _expected_transcription(om, seg, start_ms)
    starts = [t[1] for t in ref[1] if t[0] == "vad.speech_start"]
    ends = [t[1] for t in ref[1] if t[0] == "vad.speech_end"]
    assert [s["start_time_ms"] for s in starts] == [c[0] for c in cuts] and [e["end_time_ms"] for e in ends] == [c[1] for c in cuts]
    assert [np.float32(s["speech_probability"]) for s in starts] == [prob[c[0] // 32] for c in cuts]          # the contract's probability, exactly
    rng = np.random.default_rng(21)
    for N in (1, 16, 256):
        for trial in range(2):
            got = run_node(plugin, dict(base, vad_batch_frames=N), pcm, vcl.random_packets(rng, pcm.size))
            assert got[0] == ref[0] and got[1] == ref[1], (N, trial)
    # and the CPU device with frames held back: the libm gate, whose decisions agree with the contract's away from the threshold (test_cpu_vad_contract) — same cuts here
    cpu = run_node(plugin, dict(base, vad_device="cpu", vad_batch_frames=16), pcm, [960] * 400)
    cpu1 = run_node(plugin, dict(base, vad_device="cpu"), pcm, [960] * 400)
    assert cpu[0] == cpu1[0] and cpu[1] == cpu1[1] and cpu[0] == ref[0]


def test_node_with_energy_gate_logs_vad_device_as_unused(plugin, tiny_model_path):
    pcm = node_pcm()[:100 * 512]
    a = run_node(plugin, {"model_path": tiny_model_path, "vad_mode": "energy", "vad_device": "gpu", "vad_batch_frames": 16, "flush_tail": True}, pcm, [960] * 100)
    b = run_node(plugin, {"model_path": tiny_model_path, "vad_mode": "energy", "flush_tail": True}, pcm, [960] * 100)
    assert any("vad_device" in l and "unused" in l for l in a[2]) and a[0] == b[0] and len(a[0]) >= 1


@pytest.mark.parametrize("change", [{"vad_batch_frames": 1}, {"vad_batch_frames": 64}, {"vad_threshold": 0.9}, {"vad_threshold": 0.9, "vad_batch_frames": 3}, {"vad_device": "cpu"}])
def test_node_update_params_in_mid_stream_equals_the_unbatched_run(plugin, tiny_model_path, change):
    pcm = node_pcm()
    base = {"model_path": tiny_model_path, "vad_mode": "silero", "vad_model_path": vcl.model_path("cell"), "vad_device": "gpu", "min_silence_duration_ms": 320, "emit_vad_events": True}
    at = 512 * 207 + 130                                  # inside the first stretch of speech, not on a frame boundary
    rng = np.random.default_rng(22)
    upd = dict(base, **change)
    ref = run_node(plugin, dict(base, vad_batch_frames=1), pcm, [960] * 400, update=(at, dict(upd, vad_batch_frames=1)))
    assert len(ref[0]) >= 2
    for N in (16, 256):
        got = run_node(plugin, dict(base, vad_batch_frames=N), pcm, vcl.random_packets(rng, pcm.size), update=(at, dict({"vad_batch_frames": N}, **upd)))
        assert got[0] == ref[0] and got[1] == ref[1], (N, change)


def test_twenty_instances_on_threads_each_equal_their_own_single_run(plugin, tiny_model_path):
    import silero_lib
    vad_path = vcl.model_path("cell")
    cfgs, pcms = [], []
    for i in range(20):
        cfgs.append({"model_path": tiny_model_path, "vad_mode": "silero", "vad_model_path": vad_path, "vad_device": "gpu" if i % 2 else "cpu",
                     "vad_batch_frames": [1, 5, 16, 64, 256][i % 5], "min_silence_duration_ms": 320, "emit_vad_events": True})
        pcms.append(silero_lib.speechlike(300 + 10 * i, seed=100 + i, pattern=((10 + i, 0.0), (90, 0.25), (30, 0.0), (70 + i, 0.2), (40, 0.0))))
    single = [run_node(plugin, c, p, [960] * 400)[:2] for c, p in zip(cfgs, pcms)]
    assert all(len(s[0]) >= 2 for s in single)
    got, errors = [None] * 20, []

    def work(i):
        try:
            got[i] = run_node(plugin, cfgs[i], pcms[i], [960] * 400)[:2]
        except BaseException as e:              # noqa: BLE001
            errors.append((i, e))
    ts = [threading.Thread(target=work, args=(i,)) for i in range(20)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    for i in range(20):
        assert got[i] == single[i], i


def test_node_churn_with_the_gpu_gate_does_not_grow_device_memory(plugin, micro_model_path):
    import torch
    cfg = {"model_path": micro_model_path, "vad_mode": "silero", "vad_model_path": vcl.model_path("cell"), "vad_device": "gpu", "vad_batch_frames": 32, "flush_tail": True, "batch_window_ms": 1}
    pcm = node_pcm()[:200 * 512]

    def cycle():
        nodes = [plugin.create_node(cfg) for _ in range(4)]
        for n in nodes:
            for i in range(0, pcm.size, 960):
                assert n.process_audio(pcm[i:i + 960]) == 0
            assert n.flush() == 0 and len(n.outputs()) >= 1
        for n in nodes:
            n.destroy()
    keep = plugin.create_node(cfg)
    for _ in range(3):
        cycle()
    torch.cuda.synchronize(); free0 = torch.cuda.mem_get_info()[0]
    for _ in range(30):
        cycle()
    torch.cuda.synchronize(); free1 = torch.cuda.mem_get_info()[0]
    keep.destroy()
    assert free0 - free1 < 64 << 20, "device memory shrank by %.1f MB over 120 instances" % ((free0 - free1) / 2 ** 20)


def test_node_error_paths(plugin, tiny_model_path, tmp_path):
    with pytest.raises(RuntimeError) as e:
        plugin.create_node({"model_path": tiny_model_path, "vad_mode": "silero", "vad_device": "gpu", "vad_model_path": str(tmp_path / "nope.onnx")})
    assert "Failed to initialize VAD: Failed to load VAD model from '%s'" % (tmp_path / "nope.onnx") in str(e.value)
    node = plugin.create_node({"model_path": tiny_model_path, "vad_mode": "silero", "vad_model_path": vcl.model_path("cell")})
    assert node.update_params({"model_path": tiny_model_path, "vad_mode": "silero", "vad_device": "gpu", "vad_model_path": str(tmp_path / "nope.onnx")}) == -1
    assert node.last_error().startswith("Failed to reload VAD: Failed to load VAD model from")
    assert node.update_params({"model_path": tiny_model_path, "vad_mode": "silero", "vad_device": "tpu", "vad_model_path": vcl.model_path("cell")}) == -1
    assert "vad_device" in node.last_error()
    node.destroy()
