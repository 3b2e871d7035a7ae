"""Shared by tests/test_cpu_vad_contract.py and tests/test_gpu_vad.py: the three seeded Silero model files and the seeded streams."""
import os

import numpy as np

import silero_lib
import tools_path  # noqa: F401

import make_synth_silero  # noqa: E402

MODEL_KINDS = ("cell", "lstm_op", "random_lstm")      # LSTMCell tensors, ONNX LSTM operator tensors, seeded random LSTM with an open forget gate


def model_path(kind, seed=1234):
    path = "/tmp/skw_silero_contract_%s_%d.onnx" % (kind, seed)
    if not os.path.exists(path):
        data, _ = make_synth_silero.build(seed, lstm_op=kind == "lstm_op", random_lstm=kind == "random_lstm")
        with open(path + ".tmp%d" % os.getpid(), "wb") as f:
            f.write(data)
        os.replace(path + ".tmp%d" % os.getpid(), path)
    return path


def stream(seed, n_frames=1000):
    """speechlike() with seeded stretch lengths and amplitudes between -30 and -14 dBFS, where the engineered file's probabilities cross the middle of the range"""
    rng = np.random.default_rng(1000 + seed)
    amps = (0.0, 10 ** rng.uniform(-1.5, -0.7), 0.0, 10 ** rng.uniform(-1.5, -0.7), 10 ** rng.uniform(-1.4, -1.1), 0.0, 10 ** rng.uniform(-2.5, -1.0))
    pattern = tuple((int(rng.integers(5, 60)), float(a)) for a in amps)
    return silero_lib.speechlike(n_frames, seed=seed, pattern=pattern)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_packets(rng, total):
    """the size list of test_packetisation_does_not_change_what_comes_out"""
    cuts, left = [], total
    while left > 0:
        n = min(int(rng.choice([0, 1, 17, 511, 512, 513, 960, 1920, 4096, int(rng.integers(1, 7000))])), left)
        cuts.append(n); left -= n
    return cuts
