"""Clips with different parameters in one batch (skw_full_batch_mixed), the part that needs no GPU: the ABI is there — the engine's entry points, the node's
`mixed_batch` parameter and its batch counters — and the Python binding refuses the combinations the engine does not offer before it touches the device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from streamkit_amd import engine, minihost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_and_node_export_the_mixed_batch_abi(built):
    L = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libskw_engine.so"))
    for sym in ("skw_full_batch_mixed", "skw_debug_sample_rows_mixed", "skw_full_batch", "skw_full_batch_rng", "skw_full_batch_traced"):
        assert hasattr(L, sym), sym
    props = minihost.Plugin().metadata["param_schema"]["properties"]
    assert props["mixed_batch"]["type"] == "boolean" and props["mixed_batch"]["default"] is True
    assert "(additive)" in props["mixed_batch"]["description"]
    # process-wide counters of the node's schedulers, in a process of their own: no job has run there (and reading them needs no GPU)
    out = subprocess.check_output([sys.executable, "-c", "from streamkit_amd import minihost; print(minihost.whisper_batch_stats())"], cwd=ROOT)
    assert out.decode().strip() == "(0, 0, 0)"


def _context_without_a_device():
    """A Context object that was never created on a device: whatever full_batch checks before its first library call can be tested with it."""
    ctx = engine.Context.__new__(engine.Context)
    ctx.h = None
    return ctx


def test_binding_refuses_per_clip_parameters_and_generators_with_tracing(built):
    import numpy as np
    ctx = _context_without_a_device()
    p = engine.FullParams(); engine.lib().skw_full_default_params(C.byref(p))
    pcm = [np.zeros(16000, np.float32)]
    with pytest.raises(ValueError, match="one FullParams"):
        ctx.full_batch(pcm, params=[p], trace=True)
    with pytest.raises(ValueError, match="one FullParams"):
        ctx.full_batch(pcm, params=[p], forced=[np.zeros(1, np.int32)])
    with pytest.raises(ValueError, match="rng_states"):
        ctx.full_batch(pcm, rng_states=[engine.rng_state_new()], trace=True)
    with pytest.raises(ValueError, match="rng_states"):
        ctx.full_batch(pcm, params=p, rng_states=[None], forced=[np.zeros(1, np.int32)])
    # one parameter block per clip, no more and no fewer
    with pytest.raises(ValueError, match="2 parameter blocks for 1 clips"):
        ctx.full_batch(pcm, params=[p, p])
    with pytest.raises(ValueError, match="parameter blocks for 2 rows"):
        ctx.sample_rows([[], []], np.zeros((2, 8), np.float32), params=[p])
