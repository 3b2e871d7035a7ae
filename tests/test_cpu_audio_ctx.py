"""Per-clip audio context (skw_full_params.audio_ctx), the part that needs no GPU: the checker's model rewrite M'(K) (tests/audio_ctx_lib.py) is what it claims to be and the
oracle decodes it; the exported "auto" rule; the ABI field and the node's parameter are there."""
import ctypes as C
import filecmp
import os

import numpy as np
import pytest

from streamkit_amd import engine, minihost, synth
import audio_ctx_lib
from audio_ctx_lib import audio_ctx_model, scaled_max_initial_ts, tid0, write_audio_ctx_model
from oracle_lib import OracleModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rewrite_at_the_models_own_context_is_the_identity(micro_model_path, tmp_path):
    dst = str(tmp_path / "same.bin")
    nc = write_audio_ctx_model(micro_model_path, dst, 1500)
    assert nc == 1500 and filecmp.cmp(micro_model_path, dst, shallow=False)


def test_rewrite_cuts_the_positional_embedding_to_a_prefix(micro_model_path):
    from ggml_reader import read_ggml
    hp0, f0, v0, t0 = read_ggml(micro_model_path)
    hp1, f1, v1, t1 = read_ggml(audio_ctx_model(micro_model_path, 17))
    assert hp1["n_audio_ctx"] == 17 and {k: v for k, v in hp1.items() if k != "n_audio_ctx"} == {k: v for k, v in hp0.items() if k != "n_audio_ctx"}
    assert np.array_equal(f0, f1) and v0 == v1 and list(t0) == list(t1)
    for name in t0:
        if name == "encoder.positional_embedding":
            assert t1[name].shape == (17, hp0["n_audio_state"]) and np.array_equal(t1[name].view(np.uint32), t0[name][:17].view(np.uint32))
        else:
            assert t0[name].dtype == t1[name].dtype and np.array_equal(t0[name].view(np.uint8), t1[name].view(np.uint8)), name


def test_oracle_loads_and_decodes_the_rewritten_model(micro_model_path):
    """... and the transcript depends on K, so a comparison against it discriminates"""
    pcm = synth.clip(5, n_samples=16000 * 3)
    seen = {}
    for K in (1, 17, 100, 750):
        om = OracleModel(audio_ctx_model(micro_model_path, K))
        assert om.hp.n_audio_ctx == K
        p = om.default_params(); p.max_initial_ts = scaled_max_initial_ts(1.0, 1500, K)
        r = om.full(pcm, p)
        assert r["n_windows"] == 1 and len(r["tokens"]) > 0
        mel, _ = om.log_mel(pcm)
        enc, ck, cv = om.encode(mel)
        assert enc.shape == (K, om.hp.n_audio_state) and ck.shape == (om.hp.n_text_layer, K, om.hp.n_text_state) and np.isfinite(enc).all() and np.isfinite(ck).all()
        seen[K] = tuple(t[0] for t in r["tokens"])
        om.close()
    assert len(set(seen.values())) > 1, seen


def test_scaled_max_initial_ts_bans_the_same_ids():
    """the engine keeps the model's 0.02 s precision (id 50 at the default 1.0 s); the oracle on M'(K), whose precision is 30 / K, is handed the value that gives the same id"""
    assert tid0(1.0, 1500) == 50
    for K in (1, 17, 32, 100, 129, 256, 750, 1499, 1500):
        assert tid0(scaled_max_initial_ts(1.0, 1500, K), K) == 50, K
    assert scaled_max_initial_ts(0.0, 1500, 17) == 0.0      # 0 disables the rule on both sides


def test_auto_rule_on_a_table_of_sample_counts(built):
    nc = 1500
    table = {0: 32, 1: 32, 319: 32, 320: 32, 64000: 256, 471999: 1500, 480000: 1500, 480001: 1500, 16000 * 120: 1500}
    prev = 0
    for n, want in sorted(table.items()):
        k = engine.audio_ctx_for_samples(n, nc)
        assert k == want, (n, k, want)
        assert k % 32 == 0 or k == nc
        assert k * 320 >= min(n, 480000) or k == nc            # covers the audio (a position is 320 samples)
        assert k >= prev; prev = k
    ks = [engine.audio_ctx_for_samples(n, nc) for n in range(0, 500000, 997)]
    assert all(a <= b for a, b in zip(ks, ks[1:])) and all(k % 32 == 0 or k == nc for k in ks)
    assert all(k >= min(nc, -(-n // 320) + 25) for n, k in zip(range(0, 500000, 997), ks))      # half a second of margin wherever the cap allows it
    assert engine.audio_ctx_for_samples(64000, 100) == 100 and engine.audio_ctx_for_samples(10 ** 7, 448) == 448      # never more than the model's context


def test_full_params_has_the_field_and_it_defaults_to_zero(built):
    p = engine.FullParams()
    p.audio_ctx = 123                                        # (default_params must write it)
    engine.lib().skw_full_default_params(C.byref(p))
    assert p.audio_ctx == 0
    assert engine.FullParams._fields_[-1][0] == "audio_ctx" and C.sizeof(engine.FullParams) == 60      # last field; the struct grew by four bytes
    L = C.CDLL(os.path.join(ROOT, "streamkit_amd", "libskw_engine.so"))
    for sym in ("skw_audio_ctx_for_samples", "skw_conv_stem_actx", "skw_encode_actx", "skw_conv_stem", "skw_encode", "skw_decode_logits"):
        assert hasattr(L, sym), sym


def test_node_schema_lists_audio_ctx(built):
    props = minihost.Plugin().metadata["param_schema"]["properties"]
    assert props["audio_ctx"]["default"] == 0 and props["audio_ctx"]["type"] == ["integer", "string"]
    assert "(additive)" in props["audio_ctx"]["description"] and "auto" in props["audio_ctx"]["description"]
