"""timestamp_granularity through the mini-host: one Whisper node instance with "word", one with the default, fed the same audio and flushed together.
The default instance's packets are the bytes a default instance gives on its own; the word instance's segments are the words streamkit_amd/csrc/skw_words.h cuts from the engine's
tokens (tests/cpp/align_main.cpp runs the header) with the engine's token times plus the cut's start; both jobs travelled in ONE engine call (skw_whisper_plugin_batch_stats)."""
import json
import threading

import pytest

import align_ref_lib as al
from streamkit_amd import engine, minihost, synth

pytestmark = pytest.mark.gpu


def _feed(node, pcm):
    for i in range(0, pcm.size, 960):
        assert node.process_audio(pcm[i:i + 960]) == 0, node.last_error()


def _feed_and_flush_together(nodes, pcms):
    barrier = threading.Barrier(len(nodes)); rcs = [None] * len(nodes); errors = []

    def worker(k):
        try:
            _feed(nodes[k], pcms[k])
            barrier.wait(timeout=120)
            rcs[k] = nodes[k].flush()
        except Exception as e:      # noqa: BLE001
            errors.append((k, repr(e))); barrier.abort()

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(len(nodes))]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errors, errors
    return rcs


def _words(tmp_path_factory, model, r):
    """the node's use of the word rule on an engine result: every text token with its own times; a token after a timestamp (or the first) opens a word"""
    toks, first = [], True
    for tok, (t0, t1) in zip(r["tokens"], r["token_times"]):
        if t0 < 0:
            first = True
            continue
        toks.append((model.token_bytes(tok[0]), t0, t1, first)); first = False
    return al.parse_words(al.run(al.driver(tmp_path_factory), [al.rec_words2(toks)])[0])


def test_word_and_default_instances_share_a_batch(tmp_path_factory, micro_model_path):
    plugin = minihost.Plugin()
    pcm = synth.clip(3, 16000 * 5)
    cfg = dict(model_path=micro_model_path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=300, max_batch=8)
    m = engine.Model(micro_model_path); ctx = engine.Context(m, max_batch=2, max_samples=16000 * 31)
    try:
        p = ctx.default_params(); p.lang_id = 0; p.suppress_blank = 1; p.suppress_nst = 1        # the node's parameters
        want = ctx.full_batch([pcm], [p], align=[engine.align_params(top=max(1, m.hp.n_text_layer // 2), hp=m.hp)])[0]
        words = _words(tmp_path_factory, m, want)
    finally:
        ctx.close(); m.close()
    assert len(words) >= 2, "the clip gives too few words for the test to show anything"
    raw = lambda nd: [bytes(o[2]) for o in nd.outputs()]
    alone = plugin.create_node(dict(cfg))
    _feed(alone, pcm); assert alone.flush() == 0, alone.last_error()
    nodes = [plugin.create_node(dict(cfg, timestamp_granularity="word")), plugin.create_node(dict(cfg))]
    before = minihost.whisper_batch_stats()
    assert _feed_and_flush_together(nodes, [pcm, pcm]) == [0, 0], [n.last_error() for n in nodes]
    calls, jobs, _ = (a - b for a, b in zip(minihost.whisper_batch_stats(), before))
    assert (calls, jobs) == (1, 2)
    assert raw(nodes[1]) == raw(alone) and len(raw(alone)) == 1                                 # the default instance: byte for byte what it gives without a word instance beside it
    plain = json.loads(raw(alone)[0].decode()); got = json.loads(raw(nodes[0])[0].decode())
    assert set(plain) == set(got) == {"text", "segments", "language", "metadata"} and got["text"] == plain["text"] and got["language"] == plain["language"]
    assert got["segments"] == [{"text": w[4].decode(), "start_time_ms": 10 * w[2], "end_time_ms": 10 * w[3], "confidence": None} for w in words]
    assert all(s["end_time_ms"] >= s["start_time_ms"] for s in got["segments"])
    # explicit heads and a bad value
    nd = plugin.create_node(dict(cfg, timestamp_granularity="word", alignment_heads=[[1, 0], [1, 1]]))      # = top:1 on the micro model
    _feed(nd, pcm); assert nd.flush() == 0, nd.last_error()
    assert json.loads(raw(nd)[0].decode())["segments"] == got["segments"]
    for bad in (dict(timestamp_granularity="syllable"), dict(alignment_heads="top:0"), dict(alignment_heads=[[0, 32]]), dict(alignment_heads=[])):
        with pytest.raises(RuntimeError):
            plugin.create_node(dict(cfg, **bad))
    for x in (nd, alone, *nodes):
        x.destroy()
