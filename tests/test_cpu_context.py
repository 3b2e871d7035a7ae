"""Initial prompts and carried context, the parts that need no GPU: the checker (tests/context_ref_lib.py) against the oracle's own whisper_full, the ABI additions, the
tokenizer (streamkit_amd/csrc/skw_tokenizer.h through a stand-alone program, plain and under the host sanitizers) and the node's schema."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import context_ref_lib as cr
import logit_rules_lib as lr
from conftest import ROOT, synth_model
from ggml_reader import read_ggml

CLIPS = {"c5": (5, 9 * 16000), "c21": (21, 3 * 16000), "c13": (13, 47 * 16000 + 123)}
_CACHE = {}


def _clip(name):
    from streamkit_amd import synth
    seed, n = CLIPS[name]
    return synth.clip(seed, n_samples=n)


def _empty(oracle_tiny, name):
    """the checker's result for the clip with no context: computed once, shared, never modified"""
    if name not in _CACHE:
        _CACHE[name] = cr.full_with_context(oracle_tiny, _clip(name), (), cr.params_for(oracle_tiny))
    return _CACHE[name]


# ---- (a) the checker is the oracle's whisper_full when nothing is handed in
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_checker_equals_oracle_full_without_context(oracle_tiny, name):
    ref = oracle_tiny.full(_clip(name), cr.params_for(oracle_tiny))
    got = _empty(oracle_tiny, name)
    assert ref["fallback_requested"] == 0 and got["failed_passes"] == 0
    assert cr.token_bits(got["tokens"]) == cr.token_bits(ref["tokens"])            # id, tid, p and plog bit for bit
    assert [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in got["segments"]] == [(s["t0"], s["t1"], s["tokens"], s["text"]) for s in ref["segments"]]
    assert got["n_windows"] == ref["n_windows"]
    if name == "c13":      # the case the debug hook alone gets wrong: the second window's first t0 comes from a text token's tid
        assert ref["n_windows"] == 2 and any(s["t0"] < 0 for s in ref["segments"])


# ---- (b) a context changes every clip's transcript (otherwise the GPU tests would show nothing)
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_context_changes_the_transcript(oracle_tiny, name):
    sp = lr.special_ids(oracle_tiny)
    ctxt = cr.make_context(np.random.default_rng(40), sp, 40)
    assert any(t > sp["beg"] for t in ctxt)
    got = cr.full_with_context(oracle_tiny, _clip(name), ctxt, cr.params_for(oracle_tiny))
    base = _empty(oracle_tiny, name)
    assert [t[0] for t in got["tokens"]] != [t[0] for t in base["tokens"]]
    # what the call leaves: the tokens the last prompt took, then that window's kept tokens
    assert len(got["context"]) > 0 and got["context"] != base["context"]
    if got["n_windows"] == 1:
        assert got["context"][:40] == ctxt


# ---- (c) the ABI additions
def test_abi_additions(built):
    from streamkit_amd import engine
    L = engine.lib()
    for sym in ("skw_full_batch_context", "skw_model_tokenize", "skw_debug_set_prompt_xattn_mq", "skw_debug_xattn_exact"):
        assert hasattr(L, sym), sym
    hdr = open(os.path.join(ROOT, "include", "skw_engine.h")).read()
    assert re.search(r"#define\s+SKW_CONTEXT_WORDS\s+513\b", hdr) and engine.CONTEXT_WORDS == 513
    assert C.sizeof(engine.FullParams) == 60                                       # the context travels beside the parameter block, not in it
    a = engine.context_new([7, 8, 9])
    assert a.dtype == np.int32 and a.size == 513 and a[0] == 3 and engine.context_ids(a) == [7, 8, 9]


# ---- (d) the tokenizer
_PATTERN = re.compile(rb"'s|'t|'re|'ve|'m|'ll|'d| ?[A-Za-z]+| ?[0-9]+| ?[^\sA-Za-z0-9]+|\s+(?!\S)|\s+")


def py_tokenize(vocab, n_text, text):
    """the rule of include/skw_engine.h (skw_model_tokenize) restated: regex words, then the longest entry at every position, one byte skipped where none starts; where two ids
    share a string the higher wins"""
    t2i = {}
    for i, s in enumerate(vocab[:n_text]):
        t2i[s] = i
    out = []
    for w in _PATTERN.findall(text):
        i = 0
        while i < len(w):
            for j in range(len(w), i, -1):
                if w[i:j] in t2i:
                    out.append(t2i[w[i:j]]); i = j
                    break
            else:
                i += 1
    return out


@pytest.fixture(scope="module")
def tiny_vocab(tiny_model_path):
    _, _, vocab, _ = read_ggml(tiny_model_path)
    return vocab, 50257                                                            # multilingual: <|endoftext|> = 50257, every BPE entry below it


def _cases(vocab):
    words = [v for v in vocab[2000:2400] if v[:1] != b" " and v.isalpha()][:6]
    spaced = [v for v in vocab[2000:2400] if v[:1] == b" "][:6]
    assert words and spaced
    cases = [b"", b" ", b"hello world", b" hello  world ", words[0] + spaced[0] + spaced[1], b" ".join(words), words[1] + words[2],
             b"12 345 6", b"a1b22c", b"I'll say we've won't it's they're I'm he'd", b"'llama 'sx", b"(( [[ --- -( >>> ))", b'say ("hi") --- ok', b" #tag @x ~",
             "♪♪ la ♪♪♪ 「q」".encode(), b"tail   ", b"two\n\nlines\t x \n", b"caf\xc3\xa9 \x01\x02 \xff ok", b"\xc3\xa9",
             b" ".join(spaced[:3]) + b"   " + words[3] * 3]
    out = [(c, 4096) for c in cases]
    out += [(b"hello world", 3), (b"hello world", 0), (b"I'll say we've", 1), (b"", 0)]       # cap too small: -needed, nothing past cap written
    return out


def _run_tokenizer(tmp_path, vocab, n_text, cases, sanitize):
    exe = tmp_path / ("tokenize_san" if sanitize else "tokenize")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "streamkit_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "tokenize_main.cpp")])
    vf, cf = tmp_path / "vocab.bin", tmp_path / "cases.bin"
    with open(vf, "wb") as f:
        f.write(struct.pack("<2i", n_text, len(vocab)))
        for v in vocab:
            f.write(struct.pack("<I", len(v))); f.write(v)
    with open(cf, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for text, cap in cases:
            f.write(struct.pack("<iI", cap, len(text))); f.write(text)
    out = subprocess.run([str(exe), str(vf), str(cf)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-2000:]
    return [[int(x) for x in ln.split()] for ln in out.stdout.decode().splitlines()]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tokenizer_matches_the_rule(tmp_path, tiny_vocab, sanitize):
    vocab, n_text = tiny_vocab
    cases = _cases(vocab)
    # (NUL cannot travel in a C string; none of the cases holds one)
    got = _run_tokenizer(tmp_path, vocab, n_text, cases, sanitize)
    assert len(got) == len(cases)
    seen_skip = seen_multi = False
    for (text, cap), line in zip(cases, got):
        want = py_tokenize(vocab, n_text, text)
        if len(want) > cap:
            assert line == [-len(want)], (text, cap, line)
        else:
            assert line == [len(want)] + want, (text, line, want)
        seen_skip = seen_skip or sum(len(vocab[i]) for i in want) < len(text)
        seen_multi = seen_multi or any(len(vocab[i]) > 2 for i in want)
    assert seen_skip and seen_multi                                                # a byte no entry starts with was skipped; a multi-byte entry won over its prefixes
    assert py_tokenize(vocab, n_text, b"") == [] and got[0] == [0]
    # the highest id wins where two ids share a string (the map's last assignment), and ids from <|endoftext|> up never come out of text
    dup = [b"ab", b"a", b"ab", b"b"]
    assert py_tokenize(dup, 4, b"ab") == [2] and py_tokenize(dup, 2, b"ab") == [0]
    assert _run_tokenizer(tmp_path, dup, 4, [(b"ab", 8)], False) == [[1, 2]] and _run_tokenizer(tmp_path, dup, 2, [(b"abb", 8)], False) == [[1, 0]]


# ---- (e) the node's schema
def test_node_schema_has_both_parameters(built):
    from streamkit_amd import minihost
    props = minihost.Plugin().metadata["param_schema"]["properties"]
    assert props["initial_prompt"]["type"] == "string" and props["initial_prompt"]["default"] == ""
    assert props["carry_context"]["type"] == "boolean" and props["carry_context"]["default"] is False
