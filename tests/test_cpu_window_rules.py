"""The engine's own statement of whisper_full_with_state's host rules (streamkit_amd/csrc/skw_window_rules.h: the token loop's update both samplers end in, the window's
output step, the temperature ladder, the prompt rule, the pass verdict, the prompt_past update, context check and write-back) without a GPU: tests/cpp/window_rules_main.cpp is
compiled against the header alone and run as a program of its own, plain and under the host sanitizers.  Held to the transformers-pinned fixture
(tests/golden/segment_rule_cases.json, all of it), to the oracle's skwo_debug_window under the parameters the fixture does not vary, and to short statements of each rule here."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import context_ref_lib as cr
import logit_rules_lib as lr
import segment_rules_lib as sr
from conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "segment_rule_cases.json")
N_TEXT_CTX = 448                      # the tiny synthetic model's (every Whisper's)
N_MAX = N_TEXT_CTX // 2 - 4           # 220
SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
_EXE = {}


def f32(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def vec(v):
    return [len(v)] + [int(x) for x in v]


def run_driver(tmp_path_factory, sanitize, records):
    """records: lists of int32 words (kind first) -> one list of output words per record"""
    if sanitize not in _EXE:
        exe = tmp_path_factory.mktemp("window_rules") / ("driver_san" if sanitize else "driver")
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "streamkit_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                               "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "window_rules_main.cpp")])
        _EXE[sanitize] = exe
    cf = tmp_path_factory.mktemp("cases") / "cases.bin"
    words = [len(records)] + [w for r in records for w in r]
    cf.write_bytes(struct.pack("<%di" % len(words), *words))
    out = subprocess.run([str(_EXE[sanitize]), str(cf)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode(errors="replace")[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == len(records)
    return lines


def window_record(sp, toks, seek, seek_end, max_tokens=0, no_timestamps=0, single_segment=0):
    return [0, sp["beg"], sp["eot"], N_MAX, max_tokens, no_timestamps, single_segment, seek, seek_end] + vec(toks)


def parse_window(line):
    w = [int(x) for x in line.split()]
    out = dict(failed=bool(w[0]), consumed=w[1], kept=w[2], advance=w[3], segments=[])
    k = 5
    for _ in range(w[4]):
        n = w[k + 2]
        out["segments"].append([w[k], w[k + 1], w[k + 3:k + 3 + n]])
        k += 3 + n
    assert k == len(w)
    return out


def same_window(got, want, what):
    """the equalities of the oracle's own fixture test: a failed pass is compared on `failed` and `consumed` only"""
    assert got["failed"] == want["failed"] and got["consumed"] == want["consumed"], what
    if not want["failed"]:
        assert (got["kept"], got["advance"]) == (want["kept"], want["advance"]), what
        assert got["segments"] == [[a, b, list(t)] for a, b, t in want["segments"]], what


# ---- 1. the fixture, every case
@SANITIZE
def test_engine_rules_reproduce_segment_rule_fixture(tmp_path_factory, sanitize):
    fx = json.load(open(FIXTURE))
    sp, cases = fx["special"], fx["cases"]
    assert len(cases) >= 400
    lines = run_driver(tmp_path_factory, sanitize, [window_record(sp, c["tokens"], c["seek"], c["seek_end"]) for c in cases])
    for c, line in zip(cases, lines):
        same_window(parse_window(line), c, c["seed"])
    assert sum(c["failed"] for c in cases) >= 40 and sum(not c["failed"] for c in cases) >= 300


# ---- 2. the parameters the fixture does not vary, live against the oracle's skwo_debug_window
VARIANTS = [dict(single_segment=1), dict(no_timestamps=1), dict(max_tokens=1), dict(max_tokens=3), dict(max_tokens=8)]


@SANITIZE
def test_engine_rules_equal_oracle_under_other_parameters(tmp_path_factory, oracle_tiny, sanitize):
    om = oracle_tiny
    sp = lr.special_ids(om)
    assert om.hp.n_text_ctx // 2 - 4 == N_MAX
    records, wants, whats = [], [], []
    for ki, kind in enumerate(sr.KINDS):
        for n in range(6):
            toks, seek, seek_end = sr.make_stream(np.random.default_rng(770000 + 100 * ki + n), sp, om.hp.n_vocab, kind)
            for v in VARIANTS:
                p = om.default_params()
                for k, x in v.items():
                    setattr(p, k, x)
                wants.append(sr.oracle_window(om, p, toks, seek, seek_end))
                records.append(window_record(sp, toks, seek, seek_end, **v))
                whats.append((kind, n, v))
    lines = run_driver(tmp_path_factory, sanitize, records)
    for line, want, what in zip(lines, wants, whats):
        same_window(parse_window(line), want, what)
    # the variants did something: budgets cut streams short, single_segment merged cuts, no_timestamps kept whole streams
    cut = [w for w, t in zip(wants, whats) if "max_tokens" in t[2] and not w["failed"]]
    assert any(w["consumed"] == 2 for w in cut) and any(w["consumed"] == 9 for w in cut)
    assert all(len(w["segments"]) <= 1 for w, t in zip(wants, whats) if t[2] == dict(single_segment=1))
    assert all(not w["failed"] and w["kept"] == w["consumed"] and w["advance"] == 3000 for w, t in zip(wants, whats) if t[2] == dict(no_timestamps=1))


# ---- 3. the other host rules against short statements of each
def ladder_ref(t, inc):
    t, inc = np.float32(t), np.float32(inc)
    out = [t]
    if inc > 0:
        x = t + inc
        while x < np.float32(1.0) + np.float32(1e-6) and len(out) < 16:
            out.append(x)
            x = x + inc
    return out


def prompt_ref(past, t, tail, prev):
    """context_ref_lib.full_with_context's rule, plus the pass temperature: -> (ids, take)"""
    if not past or not np.float32(t) < np.float32(0.5):
        return list(tail), 0
    take = min(N_TEXT_CTX // 2, len(past), N_TEXT_CTX - N_MAX - len(tail) - 1)
    return [prev] + past[len(past) - take:] + list(tail), take


def verdict_ref(failed, n_tokens, result_len, nsp, et, lt, nt, toks):
    """whisper.cpp's two expressions: `failed || (avg_logprobs < logprob_thold && no_speech_prob < no_speech_thold)` and
    `no_speech_prob > no_speech_thold && avg_logprobs < logprob_thold`; entropy over the last 32 kept tokens, only for more than 32"""
    et, lt, nt, nsp = (float(np.float32(x)) for x in (et, lt, nt, nsp))
    avg, n_tok = -np.inf, n_tokens
    if not failed:
        n_tok = result_len
        if result_len:
            avg = sum(float(np.float32(p)) for _, p in toks[:result_len]) / result_len
            ids = [i for i, _ in toks[max(0, result_len - 32):result_len]]
            ent = -sum(ids.count(i) / len(ids) * np.log(ids.count(i) / len(ids)) for i in set(ids))
            failed = result_len > 32 and ent < et
    return [int(failed), int(failed or (avg < lt and nsp < nt)), int(nsp > nt and avg < lt), n_tok]


@SANITIZE
def test_ladder_prompt_verdict_past_and_context_rules(tmp_path_factory, sanitize):
    rng = np.random.default_rng(5150)
    prev, tails = 50361, {1: [50258], 3: [50258, 50259, 50359], 4: [50258, 50259, 50359, 50363]}
    records, wants = [], []
    # the ladder, and the prompt rule's t < 0.5 on its entries
    ladders = [(0.0, 0.2), (0.0, 0.0), (0.0, -1.0), (0.4, 0.3), (0.0, 0.05), (0.9, 0.2)]
    for (t, inc), n in zip(ladders, (6, 1, 1, 3, 16, 1)):
        ref = ladder_ref(t, inc)
        assert len(ref) == n
        records.append([1, f32(t), f32(inc)]); wants.append([n] + [f32(float(x)) & 0xffffffff for x in ref])
        for x in ref:
            ids, take = prompt_ref([7, 8, 9], float(x), tails[3], prev)
            assert take == (3 if float(x) < 0.5 else 0)
            records.append([2] + vec([7, 8, 9]) + [f32(float(x))] + vec(tails[3]) + [N_TEXT_CTX, N_MAX, prev]); wants.append([len(ids), take] + ids)
    # the prompt: past lengths around n_text_ctx / 2 x pass temperature x tail
    third_bound_binds = 0
    for n_past in (0, 1, 223, 224, 225, 512):
        past = [int(x) for x in rng.integers(0, 50257, size=n_past)]
        for t in (0.0, 0.4, 0.6):
            for tail in tails.values():
                ids, take = prompt_ref(past, t, tail, prev)
                third_bound_binds += take == N_TEXT_CTX - N_MAX - len(tail) - 1 < min(N_TEXT_CTX // 2, n_past)
                assert len(ids) <= 240
                records.append([2] + vec(past) + [f32(t)] + vec(tail) + [N_TEXT_CTX, N_MAX, prev]); wants.append([len(ids), take] + ids)
    assert third_bound_binds >= 1                                                  # (notimestamps in the tail: 223 < 224)
    # the verdict: entropy rule, then logprob / no-speech on either side of their thresholds
    et, lt, nt = 2.4, -1.0, 0.6
    rows = [(0, 41, 40, 0.1, [(11, -0.5)] * 41), (0, 33, 32, 0.1, [(11, -0.5)] * 33), (0, 41, 40, 0.1, [(100 + i, -0.5) for i in range(41)]), (1, 9, 4, 0.1, [(11, -0.5)] * 9),
            (0, 1, 0, 0.1, [(11, -0.5)])]
    for avg_side in (-1.25, -0.75):                                                # avg_logprobs = -1 -+ 1/16: just below / just above logprob_thold
        for nsp in (0.5, 0.7):
            rows.append((0, 5, 4, nsp, [(11, -1.0)] * 3 + [(12, avg_side)] + [(13, -9.0)]))
    for failed, n_tokens, result_len, nsp, toks in rows:
        records.append([3, failed, n_tokens, result_len, f32(nsp), f32(et), f32(lt), f32(nt), len(toks)] + [w for i, p in toks for w in (i, f32(p))])
        wants.append(verdict_ref(failed, n_tokens, result_len, nsp, et, lt, nt, toks))
    assert wants[-9][:2] == [1, 1] and wants[-8][:2] == [0, 0] and wants[-7][0] == 0 and wants[-6] == [1, 1, 0, 9] and wants[-5][3] == 0
    assert [w[1:3] for w in wants[-4:]] == [[1, 0], [0, 1], [0, 0], [0, 0]]        # below: fallback unless no-speech, no-speech class when it is; above: neither
    # prompt_past update and the context's way back: the newest 512 of (what the prompt took + the window's kept tokens)
    past = [int(x) for x in rng.integers(0, 50257, size=cr.CONTEXT_MAX)]
    kept = [int(x) for x in rng.integers(0, 51865, size=30)]
    for take in (0, 5, len(past)):
        for no_speech in (0, 1):
            pp = (past[len(past) - take:] if take else []) + ([] if no_speech else kept)
            records.append([4] + vec(past) + [take, no_speech] + vec(kept) + [cr.CONTEXT_MAX]); wants.append(vec(pp) + vec(pp[-cr.CONTEXT_MAX:]))
    assert len(wants[-2]) == 1 + 542 + 1 + 512
    lines = run_driver(tmp_path_factory, sanitize, records)
    for k, (line, want) in enumerate(zip(lines, wants)):
        assert [int(x) for x in line.split()] == want, (k, records[k][:12])
    # the context check: the engine's messages, word for word
    NV = 51865
    checks = [([-1], "0 clip 3: context of -1 tokens outside [0, 512]"), ([513] + [1] * 513, "0 clip 3: context of 513 tokens outside [0, 512]"),
              ([3, 5, 6, NV], "0 clip 3: context token 2 (id %d) outside [0, %d)" % (NV, NV)), ([2, 5, -1], "0 clip 3: context token 1 (id -1) outside [0, %d)" % NV),
              ([0], "1"), ([512] + [NV - 1] * 512, "1")]
    assert run_driver(tmp_path_factory, sanitize, [[5, 512, NV, 3] + vec(cx) for cx, _ in checks]) == [w for _, w in checks]
