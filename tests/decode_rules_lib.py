"""Decoding constraints per clip (skw_decode_rules, include/skw_engine.h): the transform k_dec_constrain applies to a row of logits ahead of K11, three ways —
  transform      numpy, the contract's own f32 steps (bias add; x < 0 ? x * t : x / t once per distinct text token; -inf on the tokens that would complete a repeated n-gram)
  hf_transform   transformers' SequenceBiasLogitsProcessor / SuppressTokensLogitsProcessor, RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor in that order, with
                 input_ids = T, the pass's text tokens (an independent implementation; a tool of the build machine, not needed where the GPU tests run: the committed fixture
                 tests/golden/decode_rule_cases.json carries the checked outcomes there)
  full_with_rules  context_ref_lib.full_with_context with transform(hist, raw) in front of logit_rules_lib.oracle_process: the end-to-end checker of skw_full_batch_rules
and the seeded cases all of them run on.  Test infrastructure only; oracle/ is not touched.

Rules here are plain dicts: dict(theta=float, N=int, bias=[(id, b), ...]) with b finite or -inf; None = no constraints.  to_engine() makes the binding's DecodeRules of one."""
import hashlib
import json
import os

import numpy as np

import context_ref_lib as cr
import logit_rules_lib as lr
import segment_rules_lib as sr

DEFAULT = dict(theta=1.0, N=0, bias=[])
HIST_MAX = 200      # below every model's max_tok - 1 (n_text_ctx / 2 - 1 = 223)
# The end-to-end tests' rule sets, on the micro model (seed 1234) and synth.clip(c, 160000) for c in {0, 3}: +50 on the first three text ids of the plain transcript makes the model
# loop (its text logits have a standard deviation of about 9 and a top value of about 36; at +200 the penalty no longer changes anything), and each rule then breaks the loop its way.
LOOP_IDS = (48931, 9388, 33340)
LOOP_BIAS = [(i, 50.0) for i in LOOP_IDS]
RULE_SETS = dict(plain=None, bias=dict(theta=1.0, N=0, bias=LOOP_BIAS), bias_t=dict(theta=1.5, N=0, bias=LOOP_BIAS), bias_n2=dict(theta=1.0, N=2, bias=LOOP_BIAS),
                 bias_t_n3=dict(theta=1.5, N=3, bias=LOOP_BIAS))


def fixture():
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_rule_cases.json")))


def text_tokens(hist, eot):
    return [int(t) for t in hist if t < eot]


def transform(hist, raw, rules, eot):
    """-> the row K11 sees (a new f32 array)"""
    x = np.array(raw, dtype=np.float32, copy=True)
    if rules is None:
        return x
    with np.errstate(invalid="ignore", over="ignore"):
        if rules["bias"]:
            ids = np.array([i for i, _ in rules["bias"]], dtype=np.int64)
            b = np.array([v for _, v in rules["bias"]], dtype=np.float32)
            assert len(set(ids.tolist())) == ids.size
            x[ids] = x[ids] + b                                     # 1. one f32 add per pair
        T = text_tokens(hist, eot)
        theta = np.float32(rules["theta"])
        if T:
            u = np.unique(np.array(T, dtype=np.int64))              # 2. each distinct text token once, on what step 1 left
            v = x[u]
            x[u] = np.where(v < 0, v * theta, v / theta).astype(np.float32)
        N, m = int(rules["N"]), len(T)
        if N >= 1 and m >= N:                                       # 3. the tokens that would complete an n-gram the pass already holds
            tail = T[m - N + 1:]
            for i in range(m - N + 1):
                if T[i:i + N - 1] == tail:
                    x[T[i + N - 1]] = -np.inf
    return x


def hf_transform(hist, raw, rules, eot):
    """the same through transformers' processors, input_ids = T"""
    import torch
    from transformers.generation.logits_process import (NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    T = text_tokens(hist, eot)
    ids = torch.tensor([T], dtype=torch.long).reshape(1, len(T))
    scores = torch.from_numpy(np.array(raw, dtype=np.float32, copy=True)[None, :])
    procs = []
    fin = {(int(i),): float(b) for i, b in rules["bias"] if np.isfinite(b)}      # (the dict form: the list form refuses token id 0)
    sup = [int(i) for i, b in rules["bias"] if np.isneginf(b)]
    if fin:
        procs.append(SequenceBiasLogitsProcessor(fin))
    if sup:
        procs.append(SuppressTokensLogitsProcessor(sup, device="cpu"))
    procs.append(RepetitionPenaltyLogitsProcessor(float(np.float32(rules["theta"]))))
    if rules["N"] > 0:
        procs.append(NoRepeatNGramLogitsProcessor(int(rules["N"])))
    for pr in procs:
        scores = pr(ids, scores)
    return scores[0].numpy().astype(np.float32)


def row_hash(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float32).tobytes()).hexdigest()


def bias_hash(bias):
    a = np.array([i for i, _ in bias], np.int32).tobytes() + np.array([b for _, b in bias], np.float32).tobytes()
    return hashlib.sha256(a).hexdigest()[:16]


# ---- seeded cases.  A case is (seed, spec): spec = dict(theta, N, m_kind, n_bias) chosen by the fixture's generator so that the grid of the contract is covered; history, raw
# logits and the bias pairs follow from the seed.  make_case draws repeats rarely, so the history is built here from a small pool of text ids with timestamp pairs in between —
# duplicates, n-grams repeated across timestamps and n-grams that only match when the timestamps are skipped all occur — and the raw row is make_case's ("initial": the row alone).
M_KINDS = ["0", "1", "N-1", "N", "long"]
THETAS = [0.5, 1.0, 1.3, 4.0]
NGRAMS = [0, 1, 2, 3, 5, 1000]       # 1000: larger than any m
N_BIAS = [0, 1, 256, 7]


def spec_for(k):
    """case k of the fixture: every (m_kind, N) pair and every theta / n_bias value many times over"""
    return dict(theta=THETAS[(k // 2) % 4], N=NGRAMS[(k // 5) % 6], m_kind=M_KINDS[k % 5], n_bias=N_BIAS[(k // 3) % 4])


def make_rule_case(seed, sp, NV, spec):
    """-> (hist, raw, rules)"""
    rng = np.random.default_rng(seed)
    beg, eot = sp["beg"], sp["eot"]
    N = spec["N"]
    m = {"0": 0, "1": 1, "N-1": max(0, min(N, 40) - 1), "N": max(1, min(N, 40)), "long": int(rng.integers(30, 150))}[spec["m_kind"]]
    pool = [int(x) for x in rng.integers(0, eot, size=int(rng.integers(2, 5)))]
    if rng.random() < 0.3:
        pool[0] = [0, eot - 1][int(rng.integers(0, 2))]            # the ends of the text range
    if spec["m_kind"] == "long" and rng.random() < 0.5:              # a phrase said again and again: the loop the rules are there for
        phrase = [pool[int(rng.integers(0, len(pool)))] for _ in range(int(rng.integers(2, 6)))]
        text = (phrase * (m // len(phrase) + 1))[:m]
    else:
        text = [pool[int(rng.integers(0, len(pool)))] for _ in range(m)]
    hist = []
    if m > 0 or rng.random() < 0.5:
        t = int(rng.integers(0, 40))
        hist.append(beg + t)
        for k, tok in enumerate(text):
            hist.append(tok)
            if k + 1 < len(text) and rng.random() < 0.25 and len(hist) + 2 + (len(text) - k) < HIST_MAX:      # a closed pair between two text tokens
                t = min(t + int(rng.integers(0, 60)), NV - beg - 1)
                hist += [beg + t, beg + t]
        tail = rng.random()
        if m > 0 and tail < 0.3 and len(hist) + 2 < HIST_MAX:
            t = min(t + int(rng.integers(0, 60)), NV - beg - 1)
            hist += [beg + t] if tail < 0.15 else [beg + t, beg + t]
    assert len(hist) <= HIST_MAX and len(text_tokens(hist, eot)) == m
    _, raw = lr.make_case(rng, sp, NV, "initial")
    for tok in pool:                                                  # the repeated tokens carry weight of both signs, so the penalty decides something
        raw[tok] = np.float32(rng.uniform(-8, 14))
    if rng.random() < 0.5:
        raw[pool[0]] = np.float32(0.0)
    for _ in range(3):
        raw[int(rng.integers(0, NV))] = np.float32(0.0)
    if rng.random() < 0.4:
        raw[pool[-1]] = -np.inf
    # bias pairs: first the places the contract names — a repeated token, a token the n-gram rule bans, a timestamp, <|endoftext|>, a statically suppressed special — then others
    named = [pool[0], pool[-1], beg + int(rng.integers(0, NV - beg)), eot, sp["sot"], sp["nosp"]]
    order = [int(x) for x in rng.permutation(len(named))]
    ids = []
    for j in order:
        if named[j] not in ids:
            ids.append(named[j])
    others = [int(x) for x in rng.permutation(NV)[:spec["n_bias"] + len(ids)] if int(x) not in ids]
    ids = (ids + others)[:spec["n_bias"]]
    bias = []
    for i in ids:
        b = -np.inf if rng.random() < 0.25 else float(np.float32(rng.uniform(-20, 20)))
        bias.append((int(i), b))
    return hist, raw, dict(theta=spec["theta"], N=N, bias=bias)


def to_engine(rules):
    from streamkit_amd import engine
    if rules is None:
        return None
    return engine.DecodeRules(repetition_penalty=rules["theta"], no_repeat_ngram_size=rules["N"], bias=list(rules["bias"]))


def repeats(ids, eot):
    """text tokens of a transcript that had occurred before in it"""
    T = text_tokens(ids, eot)
    return len(T) - len(set(T))


def repeated_bigrams(ids, eot):
    T = text_tokens(ids, eot)
    seen, n = set(), 0
    for a, b in zip(T, T[1:]):
        n += (a, b) in seen
        seen.add((a, b))
    return n


def full_with_rules(om, pcm, context=(), params=None, rules=None):
    """context_ref_lib.full_with_context with transform(hist, raw) in front of K11: one clip decoded behind `context` under `rules`, at temperature_inc = 0.  The history handed
    to the transform is the pass's own (hist starts empty in every window); the prompt is not part of it.  Also returns passes=[ids of each window's pass]."""
    p = params or cr.params_for(om)
    assert p.temperature_inc <= 0.0 and p.temperature == 0.0 and p.lang_id >= 0
    sp = lr.special_ids(om)
    hp = om.hp
    beg, eot = sp["beg"], sp["eot"]
    mel, n_len_org = om.log_mel(pcm)
    prompt_past = [int(x) for x in context]
    assert len(prompt_past) <= cr.CONTEXT_MAX
    tail = cr.prompt_tail(om, sp, p, p.lang_id)
    n_max = hp.n_text_ctx // 2 - 4
    out = dict(tokens=[], segments=[], n_windows=0, context=None, failed_passes=0, passes=[])
    seek, seek_end = 0, n_len_org
    if seek_end < 10:
        out["context"] = prompt_past
        return out
    while seek + 10 < seek_end:
        _, ck, cv = om.encode(mel, seek)
        out["n_windows"] += 1
        take = 0
        prompt = []
        if prompt_past:
            take = min(hp.n_text_ctx // 2, len(prompt_past), hp.n_text_ctx - n_max - len(tail) - 1)
            prompt = [sp["nosp"] - 1] + prompt_past[len(prompt_past) - take:]
        prompt = prompt + tail
        dec = om.decoder(ck, cv)
        raw = dec.step(prompt, 0)
        hist, toks = [], []
        st = dict(has_ts=False, seek_delta=3000, result_len=0, failed=False)
        for i in range(n_max):
            r = lr.oracle_process(om, p, hist, transform(hist, raw, rules, eot))
            assert r is not None
            tk = r[2]
            hist.append(tk["id"]); toks.append(tk)
            if cr.loop_update(st, p, tk["id"], i, seek, seek_end, n_max, beg, eot):
                break
            raw = dec.step([tk["id"]], len(prompt) + i)
        dec.close()
        out["passes"].append(list(hist))
        out["failed_passes"] += int(st["failed"])
        kept = st["result_len"]
        shown = toks if st["failed"] else toks[:kept]
        segs, advance = cr.window_cut(p, shown, seek, st["seek_delta"], seek_end, beg, eot)
        if not st["failed"]:      # the oracle's own cut of this window's tokens, as in full_with_context
            w = sr.oracle_window(om, p, hist, seek, seek_end)
            assert not w["failed"] and kept == w["kept"] and advance == w["advance"] and len(segs) == len(w["segments"])
        for (t0, t1, i0, i1) in segs:
            seg_ids = hist[i0:i1]
            text = b"".join(om.token_bytes(x) for x in seg_ids if x < eot)
            out["segments"].append(dict(t0=t0, t1=t1, tokens=list(seg_ids), text=text))
            out["tokens"] += [(t["id"], t["tid"], t["p"], t["plog"]) for t in toks[i0:i1]]
        ids = hist[:kept]
        prompt_past = prompt_past[len(prompt_past) - take:] + ids if take else list(ids)
        seek += advance
    out["context"] = prompt_past[-cr.CONTEXT_MAX:]
    return out
