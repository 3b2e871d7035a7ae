"""whisper_full_with_state with text handed in: the checker for skw_full_batch_context, composed from what oracle/ exports (test infrastructure only; oracle/ itself has no
entry point that takes a context, and is not touched).

Per window: OracleModel.encode; OracleDecoder.step(prompt, 0) — the prompt is [prev] + the last min(n_text_ctx / 2, n, room) tokens of prompt_past (when there are any), then sot,
language, task (, notimestamps); then per token logit_rules_lib.oracle_process(hist, raw) for the choice and OracleDecoder.step([id], n_prompt + i); the token loop stops where
segment_rules_lib.oracle_window(hist + [one dummy text id]) reports consumed <= len(hist) (the loop left at the last real token: <|endoftext|>, the end of the audio, the budget, a
failure); oracle_window(hist) gives `kept`, `advance` and the segments; prompt_past is updated as skwo_full does (oracle/skw_oracle.c, "update prompt_past": what the prompt took is
kept, the window's kept tokens are appended).

One thing the debug hook cannot know: skwo_full takes a window's first t0 from the first token's `tid` (the likeliest timestamp when that token was sampled, which for a text
token is no function of the ids).  The first segment's t0 is therefore computed here the way window_output does, from the tid oracle_process returned.

Runs at temperature_inc = 0 and no_speech_thold = 1.0, so neither the temperature ladder nor the no-speech class enters: a window has ONE pass, and a pass that fails is the
window's result as it stands (skwo_full: every sampled token goes to the output step, prompt_past gets the first result_len of them).  The synthetic model fails that way behind a
long context — its <|endoftext|> grows likely with the position, so 225 prompt tokens are answered with "<|0.00|>, <|endoftext|>", which in the middle of a file is a failed pass.
skwo_debug_window reports nothing for a failed pass, so the loop's bookkeeping and the output cut are restated below (loop_update, window_cut: oracle/skw_oracle.c
token_loop_update and window_output) — and on every pass that does not fail the restatement must give exactly what oracle_window gives, which keeps it pinned to the oracle.
test_cpu_context.py holds the whole loop against OracleModel.full with an empty context."""
import numpy as np

import logit_rules_lib as lr
import segment_rules_lib as sr

CONTEXT_MAX = 512


def params_for(om, **kw):
    p = om.default_params()
    p.temperature_inc = 0.0
    p.no_speech_thold = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def prompt_tail(om, sp, p, lang_id):
    out = [sp["sot"]]
    if om.hp.n_vocab >= 51865:
        out += [sp["sot"] + 1 + lang_id, sp["sot"] + (om.hp.n_vocab - 51865) + 99 + (1 if p.translate else 2)]
    if p.no_timestamps:
        out.append(sp["not_"])
    return out


def loop_update(st, p, tid_id, i, seek, seek_end, n_max, beg, eot):
    """token_loop_update restated: one sampled token's effect on (has_ts, seek_delta, result_len); True = the loop ends here (st["failed"] says how)"""
    if tid_id > beg:
        sd = 2 * (tid_id - beg)
        if st["has_ts"] and st["seek_delta"] > sd and st["result_len"] < i:
            st["failed"] = True
            return True
        st["seek_delta"], st["result_len"], st["has_ts"] = sd, i + 1, True
    if tid_id == eot or (p.max_tokens > 0 and i >= p.max_tokens) or (st["has_ts"] and seek + st["seek_delta"] + 10 >= seek_end):
        if st["result_len"] == 0 and not p.no_timestamps:
            if seek + st["seek_delta"] + 10 >= seek_end:
                st["result_len"] = i + 1
            else:
                st["failed"] = True
                return True
        if p.single_segment or p.no_timestamps:
            st["result_len"], st["seek_delta"] = i + 1, 3000
        return True
    if i == n_max - 1 and (st["result_len"] == 0 or st["seek_delta"] < 1500):
        st["failed"] = True
        return True
    return False


def window_cut(p, toks, seek, seek_delta, seek_end, beg, eot):
    """window_output restated on the tokens handed to it (dicts with id and tid) -> ([(t0, t1, i0, i1)], advance)"""
    segs = []
    n = len(toks)
    if n > 0:
        i0, t0, has_text, i = 0, seek + 2 * (toks[0]["tid"] - beg), False, 0
        while i < n:
            if toks[i]["id"] < eot:
                has_text = True                        # (no vocabulary entry below <|endoftext|> is empty)
            if toks[i]["id"] > beg and not p.single_segment:
                t1 = seek + 2 * (toks[i]["tid"] - beg)
                if has_text:
                    segs.append((t0, t1, i0, i + 1))
                has_text = False
                while i < n and toks[i]["id"] > beg:
                    i += 1
                i -= 1
                t0, i0 = t1, i + 1
            i += 1
        if has_text:
            segs.append((t0, seek + seek_delta, i0, n))
    if n > 1 and toks[n - 2]["id"] < beg and toks[n - 1]["id"] > beg:
        seek_delta = min(seek_end - seek, 3000)
    return segs, seek_delta


def full_with_context(om, pcm, context=(), params=None):
    """-> dict(tokens=[(id, tid, p, plog)], segments=[dict(t0, t1, tokens, text)], n_windows, context=[ids the call leaves]) for one clip decoded behind `context` (token ids,
    oldest first: prompt_past as whisper_full_with_state's window loop finds it)"""
    p = params or params_for(om)
    assert p.temperature_inc <= 0.0 and p.temperature == 0.0 and p.lang_id >= 0
    sp = lr.special_ids(om)
    hp = om.hp
    beg, eot = sp["beg"], sp["eot"]
    mel, n_len_org = om.log_mel(pcm)
    prompt_past = [int(x) for x in context]
    assert len(prompt_past) <= CONTEXT_MAX
    tail = prompt_tail(om, sp, p, p.lang_id)
    n_max = hp.n_text_ctx // 2 - 4
    out = dict(tokens=[], segments=[], n_windows=0, context=None, failed_passes=0)
    seek, seek_end = 0, n_len_org
    if seek_end < 10:                                   # "input is too short": the context comes back as it went in
        out["context"] = prompt_past
        return out
    while seek + 10 < seek_end:
        _, ck, cv = om.encode(mel, seek)
        out["n_windows"] += 1
        take = 0
        prompt = []
        if prompt_past:                                 # [prev] (the id below <|nospeech|>) + the newest `take` tokens
            take = min(hp.n_text_ctx // 2, len(prompt_past), hp.n_text_ctx - n_max - len(tail) - 1)
            prompt = [sp["nosp"] - 1] + prompt_past[len(prompt_past) - take:]
        prompt = prompt + tail
        dec = om.decoder(ck, cv)
        raw = dec.step(prompt, 0)
        hist, toks = [], []
        st = dict(has_ts=False, seek_delta=3000, result_len=0, failed=False)
        for i in range(n_max):
            r = lr.oracle_process(om, p, hist, raw)
            assert r is not None
            tk = r[2]
            hist.append(tk["id"]); toks.append(tk)
            stop = loop_update(st, p, tk["id"], i, seek, seek_end, n_max, beg, eot)
            assert stop == (sr.oracle_window(om, p, hist + [0], seek, seek_end)["consumed"] <= len(hist)) or i == n_max - 1
            if stop:
                break
            raw = dec.step([tk["id"]], len(prompt) + i)
        dec.close()
        w = sr.oracle_window(om, p, hist, seek, seek_end)
        assert w["failed"] == st["failed"]
        out["failed_passes"] += int(st["failed"])
        kept = st["result_len"]
        # a failed pass hands every sampled token to the output step; a completed one the first result_len
        shown = toks if st["failed"] else toks[:kept]
        segs, advance = window_cut(p, shown, seek, st["seek_delta"], seek_end, beg, eot)
        if not st["failed"]:      # the oracle's own answer for this window: the restatement above may not differ from it (t0 of a first segment apart, see the module's docstring)
            assert kept == w["kept"] and advance == w["advance"] and len(segs) == len(w["segments"])
            for k, ((t0, t1, i0, i1), (o0, o1, oids)) in enumerate(zip(segs, w["segments"])):
                assert hist[i0:i1] == oids and t1 == o1 and (t0 == o0 or (k == 0 and hist[0] <= beg)), "segment %d differs from skwo_debug_window's" % k
        for (t0, t1, i0, i1) in segs:
            seg_ids = hist[i0:i1]
            text = b"".join(om.token_bytes(x) for x in seg_ids if x < eot)
            out["segments"].append(dict(t0=t0, t1=t1, tokens=list(seg_ids), text=text))
            out["tokens"] += [(t["id"], t["tid"], t["p"], t["plog"]) for t in toks[i0:i1]]
        ids = hist[:kept]
        prompt_past = prompt_past[len(prompt_past) - take:] + ids if take else list(ids)
        seek += advance
    out["context"] = prompt_past[-CONTEXT_MAX:]
    return out


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def token_bits(tokens):
    """(id, tid, p bits, plog bits) per token: what the engine and the checker must agree on"""
    return [(int(t[0]), int(t[1]), bits(t[2]), bits(t[3])) for t in tokens]


def make_context(rng, sp, n, with_timestamps=True):
    """n seeded token ids as a transcript would leave them: text ids, and (with_timestamps) timestamp pairs in between"""
    out = []
    while len(out) < n:
        if with_timestamps and rng.random() < 0.2:
            out.append(sp["beg"] + int(rng.integers(1, 1400)))
        else:
            out.append(int(rng.integers(0, 2000)))
    return out
