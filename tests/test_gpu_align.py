"""Word timestamps end to end on the micro model (skw_full_batch_aligned, skw_align_batch; the align_window phase of skw_engine.hip).

What is held to what:
  - the phase's arithmetic — hook, capture, reduce, DTW, in the exact precision, f16_mfma and ggml's arithmetic of a q5_1 file — to the CPU evaluator of include/skw_align.h run on
    the pass's own tapped queries and cross K: matrix and times, bit for bit (through skw_align_batch, where the test owns text and window);
  - alignment on to alignment off: identical tokens, text, segments and log-probabilities; a call that aligns nobody to skw_full_batch_rules: the same launches per kernel class;
  - a clip alone to the clip in a mixed batch (exact); skw_align_batch on a window's own text to what the aligned call gave that window; bad records to an error naming the clip.
Clips are 2 s, 5 s and 40 s (two windows and more), audio_ctx 0 / 96 / auto, aligned and not, in one batch."""
import numpy as np
import pytest

import align_ref_lib as al
from conftest import quantized_model
from streamkit_amd import engine, synth

pytestmark = pytest.mark.gpu
EOT = 50257
MASK = [3, 3]                 # micro: 2 decoder layers x 2 heads, all four (two layers: the head mean accumulates across launches)
SECS = (2, 5, 40, 5, 2)
ACTX = (0, 96, 0, "auto", 96)
ALIGNED = (True, True, True, False, True)


@pytest.fixture(scope="module")
def micro(micro_model_path):
    m = engine.Model(micro_model_path); ctx = engine.Context(m, max_batch=8, max_samples=16000 * 41)
    yield m, ctx
    ctx.close(); m.close()


def _params(ctx, n_samples, actx):
    p = ctx.default_params()
    p.audio_ctx = engine.audio_ctx_for_samples(n_samples) if actx == "auto" else actx
    return p


def _batch(ctx):
    pcms = [synth.clip(70 + i, 16000 * s) for i, s in enumerate(SECS)]
    params = [_params(ctx, p.size, a) for p, a in zip(pcms, ACTX)]
    return pcms, params


def _core(r):
    return ([tuple(np.float32(x).view(np.uint32) if isinstance(x, float) else x for x in t) for t in r["tokens"]], [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in r["segments"]],
            r["n_windows"], r["fallback_requested"], r["n_decode_steps"])


def _seq_taps(sn, mask):
    """the taps of sequence sn of the last aligned call (skw_engine.hip, align_hook / align_window)"""
    g = engine.debug_get
    return dict(dq={l: g("align_dq16_l%d_s%d" % (l, sn)) for l, w in enumerate(mask) if w}, ck={l: g("align_ck_l%d_s%d" % (l, sn)) for l, w in enumerate(mask) if w},
                x=g("align_x_s%d" % sn), info=[int(v) for v in g("align_seq_s%d" % sn)], idx=[int(v) for v in g("align_idx_s%d" % sn)])


def _evaluate(tmp_path_factory, hp, taps, n_text, n_keys, kw, mask, width=7, seek=0):
    """the evaluator on one sequence's tapped queries (its alignment rows) and its slot's cross K: -> (x f32 [N][kw], t0, t1)"""
    N = n_text + 1
    recs = []
    for l, w in enumerate(mask):
        if not w:
            continue
        q = taps["dq"][l].astype(np.uint16).view(np.float16).reshape(N, hp.n_text_state)
        K = taps["ck"][l].astype(np.uint16).view(np.float16).reshape(hp.n_audio_ctx, hp.n_text_state)[:n_keys]
        recs += [al.rec_weights(np.ascontiguousarray(q[:, 64 * h:64 * h + 64]), np.ascontiguousarray(K[:, 64 * h:64 * h + 64])) for h in range(hp.n_text_head) if w >> h & 1]
    exe = al.driver(tmp_path_factory)
    P = np.stack([o.view(np.float32).reshape(N, n_keys) for o in al.run(exe, recs)])
    x = al.run(exe, [al.rec_reduce(P, kw, width)])[0].view(np.float32).reshape(N, kw)
    d = al.parse_dtw(al.run(exe, [al.rec_dtw(x, seek)])[0], N)
    return x, d["t0"], d["t1"]


def _aligned_with_taps(ctx, pcm, text, p, ap, mask):
    engine.debug_enable(True)
    try:
        times = ctx.align_batch([pcm], [text], [ap], params=p)[0]
        assert int(engine.debug_get("align_n")[0]) == 1
        taps = _seq_taps(0, mask)
    finally:
        engine.debug_enable(False)
    return times, taps


CASES = [("exact", None, 0, 5, 37), ("exact", None, 96, 2, 9), ("f16_mfma", None, 0, 5, 37), ("f16_mfma", None, 96, 2, 1), ("exact", "q5_1", 0, 5, 37), ("exact", None, 0, 30, 220)]


@pytest.mark.parametrize("precision,quant,actx,secs,n_text", CASES)
def test_phase_equals_evaluator_on_tapped_operands(micro, tmp_path_factory, precision, quant, actx, secs, n_text):
    m, ctx = micro
    if quant:
        m = engine.Model(quantized_model("micro", quant)); ctx = engine.Context(m, max_batch=2, max_samples=16000 * 31)
    try:
        hp = m.hp
        ctx.set_precision(precision)
        pcm = synth.clip(80 + secs, 16000 * secs)
        text = np.random.default_rng(100 + n_text).integers(300, 20000, size=n_text).astype(np.int32)
        p = _params(ctx, pcm.size, actx); ap = engine.align_params(MASK)
        times, taps = _aligned_with_taps(ctx, pcm, text, p, ap, MASK)
        n_keys = actx or hp.n_audio_ctx
        n_len_org = ctx.log_mel(pcm)[1]                                         # the clip's mel frames, as whisper.cpp counts them (499 for 5 s)
        kw = max(1, min(min(3000, n_len_org) // 2, n_keys))
        x, t0, t1 = _evaluate(tmp_path_factory, hp, taps, n_text, n_keys, kw, MASK)
        assert taps["info"][1:5] == [0, n_keys, kw, n_text + 1] and taps["idx"] == list(range(n_text))
        assert taps["x"].size == x.size and np.array_equal(taps["x"].view(np.uint32), x.reshape(-1).view(np.uint32)), "the matrix differs from the evaluator's"
        assert [a for a, _ in times] == list(t0[:n_text]) and [b for _, b in times] == list(t1[:n_text])
        assert all(0 <= a <= 2 * kw and b >= a for a, b in times) and all(times[i][0] <= times[i + 1][0] for i in range(n_text - 1))
    finally:
        ctx.set_precision("exact")
        if quant:
            ctx.close(); m.close()


BEG = 50364      # <|0.00|> of the multilingual vocabulary
MASK_B, WIDTH_B = [0, 3], 5      # a second record in the batch: its clip runs in a pass of its own


@pytest.mark.parametrize("precision,quant", [("exact", None), ("f16_mfma", None), ("exact", "q5_1")])
def test_mixed_batch_equals_evaluator_window_by_window(micro, tmp_path_factory, precision, quant):
    """The issue's batch — 2 s, 5 s and 40 s clips, audio_ctx 0 / 96 / auto, aligned and not, two different records — in ONE skw_full_batch_aligned call, in each arithmetic path.
    Every aligned window (sequence) of the call: its crop equals the rule on the clip's own frame count, its matrix and token times equal the evaluator's on the tapped queries and
    cross K, t0 lies in [seek, seek + 2 Kw] and does not step back, and where a segment of the window ends in a timestamp token the window's seek is recovered from the result
    (t1 - 2 (tid - <|0.00|>)) and must be the one the phase used.  Together the windows' tokens are all text tokens of the clip."""
    m, ctx = micro
    if quant:
        m = engine.Model(quantized_model("micro", quant)); ctx = engine.Context(m, max_batch=8, max_samples=16000 * 41)
    try:
        hp = m.hp
        ctx.set_precision(precision)
        pcms, params = _batch(ctx)
        recs = [engine.align_params(MASK) if a else None for a in ALIGNED]; recs[4] = engine.align_params(MASK_B, median_width=WIDTH_B)
        masks = {i: (MASK_B, WIDTH_B) if i == 4 else (MASK, 7) for i in range(5)}
        n_len_org = [ctx.log_mel(p)[1] for p in pcms]
        engine.debug_enable(True)
        try:
            res = ctx.full_batch(pcms, params, align=recs)
            n_seq = int(engine.debug_get("align_n")[0])
            seqs = [_seq_taps(sn, masks[int(engine.debug_get("align_seq_s%d" % sn)[0])][0]) for sn in range(n_seq)]
        finally:
            engine.debug_enable(False)
        per_clip = {i: [] for i in range(5)}
        recovered = later = 0
        for sq in seqs:
            ci, seek, n_keys, kw, N, slot, _ = sq["info"]
            mask, width = masks[ci]
            r = res[ci]; idx = sq["idx"]; T = len(idx)
            assert ALIGNED[ci] and N == T + 1 and n_keys == (params[ci].audio_ctx or hp.n_audio_ctx)
            assert kw == max(1, min(min(3000, n_len_org[ci] - seek) // 2, n_keys)), (ci, seek, kw)
            x, t0, t1 = _evaluate(tmp_path_factory, hp, sq, T, n_keys, kw, mask, width, seek)
            assert np.array_equal(sq["x"].view(np.uint32), x.reshape(-1).view(np.uint32)), ("matrix", ci, seek)
            got = [r["token_times"][k] for k in idx]
            assert [a for a, _ in got] == list(t0[:T]) and [b for _, b in got] == list(t1[:T]), ("times", ci, seek)
            assert all(seek <= a <= seek + 2 * kw for a, _ in got) and all(got[k][0] <= got[k + 1][0] for k in range(T - 1)), (ci, seek)
            assert all(r["tokens"][k][0] < EOT for k in idx)
            k0 = 0
            for sg in r["segments"]:      # the window's seek from the result alone, where a segment of it closes on a timestamp token
                k1 = k0 + len(sg["tokens"])
                if k0 <= idx[0] < k1 or k0 <= idx[-1] < k1:
                    last = r["tokens"][k1 - 1]
                    if last[0] > BEG:
                        assert sg["t1"] - 2 * (last[1] - BEG) == seek, (ci, seek, sg["t1"], last)
                        recovered += 1; later += seek > 0
                k0 = k1
            seg_of = [j for j, sg in enumerate(r["segments"]) for _ in sg["tokens"]]          # token index -> its segment
            per_clip[ci].append((seek, idx, r["segments"][seg_of[idx[-1]]]["t1"]))
        for ci, ws in per_clip.items():
            text_idx = [k for k, t in enumerate(res[ci]["tokens"]) if t[0] < EOT]
            if not ALIGNED[ci]:
                assert not ws and all(t == (-1, -1) for t in res[ci]["token_times"])
                continue
            ws.sort()
            assert [k for _, idx, _ in ws for k in idx] == text_idx, ci                     # every text token of the clip belongs to exactly one aligned window, in order
            assert all(a[0] < b[0] for a, b in zip(ws, ws[1:])) and (not ws or ws[0][0] == 0), ci
            # a later window's seek from the result alone: whisper_full advances seek to the end of the window's last segment, or — when the window closes "text, timestamp" —
            # by what is left of the 30 s chunk.  (Windows that gave no tokens lie between two aligned ones only when n_windows exceeds their number: then only the order holds.)
            for (s0, _, end0), (s1, _, _) in zip(ws, ws[1:]):
                ways = (end0, s0 + min(3000, n_len_org[ci] - s0))
                if res[ci]["n_windows"] == len(ws):
                    assert s1 in ways, (ci, s0, s1, ways)
                assert s1 >= end0, (ci, s0, s1, end0)
                later += s1 in ways
            assert all(res[ci]["token_times"][k] == (-1, -1) for k in range(len(res[ci]["tokens"])) if k not in set(text_idx))
        assert len(per_clip[2]) >= 2 and per_clip[4], "the 40 s clip must give later windows, and the second record a pass of its own"
        assert recovered > 0 and later > 0, ("no later window had its seek confirmed from the result: the test shows nothing about seek",
                                             {ci: ([(w[0], w[2]) for w in ws], res[ci]["n_windows"], [(sg["t0"], sg["t1"]) for sg in res[ci]["segments"]]) for ci, ws in per_clip.items()})
        assert any(sq["info"][5] > 0 for sq in seqs)                                          # sequences in slots above 0
    finally:
        ctx.set_precision("exact")
        if quant:
            ctx.close(); m.close()


def test_aligned_batch_leaves_the_transcripts_alone_and_times_are_ordered(micro):
    m, ctx = micro
    ctx.set_precision("exact")
    pcms, params = _batch(ctx)
    ap = engine.align_params(MASK)
    off = ctx.full_batch(pcms, params)
    on = ctx.full_batch(pcms, params, align=[ap if a else None for a in ALIGNED])
    eot = 50257
    some = 0
    for i, (a, b) in enumerate(zip(off, on)):
        assert _core(a) == _core(b), "clip %d: alignment changed the transcript" % i
        tt = b["token_times"]
        assert len(tt) == len(b["tokens"])
        end_cs = pcms[i].size // 160 + 2
        for k, (tok, (t0, t1)) in enumerate(zip(b["tokens"], tt)):
            if tok[0] >= eot or not ALIGNED[i]:
                assert (t0, t1) == (-1, -1), (i, k)
            else:
                assert 0 <= t0 <= t1 <= end_cs, (i, k, t0, t1)
                some += 1
        k0 = 0      # a segment lies inside one window: there the times do not step back
        for s in b["segments"]:
            n = len(s["tokens"])
            ts = [tt[k][0] for k in range(k0, k0 + n) if b["tokens"][k][0] < eot]
            if ALIGNED[i]:
                assert ts == sorted(ts), (i, s["t0"])
            k0 += n
    assert some > 0, "no window of the batch was aligned: the test shows nothing"
    assert on[2]["n_windows"] >= 2
    # exact precision: a clip alone is the clip in the batch
    for i in (0, 2):
        alone = ctx.full_batch([pcms[i]], [params[i]], align=[ap])[0]
        assert _core(alone) == _core(on[i]) and alone["token_times"] == on[i]["token_times"], i


def test_a_call_that_aligns_nobody_is_the_rules_call_launch_for_launch(micro):
    m, ctx = micro
    ctx.set_precision("exact")
    pcms, params = _batch(ctx)
    pcms, params = pcms[:2], params[:2]
    counts = []
    for kw in (dict(rules=[None, None]), dict(align=[None, engine.AlignParams(enabled=0, median_width=7)])):
        ctx.profile(True)
        try:
            res = ctx.full_batch(pcms, params, **kw)
            prof = ctx.profile_get()
        finally:
            ctx.profile(False)
        counts.append(({k: v["count"] for k, v in prof.items()}, [_core(r) for r in res]))
    assert counts[0] == counts[1]
    assert counts[1][0]["k_align_qk"] == 0 and counts[1][0]["k_align_dtw"] == 0 and sum(counts[1][0].values()) > 0


def test_align_batch_on_a_windows_own_text_is_the_aligned_calls_times(micro):
    m, ctx = micro
    ctx.set_precision("exact")
    ap = engine.align_params(MASK)
    found = 0
    for i, secs in enumerate((2, 5, 5, 2)):
        pcm = synth.clip(90 + i, 16000 * secs)
        p = _params(ctx, pcm.size, (0, 96, "auto", 0)[i])
        r = ctx.full_batch([pcm], [p], align=[ap])[0]
        text = [(k, t[0]) for k, t in enumerate(r["tokens"]) if t[0] < 50257]
        if r["n_windows"] != 1 or r["fallback_requested"] or not text:
            continue      # (the window's text is only known to the test when the clip is one window)
        got = ctx.align_batch([pcm], [[t for _, t in text]], [ap], params=p)[0]
        assert got == [r["token_times"][k] for k, _ in text], i
        found += 1
    assert found > 0, "no one-window clip with text among the four: the test shows nothing"


def test_bad_records_fail_the_call_and_name_the_clip(micro):
    m, ctx = micro
    pcms = [synth.clip(70, 16000 * 2), synth.clip(71, 16000 * 2)]
    good = engine.align_params(MASK)
    bad = [(engine.AlignParams(enabled=1, median_width=7), "clip 1: alignment asked for with an empty head mask"),
           (engine.align_params([3, 4]), "clip 1: alignment head 2 of layer 1 outside the model's 2 heads"),
           (engine.align_params([3, 3, 1]), "clip 1: alignment head in layer 2 outside the model's 2 decoder layers"),
           (engine.align_params(MASK, median_width=6), "clip 1: alignment median_width 6 is not an odd number in [1, 15]"),
           (engine.align_params(MASK, median_width=-1), "clip 1: alignment median_width -1 is not an odd number in [1, 15]")]
    for rec, msg in bad:
        with pytest.raises(Exception) as e:
            ctx.full_batch(pcms, [ctx.default_params()] * 2, align=[good, rec])
        assert msg in str(e.value)
        assert ctx.align_params_check(rec.enabled, rec.median_width, list(rec.head_mask), clip=1) == msg
    assert ctx.align_params_check(1, 7, MASK) is None
    r = ctx.full_batch(pcms, [ctx.default_params()] * 2, align=[good, None])      # the context still works after the refusals
    assert len(r) == 2 and all(t == (-1, -1) for t in r[1]["token_times"])
