"""Clips with different parameters in ONE batch (skw_full_batch_mixed; the sampler's per-row form, skw_dec_sample_rows; the node's `mixed_batch`).

The contract: row i of a mixed call is what the uniform call returns for clip i alone with params[i] — bit for bit in the exact precision (held here to the CPU oracle, which
knows nothing about batches), and in f16_mfma equal to the uniform f16_mfma call on that clip alone as long as no prompt pass reaches 256 rows.
The sampler is tested on its own first, against the committed fixture that was checked against transformers' logits processors: end to end the seeded models never pick a
non-speech token, so a whole-call test alone would pass with the two static masks swapped.

Each test creates its contexts once, runs every configuration once and frees them.  Oracle calls in this file: 20 + 14 (tiny) + 18 (micro) + 6 + 2 (node)."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import logit_rules_lib as lr
from oracle_lib import OracleModel
from streamkit_amd import minihost, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def plugin():
    return minihost.Plugin()


def _params(ctx_or_oracle, **kw):
    p = ctx_or_oracle.default_params()
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


# ------------------------------------------------------------------ the sampler alone
def _fixture_rows():
    """Every case of the fixture, the configurations interleaved evenly (each launch of 64 then holds rows of every (suppress_nst, suppress_blank) pair the fixture has: it
    holds three of the four pairs, 320 + 40 + 40 = 400 cases).  -> special ids, n_vocab, [(config, case, fixture index)]"""
    fx = json.load(open(os.path.join(HERE, "golden", "logit_rule_cases.json")))
    rows, k = [], 0
    for cfg in fx["configs"]:
        for i, c in enumerate(cfg["cases"]):
            rows.append(((i + 0.5) / len(cfg["cases"]), k, cfg, c)); k += 1
    rows.sort(key=lambda r: (r[0], r[1]))
    return fx["special"], fx["n_vocab"], [(cfg, c, k) for _, k, cfg, c in rows]


def _chunks(seq, n):
    for i in range(0, len(seq), n):
        yield seq[i:i + n]


@pytest.fixture(scope="module")
def gpu_tiny(tiny_model_path):
    from streamkit_amd import engine
    m = engine.Model(tiny_model_path, device=0)
    c = engine.Context(m, max_batch=64)
    yield c
    c.close(); m.close()


def test_per_row_sampler_matches_transformers_checked_fixture(gpu_tiny):
    """What test_gpu_logit_rules.py demands of the uniform launch, of launches whose rows each carry their own suppress_nst / suppress_blank: the fixture's argmax and plog in
    both sampler forms, its admissible set (mask_hash) in the streaming form, both variants.  This is what pins the pair of static masks and the per-row blank rule."""
    ctx = gpu_tiny
    sp, NV, rows = _fixture_rows()
    assert NV == ctx.model.hp.n_vocab and len(rows) == 400
    n_checked, pairs_per_launch = 0, []
    for batch in _chunks(rows, 64):
        hists, raws, ps = [], [], []
        for cfg, c, _ in batch:
            h, raw = lr.make_case(np.random.default_rng(c["seed"]), sp, NV, c["kind"])
            assert h == c["hist"]
            hists.append(h); raws.append(raw); ps.append(_params(ctx, suppress_nst=cfg["suppress_nst"], suppress_blank=cfg["suppress_blank"]))
        pairs_per_launch.append(len({(p.suppress_nst, p.suppress_blank) for p in ps}))
        for variant in ("raw", "neutral"):
            lg = []
            for h, raw in zip(hists, raws):
                x = raw.copy()
                if variant == "neutral":
                    x[lr.hf_extra_suppressed(h, sp, NV)] = -np.inf
                lg.append(x)
            lg = np.stack(lg)
            tk0, _, _ = ctx.sample_rows(hists, lg, ps, form=0)
            tk1, _, filt = ctx.sample_rows(hists, lg, ps, form=1, want_filtered=True)
            for r, (cfg, c, _) in enumerate(batch):
                want = c[variant]
                assert lr.mask_hash(filt[r]) == want["mask_hash"], (c["seed"], variant, cfg["suppress_nst"], cfg["suppress_blank"])
                assert int(tk0["id"][r]) == want["argmax"] and int(tk1["id"][r]) == want["argmax"], (c["seed"], variant, int(tk0["id"][r]), int(tk1["id"][r]), want["argmax"])
                assert np.float32(tk0["plog"][r]) == np.float32(want["plog"]) and np.float32(tk1["plog"][r]) == np.float32(want["plog"]), (c["seed"], variant)
                n_checked += 1
    assert n_checked == 2 * 400
    assert min(pairs_per_launch) >= 3, pairs_per_launch      # every launch really mixed the fixture's configurations


def test_per_row_sampler_equals_the_uniform_launch_under_each_rows_rules(gpu_tiny):
    """The rules the fixture does not vary: per row, no_timestamps in {0, 1} and max_initial_ts in {0, 0.2, 1.0}, drawn by numpy.random.default_rng(7) per case in fixture order
    (integers(0, 2), then choice([0, 0.2, 1.0])), on top of the case's configuration.  Row r of the mixed launch == row r of a uniform launch with r's rules (the code path the
    existing tests hold to the oracle): token record, trace record and, in the streaming form, the filtered row, bit for bit.
    That the draw matters — on the CPU oracle (skwo_debug_process_logits) these rules change the chosen token of 81 of the 400 rows and the admissible set of 177 against the
    default rules; the same two counts are taken here from the uniform launches and must reach 60 and 140."""
    ctx = gpu_tiny
    sp, NV, rows = _fixture_rows()
    draw = np.random.default_rng(7); rule_of = {}
    for k in range(len(rows)):      # fixture order
        rule_of[k] = (int(draw.integers(0, 2)), float(draw.choice([0, 0.2, 1.0])))
    cases = []
    for cfg, c, k in rows:
        h, raw = lr.make_case(np.random.default_rng(c["seed"]), sp, NV, c["kind"])
        cases.append(dict(hist=h, raw=raw, nst=cfg["suppress_nst"], blank=cfg["suppress_blank"], no_ts=rule_of[k][0], mits=rule_of[k][1]))

    def uniform(key_of):
        """every row through uniform launches, grouped by the rules key_of gives it -> per row (tokens form 0, trace form 0, tokens form 1, trace form 1, filtered)"""
        out = [None] * len(cases); groups = {}
        for r, c in enumerate(cases):
            groups.setdefault(key_of(c), []).append(r)
        for (nst, blank, no_ts, mits), members in sorted(groups.items()):
            p = _params(ctx, suppress_nst=nst, suppress_blank=blank, no_timestamps=no_ts, max_initial_ts=mits)
            for part in _chunks(members, 64):
                hs = [cases[r]["hist"] for r in part]; lg = np.stack([cases[r]["raw"] for r in part])
                tk0, tr0, _ = ctx.sample_rows(hs, lg, p, form=0)
                tk1, tr1, filt = ctx.sample_rows(hs, lg, p, form=1, want_filtered=True)
                for j, r in enumerate(part):
                    out[r] = (tk0[j:j + 1].tobytes(), tr0[j:j + 1].tobytes(), tk1[j:j + 1].tobytes(), tr1[j:j + 1].tobytes(), filt[j].copy(), int(tk0["id"][j]))
        return out

    own = uniform(lambda c: (c["nst"], c["blank"], c["no_ts"], c["mits"]))
    dflt = uniform(lambda c: (c["nst"], c["blank"], 0, 1.0))
    mixed = [None] * len(cases)
    for part in _chunks(list(range(len(cases))), 64):
        hs = [cases[r]["hist"] for r in part]; lg = np.stack([cases[r]["raw"] for r in part])
        ps = [_params(ctx, suppress_nst=cases[r]["nst"], suppress_blank=cases[r]["blank"], no_timestamps=cases[r]["no_ts"], max_initial_ts=cases[r]["mits"]) for r in part]
        assert len({(p.no_timestamps, p.max_initial_ts, p.suppress_nst, p.suppress_blank) for p in ps}) >= 6      # the launch is mixed in earnest
        tk0, tr0, _ = ctx.sample_rows(hs, lg, ps, form=0)
        tk1, tr1, filt = ctx.sample_rows(hs, lg, ps, form=1, want_filtered=True)
        for j, r in enumerate(part):
            mixed[r] = (tk0[j:j + 1].tobytes(), tr0[j:j + 1].tobytes(), tk1[j:j + 1].tobytes(), tr1[j:j + 1].tobytes(), filt[j].copy(), int(tk0["id"][j]))
    for r in range(len(cases)):
        for f, name in enumerate(("token (form 0)", "trace (form 0)", "token (streaming)", "trace (streaming)")):
            assert mixed[r][f] == own[r][f], (r, name, cases[r]["no_ts"], cases[r]["mits"])
        assert mixed[r][4].tobytes() == own[r][4].tobytes(), (r, "filtered row")
    changed_token = sum(own[r][5] != dflt[r][5] for r in range(len(cases)))
    changed_set = sum(not np.array_equal(np.isneginf(own[r][4]), np.isneginf(dflt[r][4])) for r in range(len(cases)))
    print("drawn rules change the token of %d rows and the admissible set of %d (oracle: 81, 177)" % (changed_token, changed_set))
    assert changed_token >= 60 and changed_set >= 140, (changed_token, changed_set)


def test_per_row_sampler_all_four_suppress_pairs_in_one_launch(gpu_tiny, oracle_tiny):
    """The fixture holds three of the four (suppress_nst, suppress_blank) pairs; here the first 128 histories take all four in turn (row r: pair r % 4), with
    no_timestamps / max_initial_ts drawn the same way on top.  Row r of the mixed launch == row r of a uniform launch with r's rules, bit for bit, in both forms — and the
    rows of the pair the fixture lacks (0, 0) are held to the CPU oracle directly (decision fields and admissible set)."""
    ctx, om = gpu_tiny, oracle_tiny
    sp, NV, rows = _fixture_rows()
    draw = np.random.default_rng(7)
    cases = []
    for r, (cfg, c, k) in enumerate(rows[:128]):
        h, raw = lr.make_case(np.random.default_rng(c["seed"]), sp, NV, c["kind"])
        cases.append(dict(hist=h, raw=raw, nst=(r % 4) >> 1, blank=(r % 4) & 1, no_ts=int(draw.integers(0, 2)), mits=float(draw.choice([0, 0.2, 1.0]))))
    n_oracle = 0
    for part in _chunks(list(range(len(cases))), 64):
        hs = [cases[r]["hist"] for r in part]; lg = np.stack([cases[r]["raw"] for r in part])
        ps = [_params(ctx, suppress_nst=cases[r]["nst"], suppress_blank=cases[r]["blank"], no_timestamps=cases[r]["no_ts"], max_initial_ts=cases[r]["mits"]) for r in part]
        assert len({(p.suppress_nst, p.suppress_blank) for p in ps}) == 4
        tk0, tr0, _ = ctx.sample_rows(hs, lg, ps, form=0)
        tk1, tr1, filt = ctx.sample_rows(hs, lg, ps, form=1, want_filtered=True)
        for j, r in enumerate(part):
            u0, ut0, _ = ctx.sample_rows([hs[j]], lg[j:j + 1], ps[j], form=0)
            u1, ut1, uf = ctx.sample_rows([hs[j]], lg[j:j + 1], ps[j], form=1, want_filtered=True)
            assert tk0[j:j + 1].tobytes() == u0.tobytes() and tr0[j:j + 1].tobytes() == ut0.tobytes(), (r, "form 0")
            assert tk1[j:j + 1].tobytes() == u1.tobytes() and tr1[j:j + 1].tobytes() == ut1.tobytes() and filt[j].tobytes() == uf[0].tobytes(), (r, "streaming")
            if (cases[r]["nst"], cases[r]["blank"]) == (0, 0):
                po = _params(om, suppress_nst=0, suppress_blank=0, no_timestamps=cases[r]["no_ts"], max_initial_ts=cases[r]["mits"])
                o = lr.oracle_process(om, po, hs[j], lg[j])
                for f in ("id", "tid", "p", "plog", "pt", "ptsum"):
                    assert np.float32(tk0[f][j]) == np.float32(o[2][f]) and np.float32(tk1[f][j]) == np.float32(o[2][f]), (r, f)
                assert np.array_equal(np.isneginf(filt[j]), np.isneginf(o[0]))
                n_oracle += 1
    assert n_oracle == 32


# ------------------------------------------------------------------ whole calls
TINY_CLIPS = [(3, 8), (5, 9), (21, 3), (11, 40)]      # (synth clip, seconds); the last has two windows, the second carrying the first's text in its prompt
TINY_SETS = [{}, {"translate": 1}, {"no_timestamps": 1}, {"single_segment": 1, "max_tokens": 12}, {"lang_id": -1}, {"lang_id": 2}, {"suppress_blank": 0, "suppress_nst": 1}]


def _ids(r):
    return [t[0] for t in r["tokens"]]


def _same_as_oracle(g, o, what):
    assert _ids(g) == _ids(o), (what, _ids(g)[:12], _ids(o)[:12])
    assert [t[1] for t in g["tokens"]] == [t[1] for t in o["tokens"]], what
    assert [np.float32(t[3]).view(np.uint32) for t in g["tokens"]] == [np.float32(t[3]).view(np.uint32) for t in o["tokens"]], what      # plog, bit for bit
    assert [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in g["segments"]] == [(s["t0"], s["t1"], s["text"], s["tokens"]) for s in o["segments"]], what
    assert g["n_windows"] == o["n_windows"] and g["lang_id"] == o["lang_id"] and g["fallback_requested"] == o["fallback_requested"], what


def test_mixed_call_exact_equals_the_oracle_per_clip_and_parameter_set(eng, tiny_model_path, oracle_tiny):
    """Four clips x seven parameter sets dealt so that every clip meets five of them (the default, translate, no_timestamps and single_segment + max_tokens on every clip; auto-detect,
    another language and the other suppress_* pair on two clips each), 20 rows in ONE mixed call, shuffled by a fixed seed.  Every row is the oracle's full() of its clip
    under its own parameters: ids, tid, plog bits, segments, n_windows, lang_id.  translate / no_timestamps / single_segment + max_tokens change every clip's tokens
    (asserted), so a build that ignored the rows' own parameters could not pass; lang_id: -1 detects a language of its own."""
    om = oracle_tiny
    pcms = [synth.clip(c, 16000 * s) for c, s in TINY_CLIPS]
    deal = [(ci, si) for ci in range(4) for si in range(4)] + [(0, 4), (3, 4), (1, 5), (2, 5), (2, 6), (3, 6)]
    assert all(sum(1 for c, _ in deal if c == ci) >= 3 for ci in range(4)) and {s for _, s in deal} == set(range(len(TINY_SETS)))
    order = np.random.default_rng(5).permutation(len(deal)); rows = [deal[i] for i in order]
    m = eng.Model(tiny_model_path); ctx = eng.Context(m, max_batch=len(rows), max_samples=16000 * 41)
    try:
        res = ctx.full_batch([pcms[ci] for ci, _ in rows], params=[_params(ctx, **TINY_SETS[si]) for _, si in rows])
    finally:
        ctx.close(); m.close()
    want = {}
    for (ci, si), g in zip(rows, res):
        o = want[(ci, si)] = om.full(pcms[ci], _params(om, **TINY_SETS[si]))
        _same_as_oracle(g, o, (TINY_CLIPS[ci], TINY_SETS[si]))
    for ci in range(4):
        for si in (1, 2, 3):
            assert _ids(want[(ci, si)]) != _ids(want[(ci, 0)]), (TINY_CLIPS[ci], TINY_SETS[si])
    assert want[(3, 0)]["n_windows"] == 2
    assert all(want[(ci, 4)]["lang_id"] > 0 for ci in (0, 3)) and all(want[(ci, 5)]["lang_id"] == 2 for ci in (1, 2))


def _stress_jobs():
    """The fourteen (clip, parameters) of test_gpu_plugin.py's threaded stress test (its seed, its draws): 4 / 9 / 17 / 30 s clips, language en / de / auto, both suppress_* flags."""
    rng = np.random.default_rng(33); jobs = []
    for i in range(14):
        pcm = synth.clip(40 + i, int(16000 * rng.choice([4, 9, 17, 30])))
        rng.choice([0, 2, 20]); rng.choice([1, 4, 64])
        sb = int(rng.integers(0, 2)); nst = int(rng.integers(0, 2)); lang = {"en": 0, "de": 2, "auto": -1}[str(rng.choice(["en", "de", "auto"]))]
        rng.choice([480, 960, 1920, 4000]); rng.uniform(0, 0.05)
        jobs.append((pcm, dict(suppress_blank=sb, suppress_nst=nst, lang_id=lang)))
    return jobs


def _full_key(r):
    return ([(t[0], t[1], np.float32(t[3]).view(np.uint32)) for t in r["tokens"]], [(s["t0"], s["t1"], s["text"]) for s in r["segments"]], r["n_windows"], r["lang_id"], r["fallback_requested"])


def test_ragged_compositions_as_a_scheduler_forms_them(eng, tiny_model_path, oracle_tiny):
    """What arrival order makes of a queue: seeded subsets of the stress test's fourteen jobs (ragged lengths, some rows auto-detecting, a job twice in a batch, the uniform call
    in between), in workspaces of different shape, with an exact and an f16_mfma context at work AT THE SAME TIME on two threads — the node runs one engine per precision.
    Exact rows equal the oracle; f16_mfma rows equal the same job alone in a quiet context (every prompt is 3 tokens: no pass comes near 256 rows)."""
    jobs = _stress_jobs(); om = oracle_tiny
    want = [_full_key(om.full(pcm, _params(om, **kw))) for pcm, kw in jobs]
    m_e = eng.Model(tiny_model_path); m_f = eng.Model(tiny_model_path)
    cf = eng.Context(m_f, max_batch=8, max_samples=16000 * 31); cf.set_precision("f16_mfma")
    alone = [_full_key(cf.full_batch([pcm], _params(cf, **kw))[0]) for pcm, kw in jobs]
    cf.close()
    bad = []; checked = {"exact": 0, "f16_mfma": 0}

    def run(kind, seed):
        try:
            draw = np.random.default_rng(seed)
            for shape in ((16, 16000 * 31), (8, 16000 * 32 + 1024), (64, 16000 * 31)):      # the node re-creates its workspace as instances come and go
                ctx = eng.Context(m_e if kind == "exact" else m_f, max_batch=shape[0], max_samples=shape[1]); ctx.set_precision(kind)
                try:
                    for rep in range(5):
                        size = int(draw.integers(2, 9)); comp = [int(x) for x in draw.choice(14, size=size, replace=rep == 4)]
                        res = ctx.full_batch([jobs[k][0] for k in comp], params=[_params(ctx, **jobs[k][1]) for k in comp])
                        res.append(ctx.full_batch([jobs[comp[0]][0]], _params(ctx, **jobs[comp[0]][1]))[0]); comp = comp + [comp[0]]
                        for r, k in zip(res, comp):
                            checked[kind] += 1
                            if _full_key(r) != (want[k] if kind == "exact" else alone[k]):
                                bad.append((kind, shape, comp, k))
                finally:
                    ctx.close()
        except Exception as e:      # noqa: BLE001
            bad.append((kind, repr(e)))

    ths = [threading.Thread(target=run, args=("exact", 11)), threading.Thread(target=run, args=("f16_mfma", 12))]
    [t.start() for t in ths]; [t.join() for t in ths]
    m_e.close(); m_f.close()
    assert not bad, bad
    assert checked["exact"] >= 45 and checked["f16_mfma"] >= 45, checked


LADDER_SETS = [{}, {"temperature_inc": 0.0}, {"temperature_inc": 0.4}, {"logprob_thold": -5.0}, {"temperature": 0.4}, {"entropy_thold": 5.0}]
LADDER_FALLBACKS = [1, 1, 3, 0, 4, 6]      # fallback_requested per set, on each of the three clips (CPU oracle, generator seeded with 0)


def test_mixed_call_runs_each_clips_own_temperature_ladder(eng):
    """A model whose greedy pass fails the default log-prob threshold (test_gpu_plugin.py's micro, gamma_text 8): three clips x six ladder settings, 18 rows in one mixed call,
    each with its own fresh generator.  Ladders of different length, thresholds and starting temperatures per row: every row equals the oracle's full() on its own generator,
    fallback_requested and the generator state afterwards included."""
    from conftest import _ensure_built
    path = "/tmp/skw_test_micro_gamma8.bin"
    if not os.path.exists(path):
        subprocess.check_call([_ensure_built(), path + ".tmp", "--size", "micro", "--gamma_text", "8"]); os.replace(path + ".tmp", path)
    om = OracleModel(path)
    clips = [(61, 8), (62, 8), (63, 20)]
    pcms = [synth.clip(c, 16000 * s) for c, s in clips]
    rows = [(ci, si) for ci in range(3) for si in range(len(LADDER_SETS))]
    m = eng.Model(path); ctx = eng.Context(m, max_batch=len(rows), max_samples=16000 * 21)
    states = [eng.rng_state_new() for _ in rows]
    try:
        res = ctx.full_batch([pcms[ci] for ci, _ in rows], params=[_params(ctx, **LADDER_SETS[si]) for _, si in rows], rng_states=states)
    finally:
        ctx.close(); m.close()
    want = {}
    for (ci, si), g, st in zip(rows, res, states):
        ost = eng.rng_state_new()
        o = want[(ci, si)] = om.full(pcms[ci], _params(om, **LADDER_SETS[si]), rng_state=ost)
        _same_as_oracle(g, o, (clips[ci], LADDER_SETS[si]))
        assert np.array_equal(st, ost), (clips[ci], LADDER_SETS[si], "generator state after the call")
    om.close()
    for ci in range(3):
        assert [want[(ci, si)]["fallback_requested"] for si in range(len(LADDER_SETS))] == LADDER_FALLBACKS, clips[ci]
        for si in range(1, len(LADDER_SETS)):
            assert _ids(want[(ci, si)]) != _ids(want[(ci, 0)]), (clips[ci], LADDER_SETS[si])


def _key(res):
    return [([tuple(np.float32(x).view(np.uint32) if isinstance(x, float) else x for x in t) for t in r["tokens"]], [(s["t0"], s["t1"], s["text"]) for s in r["segments"]],
             r["n_windows"], r["fallback_requested"], r["lang_id"], r["n_decode_steps"]) for r in res]


def test_equal_parameters_give_the_uniform_call(eng, tiny_model_path):
    """A parameter array whose entries are all the default == skw_full_batch_rng on the same ragged batch (multi-window clips with long prompts, a clip too short to transcribe),
    in both precisions, bit for bit — in f16_mfma too: the batch composition is identical."""
    from test_gpu_switches import CLIPS, MAXS
    pcms = [synth.clip(c, n) for c, n in CLIPS[:8]]
    m = eng.Model(tiny_model_path); ctx = eng.Context(m, max_batch=len(pcms), max_samples=MAXS)
    try:
        for precision in ("exact", "f16_mfma"):
            ctx.set_precision(precision)
            su = [eng.rng_state_new() for _ in pcms]; sm = [eng.rng_state_new() for _ in pcms]
            uni = ctx.full_batch(pcms, ctx.default_params(), rng_states=su)
            mix = ctx.full_batch(pcms, params=[ctx.default_params() for _ in pcms], rng_states=sm)
            assert _key(mix) == _key(uni), precision
            assert all(np.array_equal(a, b) for a, b in zip(su, sm)), precision
            assert sum(len(r["tokens"]) for r in uni) > 500
    finally:
        ctx.close(); m.close()


def test_mixed_call_f16_mfma_equals_the_uniform_call_on_each_clip_alone(eng, tiny_model_path):
    """f16_mfma: batch composition reaches the arithmetic only through a prompt pass of >= 256 rows.  Single-window clips x the seven parameter sets in one
    mixed call — prompts of 3 or 4 tokens per row, 21 rows: far below that — must equal, bit for bit, the uniform f16_mfma call on each clip alone with its parameters."""
    clips = TINY_CLIPS[:3]
    pcms = [synth.clip(c, 16000 * s) for c, s in clips]
    rows = [(ci, si) for si in range(len(TINY_SETS)) for ci in range(3)]
    assert sum(3 + TINY_SETS[si].get("no_timestamps", 0) for _, si in rows) < 256      # the precondition, checked: all prompt rows of the call together
    m = eng.Model(tiny_model_path); ctx = eng.Context(m, max_batch=len(rows), max_samples=16000 * 10)
    try:
        ctx.set_precision("f16_mfma")
        mix = ctx.full_batch([pcms[ci] for ci, _ in rows], params=[_params(ctx, **TINY_SETS[si]) for _, si in rows])
        alone = [ctx.full_batch([pcms[ci]], _params(ctx, **TINY_SETS[si]))[0] for ci, si in rows]
    finally:
        ctx.close(); m.close()
    for (ci, si), a, b in zip(rows, _key(mix), _key(alone)):
        assert a == b, (clips[ci], TINY_SETS[si])
    assert len({tuple(_ids(r)) for r in mix}) >= 9      # the rows are not all one transcript


# ------------------------------------------------------------------ the node
NODE_SETS = [{"language": "en", "suppress_blank": True, "suppress_non_speech_tokens": True}, {"language": "de", "suppress_blank": False, "suppress_non_speech_tokens": True},
             {"language": "auto", "suppress_blank": True, "suppress_non_speech_tokens": False}]


def _node_round(plugin, model_path, pcms, mixed_batch):
    """twelve instances, one thread each: feed the clip (no cut: it is shorter than a segment), meet at the barrier, flush — the twelve tails queue together"""
    n = 12
    nodes = [plugin.create_node(dict(NODE_SETS[k % 3], model_path=model_path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=200, max_batch=16,
                                     mixed_batch=mixed_batch)) for k in range(n)]
    barrier = threading.Barrier(n); errors = []; outs = [None] * n
    before = minihost.whisper_batch_stats()

    def worker(k):
        try:
            pcm = pcms[k % 2]
            for i in range(0, pcm.size, 960):
                assert nodes[k].process_audio(pcm[i:i + 960]) == 0, nodes[k].last_error()
            barrier.wait(timeout=120)
            assert nodes[k].flush() == 0, nodes[k].last_error()
            outs[k] = [json.loads(o[2].decode()) for o in nodes[k].outputs()]
        except Exception as e:      # noqa: BLE001
            errors.append((k, repr(e))); barrier.abort()

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(n)]
    [t.start() for t in ths]; [t.join() for t in ths]
    after = minihost.whisper_batch_stats()
    for nd in nodes:
        nd.destroy()
    assert not errors, errors
    return outs, tuple(a - b for a, b in zip(after, before))


def test_node_batches_differently_configured_instances_together(plugin, tiny_model_path, oracle_tiny):
    """Twelve instances under three parameter sets (language en / de / auto crossed with the two suppress_* flags) whose segments arrive together: with mixed_batch (the default)
    they share engine calls — fewer than twelve, at least one of them carrying different parameter blocks — and with mixed_batch: false no call does; either way every
    transcript is the oracle's for that instance's audio and parameters."""
    om = oracle_tiny
    pcms = [synth.clip(31, 16000 * 6), synth.clip(32, 16000 * 6 + 800)]
    want = {}
    for k in range(6):
        cfg = NODE_SETS[k % 3]
        po = _params(om, suppress_blank=int(cfg["suppress_blank"]), suppress_nst=int(cfg["suppress_non_speech_tokens"]), lang_id={"en": 0, "de": 2, "auto": -1}[cfg["language"]])
        r = om.full(pcms[k % 2], po)
        want[k] = [{"text": s["text"].decode().strip(), "start_time_ms": s["t0"] * 10, "end_time_ms": s["t1"] * 10, "confidence": None} for s in r["segments"] if s["text"].decode().strip()]
        assert want[k]

    def check(outs):
        for k, got in enumerate(outs):      # instance k: set k % 3, clip k % 2 == (k % 6)'s
            segs = want[k % 6]
            assert len(got) == 1 and got[0]["segments"] == segs and got[0]["text"] == " ".join(s["text"] for s in segs), k
            assert got[0]["language"] == NODE_SETS[k % 3]["language"], k

    outs, (calls, jobs, mixed) = _node_round(plugin, tiny_model_path, pcms, True)
    print("mixed_batch on: %d engine calls for %d jobs, %d of them mixed" % (calls, jobs, mixed))
    check(outs)
    assert jobs == 12 and mixed >= 1 and calls < 12, (calls, jobs, mixed)
    outs, (calls, jobs, mixed) = _node_round(plugin, tiny_model_path, pcms, False)
    print("mixed_batch off: %d engine calls for %d jobs, %d of them mixed" % (calls, jobs, mixed))
    check(outs)
    assert jobs == 12 and mixed == 0, (calls, jobs, mixed)


def test_english_only_model_refuses_auto_detection_naming_the_clip(eng):
    """lang_id < 0 on a model without language tokens: the uniform call's message, with the index of the first clip that asked."""
    from conftest import synth_model
    path = synth_model("tiny", vocab=51864)
    pcm = synth.clip(3, 16000 * 4)
    m = eng.Model(path); ctx = eng.Context(m, max_batch=4, max_samples=16000 * 5)
    try:
        with pytest.raises(RuntimeError, match=r"failed to auto-detect language: the model is not multilingual \(clip 2\)"):
            ctx.full_batch([pcm] * 3, params=[_params(ctx), _params(ctx, suppress_nst=1), _params(ctx, lang_id=-1)])
        ok = ctx.full_batch([pcm] * 2, params=[_params(ctx), _params(ctx, suppress_nst=1)])      # the context is usable afterwards
        assert len(ok) == 2 and len(ok[0]["tokens"]) > 0
    finally:
        ctx.close(); m.close()


def test_a_refused_request_does_not_fail_its_batch_neighbours(plugin):
    """Instances on an English-only model whose segments queue together, one configured `language: auto` (which such a model refuses): the refusal is that instance's own
    error; the `en` instances beside it — differently configured among themselves, so their call is a mixed one — get the oracle's transcripts."""
    from conftest import synth_model
    path = synth_model("tiny", vocab=51864)
    om = OracleModel(path)
    pcm = synth.clip(33, 16000 * 5)
    sets = [{"language": "en", "suppress_non_speech_tokens": True}, {"language": "auto"}, {"language": "en", "suppress_non_speech_tokens": False}, {"language": "auto"}]
    nodes = [plugin.create_node(dict(st, model_path=path, vad_mode="always", flush_tail=True, precision="exact", batch_window_ms=200, max_batch=8)) for st in sets]
    barrier = threading.Barrier(len(nodes)); rcs = [None] * len(nodes); errors = []

    def worker(k):
        try:
            for i in range(0, pcm.size, 960):
                assert nodes[k].process_audio(pcm[i:i + 960]) == 0, nodes[k].last_error()
            barrier.wait(timeout=120)
            rcs[k] = nodes[k].flush()
        except Exception as e:      # noqa: BLE001
            errors.append((k, repr(e))); barrier.abort()

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(len(nodes))]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert not errors, errors
    for k, st in enumerate(sets):
        if st["language"] == "auto":
            assert rcs[k] != 0 and "failed to auto-detect language" in nodes[k].last_error() and not nodes[k].outputs(), (k, rcs[k], nodes[k].last_error())
        else:
            assert rcs[k] == 0, (k, nodes[k].last_error())
            r = om.full(pcm, _params(om, suppress_nst=int(st["suppress_non_speech_tokens"])))
            segs = [{"text": s["text"].decode().strip(), "start_time_ms": s["t0"] * 10, "end_time_ms": s["t1"] * 10, "confidence": None} for s in r["segments"] if s["text"].decode().strip()]
            got = [json.loads(o[2].decode()) for o in nodes[k].outputs()]
            assert segs and len(got) == 1 and got[0]["segments"] == segs, k
    for nd in nodes:
        nd.destroy()
    om.close()
