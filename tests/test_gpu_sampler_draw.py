"""k_dec_sample and k_dec_sample_stream at a temperature and on greedy near-ties, against oracle/ (skwo_debug_sample_logits) bit for bit — every instantiation the engine
launches, each reported by the hook (skw_debug_sample_rows_ex) and asserted: k_dec_sample<TRACE, DRAW, ROWS> for the greedy step's <false, false, *>, the ladder's
<false, true, *> and the trace form, k_dec_sample_stream<ROWS>.  Rows, generator states and the numpy reference of the draw: tests/sampler_draw_lib.py (its CPU tier is
tests/test_cpu_sampler_draw.py).  64 rows per launch, every row on a generator of its own; all-greedy launches and launches that hold greedy rows beside sampled ones.

Compared per row and run: id, tid, p, plog, pt, ptsum, margin, no_speech_prob; the whole f32 probs row of a sampled row; the filtered row (streaming form); all 625 words
of the generator after the launch (a greedy row's untouched); the drawn index against the numpy reference on the kernel's own probs; n_tokens / cur_token after the launch.
No row is skipped or tolerated: the rows compared are counted and the total asserted."""
import collections

import numpy as np
import pytest

import conftest
import sampler_draw_lib as sd

pytestmark = pytest.mark.gpu
TOKEN_FIELDS = ("id", "tid", "p", "plog", "pt", "ptsum", "margin")


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def _run_model(path, reduced):
    from streamkit_amd import engine
    from oracle_lib import OracleModel
    import logit_rules_lib as lr
    om = OracleModel(path); po = om.default_params()
    gm = engine.Model(path, device=0); ctx = engine.Context(gm, max_batch=64)
    try:
        NV = om.hp.n_vocab; eot = lr.special_ids(om)["eot"]
        assert NV == ctx.model.hp.n_vocab
        greedy, sampled = sd.all_cases(om, po, reduced)
        launches = sd.launches(greedy, sampled)
        want = {}      # the oracle's side and numpy's u, once per row
        for c in greedy + sampled:
            o = sd.oracle_sample(om, po, c); o["u"] = sd.generator_ref(c["state"])[0] if c["temperature"] > 0 else None
            want[c["name"]] = o
        p = ctx.default_params()
        stats = collections.OrderedDict(); bad = []; n_rows = n_expected = 0
        first_mixed = next(i for i, b in enumerate(launches) if any(c["temperature"] > 0 for c in b))
        for li, batch in enumerate(launches):
            R = len(batch)
            hists = [c["hist"] for c in batch]; lg = np.stack([c["raw"] for c in batch]); T = np.array([c["temperature"] for c in batch], np.float32)
            any_sampled = bool((T > 0).any())
            per_row_forms = (False, True) if (li % 3 == 0 or li == first_mixed) else (False,)
            for per_row in per_row_forms:
                rw = "true" if per_row else "false"
                runs = [("form0/trace_off", dict(form=0, trace=False), "k_dec_sample<false, %s, %s>" % ("true" if any_sampled else "false", rw)),
                        ("form0/trace_on", dict(form=0, trace=True), "k_dec_sample<true, true, %s>" % rw),
                        ("form1", dict(form=1, trace=False, want_filtered=True), "k_dec_sample_stream<%s>" % rw)]
                for run, kw, kernel in runs:
                    st = np.stack([c["state"] for c in batch]).astype(np.uint32)
                    tk, tr, filt, ex = ctx.sample_rows(hists, lg, [p] * R if per_row else p, temperature=T, rng_state=st, extras=True, **kw)
                    assert ex["kernel"] == kernel, (li, run, ex["kernel"], kernel)
                    s = stats.setdefault(kernel, dict(launches=0, rows=0, sampled=0, mismatches=0)); s["launches"] += 1
                    n_expected += R
                    for r, c in enumerate(batch):
                        o = want[c["name"]]; where = (c["name"], run, kernel); errs = []
                        for f in TOKEN_FIELDS:
                            if (int(tk[f][r]) != o["tok"][f]) if f in ("id", "tid") else (_bits(tk[f][r]) != _bits(o["tok"][f])):
                                errs.append("%s %r != %r" % (f, tk[f][r], o["tok"][f]))
                        if _bits(ex["no_speech_prob"][r]) != _bits(o["no_speech_prob"]):
                            errs.append("no_speech_prob %r != %r" % (ex["no_speech_prob"][r], o["no_speech_prob"]))
                        if int(ex["n_tokens"][r]) != len(c["hist"]) + 1 or int(ex["cur_token"][r]) != int(tk["id"][r]) or (int(tk["id"][r]) == eot and ex["active"][r] != 0):
                            errs.append("state after: n_tokens %d cur_token %d active %d" % (ex["n_tokens"][r], ex["cur_token"][r], ex["active"][r]))
                        if not np.array_equal(st[r], o["state"]):
                            errs.append("generator state differs in %d words (index %d, oracle %d)" % (int((st[r] != o["state"]).sum()), st[r][624], o["state"][624]))
                        if c["temperature"] > 0:
                            s["sampled"] += 1
                            if not np.array_equal(ex["probs"][r].view(np.uint32), o["probs"].view(np.uint32)):
                                errs.append("probs row differs in %d entries" % int((ex["probs"][r].view(np.uint32) != o["probs"].view(np.uint32)).sum()))
                            elif sd.draw_ref(ex["probs"][r], o["u"])[0] != int(tk["id"][r]):
                                errs.append("drawn %d, numpy reference on the kernel's probs %d (u %r)" % (tk["id"][r], sd.draw_ref(ex["probs"][r], o["u"])[0], o["u"]))
                        elif not np.array_equal(st[r], c["state"]):
                            errs.append("a greedy row moved its generator")
                        if filt is not None and not np.array_equal(filt[r].view(np.uint32), o["filtered"].view(np.uint32)):
                            errs.append("filtered row differs in %d entries" % int((filt[r].view(np.uint32) != o["filtered"].view(np.uint32)).sum()))
                        if kw["trace"] and int(tr["chosen_id"][r]) != o["tok"]["id"]:
                            errs.append("trace chosen_id %d" % tr["chosen_id"][r])
                        s["rows"] += 1; n_rows += 1
                        if errs:
                            s["mismatches"] += 1; bad.append((where, errs))
        print("\nn_vocab %d: %d rows (%d greedy, %d sampled) in %d launches of the case list; kernel: launches / rows compared (sampled among them) / rows with a mismatch"
              % (NV, len(greedy) + len(sampled), len(greedy), len(sampled), len(launches)))
        for k, s in stats.items():
            print("  %-36s %3d / %5d (%4d) / %d" % (k, s["launches"], s["rows"], s["sampled"], s["mismatches"]))
        for where, errs in bad[:40]:
            print("  MISMATCH", where, "; ".join(errs))
        assert not bad, "%d rows differ from the oracle" % len(bad)
        assert n_rows == n_expected and n_rows >= 3 * (len(greedy) + len(sampled))
        return stats
    finally:
        ctx.close(); gm.close(); om.close()


ALL_KERNELS = {"k_dec_sample<%s, %s, %s>" % (t, d, r) for t, d in (("false", "false"), ("false", "true"), ("true", "true")) for r in ("false", "true")} | \
              {"k_dec_sample_stream<false>", "k_dec_sample_stream<true>"}


def test_sampler_draws_and_near_ties_match_the_oracle_tiny(tiny_model_path):
    stats = _run_model(tiny_model_path, reduced=False)
    assert set(stats) == ALL_KERNELS and all(s["rows"] > 0 for s in stats.values())      # all six k_dec_sample instantiations and both streaming forms ran


@pytest.mark.parametrize("vocab,mels", [(51864, 80), (51866, 128)])
def test_sampler_draws_and_near_ties_match_the_oracle_other_vocabularies(vocab, mels):
    """*.en's and large-v3's vocabularies: tok_eot / tok_beg, the last stripe's tail and the kill-bit packing move; the reduced set"""
    stats = _run_model(conftest.synth_model("micro", vocab=vocab, mels=mels), reduced=True)
    assert set(stats) == ALL_KERNELS


def test_hook_rejects_a_bad_generator_state_and_a_draw_without_one(tiny_model_path):
    from streamkit_amd import engine
    gm = engine.Model(tiny_model_path, device=0); ctx = engine.Context(gm, max_batch=4)
    try:
        NV = gm.hp.n_vocab
        st = sd.mt_state(0, 625)[None, :].copy()
        with pytest.raises(RuntimeError, match="not a std::mt19937 state"):
            ctx.sample_rows([[]], np.zeros((1, NV), np.float32), temperature=[0.5], rng_state=st)
        with pytest.raises(RuntimeError, match="needs rng_state"):
            ctx.sample_rows([[]], np.zeros((1, NV), np.float32), temperature=[0.5])
    finally:
        ctx.close(); gm.close()
