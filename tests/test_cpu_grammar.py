"""Grammar-constrained decoding without a GPU (include/skw_grammar.h, streamkit_amd/csrc/skw_grammar_compile.h):
  (a) the pattern compiler against Python's re — the DFA accepts exactly what re.fullmatch on the bytes pattern accepts, on 2 000 strings per pattern; every state of a compiled
      table reaches an accepting one; malformed and oversized patterns are errors with a message.  tests/cpp/grammar_main.cpp, built plain and with ASan + UBSan, runs all of it
  (b) the header's evaluator against the numpy restatement of tests/grammar_lib.py, bit for bit, on all three vocabularies
  (c) skw_grammar_check
  (d) the conditions under which tests/test_gpu_grammar.py shows anything, asserted on the oracle alone."""
import re

import numpy as np
import pytest

import context_ref_lib as cr
import grammar_lib as gl
import logit_rules_lib as lr
from conftest import synth_model

PRINTABLE = bytes(range(32, 127))
# (pattern, the alphabet its random strings are drawn from)
PATTERNS = [
    (r"abc", b"abcd"), (r"a|b|cd", b"abcd"), (r"(ab|cd)e", b"abcde"), (r"ab?c", b"abc"), (r"ab*c", b"abc"), (r"ab+c", b"abc"),
    (r"a{3}", b"ab"), (r"a{2,}", b"ab"), (r"a{1,3}b", b"ab"), (r"(ab){2,3}", b"ab"), (r"(a|bc)*", b"abc"), (r"(a*)*b", b"ab"), (r"(a|)b", b"ab"),
    (r"[0-9]{2,5}", b"0123456789a"), (r" ?(yes|no|maybe)", b" yesnomabYN"), (r"( [a-z]{3,8}){1,3}", b" abcxyz"), (r"\d+", b"0129a "), (r"\D+", b"0129a "),
    (r"\w+", b"aZ_09- "), (r"\W+", b"aZ_09- ."), (r"\s*x\s*", b" \t\n\r\f\vx"), (r"\S+", b" \tab"), (r"a.c", b"abc\n\x00\xff"), (r".*", b"ab\n"),
    (r"[abc]+", b"abcd"), (r"[^abc]+", b"abcdX"), (r"[a-cx-z]+", b"abcdwxyz"), (r"[]a]+", b"]ab"), (r"[^]a]+", b"]abc"), (r"[a-]+", b"a-b"), (r"[-a]+", b"a-b"),
    (r"[\d\s]+x", b"01 \tx"), (r"[\]\\]+", b"]\\a"), (r"[^\w]+", b"a_ -0"), (r"\.\*\+\?\(\)\[\]\{\}\|\\", b".*+?()[]{}|\\"), (r"a\|b", b"a|b"),
    (r"\n\t\r", b"\n\t\rnt"), (r"café( crème)?", "café crème".encode("utf-8")), (r"[é]+", "ée".encode("utf-8")), (r"(yes|no)[.!?]?", b"yesno.!?"),
    (r"(north|south|east|west)( (north|south|east|west))*", b" northsuaew"), (r"[A-Z][a-z]+( [A-Z][a-z]+)?", b" ABab"), (r"x{0}y", b"xy"), (r"(a{2}){2}", b"a"),
    (r"(a|b)*abb", b"ab"), (r"[Z-a]+", b"YZ[\\]^_`abz"), (r"a]b}", b"a]b}"), (r"(\d{1,3}\.){3}\d{1,3}", b"0129."), (r"-?\d+(\.\d+)?", b"-.059"),
]
assert len(PATTERNS) >= 40
CASES = [(p, a, f) for p, a in PATTERNS for f in (0, gl.IGNORE_CASE)]
N_STRINGS = 2000


def _pat_bytes(p):
    return p.encode("utf-8")


def _strings(rng, table, alphabet, ignore_case):
    """700 random strings over the alphabet, 650 strings that walk the table to an accepting state, 650 single-byte mutations of those"""
    alpha = bytes(set(alphabet + (alphabet.swapcase() if ignore_case else b"")))
    out = [b""] + [bytes(rng.choice(list(alpha), size=int(rng.integers(0, 13)))) for _ in range(699)]
    nxt, acc = table["next"], table["accept"]
    live = [np.nonzero(nxt[s] != gl.DEAD)[0] for s in range(acc.size)]
    walks = []
    while len(walks) < 650:
        s, w = 0, []
        for _ in range(64):
            if acc[s] and (live[s].size == 0 or rng.random() < 0.3):
                break
            if live[s].size == 0:
                break
            pref = np.array([b for b in live[s] if b in alpha] or live[s])      # mostly bytes of the alphabet, so the strings stay readable
            b = int(rng.choice(pref if rng.random() < 0.9 else live[s]))
            w.append(b); s = int(nxt[s, b])
        walks.append(bytes(w))
    out += walks
    for k in range(650):
        w = bytearray(walks[k])
        kind = int(rng.integers(0, 3)) if w else 1
        at = int(rng.integers(0, len(w) + (kind == 1)))
        if kind == 0:
            w[at] = int(rng.choice(list(alpha))) if rng.random() < 0.8 else int(rng.integers(0, 256))
        elif kind == 1:
            w.insert(at, int(rng.choice(list(alpha))))
        else:
            del w[at]
        out.append(bytes(w))
    assert len(out) == N_STRINGS
    return out


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("grammar")
    return d, {False: gl.build_driver(d, False), True: gl.build_driver(d, True)}


# ---- (a) the compiler against re
def test_compiler_accepts_exactly_what_re_fullmatch_accepts(drivers):
    d, exe = drivers
    pats = [(_pat_bytes(p), f) for p, _, f in CASES]
    tables = gl.run_compile(exe[False], d, [(pb, f, []) for pb, f in pats])
    rng = np.random.default_rng(20261020)
    corpus = []
    for (pb, f), (_, alpha, _), t in zip(pats, CASES, tables):
        assert t["rc"] == 0, (pb, f, t)
        corpus.append((pb, f, _strings(rng, t, alpha, bool(f))))
    n_match = n_miss = 0
    for sanitize in (False, True):                       # both builds run the whole corpus
        got = gl.run_compile(exe[sanitize], d, corpus)
        for (pb, f, strings), g, t in zip(corpus, got, tables):
            assert g["rc"] == 0 and np.array_equal(g["next"], t["next"]) and np.array_equal(g["accept"], t["accept"])      # (the compiler is deterministic)
            rx = re.compile(pb, gl.py_flags(f))
            want = np.array([rx.fullmatch(s) is not None for s in strings])
            bad = np.nonzero(want != g["accepted"])[0]
            assert bad.size == 0, (pb, f, [(strings[k], bool(want[k])) for k in bad[:5]])
            assert want.sum() >= 300 and (~want).sum() >= 300 or pb in (b".*",), (pb, f, int(want.sum()))      # both outcomes are well represented
            n_match += int(want.sum()); n_miss += int((~want).sum())
            # the trimmed table: every state reaches an accepting one, state 0 included, and no entry leaves the table
            nxt, acc = g["next"], g["accept"]
            assert acc.size <= gl.MAX_STATES and set(np.unique(acc)) <= {0, 1} and ((nxt < acc.size) | (nxt == gl.DEAD)).all()
            live = acc.astype(bool).copy()
            for _ in range(acc.size):
                reach = np.array([live[row[row != gl.DEAD]].any() for row in nxt]) | live
                if (reach == live).all():
                    break
                live = reach
            assert live.all(), (pb, f, np.nonzero(~live)[0][:5])
    assert n_match > 40000 and n_miss > 40000


MALFORMED = [b"", b"(", b"(ab", b"ab)", b"[ab", b"a{2", b"a{3,2}", b"*a", b"a**", b"a+?", b"a{,3}", b"(?:a)", b"(?i)a", b"^a", b"a$", b"\\b", b"\\1", b"a\\", b"[z-a]", b"[a-\\d]",
             b"a{2000}", b"(" * 100 + b"a" + b")" * 100, b"(a{1000}){1000}", b"[ab]*a[ab]{12}", b"((a|b)*a(a|b){11}c)|d", b"a{"]


def test_malformed_and_oversized_patterns_are_errors_not_crashes(drivers):
    d, exe = drivers
    for sanitize in (False, True):
        got = gl.run_compile(exe[sanitize], d, [(p, 0, []) for p in MALFORMED] + [(b"[ab]*a[ab]{10}", 0, [])])
        for p, g in zip(MALFORMED, got):
            assert g["rc"] != 0 and g["err"].startswith("grammar: ") and len(g["err"]) > 12, (p, g)
        assert "4096" in got[MALFORMED.index(b"[ab]*a[ab]{12}")]["err"]
        assert got[-1]["rc"] == 0 and 2048 <= got[-1]["accept"].size <= 4096      # the largest of that family that fits compiles


def test_binding_compiles_through_the_library(built):
    from streamkit_amd import engine
    g = engine.Grammar.compile(" ?(yes|no|maybe)", penalty=7.5)
    assert g.matches(b" yes") and g.matches(b"maybe") and not g.matches(b"ye") and not g.matches(b"YES") and g.walk(b"ye") != gl.DEAD and g.walk(b"x") == gl.DEAD
    assert g.rec.n_states == g.n_states and g.rec.penalty == 7.5
    assert engine.Grammar.compile("yes", ignore_case=True).matches(b"yEs")
    with pytest.raises(ValueError, match="unbalanced"):
        engine.Grammar.compile("(yes")
    with pytest.raises(ValueError, match="penalty"):
        engine.Grammar.compile("yes", penalty=0.0)


# ---- (c) the check of a record
def test_check_names_the_clip_and_the_field(drivers):
    d, exe = drivers
    ok = gl.chain_table(3)
    assert gl.run_check(exe[True], d, ok) is None and gl.run_check(exe[True], d, gl.chain_table(4096)) is None
    bad_next = gl.chain_table(3); bad_next["next"][1, 7] = 3
    bad_acc = gl.chain_table(3); bad_acc["accept"][2] = 2
    for g, what in ((dict(ok, penalty=0.0), "penalty"), (dict(ok, penalty=-1.0), "penalty"), (dict(ok, penalty=float("inf")), "penalty"), (dict(ok, penalty=float("nan")), "penalty"),
                    (bad_next, "next[1][7]"), (bad_acc, "accept[2]"), (gl.chain_table(4097), "n_states"), (dict(next=np.zeros((0, 256), np.uint16), accept=np.zeros(0, np.uint8), penalty=1.0),
                                                                                                       "n_states")):
        msg = gl.run_check(exe[True], d, g)
        assert msg is not None and msg.startswith("clip 7: grammar: ") and what in msg, (what, msg)


# ---- (b) the evaluator against the restatement
@pytest.mark.parametrize("vocab,mels", [(51865, 80), (51864, 80), (51866, 128)])
def test_evaluator_equals_the_restatement_bit_for_bit(drivers, vocab, mels):
    from oracle_lib import OracleModel
    d, exe = drivers
    om = OracleModel(synth_model("micro", vocab=vocab, mels=mels))
    try:
        sp = lr.special_ids(om); eot, beg, NV = sp["eot"], sp["beg"], om.hp.n_vocab
        voc = gl.vocab_image(om.token_bytes, eot)
        assert NV == vocab and voc[0].size == eot + 1
        rng = np.random.default_rng(vocab)
        grams = [gl.compile_py(p, penalty=pen) for p, pen in ((gl.TEST_PATTERNS["digits"], 100.0), (gl.TEST_PATTERNS["yesno"], 4096.0), (gl.TEST_PATTERNS["words"], 0.5),
                                                              (r"( ?[a-z]+)*", 100.0))]
        grams += [gl.letters_table(1, 3.0), gl.letters_table(2, 100.0), gl.letters_table(4096, 100.0), gl.chain_table(4096, 12.5)]
        ids_of = {}
        for t in range(eot):
            ids_of.setdefault(bytes(om.token_bytes(t)), t)
        word_ids = [t for t in range(256, 3000) if bytes(om.token_bytes(t)).startswith(b" ") and bytes(om.token_bytes(t))[1:].isalpha()]
        spell = lambda s: [ids_of[bytes([c])] for c in s]
        ts = lambda k: [beg + k, beg + k]
        hists = {
            0: [[], spell(b"4"), spell(b"41") + ts(3), ts(1) + spell(b"4") + ts(2) + spell(b"15") + [beg + 9], spell(b"41578"), spell(b"4a"), spell(b"415789")],
            1: [[], spell(b" ye"), spell(b" yes"), [ids_of[b" "]] + ts(5) + spell(b"mayb"), spell(b"maybe"), spell(b"nope")],
            2: [[], word_ids[:1], word_ids[:2] + ts(7), word_ids[:3], word_ids[:4], spell(b"x")],
            3: [[], word_ids[:5] + spell(b"abc"), spell(b"A")],
            4: [[], word_ids[:2], spell(b"7")], 5: [[], word_ids[:3]], 6: [[], word_ids[:40], [beg] + word_ids[:150] + ts(40), spell(b"abc") * 70],
            7: [[], spell(b"a") * 5, spell(b"a") * 223, spell(b"ab")],
        }
        rows = []
        for gi, hs in hists.items():
            for h in hs:
                x = (rng.standard_normal(NV) * 30.0).astype(np.float32)
                x[rng.integers(0, NV, 5)] = -np.inf; x[rng.integers(0, NV, 3)] = 0.0
                rows.append((gi, h, x))
        for sanitize in (False, True):
            got = gl.run_eval(exe[sanitize], d, voc, eot, NV, grams, rows)
            seen = set()
            for (gi, h, x), (s, y) in zip(rows, got):
                ws, want = gl.apply(grams[gi], voc, eot, h, x)
                assert s == ws and np.array_equal(y.view(np.uint32), want.view(np.uint32)), (vocab, gi, h[:6])
                assert np.array_equal(y[eot + 1:].view(np.uint32), x[eot + 1:].view(np.uint32))      # specials and timestamps are untouched
                changed = int((y.view(np.uint32) != x.view(np.uint32)).sum())
                seen.add("dead" if s == gl.DEAD else ("accept" if grams[gi]["accept"][s] else "open"))
                if s == gl.DEAD:
                    assert changed == 0
                else:
                    assert changed > 0 and (y[eot] != x[eot]) == (not grams[gi]["accept"][s])
            assert seen == {"dead", "accept", "open"}
    finally:
        om.close()


# ---- (d) the conditions of the GPU tests, on the oracle alone
@pytest.fixture(scope="module")
def micro_refs(oracle_micro):
    from streamkit_amd import synth
    om = oracle_micro
    sp = lr.special_ids(om)
    voc = gl.vocab_image(om.token_bytes, sp["eot"])
    p = cr.params_for(om); p.no_timestamps = 1
    return om, sp, voc, p, {s: synth.clip(s, gl.N_SAMPLES) for s in gl.TEST_SEEDS}


def test_conditions_under_which_the_gpu_tests_show_anything(micro_refs):
    om, sp, voc, p, clips = micro_refs
    eot = sp["eot"]
    n_max = om.hp.n_text_ctx // 2 - 4
    rx = {k: re.compile(v.encode()) for k, v in gl.TEST_PATTERNS.items()}
    stats = {}
    for seed, pcm in clips.items():
        plain = gl.full_with_grammar(om, pcm, None, voc, params=p, stats=stats)
        text = b"".join(s["text"] for s in plain["segments"])
        assert len(text) > 0 and all(r.fullmatch(text) is None for r in rx.values()), (seed, text)                      # (a) unconstrained, no clip matches any pattern
        for name, pat in gl.TEST_PATTERNS.items():
            g = gl.compile_py(pat, penalty=gl.TEST_PENALTY)
            out = gl.full_with_grammar(om, pcm, g, voc, params=p, stats=stats)
            assert out["n_windows"] == 1 and len(out["passes"]) == 1 and out["failed_passes"] == 0
            ids = out["passes"][0]
            assert ids[-1] == eot and len(ids) < n_max and len(ids) <= 32, (seed, name, ids)                               # (c) ends on <|endoftext|>, well inside the budget
            got = gl.transcript_bytes(om.token_bytes, ids, eot)
            assert rx[name].fullmatch(got) is not None, (seed, name, got)
            assert b"".join(s["text"] for s in out["segments"]) == got
    assert 0 < stats["spread"] < gl.TEST_PENALTY, stats                                                                   # (b) the penalty exceeds every spread seen
