"""Grammar-constrained decoding (include/skw_grammar.h): what the tests share.
  apply            an independent numpy restatement of the rule k_dec_grammar applies to a row of logits (the header's evaluator walks token by token; this one walks all tokens
                   at once, byte position by byte position)
  full_with_grammar  decode_rules_lib.full_with_rules with `apply` composed behind its transform, in front of the oracle's K11: the end-to-end checker of
                   skw_full_batch_grammar at temperature_inc = 0.  It also records the largest max - min spread of finite logits it saw.
  the driver       tests/cpp/grammar_main.cpp built with g++ (plain / sanitized) and its binary file formats
  the test patterns, clips and penalty of the end-to-end tests; the conditions under which they show anything are asserted in tests/test_cpu_grammar.py.
Test infrastructure only.  A grammar here is a dict(next=uint16 [n][256], accept=uint8 [n], penalty=float)."""
import os
import re
import struct
import subprocess

import numpy as np

import decode_rules_lib as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD = 0xFFFF
MAX_STATES = 4096
IGNORE_CASE = 1
# what the synthetic vocabulary can spell (tools/make_synth_model.c: single printable ASCII characters, lowercase words with and without a leading space)
TEST_PATTERNS = dict(digits=r"[0-9]{2,5}", yesno=r" ?(yes|no|maybe)", words=r"( [a-z]{3,8}){1,3}")
TEST_SEEDS = (0, 3, 5)
N_SAMPLES = 160000
# above the largest max - min spread of the logits on the test clips (asserted on the oracle in test_cpu_grammar.py), so a token that does not fit can never win over one that
# does, in either precision: the f16_mfma logits differ from the exact ones by a tiny fraction of that
TEST_PENALTY = 4096.0


# ---- the driver
def build_driver(tmp_path, sanitize):
    exe = tmp_path / ("grammar_san" if sanitize else "grammar")
    if not exe.exists():
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O1"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "streamkit_amd", "csrc"), "-o", str(exe),
                               os.path.join(ROOT, "tests", "cpp", "grammar_main.cpp")])
    return exe


def _run(args):
    out = subprocess.run([str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr.decode(errors="replace")[-2000:])
    return out


def run_compile(exe, tmp_path, cases):
    """cases: [(pattern bytes, flags, [byte strings])] -> [dict(rc, err) or dict(rc=0, next, accept, accepted=bool array)]"""
    fin, fout = tmp_path / "compile_in.bin", tmp_path / "compile_out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for pat, flags, strings in cases:
            f.write(struct.pack("<ii", flags, len(pat))); f.write(pat); f.write(struct.pack("<i", len(strings)))
            for s in strings:
                f.write(struct.pack("<i", len(s))); f.write(s)
    _run([exe, "compile", fin, fout])
    buf = open(fout, "rb").read()
    pos, res = 0, []
    for pat, flags, strings in cases:
        rc, = struct.unpack_from("<i", buf, pos); pos += 4
        if rc != 0:
            n, = struct.unpack_from("<i", buf, pos); pos += 4
            res.append(dict(rc=rc, err=buf[pos:pos + n].decode(errors="replace"))); pos += n
            continue
        n, = struct.unpack_from("<i", buf, pos); pos += 4
        nxt = np.frombuffer(buf, np.uint16, n * 256, pos).reshape(n, 256).copy(); pos += n * 512
        acc = np.frombuffer(buf, np.uint8, n, pos).copy(); pos += n
        ok = np.frombuffer(buf, np.uint8, len(strings), pos).astype(bool); pos += len(strings)
        res.append(dict(rc=0, next=nxt, accept=acc, accepted=ok))
    assert pos == len(buf)
    return res


def _gram_bytes(g):
    return struct.pack("<if", g["accept"].size, g["penalty"]) + np.ascontiguousarray(g["next"], np.uint16).tobytes() + np.ascontiguousarray(g["accept"], np.uint8).tobytes()


def run_eval(exe, tmp_path, voc, eot, n_vocab, grams, rows):
    """rows: [(grammar index, hist, x f32 [n_vocab])] -> [(state, x after)] from the header's evaluator"""
    off, data = voc
    fin, fout = tmp_path / "eval_in.bin", tmp_path / "eval_out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", off.size - 1)); f.write(off.astype(np.int32).tobytes()); f.write(data.tobytes())
        f.write(struct.pack("<iii", eot, n_vocab, len(grams)))
        for g in grams:
            f.write(_gram_bytes(g))
        f.write(struct.pack("<i", len(rows)))
        for gi, hist, x in rows:
            f.write(struct.pack("<ii", gi, len(hist))); f.write(np.asarray(hist, np.int32).tobytes()); f.write(np.ascontiguousarray(x, np.float32).tobytes())
    _run([exe, "eval", fin, fout])
    buf = open(fout, "rb").read()
    assert len(buf) == len(rows) * (4 + 4 * n_vocab)
    out = []
    for k in range(len(rows)):
        p = k * (4 + 4 * n_vocab)
        out.append((int(np.frombuffer(buf, np.uint32, 1, p)[0]), np.frombuffer(buf, np.float32, n_vocab, p + 4).copy()))
    return out


def run_check(exe, tmp_path, g):
    """-> None when skw_grammar_check accepts the record, else its message"""
    fin = tmp_path / "check_in.bin"
    with open(fin, "wb") as f:
        f.write(_gram_bytes(g))
    out = subprocess.run([str(exe), "check", str(fin)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode in (0, 3), out.stderr.decode(errors="replace")[-2000:]
    return None if out.returncode == 0 else out.stdout.decode().strip()


# ---- the vocabulary image and the restatement
def vocab_image(token_bytes, eot):
    """-> (off int32 [eot + 1], bytes uint8) of the text tokens"""
    texts = [bytes(token_bytes(t)) for t in range(eot)]
    off = np.zeros(eot + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in texts])
    return off, np.frombuffer(b"".join(texts), np.uint8).copy()


def walk(g, data, s=0):
    for b in bytes(data):
        if s == DEAD:
            return DEAD
        s = int(g["next"][s, b])
    return s


def state_after(g, voc, eot, hist):
    off, data = voc
    s = 0
    for t in hist:
        if 0 <= t < eot and s != DEAD:
            s = walk(g, data[off[t]:off[t + 1]].tobytes(), s)
    return s


def fits_mask(g, voc, eot, s):
    """bool [eot]: the text tokens that fit from state s — all tokens advance together, one byte position per round"""
    off, data = voc
    ln = (off[1:eot + 1] - off[:eot]).astype(np.int64)
    st = np.full(eot, s, np.int64)
    nxt = g["next"].astype(np.int64)
    for pos in range(int(ln.max()) if eot else 0):
        idx = np.nonzero((ln > pos) & (st != DEAD))[0]
        if idx.size == 0:
            break
        st[idx] = nxt[st[idx], data[off[idx] + pos]]
    return (ln > 0) & (st != DEAD)


def apply(g, voc, eot, hist, x):
    """-> (state, the row the sampler sees): include/skw_grammar.h steps 1 - 4"""
    x = np.array(x, dtype=np.float32, copy=True)
    if g is None:
        return 0, x
    s = state_after(g, voc, eot, hist)
    if s == DEAD:
        return s, x
    pen = np.float32(g["penalty"])
    bad = ~fits_mask(g, voc, eot, s)
    with np.errstate(invalid="ignore", over="ignore"):
        x[:eot][bad] = x[:eot][bad] - pen
        if not g["accept"][s]:
            x[eot] = x[eot] - pen
    return s, x


def compile_py(pattern, ignore_case=False, penalty=100.0):
    """through the engine library's skw_grammar_compile (needs no device) -> a grammar dict"""
    from streamkit_amd import engine
    g = engine.Grammar.compile(pattern, ignore_case=ignore_case, penalty=penalty)
    return dict(next=g.next, accept=g.accept, penalty=float(penalty))


def to_engine(g):
    from streamkit_amd import engine
    return None if g is None else engine.Grammar.from_tables(g["next"], g["accept"], g["penalty"])


def chain_table(n, penalty=100.0, byte=ord("a")):
    """a hand-made table of n states: state k goes to k + 1 on `byte`, the last state loops on it and accepts — a^(n-1) a*.  n = 4096 is the largest table there is"""
    nxt = np.full((n, 256), DEAD, np.uint16)
    for k in range(n):
        nxt[k, byte] = min(k + 1, n - 1)
    acc = np.zeros(n, np.uint8); acc[n - 1] = 1
    return dict(next=nxt, accept=acc, penalty=penalty)


def letters_table(n, penalty=100.0):
    """n states over lowercase letters and the space: the state counts bytes (mod n - 1 after the first), every state but 0 accepts.  Every word of the synthetic
    vocabulary fits from every state, punctuation and digits never do — a table of any size whose walk visits many of its rows"""
    nxt = np.full((n, 256), DEAD, np.uint16)
    for k in range(n):
        to = 0 if n == 1 else (k % (n - 1)) + 1
        for b in list(range(ord("a"), ord("z") + 1)) + [ord(" ")]:
            nxt[k, b] = to
    acc = np.ones(n, np.uint8)
    if n > 1:
        acc[0] = 0
    return dict(next=nxt, accept=acc, penalty=penalty)


def transcript_bytes(token_bytes, ids, eot):
    return b"".join(bytes(token_bytes(t)) for t in ids if 0 <= t < eot)


def full_with_grammar(om, pcm, gram, voc, context=(), params=None, rules=None, stats=None):
    """dr.full_with_rules with the grammar's stage behind the rules' transform: the same loop, the row K11 sees is apply(transform(raw)).  stats (a dict): 'spread' becomes
    the largest max - min over the finite logits of any raw row seen."""
    inner = dr.transform

    def composed(hist, raw, r, eot):
        x = inner(hist, raw, r, eot)
        if stats is not None:
            fin = np.asarray(raw)[np.isfinite(raw)]
            stats["spread"] = max(stats.get("spread", 0.0), float(fin.max() - fin.min()))
        return apply(gram, voc, eot, hist, x)[1]

    dr.transform = composed
    try:
        return dr.full_with_rules(om, pcm, context, params, rules)
    finally:
        dr.transform = inner


def py_flags(flags):
    return re.IGNORECASE if flags & IGNORE_CASE else 0
