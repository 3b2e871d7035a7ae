// Stand-alone driver for streamkit_amd/csrc/skw_window_rules.h (tests/test_cpu_window_rules.py compiles it against the header alone; host code, no device).
//   window_rules_main CASES
// CASES: int32 count, then count records of int32 words (floats travel as their bits): kind, then what the kind takes (below).  One output line per record.
#include "skw_window_rules.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static FILE* g_f;
static int32_t rd() { int32_t v = 0; if (fread(&v, 4, 1, g_f) != 1) { fprintf(stderr, "short case file\n"); exit(2); } return v; }
static float rdf() { const int32_t v = rd(); float f; memcpy(&f, &v, 4); return f; }
static std::vector<int> rdv(int cap) {
    const int n = rd(); if (n < 0 || n > cap) { fprintf(stderr, "bad count %d\n", n); exit(2); }
    std::vector<int> v((size_t)n); for (int& x : v) x = rd(); return v;
}
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

// kind 0: tok_beg tok_eot n_max max_tokens no_timestamps single_segment seek seek_end ids[] — one window's sampled ids through the token loop, then the output step
//   -> failed consumed kept advance n_seg, then per segment: t0 t1 n ids
static void window_case() {
    const int tok_beg = rd(), tok_eot = rd(), n_max = rd(), max_tokens = rd(), no_timestamps = rd(), single_segment = rd(), seek = rd(), seek_end = rd();
    const std::vector<int> ids = rdv(1 << 16);
    static std::vector<std::string> text; if ((int)text.size() < tok_eot) text.assign((size_t)tok_eot, "x");      // the cut only asks whether text is empty
    SkwSeqState st; memset(&st, 0, sizeof st); st.seek_delta = SKW_WINDOW_FRAMES; st.seek = seek; st.seek_end = seek_end;
    std::vector<SkwTokenOut> tk; const int n = (int)ids.size(); int i = 0;
    for (; i < n && i < n_max; ++i) {
        SkwTokenOut t; memset(&t, 0, sizeof t); t.id = ids[i]; t.tid = ids[i] >= tok_beg ? ids[i] : (i > 0 ? tk[i - 1].tid : tok_beg);
        tk.push_back(t);
        skw_token_loop_update(st, t.id, i, tok_beg, tok_eot, max_tokens, no_timestamps, single_segment, n_max);
        if (st.failed || st.completed) { ++i; break; }
    }
    if (st.failed) { printf("1 %d 0 0 0\n", i); return; }
    tk.resize((size_t)st.result_len);      // exactly the kept tokens: a read past them is the sanitizer's to catch
    SeqAcc A;
    const int advance = skw_window_output(tk.data(), st.result_len, seek, st.seek_delta, seek_end, tok_beg, tok_eot, single_segment, false, text.data(), A);
    printf("0 %d %d %d %d", i, st.result_len, advance, (int)A.seg.size());
    for (const SkwSegment& s : A.seg) { printf(" %lld %lld %d", (long long)s.t0, (long long)s.t1, s.tok_end - s.tok_begin); for (int k = s.tok_begin; k < s.tok_end; ++k) printf(" %d", A.tok[k].id); }
    printf("\n");
}
// kind 1: temperature temperature_inc -> n, then the entries' bits
static void ladder_case() {
    const float t = rdf(), inc = rdf(); const std::vector<float> tl = skw_temperature_ladder(t, inc);
    printf("%d", (int)tl.size()); for (float v : tl) printf(" %u", bits(v)); printf("\n");
}
// kind 2: past[] t tail[] n_text_ctx n_max tok_prev -> n take ids
static void prompt_case() {
    const std::vector<int> past = rdv(1 << 16); const float t = rdf(); const std::vector<int> tail = rdv(8);
    const int n_text_ctx = rd(), n_max = rd(), tok_prev = rd();
    std::vector<int> out(SKW_PROMPT_CAP, -1); int take = -1;
    const int n = skw_row_prompt(past, t, tail.data(), (int)tail.size(), n_text_ctx, n_max, tok_prev, out.data(), &take);
    printf("%d %d", n, take); for (int i = 0; i < n; ++i) printf(" %d", out[i]); printf("\n");
}
// kind 3: failed n_tokens result_len no_speech_prob entropy_thold logprob_thold no_speech_thold n, then n x (id, plog) -> failed fallback no_speech n_tok
static void verdict_case() {
    SkwSeqState s; memset(&s, 0, sizeof s); s.failed = rd(); s.n_tokens = rd(); s.result_len = rd(); s.no_speech_prob = rdf();
    const float et = rdf(), lt = rdf(), nt = rdf(); const int n = rd();
    std::vector<SkwTokenOut> tk((size_t)n); for (SkwTokenOut& t : tk) { memset(&t, 0, sizeof t); t.id = rd(); t.plog = rdf(); }
    const SkwVerdict v = skw_pass_verdict(s, tk.data(), et, lt, nt);
    printf("%d %d %d %d\n", (int)v.failed, (int)v.fallback, (int)v.no_speech, v.n_tok);
}
// kind 4: past[] take no_speech kept[] n_cap -> prompt_past after the update (n ids), then the context written back (n ids)
static void past_case() {
    std::vector<int> past = rdv(1 << 16); const int take = rd(), no_speech = rd(); const std::vector<int> kept = rdv(1 << 16); const int n_cap = rd();
    std::vector<SkwTokenOut> tk(kept.size()); for (size_t i = 0; i < kept.size(); ++i) { memset(&tk[i], 0, sizeof tk[i]); tk[i].id = kept[i]; }
    skw_prompt_past_update(past, take, tk.data(), (int)tk.size(), no_speech != 0);
    std::vector<int32_t> cx((size_t)n_cap + 1, -7);
    skw_context_write(past, n_cap, cx.data());
    printf("%d", (int)past.size()); for (int v : past) printf(" %d", v);
    printf(" %d", cx[0]); for (int i = 0; i < cx[0]; ++i) printf(" %d", cx[1 + i]); printf("\n");
}
// kind 5: n_cap n_vocab clip words[] (the context as handed in: words[0] = n) -> 1, or 0 and the message
static void check_case() {
    const int n_cap = rd(), n_vocab = rd(), clip = rd(); const std::vector<int> cx = rdv(1 << 16);
    char err[512]; err[0] = 0;
    if (skw_context_check(cx.data(), n_cap, n_vocab, clip, err, sizeof err)) printf("1\n"); else printf("0 %s\n", err);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    g_f = fopen(argv[1], "rb");
    if (!g_f) { perror(argv[1]); return 2; }
    const int count = rd();
    for (int c = 0; c < count; ++c) {
        const int kind = rd();
        if (kind == 0) window_case(); else if (kind == 1) ladder_case(); else if (kind == 2) prompt_case(); else if (kind == 3) verdict_case();
        else if (kind == 4) past_case(); else if (kind == 5) check_case(); else { fprintf(stderr, "bad kind %d in record %d\n", kind, c); return 2; }
    }
    fclose(g_f);
    return 0;
}
