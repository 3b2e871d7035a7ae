// Stand-alone driver over include/skw_align.h (the word-timestamp contract's evaluator) and streamkit_amd/csrc/skw_words.h (the word rule): no GPU, no engine library.
// stdin: little-endian int32 words — the record count, then per record its kind and fields; floats travel as their bit patterns.  stdout: per record the count of
// output words, then the words.  tests/test_cpu_align.py compiles it plain and with -fsanitize=address,undefined.
//   0 dtw      N Kw seek_cs x[N*Kw]                         -> n_path path_i[n_path] path_j[n_path] jump[N] t0[N] t1[N]
//   1 reduce   H split N K Kw width P[H][N][K]              -> x[N*Kw]      (heads [0, split) and [split, H) accumulated by two calls, as two layers would)
//   2 words    n t_eot { t0 len bytes[len] } x n            -> n_words { tok_begin tok_end start end len bytes[len] }      (one window: t1 = the next token's t0, the last one's t_eot)
//   3 params   n_layer n_head clip enabled width mask[32]   -> ok len message[len]
//   4 weights  rows n_keys q[rows*64] K[n_keys*64]          -> P[rows*n_keys]      (f16 bit patterns, one per word)
//   5 kw       n_len_org seek n_keys                        -> Kw
//   6 top      n_layer n_head n_layers                      -> mask[32] n_heads
//   7 median   N Kw width z[N*Kw]                           -> filtered[N*Kw]      (step 4 alone)
//   8 words2   n { t0 t1 first len bytes[len] } x n         -> as 2      (the node's call: every token with its own t1 and `first`)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "skw_align.h"
#include "skw_words.h"

static std::vector<int32_t> g_in;
static size_t g_pos = 0;
static int32_t rd() { if (g_pos >= g_in.size()) { fprintf(stderr, "input ends inside a record\n"); exit(2); } return g_in[g_pos++]; }
static float rdf() { return skw_bits_f32((uint32_t)rd()); }
static void emit(const std::vector<int32_t>& o) { const int32_t n = (int32_t)o.size(); fwrite(&n, 4, 1, stdout); if (n) fwrite(o.data(), 4, o.size(), stdout); }

int main() {
    { int32_t buf[16384]; size_t n; while ((n = fread(buf, 4, 16384, stdin)) > 0) g_in.insert(g_in.end(), buf, buf + n); }
    const int n_rec = rd();
    for (int rec = 0; rec < n_rec; ++rec) {
        const int kind = rd();
        std::vector<int32_t> o;
        if (kind == 0) {
            const int N = rd(), Kw = rd(), seek_cs = rd();
            std::vector<float> x((size_t)N * Kw); for (float& v : x) v = rdf();
            std::vector<int32_t> pi(N + Kw), pj(N + Kw), jump(N), t0(N), t1(N); int32_t np = 0;
            if (skw_align_dtw_ref(x.data(), N, Kw, jump.data(), pi.data(), pj.data(), &np)) return 3;
            skw_align_times(jump.data(), N, seek_cs, t0.data(), t1.data());
            o.push_back(np); o.insert(o.end(), pi.begin(), pi.begin() + np); o.insert(o.end(), pj.begin(), pj.begin() + np);
            o.insert(o.end(), jump.begin(), jump.end()); o.insert(o.end(), t0.begin(), t0.end()); o.insert(o.end(), t1.begin(), t1.end());
        } else if (kind == 1) {
            const int H = rd(), split = rd(), N = rd(), K = rd(), Kw = rd(), width = rd();
            std::vector<float> P((size_t)H * N * K); for (float& v : P) v = rdf();
            std::vector<double> acc((size_t)N * Kw, 0.0); std::vector<float> x((size_t)N * Kw);
            if (skw_align_reduce_ref(P.data(), (long)N * K, K, split, N, Kw, width, acc.data())) return 3;
            if (skw_align_reduce_ref(P.data() + (size_t)split * N * K, (long)N * K, K, H - split, N, Kw, width, acc.data())) return 3;
            skw_align_finish_ref(acc.data(), H, (long)N * Kw, x.data());
            for (float v : x) o.push_back((int32_t)skw_f32_bits(v));
        } else if (kind == 2 || kind == 8) {
            const int n = rd(), t_eot = kind == 2 ? rd() : 0;
            std::vector<std::string> text(n); std::vector<SkwWordTok> toks(n);
            for (int i = 0; i < n; ++i) { toks[i].t0 = rd(); if (kind == 8) { toks[i].t1 = rd(); toks[i].first = rd() != 0; }
                                          const int len = rd(); for (int b = 0; b < len; ++b) text[i].push_back((char)rd()); }
            for (int i = 0; i < n; ++i) { toks[i].text = text[i].data(); toks[i].len = (int)text[i].size(); if (kind == 2) toks[i].first = i == 0; }
            if (kind == 2) for (int i = 0; i < n; ++i) toks[i].t1 = i + 1 < n ? toks[i + 1].t0 : t_eot;
            const std::vector<SkwWord> w = skw_words_cut(toks.data(), n);
            o.push_back((int32_t)w.size());
            for (const SkwWord& x : w) { o.push_back(x.tok_begin); o.push_back(x.tok_end); o.push_back((int32_t)x.start); o.push_back((int32_t)x.end); o.push_back((int32_t)x.text.size());
                                         for (char ch : x.text) o.push_back((unsigned char)ch); }
        } else if (kind == 3) {
            const int n_layer = rd(), n_head = rd(), clip = rd();
            skw_align_params p; p.enabled = rd(); p.median_width = rd(); for (int l = 0; l < 32; ++l) p.head_mask[l] = (uint32_t)rd();
            char err[256] = "";
            const int ok = skw_align_check_params(&p, n_layer, n_head, clip, err, sizeof(err));
            o.push_back(ok); o.push_back((int32_t)strlen(err)); for (const char* s = err; *s; ++s) o.push_back((unsigned char)*s);
        } else if (kind == 4) {
            const int rows = rd(), n_keys = rd();
            std::vector<uint16_t> q((size_t)rows * 64), K((size_t)n_keys * 64); for (uint16_t& v : q) v = (uint16_t)rd(); for (uint16_t& v : K) v = (uint16_t)rd();
            std::vector<float> P(n_keys), e(n_keys);
            for (int r = 0; r < rows; ++r) { skw_align_weights_ref(q.data() + (size_t)r * 64, K.data(), 64, n_keys, P.data(), e.data()); for (float v : P) o.push_back((int32_t)skw_f32_bits(v)); }
        } else if (kind == 5) {
            const int n_len_org = rd(), seek = rd(), n_keys = rd();
            o.push_back(skw_align_kw(n_len_org, seek, n_keys));
        } else if (kind == 6) {
            const int n_layer = rd(), n_head = rd(), n_layers = rd();
            uint32_t mask[32]; skw_align_heads_top(n_layer, n_head, n_layers, mask);
            for (int l = 0; l < 32; ++l) o.push_back((int32_t)mask[l]);
            o.push_back(skw_align_n_heads(mask));
        } else if (kind == 7) {
            const int N = rd(), Kw = rd(), width = rd();
            std::vector<float> z((size_t)N * Kw); for (float& v : z) v = rdf();
            for (int r = 0; r < N; ++r) for (int k = 0; k < Kw; ++k) o.push_back((int32_t)skw_f32_bits(skw_align_median_at(z.data() + (size_t)r * Kw, Kw, k, width)));
        } else { fprintf(stderr, "record %d: unknown kind %d\n", rec, kind); return 2; }
        emit(o);
    }
    return 0;
}
