// Stand-alone driver of the grammar contract for tests/test_cpu_grammar.py: the pattern compiler (streamkit_amd/csrc/skw_grammar_compile.h) and the header's CPU evaluator
// (include/skw_grammar.h), with no engine and no device behind them.  Built twice by the test: plain, and with -fsanitize=address,undefined.
//   grammar_main compile IN OUT    IN : i32 n_cases, then per case: i32 flags, i32 len, pattern bytes, i32 n_strings, then per string: i32 len, bytes
//                                  OUT: per case: i32 rc; rc != 0: i32 len + the message; rc == 0: i32 n_states, next u16 [n_states][256], accept u8 [n_states],
//                                       then one byte per string: 1 = the DFA accepts it
//   grammar_main eval IN OUT       IN : i32 n_text, off i32 [n_text + 1], bytes; i32 tok_eot, i32 n_vocab; i32 n_grammars, per grammar: i32 n_states, f32 penalty, next, accept;
//                                       i32 n_rows, per row: i32 grammar index, i32 n_hist, hist i32 [n_hist], x f32 [n_vocab]
//                                  OUT: per row: u32 the state of step 1, x f32 [n_vocab] after skw_grammar_apply_ref
//   grammar_main check IN          IN : one grammar as above (i32 n_states, f32 penalty, next, accept); prints the message of skw_grammar_check, exit 0 = accepted, 3 = refused
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "skw_grammar_compile.h"

static std::vector<char> slurp(const char* path) {
    std::vector<char> b; FILE* f = fopen(path, "rb"); if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    char buf[1 << 16]; size_t n; while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f); return b;
}
struct Reader {
    const std::vector<char>& b; size_t i = 0;
    explicit Reader(const std::vector<char>& v) : b(v) {}
    void need(size_t n) { if (i + n > b.size()) { fprintf(stderr, "input truncated at %zu\n", i); exit(2); } }
    int32_t i32() { need(4); int32_t v; memcpy(&v, &b[i], 4); i += 4; return v; }
    float f32() { need(4); float v; memcpy(&v, &b[i], 4); i += 4; return v; }
    template <typename T> std::vector<T> arr(size_t n) { need(n * sizeof(T)); std::vector<T> v(n); if (n) memcpy(v.data(), &b[i], n * sizeof(T)); i += n * sizeof(T); return v; }
};
static void w(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); } }
static void w32(FILE* f, int32_t v) { w(f, &v, 4); }

struct Gram { std::vector<uint16_t> next; std::vector<uint8_t> accept; skw_grammar g; };
static void read_gram(Reader& r, Gram& G) {
    const int32_t ns = r.i32(); const float pen = r.f32(); const size_t n = ns > 0 && ns <= 2 * SKW_GRAMMAR_MAX_STATES ? (size_t)ns : 0;
    G.next = r.arr<uint16_t>(n * 256); G.accept = r.arr<uint8_t>(n);
    G.g.n_states = ns; G.g.next = G.next.data(); G.g.accept = G.accept.data(); G.g.penalty = pen;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: grammar_main compile|eval IN OUT | check IN\n"); return 2; }
    const std::string mode = argv[1];
    const std::vector<char> in = slurp(argv[2]); Reader r(in);
    if (mode == "check") {
        Gram G; read_gram(r, G); char err[256] = {0};
        if (!skw_grammar_check(&G.g, "clip 7", err, sizeof err)) { printf("%s\n", err); return 3; }
        return 0;
    }
    if (argc < 4) return 2;
    FILE* out = fopen(argv[3], "wb"); if (!out) return 2;
    if (mode == "compile") {
        const int n_cases = r.i32();
        for (int c = 0; c < n_cases; ++c) {
            const int flags = r.i32(); const int len = r.i32(); const std::vector<char> pat = r.arr<char>(len);
            const int n_str = r.i32();
            skw_grammar* g = nullptr; char err[256] = {0};
            const int rc = skw_grammar_compile_impl(pat.data(), pat.size(), flags, 100.0f, &g, err, sizeof err);
            w32(out, rc);
            if (rc != 0) { const int el = (int)strlen(err); w32(out, el); w(out, err, el); if (g) return 4; }
            else {
                if (!skw_grammar_check(g, "case", err, sizeof err)) { fprintf(stderr, "case %d: the compiler's own table is refused: %s\n", c, err); return 4; }
                w32(out, g->n_states); w(out, g->next, (size_t)g->n_states * 256 * 2); w(out, g->accept, g->n_states);
            }
            std::vector<uint8_t> res(n_str, 0);
            for (int k = 0; k < n_str; ++k) {
                const int sl = r.i32(); const std::vector<uint8_t> s = r.arr<uint8_t>(sl);
                if (rc == 0) { const uint32_t st = skw_grammar_walk(g->next, 0, s.data(), sl); res[k] = st != SKW_GRAMMAR_DEAD && g->accept[st]; }
            }
            if (rc == 0) w(out, res.data(), res.size());
            skw_grammar_free_impl(g);
        }
    } else if (mode == "eval") {
        const int n_text = r.i32(); const std::vector<int32_t> off = r.arr<int32_t>((size_t)n_text + 1);
        const std::vector<uint8_t> bytes = r.arr<uint8_t>(off[n_text]);
        const skw_grammar_vocab voc{n_text, off.data(), bytes.data()};
        const int tok_eot = r.i32(), n_vocab = r.i32();
        if (tok_eot > n_text || tok_eot >= n_vocab) return 2;
        const int ng = r.i32(); std::vector<Gram> gs(ng);
        for (int k = 0; k < ng; ++k) { read_gram(r, gs[k]); char err[256]; if (!skw_grammar_check(&gs[k].g, "grammar", err, sizeof err)) { fprintf(stderr, "%s\n", err); return 4; } }
        const int n_rows = r.i32();
        for (int k = 0; k < n_rows; ++k) {
            const int gi = r.i32(), nh = r.i32(); const std::vector<int32_t> hist = r.arr<int32_t>(nh); std::vector<float> x = r.arr<float>(n_vocab);
            if (gi < 0 || gi >= ng) return 2;
            const uint32_t s = skw_grammar_apply_ref(&gs[gi].g, &voc, tok_eot, hist.data(), nh, x.data());
            w(out, &s, 4); w(out, x.data(), sizeof(float) * x.size());
        }
    } else return 2;
    fclose(out);
    return 0;
}
