// Stand-alone driver for streamkit_amd/csrc/skw_tokenizer.h (tests/test_cpu_context.py compiles it against the header alone; host code, no device).
//   tokenize_main VOCAB CASES
// VOCAB: int32 n_text, int32 n, then n x (uint32 len, bytes) — the strings of ids 0 .. n-1, of which ids below n_text take part.
// CASES: int32 count, then count x (int32 cap, uint32 len, bytes).  One output line per case: the return value, then the ids written.
#include "skw_tokenizer.h"
#include <cstdio>
#include <cstdlib>

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s VOCAB CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t n_text = 0, n = 0;
    if (!rd(f, &n_text, 4) || !rd(f, &n, 4) || n < 0 || n > (1 << 20)) { fprintf(stderr, "bad vocabulary header\n"); return 2; }
    std::vector<std::string> tok((size_t)n);
    for (int i = 0; i < n; ++i) {
        uint32_t len = 0;
        if (!rd(f, &len, 4) || len > 4096) { fprintf(stderr, "bad vocabulary entry %d\n", i); return 2; }
        tok[i].resize(len);
        if (len && !rd(f, &tok[i][0], len)) { fprintf(stderr, "short vocabulary entry %d\n", i); return 2; }
    }
    fclose(f);
    SkwTokenizer tz; tz.build(tok, n_text);
    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    int32_t count = 0;
    if (!rd(f, &count, 4) || count < 0 || count > 4096) { fprintf(stderr, "bad case header\n"); return 2; }
    for (int c = 0; c < count; ++c) {
        int32_t cap = 0; uint32_t len = 0;
        if (!rd(f, &cap, 4) || !rd(f, &len, 4) || cap < 0 || cap > (1 << 20) || len > (1 << 20)) { fprintf(stderr, "bad case %d\n", c); return 2; }
        std::string text(len, '\0');
        if (len && !rd(f, &text[0], len)) { fprintf(stderr, "short case %d\n", c); return 2; }
        std::vector<int32_t> ids((size_t)cap);      // exactly cap words: a write past it is the sanitizer's to catch
        const int r = tz.tokenize_into(text.c_str(), ids.data(), cap);
        printf("%d", r);
        for (int i = 0; i < r; ++i) printf(" %d", ids[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
