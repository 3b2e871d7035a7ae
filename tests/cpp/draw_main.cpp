// draw_main.cpp — include/skw_draw.h's serial walks as a program of its own (tests/test_cpu_sampler_draw.py), staged exactly as block_discrete_draw
// (streamkit_amd/csrc/skw_kernels_sample.hip) stages a row: SKW_DRAW_CHUNK doubles per chunk, one bmax per SKW_DRAW_BLOCK elements, q = p / sum for the whole row between the chains.
// stdin: int32 words — the record count, then per record: n, the two words of u (a double's bit pattern, low word first), then n f32 bit patterns (the weights).
// stdout, one line per record: index, the bits of sum (hex), blocks the first chain skipped, blocks of the row, blocks the second chain skipped, blocks the second
// chain reached (up to and including the hit's) — then the plain sequential definition (oracle/skw_oracle.c discrete_draw, libstdc++'s): index, bits of sum.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "skw_draw.h"

static std::vector<int32_t> g_in;
static size_t g_pos = 0;
static int32_t rd() { if (g_pos >= g_in.size()) { fprintf(stderr, "input ends inside a record\n"); exit(2); } return g_in[g_pos++]; }
static unsigned long long bits(double x) { unsigned long long b; memcpy(&b, &x, 8); return b; }

static void stage(const double* src, int m, double* ch, double* bmax) {
    for (int i = 0; i < m; ++i) ch[i] = src[i];
    for (int t = 0; t < SKW_DRAW_CHUNK / SKW_DRAW_BLOCK; ++t) {
        double mx = 0.0; for (int i = t * SKW_DRAW_BLOCK; i < t * SKW_DRAW_BLOCK + SKW_DRAW_BLOCK && i < m; ++i) mx = ch[i] > mx ? ch[i] : mx;
        bmax[t] = mx;
    }
}

int main() {
    { int32_t buf[16384]; size_t n; while ((n = fread(buf, 4, 16384, stdin)) > 0) g_in.insert(g_in.end(), buf, buf + n); }
    const int n_rec = rd();
    alignas(16) static double ch[SKW_DRAW_CHUNK]; static double bmax[SKW_DRAW_CHUNK / SKW_DRAW_BLOCK];
    for (int rec = 0; rec < n_rec; ++rec) {
        const int n = rd();
        if (n < 1 || n > (1 << 20)) { fprintf(stderr, "bad record\n"); return 2; }
        double u; { const uint32_t lo = (uint32_t)rd(), hi = (uint32_t)rd(); const unsigned long long b = ((unsigned long long)hi << 32) | lo; memcpy(&u, &b, 8); }
        std::vector<float> p(n); for (auto& x : p) { const int32_t w = rd(); memcpy(&x, &w, 4); }
        std::vector<double> d(n), q(n);
        for (int i = 0; i < n; ++i) d[i] = (double)p[i];
        // the kernel's way
        double sum = 0.0; int skip1 = 0, skip2 = 0;
        for (int c0 = 0; c0 < n; c0 += SKW_DRAW_CHUNK) {
            const int m = n - c0 < SKW_DRAW_CHUNK ? n - c0 : SKW_DRAW_CHUNK;
            stage(d.data() + c0, m, ch, bmax);
            sum = skw_draw_sum_chunk(ch, bmax, m, sum, &skip1);
        }
        for (int i = 0; i < n; ++i) q[i] = (double)p[i] / sum;
        double cp = 0.0; int hit = -1;
        for (int c0 = 0; c0 < n && hit < 0; c0 += SKW_DRAW_CHUNK) {
            const int m = n - c0 < SKW_DRAW_CHUNK ? n - c0 : SKW_DRAW_CHUNK;
            stage(q.data() + c0, m, ch, bmax);
            hit = skw_draw_cp_chunk(ch, bmax, m, c0, n, u, &cp, &skip2);
        }
        if (hit < 0) hit = n - 1;
        // the definition
        double rsum = 0.0; for (int i = 0; i < n; ++i) rsum += (double)p[i];
        int ref = n - 1; { double c = 0.0; for (int i = 0; i < n; ++i) { c += (double)p[i] / rsum; if (i == n - 1) c = 1.0; if (!(c < u)) { ref = i; break; } } }
        printf("%d %016llx %d %d %d %d %d %016llx\n", hit, bits(sum), skip1, (n + SKW_DRAW_BLOCK - 1) / SKW_DRAW_BLOCK, skip2, hit / SKW_DRAW_BLOCK + 1, ref, bits(rsum));
    }
    return 0;
}
