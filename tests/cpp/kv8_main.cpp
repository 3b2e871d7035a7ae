// kv8_main.cpp — include/skw_kv8.h's sequential evaluator as a program of its own (tests/test_cpu_kv8_cases.py; plain and under the host sanitizers).
// stdin: int32 words — the record count, then per record: H, n_ctx, count, n_q, then n_q x H*64 query halves, n_ctx x H*64 K halves, n_ctx x H*64 V halves (one f16 bit pattern
// per word, natural order; rows at or past `count` may hold anything).  stdout per record: the word count, then the image of slot 1 of a two-slot buffer UNPACKED through the
// header's offset functions — K qs [T][H*64], K scales [T][2 H], V qs [T][H*64], V scales [T / 32][H*64] for the T = 32 ceil(count / 32) keys of the written blocks — then the
// contract's scores [n_q][H][count] as f32 bit patterns, then one word: the number of image bytes outside slot 1's written records that changed (must be 0).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "skw_kv8.h"

static std::vector<int32_t> g_in;
static size_t g_pos = 0;
static int32_t rd() { if (g_pos >= g_in.size()) { fprintf(stderr, "input ends inside a record\n"); exit(2); } return g_in[g_pos++]; }
static void emit(const std::vector<int32_t>& o) { const int32_t n = (int32_t)o.size(); fwrite(&n, 4, 1, stdout); if (n) fwrite(o.data(), 4, o.size(), stdout); }

int main() {
    { int32_t buf[16384]; size_t n; while ((n = fread(buf, 4, 16384, stdin)) > 0) g_in.insert(g_in.end(), buf, buf + n); }
    const int n_rec = rd();
    for (int rec = 0; rec < n_rec; ++rec) {
        const int H = rd(), n_ctx = rd(), count = rd(), n_q = rd();
        if (H < 1 || H > 32 || n_ctx < 1 || n_ctx > 4096 || count < 1 || count > n_ctx || n_q < 0 || n_q > 64) { fprintf(stderr, "bad record\n"); return 2; }
        const int d = H * 64, Tpad = (n_ctx + 31) & ~31, T = (count + 31) & ~31, slot = 1;
        std::vector<uint16_t> q((size_t)n_q * d), K((size_t)n_ctx * d), V((size_t)n_ctx * d);
        for (auto& x : q) x = (uint16_t)rd();
        for (auto& x : K) x = (uint16_t)rd();
        for (auto& x : V) x = (uint16_t)rd();
        const size_t sb = (size_t)skw_kv8_slot_bytes(H, Tpad);
        std::vector<uint8_t> img(2 * sb, 0xEE), seen(2 * sb, 0);
        skw_kv8_quantize_ref(K.data(), V.data(), H, n_ctx, Tpad, slot, count, img.data());
        std::vector<int32_t> o;
        auto at = [&](long off) { seen[(size_t)off] = 1; return img[(size_t)off]; };
        auto at16 = [&](long off) { return (int32_t)(at(off) | (at(off + 1) << 8)); };
        for (int k = 0; k < T; ++k) for (int f = 0; f < d; ++f) o.push_back((int8_t)at(skw_kv8_kq_off(slot, H, Tpad, k, f)));
        for (int k = 0; k < T; ++k) for (int b = 0; b < 2 * H; ++b) o.push_back(at16(skw_kv8_kd_off(slot, H, Tpad, k, 32 * b)));
        for (int k = 0; k < T; ++k) for (int f = 0; f < d; ++f) o.push_back((int8_t)at(skw_kv8_vq_off(slot, H, Tpad, f, k)));
        for (int j = 0; j < T / 32; ++j) for (int f = 0; f < d; ++f) o.push_back(at16(skw_kv8_vd_off(slot, H, Tpad, f, 32 * j)));
        std::vector<float> s((size_t)count);
        for (int r = 0; r < n_q; ++r) for (int h = 0; h < H; ++h) {
            skw_kv8_scores_ref(q.data() + (size_t)r * d + h * 64, img.data(), H, Tpad, slot, h, count, s.data());
            for (int k = 0; k < count; ++k) o.push_back((int32_t)skw_f32_bits(s[k]));
        }
        // the offset functions are a bijection onto the written records: every byte they name was written, every other byte of the buffer is untouched
        int32_t stray = 0;
        for (size_t i = 0; i < img.size(); ++i) stray += seen[i] ? 0 : (img[i] != 0xEE);
        for (int h = 0; h < H; ++h) for (int j = 0; j < T / 32; ++j) for (int b = 0; b < SKW_KV8_REC; ++b) stray += !seen[(size_t)skw_kv8_rec_off(slot, H, Tpad, h, j) + b];
        o.push_back(stray);
        emit(o);
    }
    return 0;
}
