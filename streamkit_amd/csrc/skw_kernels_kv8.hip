// skw_kernels_kv8.hip — the decode step's cross attention over 8-bit cross K / V (cross_kv = q8_0; f16_mfma precision).  Contract, storage format and the image's byte order:
// include/skw_kv8.h.  The cross K / V of a window is written once and read by every decode step; as ggml q8_0 blocks a (row, head) streams 4.25 KiB per 32 keys where the f16
// images stream 8 KiB.
//
//   k_kv8_quantize           a layer's f16 fragment-order cross K / V^T images (skw_kfrag_off / skw_vtfrag_off) -> the q8 image (skw_kv8_*_off), all slots of the encode call in
//                            one launch; a slot's key count comes from device memory (slot_k; null: n_ctx) and decides what is a pad — never the value
//   k_dec_cross_attn_kv8     k_dec_cross_attn16's one streaming pass (skw_kernels_dec.hip) over the q8 image: four waves per (row, head) taking every fourth 32-key block, RD records
//                            in flight per wave, non-temporal buffer loads, the final combine of the four (m, l, O) in LDS.  Per record:
//     scores   q quantised in the prologue (two q8_0 blocks; amax across the four lane groups by two shuffles).  S[key] = one v_mfma_i32_16x16x32_i8 per key tile and d half
//              (A = 16 keys x 32 d, 8 bytes per lane; B = the q block broadcast to every column), then the chain of skw_kv8_score on the VALU: two exact integer dots, two scale
//              products, nothing contracted.  Lane group g ends up with keys 4 e + g, the order of V^T's bytes
//     softmax  as k_dec_cross_attn16: running maximum per wave, p = exp2((s - m) log2 e) rounded to f16 unnormalised, the sum of the rounded values
//     P.V      V^T's int8 -> f16 in registers (exact): x ^ 0x80 is the byte q + 128, v_perm_b32 puts it under the exponent byte 0x64 (the f16 1024 + q + 128), one packed add of
//              -1152 leaves q — 2.5 VALU instructions per element pair; one v_mfma_f32_16x16x32_f16 per channel tile into a FRESH accumulator, then the block's f16 scale in
//              f32: o[c] = fma(dv[c], blocksum[c], o[c])
//     scales   the record's 256 B of scales arrive as one dword per lane, [lane group g][16]: the sixteen a lane group needs; a lane takes each from its row of 16 lanes with a
//              DPP row broadcast — no LDS in the loop
// RAW (tests): the same instantiation path writes its f32 scores [row][head][key] (key stride n_ctx as launched) and nothing else.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "skw_dev_common.h"

#define SKW_KV8_RD 5      // records (4.25 KiB) in flight per wave: 164 VGPRs, no scratch; 6 (the bytes k_dec_cross_attn16 keeps in flight) spills at 12 waves per CU
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// One workgroup of 128 threads per (slot, head, 32-key block): threads 0 .. 63 the K blocks (key kl = t >> 1, d half t & 1), 64 .. 127 the V^T blocks (channel t - 64).
__global__ __launch_bounds__(128) void k_kv8_quantize(const half_t* kf, const half_t* vtf, uint8_t* img, int slot0, int H, int n_ctx, int Tpad, const int* slot_k) {
    const int j = blockIdx.x, slot = slot0 + blockIdx.y / H, h = blockIdx.y % H, t = threadIdx.x;
    int count = slot_k ? slot_k[slot] : n_ctx;
    if (count <= 0 || count > n_ctx) count = n_ctx;
    if (j * 32 >= count) return;                                         // wholly past the count: not written, not read
    uint8_t* rec = img + skw_kv8_rec_off(slot, H, Tpad, h, j);
    float x[32]; int8_t qs[32]; float d, s;
    if (t < 64) {
        const int kl = t >> 1, kk = t & 1, key = 32 * j + kl;
        const bool live = key < count;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            H8 p; p.u = *(const uint4*)(kf + skw_kfrag_off(slot, H, Tpad, key, h * 64 + 32 * kk + 8 * c));
#pragma unroll
            for (int e = 0; e < 8; ++e) x[8 * c + e] = live ? h2f(p.h[e]) : 0.0f;
        }
        skw_ggml_quantize_q8_block(x, qs, &d, &s);
        const int r = kl & 15, i = 4 * (r & 3) + (r >> 2);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            union { int8_t b[8]; uint2 w; } o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o.b[e] = qs[8 * g + e];
            *(uint2*)(rec + (kl >> 4) * 1024 + (i + 16 * g) * 16 + kk * 8) = o.w;
        }
        *(uint16_t*)(rec + SKW_KV8_SCALES + (16 * (kl & 3) + (kl >> 2)) * 4 + kk * 2) = skw_f32_to_f16(d);
    } else {
        const int c = t - 64, ct = c >> 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {                                    // memory positions 8 g + e of the block = keys 4 e + g
            H8 p; p.u = *(const uint4*)(vtf + skw_vtfrag_off(slot, H, Tpad, h * 64 + c, 32 * j + 8 * g));
#pragma unroll
            for (int e = 0; e < 8; ++e) x[8 * g + e] = (32 * j + 4 * e + g < count) ? h2f(p.h[e]) : 0.0f;
        }
        skw_ggml_quantize_q8_block(x, qs, &d, &s);                       // (amax and the per-element rounding do not depend on the order of the 32)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            union { int8_t b[8]; uint2 w; } o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o.b[e] = qs[8 * g + e];
            *(uint2*)(rec + 2048 + (ct >> 1) * 1024 + ((c & 15) + 16 * g) * 16 + (ct & 1) * 8) = o.w;
        }
        *(uint16_t*)(rec + SKW_KV8_SCALES + (16 * ((c >> 2) & 3) + 8 + 2 * ct + ((c >> 1) & 1)) * 4 + (c & 1) * 2) = skw_f32_to_f16(d);
    }
}
void skw_kv8_quantize(const half_t* kf, const half_t* vtf, uint8_t* img, int slot0, int n_slots, int H, int n_ctx, int Tpad, const int* slot_k, hipStream_t s) {
    hipLaunchKernelGGL(k_kv8_quantize, dim3(Tpad >> 5, n_slots * H), dim3(128), 0, s, kf, vtf, img, slot0, H, n_ctx, Tpad, slot_k);
}

// lane j16 of the caller's row of 16 lanes (DPP row_newbcast: one VALU move, no LDS)
template <int J> __device__ __forceinline__ unsigned kv8_row_bcast(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x150 + J, 0xf, 0xf, false); }
__device__ __forceinline__ float kv8_lo(unsigned w) { return h2f(__builtin_bit_cast(half_t, (uint16_t)(w & 0xffffu))); }
__device__ __forceinline__ float kv8_hi(unsigned w) { return h2f(__builtin_bit_cast(half_t, (uint16_t)(w >> 16))); }
// four int8 -> two registers of two f16 each (see the file comment)
__device__ __forceinline__ void kv8_widen4(unsigned w, unsigned& lo, unsigned& hi) {
    const unsigned x = w ^ 0x80808080u;
    const f16x2_t bias = {(_Float16)-1152.0f, (_Float16)-1152.0f};
    const f16x2_t a = __builtin_bit_cast(f16x2_t, __builtin_amdgcn_perm(x, 0x64646464u, 0x00050004u)) + bias;
    const f16x2_t b = __builtin_bit_cast(f16x2_t, __builtin_amdgcn_perm(x, 0x64646464u, 0x00070006u)) + bias;
    lo = __builtin_bit_cast(unsigned, a); hi = __builtin_bit_cast(unsigned, b);
}

template <int HPW, int RD, bool VARK, bool RAW>
__global__ __launch_bounds__(256 * HPW, (HPW >= 3) ? 1 : 3 / HPW) void k_dec_cross_attn_kv8(const half_t* q, long ldq, const uint8_t* img, int n_ctx, int Tpad, int H, half_t* out, long ldo,
                                                                                           const int* active, int active_stride, int f32_out, const int* seq, int ofrag_k, SkwKClk* clk,
                                                                                           const int* nkeys, float* raw) {
    constexpr int AUX = 2;
    const int b = blockIdx.y;
    const bool row_live = !(active && !active[b * active_stride]);
    SkwKClkRec* rec = nullptr; unsigned long long t_in = 0;             // thread 0 only
    if (clk && threadIdx.x == 0) {
        t_in = wall_clock64();
        const unsigned wg = blockIdx.y * gridDim.x + blockIdx.x;
        if (wg < SKW_KCLK_MAX_WG) {
            const unsigned launch = clk->cnt[wg]; clk->cnt[wg] = launch + 1;
            if (row_live && launch < clk->cap) rec = &clk->rec[launch][wg % SKW_KCLK_SHARDS];
        }
    }
    if (!row_live) return;
    __shared__ float cmb[HPW][4][66];                                   // per wave: m, l, O[64]
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hs = w >> 2, part = w & 3;
    const int hraw = blockIdx.x * HPW + hs;
    const bool valid = hraw < H;
    const int h = valid ? hraw : H - 1;
    const int bs = seq ? seq[b * active_stride] : b;
    const int r16 = lane & 15, g = lane >> 4;
    const int nkb = Tpad >> 5;                                          // the image's records per (slot, head)
    const int n_stride = n_ctx;                                         // RAW: the key stride of the scores
    if constexpr (VARK) { const int nk = nkeys[b * active_stride]; if (nk > 0) n_ctx = min(nk, n_ctx); }      // (uniform per workgroup)
    const int nkw = VARK ? (n_ctx + 31) >> 5 : nkb;                     // the blocks walked
    const int first = part, step = 4, cnt = (nkw - part + 3) >> 2;
    // the query as two q8_0 blocks (skw_ggml_quantize_q8_block, operation for operation): lane group g holds d = 32 kk + 8 g .. + 7 — its share of the B operand
    long qb[2]; float dq[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const f16x8_t qv = *(const f16x8_t*)(q + (long)b * ldq + h * 64 + kk * 32 + g * 8);
        float x[8], amax = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { x[e] = (float)qv[e]; const float a = x[e] < 0.0f ? -x[e] : x[e]; if (a > amax) amax = a; }
        amax = fmaxf(amax, __shfl_xor(amax, 16)); amax = fmaxf(amax, __shfl_xor(amax, 32));      // (no NaN reaches a query; amax >= 0)
        const float d = amax / 127.0f, id = d != 0.0f ? 1.0f / d : 0.0f;
        union { int8_t b8[8]; long l; } o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.b8[e] = (int8_t)(int)skw_roundf(x[e] * id);
        qb[kk] = o.l; dq[kk] = skw_round_f16(d);
    }
    __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)(img + skw_kv8_rec_off(bs, H, Tpad, h, 0)), 0, (unsigned)(nkb * SKW_KV8_REC), 0x00020000);
    u32x4 ring[RD][4]; unsigned ring_s[RD];
    // one record's loads: 2 KiB of K bytes (two key tiles, both d halves per lane), 2 KiB of V^T bytes (two channel-tile pairs), 256 B of scales
    auto issue = [&](int slot, int kb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ring[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(rk, (unsigned)(kb * SKW_KV8_REC + i * 1024 + lane * 16), 0, AUX);
        ring_s[slot] = __builtin_amdgcn_raw_buffer_load_b32(rk, (unsigned)(kb * SKW_KV8_REC + SKW_KV8_SCALES + lane * 4), 0, AUX);
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll
    for (int j = 0; j < RD; ++j) if (j < cnt) issue(j, first + j * step);
    constexpr float LOG2E = 1.44269504088896340736f;
    float m = -INFINITY, l = 0.0f;
    f32x4 o[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) o[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < cnt; n0 += RD) {
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int n = n0 + j, kb = first + n * step;
            if (n < cnt) {                                              // wave-uniform
                const unsigned sw = ring_s[j];
                unsigned ksc[8];                                        // (dk of d 0 .. 31, dk of d 32 .. 63) of the lane group's eight keys
                ksc[0] = kv8_row_bcast<0>(sw); ksc[1] = kv8_row_bcast<1>(sw); ksc[2] = kv8_row_bcast<2>(sw); ksc[3] = kv8_row_bcast<3>(sw);
                ksc[4] = kv8_row_bcast<4>(sw); ksc[5] = kv8_row_bcast<5>(sw); ksc[6] = kv8_row_bcast<6>(sw); ksc[7] = kv8_row_bcast<7>(sw);
                float sc[2][4];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const u32x4 kt = ring[j][t];
                    const long a0 = (long)(((unsigned long)kt[1] << 32) | kt[0]), a1 = (long)(((unsigned long)kt[3] << 32) | kt[2]);
                    const i32x4 i0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, qb[0], (i32x4){0, 0, 0, 0}, 0, 0, 0);
                    const i32x4 i1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, qb[1], (i32x4){0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[t][r] = skw_kv8_score(kv8_lo(ksc[4 * t + r]), dq[0], i0[r], kv8_hi(ksc[4 * t + r]), dq[1], i1[r]);
                }
                if constexpr (RAW) {
                    if (r16 == 0 && valid) {
#pragma unroll
                        for (int t = 0; t < 2; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) { const int key = kb * 32 + 4 * (4 * t + r) + g; if (key < n_ctx) raw[((long)b * H + h) * n_stride + key] = sc[t][r]; }
                    }
                }
                if (kb * 32 + 32 > n_ctx) {                             // the block with the pad keys: -inf by the row's count
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) if (kb * 32 + 4 * (4 * t + r) + g >= n_ctx) sc[t][r] = -INFINITY;
                }
                float bm = fmaxf(fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3])), fmaxf(fmaxf(sc[1][0], sc[1][1]), fmaxf(sc[1][2], sc[1][3])));
                bm = fmaxf(bm, __shfl_xor(bm, 16)); bm = fmaxf(bm, __shfl_xor(bm, 32));
                if (bm > m) {                                           // wave-uniform (every lane holds the same bm and m)
                    const float a = __builtin_amdgcn_exp2f((m - bm) * LOG2E);       // first block: exp2(-inf) = 0 on empty accumulators
                    l = l * a;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) { o[ct][0] *= a; o[ct][1] *= a; o[ct][2] *= a; o[ct][3] *= a; }
                    m = bm;
                }
                const float mc = m * LOG2E;
                f16x8_t pb;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    // masked keys: exp2(-inf) = 0; the sum is of the rounded values the MFMA multiplies
                    for (int r = 0; r < 4; ++r) { const half_t ph = f2h(__builtin_amdgcn_exp2f(__builtin_fmaf(sc[t][r], LOG2E, -mc))); pb[4 * t + r] = ph; l = l + h2f(ph); }
                unsigned vsc[8];                                        // dv of the lane's sixteen channels 16 ct + 4 g + r: dword 2 ct + (r >> 1), half r & 1
                vsc[0] = kv8_row_bcast<8>(sw); vsc[1] = kv8_row_bcast<9>(sw); vsc[2] = kv8_row_bcast<10>(sw); vsc[3] = kv8_row_bcast<11>(sw);
                vsc[4] = kv8_row_bcast<12>(sw); vsc[5] = kv8_row_bcast<13>(sw); vsc[6] = kv8_row_bcast<14>(sw); vsc[7] = kv8_row_bcast<15>(sw);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {                        // pad keys hold qs = 0 (and any int8 is finite): p = 0 needs no help
                    const u32x4 vw = ring[j][2 + (ct >> 1)];
                    unsigned v0, v1, v2, v3;
                    kv8_widen4(vw[2 * (ct & 1)], v0, v1); kv8_widen4(vw[2 * (ct & 1) + 1], v2, v3);
                    const u32x4 vh = {v0, v1, v2, v3};
                    const f32x4 bsum = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, vh), pb, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    o[ct][0] = __builtin_fmaf(kv8_lo(vsc[2 * ct]), bsum[0], o[ct][0]); o[ct][1] = __builtin_fmaf(kv8_hi(vsc[2 * ct]), bsum[1], o[ct][1]);
                    o[ct][2] = __builtin_fmaf(kv8_lo(vsc[2 * ct + 1]), bsum[2], o[ct][2]); o[ct][3] = __builtin_fmaf(kv8_hi(vsc[2 * ct + 1]), bsum[3], o[ct][3]);
                }
                if (n + RD < cnt) issue(j, kb + RD * step);             // the slot's next record (RD - 1 records stay in flight while one is consumed)
            }
        }
    }
    if constexpr (RAW) return;                                          // (uniform: no barrier was passed)
    l = l + __shfl_xor(l, 16); l = l + __shfl_xor(l, 32);
    float* cw = cmb[hs][part];
    if (lane == 0) { cw[0] = m; cw[1] = l; }
    if (r16 == 0) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) cw[2 + ct * 16 + 4 * g + r] = o[ct][r];
    }
    __syncthreads();
    if (part == 0 && valid) {
        float M = cmb[hs][0][0];
#pragma unroll
        for (int i = 1; i < 4; ++i) M = fmaxf(M, cmb[hs][i][0]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        // an empty quarter: m = -inf, a = 0
        for (int i = 0; i < 4; ++i) { const float a = __builtin_amdgcn_exp2f((cmb[hs][i][0] - M) * LOG2E);
        num = __builtin_fmaf(cmb[hs][i][2 + lane], a, num); den = __builtin_fmaf(cmb[hs][i][1], a, den); }
        att_store_m(out, b, ldo, h * 64 + lane, num / den, f32_out, ofrag_k);
    }
    if (rec) {      // earliest begin and latest end over the workgroups, as k_dec_cross_attn16 records them
        atomicMax(&rec->t0_inv, ~t_in); atomicMax(&rec->t1, wall_clock64());
        if (blockIdx.x == 0) { atomicAdd(&rec->live_rows, 1u); atomicAdd(&rec->keys, (unsigned)n_ctx); }
    }
}

template <bool VARK, bool RAW>
static void kv8_launch(dim3 grid, dim3 blk, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, const half_t* q, long ldq, const uint8_t* img, int n_ctx, int Tpad, int H, half_t* out,
                       long ldo, const int* active, int as, int f32_out, const int* seq, int ofrag_k, SkwKClk* clk, const int* nkeys, float* raw) {
    skw_launch_ev(k_dec_cross_attn_kv8<3, SKW_KV8_RD, VARK, RAW>, grid, blk, 0, s, ev_start, ev_stop, q, ldq, img, n_ctx, Tpad, H, out, ldo, active, as, f32_out, seq, ofrag_k, clk, nkeys, raw);
}
void skw_dec_cross_attn_kv8(const half_t* q, const uint8_t* img, int B, int H, int d, int n_ctx, int Tpad, half_t* out, const int* active, hipStream_t s, int f32_out, const int* seq,
                            hipEvent_t ev_start, hipEvent_t ev_stop, int ofrag, SkwKClk* clk, const int* nkeys, float* raw) {
    const int as = (int)(sizeof(SkwSeqState) / 4);
    const dim3 grid((H + 2) / 3, B), blk(768);        // three heads per workgroup, as skw_dec_cross_attn_vt
    if (raw) {
        if (nkeys) kv8_launch<true, true>(grid, blk, s, ev_start, ev_stop, q, (long)d, img, n_ctx, Tpad, H, out, (long)d, active, as, f32_out & 1, seq, ofrag ? d : 0, clk, nkeys, raw);
        else kv8_launch<false, true>(grid, blk, s, ev_start, ev_stop, q, (long)d, img, n_ctx, Tpad, H, out, (long)d, active, as, f32_out & 1, seq, ofrag ? d : 0, clk, nkeys, raw);
    } else if (nkeys) kv8_launch<true, false>(grid, blk, s, ev_start, ev_stop, q, (long)d, img, n_ctx, Tpad, H, out, (long)d, active, as, f32_out & 1, seq, ofrag ? d : 0, clk, nkeys, raw);
    else kv8_launch<false, false>(grid, blk, s, ev_start, ev_stop, q, (long)d, img, n_ctx, Tpad, H, out, (long)d, active, as, f32_out & 1, seq, ofrag ? d : 0, clk, nkeys, raw);
}
