// skw_kernels_dec.hip — the decoder's embedding and attention kernels for gfx950 (CDNA4): self attention, the decode step's cross attention in
// both precisions, the exact precision's prompt pass.
// Compile with -ffp-contract=off: every fused multiply-add in here is explicit (see include/skw_math.h).
//
// What each kernel restates (whisper.cpp routine; the reference's call site is plugins/native/whisper/src/lib.rs:644-646 `whisper_state.full`):
//   k_dec_*            whisper_decode_internal pieces (K7-K9)
#include <atomic>
#include "skw_dev_common.h"

// (att_store / att_store_m, the attention outputs' stores: skw_dev_common.h — the q8 cross-attention kernel of skw_kernels_kv8.hip shares them)
// ------------------------------------------------------------------ decoder pieces
__global__ void k_dec_embed(const half_t* te, const float* pe, const int* tok, const int* pos, int d, float* x) {
    const int b = blockIdx.x; const int tk = tok[b * (int)(sizeof(SkwSeqState) / 4)]; const int ps = pos[b * (int)(sizeof(SkwSeqState) / 4)];
    for (int i = threadIdx.x; i < d; i += blockDim.x) x[(long)b * d + i] = h2f(te[(long)tk * d + skw_kperm(i)]) + pe[(long)ps * d + i];
}
// the same with the first layer's LayerNorm attached: one wave per row, x written in passing (d <= 1536)
template <int NC, bool FULL>
__global__ __launch_bounds__(256) void k_dec_embed_ln(const half_t* te, const float* pe, const int* tok, const int* pos, int B, int d, float* x, const float* w, const float* b, half_t* y16) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const int tk = tok[row * (int)(sizeof(SkwSeqState) / 4)], ps = pos[row * (int)(sizeof(SkwSeqState) / 4)];
    float v[1][NC], wv[NC], bv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int i = lane + 64 * c; const bool in = FULL || i < d;
        v[0][c] = in ? h2f(te[(long)tk * d + skw_kperm(i)]) + pe[(long)ps * d + i] : 0.0f; wv[c] = in ? w[i] : 0.0f; bv[c] = in ? b[i] : 0.0f;
        if (in) x[(long)row * d + i] = v[0][c];
    }
    const bool live[1] = {true}; half_t* const o16[1] = {y16 + (long)row * d}; float* const o32[1] = {nullptr};
    skw_ln_rows<1, NC, FULL>(v, wv, bv, d, lane, live, o16, o32);
}
void skw_dec_embed(const half_t* te, const float* pe, const int* tok, const int* pos, int B, int d, float* x, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_embed, dim3(B), dim3(256), 0, s, te, pe, tok, pos, d, x);
}
void skw_dec_embed_ln(const half_t* te, const float* pe, const int* tok, const int* pos, int B, int d, float* x, const float* w, const float* b, half_t* y16, hipStream_t s) {
    if (d == 768) hipLaunchKernelGGL((k_dec_embed_ln<12, true>), dim3((B + 3) / 4), dim3(256), 0, s, te, pe, tok, pos, B, d, x, w, b, y16);
    else if (d <= 768) hipLaunchKernelGGL((k_dec_embed_ln<12, false>), dim3((B + 3) / 4), dim3(256), 0, s, te, pe, tok, pos, B, d, x, w, b, y16);
    else hipLaunchKernelGGL((k_dec_embed_ln<24, false>), dim3((B + 3) / 4), dim3(256), 0, s, te, pe, tok, pos, B, d, x, w, b, y16);
}


// single-query attention over n_kv keys with plain f16 K/V rows (row stride ldkv halves), head dim 64.
//   s_j = chain_d q[d] K[j][d];  softmax as ggml_soft_max_ext (scale 1, f64 denominator);  out[c] = chain_j f16(p_j) V[j][c]
// One wave per (sequence, head), no block-level synchronisation: lane = key for the scores (64 independent d-chains per
// pass over K), lane = channel for P.V (one key-ascending chain per output, p_j broadcast with v_readlane).
// A block is 4 waves = 4 heads of one sequence.
template <int MAXT, bool FASTV = false>      // FASTV (f16_mfma only): the V rows arrive as 16-byte pieces and each lane sums its own keys' share — see below
__global__ __launch_bounds__(256) void k_dec_attn(const half_t* q, long ldq, const half_t* kbase, const half_t* vbase, long batch_stride, long ldkv,
                                                  const int* n_kv_ptr, int n_kv_stride, int n_kv_fixed, int H, half_t* out, long ldo, const int* active, int active_stride, int f32_out, SkwQ8Out q8,
                                                  const int* seq, int ofrag_k) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (h >= H) return;
    const int act = active ? active[b * active_stride] : 1;   // (tested after the prefetches below are on their way: one round trip for all of them)
    const int bs = seq ? seq[b * active_stride] : b;          // the prompt pass: row b is one prompt token of sequence seq[b] (one more round trip there; the step has seq == null)
    const half_t* K = kbase + (long)bs * batch_stride + h * 64;
    const half_t* V = vbase + (long)bs * batch_stride + h * 64;
    // Everything whose address depends on nothing loaded is requested before the first wait, in the order it is needed (a wave's loads return in
    // order): q and the first 64 K rows, which the score chains start on, then the V rows of the first NPRE keys, which arrive under them (rows
    // past n_kv exist in the cache and are simply not used): the short-context steps pay one round trip, not one per 16 keys after the softmax.
    constexpr int NPRE = (MAXT * 64 < 128) ? MAXT * 64 : 128;
    const int rows_cap = (int)(batch_stride / ldkv);
    uint4 qraw[8];
    { const uint4* qp = (const uint4*)(q + (long)b * ldq + h * 64);
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8) qraw[c8] = qp[c8]; }
    uint4 kk0[8];
    { const uint4* kr = (const uint4*)(K + (long)min(lane, rows_cap - 1) * ldkv);
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8) kk0[c8] = kr[c8]; }
    __builtin_amdgcn_sched_barrier(0);
    // FASTV.  The exact form below gives lane c the key-ascending fma chain of channel c: one 2-byte load per key and lane (128 load instructions for the prefetched keys, about a
    // microsecond of issue in a 8.6 us kernel) and a readlane + convert + fma per key.  The tolerance precision owes no order: lane (kg = lane >> 3, piece = lane & 7) takes the
    // 16-byte piece `piece` of the rows of keys kg, kg + 8, ... (one load instruction = eight whole 128-byte head rows), sums p_key * v over ITS keys for its eight channels, and the
    // eight key groups meet in three shuffle steps.  16 load instructions instead of 128, 8 fmas per key and lane group instead of 64.
    constexpr int NPV = FASTV ? NPRE / 8 : 1;
    half_t vpre[FASTV ? 1 : NPRE];
    uint4 vq[NPV];
    const int kg = lane >> 3, piece = lane & 7;
    if constexpr (FASTV) {
#pragma unroll
        for (int u = 0; u < NPV; ++u) vq[u] = *(const uint4*)(V + (long)min(u * 8 + kg, rows_cap - 1) * ldkv + piece * 8);
    } else {
        const half_t* vp0 = V + lane;
#pragma unroll
        for (int u = 0; u < NPRE; ++u) vpre[u] = vp0[(long)min(u, rows_cap - 1) * ldkv];
    }
    __builtin_amdgcn_sched_barrier(0);
    float qv[64];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) { H8 t; t.u = qraw[c8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[c8 * 8 + e] = h2f(t.h[e]); }
    const int n_kv = n_kv_ptr ? (n_kv_ptr[b * n_kv_stride] + 1) : n_kv_fixed;
    if (!act) return;                                        // a finished sequence keeps its slot in the batch; its row is never sampled again
    float sc[MAXT];
    float lmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        sc[t] = -INFINITY;
        if (t * 64 < n_kv) {   // wave-uniform
            const int key = t * 64 + lane;
            uint4 kk[8];
            if (t == 0) {
#pragma unroll
                for (int c8 = 0; c8 < 8; ++c8) kk[c8] = kk0[c8];
            } else {
                const uint4* kr = (const uint4*)(K + (long)min(key, n_kv - 1) * ldkv);
#pragma unroll
                for (int c8 = 0; c8 < 8; ++c8) kk[c8] = kr[c8];
            }
            float a = 0.0f;
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) { H8 t8; t8.u = kk[c8];
#pragma unroll
                for (int e = 0; e < 8; ++e) a = __builtin_fmaf(qv[c8 * 8 + e], h2f(t8.h[e]), a); }
            if (key < n_kv) { sc[t] = a; lmax = fmaxf(lmax, a); }
        }
    }
    lmax = skw_wave_max_f32(lmax);
    double lsum = 0.0;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) if (t * 64 < n_kv) { float e = skw_expf(sc[t] - lmax); sc[t] = e; lsum += (double)e; }
    lsum = skw_wave_sum_f64(lsum);
    const float inv = (float)(1.0 / lsum);
#pragma unroll
    for (int t = 0; t < MAXT; ++t) if (t * 64 < n_kv) sc[t] = h2f(f2h(sc[t] * inv));
    if constexpr (FASTV) {
        float a8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) a8[e] = 0.0f;
        const int ngrp = (n_kv + 7) >> 3;                     // groups of eight keys (wave-uniform)
#pragma unroll
        for (int u = 0; u < NPV; ++u) {
            if (u < ngrp) {
                const int key = u * 8 + kg;
                const float pk = __shfl(sc[(u * 8) >> 6], key & 63);          // (the group's eight keys lie in one 64-key pass)
                if (key < n_kv) { H8 v8; v8.u = vq[u];
#pragma unroll
                    for (int e = 0; e < 8; ++e) a8[e] = __builtin_fmaf(pk, h2f(v8.h[e]), a8[e]); }
            }
        }
        for (int u = NPV; u < ngrp; ++u) {                    // keys past the prefetched 128 (long prompts): one load per group
            const int key = u * 8 + kg;
            H8 v8; v8.u = *(const uint4*)(V + (long)min(key, n_kv - 1) * ldkv + piece * 8);
            float pk = 0.0f;
#pragma unroll
            for (int t = NPRE / 64; t < MAXT; ++t) if ((u * 8) >> 6 == t) pk = __shfl(sc[t], key & 63);
            if (key < n_kv) {
#pragma unroll
                for (int e = 0; e < 8; ++e) a8[e] = __builtin_fmaf(pk, h2f(v8.h[e]), a8[e]); }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { a8[e] += __shfl_xor(a8[e], 8); a8[e] += __shfl_xor(a8[e], 16); a8[e] += __shfl_xor(a8[e], 32); }
        if (kg == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) att_store_m(out, b, ldo, h * 64 + piece * 8 + e, a8[e], f32_out, ofrag_k);
        }
        return;
    }
    // P.V: lane = channel
    float acc = 0.0f;
    const half_t* vp = V + lane;
#pragma unroll
    for (int g16 = 0; g16 < NPRE / 16; ++g16) {          // keys [0, NPRE) from the prefetched rows, ascending
        const int pbits = __float_as_int(sc[g16 >> 2]);
        if (g16 * 16 + 16 <= n_kv) {
#pragma unroll
            for (int u = 0; u < 16; ++u) acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(pbits, (g16 & 3) * 16 + u)), h2f(vpre[g16 * 16 + u]), acc);
        } else if (g16 * 16 < n_kv) {
#pragma unroll
            for (int u = 0; u < 16; ++u) if (g16 * 16 + u < n_kv) acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(pbits, (g16 & 3) * 16 + u)), h2f(vpre[g16 * 16 + u]), acc);
        }
    }
#pragma unroll
    for (int t = NPRE / 64; t < MAXT; ++t) {
        if (t * 64 < n_kv) {
            const int nj = min(64, n_kv - t * 64);
            const int pbits = __float_as_int(sc[t]);
            const half_t* vt = vp + (long)t * 64 * ldkv;
            int jj = 0;
            for (; jj + 16 <= nj; jj += 16) {
                half_t vv[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) vv[u] = vt[(long)(jj + u) * ldkv];
#pragma unroll
                for (int u = 0; u < 16; ++u) acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(pbits, jj + u)), h2f(vv[u]), acc);
            }
            for (; jj < nj; ++jj) acc = __builtin_fmaf(__int_as_float(__builtin_amdgcn_readlane(pbits, jj)), h2f(vt[(long)jj * ldkv]), acc);
        }
    }
    if (q8.q) {   // the projection that follows multiplies by block-quantised weights: the row leaves as ggml's q8 blocks (a head's 64 channels = two blocks)
        float dd, ss; const int qi = q8_half_wave_block(acc, &dd, &ss);
        const int i = h * 64 + lane, blk = i >> 5;
        q8.q[(long)b * ldo + i] = (int8_t)qi;
        if ((lane & 31) == 0) { q8.dT[(long)blk * q8.M + b] = dd; q8.sT[(long)blk * q8.M + b] = ss; }
        return;
    }
    att_store_m(out, b, ldo, h * 64 + lane, acc, f32_out, ofrag_k);
}
// ------------------------------------------------------------------ decoder cross-attention (K9), bandwidth form
// Two waves per (sequence, head), three heads per workgroup (12 heads x 64 sequences = 256 workgroups of 6 waves: every CU, 1.5 waves/SIMD).
// Scores: the pair splits the keys; lane = key, 64 independent d-ascending chains per pass.  K rows [key][768] plain are fetched
// coalesced (8 lanes x 16 B = one 128-byte head row, so each cache line is consumed by the instruction that fetched it) through a
// 3-deep register ring and transposed in a per-wave LDS slab (row stride 144 B: conflict-free ds_read_b128).
// P.V on the matrix cores, the pair splitting the channels: A = V^T fragment (cross V is stored per head as [channel][Tpad kperm], one
// 16-byte load = 8 keys of one channel), B = p broadcast to every column, so each output channel is the same key-ascending fma chain
// as the scalar form; an 8-deep ring keeps V^T in flight (4 .. 16 deep measure the same within 2 %).  HBM-bound: 55.3 MB per sequence per step over all layers.
// (HIP's uint4 arrays defeat SROA and land in scratch; the rings use ext_vector types.)
#ifndef SKW_XATTN_RD16
#define SKW_XATTN_RD16 16      // V^T blocks in flight per wave in the f16_mfma P.V (8: 56.4 us per launch in tools/xattn_probe.py, 12: 55.7, 16: 55.7, 24: 56.1)
#endif
template <int MAXT, int WPH, int HPW, bool PV16 = false>
__global__ __launch_bounds__(64 * HPW * WPH, (HPW * WPH >= 12) ? 1 : 12 / (HPW * WPH)) void k_dec_cross_attn(const half_t* q, long ldq, const half_t* kbase, long k_batch_stride, long ldk,
                                                           const half_t* vtbase, int n_ctx, int Tpad, int H, half_t* out, long ldo, const int* active, int active_stride,
                                                               int f32_out, const int* seq, const int* nkeys) {
    const int bx = blockIdx.x, by = blockIdx.y;
    if (active && !active[by * active_stride]) return;      // uniform per workgroup (one sequence): a finished sequence stops streaming its 55 MB of cross K/V
    // per-clip audio context: the row's key count from device memory (0: the model's); the caller's n_ctx and Tpad stay the strides of cross K / V^T
    if (nkeys) { const int nk = nkeys[by * active_stride]; if (nk > 0) n_ctx = min(nk, n_ctx); }
    __shared__ float plds[HPW][MAXT * 64];
    __shared__ __attribute__((aligned(16))) half_t klds[HPW * WPH][64 * 72];
    __shared__ float smax[HPW][WPH];
    __shared__ double ssum[HPW][WPH];
    __shared__ __attribute__((aligned(16))) half_t p16[PV16 ? HPW : 1][PV16 ? MAXT * 64 : 8];      // PV16: the probabilities as f16 in kperm order, the f16 MFMA's second operand
    // half = this wave's part of the head (keys in the score phase, channels in P.V); readfirstlane: keeps the buffer descriptor in SGPRs (no waterfall loops)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hs = w / WPH, half = w % WPH;
    const int hraw = bx * HPW + hs, b = by;
    const bool valid = hraw < H;               // no early return: the pair meets at workgroup barriers
    const int h = valid ? hraw : H - 1;
    const int bs = seq ? seq[b * active_stride] : b;          // the prompt pass: row b attends over the cross K / V of sequence seq[b]
    const half_t* K = kbase + (long)bs * k_batch_stride + h * 64;
    auto ldk16 = [&](const half_t* p) -> u32x4 { return *(const u32x4*)p; };   // (non-temporal loads of the once-read K / V^T bytes measured 2 us slower per launch: 62.7 vs 60.4)
    H8v qh[8];                                  // q stays packed (32 VGPRs instead of 64); converted in the chain's shadow
    const int nt = (n_ctx + 63) >> 6, nth = (nt + WPH - 1) / WPH;
    const int t_lo = half * nth, t_hi = min(nt, t_lo + nth);
    float lmax = -INFINITY;
    half_t* kl = klds[w];
    float* pl = plds[hs];
    const int lrow = lane >> 3, lseg = lane & 7;
    u32x4 k0[8], k1[8], k2[8];
    auto kfill = [&](u32x4 (&dst)[8], int t) {
#pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = ldk16(K + (long)min(t * 64 + i * 8 + lrow, n_ctx - 1) * ldk + lseg * 8);
        __builtin_amdgcn_sched_barrier(0);
    };
    {
        const u32x4* qp = (const u32x4*)(q + (long)b * ldq + h * 64);
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) qh[c8].v = qp[c8];
        kfill(k0, t_lo); kfill(k1, t_lo + 1);
    }
    // one pass = 64 keys: refill the free ring slot with pass t+2 first, then consume `cur`.  Roles rotate by name (three passes per
    // loop trip) so no register copies force early waits, and the scheduling barriers keep the loads where they are written.
    auto pass = [&](int t, u32x4 (&cur)[8], u32x4 (&fill)[8]) {
        // (wave-uniform) no refill past this wave's key range: the two passes after it belong to the next wave of the head, which fetches them itself — unconditional
        // refills were a third more K requests per wave (8 passes fetched for 6 consumed), and the PMC pass showed them arriving from memory, not from a cache:
        // 338 MB read per 64-row launch against 295 MB algorithmic
        if (t + 2 < t_hi) {
#pragma unroll
            for (int i = 0; i < 8; ++i) fill[i] = ldk16(K + (long)min((t + 2) * 64 + i * 8 + lrow, n_ctx - 1) * ldk + lseg * 8);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t < t_hi) {       // wave-uniform
            const int key = t * 64 + lane;
            float a = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) *(u32x4*)(kl + (i * 8 + lrow) * 72 + lseg * 8) = cur[i];
            __builtin_amdgcn_wave_barrier();   // same wave, LDS in order: a compiler-level fence is all that is needed
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) asm volatile("" : "+v"(qh[c8].v));   // opaque: stops the 64 conversions being hoisted out of the loop into 64 live registers
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) { H8v t8; t8.v = *(const u32x4*)(kl + lane * 72 + c8 * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) a = __builtin_fmaf(h2f(qh[c8].h[e]), h2f(t8.h[e]), a); }
            __builtin_amdgcn_wave_barrier();
            if (key >= n_ctx) a = -INFINITY;
            pl[key] = a; lmax = fmaxf(lmax, a);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll 1
    for (int t = t_lo; t < t_hi; t += 3) { pass(t, k0, k2); pass(t + 1, k1, k0); pass(t + 2, k2, k1); }
    // V^T ring: start the first loads before the softmax so they fly during it
    const int r16 = lane & 15, g = lane >> 4;
    const long bh = (long)bs * H + h;
    __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(vtbase + bh * 64 * Tpad), 0, (unsigned)(64 * Tpad * 2), 0x00020000);
    constexpr int CT = 4 / WPH;                                                   // channel tiles per wave
    const unsigned vo = (unsigned)(((half * CT * 16 + r16) * Tpad + g * 8) * 2);
    const int nkb = (n_ctx + 31) >> 5;                                            // the 32-key blocks below the row's key count (a full row: Tpad >> 5)
    constexpr int RD = PV16 ? SKW_XATTN_RD16 : 8;
    H8v ring[RD][CT];
#pragma unroll
    for (int j = 0; j < RD; ++j)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) { ring[j][ct].v = __builtin_amdgcn_raw_buffer_load_b128(rv, (j < nkb) ? vo + ct * 16 * Tpad * 2 + j * 64 : 0x7fffff00u, 0, 0);
        __builtin_amdgcn_sched_barrier(0); }
    lmax = skw_wave_max_f32(lmax);
    if (lane == 0) smax[hs][half] = lmax;
    __syncthreads();
    lmax = smax[hs][0];
#pragma unroll
    for (int i = 1; i < WPH; ++i) lmax = fmaxf(lmax, smax[hs][i]);
    double lsum = 0.0;
    for (int t = t_lo; t < t_hi; ++t) { float e = skw_expf(pl[t * 64 + lane] - lmax); pl[t * 64 + lane] = e; lsum += (double)e; }   // exp(-inf) == 0 for masked keys
    lsum = skw_wave_sum_f64(lsum);
    if (lane == 0) ssum[hs][half] = lsum;
    __syncthreads();
    double tot = ssum[hs][0];
#pragma unroll
    for (int i = 1; i < WPH; ++i) tot += ssum[hs][i];
    const float inv = (float)(1.0 / tot);
    if constexpr (PV16) {
        for (int t = t_lo; t < t_hi; ++t) p16[hs][skw_kperm(t * 64 + lane)] = f2h(pl[t * 64 + lane] * inv);
        for (int t = nt + half; t < MAXT; t += WPH) p16[hs][t * 64 + lane] = (half_t)0.0f;
    } else {
    for (int t = t_lo; t < t_hi; ++t) pl[t * 64 + lane] = h2f(f2h(pl[t * 64 + lane] * inv));
    for (int t = nt + half; t < MAXT; t += WPH) pl[t * 64 + lane] = 0.0f;      // key slots past the last pass (V^T pad is zero as well)
    }
    __syncthreads();
    f32x4 oacc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) oacc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kb0 = 0; kb0 < nkb; kb0 += RD) {
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int kb = kb0 + j;
            H8v vf[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) vf[ct] = ring[j][ct];
            const int nb = kb + RD;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) ring[j][ct].v = __builtin_amdgcn_raw_buffer_load_b128(rv, (nb < nkb) ? vo + ct * 16 * Tpad * 2 + nb * 64 : 0x7fffff00u, 0, 0);
            const int kbc = min(kb, nkb - 1);     // blocks past the end multiply p by zero-filled fragments
            // keys past the row's count in its last block: V^T there is an earlier, longer call's (or a don't-care encoder row's) — replaced by zeros, never multiplied by p = 0
            if (kbc * 32 + 32 > n_ctx) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (kbc * 32 + 4 * e + g >= n_ctx) vf[ct].h[e] = f2h(0.0f);
            }
            if constexpr (PV16) {
                // f16_mfma precision: p is f16-valued and V^T is f16, so a 32-key block is ONE v_mfma_f32_16x16x32_f16 (16 cycles) instead of eight dependent
                // f32 MFMAs (256 cycles: tools/xattn_probe.py put them at 8.7 us of a 65 us launch that is otherwise at the memory system's pace).
                // Same products, summed in the matrix core's order for the block rather than key by key.
                typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
                const f16x8_t pb = *(const f16x8_t*)(&p16[hs][kbc * 32 + g * 8]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) oacc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, vf[ct].v), pb, oacc[ct], 0, 0, 0);
                continue;
            }
            float pe[8], xv[CT][8];      // operands first, then the MFMAs back to back (a dependent MFMA directly behind its producer is the cheap case)
#pragma unroll
            for (int e = 0; e < 8; ++e) { pe[e] = pl[kbc * 32 + 4 * e + g];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) xv[ct][e] = h2f(vf[ct].h[e]); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) oacc[ct] = MFMA16(xv[ct][e], pe[e], oacc[ct]);   // O^T[c][*] += V^T[c][key] * p[key]
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // D = O^T replicated over columns: lane (col n = r16, rows 4*g + r) -> channel 32*half + ct*16 + 4*g + r; take column 0
    if (r16 == 0 && valid) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) att_store(out, (long)b * ldo, h * 64 + (half * CT + ct) * 16 + 4 * g + r, oacc[ct][r], f32_out);
    }
}
// ------------------------------------------------------------------ decoder cross-attention (K9), f16_mfma precision: one streaming pass
// The tolerance precision owes the oracle no summation order, so the two-phase form above (all scores, a workgroup-wide softmax, then P.V — a barrier with the HBM
// stream drained in the middle of a 50 us launch) becomes one pass per wave with a running maximum.  Four waves per (row, head), each a contiguous quarter of the
// 32-key blocks; per block a wave takes 4 KB of K rows and 4 KB of V^T straight from memory into MFMA operands — no LDS, no transposes, no conversions:
//   scores   S[key][*] = K[key][:] . q on the f16 matrix cores: A = 16 K rows x 32 d (one 16-byte load per lane), B = q broadcast to every column; two d halves chain;
//            A row i of tile j is key 16 j + 4 (i & 3) + (i >> 2), so that lane group g ends up holding keys 4 e + g (e = 4 j + r) — the order V^T's 32-key blocks
//            are stored in (skw_kperm): the probabilities go into the next MFMA as its B operand as they stand
//   softmax  block maximum across the wave's four lane groups (two DPP-free shuffles per 8 KB), rescale of the 16 accumulators only when the maximum grows,
//            p = exp2((s - m) log2 e) rounded to f16 unnormalised (<= 1: no subnormal loss that 1 / sum would add), per-lane partial sums
//   P.V      O^T[c][*] += V^T[c][keys] . p, four 16-channel tiles, one MFMA each
// and the four partial (m, l, O) meet in LDS at the end (one barrier).  RD blocks (8 KB each) are in flight per wave, 12 waves per CU.
// K and V^T are the fragment-order images (skw_kfrag_off / skw_vtfrag_off): every load instruction is one contiguous KiB, and the loads carry the non-temporal policy (aux = 2: the
// once-read stream stays out of the caches the step's weights live in; 49.5 -> 45.7-46.2 us per full launch, profiles/r03h).  The four waves of a head take every fourth 32-key block, so
// together they walk one sequential stream.  What lost against this form (profiles/r03g, r03h, r04i): the row layouts (16 x 64 B per load instruction), contiguous quarters per wave, 2 / 4
// blocks in flight, one or two heads per workgroup, XCD-aware placement of a sequence's workgroups.
// clk (bench.py's roofline line; null in every other run): the launch's own begin and end on the device's constant-rate clock — see SkwKClk in skw_kernels.h.
// VARK (per-clip audio context; the uniform full-length step keeps the VARK = false instantiation): the row's key count comes from device memory (nkeys, next to `active`), a wave
// walks only the 32-key blocks below it — so no block is all pad, and exp2(-inf - -inf) never happens — and the V^T of the pad keys in the row's last block is replaced by zeros.
template <int HPW, int RD, bool VARK = false>
__global__ __launch_bounds__(256 * HPW, (HPW >= 3) ? 1 : 3 / HPW) void k_dec_cross_attn16(const half_t* q, long ldq, const half_t* kbase, long k_batch_stride, long ldk, const half_t* vtbase,
                                                                                         int n_ctx, int Tpad, int H, half_t* out, long ldo, const int* active,
                                                                                             int active_stride, int f32_out, const int* seq, int ofrag_k, SkwKClk* clk, const int* nkeys) {
    typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
    constexpr int AUX = 2;
    const int b = blockIdx.y;
    const bool row_live = !(active && !active[b * active_stride]);
    SkwKClkRec* rec = nullptr; unsigned long long t_in = 0;             // thread 0 only
    if (clk && threadIdx.x == 0) {
        // this workgroup's own launch count (finished rows count too): launches of one graph node are serial on its stream, the cell is nobody else's
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
    // a wave's blocks: every fourth 32-key block (the four waves of a head walk one sequential stream together)
    const int nkb = Tpad >> 5;                                          // the images' stride
    if constexpr (VARK) { const int nk = nkeys[b * active_stride]; if (nk > 0) n_ctx = min(nk, n_ctx); }      // (uniform per workgroup)
    const int nkw = VARK ? (n_ctx + 31) >> 5 : nkb;                     // the blocks walked
    const int first = part, step = 4, cnt = (nkw - part + 3) >> 2;
    f16x8_t qb[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) qb[kk] = *(const f16x8_t*)(q + (long)b * ldq + h * 64 + kk * 32 + g * 8);
    __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)(kbase + (long)bs * k_batch_stride), 0, (unsigned)((long)Tpad * ldk * 2), 0x00020000);
    __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(vtbase + ((long)bs * H + h) * 64 * Tpad), 0, (unsigned)(64 * Tpad * 2), 0x00020000);
    u32x4 ring[RD][8];
    // one block's loads: 4 KiB of K (two score tiles x two d halves) and 4 KiB of V^T (four channel tiles); pad keys of the last tile hold whatever memory held (masked below)
    auto issue = [&](u32x4 (&slot)[8], int kb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) slot[i] = __builtin_amdgcn_raw_buffer_load_b128(rk, (unsigned)(((h * (nkb * 2) + kb * 2) * 2 + i) * 1024 + lane * 16), 0, AUX);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) slot[4 + ct] = __builtin_amdgcn_raw_buffer_load_b128(rv, (unsigned)((kb * 4 + ct) * 1024 + lane * 16), 0, AUX);
        __builtin_amdgcn_sched_barrier(0);
    };
#pragma unroll
    for (int j = 0; j < RD; ++j) if (j < cnt) issue(ring[j], first + j * step);
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
                f32x4 sc[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, ring[j][t * 2]), qb[0], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, ring[j][t * 2 + 1]), qb[1], sc[t], 0, 0, 0);
                }
                if (kb * 32 + 32 > n_ctx) {                             // the block with the pad keys (their K rows were read from the last real key)
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
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    f16x8_t vt = __builtin_bit_cast(f16x8_t, ring[j][4 + ct]);
                    if constexpr (VARK) {
                        if (kb * 32 + 32 > n_ctx) {                     // (wave-uniform) element e of lane group g is key 4 e + g of the block
#pragma unroll
                            for (int e = 0; e < 8; ++e) if (kb * 32 + 4 * e + g >= n_ctx) vt[e] = (half_t)0.0f;
                        }
                    }
                    o[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vt, pb, o[ct], 0, 0, 0);
                }
                if (n + RD < cnt) issue(ring[j], kb + RD * step);              // the slot's next block (RD - 1 blocks stay in flight while one is consumed)
            }
        }
    }
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
    if (rec) {      // earliest begin and latest end over the workgroups, off the critical path (thread 0 sits in a wave that does the final combine and store)
        atomicMax(&rec->t0_inv, ~t_in); atomicMax(&rec->t1, wall_clock64());
        if (blockIdx.x == 0) { atomicAdd(&rec->live_rows, 1u); atomicAdd(&rec->keys, (unsigned)n_ctx); }
    }
}
void skw_dec_cross_attn_vt(const half_t* q, const half_t* ck, const half_t* cvt, int B, int H, int d, int n_ctx, int Tpad, half_t* out, const int* active, hipStream_t s,
    int f32_out, int pv16, const int* seq, hipEvent_t ev_start, hipEvent_t ev_stop, int ofrag, SkwKClk* clk, const int* nkeys) {
    const int as = (int)(sizeof(SkwSeqState) / 4);
    const dim3 grid((H + 2) / 3, B), blk(768);        // three heads per workgroup: 256 workgroups of 12 waves at 64 rows x 12 heads, one per CU
    // (with events: the kernel's own begin and end are stamped — skw_launch_ev, skw_dev_common.h)
    if (pv16 == 2) {          // f16_mfma precision, fragment-order cross K / V^T: the one-pass streaming kernel
        auto launch = [&](auto kernel) { skw_launch_ev(kernel, grid, blk, 0, s, ev_start, ev_stop, q, (long)d, ck, (long)Tpad * d, (long)d, cvt, n_ctx, Tpad, H, out, (long)d, active, as,
                                                       f32_out & 1, seq, ofrag ? d : 0, clk, nkeys); };
        if (nkeys) launch(k_dec_cross_attn16<3, 3, true>); else launch(k_dec_cross_attn16<3, 3>);
        return;
    }
    // row layouts: the two-phase kernel; pv16 == 1 (f16_mfma with SKW_XATTN_FRAG=0) takes a 32-key block of P.V in one f16 MFMA, the exact precision chains f32 MFMAs key by key
    auto launch = [&](auto kernel) { skw_launch_ev(kernel, grid, blk, 0, s, ev_start, ev_stop, q, (long)d, ck, (long)n_ctx * d, (long)d, cvt, n_ctx, Tpad, H, out, (long)d, active, as,
                                                   f32_out & 1, seq, nkeys); };
    if (pv16) launch(k_dec_cross_attn<24, 4, 3, true>); else launch(k_dec_cross_attn<24, 4, 3>);
}

// ------------------------------------------------------------------ the exact precision's prompt pass: cross attention of 16 queries per workgroup
// A prompt of up to 224 tokens is 224 rows of ONE decoder pass that attend over the same cross K / V^T; k_dec_cross_attn streams the sequence's 4.6 MB per layer once per row.
// Here one workgroup (four waves) serves 16 queries of one (sequence, head): every K / V^T byte is loaded once per 16 queries, and every output element is the bits
// k_dec_cross_attn<24, 4, 3> produces for that row, because each (query, key) and each (channel, query) keeps its own chain:
//   scores   S[key][query] on v_mfma_f32_16x16x4_f32: A = 16 keys x 4 d, B = 4 d x 16 queries, 16 instructions chained over d — the d-ascending chain from 0 of f16-valued
//            products in f32 that the single-query kernel writes as fmas (the columns it would spend on a broadcast hold the other 15 queries).  Wave w takes the 64-key tiles
//            w, w + 4, ..: K rows come in coalesced (16 B per lane), are transposed through a per-wave LDS slab (row stride 144 B) and the next tile's loads fly meanwhile.
//            Keys at or past the row's count are -inf.  The scores of all 16 queries stay in LDS: 16 x (64 nt + 4) floats, 96 KiB at 1500 keys (one workgroup per CU).
//   softmax  wave w owns queries 4 w .. 4 w + 3.  Maximum over all keys (exact in any order), e = skw_expf(s - max), and the f64 sum in the single-query kernel's grouping:
//            its WPH = 4 waves split the nt tiles into contiguous parts of ceil(nt / 4), each lane (key mod 64) adds its part's tiles in ascending order, skw_wave_sum_f64 folds
//            the lanes, the four parts add in ascending order.  An f64 sum of floats is not exact, so the grouping is part of the contract.  p = h2f(f2h(e * (float)(1 / tot))).
//   P.V      wave w owns channels 16 w .. 16 w + 15: O^T[channel][query] += V^T[channel][key] * p[query][key], one MFMA per four keys, 32-key blocks in skw_kperm order
//            (lane group g of element e holds key 4 e + g), so the chain per (channel, query) is key-ascending; V^T of keys past the row's count is replaced by zeros.
// Rows outside every sequence and query slots past nq in a sequence's last tile are not written.
#define SKW_XQ_SLAB (64 * 72)      // halves of one wave's K slab
__global__ __launch_bounds__(256, 1) void k_xattn_prefill_exact(const half_t* q, long ldq, const half_t* kbase, long k_slot_stride, long ldk, const half_t* vtbase, int n_ctx, int Tpad, int H,
                                                                half_t* out, long ldo, int f32_out, const int* row0, const int* nq, const int* slot, const int* slot_k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char xq_lds[];
    const int sq = blockIdx.z, h = blockIdx.y, qt = blockIdx.x;
    const int nqs = nq[sq];
    if (qt * 16 >= nqs) return;                  // uniform per workgroup
    const int r0 = row0[sq] + qt * 16, nqt = min(16, nqs - qt * 16), sl = slot[sq];
    if (slot_k) { const int nk = slot_k[sl]; if (nk > 0) n_ctx = min(nk, n_ctx); }      // per-clip audio context: the slot's key count; n_ctx and Tpad stay the strides
    const int nt = (n_ctx + 63) >> 6, SP = nt * 64 + 4;      // (+ 4: the 16 queries' rows start 4 banks apart, so the P.V reads of a lane group do not collide)
    float* pl = (float*)xq_lds;
    half_t* klds = (half_t*)(xq_lds + (size_t)16 * SP * 4);
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    // ---- scores
    const half_t* K = kbase + (long)sl * k_slot_stride + h * 64;
    float qf[16];
    {
        const half_t* qp = q + (long)(r0 + min(r16, nqt - 1)) * ldq + h * 64;      // query slots past nq repeat the last row (computed, never stored)
#pragma unroll
        for (int m = 0; m < 16; ++m) qf[m] = h2f(qp[4 * m + g]);
    }
    half_t* kl = klds + w * SKW_XQ_SLAB;
    const int lrow = lane >> 3, lseg = lane & 7;
    u32x4 kr[8];
    auto kload = [&](int t) {
#pragma unroll
        for (int i = 0; i < 8; ++i) kr[i] = *(const u32x4*)(K + (long)min(t * 64 + i * 8 + lrow, n_ctx - 1) * ldk + lseg * 8);
    };
    if (w < nt) kload(w);
    for (int t = w; t < nt; t += 4) {            // wave-uniform
#pragma unroll
        for (int i = 0; i < 8; ++i) *(u32x4*)(kl + (i * 8 + lrow) * 72 + lseg * 8) = kr[i];
        __builtin_amdgcn_wave_barrier();         // same wave, LDS in order: a compiler-level fence is all that is needed
        if (t + 4 < nt) kload(t + 4);
        f32x4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 16; ++m)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = MFMA16(h2f(kl[(s * 16 + r16) * 72 + 4 * m + g]), qf[m], acc[s]);      // S[key][query] += K[key][d] * q[query][d], d = 4 m + g
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 4; ++s) {            // D: lane (r16, g) holds keys 4 g .. 4 g + 3 of the sub-tile for query r16
            const int key0 = t * 64 + s * 16 + 4 * g; f32x4 v = acc[s];
#pragma unroll
            for (int r = 0; r < 4; ++r) if (key0 + r >= n_ctx) v[r] = -INFINITY;
            *(f32x4*)(pl + r16 * SP + key0) = v;
        }
    }
    // V^T ring: the first loads fly during the softmax
    __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(vtbase + ((long)sl * H + h) * 64 * Tpad), 0, (unsigned)(64 * Tpad * 2), 0x00020000);
    const unsigned vo = (unsigned)(((w * 16 + r16) * Tpad + g * 8) * 2);
    const int nkb = (n_ctx + 31) >> 5;
    constexpr int RD = 8;
    H8v ring[RD];
#pragma unroll
    for (int j = 0; j < RD; ++j) { ring[j].v = __builtin_amdgcn_raw_buffer_load_b128(rv, (j < nkb) ? vo + j * 64 : 0x7fffff00u, 0, 0); __builtin_amdgcn_sched_barrier(0); }
    __syncthreads();
    // ---- softmax, four queries per wave
    const int nth = (nt + 3) >> 2;
    for (int jq = 0; jq < 4; ++jq) {
        const int j = w * 4 + jq;
        if (j >= nqt) break;                     // wave-uniform
        float* pj = pl + j * SP;
        float lmax = -INFINITY;
        for (int t = 0; t < nt; ++t) lmax = fmaxf(lmax, pj[t * 64 + lane]);
        lmax = skw_wave_max_f32(lmax);
        double tot = 0.0;
        for (int part = 0; part < 4; ++part) {
            const int t_lo = part * nth, t_hi = min(nt, t_lo + nth);
            double lsum = 0.0;
            for (int t = t_lo; t < t_hi; ++t) { float e = skw_expf(pj[t * 64 + lane] - lmax); pj[t * 64 + lane] = e; lsum += (double)e; }   // exp(-inf) == 0 for masked keys
            lsum = skw_wave_sum_f64(lsum);
            tot = part == 0 ? lsum : tot + lsum;
        }
        const float inv = (float)(1.0 / tot);
        for (int t = 0; t < nt; ++t) pj[t * 64 + lane] = h2f(f2h(pj[t * 64 + lane] * inv));
    }
    __syncthreads();
    // ---- P.V
    f32x4 oacc = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* pq = pl + r16 * SP + g;
    for (int kb0 = 0; kb0 < nkb; kb0 += RD) {
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int kb = kb0 + j;
            if (kb < nkb) {                      // wave-uniform
                H8v vf = ring[j];
                const int nb = kb + RD;
                ring[j].v = __builtin_amdgcn_raw_buffer_load_b128(rv, (nb < nkb) ? vo + nb * 64 : 0x7fffff00u, 0, 0);
                // keys past the row's count in its last block: V^T there is an earlier, longer call's (or a don't-care encoder row's) — replaced by zeros, never multiplied by p = 0
                if (kb * 32 + 32 > n_ctx) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (kb * 32 + 4 * e + g >= n_ctx) vf.h[e] = f2h(0.0f);
                }
                float pe[8], xv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) { pe[e] = pq[kb * 32 + 4 * e]; xv[e] = h2f(vf.h[e]); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int e = 0; e < 8; ++e) oacc = MFMA16(xv[e], pe[e], oacc);      // O^T[c][query] += V^T[c][key] * p[query][key]
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // D: lane (r16, g) holds channels 16 w + 4 g .. + 3 of query r16
    if (r16 < nqt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) att_store(out, (long)(r0 + r16) * ldo, h * 64 + w * 16 + 4 * g + r, oacc[r], f32_out);
    }
}
size_t skw_xattn_prefill_exact_lds(int n_ctx) { return (size_t)16 * ((size_t)((n_ctx + 63) >> 6) * 64 + 4) * 4 + (size_t)4 * SKW_XQ_SLAB * 2; }
// the prompt pass's cross attention in the exact precision: n_seq sequences, sequence i's queries are rows row0[i] .. row0[i] + nq[i] of q [rows][d] (plain f16, already scaled), its
// K (rows [n_ctx][d]) / V^T ([H][64][Tpad], kperm) those of window slot slot[i]; out: f16 kperm rows, or f32 rows (f32_out) — what skw_dec_cross_attn_vt(pv16 = 0) writes for each row.
// False (nothing launched): a geometry the kernel does not hold (more than SKW_XATTN_MQ_MAX_CTX keys).
bool skw_xattn_prefill_exact(const half_t* q, const half_t* ck, const half_t* cvt, half_t* out, int n_seq, int nq_max, const int* row0, const int* nq, const int* slot,
                             int H, int d, int n_ctx, int Tpad, hipStream_t s, int f32_out, const int* slot_k) {
    if (n_seq < 1 || nq_max < 1 || n_ctx < 1 || n_ctx > SKW_XATTN_MQ_MAX_CTX) return false;
    const size_t lds = skw_xattn_prefill_exact_lds(n_ctx);
    if (lds > 64 * 1024) {      // more dynamic LDS than the default limit: raise it on this device (per device: several GPUs may run in one process)
        static std::atomic<bool> raised[64]; int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (!raised[dev].load(std::memory_order_acquire)) { hipFuncSetAttribute((const void*)k_xattn_prefill_exact, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        raised[dev].store(true, std::memory_order_release); }
    }
    hipLaunchKernelGGL(k_xattn_prefill_exact, dim3((nq_max + 15) / 16, H, n_seq), dim3(256), lds, s, q, (long)d, ck, (long)n_ctx * d, (long)d, cvt, n_ctx, Tpad, H, out, (long)d,
                       f32_out & 1, row0, nq, slot, slot_k);
    return true;
}

void skw_dec_self_attn(const half_t* q, const half_t* kc, const half_t* vc, const int* pos, int B, int H, int d, int n_text_ctx, half_t* out, const int* active,
    hipStream_t s, int f32_out, SkwQ8Out q8, const int* seq, int fastv, int ofrag) {
    if (fastv && skw_sw(SW_DEC_ATTN_FASTV) && !q8.q && !f32_out) { hipLaunchKernelGGL((k_dec_attn<7, true>), dim3((H + 3) / 4, B), dim3(256), 0, s, q, (long)d, kc, vc, (long)n_text_ctx * d, (long)d,
                       pos, (int)(sizeof(SkwSeqState) / 4), 0, H, out, (long)d, active, (int)(sizeof(SkwSeqState) / 4), f32_out, q8, seq, ofrag ? d : 0); return; }
    hipLaunchKernelGGL((k_dec_attn<7>), dim3((H + 3) / 4, B), dim3(256), 0, s, q, (long)d, kc, vc, (long)n_text_ctx * d, (long)d,
                       pos, (int)(sizeof(SkwSeqState) / 4), 0, H, out, (long)d, active, (int)(sizeof(SkwSeqState) / 4), f32_out, q8, seq, (ofrag && !q8.q && !f32_out) ? d : 0);
}
