/*
 * skw_kv8.h — the CONTRACT of the decode step's cross attention over 8-bit cross K / V (cross_kv = q8_0, f16_mfma precision only): the storage format, the
 * offset functions that state the image's byte order once, and a sequential CPU evaluator (the *_ref functions at the end) of the two parts that are owed
 * bit for bit — the quantiser and the scores.  The HIP side is streamkit_amd/csrc/skw_kernels_kv8.hip.  Built on include/skw_math.h and
 * include/skw_ggml_quant.h: plain C, host/device, no libm; compile with -ffp-contract=off.
 *
 * STORAGE.  Both operands are ggml q8_0 along their contraction axis (skw_ggml_quantize_q8_block on the stored f16 values widened to f32: int8 qs[32], d rounded
 * to f16 as that function returns it):
 *   K    per (slot, head, key): the 64 d-values of the stored f16 K row are two blocks, d 0 .. 31 and 32 .. 63
 *   V^T  per (slot, head, channel): the keys in logical order, cut into the blocks 32 j .. 32 j + 31 (the blocks skw_kperm and skw_vtfrag_off use)
 * Pad keys: a key at or past the slot's key count (n_audio_ctx, or the slot's audio_ctx) is ZERO for the quantiser — not part of amax, qs = 0; the K row of a
 * pad key inside the slot's last 32-key block has d = 0 and qs = 0.  The quantiser decides by the count, never by the value (the f16 pads may be NaNs).  Blocks
 * wholly past the count are not written; nothing reads them.
 *
 * THE IMAGE.  One image per layer holds K and V^T together: per (slot, head) Tpad / 32 RECORDS of SKW_KV8_REC = 4352 bytes, one per 32-key block j, so that the
 * four waves of a head — taking every fourth block — walk one sequential stream, a block's scales travelling with its bytes:
 *   [   0, 2048)  K qs    two key tiles t of 1 KiB = [lane i + 16 g][d half kk][8 bytes]: lane row i holds key 32 j + 16 t + 4 (i & 3) + (i >> 2) (the order in which
 *                         the score MFMA's accumulators come out in V^T's key order, as skw_kfrag_off), the bytes d = 32 kk + 8 g .. + 7
 *   [2048, 4096)  V^T qs  two channel-tile pairs v of 1 KiB = [lane i + 16 g][u][8 bytes]: channel 16 (2 v + u) + i, byte e = key 32 j + 4 e + g (kperm order)
 *   [4096, 4352)  scales  64 dwords [g][16] of two f16 each: dword 16 g + e (e < 8) = (d of K block d 0 .. 31, d of K block d 32 .. 63) of key 32 j + 4 e + g;
 *                         dword 16 g + 8 + 2 ct + p = d of V^T channels 16 ct + 4 g + 2 p and + 1 — what lane group g of the kernel's accumulators needs
 * The kernel reads a record with four 16-byte loads per lane (one contiguous KiB each) and one 4-byte load (the 256 B of scales, the tail of the same run).
 * 1.0625 bytes per element: H * (Tpad / 32) * 4352 bytes per slot and layer.
 *
 * SCORES.  The query row of a (row, head) is the f16 q the kernel is handed (scale folded in), quantised the same way: two q8_0 blocks over d 0 .. 31 and 32 .. 63.
 * The score of a key is ggml's vec_dot_q8_0_q8_0 — skw_ggml_block_dot form 2 on block 0 then block 1, from 0.0f:
 *     s = (0 + (dk0 * dq0) * (float)i0) + (dk1 * dq1) * (float)i1          i0, i1 exact int32 dots; every product and sum rounded to f32, nothing contracted
 * skw_kv8_scores_ref restates it; the kernel is held to it bit for bit (raw mode).
 *
 * SOFTMAX AND P.V follow the f16_mfma rules and owe no summation order: a running maximum per wave, p = exp2((s - m) log2 e) rounded to f16, the normaliser the
 * sum of the rounded values; V's int8 values widened to f16 (exact); a 32-key block of P.V is one f16 MFMA per channel tile into a fresh accumulator, then the
 * block's scale in f32: o[c] = fma(dv[c][block], blocksum[c], o[c]); one f16 rounding of the output.  tests/kv8_ref_lib.py derives the bound.
 */
#ifndef SKW_KV8_H
#define SKW_KV8_H

#include <stdint.h>
#include "skw_math.h"
#include "skw_ggml_quant.h"

#define SKW_KV8_REC 4352            /* bytes per (slot, head, 32-key block) */
#define SKW_KV8_SCALES 4096         /* the scales' offset inside a record */

/* ---- the layout, in bytes from the image's start.  feat = head * 64 + (d | channel) ---- */
SKW_HD long skw_kv8_slot_bytes(int H, int Tpad) { return (long)H * (Tpad >> 5) * SKW_KV8_REC; }
SKW_HD long skw_kv8_rec_off(int slot, int H, int Tpad, int head, int block) { return (((long)slot * H + head) * (Tpad >> 5) + block) * SKW_KV8_REC; }
/* the int8 of K[key][feat] */
SKW_HD long skw_kv8_kq_off(int slot, int H, int Tpad, int key, int feat) {
    const int dd = feat & 63, r = key & 15, i = 4 * (r & 3) + (r >> 2), g = (dd >> 3) & 3;
    return skw_kv8_rec_off(slot, H, Tpad, feat >> 6, key >> 5) + ((key >> 4) & 1) * 1024 + (i + 16 * g) * 16 + (dd >> 5) * 8 + (dd & 7);
}
/* the f16 scale of K[key]'s block holding feat */
SKW_HD long skw_kv8_kd_off(int slot, int H, int Tpad, int key, int feat) {
    const int kl = key & 31;
    return skw_kv8_rec_off(slot, H, Tpad, feat >> 6, key >> 5) + SKW_KV8_SCALES + (16 * (kl & 3) + (kl >> 2)) * 4 + ((feat >> 5) & 1) * 2;
}
/* the int8 of V[key][feat] */
SKW_HD long skw_kv8_vq_off(int slot, int H, int Tpad, int feat, int key) {
    const int c = feat & 63, ct = c >> 4, kl = key & 31;
    return skw_kv8_rec_off(slot, H, Tpad, feat >> 6, key >> 5) + 2048 + (ct >> 1) * 1024 + ((c & 15) + 16 * (kl & 3)) * 16 + (ct & 1) * 8 + (kl >> 2);
}
/* the f16 scale of channel feat's block holding key */
SKW_HD long skw_kv8_vd_off(int slot, int H, int Tpad, int feat, int key) {
    const int c = feat & 63;
    return skw_kv8_rec_off(slot, H, Tpad, feat >> 6, key >> 5) + SKW_KV8_SCALES + (16 * ((c >> 2) & 3) + 8 + 2 * (c >> 4) + ((c >> 1) & 1)) * 4 + (c & 1) * 2;
}

/* ---- pieces both sides evaluate ---- */
/* one block of 32 f16 bit patterns, element j counted only when live[j] (a pad is zero whatever it holds) -> qs, the scale's f16 bit pattern */
SKW_HD uint16_t skw_kv8_quantize_block(const uint16_t* x16, const int* live, int8_t* qs) {
    float x[32], d, s;
    for (int j = 0; j < 32; ++j) x[j] = live[j] ? skw_f16_to_f32(x16[j]) : 0.0f;
    skw_ggml_quantize_q8_block(x, qs, &d, &s);
    return skw_f32_to_f16(d);
}
/* the score chain above */
SKW_HD float skw_kv8_score(float dk0, float dq0, int i0, float dk1, float dq1, int i1) {
    float s = skw_ggml_block_dot(2, 0.0f, i0, dk0, 0.0f, dq0, 0.0f);
    return skw_ggml_block_dot(2, s, i1, dk1, 0.0f, dq1, 0.0f);
}

/* ---- the sequential evaluator (host) ---- */
/* One slot's image from its K / V in natural order ([n_ctx][H * 64] f16 bit patterns; rows at or past `count` are never read).  img: the whole image (slot picks
 * the records); records of blocks below ceil(count / 32) are written in full, the others left alone. */
static inline void skw_kv8_quantize_ref(const uint16_t* K, const uint16_t* V, int H, int n_ctx, int Tpad, int slot, int count, uint8_t* img) {
    const int d = H * 64;
    if (count > n_ctx) count = n_ctx;
    for (int h = 0; h < H; ++h) for (int j = 0; j * 32 < count; ++j) {
        for (int kl = 0; kl < 32; ++kl) for (int kk = 0; kk < 2; ++kk) {
            const int key = 32 * j + kl, f0 = h * 64 + 32 * kk; uint16_t x[32]; int live[32]; int8_t qs[32];
            for (int e = 0; e < 32; ++e) { live[e] = key < count; x[e] = live[e] ? K[(size_t)key * d + f0 + e] : 0; }
            const uint16_t dh = skw_kv8_quantize_block(x, live, qs);
            for (int e = 0; e < 32; ++e) img[skw_kv8_kq_off(slot, H, Tpad, key, f0 + e)] = (uint8_t)qs[e];
            memcpy(img + skw_kv8_kd_off(slot, H, Tpad, key, f0), &dh, 2);
        }
        for (int c = 0; c < 64; ++c) {
            const int f = h * 64 + c; uint16_t x[32]; int live[32]; int8_t qs[32];
            for (int e = 0; e < 32; ++e) { const int key = 32 * j + e; live[e] = key < count; x[e] = live[e] ? V[(size_t)key * d + f] : 0; }
            const uint16_t dh = skw_kv8_quantize_block(x, live, qs);
            for (int e = 0; e < 32; ++e) img[skw_kv8_vq_off(slot, H, Tpad, f, 32 * j + e)] = (uint8_t)qs[e];
            memcpy(img + skw_kv8_vd_off(slot, H, Tpad, f, 32 * j), &dh, 2);
        }
    }
}
/* The contract's scores of one (row, head): q [64] f16 bit patterns of that head, keys [0, count) of `slot` -> s [count] */
static inline void skw_kv8_scores_ref(const uint16_t* q, const uint8_t* img, int H, int Tpad, int slot, int head, int count, float* s) {
    int8_t qq[2][32]; float dq[2]; int live[32];
    for (int e = 0; e < 32; ++e) live[e] = 1;
    for (int kk = 0; kk < 2; ++kk) dq[kk] = skw_f16_to_f32(skw_kv8_quantize_block(q + 32 * kk, live, qq[kk]));
    for (int key = 0; key < count; ++key) {
        int idot[2]; float dk[2];
        for (int kk = 0; kk < 2; ++kk) {
            const int f0 = head * 64 + 32 * kk; uint16_t dh; int acc = 0;
            for (int e = 0; e < 32; ++e) acc += (int)(int8_t)img[skw_kv8_kq_off(slot, H, Tpad, key, f0 + e)] * (int)qq[kk][e];
            memcpy(&dh, img + skw_kv8_kd_off(slot, H, Tpad, key, f0), 2);
            idot[kk] = acc; dk[kk] = skw_f16_to_f32(dh);
        }
        s[key] = skw_kv8_score(dk[0], dq[0], idot[0], dk[1], dq[1], idot[1]);
    }
}
#endif
