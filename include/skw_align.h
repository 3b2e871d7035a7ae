/*
 * skw_align.h — the arithmetic CONTRACT of word timestamps: cross-attention weights of a set of alignment heads, normalised, median
 * filtered, averaged and warped against the token axis (openai-whisper's find_alignment, transformers' _extract_token_timestamps,
 * whisper.cpp's dtw_token_timestamps).  One statement that a sequential CPU loop (the *_ref evaluator at the end of this file) and
 * the HIP kernels (streamkit_amd/csrc/skw_kernels_align.hip) evaluate to the SAME BITS.  Built on include/skw_math.h: compile with
 * -ffp-contract=off; every fma below is written out.  The host side needs no HIP runtime.
 *
 * Input, per (clip, window): the teacher-forced sequence S = [sot, (language, task), no_timestamps] + text + [eot] run from position 0
 * with no [prev] context; text = the window's kept tokens below <|endoftext|>.  Row r of the alignment matrix is the decoder position
 * whose OUTPUT is text[r]; the last row's output is eot: N = len(text) + 1 rows, starting at the no_timestamps input position.
 *
 * Alignment heads: a set A of (layer, head) pairs as uint32_t head_mask[32], bit h of word l.
 *
 * Step 1  weights, for (l, h) in A, row r, key k < n_keys (the row's key count: audio_ctx, or n_audio_ctx when that is 0):
 *           s_k = sum_c q[c] * K[k][c]     an f32 fma chain from 0, c ascending over the head's 64 channels; q and K are the f16 values the
 *                                          decoder stores (the cross query after its GEMM, the slot's cross K), each already scaled by
 *                                          d_head^-0.25, widened to f32
 *           m   = max_k s_k                (no rounding: any order)
 *           e_k = skw_expf(s_k - m)        one f32 subtraction, then include/skw_math.h's expf
 *           Z   = f64 sum of the e_k, grouped as a wave evaluates it: 64 partial sums p[j] = sum over k = j, j + 64, j + 128 .. (ascending)
 *                 from 0.0, then the tree  for s in 32, 16, 8, 4, 2, 1: p[j] += p[j + s] for j < s;  Z = p[0]
 *           P_k = (float)((double)e_k / Z)
 * Step 2  crop to Kw = clamp(min(3000, n_len_org - seek) / 2, 1, n_keys) keys (skw_align_kw)
 * Step 3  normalise over the token axis, per (head, key), in f64, rows ascending, rounded once to f32:
 *           mean = (sum_r x_r) / N;  var = (sum_r (x_r - mean) * (x_r - mean)) / N;  z_r = (float)((x_r - mean) / sqrt(var));  var == 0: z_r = 0
 *         (transformers gives NaN for a zero-variance column: the one stated difference)
 * Step 4  median filter of odd width w (7) along keys, reflect padding (index -i -> i, Kw - 1 + i -> Kw - 1 - i); Kw <= w / 2: unfiltered
 *         (transformers' rule).  Pure selection: the element with at most w / 2 elements below it and more than w / 2 not above it.
 * Step 5  mean over heads in f64: the sum from 0.0 in (layer, head) ascending order, divided by |A|, rounded once to f32, then negated.
 * Step 6  DTW over the N x Kw matrix x:  cost[0][0] = 0, the rest of row 0 and column 0 +inf;  cost[i][j] = x[i-1][j-1] + min — one f32 add;
 *         with c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]: diagonal if c0 < c1 and c0 < c2, else up if c1 < c0 and c1 < c2, else left.
 *         Backtrace from (N, Kw) with trace[0][*] = left, trace[*][0] = up.
 * Step 7  jump[r] = the first key index the path visits in row r;  t0[r] = seek_cs + 2 * jump[r];  t1[r] = t0[r + 1], the eot row supplies the
 *         last text token's t1 (its own t1 is its t0).  Centiseconds from the clip's start.
 */
#ifndef SKW_ALIGN_H
#define SKW_ALIGN_H

#include <stdio.h>
#include <stdlib.h>
#include "skw_math.h"

#include "skw_align_params.h"       /* skw_align_params and the limits: all a caller of the engine needs */
#define SKW_ALIGN_DH 64             /* channels per head (every Whisper) */

/* ---- pieces both sides evaluate (host and device) ---- */
/* step 2 */
SKW_HD int skw_align_kw(int n_len_org, int seek, int n_keys) {
    int f = n_len_org - seek; if (f > 3000) f = 3000;
    int kw = f / 2; if (kw > n_keys) kw = n_keys; if (kw < 1) kw = 1;
    return kw;
}
/* step 3: one element, given the column's statistics (sd = sqrt(var)) */
SKW_HD float skw_align_z(float x, double mean, double var, double sd) { return var == 0.0 ? 0.0f : (float)(((double)x - mean) / sd); }
/* step 4: reflect padding of index i into [0, n) (|overhang| < n) */
SKW_HD int skw_align_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
/* step 4: the median of w (odd) values by counting — no arithmetic, so no rounding */
SKW_HD float skw_align_median(const float* v, int w) {
    const int half = w / 2;
    for (int a = 0; a < w; ++a) {
        int lt = 0, le = 0;
        for (int b = 0; b < w; ++b) { lt += v[b] < v[a]; le += v[b] <= v[a]; }
        if (lt <= half && le > half) return v[a];
    }
    return v[half];      /* unreachable for ordered values (NaNs never reach this step) */
}
/* step 4 at key k of one row z [Kw] */
SKW_HD float skw_align_median_at(const float* z, int Kw, int k, int width) {
    const int half = width / 2;
    if (Kw <= half) return z[k];
    float v[SKW_ALIGN_MEDIAN_MAX];
    for (int a = 0; a < width; ++a) v[a] = z[skw_align_reflect(k - half + a, Kw)];
    return skw_align_median(v, width);
}
/* step 6: the tie rule; returns the chosen predecessor's cost, *t = 0 diagonal, 1 up, 2 left */
SKW_HD float skw_align_pick(float c0, float c1, float c2, int* t) {
    if (c0 < c1 && c0 < c2) { *t = 0; return c0; }
    if (c1 < c0 && c1 < c2) { *t = 1; return c1; }
    *t = 2; return c2;
}

/* ---- the alignment heads ---- */
/* all heads of the top n_layers decoder layers (whisper.cpp's N_TOP_MOST; n_layers = n_text_layer / 2 is openai's default for a model that names no heads) */
SKW_HD void skw_align_heads_top(int n_text_layer, int n_text_head, int n_layers, uint32_t* mask /* [32] */) {
    for (int l = 0; l < SKW_ALIGN_MAX_LAYERS; ++l) mask[l] = 0;
    if (n_layers > n_text_layer) n_layers = n_text_layer;
    for (int l = n_text_layer - n_layers; l < n_text_layer && l < SKW_ALIGN_MAX_LAYERS; ++l)
        if (l >= 0) mask[l] = n_text_head >= 32 ? 0xffffffffu : ((1u << n_text_head) - 1u);
}
SKW_HD int skw_align_popcount(uint32_t w) { int n = 0; while (w) { w &= w - 1; ++n; } return n; }
SKW_HD int skw_align_n_heads(const uint32_t* mask) { int n = 0; for (int l = 0; l < SKW_ALIGN_MAX_LAYERS; ++l) n += skw_align_popcount(mask[l]); return n; }

/* A clip's record, checked before anything runs: 1 = good (or alignment not asked for); 0 = bad, err names the clip.
 * Bad: an empty mask, a head or layer outside the model, an even, non-positive or too wide median_width. */
static inline int skw_align_check_params(const skw_align_params* p, int n_text_layer, int n_text_head, int clip, char* err, size_t errlen) {
    if (!p || !p->enabled) return 1;
    if (p->median_width < 1 || (p->median_width & 1) == 0 || p->median_width > SKW_ALIGN_MEDIAN_MAX) {
        snprintf(err, errlen, "clip %d: alignment median_width %d is not an odd number in [1, %d]", clip, (int)p->median_width, SKW_ALIGN_MEDIAN_MAX); return 0; }
    int n = 0;
    for (int l = 0; l < SKW_ALIGN_MAX_LAYERS; ++l) {
        if (!p->head_mask[l]) continue;
        if (l >= n_text_layer) { snprintf(err, errlen, "clip %d: alignment head in layer %d outside the model's %d decoder layers", clip, l, n_text_layer); return 0; }
        if (n_text_head < 32 && (p->head_mask[l] >> n_text_head)) {
            int h = 31; while (!((p->head_mask[l] >> h) & 1u)) --h;
            snprintf(err, errlen, "clip %d: alignment head %d of layer %d outside the model's %d heads", clip, h, l, n_text_head); return 0; }
        n += skw_align_popcount(p->head_mask[l]);
    }
    if (!n) { snprintf(err, errlen, "clip %d: alignment asked for with an empty head mask", clip); return 0; }
    return 1;
}

/* ---- the evaluator: sequential host loops over the statement above ---- */
/* step 1 for one (row, head): q [64] f16 bits; key k's 64 channels at K + k * k_stride (f16 bits); P [n_keys] out; e: [n_keys] scratch */
static inline void skw_align_weights_ref(const uint16_t* q, const uint16_t* K, long k_stride, int n_keys, float* P, float* e) {
    float m = 0.0f;
    for (int k = 0; k < n_keys; ++k) {
        float s = 0.0f;
        for (int c = 0; c < SKW_ALIGN_DH; ++c) s = __builtin_fmaf(skw_f16_to_f32(q[c]), skw_f16_to_f32(K[(long)k * k_stride + c]), s);
        e[k] = s;
        if (k == 0 || s > m) m = s;
    }
    double p[64];
    for (int j = 0; j < 64; ++j) p[j] = 0.0;
    for (int k = 0; k < n_keys; ++k) { e[k] = skw_expf(e[k] - m); p[k & 63] += (double)e[k]; }
    for (int s = 32; s >= 1; s >>= 1) for (int j = 0; j < s; ++j) p[j] += p[j + s];
    for (int k = 0; k < n_keys; ++k) P[k] = (float)((double)e[k] / p[0]);
}
/* steps 3-4 for H heads (in ascending order), added into the cells' f64 accumulators acc [N][Kw] (step 5's running sum: zero it before the first head of the
 * first layer).  P: head h, row r, key k at P[h * head_stride + r * row_stride + k]; only keys < Kw are read (step 2).  Returns 0, or -1 without memory. */
static inline int skw_align_reduce_ref(const float* P, long head_stride, long row_stride, int H, int N, int Kw, int width, double* acc) {
    float* z = (float*)malloc(sizeof(float) * (size_t)N * Kw);
    if (!z) return -1;
    for (int h = 0; h < H; ++h) {
        const float* Ph = P + h * head_stride;
        for (int k = 0; k < Kw; ++k) {
            double sum = 0.0, sq = 0.0;
            for (int r = 0; r < N; ++r) sum += (double)Ph[r * row_stride + k];
            const double mean = sum / (double)N;
            for (int r = 0; r < N; ++r) { const double d = (double)Ph[r * row_stride + k] - mean; sq += d * d; }
            const double var = sq / (double)N, sd = sqrt(var);
            for (int r = 0; r < N; ++r) z[(size_t)r * Kw + k] = skw_align_z(Ph[r * row_stride + k], mean, var, sd);
        }
        for (int r = 0; r < N; ++r) for (int k = 0; k < Kw; ++k) acc[(size_t)r * Kw + k] += (double)skw_align_median_at(z + (size_t)r * Kw, Kw, k, width);
    }
    free(z);
    return 0;
}
/* step 5's end: x = -(float)(acc / n_heads) */
static inline void skw_align_finish_ref(const double* acc, int n_heads, long cells, float* x) {
    for (long i = 0; i < cells; ++i) x[i] = -(float)(acc[i] / (double)n_heads);
}
/* steps 6-7: x [N][Kw] -> jump [N]; when path_i / path_j are non-null they receive the path in forward order ((row, key) pairs, at most N + Kw of them) and
 * *n_path its length.  Returns 0, or -1 without memory. */
static inline int skw_align_dtw_ref(const float* x, int N, int Kw, int32_t* jump, int32_t* path_i, int32_t* path_j, int32_t* n_path) {
    const float inf = skw_bits_f32(0x7f800000u);
    float* cost = (float*)malloc(sizeof(float) * 2 * (size_t)(N + 1));      /* two columns: j - 1 and j */
    uint8_t* trace = (uint8_t*)malloc((size_t)(N + 1) * (Kw + 1));
    if (!cost || !trace) { free(cost); free(trace); return -1; }
    float *prev = cost, *cur = cost + (N + 1);
    for (int i = 0; i <= N; ++i) prev[i] = inf;
    prev[0] = 0.0f;
    for (int j = 1; j <= Kw; ++j) {
        cur[0] = inf;
        for (int i = 1; i <= N; ++i) {
            int t; const float c = skw_align_pick(prev[i - 1], cur[i - 1], prev[i], &t);
            cur[i] = x[(size_t)(i - 1) * Kw + (j - 1)] + c;
            trace[(size_t)i * (Kw + 1) + j] = (uint8_t)t;
        }
        float* sw = prev; prev = cur; cur = sw;
    }
    for (int j = 0; j <= Kw; ++j) trace[j] = 2;
    for (int i = 0; i <= N; ++i) trace[(size_t)i * (Kw + 1)] = 1;
    int i = N, j = Kw, n = 0;
    while (i > 0 || j > 0) {
        if (i > 0) jump[i - 1] = j - 1;      /* walking backwards: the last store into a row is the path's first visit of it */
        if (path_i) { path_i[n] = i - 1; path_j[n] = j - 1; }
        ++n;
        const int t = trace[(size_t)i * (Kw + 1) + j];
        if (t == 0) { --i; --j; } else if (t == 1) --i; else --j;
    }
    if (path_i) for (int a = 0, b = n - 1; a < b; ++a, --b) {
        int32_t s = path_i[a]; path_i[a] = path_i[b]; path_i[b] = s; s = path_j[a]; path_j[a] = path_j[b]; path_j[b] = s; }
    if (n_path) *n_path = n;
    free(cost); free(trace);
    return 0;
}
/* step 7 */
SKW_HD void skw_align_times(const int32_t* jump, int N, int seek_cs, int32_t* t0, int32_t* t1) {
    for (int r = 0; r < N; ++r) t0[r] = seek_cs + 2 * jump[r];
    for (int r = 0; r < N; ++r) t1[r] = r + 1 < N ? t0[r + 1] : t0[r];
}

#endif /* SKW_ALIGN_H */
