// skw_kernels_mel.hip — the log-mel front end for gfx950 (CDNA4).
// Compile with -ffp-contract=off: every fused multiply-add in here is explicit (see include/skw_math.h).
//
// What each kernel restates (whisper.cpp routine):
//   k_mel_*            log_mel_spectrogram + worker (K1)
#include "skw_dev_common.h"

// ------------------------------------------------------------------ log-mel front end (K1)
// one 128-thread block per frame; restates whisper.cpp fft()/dft() operation by operation (f32, no contraction)
__global__ __launch_bounds__(128) void k_mel_frames(const float* pcm, const long* pcm_off, const int* n_samples, const int* n_len, int n_len_max,
                                                    SkwMelTables t, float* mel_raw) {
    __shared__ float x[400];
    __shared__ float bufA[800], bufB[800];
    __shared__ float cs_t[400], sn_t[400];           // twiddles: 25 x 400 + 4 x 200 reads per frame, served from LDS instead of L1/L2
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int ns_raw = n_samples[b], nl = n_len[b];
    if (i >= nl) return;
    float* outp = mel_raw + ((long)b * n_len_max + i) * t.n_mel;
    const int ns = ns_raw + 200;
    int n_calc = ns / 160 + 1; if (n_calc > nl) n_calc = nl;
    if (i >= n_calc) { if (tid < t.n_mel) outp[tid] = (float)log10(1e-10); return; }
    for (int j = tid; j < 400; j += 128) { cs_t[j] = t.cos_t[j]; sn_t[j] = t.sin_t[j]; }
    const float* p = pcm + pcm_off[b];
    const int offset = i * 160;
    int lim = ns - offset; if (lim > 400) lim = 400;
    for (int j = tid; j < 400; j += 128) {
        float v = 0.0f;
        if (j < lim) {
            int pp = offset + j; float sm;
            if (pp < 200) { int q = 200 - pp; sm = (q < ns_raw) ? p[q] : 0.0f; }
            else { int q = pp - 200; sm = (q < ns_raw) ? p[q] : 0.0f; }
            v = t.hann[j] * sm;
        }
        x[j] = v;
    }
    __syncthreads();
    // 16 leaf DFTs of length 25: leaf o holds x[o + 16 n].  A thread owns one output bin k of up to four leaves (o = og, og + 5, og + 10, og + 15):
    // the twiddle of term n is the same for all of them, so it is fetched (and its index advanced) once per term instead of once per output —
    // each output is still its own n-ascending chain of separately rounded products and sums.
    if (tid < 125) {
        const int k = tid % 25, og = tid / 25;
        float re[4] = {0.0f, 0.0f, 0.0f, 0.0f}, im[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int step = (k * 16) % 400; int idx = 0;          // (k * n * 16) % 400 without a division per term
        const bool four = og == 0;                             // leaf 15 exists only for og = 0
        for (int n = 0; n < 25; ++n) {
            const float c = cs_t[idx], sn = sn_t[idx];
#pragma unroll
            for (int j = 0; j < 3; ++j) { const float xin = x[og + 5 * j + 16 * n]; re[j] += xin * c; im[j] -= xin * sn; }
            if (four) { const float xin = x[15 + 16 * n]; re[3] += xin * c; im[3] -= xin * sn; }
            idx += step; if (idx >= 400) idx -= 400;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) { const int o = og + 5 * j; bufA[2 * (o * 25 + k)] = re[j]; bufA[2 * (o * 25 + k) + 1] = im[j]; }
        if (four) { bufA[2 * (15 * 25 + k)] = re[3]; bufA[2 * (15 * 25 + k) + 1] = im[3]; }
    }
    __syncthreads();
    float* src = bufA; float* dst = bufB;
    for (int N = 50; N <= 400; N <<= 1) {
        const int half_n = N >> 1, groups = 400 / N, step = 400 / N;
        for (int u = tid; u < 200; u += 128) {
            int gi = u / half_n, k = u % half_n;
            int idx = k * step;
            float re = cs_t[idx], im = -sn_t[idx];
            const float* ev = src + 2 * (gi * half_n + k); const float* od = src + 2 * ((gi + groups) * half_n + k);
            float er = ev[0], ei = ev[1], orr = od[0], oi = od[1];
            float* o0 = dst + 2 * (gi * N + k); float* o1 = dst + 2 * (gi * N + k + half_n);
            o0[0] = (er + re * orr) - im * oi;
            o0[1] = (ei + re * oi) + im * orr;
            o1[0] = (er - re * orr) + im * oi;
            o1[1] = (ei - re * oi) - im * orr;
        }
        __syncthreads();
        float* tmp = src; src = dst; dst = tmp;
    }
    // power spectrum into x[0..200]
    for (int j = tid; j < 201; j += 128) { float re = src[2 * j], im = src[2 * j + 1]; x[j] = re * re + im * im; }
    __syncthreads();
    if (tid < t.n_mel) {
        const float* fl = t.filters + (long)tid * t.n_fft_bins;
        // whisper.cpp's loop runs over all bins in groups of four; a group whose four taps are all zero adds +0.0 to the f64 sum, so
        // only the groups [g_lo, g_hi) that hold this filter's non-zero taps are visited (same groups, same order, same bits)
        double sum = 0.0; int k = t.grp_lo ? 4 * t.grp_lo[tid] : 0;
        const int k_end = t.grp_hi ? min(4 * t.grp_hi[tid], t.n_fft_bins - 3) : t.n_fft_bins - 3;
        for (; k < k_end; k += 4) {
            float s4 = x[k] * fl[k] + x[k + 1] * fl[k + 1] + x[k + 2] * fl[k + 2] + x[k + 3] * fl[k + 3];
            sum += (double)s4;
        }
        for (k = (t.n_fft_bins - 3 > 0) ? ((t.n_fft_bins - 3 + 3) / 4) * 4 : 0; k < t.n_fft_bins; ++k) sum += (double)(x[k] * fl[k]);
        sum = log10(sum > 1e-10 ? sum : 1e-10);
        outp[tid] = (float)sum;
    }
}
void skw_mel_frames(const float* pcm, const long* pcm_off, const int* n_samples, const int* n_len, int B, int n_len_max, SkwMelTables t, float* mel_raw, hipStream_t s) {
    hipLaunchKernelGGL(k_mel_frames, dim3(n_len_max, B), dim3(128), 0, s, pcm, pcm_off, n_samples, n_len, n_len_max, t, mel_raw);
}

__device__ __forceinline__ unsigned f2ord(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__global__ void k_mel_max(const float* mel, const int* n_len, int n_len_max, int n_mel, unsigned* clip_max_ord) {
    const int b = blockIdx.y; const long n = (long)n_len[b] * n_mel; const float* p = mel + (long)b * n_len_max * n_mel;
    float m = -INFINITY;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) m = fmaxf(m, p[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&clip_max_ord[b], f2ord(m));
}
__global__ void k_mel_norm(float* mel, const int* n_len, int n_len_max, int n_mel, const unsigned* clip_max_ord) {
    const int b = blockIdx.y; const long n = (long)n_len[b] * n_mel; float* p = mel + (long)b * n_len_max * n_mel;
    double mmax = (double)ord2f(clip_max_ord[b]) - 8.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = p[i]; if ((double)v < mmax) v = (float)mmax;
        p[i] = (float)(((double)v + 4.0) / 4.0);
    }
}
void skw_mel_normalize(float* mel, const int* n_len, int B, int n_len_max, int n_mel, float* clip_max, hipStream_t s) {
    hipMemsetAsync(clip_max, 0, sizeof(unsigned) * B, s);
    hipLaunchKernelGGL(k_mel_max, dim3(64, B), dim3(256), 0, s, mel, n_len, n_len_max, n_mel, (unsigned*)clip_max);
    hipLaunchKernelGGL(k_mel_norm, dim3(64, B), dim3(256), 0, s, mel, n_len, n_len_max, n_mel, (const unsigned*)clip_max);
}
// conv1 im2col: out[(bw*T + t)][kperm(k)], k = tap*n_mel + c (k < 3*n_mel), zero padded to k_pad (256 for 80 bands, 384 for large-v3's 128: the width of the conv1 weight image)
__global__ void k_mel_im2col(const float* mel, const int* clip_idx, const int* seek, const int* n_len, int n_len_max, int n_mel, int T, int k_pad, half_t* out, const int* slot_k) {
    const int bw = blockIdx.y, t = blockIdx.x;   // 256 threads
    const int clip = clip_idx[bw], sk = seek[bw], nl = n_len[clip];
    const int lim = slot_k ? min(T, 2 * slot_k[bw]) : T;      // the slot's own window: frames past 2 K read as zero (conv1 output 2 K - 1 reads frame 2 K)
    for (int k = threadIdx.x; k < k_pad; k += blockDim.x) {
        float v = 0.0f;
        if (k < 3 * n_mel) {
            int tap = k / n_mel, c = k % n_mel; int tt = t - 1 + tap; int fr = sk + tt;
            if (tt >= 0 && tt < lim && fr < nl) v = mel[((long)clip * n_len_max + fr) * n_mel + c];
        }
        out[((long)bw * T + t) * k_pad + skw_kperm(k)] = f2h(v);
    }
}
void skw_mel_im2col(const float* mel, const int* clip_idx, const int* seek, const int* n_len, int Bw, int n_len_max, int n_mel, int T, int k_pad, half_t* out, hipStream_t s,
                    const int* slot_k) {
    hipLaunchKernelGGL(k_mel_im2col, dim3(T, Bw), dim3(256), 0, s, mel, clip_idx, seek, n_len, n_len_max, n_mel, T, k_pad, out, slot_k);
}
