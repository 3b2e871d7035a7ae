// skw_kernels_resample.hip — the resampler's kernels for gfx950 (CDNA4): rubato's linear walk and the polyphase windowed sinc.
// Compile with -ffp-contract=off: every fused multiply-add in here is explicit (see include/skw_math.h).
#include <atomic>
#include "skw_dev_common.h"

// ------------------------------------------------------------------ R1: audio::resampler arithmetic (rubato FastFixedIn, Linear)
// Restates /root/reference/crates/nodes/src/audio/filters/resampler.rs:231-244, 384-514 (rubato 0.16.2 asynchro_fast.rs):
// per chunk: idx starts at last_index, `while idx < end_idx { idx += t_ratio; out = (1-frac)*y[floor idx] + frac*y[floor idx + 1] }`,
// last_index = idx - chunk.  The index recurrence is a sequential f64 accumulation whose roundings decide `frac`, across the whole
// stream.  It is parallelised without giving that up:
//   k_resample_starts* one lane proposes every chunk's start index, output count and output offset: first by a closed form (one
//                      division per chunk; right whenever every addition of the walk is exact), and if that fails its check by
//                      stepping whole binades of the f64 index at a time (exact integer arithmetic per binade, ties included);
//   k_resample_walk    one lane PER CHUNK walks its chunk with the real f64 recurrence from the proposed start, writes
//                      (sample index, frac) for its outputs and checks that it produced the proposed count and hands the next chunk
//                      exactly the proposed start — by induction the proposal then IS the sequential walk, bit for bit;
//   k_resample_scan    the original single-lane walk, which only runs when a check failed or the proposal met a rounding tie.
// The interpolation (k_resample_lerp) is data parallel.
// The proposal must reproduce n dependent f64 additions exactly.  Inside one binade [2^e, 2^(e+1)) every x is a multiple of
// ulp_e = 2^(e-52), so fl(x + t) = x + RN_e(t), t rounded to that grid: a whole binade is one integer multiply-add.  When t sits
// exactly halfway between two grid points (44.1 kHz sources: t = 441/160 has one bit below the grid of [4, 8)) round-to-even picks
// the step that makes the result even: from an odd x that is one real addition, after which x is even and the step is the even
// neighbour for the rest of the binade.  A chunk crosses ~10 binades (index -10 .. 950), each crossing is one real f64 addition;
// 1500 chunks cost one lane well under a millisecond instead of ~30 ms.  (tests/test_cpu_frontend.py checks the same stepping against the sequential walk for 11 source
// rates x 3000 chunks on the CPU; on the device k_resample_walk checks every launch.)
__device__ __forceinline__ long long ceil_div_pos(long long a, long long b) {      // a > 0, b > 0, a < 2^62: no 64-bit integer division (software, ~1 us for one lane)
    long long q = (long long)((double)a / (double)b);
    while (q * b < a) ++q;
    while ((q - 1) * b >= a) --q;
    return q;
}
// first proposal: the closed form n = ceil((end - s) / t), s' = (s + n t) - chunk — one division per chunk, exact whenever every
// addition of the walk is exact (48 / 32 / 96 kHz -> 16 kHz: t is a small integer), which k_resample_walk then proves
__global__ void k_resample_starts_simple(double last_index, double t_ratio, int chunk, int n_chunks, double* start, int* count, int* offset, int* flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double end_idx = (double)(chunk - 9) - ceil(t_ratio);
    double s = last_index; int off = 0;
    for (int c = 0; c < n_chunks; ++c) {
        int n = 0;
        if (s < end_idx) { n = (int)ceil((end_idx - s) / t_ratio); if (n < 1) n = 1; while (n > 1 && s + (double)(n - 1) * t_ratio >= end_idx) --n; while (s + (double)n * t_ratio < end_idx) ++n; }
        start[c] = s; count[c] = n; offset[c] = off; off += n;
        s = (s + (double)n * t_ratio) - (double)chunk;
    }
    start[n_chunks] = s; offset[n_chunks] = off; *flag = 0;
}
// second proposal (runs only when the first one failed its check: *flag != 0)
__global__ void k_resample_starts(double last_index, double t_ratio, int chunk, int n_chunks, double* start, int* count, int* offset, int* flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!*flag) return;
    const double end_idx = (double)(chunk - 9) - ceil(t_ratio);
    double s = last_index; int off = 0;
    for (int c = 0; c < n_chunks; ++c) {
        double x = s; int n = 0;
        while (x < end_idx && x < 4.0) { x += t_ratio; n++; }               // negative / small indices: the few plain additions the walk makes too
        while (x < end_idx) {
            const long long bits = __double_as_longlong(x);
            const int e = (int)((bits >> 52) & 0x7ff) - 1023;                 // x in [2^e, 2^(e+1)), e >= 2
            long long xi = (bits & 0xfffffffffffffLL) | (1LL << 52);          // x / ulp_e
            const double ts = ldexp(t_ratio, 52 - e);                         // t / ulp_e, exact
            const double fl = floor(ts), fr = ts - fl;
            long long ti = (long long)fl;
            if (fr == 0.5) {
                if (xi & 1) { x = x + t_ratio; n++; continue; }               // odd x on a tie: the hardware rounds this one
                ti += ti & 1;                                                 // the even neighbour
            } else if (fr > 0.5) ti += 1;
            if (ti < 1) { x = x + t_ratio; n++; continue; }                   // (degenerate ratios: plain additions)
            const long long Bi = 1LL << 53, endi = (long long)ldexp(end_idx, 52 - e);
            const long long in_binade = ceil_div_pos(Bi - xi, ti) - 1;        // additions whose result stays below 2^(e+1)
            const long long to_end = xi < endi ? ceil_div_pos(endi - xi, ti) : 0;   // additions the loop condition still allows
            const long long k = in_binade < to_end ? in_binade : to_end;
            xi += k * ti; n += (int)k; x = ldexp((double)xi, e - 52);
            if (k == to_end) break;
            x = x + t_ratio; n++;                                             // the addition that crosses into the next binade: rounded by the hardware
        }
        start[c] = s; count[c] = n; offset[c] = off; off += n;
        s = x - (double)chunk;
    }
    start[n_chunks] = s; offset[n_chunks] = off; *flag = 2;        // 2: this proposal is the one to check
}
__global__ void k_resample_walk(const double* start, const int* count, const int* offset, double t_ratio, int chunk, int n_chunks, int* pos, float* frac,
                                int* n_out, double* last_index_out, int cap, int* flag, int* fail, int level) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    if (level == 2 && *flag != 2) return;                                      // the first proposal was proven: nothing to redo
    const double end_idx = (double)(chunk - 9) - ceil(t_ratio);
    double idx = start[c]; int n = 0; const int o = offset[c];
    while (idx < end_idx) {
        idx += t_ratio;
        const double fl = floor(idx);
        if (o + n < cap) { pos[o + n] = c * chunk + (int)fl; frac[o + n] = (float)(idx - fl); }
        n++;
    }
    idx = idx - (double)chunk;
    if (n != count[c] || idx != start[c + 1]) atomicOr(fail, 1);      // the proposal is not the sequential walk: the next level redoes it
    if (c == n_chunks - 1) { *n_out = o + n; *last_index_out = idx; }
}
__global__ void k_resample_scan(double last_index, double t_ratio, int chunk, int n_chunks, int* pos, float* frac, int* n_out, double* last_index_out, int cap, const int* flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (flag && !*flag) return;
    const double end_idx = (double)(chunk - 9) - ceil(t_ratio);
    double idx = last_index; int n = 0;
    for (int c = 0; c < n_chunks; ++c) {
        while (idx < end_idx) {
            idx += t_ratio;
            const double fl = floor(idx);
            if (n < cap) { pos[n] = c * chunk + (int)fl; frac[n] = (float)(idx - fl); }
            n++;
        }
        idx = idx - (double)chunk;
    }
    *n_out = n; *last_index_out = idx;
}
// in: [16*ch history | n_chunks*chunk*ch] interleaved (history = the 16 frames preceding the first chunk); out interleaved
__global__ void k_resample_lerp(const float* in, int channels, const int* pos, const float* frac, const int* n_out, float* out, int cap) {
    const int n = min(*n_out, cap);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)n * channels; i += (long)gridDim.x * blockDim.x) {
        const int f = (int)(i / channels), c = (int)(i % channels);
        const float fr = frac[f]; const float* y = in + ((long)(pos[f] + 16)) * channels + c;
        out[i] = (1.0f - fr) * y[0] + fr * y[channels];
    }
}
void skw_resample_linear_launch(const float* in, int channels, double last_index, double t_ratio, int chunk, int n_chunks, int* pos, float* frac, int* n_out, double* last_index_out,
                                float* out, int cap, double* start, int* count, int* offset, int* flag, hipStream_t s, bool host_proposal) {
    const bool force_scan = skw_sw(SW_RESAMPLE_SCAN) != 0;     // the single-lane walk only (the fallback of both proposals; tests hold it to the same bits)
    if (force_scan) {
        // both flags set: "both proposals failed" is what this path stands for (skw_dsp_last_scan_fallback reports 2).  They were left as the allocation held them before round 5's
        // last day: the switch test passed or failed with whatever hipMalloc returned.
        hipMemsetAsync(flag, 0xFF, 2 * sizeof(int), s);
        hipLaunchKernelGGL(k_resample_scan, dim3(1), dim3(64), 0, s, last_index, t_ratio, chunk, n_chunks, pos, frac, n_out, last_index_out, cap, (const int*)nullptr);
    }
    else {
        // flag[0]: 0 = first proposal stands, 1 = it failed, 2 = second proposal to be checked; flag[1]: the second one failed too
        int* fail2 = flag + 1;
        hipMemsetAsync(flag, 0, 2 * sizeof(int), s);
        // first proposal: the closed form on the device, or — an inexact step over many chunks — the chunk starts the host walked and uploaded (skw_resample_linear)
        if (!host_proposal) hipLaunchKernelGGL(k_resample_starts_simple, dim3(1), dim3(64), 0, s, last_index, t_ratio, chunk, n_chunks, start, count, offset, flag);
        hipLaunchKernelGGL(k_resample_walk, dim3((n_chunks + 63) / 64), dim3(64), 0, s, start, count, offset, t_ratio, chunk, n_chunks, pos, frac, n_out, last_index_out, cap, flag, flag, 1);
        hipLaunchKernelGGL(k_resample_starts, dim3(1), dim3(64), 0, s, last_index, t_ratio, chunk, n_chunks, start, count, offset, flag);
        hipLaunchKernelGGL(k_resample_walk, dim3((n_chunks + 63) / 64), dim3(64), 0, s, start, count, offset, t_ratio, chunk, n_chunks, pos, frac, n_out, last_index_out, cap, flag, fail2, 2);
        hipLaunchKernelGGL(k_resample_scan, dim3(1), dim3(64), 0, s, last_index, t_ratio, chunk, n_chunks, pos, frac, n_out, last_index_out, cap, (const int*)fail2);
    }
    hipLaunchKernelGGL(k_resample_lerp, dim3(256), dim3(256), 0, s, in, channels, pos, frac, n_out, out, cap);
}

// ------------------------------------------------------------------ polyphase windowed-sinc resampler (quality mode; north_star's "polyphase resampler")
// out[n] = sum_t h[phase(n)][t] * x[base(n) + t - (T/2 - 1)], rational ratio L/M, T taps per phase, coefficients [L][T] from the host.
// One workgroup = PP_TILE consecutive output frames (all channels): the input span they read and, when it fits, the whole coefficient
// table are staged in LDS (coalesced 4-byte loads; table rows padded to an odd stride so that lanes on different phases hit different
// banks); per output the phase and base come from 32-bit arithmetic on the tile's (base0, phase0) — the one 64-bit division is per
// workgroup — and the tap loop is fma on two LDS operands.  Inputs are addressed absolutely: `in` holds frames [in_base, in_base + n_in)
// of the stream and everything outside [0, n_total) reads as zero, so a stream can be filtered packet by packet from a device-resident
// tail (skw_polyphase_stream_*) with results identical to filtering it whole.
#define PP_TILE 256
__global__ __launch_bounds__(256) void k_resample_polyphase(const float* in, long in_base, long n_in, long n_total, int channels, const float* coef, int L, int M, int T, int coef_in_lds,
                                                            float* out, long out_first, long n_out) {
    extern __shared__ float pp_lds[];
    const int tid = threadIdx.x, Ts = T | 1;
    const long o0 = out_first + (long)blockIdx.x * PP_TILE;
    const long num0 = o0 * (long)M; const long base0 = num0 / L; const int ph0 = (int)(num0 % L);
    const int span = (int)(((long)ph0 + (long)(PP_TILE - 1) * M) / L) + T;                 // frames [base0 - (T/2 - 1), base0 - (T/2 - 1) + span)
    const long first = base0 - (T / 2 - 1);
    float* xs = pp_lds; float* hs = pp_lds + (size_t)span * channels;
    for (int i = tid; i < span * channels; i += 256) {
        const long f = first + i / channels; const int c = i % channels;
        xs[i] = (f >= 0 && f < n_total && f >= in_base && f < in_base + n_in) ? in[(f - in_base) * channels + c] : 0.0f;
    }
    if (coef_in_lds) for (int i = tid; i < L * T; i += 256) hs[(i / T) * Ts + i % T] = coef[i];
    __syncthreads();
    const long o = o0 + tid;
    if (tid >= PP_TILE || o >= out_first + n_out) return;
    const int num = ph0 + tid * M; const int rel = num / L, ph = num % L;                  // 32-bit: ph0 < L <= 4096, tid < 256, M <= 4096
    const float* h = coef_in_lds ? hs + ph * Ts : coef + (long)ph * T;
    for (int c = 0; c < channels; ++c) {
        float acc = 0.0f; const float* x = xs + (size_t)rel * channels + c;
#pragma unroll 8
        for (int t = 0; t < T; ++t) acc = __builtin_fmaf(h[t], x[(size_t)t * channels], acc);
        out[(o - out_first) * channels + c] = acc;
    }
}
// outputs [out_first, out_first + n_out) of the stream into out[0 ..]; in = frames [in_base, in_base + n_in), n_total = frames of the stream known so far (beyond: zeros)
void skw_resample_polyphase_launch(const float* in, long in_base, long n_in, long n_total, int channels, const float* coef, int L, int M, int T, float* out,
    long out_first, long n_out, hipStream_t s) {
    if (n_out <= 0) return;
    const int span_max = (int)(((long)(L - 1) + (long)(PP_TILE - 1) * M) / L) + T;
    const size_t x_bytes = (size_t)span_max * channels * 4, h_bytes = (size_t)L * (T | 1) * 4;
    const int coef_in_lds = (x_bytes + h_bytes <= 96 * 1024) ? 1 : 0;
    if (x_bytes + (coef_in_lds ? h_bytes : 0) > 64 * 1024) {      // more dynamic LDS than the default limit: raise it on this device (per device: several GPUs may run in one process)
        static std::atomic<bool> raised[64]; int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (!raised[dev].load(std::memory_order_acquire)) { hipFuncSetAttribute((const void*)k_resample_polyphase, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        raised[dev].store(true, std::memory_order_release); }
    }
    hipLaunchKernelGGL(k_resample_polyphase, dim3((unsigned)((n_out + PP_TILE - 1) / PP_TILE)), dim3(256), x_bytes + (coef_in_lds ? h_bytes : 0), s,
                       in, in_base, n_in, n_total, channels, coef, L, M, T, coef_in_lds, out, out_first, n_out);
}
