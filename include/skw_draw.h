/*
 * skw_draw.h — the two SERIAL chains of the sampler's workgroup-wide draw (block_discrete_draw, streamkit_amd/csrc/skw_kernels_sample.hip), host and device.
 *
 * std::discrete_distribution as libstdc++ implements it is sequential: sum = p_0 + p_1 + ... in f64, q_i = p_i / sum, cp_i = q_0 + ... + q_i with the last forced to 1.0,
 * the first i with cp_i >= u.  The kernel stages the row through LDS in chunks of SKW_DRAW_CHUNK doubles, with the largest element of every SKW_DRAW_BLOCK of them beside
 * it (bmax), and ONE lane walks each chunk with the functions below; staging, barriers and the divisions are the kernel's.  tests/cpp/draw_main.cpp stages rows the same
 * way on the CPU and holds these walks to the plain sequential definition, bit for bit (tests/test_cpu_sampler_draw.py).
 *
 * Skipping.  S + p == S under round-to-nearest whenever 0 <= p < ulp(S) / 2: a block whose largest element is below that bound cannot move the running sum, whatever the
 * order inside it, and since the sum never decreases it stays immovable — such blocks are skipped WITHOUT changing a bit of the sequential result.  The bound is strict:
 * p == ulp(S) / 2 is a tie, and round-to-even moves an odd S.
 *
 * Chunks are 16-byte aligned (the walks read two doubles at a time).  n_skipped (may be null): incremented once per block skipped by the bound — tests only.
 */
#ifndef SKW_DRAW_H
#define SKW_DRAW_H

#include <stdint.h>
#include <string.h>
#include "skw_math.h"

#define SKW_DRAW_CHUNK 4096     /* doubles per staged chunk (32 KB of LDS) */
#define SKW_DRAW_BLOCK 64       /* elements per bmax entry */

#if defined(__clang__)
typedef double skw_f64x2 __attribute__((ext_vector_type(2)));
#else
typedef double skw_f64x2 __attribute__((vector_size(16)));
#endif

/* 2^(exponent(s) - 53); 0 for s == 0 / subnormal: nothing is skipped then */
SKW_HD double skw_half_ulp_f64(double s) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int e = (int)((__double_as_longlong(s) >> 52) & 0x7ff);
    return e == 0 ? 0.0 : __longlong_as_double((long long)(e - 53 > 1 ? e - 53 : 1) << 52);
#else
    long long b; memcpy(&b, &s, 8);
    const int e = (int)((b >> 52) & 0x7ff);
    if (e == 0) return 0.0;
    b = (long long)(e - 53 > 1 ? e - 53 : 1) << 52;
    double r; memcpy(&r, &b, 8); return r;
#endif
}

/* first chain over one staged chunk: ch[0 .. m) in ascending order onto sum; returns the new sum */
SKW_HD double skw_draw_sum_chunk(const double* ch, const double* bmax, int m, double sum, int* n_skipped) {
    for (int b0 = 0; b0 < m; b0 += SKW_DRAW_BLOCK) {
        if (bmax[b0 >> 6] < skw_half_ulp_f64(sum)) { if (n_skipped) ++*n_skipped; continue; }
        const int e = b0 + SKW_DRAW_BLOCK < m ? b0 + SKW_DRAW_BLOCK : m; int i = b0;
        for (; i + 2 <= e; i += 2) { const skw_f64x2 v = *(const skw_f64x2*)(ch + i); sum += v[0]; sum += v[1]; }
        for (; i < e; ++i) sum += ch[i];
    }
    return sum;
}

/* second chain over one staged chunk of q = p / sum: elements c0 .. c0 + m of a row of n; *cp is the running partial sum (in and out).  Returns the index of the hit
 * (the first i with cp_i >= u; cp_{n-1} = 1.0 by definition) or -1 when the chunk holds none. */
SKW_HD int skw_draw_cp_chunk(const double* ch, const double* bmax, int m, int c0, int n, double u, double* cp_io, int* n_skipped) {
    double cp = *cp_io; int hit = -1;
    for (int b0 = 0; b0 < m && hit < 0; b0 += SKW_DRAW_BLOCK) {
        const int e = b0 + SKW_DRAW_BLOCK < m ? b0 + SKW_DRAW_BLOCK : m; const bool last_block = c0 + e == n;
        if (!last_block && bmax[b0 >> 6] < skw_half_ulp_f64(cp)) { if (n_skipped) ++*n_skipped; continue; }      /* (the block that holds the last element is walked: cp = 1 there by definition) */
        if (!last_block) {      /* cp never decreases: a block whose END is still below u holds no hit — one compare per block instead of one per element */
            double c2 = cp; int i = b0;
            for (; i + 2 <= e; i += 2) { const skw_f64x2 v = *(const skw_f64x2*)(ch + i); c2 += v[0]; c2 += v[1]; }
            for (; i < e; ++i) c2 += ch[i];
            if (c2 < u) { cp = c2; continue; }
        }
        for (int i = b0; i < e; ++i) { cp += ch[i]; if (c0 + i == n - 1) cp = 1.0; if (!(cp < u)) { hit = c0 + i; break; } }
    }
    *cp_io = cp;
    return hit;
}

#endif
