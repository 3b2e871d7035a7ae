// skw_kernels_align.hip — word timestamps on the GPU: the three kernels that evaluate include/skw_align.h (the contract: every order of operations below is the one stated there,
// and the header's *_ref evaluator produces the same bits on a CPU).  A first form, shaped for being exact and ragged, not yet for speed (per-launch times: profiles/align/).
//   k_align_qk      step 1: the softmaxed cross-attention weights of one decoder layer's alignment heads, for every row of every sequence of the pass
//   k_align_reduce  steps 2-5 for one layer's heads, accumulated into each sequence's N x Kw matrix (an f64 running sum per cell across layers, rounded after the last)
//   k_align_dtw     steps 6-7: one workgroup per sequence, an anti-diagonal wavefront, then one lane walks the path back
#include <atomic>
#include "skw_dev_common.h"
#include "../../include/skw_align.h"

// ------------------------------------------------------------------ step 1
// One WAVE per (row, alignment head): lane j owns keys j, j + 64, ... — the lane-strided partial sums of the contract's Z.  Scores, then exponentials, wait in the wave's own
// 6 KiB of LDS between the passes; every lane reads back only what it wrote itself, so there is no barrier.  K is read in either stored layout: rows ([slot][n_ctx][d]) or the
// fragment-order image (skw_kfrag_off); a key's 64 channels of one head are eight 16-byte pieces in both.
#define SKW_ALIGN_QK_WAVES 4
__global__ __launch_bounds__(64 * SKW_ALIGN_QK_WAVES) void k_align_qk(const half_t* __restrict__ q, long ldq, const half_t* __restrict__ ck, const SkwAlignSeq* __restrict__ seqs, int n_seq,
                                                                       unsigned head_mask, int nh, int H, int n_ctx, int Tpad, int frag, float* __restrict__ P, long p_rows, long p_stride,
                                                                       int rows_total) {
    __shared__ float sc[SKW_ALIGN_QK_WAVES][SKW_XATTN_MQ_MAX_CTX];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int item = blockIdx.x * SKW_ALIGN_QK_WAVES + w;
    if (item >= rows_total * nh) return;                                    // (wave-uniform)
    const int prow = item / nh, hl = item % nh;
    int h = 0; { unsigned m = head_mask; for (int i = 0; i < hl; ++i) m &= m - 1; h = __builtin_ctz(m); }
    int si = 0; while (si + 1 < n_seq && prow >= seqs[si].prow0 + seqs[si].n) ++si;      // the sequences' rows are contiguous and ascending in P
    const SkwAlignSeq sq = seqs[si];
    const int r = prow - sq.prow0;
    if (r < 0 || r >= sq.n) return;
    const int n_keys = sq.n_keys > 0 && sq.n_keys < n_ctx ? sq.n_keys : n_ctx;
    float qf[64];
    { const H8* qp = (const H8*)(q + (long)(sq.qrow0 + r) * ldq + h * 64);
#pragma unroll
      for (int p = 0; p < 8; ++p) { const H8 v = qp[p];
#pragma unroll
          for (int j = 0; j < 8; ++j) qf[8 * p + j] = h2f(v.h[j]); } }
    float* s = sc[w];
    float m = -__builtin_inff();
    for (int k = lane; k < n_keys; k += 64) {
        float a = 0.0f;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const long off = frag ? skw_kfrag_off(sq.slot, H, Tpad, k, h * 64 + 8 * p) : ((long)sq.slot * n_ctx + k) * ((long)H * 64) + h * 64 + 8 * p;
            const H8 v = *(const H8*)(ck + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) a = __builtin_fmaf(qf[8 * p + j], h2f(v.h[j]), a);
        }
        s[k] = a;
        m = fmaxf(m, a);
    }
    m = skw_wave_max_f32(m);
    double z = 0.0;
    for (int k = lane; k < n_keys; k += 64) { const float e = skw_expf(s[k] - m); s[k] = e; z += (double)e; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) z += __shfl_xor(z, o, 64);            // lane 0: p[j] += p[j + o] for j < o, the contract's tree (addition commutes)
    z = __shfl(z, 0, 64);
    float* out = P + ((long)hl * p_rows + prow) * p_stride;
    for (int k = lane; k < n_keys; k += 64) out[k] = (float)((double)s[k] / z);
}

bool skw_align_qk(const half_t* q, long ldq, const half_t* ck, const SkwAlignSeq* seqs, int n_seq, int rows_total, unsigned head_mask, int H, int n_ctx, int Tpad, int frag,
                  float* P, long p_rows, long p_stride, hipStream_t s) {
    const int nh = skw_align_popcount(head_mask);
    if (n_seq < 1 || rows_total < 1 || nh < 1 || H < 1 || H > 32 || (H < 32 && (head_mask >> H)) || n_ctx < 1 || n_ctx > SKW_XATTN_MQ_MAX_CTX || p_stride < n_ctx || p_rows < rows_total) return false;
    const long items = (long)rows_total * nh;
    hipLaunchKernelGGL(k_align_qk, dim3((unsigned)((items + SKW_ALIGN_QK_WAVES - 1) / SKW_ALIGN_QK_WAVES)), dim3(64 * SKW_ALIGN_QK_WAVES), 0, s, q, ldq, ck, seqs, n_seq, head_mask, nh, H,
                       n_ctx, Tpad, frag, P, p_rows, p_stride, rows_total);
    return true;
}

// ------------------------------------------------------------------ steps 2-5
// Workgroup = (key tile, sequence); thread = one key column (the tile's output columns plus the median's reflected margin on both sides).  Per head: the column's f64 statistics
// (rows ascending, as the contract sums them), then row by row every thread normalises its element into LDS and the tile's threads select the median of their window and add
// it to their cell's accumulator.  A cell is owned by one thread, and the layers are launched in ascending order: the running sum is the (layer, head)-ascending one.
__global__ __launch_bounds__(256) void k_align_reduce(const float* __restrict__ P, long p_rows, long p_stride, const SkwAlignSeq* __restrict__ seqs, int nh, int width, int first, int last,
                                                      int n_heads_total, double* __restrict__ acc, float* __restrict__ x) {
    __shared__ float zs[2][256];
    const SkwAlignSeq sq = seqs[blockIdx.y];
    const int half = width / 2, tile = 256 - 2 * half, kw = sq.kw, N = sq.n, filt = kw > half;
    const int k0 = blockIdx.x * tile;
    if (k0 >= kw) return;                                                   // (uniform: every barrier below is reached by all threads or none)
    const int tid = threadIdx.x, oc = k0 + tid - half;                      // the column this thread stands for, before reflection
    const bool have = filt ? (oc > -kw && oc < 2 * kw - 1 && oc >= -half && oc < kw + half) : (oc >= 0 && oc < kw);
    const int col = have ? (filt ? skw_align_reflect(oc, kw) : oc) : 0;
    const bool outv = tid >= half && tid < 256 - half && oc < kw;           // this thread owns cell column oc
    for (int hl = 0; hl < nh; ++hl) {
        const float* Ph = P + ((long)hl * p_rows + sq.prow0) * p_stride + col;
        double sum = 0.0, sq2 = 0.0;
        if (have) for (int r = 0; r < N; ++r) sum += (double)Ph[(long)r * p_stride];
        const double mean = sum / (double)N;
        if (have) for (int r = 0; r < N; ++r) { const double d = (double)Ph[(long)r * p_stride] - mean; sq2 += d * d; }
        const double var = sq2 / (double)N, sd = sqrt(var);
        for (int r = 0; r < N; ++r) {
            const float z = have ? skw_align_z(Ph[(long)r * p_stride], mean, var, sd) : 0.0f;
            float med = z;
            if (filt) {
                zs[r & 1][tid] = z;
                __syncthreads();
                if (outv) { float v[SKW_ALIGN_MEDIAN_MAX]; for (int a = 0; a < width; ++a) v[a] = zs[r & 1][tid - half + a]; med = skw_align_median(v, width); }
            }
            if (outv) {
                const long cell = sq.xoff + (long)r * kw + oc;
                double a = (first && hl == 0) ? 0.0 : acc[cell];
                a += (double)med;
                acc[cell] = a;
                if (last && hl == nh - 1) x[cell] = -(float)(a / (double)n_heads_total);
            }
        }
        __syncthreads();                                                    // the next head's first row reuses zs[0]
    }
}

bool skw_align_reduce(const float* P, long p_rows, long p_stride, const SkwAlignSeq* seqs, int n_seq, int kw_max, int nh, int width, int first, int last, int n_heads_total,
                      double* acc, float* x, hipStream_t s) {
    if (n_seq < 1 || kw_max < 1 || nh < 1 || width < 1 || !(width & 1) || width > SKW_ALIGN_MEDIAN_MAX || n_heads_total < nh) return false;
    const int tile = 256 - 2 * (width / 2);
    hipLaunchKernelGGL(k_align_reduce, dim3((kw_max + tile - 1) / tile, n_seq), dim3(256), 0, s, P, p_rows, p_stride, seqs, nh, width, first, last, n_heads_total, acc, x);
    return true;
}

// ------------------------------------------------------------------ steps 6-7
// One workgroup per sequence; thread i owns row i (1 .. N) of the cost table and walks it along the anti-diagonals d = i + j: a cell needs the row above at the previous diagonal
// (up), the row above two diagonals back (diagonal: what this thread read as `up` one step earlier, kept in a register) and its own previous cell (left, a register).  So one
// diagonal of cost travels through LDS per step, double buffered, one barrier per diagonal; N + Kw - 1 steps.
// The 2-bit trace lives in LDS: a thread packs 16 cells of its row into a word it alone writes — 226 rows x 94 words = 85 KB for the largest problem (226 x 1500), inside the
// 160 KiB of a CU (one workgroup per CU then, which is what a handful of sequences per window wants anyway); in global memory the single lane's backtrace would pay a
// dependent global load per step of its N + Kw walk.  Problems whose trace does not fit are refused by the launcher.
__global__ __launch_bounds__(SKW_ALIGN_MAX_ROWS) void k_align_dtw(const float* __restrict__ x, const SkwAlignSeq* __restrict__ seqs, int* __restrict__ jump, int* __restrict__ t0,
                                                                  int* __restrict__ t1, int lds_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned al_lds[];
    const SkwAlignSeq sq = seqs[blockIdx.x];
    const int N = sq.n, Kw = sq.kw, ws = (Kw + 15) >> 4;
    if (N < 1 || N > SKW_ALIGN_MAX_ROWS || Kw < 1 || 2 * (SKW_ALIGN_MAX_ROWS + 1) + (long)N * ws > lds_words) return;      // (uniform; the launcher has checked)
    float* cbuf = (float*)al_lds;                                           // [2][SKW_ALIGN_MAX_ROWS + 1]: cost of row i at the last two diagonals
    unsigned* tr = al_lds + 2 * (SKW_ALIGN_MAX_ROWS + 1);                    // [N][ws]
    const int i = threadIdx.x + 1;
    const bool mine = i <= N;
    const float inf = __builtin_inff();
    const float* xr = x + sq.xoff + (long)(i - 1) * Kw;
    float left = inf, diag = i == 1 ? 0.0f : inf, xn = mine ? xr[0] : 0.0f;
    unsigned word = 0;
    for (int d = 2; d <= N + Kw; ++d) {
        const int j = d - i;
        if (mine && j >= 1 && j <= Kw) {
            const float up = i == 1 ? inf : cbuf[((d - 1) & 1) * (SKW_ALIGN_MAX_ROWS + 1) + i - 1];
            int t; const float c = skw_align_pick(diag, up, left, &t);
            const float v = xn + c;
            if (j < Kw) xn = xr[j];
            cbuf[(d & 1) * (SKW_ALIGN_MAX_ROWS + 1) + i] = v;
            left = v; diag = up;
            word |= (unsigned)t << (2 * ((j - 1) & 15));
            if (((j - 1) & 15) == 15 || j == Kw) { tr[(i - 1) * ws + ((j - 1) >> 4)] = word; word = 0; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int* jp = jump + sq.prow0;
        int a = N, b = Kw;
        for (int guard = 0; (a > 0 || b > 0) && guard < N + Kw + 2; ++guard) {
            if (a > 0) jp[a - 1] = b - 1;                                   // walking backwards: the last store into a row is the path's first visit of it
            const int t = a == 0 ? 2 : (b == 0 ? 1 : (int)((tr[(a - 1) * ws + ((b - 1) >> 4)] >> (2 * ((b - 1) & 15))) & 3u));
            if (t == 0) { --a; --b; } else if (t == 1) --a; else --b;
        }
        skw_align_times(jp, N, sq.seek_cs, t0 + sq.prow0, t1 + sq.prow0);
    }
}

// n_max / kw_max: the largest N and Kw among the sequences (the LDS request); false, nothing launched: a problem beyond SKW_ALIGN_MAX_ROWS rows or 150 KiB of trace
bool skw_align_dtw(const float* x, const SkwAlignSeq* seqs, int n_seq, int n_max, int kw_max, int* jump, int* t0, int* t1, hipStream_t s) {
    if (n_seq < 1 || n_max < 1 || n_max > SKW_ALIGN_MAX_ROWS || kw_max < 1) return false;
    const long words = 2 * (SKW_ALIGN_MAX_ROWS + 1) + (long)n_max * ((kw_max + 15) >> 4);
    if (words * 4 > 150 * 1024) return false;
    if (words * 4 > 64 * 1024) {      // more dynamic LDS than the default limit: raise it on this device
        static std::atomic<bool> raised[64]; int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (!raised[dev].load(std::memory_order_acquire)) {
            if (hipFuncSetAttribute((const void*)k_align_dtw, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return false;      // (nothing launched)
            raised[dev].store(true, std::memory_order_release); }
    }
    hipLaunchKernelGGL(k_align_dtw, dim3(n_seq), dim3(SKW_ALIGN_MAX_ROWS), (size_t)words * 4, s, x, seqs, jump, t0, t1, (int)words);
    return true;
}
