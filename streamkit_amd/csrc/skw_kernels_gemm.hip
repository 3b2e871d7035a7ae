// skw_kernels_gemm.hip — the exact precision's GEMMs (f32 MFMA) and LayerNorm for gfx950 (CDNA4).
// Compile with -ffp-contract=off: every fused multiply-add in here is explicit (see include/skw_math.h).
//
// What each kernel restates (whisper.cpp routine):
//   k_gemm*            ggml_mul_mat with f16 src0 / f16-converted src1, f32 accumulate (K2, K4-K6, K8-K10)
//   k_layernorm        ggml_norm + ggml_mul + ggml_add (K3)
#include "skw_dev_common.h"

// ------------------------------------------------------------------ big-M GEMM
// C[m][n] = chain_k A[m][k] * W[n][k]; 128x128 block tile, 4 waves (2x2), wave tile 64x64 = 4x4 MFMA 16x16x4 tiles.
// LDS rows are 32 halves (one kperm block) + 8 halves of padding (80 B) -> conflict-free ds_read_b128.
#define G_BM 128
#define G_BN 128
#define G_LDS_ROW 40   // halves
template <int EPI>
__global__ __launch_bounds__(256, 2) void k_gemm(SkwGemmArgs a) {
    __shared__ __attribute__((aligned(16))) half_t lds[2][2][G_BM * G_LDS_ROW];   // [buf][A/B][rows*40]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbn = (a.N + G_BN - 1) / G_BN, nbm = (a.M + G_BM - 1) / G_BM, nblk = nbn * nbm;
    // XCD-aware bijective remap: blocks b and b+8 share an XCD; give each XCD a contiguous run of tiles
    int bid = blockIdx.x;
    { int q = nblk >> 3, r = nblk & 7, x = bid & 7, y = bid >> 3; bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y; }
    const int bm = bid / nbn, bn = bid % nbn;       // n-tiles of one m-tile adjacent -> A panel reused from L2
    const int m0 = bm * G_BM, n0 = bn * G_BN;
    const int wr = wave >> 1, wc = wave & 1, r16 = lane & 15, kq = lane >> 4;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // staging: 512 16-byte chunks per operand tile, 2 per thread per operand; buffer loads with hardware range checking (rows past
    // M / N read as zeros, no branches), per-thread byte offsets fixed up front, the k-block offset in an SGPR
    u32x4 stA[2], stB[2];
    const int nk = a.K >> 5;
    const long a_rows = a.a_rows_per_batch ? (long)((a.M - 1) / a.a_rows_per_batch) * a.a_batch_stride + (long)((a.M - 1) % a.a_rows_per_batch) * a.lda : (long)(a.M - 1) * a.lda;
    __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, 0, (unsigned)((a_rows + a.K) * 2), 0x00020000);
    __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, (unsigned)(((long)(a.N - 1) * a.ldw + a.K) * 2), 0x00020000);
    unsigned voA[2], voB[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int c = tid + 256 * i, row = c >> 2, kc = c & 3;
        int gm = m0 + row, gn = n0 + row;
        long aoff = a.a_rows_per_batch ? (long)(gm / a.a_rows_per_batch) * a.a_batch_stride + (long)(gm % a.a_rows_per_batch) * a.lda : (long)gm * a.lda;
        voA[i] = (gm < a.M) ? (unsigned)((aoff + kc * 8) * 2) : 0x7fffff00u;
        voB[i] = (gn < a.N) ? (unsigned)(((long)gn * a.ldw + kc * 8) * 2) : 0x7fffff00u;
    }
    auto gload = [&](int kb) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            stA[i] = __builtin_amdgcn_raw_buffer_load_b128(rA, voA[i], kb * 64, 0);
            stB[i] = __builtin_amdgcn_raw_buffer_load_b128(rB, voB[i], kb * 64, 0);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int c = tid + 256 * i, row = c >> 2, kc = c & 3;
            *(u32x4*)(&lds[buf][0][row * G_LDS_ROW + kc * 8]) = stA[i];
            *(u32x4*)(&lds[buf][1][row * G_LDS_ROW + kc * 8]) = stB[i];
        }
    };
    gload(0); lstore(0); __syncthreads();
    for (int kb = 0; kb < nk; ++kb) {
        const int buf = kb & 1;
        if (kb + 1 < nk) gload(kb + 1);
        H8 fa[4], fb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            fa[t].u = *(const uint4*)(&lds[buf][0][(wr * 64 + t * 16 + r16) * G_LDS_ROW + kq * 8]);
            fb[t].u = *(const uint4*)(&lds[buf][1][(wc * 64 + t * 16 + r16) * G_LDS_ROW + kq * 8]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { av[t] = h2f(fa[t].h[e]); bv[t] = h2f(fb[t].h[e]); }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = MFMA16(av[i], bv[j], acc[i][j]);
        }
        if (kb + 1 < nk) lstore(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int m = m0 + wr * 64 + i * 16 + kq * 4 + r, n = n0 + wc * 64 + j * 16 + r16;
                if (m < a.M && n < a.N) epi_store<EPI>(a, m, n, acc[i][j][r]);
            }
}

// ------------------------------------------------------------------ small-M GEMM (decode, M <= 64), exact precision
// Weight-streaming form: fragments straight from global memory, a ring of SM_DEPTH k-blocks (16 B per lane per operand per block) in flight to hide HBM latency.
// The contraction runs in FOUR contiguous K segments (D3'): a workgroup is one 16-column strip x one 16-row tile, wave s
// chains segment s (k-blocks [s nk/4, (s+1) nk/4), k-ascending from zero), the partial tiles meet in LDS and wave 0 adds them in ascending
// segment order, ((s0 + s1) + s2) + s3 — oracle/skw_oracle.c gemm_chain_seg4, bit for bit.  A quarter of the dependent-MFMA chain per wave.
template <int EPI, int SM_DEPTH>
__global__ __launch_bounds__(256) void k_gemm_smallm_seg(SkwGemmArgs a) {
    __shared__ f32x4 red[4][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = blockIdx.x * 16, mt = blockIdx.y;
    const int r16 = lane & 15, kq = lane >> 4;
    const int gn = n0 + r16, gm = mt * 16 + r16;
    const unsigned wbytes = (unsigned)((long)a.N * a.ldw * 2), abytes = (unsigned)(((long)(a.M - 1) * a.lda + a.K) * 2);
    // fragment-order weight image (SkwGemmArgs::Wf, built for the f16 decode kernels): the same sixteen bytes per lane from one contiguous KiB per (strip, k-block) instead of 16 rows x 64 B —
    // the values, and so every chain, are unchanged.  (Not for the GELU product: its image holds the rows in the f16 kernels' output order.)
    const bool wfrag = a.Wf != nullptr && EPI != EPI_GELU_F16_KPERM && !(a.N & 15);
    const unsigned wstep = wfrag ? 1024u : 64u;
    __amdgpu_buffer_rsrc_t rw = wfrag ? __builtin_amdgcn_make_buffer_rsrc((void*)a.Wf, 0, (unsigned)((long)a.N * a.K * 2),
        0x00020000) : __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, wbytes, 0x00020000);
    __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, 0, abytes, 0x00020000);
    const unsigned oob = 0x7fffff00u;
    const int nkq = (a.K >> 5) >> 2, kb_lo = wave * nkq;                 // host guarantees K % 128 == 0
    const unsigned wo = wfrag ? (unsigned)(((long)blockIdx.x * (a.K >> 5) + kb_lo) * 1024 + lane * 16) : (gn < a.N) ? (unsigned)(((long)gn * a.ldw + kb_lo * 32 + kq * 8) * 2) : oob;
    const unsigned ao = (gm < a.M) ? (unsigned)(((long)gm * a.lda + kb_lo * 32 + kq * 8) * 2) : oob;
    H8v fw[SM_DEPTH], fa[SM_DEPTH];
#pragma unroll
    for (int j = 0; j < SM_DEPTH; ++j) {
        fw[j].v = __builtin_amdgcn_raw_buffer_load_b128(rw, (wo == oob || j >= nkq) ? oob : wo + j * wstep, 0, 0);
        fa[j].v = __builtin_amdgcn_raw_buffer_load_b128(ra, (ao == oob || j >= nkq) ? oob : ao + j * 64, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    const int en = n0 + r16; const bool en_ok = en < a.N && wave == 0;
    float pre_bias = 0.0f, pre_res[4] = {0.f, 0.f, 0.f, 0.f}; long pre_po[4] = {0, 0, 0, 0};
    if (EPI != EPI_VT_F16 && a.bias && en_ok) pre_bias = a.bias[en];
    if (EPI == EPI_F32 && a.res && en_ok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int m = mt * 16 + kq * 4 + r; if (m < a.M) pre_res[r] = a.res[(long)m * a.ldres + en]; }
    }
    if (EPI == EPI_DEC_QKV && a.pos_ptr && wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int m = mt * 16 + kq * 4 + r; if (m < a.M) pre_po[r] = (long)a.pos_ptr[(long)m * a.pos_stride] * a.n_ctx; }
    }
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kb0 = 0; kb0 < nkq; kb0 += SM_DEPTH) {
#pragma unroll
        for (int j = 0; j < SM_DEPTH; ++j) {
            float xa[8], xw[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { xa[e] = h2f(fa[j].h[e]); xw[e] = h2f(fw[j].h[e]); }
            __builtin_amdgcn_sched_barrier(0);
            const int nb = kb0 + j + SM_DEPTH;
            fw[j].v = __builtin_amdgcn_raw_buffer_load_b128(rw, (wo == oob || nb >= nkq) ? oob : wo + nb * wstep, 0, 0);
            fa[j].v = __builtin_amdgcn_raw_buffer_load_b128(ra, (ao == oob || nb >= nkq) ? oob : ao + nb * 64, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (kb0 + j < nkq) {                                         // (uniform) blocks past the segment are skipped, not multiplied by zeros
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = MFMA16(xa[e], xw[e], acc);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    {
        const f32x4 s1 = red[1][lane], s2 = red[2][lane], s3 = red[3][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) { float v = acc[r] + s1[r]; v = v + s2[r]; v = v + s3[r]; acc[r] = v; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int m = mt * 16 + kq * 4 + r, n = n0 + r16;
        if (!(m < a.M && n < a.N)) continue;
        float v = acc[r];
        if (EPI == EPI_F32) {
            if (a.bias) v = v + pre_bias;
            if (a.res) v = v + pre_res[r];
            ((float*)a.C)[(long)m * a.ldc + n] = v;
        } else if (EPI == EPI_F16_PLAIN) {
            if (a.bias) v = v + pre_bias;
            if (a.has_scale) v = v * a.scale;
            ((half_t*)a.C)[(long)m * a.ldc + n] = f2h(v);
        } else if (EPI == EPI_GELU_F16_KPERM) {
            if (a.bias) v = v + pre_bias;
            ((half_t*)a.C)[(long)m * a.ldc + skw_kperm(n)] = f2h(gelu_dev(v, a.gelu_tab));
        } else if (EPI == EPI_DEC_QKV) {
            const int d = a.n_ctx;
            if (a.bias) v = v + pre_bias;
            if (n < 2 * d) v = v * a.scale;
            if (n < d) ((half_t*)a.C)[(long)m * a.ldc + n] = f2h(v);
            else if (n < 2 * d) ((half_t*)a.C2)[(long)m * a.ldc2 + pre_po[r] + (n - d)] = f2h(v);
            else ((half_t*)a.C3)[(long)m * a.ldc2 + pre_po[r] + (n - 2 * d)] = f2h(v);
        } else epi_store<EPI>(a, m, n, acc[r]);
    }
}

template <int EPI> static void launch_gemm(const SkwGemmArgs& a, hipStream_t s) {
    int nbn = (a.N + G_BN - 1) / G_BN, nbm = (a.M + G_BM - 1) / G_BM;
    hipLaunchKernelGGL(k_gemm<EPI>, dim3(nbn * nbm), dim3(256), 0, s, a);
}
void skw_gemm(const SkwGemmArgs& a, hipStream_t s) {
    switch (a.epi) {
        case EPI_F32: launch_gemm<EPI_F32>(a, s); break;
        case EPI_F16_KPERM: launch_gemm<EPI_F16_KPERM>(a, s); break;
        case EPI_GELU_F16_KPERM: launch_gemm<EPI_GELU_F16_KPERM>(a, s); break;
        case EPI_GELU_F16_KPERM_ROWPAD: launch_gemm<EPI_GELU_F16_KPERM_ROWPAD>(a, s); break;
        case EPI_CONV2: launch_gemm<EPI_CONV2>(a, s); break;
        case EPI_HEADS_F16: launch_gemm<EPI_HEADS_F16>(a, s); break;
        case EPI_VT_F16: launch_gemm<EPI_VT_F16>(a, s); break;
        case EPI_F16_PLAIN: launch_gemm<EPI_F16_PLAIN>(a, s); break;
    }
}
// K % 128 == 0 (skw_model_load rejects any other decoder width: the oracle's segmented chain, gemm_chain_seg4, is defined for it)
template <int EPI> static void launch_gemm_small(const SkwGemmArgs& a, hipStream_t s) {
    const int nk = a.K >> 5, nkq = nk >> 2;
    const dim3 gs((a.N + 15) / 16, (a.M + 15) / 16);
    if (nkq % 24 == 0) hipLaunchKernelGGL((k_gemm_smallm_seg<EPI, 24>), gs, dim3(256), 0, s, a);
    else if (nkq <= 6) hipLaunchKernelGGL((k_gemm_smallm_seg<EPI, 6>), gs, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_gemm_smallm_seg<EPI, 8>), gs, dim3(256), 0, s, a);
}
void skw_gemm_smallm(const SkwGemmArgs& a, hipStream_t s) {
    switch (a.epi) {
        case EPI_F32: launch_gemm_small<EPI_F32>(a, s); break;
        case EPI_F16_KPERM: launch_gemm_small<EPI_F16_KPERM>(a, s); break;
        case EPI_GELU_F16_KPERM: launch_gemm_small<EPI_GELU_F16_KPERM>(a, s); break;
        case EPI_F16_PLAIN: launch_gemm_small<EPI_F16_PLAIN>(a, s); break;
        case EPI_DEC_QKV: launch_gemm_small<EPI_DEC_QKV>(a, s); break;
        default: break;
    }
}

// ------------------------------------------------------------------ LayerNorm
// one wave per R rows; d <= 64 NC (NC = 12 for every width up to Whisper-small's, 24 up to 1536); FULL: d == 64 NC (Whisper-small: straight-line code, no tail predicates).
// R = 2 for the encoder's 96 000-row launches: the kernel is a stream (442 MB per launch) and a wave with one 3 KiB row in flight leaves the CU short of bytes in flight;
// the rows' arithmetic is skw_ln_rows' either way (same bits; profiles/r04i: 0.085 vs 0.11 ms per launch).
template <int NC, bool FULL, int R = 1>
__global__ __launch_bounds__(256) void k_layernorm(const float* x, int rows, int d, const float* w, const float* b, half_t* out16, float* out32) {
    const int lane = threadIdx.x & 63, row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;
    float v[R][NC], wv[NC], bv[NC];
    bool live[R]; half_t* o16[R]; float* o32[R];
    // the gain / bias loads go out together with the rows (a 64-row decode launch is three dependent round trips otherwise)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = row0 + r; live[r] = row < rows;
        const float* xr = x + (long)(live[r] ? row : row0) * d;
#pragma unroll
        for (int c = 0; c < NC; ++c) { const int i = lane + 64 * c; v[r][c] = (FULL || i < d) ? xr[i] : 0.0f; }
        o16[r] = out16 ? out16 + (long)(live[r] ? row : row0) * d : nullptr; o32[r] = out32 ? out32 + (long)(live[r] ? row : row0) * d : nullptr;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) { const int i = lane + 64 * c; const bool in = FULL || i < d; wv[c] = in ? w[i] : 0.0f; bv[c] = in ? b[i] : 0.0f; }
    skw_ln_rows<R, NC, FULL>(v, wv, bv, d, lane, live, o16, o32);
}
void skw_layernorm(const float* x, int rows, int d, const float* w, const float* b, half_t* out16, float* out32, hipStream_t s) {
    const bool two = rows >= 8192 && d == 768;
    const dim3 g(two ? (rows + 7) / 8 : (rows + 3) / 4);
    if (two) hipLaunchKernelGGL((k_layernorm<12, true, 2>), g, dim3(256), 0, s, x, rows, d, w, b, out16, out32);
    else if (d == 768) hipLaunchKernelGGL((k_layernorm<12, true>), g, dim3(256), 0, s, x, rows, d, w, b, out16, out32);
    else if (d <= 768) hipLaunchKernelGGL((k_layernorm<12, false>), g, dim3(256), 0, s, x, rows, d, w, b, out16, out32);
    else hipLaunchKernelGGL((k_layernorm<24, false>), g, dim3(256), 0, s, x, rows, d, w, b, out16, out32);
}
