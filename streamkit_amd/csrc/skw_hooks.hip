// skw_hooks.hip — the kernel-level test and measurement hooks of libskw_engine.so: each skw_debug_* entry here runs ONE kernel (through its public launcher) on operands the
// caller supplies, on the context's stream, and hands back what the kernel wrote; the skw_layout_* exports are the host-side view of the layouts those operands are packed into.
// Of the engine they need the context's stream, device and error buffer, the model's constants, the switchboard and the loader's repack (skw_engine_priv.h) — nothing of its phases.
// The hooks that drive the engine's own phases (skw_debug_sample_rows*, the stage taps, skw_debug_xattn, the kernel clock) are at the end of skw_engine.hip.
#include "skw_engine_priv.h"

// host-side view of the fragment-order layouts (tests/test_cpu_layouts.py checks them without a GPU): element offset of the 16-byte chunk that holds (key, feat .. feat + 7) of cross K /
// (feat, positions pos .. pos + 7) of cross V^T
extern "C" long skw_layout_kfrag_off(int slot, int H, int Tpad, int key, int feat) { return skw_kfrag_off(slot, H, Tpad, key, feat); }
extern "C" long skw_layout_vtfrag_off(int slot, int H, int Tpad, int feat, int pos) { return skw_vtfrag_off(slot, H, Tpad, feat, pos); }
extern "C" int skw_layout_kperm(int k) { return skw_kperm(k); }
// the q8 image of cross_kv = q8_0 (include/skw_kv8.h), in bytes: the int8 / the f16 block scale of K[key][feat] and of V[key][feat], and a slot's size
extern "C" long skw_layout_kv8_kq_off(int slot, int H, int Tpad, int key, int feat) { return skw_kv8_kq_off(slot, H, Tpad, key, feat); }
extern "C" long skw_layout_kv8_kd_off(int slot, int H, int Tpad, int key, int feat) { return skw_kv8_kd_off(slot, H, Tpad, key, feat); }
extern "C" long skw_layout_kv8_vq_off(int slot, int H, int Tpad, int feat, int key) { return skw_kv8_vq_off(slot, H, Tpad, feat, key); }
extern "C" long skw_layout_kv8_vd_off(int slot, int H, int Tpad, int feat, int key) { return skw_kv8_vd_off(slot, H, Tpad, feat, key); }
extern "C" long skw_layout_kv8_slot_bytes(int H, int Tpad) { return skw_kv8_slot_bytes(H, Tpad); }
extern "C" long skw_layout_afrag_off(int m, int p, int K) { return skw_afrag_off(m, p, K); }

// ------------------------------------------------------------------ the hooks' scaffold
// One call's device allocations and its error text.  Whatever a hook allocates is freed when the call returns, on every path; ok() / bad() write "<entry>: <what>" into errbuf.
struct HookBufs {
    char* errbuf; const char* who; std::vector<void*> dev;
    HookBufs(char* errbuf_, const char* entry) : errbuf(errbuf_), who(entry) {}
    HookBufs(const HookBufs&) = delete; HookBufs& operator=(const HookBufs&) = delete;
    ~HookBufs() { for (void* p : dev) hipFree(p); }
    int bad(const char* what) { if (errbuf) snprintf(errbuf, 512, "%s: %s", who, what); return -1; }
    bool ok(hipError_t e) { if (e != hipSuccess) { bad(hipGetErrorString(e)); return false; } return true; }
    // n elements of T, uninitialised / a copy of host[0 .. n) / every byte `byte`; null on failure
    template <typename T> T* alloc(size_t n) { void* p = nullptr; if (!ok(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)))) return nullptr; dev.push_back(p); return (T*)p; }
    template <typename T> T* up(const T* host, size_t n) { T* p = alloc<T>(n); return p && (!n || ok(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice))) ? p : nullptr; }
    template <typename T> T* fill(int byte, size_t n) { T* p = alloc<T>(n); return p && ok(hipMemset(p, byte, n * sizeof(T))) ? p : nullptr; }
    template <typename T> bool down(T* host, const T* d, size_t n) { return ok(hipMemcpy(host, d, n * sizeof(T), hipMemcpyDeviceToHost)); }
    bool ran(hipStream_t stream) { return ok(hipStreamSynchronize(stream)) && ok(hipGetLastError()); }      // the launches finished, and none was refused
    // The rows' SkwSeqState array on the device: row r = (active, pad = its sequence, cur_pos, n_keys) from the arrays given, a null array standing for 1 / r / 0 / 0.  A launch
    // takes &st[0].active / .pad / .cur_pos / .n_keys, so the fields reach the kernel with the real struct stride (the launchers' contract)
    SkwSeqState* seq_rows(int rows, const int* active, const int* seq, const int* pos, const int* n_keys) {
        std::vector<SkwSeqState> st(rows); memset((void*)st.data(), 0, sizeof(SkwSeqState) * rows);
        for (int r = 0; r < rows; ++r) { st[r].active = active ? active[r] : 1; st[r].pad = seq ? seq[r] : r; st[r].cur_pos = pos ? pos[r] : 0; st[r].n_keys = n_keys ? n_keys[r] : 0; }
        return up(st.data(), (size_t)rows);
    }
    // the prompt pass's sequences and the slots' key counts in one block of 4 x 64 ints: row0 | nq | slot | slot_k (null arrays: zeros)
    int* seq_meta(int n_seq, const int* row0, const int* nq, const int* slot, int n_slots, const int* slot_k) {
        int meta[4 * 64] = {0};
        for (int i = 0; i < n_seq; ++i) { meta[i] = row0[i]; meta[64 + i] = nq[i]; meta[128 + i] = slot[i]; }
        if (slot_k) for (int s = 0; s < n_slots; ++s) meta[192 + s] = slot_k[s];
        return up(meta, (size_t)4 * 64);
    }
};
// f16 output rows as an attention kernel leaves them (features in kperm order; ofrag: the fragment-order image) -> natural order, f32
static void unpermute_f16(const std::vector<uint16_t>& o, int rows, int d, int ofrag, float* out) {
    for (int r = 0; r < rows; ++r) for (int n = 0; n < d; ++n) out[(size_t)r * d + n] = skw_f16_to_f32(o[ofrag ? (size_t)skw_afrag_off(r, skw_kperm(n), d) : (size_t)r * d + skw_kperm(n)]);
}
// what up_q pushed onto the model's allocation list since `before` is the call's, not the model's: freed and popped when the call returns
struct ModelAllocsGuard {
    skw_model* m; size_t before;
    explicit ModelAllocsGuard(skw_model* m_) : m(m_), before(m_->allocs.size()) {}
    ~ModelAllocsGuard() { while (m->allocs.size() > before) { hipFree(m->allocs.back()); m->allocs.pop_back(); } }
};

// tests: the fragment-order image of a host weight [N][K] (f16 bits), as the decode kernels read it (skw_make_wfrag)
extern "C" int skw_debug_make_wfrag(const uint16_t* w_host, int N, int K, int perm, uint16_t* img_host) {
    if (N <= 0 || K <= 0 || (K & 31)) return -1;
    const size_t n_in = (size_t)N * K, n_out = (size_t)((N + 15) & ~15) * K;
    HookBufs b(nullptr, "skw_debug_make_wfrag");
    half_t *dw = b.alloc<half_t>(n_in), *di = b.alloc<half_t>(n_out);
    if (!dw || !di) return -2;
    if (hipMemcpy(dw, w_host, n_in * 2, hipMemcpyHostToDevice) != hipSuccess || hipMemset(di, 0xff, n_out * 2) != hipSuccess) return -3;
    skw_make_wfrag(dw, K, N & ~15, K, perm, di, nullptr);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(img_host, di, (size_t)(N & ~15) * K * 2, hipMemcpyDeviceToHost) != hipSuccess) return -4;
    return 0;
}

// ------------------------------------------------------------------ arithmetic-contract probes (tests/test_gpu_math.py)
__global__ void k_math_probe(int kind, const float* in, float* out, long n, const uint16_t* gelu_tab) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    float x = in[i], y;
    if (kind == 0) y = skw_expf(x);
    else if (kind == 1) y = skw_logf(x);
    else if (kind == 2) y = (float)((half_t)x);
    else if (kind == 3) y = skw_round_f16(x);
    else if (kind == 4) { if (x <= -10.0f) y = 0.0f; else if (x >= 10.0f) y = x; else { half_t h = (half_t)x; uint16_t b = __builtin_bit_cast(uint16_t, h);
    uint16_t o = gelu_tab[b]; y = (float)__builtin_bit_cast(half_t, o); } }
    else if (kind == 5) y = 1.0f / sqrtf(x + 1e-5f);
    else if (kind == 6) y = (float)(1.0 / (double)x);
    else y = (float)log10((double)x);
    out[i] = y;
}
extern "C" int skw_debug_math(skw_ctx* c, int kind, const float* in, float* out, long n) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_math");
    float *di = b.up(in, (size_t)n), *dout = b.alloc<float>((size_t)n);
    if (!di || !dout) return -1;
    hipLaunchKernelGGL(k_math_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, kind, di, dout, n, c->m->gelu_tab);
    HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipMemcpy(out, dout, n * 4, hipMemcpyDeviceToHost)); return 0;
}

// measurement hook (tools/gemm16_probe.py): one f16-MFMA GEMM of the given shape on scratch buffers, timed with HIP events on the engine stream.
// probe: bit 0 no K-loop DMA, bit 1 no MFMAs, bit 2 no epilogue stores; epi: EPI_* of skw_kernels.h (n_ctx / H / Tpad taken from the model)
extern "C" int skw_debug_gemm16(skw_ctx* c, int M, int N, int K, int epi, int probe, int iters, float* ms_per_launch) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_gemm16");
    const size_t cbytes = (size_t)M * N * 4 + (size_t)64 * c->Tpad * N;
    // probe bits 12-19 = n (decode shapes): the launches walk n copies of W (n x N x K x 2 bytes > the 256 MB Infinity Cache: every launch finds its weights in HBM, as a decode step does)
    const int wcycle = M <= 64 ? std::max(1, (probe >> 12) & 255) : 1; if (M <= 64) probe &= 0xfff;      // (big shapes: bits 10-16 are k_gemm16w's measurement hooks)
    half_t *A = b.alloc<half_t>((size_t)M * K), *W = b.alloc<half_t>((size_t)N * K * wcycle); void* C = b.alloc<char>(cbytes);
    float *bias = b.fill<float>(0, (size_t)std::max(M, N)), *res = b.fill<float>(0, (size_t)M * N);
    if (!A || !W || !C || !bias || !res) return -1;
    { std::vector<uint16_t> h((size_t)std::max(M, N) * K); uint32_t x = 12345; for (auto& v : h) { x = x * 1664525u + 1013904223u; v = skw_f32_to_f16(((x >> 8) & 0xffff) / 65536.0f - 0.5f); }
      HIPCHK(hipMemcpy(A, h.data(), (size_t)M * K * 2, hipMemcpyHostToDevice));
      for (int w = 0; w < wcycle; ++w) HIPCHK(hipMemcpy(W + (size_t)w * N * K, h.data(), (size_t)N * K * 2, hipMemcpyHostToDevice)); }
    SkwGemmArgs a{}; a.A = A; a.lda = K; a.W = W; a.ldw = K; a.M = M; a.N = N; a.K = K; a.C = C; a.ldc = N; a.bias = bias; a.epi = epi; a.scale = 1.0f; a.probe = probe;
    a.gelu_tab = c->m->gelu_tab; a.pe = res; a.n_ctx = c->m->hp.n_audio_ctx; a.H = N / 64; a.Tpad = c->Tpad; if (epi == EPI_F32 && N < 8192) { a.res = res; a.ldres = N; }
    if (N >= 8192) a.bias = nullptr;                               // the vocabulary projection: no bias, no residual
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    const bool small = M <= 64;                                      // the decode-step form: a chain of dependent launches, so the figure includes the kernel boundary
    if (small && epi == EPI_DEC_QKV) { a.C2 = res; a.C3 = res; a.ldc2 = N; a.n_ctx = N / 3; a.ldc = N / 3; }
    if (small && (probe & 64) && !(M & 15)) { a.a_frag = 1; a.probe &= ~64; }      // probe bit 6 (decode shapes, timing only): the activations addressed as a fragment-order image
    half_t* Wfrag = nullptr;      // probe bit 5 (decode shapes): the weights as fragment-order images (one per W copy of the cycle), what the step's launches read
    if (small && (probe & 32) && !(N & 15)) { if (!(Wfrag = b.alloc<half_t>((size_t)N * K * wcycle))) return -1;
    for (int w = 0; w < wcycle; ++w) skw_make_wfrag(W + (size_t)w * N * K, K, N, K, epi == EPI_GELU_F16_KPERM, Wfrag + (size_t)w * N * K, c->stream);
    a.Wf = Wfrag; a.probe &= ~32; }
    // probe bit 9 (big shapes): the weights also as a fragment-order image and no measurement hooks — the launch takes k_gemm16w, as the encoder's do
    if (!small && (probe & 512) && !(N & 15)) {
        if (!(Wfrag = b.alloc<half_t>((size_t)N * K))) return -1;
        skw_make_wfrag(W, K, N, K, epi == EPI_GELU_F16_KPERM || epi == EPI_HEADS_F16, Wfrag, c->stream);
        a.Wf = Wfrag; a.probe = probe & ~1023;
    }
    for (int i = 0; i < 3; ++i) { if (small) skw_gemm16_small(a, c->stream); else skw_gemm16(a, c->stream); }
    HIPCHK(hipEventRecord(e0, c->stream));
    // (a launch that also touched the NEXT launch's copy of W — LDS-DMA into a scratch slab, so the bytes sit in the Infinity Cache when wanted — measured no gain:
    //  7.63 vs 7.66 us for the QKV shape.  The cold-weight cost is the transfer into the consuming XCD's L2, ~1 us per 3.5 MB whether it starts in HBM or in the Infinity Cache.)
    for (int i = 0; i < iters; ++i) { a.W = W + (size_t)(i % wcycle) * N * K;
    if (Wfrag) a.Wf = Wfrag + (size_t)(i % wcycle) * N * K; if (small) skw_gemm16_small(a, c->stream); else skw_gemm16(a, c->stream); }
    HIPCHK(hipEventRecord(e1, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
    float ms = 0; hipEventElapsedTime(&ms, e0, e1); *ms_per_launch = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return 0;
}

// tests (tests/test_gpu_gemm16w.py; the regression cover of the round-4 k_gemm16w fault): ONE product on seeded operands through k_gemm16w — the encoder's GEMM, weights from a
// fragment-order image, two memory queues counted by hand — and through k_gemm16 (both operands through LDS), every output byte compared.  epi: EPI_* of skw_kernels.h;
// frag: EPI_F16_PLAIN / EPI_VT_F16 write the fragment-order cross K / V^T image; n_ctx / Tpad: rows per clip of the per-clip layouts (M must be a multiple of n_ctx for them);
// ngroups: GEMM16W_NGROUPS for the k_gemm16w launch; with_res: EPI_F32 adds a residual.  Returns the number of differing bytes (0 = bit-identical), -2 when skw_gemm16 would not
// take k_gemm16w for this geometry (nothing compared), -1 on error.
extern "C" long skw_debug_gemm16_compare(skw_ctx* c, int M, int N, int K, int epi, int frag, int n_ctx, int Tpad, int ngroups, int with_res) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_gemm16_compare");
    if (M < 1 || N < 16 || (N & 15) || (K & 63) || n_ctx < 1 || (Tpad & 31) || Tpad < n_ctx) return b.bad("bad geometry");
    const bool per_clip = epi == EPI_HEADS_F16 || epi == EPI_VT_F16 || epi == EPI_GELU_F16_KPERM_ROWPAD || epi == EPI_CONV2 || frag;
    if (per_clip && M % n_ctx) return b.bad("M must be whole clips for this epilogue");
    if ((epi == EPI_HEADS_F16 || epi == EPI_VT_F16 || frag) && (N & 63)) return b.bad("N must be whole heads for this epilogue");
    const size_t cbytes = ((size_t)(M / n_ctx + 2) * (Tpad + 2) * N + (size_t)M * N) * 4 + 4096;
    half_t *A, *W, *Wf = b.alloc<half_t>((size_t)N * K); float *bias, *res, *pe;
    {   // seeded operands: values of order 1 / sqrt(K) so that sums stay well inside f16's range after the epilogue
        uint32_t x = 0x9e3779b9u ^ (uint32_t)(M * 31 + N * 17 + K * 7 + epi);
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return ((x >> 8) & 0xffff) / 65536.0f - 0.5f; };
        const float sc = 2.0f / sqrtf((float)K);
        std::vector<uint16_t> h((size_t)std::max(M, N) * K);
        for (auto& v : h) v = skw_f32_to_f16(rnd() * sc);
        A = (half_t*)b.up(h.data(), (size_t)M * K);
        for (auto& v : h) v = skw_f32_to_f16(rnd() * 2.0f);
        W = (half_t*)b.up(h.data(), (size_t)N * K);
        std::vector<float> f((size_t)std::max((size_t)M * N, (size_t)n_ctx * N));
        for (auto& v : f) v = rnd();
        res = b.up(f.data(), (size_t)M * N); pe = b.up(f.data(), (size_t)n_ctx * N); bias = b.up(f.data(), (size_t)std::max(M, N));
    }
    if (!Wf || !A || !W || !res || !pe || !bias) return -1;
    const bool perm = epi == EPI_F16_KPERM || epi == EPI_GELU_F16_KPERM || epi == EPI_GELU_F16_KPERM_ROWPAD || epi == EPI_HEADS_F16;
    skw_make_wfrag(W, K, N, K, perm ? 1 : 0, Wf, c->stream);
    SkwGemmArgs a{}; a.A = A; a.lda = K; a.W = W; a.ldw = K; a.Wf = Wf; a.M = M; a.N = N; a.K = K; a.ldc = N; a.bias = bias; a.epi = epi; a.scale = 0.125f;
    a.has_scale = (epi == EPI_F16_KPERM || epi == EPI_HEADS_F16 || epi == EPI_F16_PLAIN) ? 1 : 0;
    a.gelu_tab = c->m->gelu_tab; a.pe = pe; a.n_ctx = per_clip ? n_ctx : 0; a.H = N / 64; a.Tpad = Tpad; a.frag = frag;
    if (epi == EPI_F32 && with_res) { a.res = res; a.ldres = N; }
    if (!skw_gemm16_takes_w(a)) return -2;
    char *C1 = b.alloc<char>(cbytes), *C2 = b.alloc<char>(cbytes);
    if (!C1 || !C2 || !b.ok(hipMemsetAsync(C1, 0xAB, cbytes, c->stream)) || !b.ok(hipMemsetAsync(C2, 0xAB, cbytes, c->stream))) return -1;
    {
        SwOverride w(SW_GEMM16W, 1), ng(SW_GEMM16W_NGROUPS, ngroups);
        a.C = C1; skw_gemm16(a, c->stream);
        w.set(0); a.C = C2; skw_gemm16(a, c->stream);
    }
    if (!b.ran(c->stream)) return -1;
    std::vector<char> h1(cbytes), h2(cbytes);
    if (!b.down(h1.data(), C1, cbytes) || !b.down(h2.data(), C2, cbytes)) return -1;
    long diff = 0, written = 0;
    for (size_t i = 0; i < cbytes; ++i) { diff += h1[i] != h2[i]; written += (unsigned char)h2[i] != 0xAB; }
    if (written < (long)M * N) { snprintf(errbuf, 512, "skw_debug_gemm16_compare: only %ld bytes written for %d x %d outputs", written, M, N); return -1; }
    return diff;
}

// tests (tests/test_gpu_mfma_model.py): P independent v_mfma_f32_16x16x32_f16 instructions — A: P x [16][32] f16 (row i, slot k), B: P x [32][16] f16 (slot k, column j), C / D: P x [16][16] f32 —
// what the committed hardware vectors (tests/golden/mfma_f16_hw_vectors.npz) were taken with and are re-taken with on every GPU run
__global__ void k_debug_mfma16x32(const half_t* A, const half_t* B, const float* C, float* D) {
    const int p = blockIdx.x, l = threadIdx.x, r16 = l & 15, g = l >> 4;
    const half_t* a = A + (size_t)p * 512; const half_t* b = B + (size_t)p * 512; const float* c = C + (size_t)p * 256; float* d = D + (size_t)p * 256;
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f16x8 fa, fb;
    for (int e = 0; e < 8; ++e) { fa[e] = a[r16 * 32 + 8 * g + e]; fb[e] = b[(8 * g + e) * 16 + r16]; }      // lane (row / column r16, group g) holds slots 8 g .. 8 g + 7
    f32x4 acc; for (int r = 0; r < 4; ++r) acc[r] = c[(4 * g + r) * 16 + r16];
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, fb, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) d[(4 * g + r) * 16 + r16] = acc[r];
}
extern "C" int skw_debug_mfma16x32(skw_ctx* c, long P, const uint16_t* A_host, const uint16_t* B_host, const float* C_host, float* D_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_mfma16x32");
    if (P < 1 || P > (1 << 20)) return b.bad("bad problem count");
    char* buf = b.alloc<char>((size_t)P * 4096);
    if (!buf) return -1;
    half_t* A = (half_t*)buf; half_t* B = (half_t*)(buf + P * 1024); float* C = (float*)(buf + P * 2048); float* D = (float*)(buf + P * 3072);
    if (!b.ok(hipMemcpy(A, A_host, P * 1024, hipMemcpyHostToDevice)) || !b.ok(hipMemcpy(B, B_host, P * 1024, hipMemcpyHostToDevice))) return -1;
    if (!b.ok(hipMemcpy(C, C_host, P * 1024, hipMemcpyHostToDevice))) return -1;
    hipLaunchKernelGGL(k_debug_mfma16x32, dim3((unsigned)P), dim3(64), 0, c->stream, A, B, C, D);
    if (!b.ran(c->stream) || !b.down(D_host, D, (size_t)P * 256)) return -1;
    return 0;
}
// tests (tests/test_gpu_mfma_model.py): C = A . W^T through one of the f16_mfma GEMM kernels, plain f32 epilogue (no bias, no residual), operands given as f16 bit patterns in the
// kernels' memory order ([M][K] and [N][K], K axis as the kernels load it) — to be compared bit for bit with oracle/'s restatement of the matrix cores (skwo_gemm_f16mfma).
// kernel: 0 = k_gemm16w (weights from a fragment-order image), 1 = k_gemm16 (both operands through LDS), 2 = the decode step's product: k_gemm16_small (four waves split K) for N < 8192,
// k_gemm16_vocab (one wave chains the whole K) from there on
extern "C" int skw_debug_gemm16_out(skw_ctx* c, int kernel, int M, int N, int K, const uint16_t* A_host, const uint16_t* W_host, float* C_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_gemm16_out");
    if (M < 1 || (N & 15) || (K & 127) || kernel < 0 || kernel > 2) return b.bad("bad geometry");
    half_t *A = (half_t*)b.up(A_host, (size_t)M * K), *W = (half_t*)b.up(W_host, (size_t)N * K), *Wf = b.alloc<half_t>((size_t)N * K); float* C = b.fill<float>(0xAB, (size_t)M * N);
    if (!A || !W || !Wf || !C) return -1;
    skw_make_wfrag(W, K, N, K, 0, Wf, c->stream);
    SkwGemmArgs a{}; a.A = A; a.lda = K; a.W = W; a.ldw = K; a.M = M; a.N = N; a.K = K; a.C = C; a.ldc = N; a.epi = EPI_F32; a.scale = 1.0f;
    if (kernel == 2) { a.Wf = Wf; if (!skw_gemm16_small(a, c->stream)) return b.bad("k_gemm16_small does not take this geometry"); }
    else {
        a.Wf = kernel == 0 ? Wf : nullptr; SwOverride w(SW_GEMM16W, kernel == 0 ? 1 : 0);
        if (kernel == 0 && !skw_gemm16_takes_w(a)) return b.bad("k_gemm16w does not take this geometry");
        skw_gemm16(a, c->stream);
    }
    if (!b.ran(c->stream) || !b.down(C_host, C, (size_t)M * N)) return -1;
    return 0;
}

// The packing the attention hooks below share: natural-order f16 bit patterns -> what a kernel reads.  Q [n_slots][n_ctx][H*64] into per-head rows of stride Tpad (qheads; a plain
// Q is copied as it stands, q.size() halves), K / V [n_slots][n_ctx][H*64] into per-head rows (kheads), the fragment-order images (kfrag / vfrag), plain rows (K otherwise; vrows) or
// V^T per head in kperm key order (V otherwise).  q / k / v arrive sized and filled with the caller's pad patterns; only keys below fill_from[slot] are written.
struct AttnHookLayout { int qheads, kheads, kfrag, vrows, vfrag; };
static void attn_hook_pack(const AttnHookLayout& L, int H, int n_ctx, int n_slots, const uint16_t* Q_host, const uint16_t* K_host, const uint16_t* V_host, const int* fill_from,
                           std::vector<uint16_t>& q, std::vector<uint16_t>& k, std::vector<uint16_t>& v) {
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31;
    if (L.qheads) { for (int s = 0; s < n_slots; ++s) for (int i = 0; i < n_ctx; ++i) for (int n = 0; n < d; ++n)
                        q[(((size_t)s * H + (n >> 6)) * Tpad + i) * 64 + skw_kperm(n & 63)] = Q_host[((size_t)s * n_ctx + i) * d + n]; }
    else memcpy(q.data(), Q_host, q.size() * 2);
    for (int s = 0; s < n_slots; ++s) for (int i = 0; i < fill_from[s]; ++i) for (int n = 0; n < d; ++n) {
        const uint16_t kv = K_host[((size_t)s * n_ctx + i) * d + n], vv = V_host[((size_t)s * n_ctx + i) * d + n];
        const int p = skw_kperm(i);
        if (L.kheads) k[(((size_t)s * H + (n >> 6)) * Tpad + i) * 64 + skw_kperm(n & 63)] = kv;
        else if (L.kfrag) k[skw_kfrag_off(s, H, Tpad, i, n & ~7) + (n & 7)] = kv;
        else k[((size_t)s * n_ctx + i) * d + n] = kv;
        if (L.vrows) v[((size_t)s * n_ctx + i) * d + n] = vv;
        else if (L.vfrag) v[skw_vtfrag_off(s, H, Tpad, n, p & ~7) + (p & 7)] = vv;
        else v[((size_t)s * d + n) * Tpad + p] = vv;
    }
}

// tests (tests/test_gpu_attn16.py): one f16_mfma attention launcher on host-supplied operands, to be held to a float64 softmax(Q K^T) V kernel by kernel.  Q [rows][H*64], K / V
// [slot][n_ctx][H*64] arrive as f16 bit patterns in NATURAL order; this packs them into what the kernel reads (per-head rows of stride Tpad, V^T, the fragment-order images), launches
// through the public launcher (the template dispatch is part of what is tested) and returns the output un-permuted as f32 [rows][H*64].
//   form 0  skw_attn_encoder16: Q is [slot][n_ctx][H*64]; slot_k null: out rows = n_slots * n_ctx; given: n_slots * out_rows (out_rows 0: n_ctx)
//   form 1  skw_xattn_prefill16: n_seq sequences (row0, nq, slot), frag = flags & 1, ofrag = flags & 2, slot_k null or [n_slots]
//   form 2  skw_dec_cross_attn_vt, pv16 = 2 (one pass over the fragment-order images), ofrag = flags & 2;   form 3  the same, pv16 = 1 (two phases over the row layouts)
//           active / seq / count (= n_keys) are [rows] or null and reach the kernel as fields of a SkwSeqState array (its stride is the launchers' contract)
//   form 4  skw_dec_self_attn, fastv = 1: K / V are the caches [slot][n_ctx = n_text_ctx][H*64], count = pos [rows] (required), ofrag = flags & 2
// Pad: every K position of slot s from fill_from[s] up (to Tpad where the layout has a Tpad) holds the bit pattern k_pad, every V position v_pad — what the kernel must not use is the
// caller's to poison.  The output buffer starts as `sentinel` in every half, so rows the kernel must leave alone (inactive, past nq, past a slot's queries) are visible.
extern "C" int skw_debug_attn16(skw_ctx* c, int form, int H, int n_ctx, int n_slots, int rows, int flags, int out_rows, const uint16_t* Q_host, const uint16_t* K_host,
                                const uint16_t* V_host, const int* fill_from, int k_pad, int v_pad, const int* slot_k, int n_seq, const int* row0, const int* nq, const int* slot,
                                const int* active, const int* seq, const int* count, int sentinel, float* out_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_attn16"); auto bad = [&](const char* what) { return b.bad(what); };
    if (form < 0 || form > 4 || H < 1 || H > 32 || n_ctx < 1 || n_ctx > 4096 || n_slots < 1 || n_slots > 64 || rows < 1 || rows > 65536 || !fill_from) return bad("bad geometry");
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31, frag = flags & 1, ofrag = (flags >> 1) & 1;
    for (int s = 0; s < n_slots; ++s) if (fill_from[s] < 0 || fill_from[s] > n_ctx) return bad("fill_from outside [0, n_ctx]");
    int orows = rows, nq_max = 0;
    if (form == 0) {
        orows = n_slots * (slot_k && out_rows ? out_rows : n_ctx);
        if (slot_k) for (int s = 0; s < n_slots; ++s) if ((out_rows ? out_rows : n_ctx) < std::min(n_ctx, std::max(1, slot_k[s]))) return bad("out_rows below a slot's query count");
        if (ofrag || frag) return bad("the encoder form has no frag / ofrag");
    } else if (form == 1) {
        if (n_seq < 1 || n_seq > 64 || !row0 || !nq || !slot) return bad("the prompt pass needs row0 / nq / slot");
        for (int i = 0; i < n_seq; ++i) {
            if (row0[i] < 0 || nq[i] < 0 || row0[i] + nq[i] > rows || slot[i] < 0 || slot[i] >= n_slots) return bad("a sequence's rows or slot lie outside the buffers");
            nq_max = std::max(nq_max, nq[i]);
        }
        if (nq_max < 1) return bad("no queries");
    } else {
        if (form == 3 && n_ctx > 24 * 64) return bad("the two-phase kernel holds at most 1536 keys");
        if (form == 4 && (n_ctx > 7 * 64 || !count)) return bad("the self-attention form needs pos and n_text_ctx <= 448");
        if (form == 4 && !skw_sw(SW_DEC_ATTN_FASTV)) return bad("SKW_DEC_ATTN_FASTV is off: the launcher would not reach the FASTV form");
        if (frag || (ofrag && form == 3)) return bad("flag does not apply to this form");
        for (int b = 0; b < rows; ++b) {
            const int s = seq ? seq[b] : b;
            if (s < 0 || s >= n_slots) return bad("a row's sequence lies outside the slots");
            if (form == 4 && (count[b] < 0 || count[b] >= n_ctx)) return bad("pos outside the cache");
        }
    }
    const int kfrag = (form == 1 && frag) || form == 2, vfrag = kfrag, kheads = form == 0, vrows = form == 4;      // which layouts this form reads
    const int kkeys = (kfrag || kheads) ? Tpad : n_ctx, vkeys = vrows ? n_ctx : Tpad;
    const size_t nQ = form == 0 ? (size_t)n_slots * Tpad * d : (size_t)rows * d, nK = (size_t)n_slots * kkeys * d, nV = (size_t)n_slots * vkeys * d;
    const size_t nO = (size_t)(ofrag ? (orows + 15) & ~15 : orows) * d;
    std::vector<uint16_t> q(nQ, (uint16_t)k_pad), k(nK, (uint16_t)k_pad), v(nV, (uint16_t)v_pad), o(nO, (uint16_t)sentinel);
    attn_hook_pack(AttnHookLayout{form == 0, kheads, kfrag, vrows, vfrag}, H, n_ctx, n_slots, Q_host, K_host, V_host, fill_from, q, k, v);
    half_t *dq = (half_t*)b.up(q.data(), nQ), *dk = (half_t*)b.up(k.data(), nK), *dv = (half_t*)b.up(v.data(), nV), *dout = (half_t*)b.up(o.data(), nO);
    SkwSeqState* dst = form >= 2 ? b.seq_rows(rows, active, seq, form == 4 ? count : nullptr, form == 4 ? nullptr : count) : b.fill<SkwSeqState>(0, (size_t)rows);
    int* dmeta = b.seq_meta(form == 1 ? n_seq : 0, row0, nq, slot, n_slots, slot_k);
    if (!dq || !dk || !dv || !dout || !dst || !dmeta) return -1;
    const int* dslot_k = slot_k ? dmeta + 192 : nullptr;
    if (form == 0) skw_attn_encoder16(dq, dk, dv, dout, d, n_slots, H, n_ctx, Tpad, c->stream, dslot_k, out_rows);
    else if (form == 1) skw_xattn_prefill16(dq, dk, dv, dout, n_seq, nq_max, dmeta, dmeta + 64, dmeta + 128, H, d, n_ctx, Tpad, c->stream, frag, ofrag, dslot_k);
    else if (form == 4) skw_dec_self_attn(dq, dk, dv, &dst[0].cur_pos, rows, H, d, n_ctx, dout, active ? &dst[0].active : nullptr, c->stream, 0, SkwQ8Out{nullptr, nullptr, nullptr, 0},
                                          seq ? &dst[0].pad : nullptr, 1, ofrag);
    else skw_dec_cross_attn_vt(dq, dk, dv, rows, H, d, n_ctx, Tpad, dout, active ? &dst[0].active : nullptr, c->stream, 0, form == 2 ? 2 : 1, seq ? &dst[0].pad : nullptr, nullptr, nullptr,
                               ofrag, nullptr, count ? &dst[0].n_keys : nullptr);
    if (!b.ran(c->stream) || !b.down(o.data(), (const uint16_t*)dout, nO)) return -1;
    unpermute_f16(o, orows, d, ofrag, out_host);
    return 0;
}

// tests (tests/test_gpu_kv8.py): the two kernels of cross_kv = q8_0 on host-supplied operands, in the style of skw_debug_attn16 (whose packing, pads and sentinel these share).
// K / V [slot][n_ctx][H*64] arrive as f16 bit patterns in natural order and become the f16 fragment-order images, pad patterns from fill_from[s] up; slot_k (null: n_ctx) are the
// quantiser's key counts per slot.  The q8 image starts as the byte 0xEE, so what k_kv8_quantize does not write is visible.
// -> the q8 image on the device (b's, *img_bytes long), the quantise kernel launched on it; null: b.bad said why
static uint8_t* kv8_hook_quantize(skw_ctx* c, HookBufs& b, int H, int n_ctx, int n_slots, const uint16_t* K_host, const uint16_t* V_host, const int* fill_from, int k_pad, int v_pad,
                                  const int* slot_k, size_t* img_bytes) {
    auto bad = [&](const char* what) { b.bad(what); return (uint8_t*)nullptr; };
    if (H < 1 || H > 32 || n_ctx < 1 || n_ctx > 4096 || n_slots < 1 || n_slots > 64 || !fill_from || !K_host || !V_host) return bad("bad geometry");
    for (int s = 0; s < n_slots; ++s) if (fill_from[s] < 0 || fill_from[s] > n_ctx || (slot_k && (slot_k[s] < 1 || slot_k[s] > n_ctx))) return bad("fill_from / slot_k outside the slot");
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31; const size_t nKV = (size_t)n_slots * Tpad * d;
    std::vector<uint16_t> q(1), k(nKV, (uint16_t)k_pad), v(nKV, (uint16_t)v_pad);
    const uint16_t q0 = 0;
    attn_hook_pack(AttnHookLayout{0, 0, 1, 0, 1}, H, n_ctx, n_slots, &q0, K_host, V_host, fill_from, q, k, v);
    *img_bytes = (size_t)n_slots * skw_kv8_slot_bytes(H, Tpad);
    half_t *dk = b.alloc<half_t>(nKV), *dv = b.alloc<half_t>(nKV); uint8_t* img = b.alloc<uint8_t>(*img_bytes); int* dslot_k = b.alloc<int>(64);
    if (!dk || !dv || !img || !dslot_k) return bad("device allocation failed");
    int sk[64] = {0}; if (slot_k) for (int s = 0; s < n_slots; ++s) sk[s] = slot_k[s];
    if (hipMemcpy(dk, k.data(), nKV * 2, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dv, v.data(), nKV * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(img, 0xEE, *img_bytes) != hipSuccess || hipMemcpy(dslot_k, sk, sizeof sk, hipMemcpyHostToDevice) != hipSuccess) return bad("copy to the device failed");
    skw_kv8_quantize(dk, dv, img, 0, n_slots, H, n_ctx, Tpad, slot_k ? dslot_k : nullptr, c->stream);
    return img;
}
// -> img_host [n_slots * skw_layout_kv8_slot_bytes(H, Tpad)]: the image as the kernel wrote it
extern "C" int skw_debug_kv8_quantize(skw_ctx* c, int H, int n_ctx, int n_slots, const uint16_t* K_host, const uint16_t* V_host, const int* fill_from, int k_pad, int v_pad,
                                      const int* slot_k, uint8_t* img_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_kv8_quantize"); size_t img_bytes = 0;
    const uint8_t* img = kv8_hook_quantize(c, b, H, n_ctx, n_slots, K_host, V_host, fill_from, k_pad, v_pad, slot_k, &img_bytes);
    if (!img) return -1;
    HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(img_host, img, img_bytes, hipMemcpyDeviceToHost));
    return 0;
}
// The quantise kernel, then skw_dec_cross_attn_kv8 through its launcher.  Q [rows][H*64]; active / seq / count (= n_keys) are [rows] or null and reach the kernel as fields of a
// SkwSeqState array.  flags: 2 ofrag, 4 f32_out (the output rows unrounded), 8 raw.  out_host: f32 [rows][H*64] in natural order — rows the kernel leaves alone hold `sentinel`
// (as f16; with f32_out the 32-bit pattern sentinel | sentinel << 16) — or, raw, the f32 scores [rows][H][n_ctx], NaN where nothing was written.
extern "C" int skw_debug_attn_kv8(skw_ctx* c, int H, int n_ctx, int n_slots, int rows, int flags, const uint16_t* Q_host, const uint16_t* K_host, const uint16_t* V_host,
                                  const int* fill_from, int k_pad, int v_pad, const int* slot_k, const int* active, const int* seq, const int* count, int sentinel, float* out_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_attn_kv8"); auto bad = [&](const char* what) { return b.bad(what); };
    if (rows < 1 || rows > 65536 || !Q_host || !out_host) return bad("bad geometry");
    const int ofrag = (flags >> 1) & 1, f32_out = (flags >> 2) & 1, raw = (flags >> 3) & 1;
    if (ofrag && f32_out) return bad("ofrag and f32_out exclude each other");
    size_t img_bytes = 0;
    const uint8_t* img = kv8_hook_quantize(c, b, H, n_ctx, n_slots, K_host, V_host, fill_from, k_pad, v_pad, slot_k, &img_bytes);
    if (!img) return -1;
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31;
    for (int r = 0; r < rows; ++r) {
        const int s = seq ? seq[r] : r;
        if (s < 0 || s >= n_slots) return bad("a row's sequence lies outside the slots");
        if (count && (count[r] < 0 || count[r] > (slot_k ? slot_k[s] : n_ctx))) return bad("a row's key count lies beyond what its slot was quantised with");
    }
    const size_t nO = (size_t)(ofrag ? (rows + 15) & ~15 : rows) * d * (f32_out ? 2 : 1), nR = raw ? (size_t)rows * H * n_ctx : 1;
    std::vector<uint16_t> o(nO, (uint16_t)sentinel);
    half_t *dq = (half_t*)b.up(Q_host, (size_t)rows * d), *dout = (half_t*)b.up(o.data(), nO); SkwSeqState* dst = b.seq_rows(rows, active, seq, nullptr, count);
    float* draw = b.fill<float>(0xFF, nR);
    if (!dq || !dout || !dst || !draw) return -1;
    skw_dec_cross_attn_kv8(dq, img, rows, H, d, n_ctx, Tpad, dout, active ? &dst[0].active : nullptr, c->stream, f32_out, seq ? &dst[0].pad : nullptr, nullptr, nullptr, ofrag, nullptr,
                           count ? &dst[0].n_keys : nullptr, raw ? draw : nullptr);
    if (!b.ran(c->stream)) return -1;
    if (raw) return b.down(out_host, draw, nR) ? 0 : -1;
    if (!b.down(o.data(), (const uint16_t*)dout, nO)) return -1;
    if (f32_out) memcpy(out_host, o.data(), (size_t)rows * d * 4);
    else unpermute_f16(o, rows, d, ofrag, out_host);
    return 0;
}

// tests (tests/test_gpu_attn_exact.py): the two exact-precision attention launchers that skw_debug_xattn_exact does not reach, on host-supplied operands, to be held bit for bit to
// the numpy restatement of the contract (tests/attn_exact_ref_lib.py).  Operands, fill_from, k_pad / v_pad and the sentinel are skw_debug_attn16's (whose packing this shares).
//   form 0  skw_attn_encoder — the launcher, so its choice between k_attn_encoder and k_attn_encoder_v3 is part of what is tested; *kernel_id is what skw_attn_encoder_kernel, the
//           function the launcher branches on, answers for the launch.  Q is [slot][n_ctx][H*64]; slot_k null: out rows = n_slots * n_ctx; given ([n_slots], each in 1 .. n_ctx):
//           n_slots * out_rows (out_rows 0: n_ctx)
//   form 1  skw_dec_self_attn, fastv = 0, no q8 output (k_dec_attn<7>): Q [rows][H*64], K / V the caches [slot][n_ctx = n_text_ctx][H*64]; pos [rows] (required), active / seq
//           [rows] or null, reaching the kernel as fields of a SkwSeqState array; *kernel_id = -1
// out: orows x H*64 elements of 2 bytes (f16 bits), or 4 (f32_out: the kernel's unrounded f32 rows).  raw: the f16 rows as the kernel leaves them (kperm order); otherwise un-permuted.
extern "C" int skw_debug_attn_exact(skw_ctx* c, int form, int H, int n_ctx, int n_slots, int rows, int f32_out, int raw, int out_rows, const uint16_t* Q_host, const uint16_t* K_host,
                                    const uint16_t* V_host, const int* fill_from, int k_pad, int v_pad, const int* slot_k, const int* active, const int* seq, const int* pos, int sentinel,
                                    void* out_host, int* kernel_id) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_attn_exact"); auto bad = [&](const char* what) { return b.bad(what); };
    if (form < 0 || form > 1 || H < 1 || H > 32 || n_ctx < 1 || n_ctx > 4096 || n_slots < 1 || n_slots > 64 || rows < 1 || rows > 4096 || !fill_from || !Q_host || !K_host || !V_host ||
        !out_host || !kernel_id) return bad("bad geometry");
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31, esz = f32_out ? 2 : 1;      // (output element size in halves)
    for (int s = 0; s < n_slots; ++s) if (fill_from[s] < 0 || fill_from[s] > n_ctx) return bad("fill_from outside [0, n_ctx]");
    int orows = rows;
    if (form == 0) {
        if (slot_k) for (int s = 0; s < n_slots; ++s) if (slot_k[s] < 1 || slot_k[s] > n_ctx || (out_rows && out_rows < slot_k[s])) return bad("slot_k outside [1, n_ctx] or above out_rows");
        if (!slot_k && out_rows && out_rows != n_ctx) return bad("out_rows needs slot_k");
        if (out_rows < 0 || out_rows > 4096) return bad("out_rows outside [0, 4096]");
        orows = n_slots * (out_rows ? out_rows : n_ctx);
    } else {
        if (n_ctx > 7 * 64 || !pos) return bad("the self-attention form needs pos and n_text_ctx <= 448");
        for (int b = 0; b < rows; ++b) {
            const int s = seq ? seq[b] : b;
            if (s < 0 || s >= n_slots || pos[b] < 0 || pos[b] >= n_ctx) return bad("a row's sequence or pos lies outside the caches");
        }
    }
    const size_t nQ = form == 0 ? (size_t)n_slots * Tpad * d : (size_t)rows * d, nK = (size_t)n_slots * (form == 0 ? Tpad : n_ctx) * d, nV = nK, nO = (size_t)orows * d * esz;
    std::vector<uint16_t> q(nQ, (uint16_t)k_pad), k(nK, (uint16_t)k_pad), v(nV, (uint16_t)v_pad), o(nO, (uint16_t)sentinel);
    attn_hook_pack(AttnHookLayout{form == 0, form == 0, 0, form == 1, 0}, H, n_ctx, n_slots, Q_host, K_host, V_host, fill_from, q, k, v);
    half_t *dq = (half_t*)b.up(q.data(), nQ), *dk = (half_t*)b.up(k.data(), nK), *dv = (half_t*)b.up(v.data(), nV), *dout = (half_t*)b.up(o.data(), nO);
    SkwSeqState* dst = form == 1 ? b.seq_rows(rows, active, seq, pos, nullptr) : b.fill<SkwSeqState>(0, (size_t)rows);
    int* dmeta = b.seq_meta(0, nullptr, nullptr, nullptr, n_slots, slot_k);
    if (!dq || !dk || !dv || !dout || !dst || !dmeta) return -1;
    *kernel_id = -1;
    if (form == 0) {
        *kernel_id = skw_attn_encoder_kernel(n_ctx, Tpad, false, slot_k != nullptr);
        skw_attn_encoder(dq, dk, dv, dout, d, n_slots, H, n_ctx, Tpad, c->stream, nullptr, nullptr, f32_out ? 1 : 0, slot_k ? dmeta + 192 : nullptr, out_rows);
    } else skw_dec_self_attn(dq, dk, dv, &dst[0].cur_pos, rows, H, d, n_ctx, dout, active ? &dst[0].active : nullptr, c->stream, f32_out ? 1 : 0, SkwQ8Out{nullptr, nullptr, nullptr, 0},
                             seq ? &dst[0].pad : nullptr, 0, 0);
    if (!b.ran(c->stream) || !b.down(o.data(), (const uint16_t*)dout, nO)) return -1;
    if (f32_out || raw) memcpy(out_host, o.data(), nO * 2);
    else for (int r = 0; r < orows; ++r) for (int n = 0; n < d; ++n) ((uint16_t*)out_host)[(size_t)r * d + n] = o[(size_t)r * d + skw_kperm(n)];
    return 0;
}

// tests (tests/test_gpu_q8.py): one product of ggml's arithmetic for quantised files on host-supplied operands, through everything the engine itself goes through — the model
// loader's repack of the file's blocks (host_q / up_q), skw_q8_quantize on the f32 rows A [M][lda], then skw_gemm_q8 (so the dispatch is part of what is tested; *kernel_id is what
// skw_gemm_q8_kernel — the function the launcher branches on — answers for the launch's arguments).  The output buffers are the caller's: C (c_bytes; ldc elements per row where the
// epilogue has rows) and, for EPI_DEC_QKV, C2 / C3 (c2_bytes each, ldc2) are uploaded as given — a sentinel pattern with a margin past M and N is the caller's to lay down — and read
// back after the launch.  res_alias (EPI_F32): the residual is C itself, as the engine calls it, so C's first M x N region holds the residual on entry.  pos (EPI_DEC_QKV): [M], reaches
// the kernel as the cur_pos fields of a SkwSeqState array.  Every index the epilogue can form is checked against the buffer sizes here, before anything is launched.
extern "C" int skw_debug_gemm_q8(skw_ctx* c, int type, const uint8_t* blocks_host, int N, int K, const float* A_host, long lda, int M, int segmented, int epi,
                                 int n_ctx, int H, int Tpad, const float* bias_host, int res_alias, float scale, int has_scale, const int* pos,
                                 void* C_host, long c_bytes, long ldc, void* C2_host, void* C3_host, long c2_bytes, long ldc2, int* kernel_id) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_gemm_q8"); auto bad = [&](const char* what) { return b.bad(what); };
    const int form = skw_ggml_dot_form(type);
    if (!form || M < 1 || M > 65536 || N < 1 || N > 65536 || K < 32 || K > 8192 || (K & 31) || lda < K || (lda & 3) || !blocks_host || !A_host || !C_host || !kernel_id) return bad("bad geometry");
    if (segmented && ((K & 127) || M > 4096)) return bad("the segmented form needs K % 128 == 0 and M <= 4096");
    const long MN_last = (long)(M - 1) * ldc + N;
    switch (epi) {
        case EPI_F32: case EPI_GELU_F32: if (ldc < N || MN_last * 4 > c_bytes) return bad("C too small"); break;
        case EPI_F16_PLAIN: if (ldc < N || MN_last * 2 > c_bytes) return bad("C too small"); break;
        case EPI_HEADS_F16: case EPI_VT_F16:
            if (n_ctx < 1 || M % n_ctx || (N & 63) || H != N / 64 || Tpad < n_ctx || (Tpad & 31) || (long)(M / n_ctx) * H * Tpad * 64 * 2 > c_bytes) return bad("heads / V^T geometry");
            break;
        case EPI_DEC_QKV:
            if (N % 3 || n_ctx != N / 3 || !pos || !C2_host || !C3_host || ldc < n_ctx || ((long)(M - 1) * ldc + n_ctx) * 2 > c_bytes) return bad("q|k|v geometry");
            for (int m = 0; m < M; ++m) if (pos[m] < 0 || ((long)m * ldc2 + (long)(pos[m] + 1) * n_ctx) * 2 > c2_bytes) return bad("a row's cache position lies outside C2 / C3");
            break;
        default: return bad("an epilogue skw_gemm_q8 does not take");
    }
    if (res_alias && epi != EPI_F32) return bad("res_alias is EPI_F32's");
    HostQ hq; host_q(type, blocks_host, N, K, &hq);
    DevLin L; ModelAllocsGuard weight(c->m);
    if (!up_q(c->m, hq, type, &L)) return bad("device allocation failed for the weight");
    const int nb = K / 32;
    float *dA = b.up(A_host, (size_t)M * lda), *dd = b.alloc<float>((size_t)M * nb), *ds = b.alloc<float>((size_t)M * nb); int8_t* dq = b.alloc<int8_t>((size_t)M * K);
    void* dC = b.up((const char*)C_host, (size_t)c_bytes); float* dbias = bias_host ? b.up(bias_host, (size_t)N) : nullptr;
    if (!dA || !dd || !ds || !dq || !dC || (bias_host && !dbias)) return -1;
    SkwGemmArgs a{}; a.M = M; a.N = N; a.K = K; a.C = dC; a.ldc = ldc; a.epi = epi; a.scale = scale; a.has_scale = has_scale; a.bias = dbias; a.n_ctx = n_ctx; a.H = H; a.Tpad = Tpad;
    a.gelu_tab = c->m->gelu_tab;
    if (res_alias) { a.res = (const float*)dC; a.ldres = ldc; }
    void *dC2 = nullptr, *dC3 = nullptr;
    if (epi == EPI_DEC_QKV) {
        const std::vector<int> seq0(M, 0);      // (the rows' pad fields stay 0: this launch reads cur_pos alone)
        SkwSeqState* dst = b.seq_rows(M, nullptr, seq0.data(), pos, nullptr); dC2 = b.up((const char*)C2_host, (size_t)c2_bytes); dC3 = b.up((const char*)C3_host, (size_t)c2_bytes);
        if (!dst || !dC2 || !dC3) return -1;
        a.C2 = dC2; a.C3 = dC3; a.ldc2 = ldc2; a.pos_ptr = &dst[0].cur_pos; a.pos_stride = (int)(sizeof(SkwSeqState) / sizeof(int));
    }
    skw_q8_quantize(dA, lda, M, K, dq, dd, ds, c->stream);
    SkwQ8Args qa{dq, dd, ds, L.qw, L.dwT, L.mwT, L.n_pad, L.qform, segmented ? 1 : 0};
    *kernel_id = skw_gemm_q8_kernel(a, qa);
    if (!skw_gemm_q8(a, qa, c->stream)) return bad("skw_gemm_q8 refused the arguments");
    if (!b.ran(c->stream) || !b.down((char*)C_host, (const char*)dC, (size_t)c_bytes)) return -1;
    if (epi == EPI_DEC_QKV && (!b.down((char*)C2_host, (const char*)dC2, (size_t)c2_bytes) || !b.down((char*)C3_host, (const char*)dC3, (size_t)c2_bytes))) return -1;
    return 0;
}
// tests (tests/test_gpu_gemm16_epi.py): one product of the f16_mfma precision on host-supplied operands through the public launchers, so that the dispatch is part of what is tested,
// with EVERY argument of the epilogues in the caller's hands — to be compared bit for bit with tests/gemm16_ref_lib.py.  Modelled on skw_debug_gemm_q8: the output buffers are the
// caller's (C, and C2 / C3 for EPI_DEC_QKV: uploaded as given — the caller's sentinel with its margins — and read back after the launch), every index the launch can form is checked
// against the buffer sizes here, BEFORE anything is launched (-1 and a message otherwise), kernel_id is what the launcher itself branches on (SkwGemm16Kernel), and -2 means the
// launcher refuses the geometry (so a case never silently tests another kernel).
//   launcher 0 / 1: skw_gemm16 with GEMM16W forced 1 / 0 in-process (k_gemm16w / k_gemm16), restored afterwards; 2: skw_gemm16_small; 3: skw_gemm16_small_lnA
//   A: f16 bits, a_halves of them (rows at lda, or a_rows_per_batch / a_batch_stride; a_frag: the fragment-order image, pad rows M .. ceil16(M) included); launcher 3: ln_x [M][K],
//   ln_w, ln_b [K] f32 instead.  W: [N][K] f16 bits in the order the kernel reads k; use_wf: the entry builds the fragment-order image itself (perm as the engine picks it: the
//   kperm'ed-output epilogues).  res: separate [M][ldres] f32, or res_alias: C itself.  pos [M] (EPI_DEC_QKV) reaches the kernel as SkwSeqState::cur_pos with the real stride.
//   force_small: probe bit 4 of the launcher — k_gemm16_small where the vocabulary kernel would apply.
struct skw_gemm16_epi_args {
    int32_t launcher, M, N, K, epi;
    const uint16_t* A; int64_t a_halves, lda; int32_t a_rows_per_batch; int64_t a_batch_stride; int32_t a_frag;
    const float *ln_x, *ln_w, *ln_b;
    const uint16_t* W; int32_t use_wf;
    const float* bias; const float* res; int64_t ldres; int32_t res_alias;
    float scale; int32_t has_scale;
    const float* pe; int32_t n_ctx, H, Tpad, frag, c_frag;
    const int32_t* pos; int32_t force_small;
    void* C; int64_t c_bytes, ldc; void* C2; void* C3; int64_t c2_bytes, ldc2;
    int32_t kernel_id;      // out
};
extern "C" int skw_debug_gemm16_epi(skw_ctx* c, skw_gemm16_epi_args* p) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_gemm16_epi"); auto bad = [&](const char* what) { return b.bad(what); };
    if (!p) return bad("no arguments");
    const int M = p->M, N = p->N, K = p->K, epi = p->epi, L = p->launcher; const long ldc = p->ldc;
    p->kernel_id = SKW_G16K_NONE;
    if (L < 0 || L > 3 || M < 1 || M > 65536 || N < 1 || N > 65536 || K < 64 || K > 8192 || !p->W || !p->C || p->c_bytes < 1) return bad("bad geometry");
    const bool big = L <= 1, lna = L == 3;
    const bool f32out = epi == EPI_F32 || epi == EPI_CONV2;
    const bool permo = epi == EPI_F16_KPERM || epi == EPI_GELU_F16_KPERM || epi == EPI_GELU_F16_KPERM_ROWPAD || epi == EPI_HEADS_F16;      // features stored in kperm order
    const bool per_clip = epi == EPI_HEADS_F16 || epi == EPI_VT_F16 || epi == EPI_GELU_F16_KPERM_ROWPAD || epi == EPI_CONV2 || p->frag;
    const long esz = f32out ? 4 : 2;
    // ---- operands
    if (big) {
        if ((K & 63) || (N & 15) || (permo && (N & 31))) return bad("the big kernels take K % 64 == 0, N % 16 == 0 (N % 32 == 0 for kperm'ed outputs)");
        if (p->a_frag || p->c_frag || p->ln_x || p->force_small || epi == EPI_DEC_QKV) return bad("a decode kernels' argument on a big-kernel launch");
        if (!p->A || p->lda < 8 || (p->lda & 7) || (p->a_rows_per_batch ? (p->a_rows_per_batch < 1 || (p->a_batch_stride & 7) || p->a_batch_stride < 0) : p->lda < K)) return bad("A rows");
        const long last = p->a_rows_per_batch ? (long)((M - 1) / p->a_rows_per_batch) * p->a_batch_stride + (long)std::min(M - 1, p->a_rows_per_batch - 1) * p->lda : (long)(M - 1) * p->lda;
        if (last + K > p->a_halves) return bad("A too small for its rows");
        if (ldc & (f32out ? 3 : 7)) return bad("ldc must keep 16-byte chunks aligned");
    } else {
        if ((K & 127)) return bad("the decode kernels take K % 128 == 0");
        if (p->frag || p->a_rows_per_batch || per_clip) return bad("a big kernels' argument on a decode launch");
        if (epi != EPI_F32 && epi != EPI_F16_PLAIN && epi != EPI_GELU_F16_KPERM && epi != EPI_DEC_QKV) return bad("an epilogue the decode kernels do not take");
        if (epi != EPI_F32 && ((N & 15) || (ldc & 3))) return bad("the f16 epilogues store 8-byte groups: N % 16 == 0, ldc % 4 == 0");
        if (epi == EPI_GELU_F16_KPERM && (N & 31)) return bad("kperm'ed outputs need N % 32 == 0");
        if (p->c_frag && epi != EPI_GELU_F16_KPERM) return bad("c_frag is EPI_GELU_F16_KPERM's");
        if (lna) {
            if (!p->ln_x || !p->ln_w || !p->ln_b || p->a_frag || p->A) return bad("launcher 3 takes ln_x / ln_w / ln_b and no A");
        } else {
            if (!p->A || p->ln_x) return bad("launcher 2 takes A");
            if (p->a_frag ? (long)((M + 15) & ~15) * K > p->a_halves : (p->lda < K || (p->lda & 7) || (long)(M - 1) * p->lda + K > p->a_halves)) return bad("A too small for its rows");
        }
    }
    if (p->use_wf && ((N & 15) || (K & 31)) && big) return bad("a fragment-order image holds whole strips");
    // ---- outputs: the last element each epilogue can reach
    if (p->res_alias && (epi != EPI_F32 || p->res)) return bad("res_alias is EPI_F32's, and excludes a separate residual");
    if (p->res && ((epi != EPI_F32 && !lna) || p->ldres < N || (big && (p->ldres & 3)))) return bad("residual rows");      // (launcher 3 takes none: given one, it must refuse)
    const long B = (per_clip && p->n_ctx > 0) ? M / p->n_ctx : 0;
    if (per_clip && (p->n_ctx < 1 || M % p->n_ctx)) return bad("M must be whole clips for this epilogue");
    if (epi == EPI_HEADS_F16 || epi == EPI_VT_F16 || p->frag) {
        if ((N & 63) || p->H != N / 64 || p->Tpad < p->n_ctx || (p->Tpad & 31) || B * p->H * p->Tpad * 64 * 2 > p->c_bytes) return bad("heads / V^T / fragment-order geometry");
        if (p->frag && epi != EPI_F16_PLAIN && epi != EPI_VT_F16) return bad("frag is EPI_F16_PLAIN's and EPI_VT_F16's");
    } else if (epi == EPI_GELU_F16_KPERM_ROWPAD) {
        if (ldc < N || ((B * (p->n_ctx + 2) - 2) * ldc + N) * 2 > p->c_bytes) return bad("C too small for the padded rows");
    } else if (epi == EPI_DEC_QKV) {
        const int d = p->n_ctx;
        if (d < 16 || (d & 15) || N != 3 * d || !p->pos || !p->C2 || !p->C3 || ldc < d || ((long)(M - 1) * ldc + d) * 2 > p->c_bytes || (p->ldc2 & 3) || !p->has_scale) return bad("q|k|v geometry");
        for (int m = 0; m < M; ++m) if (p->pos[m] < 0 || ((long)m * p->ldc2 + (long)(p->pos[m] + 1) * d) * 2 > p->c2_bytes) return bad("a row's cache position lies outside C2 / C3");
    } else if (p->c_frag) {
        if ((long)((M + 15) & ~15) * N * 2 > p->c_bytes) return bad("C too small for the fragment-order image");
    } else {
        if (epi != EPI_F32 && epi != EPI_CONV2 && epi != EPI_F16_PLAIN && epi != EPI_F16_KPERM && epi != EPI_GELU_F16_KPERM) return bad("an epilogue skw_gemm16 does not take");
        if (ldc < N || ((long)(M - 1) * ldc + N) * esz > p->c_bytes) return bad("C too small");
    }
    if (epi == EPI_CONV2 && (!p->pe || !p->bias)) return bad("EPI_CONV2 needs pe [n_ctx][N] and a bias");
    if (p->res_alias && (ldc < N)) return bad("res_alias: C rows");
    // ---- device copies
    const bool perm = permo;                                  // the image's strip rows in the order of the epilogue that consumes the product, as the model loader picks it
    half_t *dA = nullptr, *dW, *dWf = nullptr; float *dx = nullptr, *dg = nullptr, *db = nullptr, *dbias = nullptr, *dres = nullptr, *dpe = nullptr; void *dC, *dC2 = nullptr, *dC3 = nullptr;
    if (p->A && !(dA = (half_t*)b.up(p->A, (size_t)p->a_halves))) return -1;
    if (!(dW = (half_t*)b.up(p->W, (size_t)N * K))) return -1;
    if (lna && (!(dx = b.up(p->ln_x, (size_t)M * K)) || !(dg = b.up(p->ln_w, (size_t)K)) || !(db = b.up(p->ln_b, (size_t)K)))) return -1;
    if (p->bias && !(dbias = b.up(p->bias, (size_t)N))) return -1;
    if (p->res && !(dres = b.up(p->res, (size_t)((long)(M - 1) * p->ldres + N)))) return -1;
    if (p->pe && !(dpe = b.up(p->pe, (size_t)p->n_ctx * N))) return -1;
    if (!(dC = b.up((const char*)p->C, (size_t)p->c_bytes))) return -1;
    SkwGemmArgs a{}; a.A = dA; a.lda = p->lda; a.a_rows_per_batch = p->a_rows_per_batch; a.a_batch_stride = p->a_batch_stride; a.W = dW; a.ldw = K; a.M = M; a.N = N; a.K = K;
    a.C = dC; a.ldc = ldc; a.bias = dbias; a.scale = p->scale; a.has_scale = p->has_scale; a.gelu_tab = c->m->gelu_tab; a.pe = dpe; a.n_ctx = p->n_ctx; a.H = p->H; a.Tpad = p->Tpad;
    a.epi = epi; a.c_frag = p->c_frag; a.a_frag = p->a_frag; a.frag = p->frag; a.probe = p->force_small ? 16 : 0; a.ln_x = dx; a.ln_w = dg; a.ln_b = db;
    if (p->res) { a.res = dres; a.ldres = p->ldres; }
    if (p->res_alias) { a.res = (const float*)dC; a.ldres = ldc; }
    if (epi == EPI_DEC_QKV) {
        const std::vector<int> seq0(M, 0);      // (the rows' pad fields stay 0: this launch reads cur_pos alone)
        dC2 = b.up((const char*)p->C2, (size_t)p->c2_bytes); dC3 = b.up((const char*)p->C3, (size_t)p->c2_bytes);
        SkwSeqState* dst = b.seq_rows(M, nullptr, seq0.data(), p->pos, nullptr);
        if (!dst || !dC2 || !dC3) return -1;
        a.C2 = dC2; a.C3 = dC3; a.ldc2 = p->ldc2; a.pos_ptr = &dst[0].cur_pos; a.pos_stride = (int)(sizeof(SkwSeqState) / sizeof(int));
    }
    if (p->use_wf && !(N & 15)) {
        if (!(dWf = b.alloc<half_t>((size_t)N * K))) return -1;
        skw_make_wfrag(dW, K, N, K, perm ? 1 : 0, dWf, c->stream); a.Wf = dWf;
    } else if (p->use_wf) {      // N % 16 != 0: no image exists for such a weight; a non-null Wf shows the launcher's refusal (the buffer is never read)
        if (!(dWf = b.fill<half_t>(0, (size_t)((N + 15) & ~15) * K))) return -1;
        a.Wf = dWf;
    }
    bool ran = true;
    if (big) {
        SwOverride w(SW_GEMM16W, L == 0 ? 1 : 0);
        if (L == 0 && !skw_gemm16_takes_w(a)) ran = false;
        else { p->kernel_id = skw_gemm16_kernel(a); skw_gemm16(a, c->stream); }
    } else if (L == 2) { p->kernel_id = skw_gemm16_small_kernel(a); ran = skw_gemm16_small(a, c->stream); }
    else { p->kernel_id = skw_gemm16_small_lnA_kernel(a); ran = skw_gemm16_small_lnA(a, c->stream); }
    if (!ran) { bad("the launcher refuses these arguments"); return -2; }
    if (!b.ran(c->stream) || !b.down((char*)p->C, (const char*)dC, (size_t)p->c_bytes)) return -1;
    if (epi == EPI_DEC_QKV && (!b.down((char*)p->C2, (const char*)dC2, (size_t)p->c2_bytes) || !b.down((char*)p->C3, (const char*)dC3, (size_t)p->c2_bytes))) return -1;
    return 0;
}
// tests: k_q8_quantize on host rows x [M][ldx] (ldx >= K, a multiple of 4): q int8 [M][K], dT / sT f32 [K/32][M]
extern "C" int skw_debug_q8_quantize(skw_ctx* c, const float* x_host, long ldx, int M, int K, int8_t* q, float* dT, float* sT) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_q8_quantize");
    if (M < 1 || M > 65536 || K < 32 || K > 8192 || (K & 31) || ldx < K || (ldx & 3) || !x_host || !q || !dT || !sT) return b.bad("bad geometry");
    const int nb = K / 32;
    float *dx = b.up(x_host, (size_t)M * ldx), *dd = b.alloc<float>((size_t)M * nb), *ds = b.alloc<float>((size_t)M * nb); int8_t* dq = b.alloc<int8_t>((size_t)M * K);
    if (!dx || !dd || !ds || !dq) return -1;
    skw_q8_quantize(dx, ldx, M, K, dq, dd, ds, c->stream);
    if (!b.ran(c->stream) || !b.down(q, dq, (size_t)M * K) || !b.down(dT, dd, (size_t)M * nb) || !b.down(sT, ds, (size_t)M * nb)) return -1;
    return 0;
}
// tests: the decoder's self attention (the exact form of k_dec_attn) twice on the same operands — once with f32_out = 1 (out_f32 [rows][H*64]), once leaving its rows as q8 blocks
// (SkwQ8Out: q int8 [rows][H*64], dT / sT f32 [H*2][rows]) — so that the in-kernel quantiser can be held to quantize_rows of the first launch's rows.  Q [rows][H*64], K / V
// [rows][n_text_ctx][H*64] f16 bit patterns (row b reads the cache of sequence seq[b], or b); pos / active / seq: [rows] (the last two may be null), reaching the kernel as fields of a
// SkwSeqState array.  All four output buffers are uploaded as the caller filled them (a sentinel), so what an inactive row leaves is visible.
extern "C" int skw_debug_self_attn_q8(skw_ctx* c, int H, int n_text_ctx, int rows, const uint16_t* Q_host, const uint16_t* K_host, const uint16_t* V_host, const int* pos, const int* active,
                                      const int* seq, float* out_f32, int8_t* q, float* dT, float* sT) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_self_attn_q8"); auto bad = [&](const char* what) { return b.bad(what); };
    if (H < 1 || H > 32 || n_text_ctx < 1 || n_text_ctx > 7 * 64 || rows < 1 || rows > 4096 || !Q_host || !K_host || !V_host || !pos || !out_f32 || !q || !dT || !sT) return bad("bad geometry");
    for (int b = 0; b < rows; ++b) if (pos[b] < 0 || pos[b] >= n_text_ctx || (seq && (seq[b] < 0 || seq[b] >= rows))) return bad("pos or seq outside the caches");
    const int d = H * 64; const size_t nQ = (size_t)rows * d, nKV = (size_t)rows * n_text_ctx * d, nS = (size_t)2 * H * rows;
    half_t *dq16 = (half_t*)b.up(Q_host, nQ), *dk = (half_t*)b.up(K_host, nKV), *dv = (half_t*)b.up(V_host, nKV);
    float *dout = b.up(out_f32, nQ), *dd = b.up(dT, nS), *ds = b.up(sT, nS); int8_t* dq8 = b.up(q, nQ); SkwSeqState* dst = b.seq_rows(rows, active, seq, pos, nullptr);
    if (!dq16 || !dk || !dv || !dout || !dd || !ds || !dq8 || !dst) return -1;
    const int* act = active ? &dst[0].active : nullptr; const int* sq = seq ? &dst[0].pad : nullptr;
    skw_dec_self_attn(dq16, dk, dv, &dst[0].cur_pos, rows, H, d, n_text_ctx, (half_t*)dout, act, c->stream, 1, SkwQ8Out{nullptr, nullptr, nullptr, 0}, sq);
    skw_dec_self_attn(dq16, dk, dv, &dst[0].cur_pos, rows, H, d, n_text_ctx, nullptr, act, c->stream, 0, SkwQ8Out{dq8, dd, ds, rows}, sq);
    if (!b.ran(c->stream) || !b.down(out_f32, dout, nQ) || !b.down(q, dq8, nQ) || !b.down(dT, dd, nS) || !b.down(sT, ds, nS)) return -1;
    return 0;
}

// Test hook (tests/test_gpu_xattn_mq_exact.py): the exact precision's two prompt-pass cross attentions on caller-supplied operands, in the style of skw_debug_attn16.
//   Q [rows][H*64] f16 bit patterns, plain order; K / V [n_slots][n_ctx][H*64] f16 bit patterns in natural order (the hook lays them out as the exact precision keeps them: K rows,
//   V^T per head in kperm key order); every K / V position of slot s from fill_from[s] up holds k_pad / v_pad when the kernel runs, and so do the pad keys n_ctx .. Tpad of V^T.
//   n_seq sequences (row0, nq, slot); slot_k null or [n_slots].  mq = 0: skw_dec_cross_attn_vt (pv16 = 0), one row per query, `seq` / `nkeys` built from the same description;
//   mq = 1: skw_xattn_prefill_exact.  The output buffer starts as `sentinel` in every 16-bit half; out: the raw buffer, rows x H*64 x (f32_out ? 4 : 2) bytes (f16 rows in kperm order).
extern "C" int skw_debug_xattn_exact(skw_ctx* c, int mq, int H, int n_ctx, int n_slots, int rows, int f32_out, const uint16_t* Q_host, const uint16_t* K_host, const uint16_t* V_host,
                                     const int* fill_from, int k_pad, int v_pad, const int* slot_k, int n_seq, const int* row0, const int* nq, const int* slot, int sentinel, void* out_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_xattn_exact"); auto bad = [&](const char* what) { return b.bad(what); };
    if (H < 1 || H > 32 || n_ctx < 1 || n_ctx > SKW_XATTN_MQ_MAX_CTX || n_slots < 1 || n_slots > 64 || rows < 1 || rows > 65536 || !fill_from) return bad("bad geometry");
    if (n_seq < 1 || n_seq > 64 || !row0 || !nq || !slot) return bad("the prompt pass needs row0 / nq / slot");
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31; int nq_max = 0;
    for (int s = 0; s < n_slots; ++s) if (fill_from[s] < 0 || fill_from[s] > n_ctx) return bad("fill_from outside [0, n_ctx]");
    std::vector<SkwSeqState> st(rows); memset((void*)st.data(), 0, sizeof(SkwSeqState) * rows);      // rows outside every sequence stay inactive: the single-query kernel skips them
    for (int i = 0; i < n_seq; ++i) {
        if (row0[i] < 0 || nq[i] < 0 || row0[i] + nq[i] > rows || slot[i] < 0 || slot[i] >= n_slots) return bad("a sequence's rows or slot lie outside the buffers");
        nq_max = std::max(nq_max, nq[i]);
        for (int r = row0[i]; r < row0[i] + nq[i]; ++r) { if (st[r].active) return bad("sequences overlap"); st[r].active = 1; st[r].pad = slot[i]; st[r].n_keys = slot_k ? slot_k[slot[i]] : 0; }
    }
    if (nq_max < 1) return bad("no queries");
    const size_t nQ = (size_t)rows * d, nK = (size_t)n_slots * n_ctx * d, nV = (size_t)n_slots * Tpad * d, nO = (size_t)rows * d * (f32_out ? 2 : 1);
    std::vector<uint16_t> k(nK, (uint16_t)k_pad), v(nV, (uint16_t)v_pad), o(nO, (uint16_t)sentinel);
    for (int s = 0; s < n_slots; ++s) for (int i = 0; i < fill_from[s]; ++i) for (int n = 0; n < d; ++n) {
        k[((size_t)s * n_ctx + i) * d + n] = K_host[((size_t)s * n_ctx + i) * d + n];
        v[((size_t)s * d + n) * Tpad + skw_kperm(i)] = V_host[((size_t)s * n_ctx + i) * d + n];
    }
    half_t *dq = (half_t*)b.up(Q_host, nQ), *dk = (half_t*)b.up(k.data(), nK), *dv = (half_t*)b.up(v.data(), nV), *dout = (half_t*)b.up(o.data(), nO);
    SkwSeqState* dst = b.up(st.data(), (size_t)rows); int* dmeta = b.seq_meta(n_seq, row0, nq, slot, n_slots, slot_k);
    if (!dq || !dk || !dv || !dout || !dst || !dmeta) return -1;
    if (mq) {
        if (!skw_xattn_prefill_exact(dq, dk, dv, dout, n_seq, nq_max, dmeta, dmeta + 64, dmeta + 128, H, d, n_ctx, Tpad, c->stream, f32_out, slot_k ? dmeta + 192 : nullptr))
            return bad("the multi-query launcher refused the geometry");
    } else skw_dec_cross_attn_vt(dq, dk, dv, rows, H, d, n_ctx, Tpad, dout, &dst[0].active, c->stream, f32_out, 0, &dst[0].pad, nullptr, nullptr, 0, nullptr, slot_k ? &dst[0].n_keys : nullptr);
    if (!b.ran(c->stream) || !b.down((uint16_t*)out_host, (const uint16_t*)dout, nO)) return -1;
    return 0;
}

// Test hooks (tests/test_gpu_align_kernels.py): the three word-timestamp kernels on caller-supplied arrays, each held by its test to the evaluator of include/skw_align.h.
// Sequences are described by parallel arrays and laid out back to back: sequence i's rows are prow0 = n[0] + .. + n[i-1] onwards, its matrix starts at cell sum of n[j] * kw[j].
static bool align_hook_seqs(std::vector<SkwAlignSeq>& sq, int n_seq, const int* n, const int* kw, long* rows_total, long* cells) {
    long r = 0, x = 0;
    for (int i = 0; i < n_seq; ++i) {
        if (n[i] < 1 || n[i] > SKW_ALIGN_MAX_ROWS || kw[i] < 1) return false;
        sq[i].n = n[i]; sq[i].kw = kw[i]; sq[i].prow0 = (int)r; sq[i].xoff = x;
        r += n[i]; x += (long)n[i] * kw[i];
    }
    *rows_total = r; *cells = x;
    return true;
}
// step 1.  Q [q_rows][H*64], K [n_slots][n_ctx][H*64] f16 bit patterns, natural order (frag: the hook lays K out as the fragment-order image, Tpad rows, pad keys k_pad).
// Sequence i: alignment rows qrow0[i] .. + n[i] of Q, slot[i], n_keys[i] (0: n_ctx).  P: [heads of head_mask][rows_total][n_ctx] f32, uploaded as the caller filled it
// (a sentinel), so what the kernel leaves alone — keys past n_keys — is visible.
extern "C" int skw_debug_align_qk(skw_ctx* c, int H, int n_ctx, int n_slots, int q_rows, int frag, const uint16_t* Q_host, const uint16_t* K_host, int k_pad, unsigned head_mask,
                                  int n_seq, const int* qrow0, const int* n, const int* slot, const int* n_keys, float* P_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_align_qk"); auto bad = [&](const char* what) { return b.bad(what); };
    if (H < 1 || H > 32 || n_ctx < 1 || n_ctx > SKW_XATTN_MQ_MAX_CTX || n_slots < 1 || n_slots > 64 || q_rows < 1 || n_seq < 1 || n_seq > 4096 || !head_mask) return bad("bad geometry");
    const int d = H * 64, Tpad = (n_ctx + 31) & ~31, nh = skw_align_popcount(head_mask);
    std::vector<SkwAlignSeq> sq(n_seq); memset((void*)sq.data(), 0, sizeof(SkwAlignSeq) * n_seq);
    std::vector<int> kw(n_seq, 1); long rows_total = 0, cells = 0;
    if (!align_hook_seqs(sq, n_seq, n, kw.data(), &rows_total, &cells)) return bad("a sequence's row count lies outside [1, 256]");
    for (int i = 0; i < n_seq; ++i) {
        if (qrow0[i] < 0 || qrow0[i] + n[i] > q_rows || slot[i] < 0 || slot[i] >= n_slots || n_keys[i] < 0 || n_keys[i] > n_ctx) return bad("a sequence's rows, slot or keys lie outside the buffers");
        sq[i].qrow0 = qrow0[i]; sq[i].slot = slot[i]; sq[i].n_keys = n_keys[i];
    }
    const size_t nK = (size_t)n_slots * (frag ? Tpad : n_ctx) * d, nP = (size_t)nh * rows_total * n_ctx;
    std::vector<uint16_t> k(nK, (uint16_t)k_pad);
    for (int s = 0; s < n_slots; ++s) for (int i = 0; i < n_ctx; ++i) for (int f = 0; f < d; ++f)
        k[frag ? (size_t)skw_kfrag_off(s, H, Tpad, i, f & ~7) + (f & 7) : ((size_t)s * n_ctx + i) * d + f] = K_host[((size_t)s * n_ctx + i) * d + f];
    const half_t* dq = (const half_t*)b.up(Q_host, (size_t)q_rows * d); const half_t* dk = (const half_t*)b.up(k.data(), nK);
    SkwAlignSeq* dsq = b.up(sq.data(), (size_t)n_seq); float* dP = b.up(P_host, nP);
    if (!dq || !dk || !dsq || !dP) return -1;
    if (!skw_align_qk(dq, d, dk, dsq, n_seq, (int)rows_total, head_mask, H, n_ctx, Tpad, frag, dP, rows_total, n_ctx, c->stream)) return bad("the launcher refused the geometry");
    if (!b.ok(hipStreamSynchronize(c->stream)) || !b.ok(hipGetLastError()) || !b.ok(hipMemcpy(P_host, dP, nP * 4, hipMemcpyDeviceToHost))) return -1;
    return 0;
}
// steps 2-5.  P_host: the layers' captures back to back, layer l = [nh[l]][rows_total][p_stride] f32; one launch per layer in ascending order, the first starting and the last
// finishing the sums.  x_host: [cells] f32, uploaded as the caller filled it.
extern "C" int skw_debug_align_reduce(skw_ctx* c, int n_layers, const int* nh, const float* P_host, int p_stride, int width, int n_seq, const int* n, const int* kw, float* x_host) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_align_reduce"); auto bad = [&](const char* what) { return b.bad(what); };
    if (n_layers < 1 || n_layers > SKW_ALIGN_MAX_LAYERS || p_stride < 1 || n_seq < 1 || n_seq > 4096) return bad("bad geometry");
    std::vector<SkwAlignSeq> sq(n_seq); memset((void*)sq.data(), 0, sizeof(SkwAlignSeq) * n_seq);
    long rows_total = 0, cells = 0; int kw_max = 0, n_heads = 0;
    if (!align_hook_seqs(sq, n_seq, n, kw, &rows_total, &cells)) return bad("a sequence's row count lies outside [1, 256], or its crop below 1");
    for (int i = 0; i < n_seq; ++i) { if (kw[i] > p_stride) return bad("a crop beyond the capture's keys"); kw_max = std::max(kw_max, kw[i]); }
    for (int l = 0; l < n_layers; ++l) { if (nh[l] < 1 || nh[l] > 32) return bad("a layer without heads"); n_heads += nh[l]; }
    const float* dP = b.up(P_host, (size_t)n_heads * rows_total * p_stride); SkwAlignSeq* dsq = b.up(sq.data(), (size_t)n_seq); float* dx = b.up(x_host, (size_t)cells);
    double* dacc = nullptr; { std::vector<double> nanfill((size_t)cells, (double)NAN); dacc = b.up(nanfill.data(), (size_t)cells); }      // (no launch may read a sum it did not start)
    if (!dP || !dsq || !dx || !dacc) return -1;
    size_t off = 0;
    for (int l = 0; l < n_layers; ++l) {
        const bool launched = skw_align_reduce(dP + off, rows_total, p_stride, dsq, n_seq, kw_max, nh[l], width, l == 0, l == n_layers - 1, n_heads, dacc, dx, c->stream);
        if (!launched) return bad("the launcher refused the geometry");
        off += (size_t)nh[l] * rows_total * p_stride;
    }
    if (!b.ok(hipStreamSynchronize(c->stream)) || !b.ok(hipGetLastError()) || !b.ok(hipMemcpy(x_host, dx, (size_t)cells * 4, hipMemcpyDeviceToHost))) return -1;
    return 0;
}
// steps 6-7, one launch for all n_seq problems.  x_host: the matrices back to back; jump / t0 / t1: [rows_total] int32, uploaded as the caller filled them.
extern "C" int skw_debug_align_dtw(skw_ctx* c, int n_seq, const int* n, const int* kw, const int* seek_cs, const float* x_host, int32_t* jump, int32_t* t0, int32_t* t1) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    HookBufs b(errbuf, "skw_debug_align_dtw"); auto bad = [&](const char* what) { return b.bad(what); };
    if (n_seq < 1 || n_seq > 4096) return bad("bad geometry");
    std::vector<SkwAlignSeq> sq(n_seq); memset((void*)sq.data(), 0, sizeof(SkwAlignSeq) * n_seq);
    long rows_total = 0, cells = 0; int kw_max = 0, n_max = 0;
    if (!align_hook_seqs(sq, n_seq, n, kw, &rows_total, &cells)) return bad("a sequence's row count lies outside [1, 256], or its crop below 1");
    for (int i = 0; i < n_seq; ++i) { sq[i].seek_cs = seek_cs[i]; kw_max = std::max(kw_max, kw[i]); n_max = std::max(n_max, n[i]); }
    const float* dx = b.up(x_host, (size_t)cells); SkwAlignSeq* dsq = b.up(sq.data(), (size_t)n_seq);
    int *dj = b.up(jump, (size_t)rows_total), *d0 = b.up(t0, (size_t)rows_total), *d1 = b.up(t1, (size_t)rows_total);
    if (!dx || !dsq || !dj || !d0 || !d1) return -1;
    if (!skw_align_dtw(dx, dsq, n_seq, n_max, kw_max, dj, d0, d1, c->stream)) return bad("the launcher refused the geometry");
    if (!b.ok(hipStreamSynchronize(c->stream)) || !b.ok(hipGetLastError())) return -1;
    if (!b.ok(hipMemcpy(jump, dj, (size_t)rows_total * 4, hipMemcpyDeviceToHost)) || !b.ok(hipMemcpy(t0, d0, (size_t)rows_total * 4, hipMemcpyDeviceToHost)) ||
        !b.ok(hipMemcpy(t1, d1, (size_t)rows_total * 4, hipMemcpyDeviceToHost))) return -1;
    return 0;
}
