// skw_vad_gpu.hip — the Silero VAD gate on gfx950, batched over frames and streams (C ABI: include/skw_vad_batch.h).
//
// Arithmetic: include/skw_silero_net.h, bit for bit (tests/test_gpu_vad.py).  Every output element is ONE thread's fmaf chain in
// the contract's index order; the kernels differ from the scalar specification only in which thread owns which element and in
// how many frames share one pass over a layer's weights.
//
// Two phases per call:
//   feed-forward (parallel over all frames of all streams): k_stft -> k_conv x4 -> k_conv as W_ih.  A thread owns one output
//     channel for a tile of frames, the tile's inputs sit in LDS (every LDS read is a wave-wide broadcast), the weights are
//     stored transposed ([tap][channel]) so that a wave reads one coalesced line per tap and uses it for the whole tile.
//     Intermediates go through HBM in chunks of FF_CHUNK frames (7.4 KB per frame written and read once: ~0.2 ms of traffic
//     for 60 000 frames, against milliseconds of arithmetic and of the recurrent phase), which also gives the test taps for free.
//   recurrent (one 512-thread workgroup per stream): thread r keeps row r of W_hh in 128 registers for the whole launch, h is
//     broadcast through LDS, the four gate non-linearities are applied by the thread that owns the row, threads 0..127 update
//     c and h.  h_t is stored; the output convolution (another 128-term chain) is deferred to k_out, parallel over frames.
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include "../../include/skw_vad_batch.h"
#include "../../include/skw_silero_net.h"
#include "skw_silero.h"

namespace {

constexpr int FF_CHUNK = 8192;                          // frames whose intermediates are resident at once
constexpr int MAX_FRAMES_PER_CALL = 1 << 21;            // 18 hours of audio; keeps every index in int range
std::atomic<int> g_vad_poison{0};

// ---- STFT magnitudes: thread = bin, FT frames (4 FT columns) per block
template <int FT>
__global__ __launch_bounds__(192) void k_stft(const float* __restrict__ BT /* [256][258] */, const float* __restrict__ audio, const float* __restrict__ state,
                                              const int* __restrict__ fstream, const int* __restrict__ sfirst, float* __restrict__ mag, int g0, int n) {
    __shared__ float s_x[FT][640];
    const int tid = threadIdx.x, l0 = blockIdx.x * FT;
    for (int i = tid; i < FT * 640; i += 192) {
        const int f = i / 640, j = i - f * 640, l = l0 + f;
        float v = 0.0f;
        if (l < n) {
            const int g = g0 + l, s = fstream[g];
            if (j < 64) v = g == sfirst[s] ? state[(size_t)s * 320 + j] : audio[(size_t)(g - 1) * 512 + 448 + j];
            else if (j < 576) v = audio[(size_t)g * 512 + (j - 64)];
            else v = audio[(size_t)g * 512 + (1150 - j - 64)];           // x[576 + m] = x[574 - m]
        }
        s_x[f][j] = v;
    }
    __syncthreads();
    const int bin = tid;
    if (bin >= 129) return;
    float re[FT][4], im[FT][4];
#pragma unroll
    for (int f = 0; f < FT; ++f)
#pragma unroll
        for (int fr = 0; fr < 4; ++fr) { re[f][fr] = 0.0f; im[f][fr] = 0.0f; }
    for (int k = 0; k < 256; ++k) {
        const float br = BT[k * 258 + bin], bi = BT[k * 258 + 129 + bin];
#pragma unroll
        for (int f = 0; f < FT; ++f)
#pragma unroll
            for (int fr = 0; fr < 4; ++fr) { const float xs = s_x[f][128 * fr + k]; re[f][fr] = fmaf(br, xs, re[f][fr]); im[f][fr] = fmaf(bi, xs, im[f][fr]); }
    }
#pragma unroll
    for (int f = 0; f < FT; ++f)
        if (l0 + f < n)
#pragma unroll
            for (int fr = 0; fr < 4; ++fr) mag[(size_t)(l0 + f) * 516 + bin * 4 + fr] = __builtin_sqrtf(fmaf(im[f][fr], im[f][fr], re[f][fr] * re[f][fr]));
}

// ---- Conv1d(kernel KW, padding KW / 2, stride ST) [+ ReLU] over in [frame][CI][T]; KW = 1, T = 1 is the dense layer W_ih.
// 256 threads = OB output channels x G frame groups; a thread owns channel o for FT frames.  WT is [CI * KW][CO].
template <int CI, int T, int ST, int KW, int CO, bool RELU, int FT>
__global__ __launch_bounds__(256) void k_conv(const float* __restrict__ WT, const float* __restrict__ bias, const float* __restrict__ in, float* __restrict__ out, int n) {
    constexpr int PAD = KW / 2, TO = (T + 2 * PAD - KW) / ST + 1, OB = CO < 256 ? CO : 256, G = 256 / OB, ROW = CI * T;
    __shared__ float s_in[G * FT * ROW];
    const int tid = threadIdx.x, g = tid / OB, o = blockIdx.y * OB + (tid - g * OB), l0 = blockIdx.x * (G * FT);
    for (int i = tid; i < G * FT * ROW; i += 256) s_in[i] = (l0 + i / ROW) < n ? in[(size_t)l0 * ROW + i] : 0.0f;
    __syncthreads();
    float acc[FT][TO];
    const float b = bias[o];
#pragma unroll
    for (int f = 0; f < FT; ++f)
#pragma unroll
        for (int t = 0; t < TO; ++t) acc[f][t] = b;
    const float* sp = s_in + g * FT * ROW;
    for (int c = 0; c < CI; ++c) {
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const float w = WT[(size_t)(c * KW + k) * CO + o];
#pragma unroll
            for (int t = 0; t < TO; ++t) {
                const int p = t * ST - PAD + k;                           // a constant after unrolling: padded taps cost nothing and are skipped
                if (p >= 0 && p < T) {
#pragma unroll
                    for (int f = 0; f < FT; ++f) acc[f][t] = fmaf(w, sp[f * ROW + c * T + p], acc[f][t]);
                }
            }
        }
    }
#pragma unroll
    for (int f = 0; f < FT; ++f) {
        const int l = l0 + g * FT + f;
        if (l < n)
#pragma unroll
            for (int t = 0; t < TO; ++t) { const float v = acc[f][t]; out[(size_t)l * (CO * TO) + o * TO + t] = RELU ? (v > 0.0f ? v : 0.0f) : v; }
    }
}

// ---- the recurrent phase: one workgroup per stream, thread r = gate row r
__global__ __launch_bounds__(512) void k_lstm(const float* __restrict__ WhhT /* [128][512] */, const float* __restrict__ b_hh, const float* __restrict__ gin /* [frame][512] */,
                                              const int* __restrict__ sfirst /* [S + 1] */, float* __restrict__ state /* [S][320] */, float* __restrict__ hout /* [frame][128] */) {
    __shared__ float4 s_h4[32];
    __shared__ float s_g[512];
    float* s_h = reinterpret_cast<float*>(s_h4);
    const int r = threadIdx.x, s = blockIdx.x, f0 = sfirst[s], f1 = sfirst[s + 1];
    if (f0 >= f1) return;
    float w[128];
#pragma unroll
    for (int k = 0; k < 128; ++k) w[k] = WhhT[k * 512 + r];
    const float b = b_hh[r];
    float c = 0.0f;
    if (r < 128) { s_h[r] = state[(size_t)s * 320 + 64 + r]; c = state[(size_t)s * 320 + 192 + r]; }
    __syncthreads();
    float sv = gin[(size_t)f0 * 512 + r];
    for (int f = f0; f < f1; ++f) {
        const float sn = f + 1 < f1 ? gin[(size_t)(f + 1) * 512 + r] : 0.0f;     // the next step's input half, in flight during this step's chain
        float u = b;
#pragma unroll
        for (int k4 = 0; k4 < 32; ++k4) {
            const float4 h = s_h4[k4];
            u = fmaf(w[4 * k4 + 0], h.x, u); u = fmaf(w[4 * k4 + 1], h.y, u); u = fmaf(w[4 * k4 + 2], h.z, u); u = fmaf(w[4 * k4 + 3], h.w, u);
        }
        const float gate = sv + u;
        s_g[r] = (r >> 7) == 2 ? skw_silero_tanh(gate) : skw_silero_sigmoid(gate);   // wave-uniform: rows 256..383 are the candidate gate
        __syncthreads();
        if (r < 128) {
            c = fmaf(s_g[128 + r], c, s_g[r] * s_g[256 + r]);
            const float h = s_g[384 + r] * skw_silero_tanh(c);
            s_h[r] = h; hout[(size_t)f * 128 + r] = h;
        }
        __syncthreads();
        sv = sn;
    }
    if (r < 128) { state[(size_t)s * 320 + 64 + r] = s_h[r]; state[(size_t)s * 320 + 192 + r] = c; }
}

// ---- output convolution + sigmoid, one thread per frame (a 128-term chain, not a tree)
__global__ __launch_bounds__(256) void k_out(const float* __restrict__ ow, float ob, const float* __restrict__ hout, float* __restrict__ probs, int n) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const float4* h4 = reinterpret_cast<const float4*>(hout + (size_t)f * 128);
    float acc = ob;
    for (int k4 = 0; k4 < 32; ++k4) {
        const float4 h = h4[k4];
        acc = fmaf(ow[4 * k4 + 0], h.x > 0.0f ? h.x : 0.0f, acc); acc = fmaf(ow[4 * k4 + 1], h.y > 0.0f ? h.y : 0.0f, acc);
        acc = fmaf(ow[4 * k4 + 2], h.z > 0.0f ? h.z : 0.0f, acc); acc = fmaf(ow[4 * k4 + 3], h.w > 0.0f ? h.w : 0.0f, acc);
    }
    probs[f] = skw_silero_sigmoid(acc);
}

struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    bool reserve(size_t bytes) { if (bytes <= cap) return true; if (p) (void)hipFree(p); p = nullptr; cap = 0; const size_t want = bytes + bytes / 4;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return false; } cap = want; return true; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct HostBuf {
    void* p = nullptr; size_t cap = 0;
    bool reserve(size_t bytes) { if (bytes <= cap) return true; if (p) (void)hipHostFree(p); p = nullptr; cap = 0; const size_t want = bytes + bytes / 4;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; } cap = want; return true; }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

struct skw_vad_gpu {
    int device = 0; hipStream_t stream = nullptr; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; std::mutex mu; char errbuf[512] = {0}; float timing[3] = {0, 0, 0};
    // weights, device: transposed for coalesced reads
    DevBuf basisT, cwT[4], cb[4], wihT, b_ih, whhT, b_hh, ow; float ob = 0.0f;
    // per call, grow-only
    DevBuf audio, state, fstream, sfirst, gin, hout, probs, mag, c1, c2, c3, c4;
    HostBuf h_audio, h_state, h_meta, h_probs;
};

namespace {

bool fail(skw_vad_gpu* g, const char* what, hipError_t e) { snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: %s: %s", what, hipGetErrorString(e)); return false; }
#define VG_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(g, #call, e_); } while (0)
#define VG_RESERVE(buf, bytes) do { if (!(buf).reserve(bytes)) { \
    snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: out of memory reserving %zu bytes for " #buf, (size_t)(bytes)); return false; } } while (0)

bool upload(skw_vad_gpu* g, DevBuf& d, const std::vector<float>& v) { VG_RESERVE(d, v.size() * 4); VG_HIP(hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice)); return true; }
std::vector<float> transposed(const std::vector<float>& w, int rows, int cols) {   // [rows][cols] -> [cols][rows]
    std::vector<float> t((size_t)rows * cols);
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = w[(size_t)r * cols + c];
    return t;
}

bool poison(skw_vad_gpu* g, DevBuf& b) { if (b.p) VG_HIP(hipMemsetAsync(b.p, 0xff, b.cap, g->stream)); return true; }   // 0xffffffff is a NaN

// the six feed-forward launches for frames [g0, g0 + n) of the packed batch; intermediates are indexed from 0
bool feed_forward(skw_vad_gpu* g, int g0, int n) {
    const hipStream_t st = g->stream;
    k_stft<4><<<dim3((n + 3) / 4), dim3(192), 0, st>>>(g->basisT.as<float>(), g->audio.as<float>(), g->state.as<float>(), g->fstream.as<int>(), g->sfirst.as<int>(), g->mag.as<float>(), g0, n);
    k_conv<129, 4, 1, 3, 128, true, 4><<<dim3((n + 7) / 8, 1), dim3(256), 0, st>>>(g->cwT[0].as<float>(), g->cb[0].as<float>(), g->mag.as<float>(), g->c1.as<float>(), n);
    k_conv<128, 4, 2, 3, 64, true, 4><<<dim3((n + 15) / 16, 1), dim3(256), 0, st>>>(g->cwT[1].as<float>(), g->cb[1].as<float>(), g->c1.as<float>(), g->c2.as<float>(), n);
    k_conv<64, 2, 2, 3, 64, true, 8><<<dim3((n + 31) / 32, 1), dim3(256), 0, st>>>(g->cwT[2].as<float>(), g->cb[2].as<float>(), g->c2.as<float>(), g->c3.as<float>(), n);
    k_conv<64, 1, 1, 3, 128, true, 8><<<dim3((n + 15) / 16, 1), dim3(256), 0, st>>>(g->cwT[3].as<float>(), g->cb[3].as<float>(), g->c3.as<float>(), g->c4.as<float>(), n);
    k_conv<128, 1, 1, 1, 512, false, 8><<<dim3((n + 7) / 8, 2), dim3(256), 0, st>>>(g->wihT.as<float>(), g->b_ih.as<float>(), g->c4.as<float>(), g->gin.as<float>() + (size_t)g0 * 512, n);
    VG_HIP(hipGetLastError());
    return true;
}

bool reserve_call(skw_vad_gpu* g, int S, int total) {
    const size_t chunk = (size_t)(total < FF_CHUNK ? total : FF_CHUNK);
    VG_RESERVE(g->audio, (size_t)total * 512 * 4); VG_RESERVE(g->state, (size_t)S * 320 * 4); VG_RESERVE(g->fstream, (size_t)total * 4); VG_RESERVE(g->sfirst, (size_t)(S + 1) * 4);
    VG_RESERVE(g->gin, (size_t)total * 512 * 4); VG_RESERVE(g->hout, (size_t)total * 128 * 4); VG_RESERVE(g->probs, (size_t)total * 4);
    VG_RESERVE(g->mag, chunk * 516 * 4); VG_RESERVE(g->c1, chunk * 512 * 4); VG_RESERVE(g->c2, chunk * 128 * 4); VG_RESERVE(g->c3, chunk * 64 * 4); VG_RESERVE(g->c4, chunk * 128 * 4);
    VG_RESERVE(g->h_audio, (size_t)total * 512 * 4); VG_RESERVE(g->h_state, (size_t)S * 320 * 4); VG_RESERVE(g->h_meta, (size_t)(total + S + 1) * 4); VG_RESERVE(g->h_probs, (size_t)total * 4);
    if (g_vad_poison.load()) for (DevBuf* b : {&g->audio, &g->state, &g->fstream, &g->sfirst, &g->gin, &g->hout, &g->probs, &g->mag, &g->c1, &g->c2, &g->c3, &g->c4}) if (!poison(g, *b)) return false;
    return true;
}

// packs the streams, uploads; leaves sfirst/fstream on the device
bool stage_in(skw_vad_gpu* g, int S, const float* const* frames, const int32_t* n_frames, const float* const* state, int total) {
    float* ha = g->h_audio.as<float>(); float* hs = g->h_state.as<float>(); int* fstream = g->h_meta.as<int>(); int* sfirst = fstream + total;
    int pos = 0;
    for (int s = 0; s < S; ++s) {
        sfirst[s] = pos;
        if (n_frames[s] > 0) memcpy(ha + (size_t)pos * 512, frames[s], (size_t)n_frames[s] * 512 * 4);
        for (int i = 0; i < n_frames[s]; ++i) fstream[pos + i] = s;
        memcpy(hs + (size_t)s * 320, state[s], 320 * 4);
        pos += n_frames[s];
    }
    sfirst[S] = pos;
    VG_HIP(hipMemcpyAsync(g->audio.p, ha, (size_t)total * 512 * 4, hipMemcpyHostToDevice, g->stream));
    VG_HIP(hipMemcpyAsync(g->state.p, hs, (size_t)S * 320 * 4, hipMemcpyHostToDevice, g->stream));
    VG_HIP(hipMemcpyAsync(g->fstream.p, fstream, (size_t)total * 4, hipMemcpyHostToDevice, g->stream));
    VG_HIP(hipMemcpyAsync(g->sfirst.p, sfirst, (size_t)(S + 1) * 4, hipMemcpyHostToDevice, g->stream));
    return true;
}

bool process(skw_vad_gpu* g, int S, const float* const* frames, const int32_t* n_frames, float* const* state, float* const* probs) {
    long total_l = 0;
    for (int s = 0; s < S; ++s) {
        if (n_frames[s] < 0 || !state[s] || (n_frames[s] > 0 && (!frames[s] || !probs[s]))) {
            snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: stream %d: negative frame count or missing pointer", s); return false; }
        total_l += n_frames[s];
    }
    if (total_l > MAX_FRAMES_PER_CALL) { snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: %ld frames in one call (limit %d)", total_l, MAX_FRAMES_PER_CALL); return false; }
    const int total = (int)total_l;
    if (total == 0) return true;
    VG_HIP(hipSetDevice(g->device));
    if (!reserve_call(g, S, total)) return false;
    VG_HIP(hipEventRecord(g->ev[0], g->stream));
    if (!stage_in(g, S, frames, n_frames, state, total)) return false;
    VG_HIP(hipEventRecord(g->ev[1], g->stream));
    for (int g0 = 0; g0 < total; g0 += FF_CHUNK) if (!feed_forward(g, g0, total - g0 < FF_CHUNK ? total - g0 : FF_CHUNK)) return false;
    k_lstm<<<dim3(S), dim3(512), 0, g->stream>>>(g->whhT.as<float>(), g->b_hh.as<float>(), g->gin.as<float>(), g->sfirst.as<int>(), g->state.as<float>(), g->hout.as<float>());
    k_out<<<dim3((total + 255) / 256), dim3(256), 0, g->stream>>>(g->ow.as<float>(), g->ob, g->hout.as<float>(), g->probs.as<float>(), total);
    VG_HIP(hipGetLastError());
    VG_HIP(hipEventRecord(g->ev[2], g->stream));
    VG_HIP(hipMemcpyAsync(g->h_probs.p, g->probs.p, (size_t)total * 4, hipMemcpyDeviceToHost, g->stream));
    VG_HIP(hipMemcpyAsync(g->h_state.p, g->state.p, (size_t)S * 320 * 4, hipMemcpyDeviceToHost, g->stream));
    VG_HIP(hipEventRecord(g->ev[3], g->stream));
    VG_HIP(hipStreamSynchronize(g->stream));
    for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&g->timing[i], g->ev[i], g->ev[i + 1]);
    const float* hp = g->h_probs.as<float>(); const float* hs = g->h_state.as<float>();
    int pos = 0;
    for (int s = 0; s < S; ++s) {
        const int n = n_frames[s];
        if (n == 0) continue;                                                  // an idle stream keeps its state as it is
        memcpy(probs[s], hp + pos, (size_t)n * 4);
        memcpy(state[s], frames[s] + (size_t)n * 512 - 64, 64 * 4);           // the context is the audio's last 64 samples
        memcpy(state[s] + 64, hs + (size_t)s * 320 + 64, 256 * 4);
        pos += n;
    }
    return true;
}

bool taps(skw_vad_gpu* g, const float* frames, int n, const float* state320, float* mag, float* c1, float* c2, float* c3, float* c4, float* gin) {
    if (n < 1 || n > FF_CHUNK || !frames || !state320) { snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: taps take 1..%d frames", FF_CHUNK); return false; }
    VG_HIP(hipSetDevice(g->device));
    if (!reserve_call(g, 1, n)) return false;
    const float* fp[1] = {frames}; const int32_t nf[1] = {n}; const float* sp[1] = {state320};
    if (!stage_in(g, 1, fp, nf, sp, n) || !feed_forward(g, 0, n)) return false;
    VG_HIP(hipStreamSynchronize(g->stream));
    struct { float* dst; DevBuf* src; size_t per; } out[6] = {{mag, &g->mag, 516}, {c1, &g->c1, 512}, {c2, &g->c2, 128}, {c3, &g->c3, 64}, {c4, &g->c4, 128}, {gin, &g->gin, 512}};
    for (auto& o : out) if (o.dst) VG_HIP(hipMemcpy(o.dst, o.src->p, (size_t)n * o.per * 4, hipMemcpyDeviceToHost));
    return true;
}

bool init(skw_vad_gpu* g, const skw::SileroWeights& w) {
    VG_HIP(hipSetDevice(g->device));
    VG_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    for (auto& e : g->ev) VG_HIP(hipEventCreate(&e));
    static const int KW[4] = {3, 3, 3, 3};
    if (!upload(g, g->basisT, transposed(w.basis, 258, 256))) return false;
    for (int l = 0; l < 4; ++l) if (!upload(g, g->cwT[l], transposed(w.cw[l], skw::SILERO_CO[l], skw::SILERO_CI[l] * KW[l])) || !upload(g, g->cb[l], w.cb[l])) return false;
    if (!upload(g, g->wihT, transposed(w.w_ih, 512, 128)) || !upload(g, g->b_ih, w.b_ih) || !upload(g, g->whhT, transposed(w.w_hh, 512, 128)) || !upload(g, g->b_hh, w.b_hh)) return false;
    if (!upload(g, g->ow, w.ow)) return false;
    g->ob = w.ob;
    return true;
}

void destroy(skw_vad_gpu* g) {
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    for (DevBuf* b : {&g->basisT, &g->cwT[0], &g->cwT[1], &g->cwT[2], &g->cwT[3], &g->cb[0], &g->cb[1], &g->cb[2], &g->cb[3], &g->wihT, &g->b_ih, &g->whhT, &g->b_hh, &g->ow,
                      &g->audio, &g->state, &g->fstream, &g->sfirst, &g->gin, &g->hout, &g->probs, &g->mag, &g->c1, &g->c2, &g->c3, &g->c4}) b->release();
    for (HostBuf* b : {&g->h_audio, &g->h_state, &g->h_meta, &g->h_probs}) b->release();
    for (auto& e : g->ev) if (e) (void)hipEventDestroy(e);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

}  // namespace

extern "C" skw_vad_gpu* skw_vad_gpu_create(const char* path, int device, char* err, size_t errlen) {
    auto say = [&](const std::string& m) { if (err && errlen) snprintf(err, errlen, "%s", m.c_str()); };
    try {
        skw::SileroWeights w; std::string e;
        if (!path) { say("Failed to load VAD model from '': no path"); return nullptr; }
        if (!skw::SileroVad::load_weights(path, &w, &e)) { say(e); return nullptr; }
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { say("skw_vad_gpu: no HIP device"); return nullptr; }
        if (device < 0 || device >= n) { say("skw_vad_gpu: device " + std::to_string(device) + " out of range (" + std::to_string(n) + " HIP device" + (n == 1 ? "" : "s") + ")"); return nullptr; }
        skw_vad_gpu* g = new skw_vad_gpu(); g->device = device;
        if (!init(g, w)) { say(g->errbuf); destroy(g); return nullptr; }
        return g;
    } catch (const std::exception& ex) { say(std::string("Failed to load VAD model from '") + (path ? path : "") + "': " + ex.what()); return nullptr; }
}
extern "C" int skw_vad_gpu_process(skw_vad_gpu* g, int n_streams, const float* const* frames, const int32_t* n_frames, float* const* state, float* const* probs) {
    if (!g) return -1;
    try {
        std::lock_guard<std::mutex> lk(g->mu);
        if (n_streams < 0 || (n_streams > 0 && (!frames || !n_frames || !state || !probs))) { snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: invalid arguments"); return 1; }
        if (n_streams == 0) return 0;
        return process(g, n_streams, frames, n_frames, state, probs) ? 0 : 1;
    } catch (const std::exception& ex) { snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: %s", ex.what()); return 1; }
}
extern "C" int skw_vad_gpu_debug_feed_forward(skw_vad_gpu* g, const float* frames, int n, const float* state320, float* mag, float* c1, float* c2, float* c3, float* c4, float* gin) {
    if (!g) return -1;
    try { std::lock_guard<std::mutex> lk(g->mu); return taps(g, frames, n, state320, mag, c1, c2, c3, c4, gin) ? 0 : 1; }
    catch (const std::exception& ex) { snprintf(g->errbuf, sizeof g->errbuf, "skw_vad_gpu: %s", ex.what()); return 1; }
}
extern "C" const char* skw_vad_gpu_last_error(const skw_vad_gpu* g) { return g ? g->errbuf : "skw_vad_gpu: null handle"; }
extern "C" void skw_vad_gpu_last_timing(const skw_vad_gpu* g, float* out3) { for (int i = 0; i < 3; ++i) out3[i] = g ? g->timing[i] : 0.0f; }
extern "C" void skw_vad_gpu_free(skw_vad_gpu* g) { if (g) destroy(g); }
extern "C" void skw_vad_gpu_debug_alloc_poison(int on) { g_vad_poison.store(on); }
