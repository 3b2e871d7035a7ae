// skw_kernels_sample.hip — logits -> token for gfx950 (CDNA4): the sampler in its two forms, its generator and draw, the decoding constraints.
// Compile with -ffp-contract=off: every fused multiply-add in here is explicit (see include/skw_math.h).
//
// What each kernel restates (whisper.cpp routine):
//   k_dec_sample*      whisper_process_logits + greedy / whisper_sample_token (K11)
#include <algorithm>
#include <cstring>
#include "../../include/skw_draw.h"
#include "skw_dev_common.h"

// ------------------------------------------------------------------ K11: logits -> token (+ state update)
struct ArgBest { float v; int i; };
__device__ __forceinline__ ArgBest better(ArgBest a, ArgBest b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ ArgBest block_argbest(ArgBest x, ArgBest* sh) {
    for (int o = 32; o > 0; o >>= 1) { ArgBest y; y.v = __shfl_xor(x.v, o, 64); y.i = __shfl_xor(x.i, o, 64); x = better(x, y); }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = x;
    __syncthreads();
    ArgBest r = sh[0]; for (int i = 1; i < nw; ++i) r = better(r, sh[i]);
    __syncthreads();
    return r;
}
// log-softmax statistics of the admissible logits in [lo,hi): returns max and logsumexp
__device__ void block_lse(const float* lg, int lo, int hi, float* sh_f, double* sh_d, float* out_max, float* out_lse) {
    float m = -INFINITY;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) m = fmaxf(m, lg[i]);
    m = block_max(m, sh_f);
    double acc = 0.0;
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) { float v = lg[i]; if (v > -INFINITY) acc += (double)skw_expf(v - m); }
    acc = block_sum_f64(acc, sh_d);
    *out_max = m;
    *out_lse = (acc > 0.0) ? skw_logf((float)acc) + m : -INFINITY;
}

// std::mt19937 / std::generate_canonical<double,53> / std::discrete_distribution as libstdc++ implements them (restated in
// oracle/skw_oracle.c, pinned there against the real library); run by one lane: the f64 sums are sequential by definition.
__global__ void k_rng_seed(uint32_t* rng_all, uint32_t seed) {
    uint32_t* mt = rng_all + (long)blockIdx.x * SKW_RNG_WORDS;
    mt[0] = seed; for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    mt[624] = 624;
}
void skw_rng_seed(uint32_t* rng, int n_clips, uint32_t seed, hipStream_t s) { hipLaunchKernelGGL(k_rng_seed, dim3(n_clips), dim3(1), 0, s, rng, seed); }
__device__ uint32_t mt_next(uint32_t* mt) {
    int idx = (int)mt[624];
    if (idx >= 624) {
        for (int i = 0; i < 624; ++i) {
            uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        idx = 0;
    }
    uint32_t y = mt[idx]; mt[624] = (uint32_t)(idx + 1);
    y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
    return y;
}
__device__ int discrete_draw(const float* probs, int n, uint32_t* mt) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += (double)probs[i];
    double cs = 0.0, tmp = 1.0;
    for (int k = 0; k < 2; ++k) { cs += (double)mt_next(mt) * tmp; tmp *= 4294967296.0; }
    double u = cs / tmp; if (u >= 1.0) u = 0.99999999999999988897769753748;   // nextafter(1.0, 0.0)
    double cp = 0.0;
    for (int i = 0; i < n; ++i) { cp += (double)probs[i] / sum; if (i == n - 1) cp = 1.0; if (!(cp < u)) return i; }
    return n - 1;
}

// Trace / teacher-forced decisions (skw_full_batch_traced): record what this precision chose and, when `forced` names another token, feed that one —
// the state below then evolves exactly as in the run the forced tokens came from.  lg: the row's logits in memory (filtered in place by the streaming
// kernel and by sampled passes; raw otherwise — the same number for an admissible token).
__device__ __forceinline__ void smp_trace_step(SkwTokenOut& tk, const float* lg, float lse, int i, int max_tok, long row, const int* forced, SkwTraceStep* trace,
                                               int i1, int i2, float t1, float t2, const SkwLogitParams& p, float temperature) {
    if (!trace || i >= max_tok) return;
    int fid = forced ? forced[row * max_tok + i] : -1;
    if (fid < 0 || fid >= p.n_vocab) fid = tk.id;
    SkwTraceStep ts; ts.chosen_id = tk.id; ts.forced_id = fid; ts.top1_id = i1; ts.top2_id = (t2 > -INFINITY) ? i2 : -1; ts.top1 = t1; ts.top2 = t2;
    ts.forced_logit = lg[fid]; ts.lse = lse; ts.temperature = temperature; ts.pad = 0;
    trace[row * max_tok + i] = ts;
    if (fid != tk.id) { tk.id = fid; tk.plog = lg[fid] - lse; tk.p = skw_expf(tk.plog); }
}
// The same draw by the whole workgroup.  What libstdc++ defines is sequential — sum = p_0 + p_1 + ... in f64, q_i = p_i / sum, cp_i = q_0 + ... + q_i, the first
// cp_i >= u — and the two sums stay one lane's k-ascending chains (their roundings ARE the definition).  But one lane fetching 51 865 floats from memory one at
// a time and dividing each by the sum inside the chain made a sampled step 5.8 ms (a long-form batch with temperature fall-backs: 4.5 s of a 6.4 s call).  Here
// the workgroup stages the row through LDS (64 KB at a time), the divisions — independent — are done by all threads, and the second chain stops at the hit.
// Same bits as discrete_draw (oracle/skw_oracle.c).  lds: 8 192 floats = 4 096 doubles (static LDS stays under 64 KB).
// S + p == S under round-to-nearest whenever 0 <= p < ulp(S) / 2: a 64-element block whose largest element is below that bound cannot move the running sum,
// whatever the order inside it, and since the sum never decreases it stays immovable — such blocks are skipped WITHOUT changing a bit of the sequential result.
// (Peaked distributions — most real steps — leave a few dozen elements in the chain; a flat one keeps all 51 865.)
// The serial walks themselves (the half-ulp bound, the first chain's sum, the second chain's cp with its block-end compare and last-element rule) are
// include/skw_draw.h: host and device, held to the sequential definition on the CPU by tests/cpp/draw_main.cpp.
__device__ int block_discrete_draw(const float* probs, double* q, int n, uint32_t* mt, float* lds, double* s_sum, int* s_hit) {
    const int tid = threadIdx.x, nt = blockDim.x;
    __shared__ double bmax[SKW_DRAW_CHUNK / SKW_DRAW_BLOCK];      // per 64-element block of the staged chunk
    double* ldsd = (double*)lds;                                 // the chunk as doubles: 4 096 per stage (the serial lane then issues one LDS read and two adds per two elements)
    double sum = 0.0;
    for (int c0 = 0; c0 < n; c0 += SKW_DRAW_CHUNK) {
        const int m = min(SKW_DRAW_CHUNK, n - c0);
        for (int i = tid; i < m; i += nt) ldsd[i] = (double)probs[c0 + i];
        __syncthreads();
        if (tid < 64) { double mx = 0.0; for (int i = tid * 64; i < min(tid * 64 + 64, m); ++i) mx = fmax(mx, ldsd[i]); bmax[tid] = mx; }
        __syncthreads();
        if (tid == 0) sum = skw_draw_sum_chunk(ldsd, bmax, m, sum, nullptr);
        __syncthreads();
    }
    if (tid == 0) {
        double cs = 0.0, tmp = 1.0;
        for (int k = 0; k < 2; ++k) { cs += (double)mt_next(mt) * tmp; tmp *= 4294967296.0; }
        double u = cs / tmp; if (u >= 1.0) u = 0.99999999999999988897769753748;   // nextafter(1.0, 0.0)
        s_sum[0] = sum; s_sum[1] = u; *s_hit = -1;
    }
    __syncthreads();
    sum = s_sum[0]; const double u = s_sum[1];
    for (int i = tid; i < n; i += nt) q[i] = (double)probs[i] / sum;
    __threadfence_block();
    __syncthreads();
    double cp = 0.0;
    for (int c0 = 0; c0 < n; c0 += SKW_DRAW_CHUNK) {
        const int m = min(SKW_DRAW_CHUNK, n - c0);
        for (int i = tid; i < m; i += nt) ldsd[i] = q[c0 + i];
        __syncthreads();
        if (tid < 64) { double mx = 0.0; for (int i = tid * 64; i < min(tid * 64 + 64, m); ++i) mx = fmax(mx, ldsd[i]); bmax[tid] = mx; }
        __syncthreads();
        if (tid == 0) *s_hit = skw_draw_cp_chunk(ldsd, bmax, m, c0, n, u, &cp, nullptr);
        __syncthreads();
        if (*s_hit >= 0) break;      // (uniform)
        __syncthreads();
    }
    const int h = *s_hit;
    return h >= 0 ? h : n - 1;
}

// one packed static mask: n_vocab bytes padded to 16, then the transposed bits (two 64-bit words per thread of the register-resident sampler; SMP_NT below)
__host__ __device__ inline size_t smp_mask_bytes(int n_vocab) { return (size_t)((n_vocab + 15) & ~15) + 2 * 512 * sizeof(unsigned long long); }
// a row's own rules into the launch's parameter block; returns the row's mask of the pair [without | with the non-speech list]
__device__ __forceinline__ const uint8_t* smp_row_rules(SkwLogitParams& p, const SkwRowRules& r, const uint8_t* mask_pair) {
    p.suppress_blank = r.suppress_blank; p.suppress_nst = r.suppress_nst; p.no_timestamps = r.no_timestamps; p.single_segment = r.single_segment;
    p.max_tokens = r.max_tokens; p.tid0_initial = r.tid0_initial;
    return mask_pair + (r.suppress_nst ? smp_mask_bytes(p.n_vocab) : 0);
}
// ---- what both sampler forms share: the prompt feed, the index rules of whisper_process_logits, the commit tail.  Each form keeps its own reductions and passes.
// The shapes below are the ones that leave every instantiation's registers, LDS and occupancy where the spelled-out text had them (profiles/kernels_split): the feed's test
// stays a branch of the kernel, the index rule takes its parameters by value, `sampled` travels as an int.
// Still feeding the prompt ([prev] + past text + sot/lang/task; uniform per block): the row takes its next prompt token, nothing is sampled and the kernel returns
__device__ __forceinline__ bool smp_in_prompt(const SkwSeqState* st) { return st->cur_pos < st->n_prompt - 1; }
__device__ __forceinline__ void smp_feed_prompt(SkwSeqState* st, const int* prompt_buf, int b) {
    if (threadIdx.x == 0) { const int np = st->cur_pos + 1; st->cur_token = prompt_buf[(long)b * SKW_PROMPT_CAP + np]; st->cur_pos = np; }
}
// the facts of a row that the index rules depend on, from its token count, its last two tokens and the window's timestamp floor
struct SmpRowFacts { bool is_initial, last_ts, pen_ts; int has_ts, ts_lo; };
__device__ __forceinline__ SmpRowFacts smp_row_facts(const SkwLogitParams& p, const SkwSeqState* st, const SkwTokenOut* toks, int n_tok) {
    SmpRowFacts f;
    const int last_id = n_tok > 0 ? toks[n_tok - 1].id : -1;
    const int pen_id = n_tok > 1 ? toks[n_tok - 2].id : -1;
    f.is_initial = n_tok == 0;
    f.last_ts = n_tok > 0 && last_id >= p.tok_beg;
    f.pen_ts = n_tok < 2 || pen_id >= p.tok_beg;
    f.has_ts = st->has_ts; f.ts_lo = f.has_ts ? p.tok_beg + st->seek_delta / 2 : 0;
    return f;
}
// whisper_process_logits' rules on the index i: blank, no_timestamps, timestamp pairing, max_initial_ts, monotonic timestamps.  kill: what the static mask says of i.
__device__ __forceinline__ bool smp_index_killed(bool kill, int i, SkwLogitParams p, SmpRowFacts f) {
    if (f.is_initial && p.suppress_blank && (i == p.tok_eot || i == p.tok_space)) kill = true;
    if (p.no_timestamps && i >= p.tok_beg) kill = true;
    if (f.last_ts) { if (f.pen_ts) { if (i >= p.tok_beg) kill = true; } else { if (i < p.tok_eot) kill = true; } }
    if (f.is_initial && p.tid0_initial >= 0 && i >= p.tok_beg + p.tid0_initial + 1) kill = true;
    if (f.has_ts && i >= p.tok_beg && i < f.ts_lo) kill = true;
    return kill;
}
// The commit tail, by the row's thread 0: tk holds the chosen token (id, p, plog); the timestamp fields, the margin, the token store, the token loop's update and the live flag
__device__ __forceinline__ void smp_commit(SkwTokenOut& tk, const ArgBest& bts, double sum_ts, int sampled, float t1, float t2, int i, int max_tok, const SkwLogitParams& p,
                                           SkwSeqState* st, SkwTokenOut* toks, int* n_active, int b) {
    tk.tid = (bts.v > 0.0f) ? bts.i : 0; tk.pt = (float)((double)bts.v / (sum_ts + 1e-10)); tk.ptsum = (float)sum_ts;
    if (tk.id >= p.tok_beg) { tk.tid = tk.id; tk.pt = tk.p; }
    tk.margin = (!sampled && t2 > -INFINITY) ? t1 - t2 : INFINITY;
    if (!sampled && t2 > -INFINITY && t1 - t2 < st->min_margin) st->min_margin = t1 - t2;   // argmax passes only (diagnostic)
    if (i < max_tok) toks[i] = tk;
    st->n_tokens = i + 1;
    const int done = skw_token_loop_update(*st, tk.id, i, p.tok_beg, p.tok_eot, p.max_tokens, p.no_timestamps, p.single_segment, p.n_max);
    st->cur_token = tk.id; st->cur_pos = st->n_prompt + i;
    if (done) { st->active = 0; n_active[b] = 0; }     // the row's live flag, in host-mapped memory: the host reads it after the stream drains (no copy kernel in the step)
}
// ROWS (both sampler forms): the request's rules come from rules[row] in device memory instead of the by-value p, and the row picks its static mask out of the
//  pair (skw_full_batch_mixed: rows of one launch decode under different skw_full_params); p then carries the model constants only
template <bool ROWS>
__global__ __launch_bounds__(1024) void k_dec_sample_stream(float* logits_all, const uint8_t* static_mask, SkwLogitParams p, SkwSeqState* st_all, SkwTokenOut* toks_all,
                                                     int max_tok, int* n_active, float* probs_all, uint32_t* rng_all, const int* clip_idx, const int* prompt_buf,
                                                     const int* forced, SkwTraceStep* trace, const SkwRowRules* rules) {
    __shared__ float sh_f[16]; __shared__ double sh_d[16]; __shared__ ArgBest sh_a[16];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    SkwSeqState* st = &st_all[b];
    if (!st->active) return;   // uniform per block
    if (smp_in_prompt(st)) { smp_feed_prompt(st, prompt_buf, b); return; }
    float* lg = logits_all + (long)b * p.n_vocab;
    const int NV = p.n_vocab;
    if constexpr (ROWS) static_mask = smp_row_rules(p, rules[b], static_mask);
    SkwTokenOut* toks = toks_all + (long)b * max_tok;
    const int n_tok = st->n_tokens;
    const bool is_initial = n_tok == 0;
    float mx, lse;
    if (is_initial) {   // no_speech_prob from the unfiltered distribution
        block_lse(lg, 0, NV, sh_f, sh_d, &mx, &lse);
        if (tid == 0) st->no_speech_prob = skw_expf(lg[p.tok_nosp] - lse);
    }
    const float temperature = st->temperature;
    if (temperature > 0.0f) { __syncthreads(); for (int i = tid; i < NV; i += nt) lg[i] = lg[i] / temperature; __syncthreads(); }   // before any filter
    const SmpRowFacts facts = smp_row_facts(p, st, toks, n_tok);
    for (int i = tid; i < NV; i += nt) if (smp_index_killed(static_mask[i] != 0, i, p, facts)) lg[i] = -INFINITY;
    __syncthreads();
    block_lse(lg, 0, NV, sh_f, sh_d, &mx, &lse);
    // timestamp mass rule, on logprobs = logits - lse
    float ts_logprob = -INFINITY;
    {
        float m = -INFINITY;
        for (int i = p.tok_beg + tid; i < NV; i += nt) { float v = lg[i]; if (v > -INFINITY) m = fmaxf(m, v - lse); }
        m = block_max(m, sh_f);
        double acc = 0.0;
        for (int i = p.tok_beg + tid; i < NV; i += nt) { float v = lg[i]; if (v > -INFINITY) acc += (double)skw_expf((v - lse) - m); }
        acc = block_sum_f64(acc, sh_d);
        if (acc > 0.0) ts_logprob = skw_logf((float)acc) + m;
    }
    float max_text = -INFINITY;
    for (int i = tid; i < p.tok_beg; i += nt) { float v = lg[i]; if (v > -INFINITY) max_text = fmaxf(max_text, v - lse); }
    max_text = block_max(max_text, sh_f);
    const bool force_ts = ts_logprob > max_text;
    const int lo = force_ts ? p.tok_beg : 0;
    if (force_ts) { for (int i = tid; i < p.tok_beg; i += nt) lg[i] = -INFINITY; __syncthreads(); }
    // best token over probs = expf(logprob), first index wins ties; timestamp statistics
    ArgBest best = {0.0f, 0}, bts = {0.0f, 0x7fffffff};
    double sum_ts = 0.0; float top1 = -INFINITY, top2 = -INFINITY;
    const bool sampled = temperature > 0.0f;
    float* probs = probs_all + (long)b * skw_probs_row_floats(NV);
    if (sampled) { for (int i = tid; i < NV; i += nt) probs[i] = 0.0f; __syncthreads(); }   // (the loop below starts at lo: another thread owns the entry)
    for (int i = lo + tid; i < NV; i += nt) {
        float v = lg[i];
        if (v > -INFINITY) {
            float pr = skw_expf(v - lse);
            if (sampled) probs[i] = pr;
            ArgBest c = {pr, i}; if (pr > best.v || (pr == best.v && i < best.i)) best = c;
            if (i >= p.tok_beg) { sum_ts += (double)pr; if (pr > bts.v || (pr == bts.v && pr > 0.0f && i < bts.i)) { bts.v = pr; bts.i = i; } }
            if (v > top1) { top2 = top1; top1 = v; } else if (v > top2) top2 = v;
        }
    }
    best = block_argbest(best, sh_a);
    bts = block_argbest(bts, sh_a);
    sum_ts = block_sum_f64(sum_ts, sh_d);
    // margin between the two largest admissible logits
    float t1 = block_max(top1, sh_f);
    float cand = (top1 == t1) ? top2 : top1;
    float t2 = block_max(cand, sh_f);
    // an exact duplicate of the maximum in ANOTHER thread is the runner-up (margin 0, as the sequential rule and the register-resident form have it): a thread that holds
    // the maximum offers only its own second value above
    if (block_sum_f64(top1 == t1 ? 1.0 : 0.0, sh_d) > 1.0) t2 = t1;
    if (sampled) { __threadfence_block(); __syncthreads(); }
    if (tid != 0) return;
    SkwTokenOut tk; tk.id = best.i; tk.p = best.v;
    if (sampled) { tk.id = discrete_draw(probs, NV, rng_all + (long)clip_idx[b] * SKW_RNG_WORDS); tk.p = probs[tk.id]; }
    tk.plog = lg[tk.id] - lse;
    const int i = n_tok;
    smp_trace_step(tk, lg, lse, i, max_tok, b, forced, trace, best.i, -1, t1, t2, p, temperature);
    smp_commit(tk, bts, sum_ts, sampled, t1, t2, i, max_tok, p, st, toks, n_active, b);
}
// Register-resident form: the row's logits (<= 104 per thread) are loaded once, every pass of whisper_process_logits then runs on
// registers -- the streaming form above re-reads the row from L2 six times with nothing to overlap the latency (90 us per step).
// Same operations per logit; skw_expf(-inf) == 0, so suppressed logits need no branches; exponentials go two at a time through
// packed math; f64 partial sums are grouped differently, which the f64 accumulation makes immaterial (D1).
#define SMP_PT 104
#define SMP_NT 512      // 8 waves: 2 per SIMD, so the 104 resident logits fit the 256-VGPR budget
#define SMP_TX 96       // stripes [0, SMP_TX) hold text tokens only in every Whisper vocabulary (tok_eot = 50256 / 50257 >= 96 * 512)
struct SmpMain { ArgBest best; float best_logit; ArgBest bts; double sum_ts; float top1, top2; };
// element index of slot c: recomputed inside each pass from a value the optimiser cannot see through -- shared across passes, the
// ~100 indices would stay live for the whole kernel and push the logits into scratch
#define SMP_PASS_BEGIN { int tq = tid; asm volatile("" : "+v"(tq));
#define SMP_PASS_END }
#define SMP_IDX(c) (tq + SMP_NT * (c))
// TRACE: the trace / teacher-forced form (one more pass for the runner-up's index); DRAW: rows at a temperature > 0 may be present (the workgroup-wide draw and its LDS
//  staging are compiled in); the greedy step's graph holds <false, false>
template <bool TRACE, bool DRAW, bool ROWS>
__global__ __launch_bounds__(SMP_NT) void k_dec_sample(float* logits_all, const uint8_t* static_mask, SkwLogitParams p, SkwSeqState* st_all, SkwTokenOut* toks_all,
                                                       int max_tok, int* n_active, float* probs_all, uint32_t* rng_all, const int* clip_idx, const int* prompt_buf,
                                                       const int* forced, SkwTraceStep* trace, const SkwRowRules* rules) {
    __shared__ float sh_f[2][SMP_NT / 64]; __shared__ double sh_d[SMP_NT / 64]; __shared__ SmpMain sh_m[SMP_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    SkwSeqState* st = &st_all[b];
    if (!st->active) return;   // uniform per block
    if (smp_in_prompt(st)) { smp_feed_prompt(st, prompt_buf, b); return; }
    float* lg = logits_all + (long)b * p.n_vocab;
    const int NV = p.n_vocab;
    if constexpr (ROWS) static_mask = smp_row_rules(p, rules[b], static_mask);
    SkwTokenOut* toks = toks_all + (long)b * max_tok;
    const int n_tok = st->n_tokens;
    const bool is_initial = n_tok == 0;
    float v[SMP_PT]; unsigned long long killbits[2];
    { const unsigned long long* kw = (const unsigned long long*)(static_mask + ((NV + 15) & ~15)); killbits[0] = kw[tid]; killbits[1] = kw[SMP_NT + tid]; }
#pragma unroll
    for (int c = 0; c < SMP_PT; ++c) {
        if (SMP_NT * (c + 1) <= NV) v[c] = lg[tid + SMP_NT * c];                                  // whole stripe inside the row (uniform test)
        else { const int i = tid + SMP_NT * c; v[c] = (i < NV) ? lg[i] : -INFINITY; }
    }
    const SmpRowFacts facts = smp_row_facts(p, st, toks, n_tok);
    const float temperature = st->temperature;
    auto bmax2 = [&](float a, float c2, float* oa, float* oc) {     // two block-wide maxima with one exchange
        a = skw_wave_max_f32(a); c2 = skw_wave_max_f32(c2);
        if (lane == 0) { sh_f[0][w] = a; sh_f[1][w] = c2; }
        __syncthreads();
        float ra = sh_f[0][0], rc = sh_f[1][0];
        for (int k = 1; k < SMP_NT / 64; ++k) { ra = fmaxf(ra, sh_f[0][k]); rc = fmaxf(rc, sh_f[1][k]); }
        __syncthreads();
        *oa = ra; *oc = rc;
    };
    float dummy;
    if (is_initial) {   // no_speech_prob from the unfiltered distribution
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < SMP_PT; ++c) m = fmaxf(m, v[c]);
        bmax2(m, m, &m, &dummy);
        double acc0 = 0.0;
#pragma unroll
        for (int c = 0; c < SMP_PT; c += 2) {
            f32x2 e = expf_nonpos_x2((f32x2){v[c], v[c + 1]} - (f32x2){m, m}); acc0 += (double)e[0]; acc0 += (double)e[1];
            if ((c & 7) == 6) __builtin_amdgcn_sched_barrier(0);   // keeps the scheduler from overlapping dozens of exponentials and spilling
        }
        acc0 = block_sum_f64(acc0, sh_d);
        const float lse0 = (acc0 > 0.0) ? skw_logf((float)acc0) + m : -INFINITY;
        SMP_PASS_BEGIN
#pragma unroll
        for (int c = 0; c < SMP_PT; ++c) if (SMP_IDX(c) == p.tok_nosp) st->no_speech_prob = skw_expf(v[c] - lse0);
        SMP_PASS_END
    }
    if (temperature > 0.0f) {
#pragma unroll
        for (int c = 0; c < SMP_PT; ++c) v[c] = v[c] / temperature;      // before any filter
    }
    // stripes [0, tx) hold text tokens only (every index below both tok_eot and tok_beg): there the index rules reduce to block-uniform
    // conditions plus the blank rule's tok_space, and no pass needs a per-lane index compare — 98 of the 104 stripes of the multilingual vocabulary
    constexpr int tx = SMP_TX;      // (compile-time: the index rules are then only compiled for the last SMP_PT - SMP_TX stripes; the host checks tok_eot, tok_beg >= SMP_TX * SMP_NT)
    const bool text_all_killed = facts.last_ts && !facts.pen_ts;            // "a lone timestamp must be followed by a timestamp": every token below tok_eot goes
    // (the blank rule's tok_space joins the static kill bits of the thread that owns it, so a text stripe's rule is one bit test: written with
    //  index compares, hipcc turned the rules into 104 scalar lane masks, spilled through v_writelane, ~50 instructions and four branches per logit)
    if (is_initial && p.suppress_blank) {
        const int cs = p.tok_space / SMP_NT;
        if (tid == p.tok_space % SMP_NT && cs < SMP_PT) { if (cs < 64) killbits[0] |= 1ull << cs; else killbits[1] |= 1ull << (cs - 64); }
    }
    if (text_all_killed) {      // (uniform)
#pragma unroll
        for (int c = 0; c < SMP_PT; ++c) if (c < tx) v[c] = -INFINITY;
    }
    SMP_PASS_BEGIN
#pragma unroll
    for (int c = 0; c < SMP_PT; ++c) {
        const int i = SMP_IDX(c);
        bool kill = (killbits[c >> 6] >> (c & 63)) & 1;
        if (c < tx) {      // (uniform)
            v[c] = kill ? -INFINITY : v[c];
            continue;
        }
        if (smp_index_killed(kill, i, p, facts)) v[c] = -INFINITY;
    }
    SMP_PASS_END
    // log-softmax statistics of the admissible logits
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < SMP_PT; ++c) mx = fmaxf(mx, v[c]);
    bmax2(mx, mx, &mx, &dummy);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < SMP_PT; c += 2) {
        f32x2 e = expf_nonpos_x2((f32x2){v[c], v[c + 1]} - (f32x2){mx, mx}); acc += (double)e[0]; acc += (double)e[1];
        if ((c & 7) == 6) __builtin_amdgcn_sched_barrier(0);
    }
    acc = block_sum_f64(acc, sh_d);
    const float lse = (acc > 0.0) ? skw_logf((float)acc) + mx : -INFINITY;
    // timestamp mass rule, on logprobs = logits - lse
    float m_ts = -INFINITY, max_text = -INFINITY;
    SMP_PASS_BEGIN
#pragma unroll
    for (int c = 0; c < SMP_PT; ++c) { const float lp = v[c] - lse;
    if (c < tx) max_text = fmaxf(max_text, lp); else if (SMP_IDX(c) >= p.tok_beg) m_ts = fmaxf(m_ts, lp); else max_text = fmaxf(max_text, lp); }
    SMP_PASS_END
    bmax2(m_ts, max_text, &m_ts, &max_text);
    double acc_ts = 0.0;
    SMP_PASS_BEGIN
#pragma unroll
    for (int c = 0; c < SMP_PT; ++c) {
        if (c >= tx && SMP_NT * (c + 1) > p.tok_beg) {     // (uniform) only the last few stripes reach the timestamp range
            const float e = skw_expf((v[c] - lse) - m_ts);
            if (SMP_IDX(c) >= p.tok_beg) acc_ts += (double)e;
        }
    }
    SMP_PASS_END
    acc_ts = block_sum_f64(acc_ts, sh_d);
    const float ts_logprob = (acc_ts > 0.0) ? skw_logf((float)acc_ts) + m_ts : -INFINITY;
    const bool force_ts = ts_logprob > max_text;
    if (force_ts) {
        SMP_PASS_BEGIN
#pragma unroll
        for (int c = 0; c < SMP_PT; ++c) if (c < tx || SMP_IDX(c) < p.tok_beg) v[c] = -INFINITY;
        SMP_PASS_END
    }
    // The two largest admissible logits and the owner of the largest (order-free; also the margin diagnostic).  exp is increasing and
    // skw_expf follows it to a couple of ulps, so a logit more than 1e-4 below another has a strictly smaller probability (1e-4 is ~1700 ulps
    // of the ratio): when the runner-up is that far down, the winner of "largest probability, first index on ties" is the owner of
    // the largest logit, and the only exponentials the step still needs are the timestamp stripes' (their sum and their best).  Otherwise —
    // a near-tie, or a temperature pass that needs every probability — the whole row goes through the pass, as before.  Same bits either way.
    const bool sampled = DRAW && temperature > 0.0f;
    float* probs = probs_all + (long)b * skw_probs_row_floats(NV);
    float t1 = -INFINITY, t2 = -INFINITY; int i1 = 0;
    SMP_PASS_BEGIN
#pragma unroll
    // (selects, not branches; i1 counts stripes here)
    for (int c = 0; c < SMP_PT; ++c) { const float x = v[c]; const bool gt = x > t1; t2 = gt ? t1 : fmaxf(t2, x); i1 = gt ? c : i1; t1 = gt ? x : t1; }
    i1 = SMP_IDX(i1);
    SMP_PASS_END
    for (int o = 32; o > 0; o >>= 1) {
        const float o1 = __shfl_xor(t1, o, 64), o2 = __shfl_xor(t2, o, 64); const int oi = __shfl_xor(i1, o, 64);
        if (o1 > t1 || (o1 == t1 && oi < i1)) { t2 = fmaxf(t1, o2); t1 = o1; i1 = oi; } else t2 = fmaxf(t2, o1);
    }
    __shared__ float sh_t1[SMP_NT / 64], sh_t2[SMP_NT / 64]; __shared__ int sh_i1[SMP_NT / 64];
    if (lane == 0) { sh_t1[w] = t1; sh_t2[w] = t2; sh_i1[w] = i1; }
    __syncthreads();
    t1 = sh_t1[0]; t2 = sh_t2[0]; i1 = sh_i1[0];
    for (int k = 1; k < SMP_NT / 64; ++k) { const float o1 = sh_t1[k], o2 = sh_t2[k]; const int oi = sh_i1[k];
        if (o1 > t1 || (o1 == t1 && oi < i1)) { t2 = fmaxf(t1, o2); t1 = o1; i1 = oi; } else t2 = fmaxf(t2, o1); }
    int i2 = 0x7fffffff;
    if (TRACE) {      // owner of the runner-up: lowest index other than i1 that holds t2
        SMP_PASS_BEGIN
#pragma unroll
        for (int c = 0; c < SMP_PT; ++c) { const int i = SMP_IDX(c); if (v[c] == t2 && i != i1 && i < i2) i2 = i; }
        SMP_PASS_END
        for (int o = 32; o > 0; o >>= 1) i2 = min(i2, __shfl_xor(i2, o, 64));
        __syncthreads();
        if (lane == 0) sh_i1[w] = i2;
        __syncthreads();
        i2 = sh_i1[0]; for (int k = 1; k < SMP_NT / 64; ++k) i2 = min(i2, sh_i1[k]);
    }
    const bool fast = !sampled && (t1 - t2 > 1e-4f);           // (t2 == -inf: a single admissible token)
    const int c_lo = fast ? tx : 0;
    // best token over probs = expf(logprob), first index wins ties; timestamp statistics
    SmpMain r; r.best = {0.0f, 0}; r.best_logit = -INFINITY; r.bts = {0.0f, 0x7fffffff}; r.sum_ts = 0.0; r.top1 = t1; r.top2 = t2;
    SMP_PASS_BEGIN
#pragma unroll
    for (int c = 0; c < SMP_PT; c += 2) {
        if (c < c_lo) continue;      // (uniform)
        const f32x2 e2 = expf_nonpos_x2((f32x2){v[c], v[c + 1]} - (f32x2){lse, lse});     // 0 for suppressed logits: they can win nothing below
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = SMP_IDX(c + u); const float x = v[c + u]; const float pr = e2[u];
            if (pr > r.best.v || (pr == r.best.v && i < r.best.i)) { r.best.v = pr; r.best.i = i; r.best_logit = x; }
            if (c >= tx && i >= p.tok_beg) { r.sum_ts += (double)pr; if (pr > r.bts.v || (pr == r.bts.v && pr > 0.0f && i < r.bts.i)) { r.bts.v = pr; r.bts.i = i; } }
            if (sampled && i < NV) { probs[i] = pr; lg[i] = x; }     // the draw (one lane, below) walks the row in memory
        }
        if ((c & 7) == 6) __builtin_amdgcn_sched_barrier(0);
    }
    SMP_PASS_END
    if (fast && tid == 0) {      // the row's winner, wherever its stripe is: (probability, index) beats whatever the timestamp stripes hold
        const f32x2 e1 = expf_nonpos_x2((f32x2){t1, t1} - (f32x2){lse, lse});
        if (e1[0] > r.best.v || (e1[0] == r.best.v && i1 < r.best.i)) { r.best.v = e1[0]; r.best.i = i1; r.best_logit = t1; }
    }
    auto comb = [](SmpMain a, const SmpMain& c2) {
        if (c2.best.v > a.best.v || (c2.best.v == a.best.v && c2.best.i < a.best.i)) { a.best = c2.best; a.best_logit = c2.best_logit; }
        a.bts = better(a.bts, c2.bts); a.sum_ts += c2.sum_ts;
        return a;
    };
    for (int o = 32; o > 0; o >>= 1) {
        SmpMain y;
        y.best.v = __shfl_xor(r.best.v, o, 64); y.best.i = __shfl_xor(r.best.i, o, 64); y.best_logit = __shfl_xor(r.best_logit, o, 64);
        y.bts.v = __shfl_xor(r.bts.v, o, 64); y.bts.i = __shfl_xor(r.bts.i, o, 64); y.sum_ts = __shfl_xor(r.sum_ts, o, 64);
        y.top1 = t1; y.top2 = t2;
        r = comb(r, y);
    }
    if (lane == 0) sh_m[w] = r;
    if (sampled) __threadfence_block();
    __syncthreads();
    int drawn = -1;
    if constexpr (DRAW) if (sampled) {      // (uniform) every thread takes part in the draw
        __shared__ __attribute__((aligned(16))) float draw_lds[8192]; __shared__ double draw_s[2]; __shared__ int draw_hit;
        drawn = block_discrete_draw(probs, (double*)(probs + ((NV + 1) & ~1)), NV, rng_all + (long)clip_idx[b] * SKW_RNG_WORDS, draw_lds, draw_s, &draw_hit);
    }
    if (tid != 0) return;
    r = sh_m[0]; for (int k = 1; k < SMP_NT / 64; ++k) r = comb(r, sh_m[k]);
    const ArgBest best = r.best, bts = r.bts; const double sum_ts = r.sum_ts;
    SkwTokenOut tk; tk.id = best.i; tk.p = best.v; tk.plog = r.best_logit - lse;
    if (sampled) { tk.id = drawn; tk.p = probs[tk.id]; tk.plog = lg[tk.id] - lse; }
    const int i = n_tok;
    if (TRACE) smp_trace_step(tk, lg, lse, i, max_tok, b, forced, trace, i1, i2, t1, t2, p, temperature);
    smp_commit(tk, bts, sum_ts, sampled, t1, t2, i, max_tok, p, st, toks, n_active, b);
}
static_assert(SMP_NT == 512, "smp_mask_bytes restates SMP_NT");
size_t skw_static_mask_bytes(int n_vocab) { return smp_mask_bytes(n_vocab); }
void skw_static_mask_pack(const uint8_t* mask, int n_vocab, uint8_t* out) {
    memset(out, 0, skw_static_mask_bytes(n_vocab)); memcpy(out, mask, n_vocab);
    unsigned long long* kw = (unsigned long long*)(out + ((n_vocab + 15) & ~15));
    for (int i = 0; i < n_vocab && i < SMP_PT * SMP_NT; ++i) if (mask[i]) { const int t = i % SMP_NT, c = i / SMP_NT; kw[(c >> 6) * SMP_NT + t] |= 1ull << (c & 63); }
}
static int g_force_stream_sampler = 0;      // tests: run the streaming form where the register-resident one would (it leaves the filtered row in memory)
void skw_debug_force_stream_sampler(int on) { g_force_stream_sampler = on; }
// which sampler a launch runs: the function the launcher itself branches on (tests assert it through skw_debug_sample_rows_ex)
int skw_dec_sample_kernel(const SkwLogitParams& p, bool trace, bool rows) {
    if (!g_force_stream_sampler && p.n_vocab <= SMP_PT * SMP_NT && std::min(p.tok_eot, p.tok_beg) >= SMP_TX * SMP_NT)
        return (trace ? SKW_SMPK_TRACE | SKW_SMPK_DRAW : p.any_sampled ? SKW_SMPK_DRAW : 0) | (rows ? SKW_SMPK_ROWS : 0);
    return SKW_SMPK_STREAM | (rows ? SKW_SMPK_ROWS : 0);
}
template <bool ROWS>
static void dec_sample_launch(float* logits, const uint8_t* static_mask, const SkwLogitParams& p, SkwSeqState* st, SkwTokenOut* toks, int max_tok, int B, int* n_active,
                              float* probs, uint32_t* rng, const int* clip_idx, const int* prompt_buf, hipStream_t s, const int* forced, SkwTraceStep* trace, const SkwRowRules* rules) {
    const int k = skw_dec_sample_kernel(p, trace != nullptr, ROWS);
    if (k & SKW_SMPK_STREAM) hipLaunchKernelGGL(k_dec_sample_stream<ROWS>, dim3(B), dim3(1024), 0, s, logits, static_mask, p, st, toks, max_tok, n_active, probs, rng, clip_idx,
        prompt_buf, forced, trace, rules);
    else if (k & SKW_SMPK_TRACE) hipLaunchKernelGGL((k_dec_sample<true, true, ROWS>), dim3(B), dim3(SMP_NT), 0, s, logits, static_mask, p, st, toks, max_tok, n_active, probs, rng,
        clip_idx, prompt_buf, forced, trace, rules);
    else if (k & SKW_SMPK_DRAW) hipLaunchKernelGGL((k_dec_sample<false, true, ROWS>), dim3(B), dim3(SMP_NT), 0, s, logits, static_mask, p, st, toks, max_tok, n_active, probs,
        rng, clip_idx, prompt_buf, nullptr, nullptr, rules);
    else hipLaunchKernelGGL((k_dec_sample<false, false, ROWS>), dim3(B), dim3(SMP_NT), 0, s, logits, static_mask, p, st, toks, max_tok, n_active, probs, rng, clip_idx, prompt_buf,
        nullptr, nullptr, rules);
}
void skw_dec_sample(float* logits, const uint8_t* static_mask, SkwLogitParams p, SkwSeqState* st, SkwTokenOut* toks, int max_tok, int B, int* n_active,
                    float* probs, uint32_t* rng, const int* clip_idx, const int* prompt_buf, hipStream_t s, const int* forced, SkwTraceStep* trace) {
    dec_sample_launch<false>(logits, static_mask, p, st, toks, max_tok, B, n_active, probs, rng, clip_idx, prompt_buf, s, forced, trace, nullptr);
}
void skw_dec_sample_rows(float* logits, const uint8_t* static_mask_pair, SkwLogitParams p, const SkwRowRules* rules, SkwSeqState* st, SkwTokenOut* toks, int max_tok, int B, int* n_active,
                         float* probs, uint32_t* rng, const int* clip_idx, const int* prompt_buf, hipStream_t s, const int* forced, SkwTraceStep* trace) {
    dec_sample_launch<true>(logits, static_mask_pair, p, st, toks, max_tok, B, n_active, probs, rng, clip_idx, prompt_buf, s, forced, trace, rules);
}

// ------------------------------------------------------------------ decoding constraints (skw_full_batch_rules): bias, repetition penalty, no-repeat n-gram
// One workgroup per row, ahead of the sampler and outside it (k_dec_sample's registers are spoken for).  T = the text tokens (id < tok_eot) among the row's sampled tokens of
// this pass, compacted into LDS in order (a ballot per wave, the waves' counts through LDS); then three phases on the row in global memory, a barrier between them:
//   bias      one thread per pair; the ids are distinct (host-checked), so no two threads meet
//   penalty   one thread per element of T, and only the FIRST occurrence of an id acts: it reads what the bias phase left and writes once, so a token seen three times is penalised once
//   n-gram    one thread per candidate start i: T[i .. i+N-1) against the last N-1 text tokens; a match bans T[i+N-1] (several threads may store the same -inf)
#define CONSTRAIN_NT 256
__global__ __launch_bounds__(CONSTRAIN_NT) void k_dec_constrain(float* logits_all, int n_vocab, int tok_eot, const SkwRowConstraints* cons, const SkwSeqState* st_all,
                                                                const SkwTokenOut* toks_all, int max_tok) {
    extern __shared__ int s_T[];      // [max_tok]
    __shared__ int s_cnt[CONSTRAIN_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const SkwSeqState* st = &st_all[b];
    if (!st->active) return;                        // (all three uniform per block)
    if (smp_in_prompt(st)) return;     // still feeding the prompt: the sampler does not sample either
    const SkwRowConstraints& r = cons[b];
    const float theta = r.penalty; const int N = r.ngram, n_bias = min(r.n_bias, SKW_CONSTRAIN_BIAS_MAX);
    if (theta == 1.0f && N == 0 && n_bias <= 0) return;
    float* lg = logits_all + (long)b * n_vocab;
    const SkwTokenOut* toks = toks_all + (long)b * max_tok;
    const int n = min(st->n_tokens, max_tok);
    int m = 0;
    for (int c0 = 0; c0 < n; c0 += CONSTRAIN_NT) {      // (one round for every Whisper model: max_tok = n_text_ctx / 2 = 224)
        const int i = c0 + tid; const int id = i < n ? toks[i].id : 0x7fffffff;
        const bool text = id >= 0 && id < tok_eot;
        const unsigned long long bal = __ballot(text);
        if (lane == 0) s_cnt[w] = __popcll(bal);
        __syncthreads();
        int off = m; for (int k = 0; k < w; ++k) off += s_cnt[k];
        if (text) s_T[off + __popcll(bal & ((1ull << lane) - 1ull))] = id;
        for (int k = 0; k < CONSTRAIN_NT / 64; ++k) m += s_cnt[k];
        __syncthreads();
    }
    for (int k = tid; k < n_bias; k += CONSTRAIN_NT) { const int id = r.bias_id[k]; if (id >= 0 && id < n_vocab) lg[id] = lg[id] + r.bias[k]; }
    __syncthreads();
    if (theta != 1.0f) for (int j = tid; j < m; j += CONSTRAIN_NT) {
        const int t = s_T[j]; bool first = true;
        for (int i = 0; i < j; ++i) if (s_T[i] == t) { first = false; break; }
        if (first) { const float x = lg[t]; lg[t] = x < 0.0f ? x * theta : x / theta; }
    }
    __syncthreads();
    if (N >= 1 && m >= N) for (int i = tid; i <= m - N; i += CONSTRAIN_NT) {
        bool same = true;
        for (int k = 0; k < N - 1; ++k) if (s_T[i + k] != s_T[m - N + 1 + k]) { same = false; break; }
        if (same) lg[s_T[i + N - 1]] = -INFINITY;
    }
}
void skw_dec_constrain(float* logits, int n_vocab, int tok_eot, const SkwRowConstraints* cons, const SkwSeqState* st, const SkwTokenOut* toks, int max_tok, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_constrain, dim3(B), dim3(CONSTRAIN_NT), sizeof(int) * (size_t)max_tok, s, logits, n_vocab, tok_eot, cons, st, toks, max_tok);
}
