// skw_engine.hip — the engine proper of libskw_engine.so: the switchboard, the context and its device workspace, and the batched restatement of
// whisper_full_with_state (greedy, T = 0) on top of skw_kernels; at its end, the test hooks that drive the engine's own phases.
// The rest of the library's host side lives beside it: GGML model loading, the quantised-weight repack and the tokenizer accessors in skw_model.hip; the kernel-level
// test and measurement hooks (skw_debug_* on caller-supplied operands, skw_layout_*) in skw_hooks.hip; the model-free resampler context in skw_dsp.hip.
// What they share is skw_engine_priv.h.
//
// Reference call sites this replaces: /root/reference/plugins/native/whisper/src/lib.rs
//   :377-379 state, :624-646 params + full(), :650-660 segment readout.
#include "skw_engine_priv.h"

// the "auto" audio context of a clip: the positions its audio covers (20 ms each), half a second of margin, whole 32-key blocks — never more than the model's context
extern "C" int skw_audio_ctx_for_samples(int n_samples, int n_audio_ctx) {
    if (n_samples >= WHISPER_SAMPLE_RATE * WHISPER_CHUNK_SIZE) return n_audio_ctx;
    const int pos = ((n_samples > 0 ? n_samples : 0) + 319) / 320;
    return std::min(n_audio_ctx, 32 * ((pos + 25 + 31) / 32));
}
extern "C" void skw_full_default_params(skw_full_params* p) {
    memset(p, 0, sizeof *p); p->lang_id = 0; p->suppress_blank = 1; p->suppress_nst = 0; p->max_initial_ts = 1.0f; p->entropy_thold = 2.4f; p->logprob_thold = -1.0f; p->no_speech_thold = 0.6f;
    p->temperature = 0.0f; p->temperature_inc = 0.2f;
}

// ------------------------------------------------------------------ the switchboard (SkwSw, skw_kernels.h)
struct SwDef { const char* name; int def; const char* what; };
static const SwDef g_sw_defs[SW_COUNT] = {
    {"QUANT_TWIN", 0, "1: a block-quantised file runs as its dequantised f16 twin in both precisions (model load)"},
    {"DEC_WFRAG", 1, "0: the decode GEMMs read their weights as rows, no fragment-order images are built (model load)"},
    {"GEMM16W", 1, "0: the encoder / cross-K-V / prompt-pass GEMMs run k_gemm16 (both operands through LDS) instead of k_gemm16w (weights from fragment-order images)"},
    {"GEMM16W_NGROUPS", 0, "k_gemm16w's feature-split tile walk: 0 automatic, 1 off, 2 / 4 / 8 forced"},
    {"XATTN_FRAG", 1, "0: f16_mfma keeps cross K / V^T as rows and runs the two-phase cross attention (context creation)"},
    {"DECODE_GRAPHS", -1, "0: the decode steps are launched eagerly instead of as captured step graphs (context creation)"},
    {"DECODE_GROUPS", 0, "row groups of the decode step, each a step graph on its own stream: 0 = one group (the default), n forced (context creation)"},
    {"DEC_LN_STATS", 1, "0: f16_mfma launches the decode step's LayerNorms instead of normalising inside the consuming GEMM (context creation)"},
    {"PROMPT_PASS", 1, "0: the prompt is fed one token per step instead of in one multi-row pass (context creation)"},
    {"PROMPT_SMALL_GEMM", 0, "1: a prompt pass of >= 256 rows keeps the small-M decode GEMMs instead of the big-tile kernel (f16_mfma)"},
    {"PROMPT_XATTN_MQ", 1, "0: the f16_mfma prompt pass streams cross K / V^T once per prompt token (single-query kernel) instead of once per 128 (multi-query)"},
    {"DEC_AFRAG", 1, "0: the f16_mfma decode step hands attention / FC1 outputs to the next GEMM as rows instead of fragment-order images"},
    {"DEC_ATTN_FASTV", 1, "0: the f16_mfma decode self-attention uses the exact form's per-channel P.V chain"},
    {"Q8_LDS", 1, "0: ggml-arithmetic GEMMs of quantised files take their operands from global memory (the form tails and odd geometries always use)"},
    {"RESAMPLE_SCAN", 0, "1: the linear resampler's index sequence comes from the single-lane sequential walk only"},
    {"RESAMPLE_NO_HOST_WALK", 0, "1: long resampler calls step the chunk starts on the device instead of on the host"},
};
static int g_sw_val[SW_COUNT];
static std::once_flag g_sw_once;
static std::atomic<unsigned> g_sw_epoch{0};
// the one place this library reads its environment: SKW_<NAME> for every row of the table, once
static void sw_init() {
    for (int i = 0; i < SW_COUNT; ++i) { const std::string k = std::string("SKW_") + g_sw_defs[i].name; const char* e = getenv(k.c_str()); g_sw_val[i] = e ? atoi(e) : g_sw_defs[i].def; }
}
int skw_sw(int id) { std::call_once(g_sw_once, sw_init); return g_sw_val[id]; }
unsigned skw_sw_epoch() { return g_sw_epoch.load(); }
extern "C" int skw_debug_switch_count(void) { return SW_COUNT; }
extern "C" const char* skw_debug_switch_name(int i) { return i >= 0 && i < SW_COUNT ? g_sw_defs[i].name : nullptr; }
extern "C" const char* skw_debug_switch_what(int i) { return i >= 0 && i < SW_COUNT ? g_sw_defs[i].what : nullptr; }
extern "C" int skw_debug_switch_default(int i) { return i >= 0 && i < SW_COUNT ? g_sw_defs[i].def : 0; }
static int sw_find(const char* name) { for (int i = 0; i < SW_COUNT; ++i) if (!strcmp(name, g_sw_defs[i].name)) return i; return -1; }
extern "C" int skw_debug_switch_get(const char* name) { const int i = sw_find(name); return i < 0 ? -1 : skw_sw(i); }
// tests flip a switch in-process (takes effect at the point the table says: the next launch, context creation or model load; cached step graphs are re-captured)
extern "C" int skw_debug_switch_set(const char* name, int value) { const int i = sw_find(name); if (i < 0) return -1; (void)skw_sw(i); g_sw_val[i] = value; g_sw_epoch.fetch_add(1); return 0; }

// a row held at a value for a scope (skw_engine_priv.h): like skw_debug_switch_set, but the epoch stands — the kernel hooks launch no step graph
SwOverride::SwOverride(int id_, int value) : id(id_), was(skw_sw(id_)) { g_sw_val[id] = value; }
SwOverride::~SwOverride() { g_sw_val[id] = was; }
void SwOverride::set(int value) { g_sw_val[id] = value; }

// ------------------------------------------------------------------ context / workspace
// tests (SKW_TEST_ALLOC_POISON=1 in tests/conftest.py): workspace buffers of floating type that the engine does not zero are filled with NaNs when a context is created, so that a
// kernel reading what no kernel wrote shows up as a changed result instead of passing on whatever hipMalloc returned (round 5: a resampler flag was read that way)
static int g_alloc_poison = 0; static std::atomic<long> g_alloc_poisoned{0};
extern "C" void skw_debug_alloc_poison(int on) { g_alloc_poison = on; }
extern "C" long skw_debug_alloc_poisoned(void) { return g_alloc_poisoned.load(); }      // buffers filled so far
void skw_priv::poison_floats(void* p, size_t bytes) { if (g_alloc_poison && p) { (void)hipMemset(p, 0xFF, bytes); g_alloc_poisoned.fetch_add(1); } }
struct SkwKClk;
static SkwKClk* kclk_node(const skw_ctx* c, int g, int l);
static int kclk_reset(skw_ctx* c);
extern "C" const char* skw_ctx_last_error(const skw_ctx* c) { return c->errbuf; }
// The q8 image of cross_kv = q8_0 (1.0625 bytes per element of cross K and V^T, every layer and slot) is allocated when it can first be used: the flag asks for q8_0 AND the
// context runs f16_mfma — a context that stays in the exact precision, which ignores the flag, never pays for it.  Entered in the workspace table by name.
static int kv8_ensure(skw_ctx* c, int precision, int cross_kv) {
    if (cross_kv != SKW_CROSS_KV_Q8_0 || precision != SKW_PRECISION_F16_MFMA || c->crossKV8) return 0;
    const size_t bytes = (size_t)c->m->hp.n_text_layer * c->max_batch * c->kv8_slot(); void* p = nullptr;
    if (hipSetDevice(c->m->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess || !p) {
        snprintf(c->errbuf, 512, "workspace buffer 'crossKV8' could not be allocated (%zu bytes, max_batch %d)", bytes, c->max_batch); return -1;
    }
    c->crossKV8 = (uint8_t*)p; c->allocs.push_back(p);
    c->ws_table.push_back(skw_ctx::WsEntry{"crossKV8", (void**)&c->crossKV8, bytes, false, false});
    return 0;
}
extern "C" int skw_ctx_set_precision(skw_ctx* c, int precision) {
    if (precision != SKW_PRECISION_EXACT && precision != SKW_PRECISION_F16_MFMA) { snprintf(c->errbuf, 512, "unknown precision %d", precision); return -1; }
    if (kv8_ensure(c, precision, c->cross_kv)) return -1;
    c->precision = precision; return 0;
}
extern "C" int skw_ctx_get_precision(const skw_ctx* c) { return c->precision; }
extern "C" int skw_ctx_set_cross_kv(skw_ctx* c, int type) {
    if (type != SKW_CROSS_KV_F16 && type != SKW_CROSS_KV_Q8_0) { snprintf(c->errbuf, 512, "unknown cross_kv type %d", type); return -1; }
    if (kv8_ensure(c, c->precision, type)) return -1;
    c->cross_kv = type; return 0;
}
extern "C" int skw_ctx_get_cross_kv(const skw_ctx* c) { return c->cross_kv; }
extern "C" void* skw_ctx_stream(const skw_ctx* c) { return (void*)c->stream; }
extern "C" void skw_ctx_last_timing(const skw_ctx* c, skw_timing* out) { *out = c->timing; }

extern "C" skw_ctx* skw_ctx_create(skw_model* m, int max_batch, int max_samples, char* err, size_t errlen) {
    if (!m || max_batch < 1) { set_err(err, errlen, "bad arguments"); return nullptr; }
    if (hipSetDevice(m->device) != hipSuccess) { set_err(err, errlen, "hipSetDevice failed"); return nullptr; }
    skw_ctx* c = new skw_ctx(); c->m = m; c->max_batch = max_batch;
    if (max_samples <= 0) max_samples = WHISPER_SAMPLE_RATE * 31;
    c->max_samples = max_samples;
    c->n_len_max = (max_samples + WHISPER_SAMPLE_RATE * 30 + 2 * (WHISPER_N_FFT / 2) - WHISPER_N_FFT) / WHISPER_HOP + 1;
    const skw_hparams& hp = m->hp; const int B = max_batch, nc = hp.n_audio_ctx, T = 2 * nc, d = hp.n_audio_state, dt = hp.n_text_state;
    c->Tpad = (nc + 31) & ~31; c->enc_rows = nc; c->h1_T = T;
    c->kv_frag_on = skw_sw(SW_XATTN_FRAG) != 0;
    bool ok = true;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) ok = false;
    c->cur = c->stream;
    // decode groups: the step kernels are latency-bound chains that leave most CUs idle, so independent row groups run concurrently
    // -1 = default (see skw_full_batch): one row group as a captured step graph in both precisions (dependent chains on two streams do
    // not overlap on this part: tools/probe/probe_stream_overlap.hip)
    c->use_graphs = skw_sw(SW_DECODE_GRAPHS);
    c->ln_stats_on = skw_sw(SW_DEC_LN_STATS) != 0;
    c->prompt_pass_on = skw_sw(SW_PROMPT_PASS) != 0;
    c->rows_cap = std::max(max_batch, std::min(max_batch * (SKW_PROMPT_CAP - 1), 4096));
    c->n_groups = skw_sw(SW_DECODE_GROUPS); if (c->n_groups <= 0) c->n_groups = -1; if (c->n_groups > skw_ctx::MAX_GROUPS) c->n_groups = skw_ctx::MAX_GROUPS;
    for (int g = 0; g < skw_ctx::MAX_GROUPS && g < (c->n_groups < 0 ? 1 : c->n_groups) && ok; ++g) { ok = ok && hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->gev[g], hipEventDisableTiming) == hipSuccess; }
    for (int i = 0; i < 6 && ok; ++i) ok = hipEventCreate(&c->ev[i]) == hipSuccess;
    // The workspace, as a table: one buffer per line — name, the context field it fills, element count, zero-filled or not.  Every entry is
    // allocated by the loop below and verified non-null BY NAME (skw_ctx_create fails with the buffer's name; full_batch_impl re-checks the table
    // before its first launch), so a buffer that is declared but never allocated cannot reach a kernel as a null pointer.
    const size_t R = (size_t)c->rows_cap;
    const size_t enc_rows = (size_t)B * nc;
    const int kmax = 4 * std::max(d, dt);
    c->max_tok = hp.n_text_ctx / 2;
    if (m->quant) c->q8_kmax = kmax;
    auto want = [&](const char* name, auto*& field, size_t count, bool zero) {
        c->ws_table.push_back(skw_ctx::WsEntry{name, (void**)&field, count * sizeof(*field), zero, !std::is_integral<std::remove_pointer_t<std::remove_reference_t<decltype(field)>>>::value});
    };
    // front end
    want("pcm", c->pcm, (size_t)B * max_samples, false);
    want("pcm_off", c->pcm_off, B, false);
    want("n_samples", c->n_samples, B, false);
    want("n_len", c->n_len, B, false);
    want("mel", c->mel, (size_t)B * c->n_len_max * hp.n_mels, false);
    want("clip_max", c->clip_max, B, false);
    want("clip_idx", c->clip_idx, B, false);
    want("seek", c->seek, B, false);
    want("slot_k", c->slot_k, B, true);
    want("row_tok", c->row_tok, B, true);
    want("prompt_buf", c->prompt_buf, (size_t)B * SKW_PROMPT_CAP, true);
    want("im2col", c->im2col, (size_t)B * T * c->m->conv1.k_pad, false);
    want("h1", c->h1, (size_t)B * (T + 2) * d, true);
    // encoder
    want("x", c->x, enc_rows * d, false);
    want("y16", c->y16, enc_rows * d, false);
    want("Qh", c->Qh, (size_t)B * hp.n_audio_head * c->Tpad * 64, true);
    want("Kh", c->Kh, (size_t)B * hp.n_audio_head * c->Tpad * 64, true);
    want("Vt", c->Vt, (size_t)B * hp.n_audio_head * 64 * c->Tpad, true);
    want("hbuf", c->hbuf, enc_rows * 4 * d, false);
    want("enc_out32", c->enc_out32, (size_t)nc * d, false);
    // cross K: zeroed — the fragment-order image's pad keys, rows n_audio_ctx .. Tpad of a slot, are never written
    want("crossK", c->crossK, (size_t)hp.n_text_layer * B * c->Tpad * dt, true);
    // cross V^T per head, keys kperm'ed, pad keys stay zero
    want("crossV", c->crossV, (size_t)hp.n_text_layer * B * hp.n_text_head * 64 * c->Tpad, true);
    // decoder: step scratch rows (sized for the prompt pass), caches, logits, sampler state
    want("dx", c->dx, R * dt, false);
    want("dy16", c->dy16, R * dt, false);
    want("dq16", c->dq16, R * dt, false);
    want("datt16", c->datt16, (R + 16) * dt, false);
    want("dh16", c->dh16, (R + 16) * 4 * dt, false);
    want("pf_st", c->pf_st, R, true);
    want("pf_meta", c->pf_meta, (size_t)3 * B, true);
    want("selfK", c->selfK, (size_t)hp.n_text_layer * B * hp.n_text_ctx * dt, true);
    want("selfV", c->selfV, (size_t)hp.n_text_layer * B * hp.n_text_ctx * dt, true);
    want("logits", c->logits, (size_t)B * hp.n_vocab, false);
    want("st", c->st, B, true);
    want("toks", c->toks, (size_t)B * c->max_tok, true);
    want("probs", c->probs, (size_t)B * skw_probs_row_floats(hp.n_vocab), false);
    want("rng", c->rng, (size_t)B * SKW_RNG_WORDS, true);
    want("static_mask", c->static_mask, skw_static_mask_bytes(hp.n_vocab), true);
    want("static_mask_pair", c->static_mask_pair, 2 * skw_static_mask_bytes(hp.n_vocab), true);
    want("row_rules", c->row_rules, B, true);
    want("row_cons", c->row_cons, B, true);
    want("row_gram", c->row_gram, B, true);
    if (m->quant) {      // ggml q8 arithmetic (quantised files, exact precision): unrounded f32 activations and their q8 blocks
        want("y32", c->y32, enc_rows * d, false);
        want("h32", c->h32, enc_rows * 4 * d, false);
        want("encq32", c->encq32, enc_rows * d, false);
        want("dy32", c->dy32, R * dt, false);
        want("datt32", c->datt32, R * dt, false);
        want("dh32", c->dh32, R * 4 * dt, false);
        want("q8_a", c->q8_a, enc_rows * kmax, false);
        want("q8_d", c->q8_d, enc_rows * (kmax / 32), false);
        want("q8_s", c->q8_s, enc_rows * (kmax / 32), false);
    }
    const char* ws_failed = nullptr;
    size_t ws_failed_bytes = 0;
    for (const skw_ctx::WsEntry& e : c->ws_table) {
        if (!ok) break;
        void* p = nullptr;
        if (hipMalloc(&p, e.bytes) != hipSuccess || !p) { ok = false; ws_failed = e.name; ws_failed_bytes = e.bytes; break; }
        c->allocs.push_back(p);
        if (e.zero) (void)hipMemset(p, 0, e.bytes);
        else if (e.is_float) poison_floats(p, e.bytes);       // tests: every f16 / f32 / f64 buffer the engine does not zero starts as NaNs (skw_debug_alloc_poison)
        *e.slot = p;
    }
    if (ok) ws_failed = ws_first_null(c);
    if (ws_failed) {
        set_err(err, errlen, "workspace buffer '%s' could not be allocated (%zu bytes, max_batch %d)", ws_failed, ws_failed_bytes, max_batch);
        skw_ctx_free(c);
        return nullptr;
    }
    ok = ok && hipHostMalloc((void**)&c->h_st, sizeof(SkwSeqState) * B) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->h_toks, sizeof(SkwTokenOut) * B * c->max_tok) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&c->h_row_live, sizeof(int) * B, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer((void**)&c->d_row_live, c->h_row_live, 0) == hipSuccess;
    if (!ok) { set_err(err, errlen, "stream, event or pinned host allocation failed (max_batch %d)", max_batch); skw_ctx_free(c); return nullptr; }
    hipDeviceSynchronize();
    return c;
}
static void prof_free(skw_ctx* c);
extern "C" void skw_ctx_free(skw_ctx* c) {
    if (!c) return; hipSetDevice(c->m->device);
    prof_free(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto& sg : c->step_graphs) hipGraphExecDestroy(sg.exec);
    c->step_graphs.clear();
    for (int g = 0; g < skw_ctx::MAX_GROUPS; ++g) { if (c->gstream[g]) { hipStreamSynchronize(c->gstream[g]); hipStreamDestroy(c->gstream[g]); } if (c->gev[g]) hipEventDestroy(c->gev[g]); }
    for (void* p : c->allocs) hipFree(p);
    hipFree(c->stageK); hipFree(c->stageV); hipFree(c->slot_map); hipFree(c->forced_dev); hipFree(c->trace_dev); hipFree(c->kclk);
    for (auto& gi : c->gr_cache) hipFree(gi.d_next);      // (d_accept is the tail of the same allocation)
    hipFree(c->gr_voc_off);
    hipFree(c->al_P); hipFree(c->al_acc); hipFree(c->al_x); hipFree(c->al_seqs); hipFree(c->al_times);
    if (c->h_st) hipHostFree(c->h_st); if (c->h_toks) hipHostFree(c->h_toks); if (c->h_row_live) hipHostFree(c->h_row_live);
    for (int i = 0; i < 6; ++i) if (c->ev[i]) hipEventDestroy(c->ev[i]);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

// the debug taps the phases below fill (tap() and the entry points that read them: with the test hooks at the end of this file)
enum TapLayout { TAP_F32, TAP_F16_KPERM, TAP_HEADS, TAP_VT, TAP_F16_PLAIN };
static std::map<std::string, std::vector<float>> g_taps; static bool g_taps_on = false;
static void tap(skw_ctx* c, const char* name, const void* dev, int rows, int cols, TapLayout lay);

// ------------------------------------------------------------------ per-kernel-class profiling (HIP events on the engine stream)
enum ProfClass { PC_GEMM = 0, PC_GEMM_SMALL, PC_ATTN_ENC, PC_LAYERNORM, PC_MEL, PC_DEC_ATTN, PC_DEC_SAMPLE, PC_OTHER, PC_DEC_XATTN, PC_DEC_CONSTRAIN, PC_ALIGN_QK,
                 PC_ALIGN_REDUCE, PC_ALIGN_DTW, PC_DEC_GRAMMAR, PC_COUNT };
static const char* const g_prof_names[PC_COUNT] = {"k_gemm", "k_gemm_smallm", "k_attn_encoder", "k_layernorm", "k_mel", "k_dec_self_attn", "k_dec_sample", "other", "k_dec_cross_attn",
                                                 "k_dec_constrain", "k_align_qk", "k_align_reduce", "k_align_dtw", "k_dec_grammar"};
struct ProfRec { int cls; double flops, bytes; hipEvent_t a, b; };
struct ProfState { bool on = false; std::vector<ProfRec> recs;
std::vector<hipEvent_t> pool; size_t next = 0; double ms[PC_COUNT] = {}, flops[PC_COUNT] = {}, bytes[PC_COUNT] = {}; long count[PC_COUNT] = {}; };
static void prof_free(skw_ctx* c) { if (!c->prof) return; for (hipEvent_t e : c->prof->pool) hipEventDestroy(e); delete c->prof; c->prof = nullptr; }
struct ProfScope {
    ProfState* ps; skw_ctx* c; size_t idx; bool ext;      // ext: the launch stamps the two events itself (hipExtLaunchKernelGGL: kernel begin / end, what rocprofv3 calls the duration)
    ProfScope(skw_ctx* c_, int cls, double flops, double bytes, bool ext_ = false);
    ~ProfScope();
    hipEvent_t ev_a() const; hipEvent_t ev_b() const;
    void cancel() { if (ps) { ps->recs[idx].flops = 0.0; ps->recs[idx].bytes = 0.0; ps->recs[idx].cls = PC_OTHER; } }      // the launch did not happen: book nothing for it
};

// ------------------------------------------------------------------ GEMM helpers
ProfScope::ProfScope(skw_ctx* c_, int cls, double flops, double bytes, bool ext_) : ps(nullptr), c(c_), idx(0), ext(ext_) {
    if (!c_->prof || !c_->prof->on) return;
    ps = c_->prof;
    auto get = [&]() { if (ps->next == ps->pool.size()) { hipEvent_t e; hipEventCreate(&e); ps->pool.push_back(e); } return ps->pool[ps->next++]; };
    ProfRec r; r.cls = cls; r.flops = flops; r.bytes = bytes; r.a = get(); r.b = get(); idx = ps->recs.size(); ps->recs.push_back(r);
    if (!ext) hipEventRecord(r.a, c->cur);
}
ProfScope::~ProfScope() { if (ps && !ext) hipEventRecord(ps->recs[idx].b, c->cur); }
hipEvent_t ProfScope::ev_a() const { return (ps && ext) ? ps->recs[idx].a : nullptr; }
hipEvent_t ProfScope::ev_b() const { return (ps && ext) ? ps->recs[idx].b : nullptr; }
static void prof_collect(skw_ctx* c) {
    if (!c->prof || !c->prof->on) return; ProfState& ps = *c->prof;
    hipStreamSynchronize(c->stream);
    for (auto& r : ps.recs) { float ms = 0; if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
    ps.ms[r.cls] += ms; ps.flops[r.cls] += r.flops; ps.bytes[r.cls] += r.bytes; ps.count[r.cls]++; }
    ps.recs.clear(); ps.next = 0;
}
extern "C" void skw_ctx_profile(skw_ctx* c, int on) { if (!c->prof) c->prof = new ProfState();
ProfState& ps = *c->prof; ps.on = on != 0; for (int i = 0; i < PC_COUNT; ++i) { ps.ms[i] = ps.flops[i] = ps.bytes[i] = 0;
ps.count[i] = 0; } ps.recs.clear(); ps.next = 0; }
extern "C" int skw_ctx_profile_get(skw_ctx* c, int cls, char* name, size_t name_len, long* count, double* ms, double* flops, double* bytes) {
    if (cls < 0 || cls >= PC_COUNT || !c->prof) return -1; ProfState& ps = *c->prof;
    if (name) snprintf(name, name_len, "%s", g_prof_names[cls]); *count = ps.count[cls]; *ms = ps.ms[cls]; *flops = ps.flops[cls]; *bytes = ps.bytes[cls]; return 0;
}
// algorithmic work of one GEMM launch: 2*M*N*K flops; bytes = operands read once + result written once
static void gemm_work(const SkwGemmArgs& a, int k_logical, double* fl, double* by) { *fl = 2.0 * a.M * a.N * k_logical;
*by = 2.0 * ((double)a.M * k_logical + (double)a.N * k_logical) + 2.0 * a.M * a.N; }
static void GEMM(skw_ctx* c, const SkwGemmArgs& a, int k_logical) {
    double fl, by; gemm_work(a, k_logical, &fl, &by); ProfScope p(c, PC_GEMM, fl, by);
    if (c->precision == SKW_PRECISION_F16_MFMA && (a.K & 63) == 0) skw_gemm16(a, c->cur);   // K step of the f16 kernel is 64; every Whisper geometry satisfies it
    else skw_gemm(a, c->cur);
}
static void GEMM_S(skw_ctx* c, const SkwGemmArgs& a, int k_logical) {
    double fl, by; gemm_work(a, k_logical, &fl, &by); ProfScope p(c, PC_GEMM_SMALL, fl, by);
    // (a VALU row-parallel variant — lane = batch row, v_fma_mix chains — was measured slower: a dependent v_fma costs 8-10 cycles
    //  on gfx950, no better than the MFMA's 40 cycles per 4 k)
    if (c->precision == SKW_PRECISION_F16_MFMA && skw_gemm16_small(a, c->cur)) return;
    skw_gemm_smallm(a, c->cur);
}

// decode GEMM fed by a LayerNorm of x, as two launches (the exact precision; f16_mfma where the normalising GEMM does not cover the geometry)
static void GEMM_S(skw_ctx* c, const SkwGemmArgs& a, int k_logical);
static void GEMM_LN(skw_ctx* c, SkwGemmArgs a, const float* x, const DevLN& ln, half_t* y16, hipStream_t s, bool normalised = false) {
    if (normalised) { GEMM_S(c, a, a.K); return; }                     // y16 already holds LayerNorm(x): the embedding kernel did it (layer 0)
    { ProfScope p_(c, PC_LAYERNORM, 0, 6.0 * a.M * a.K); skw_layernorm(x, a.M, a.K, ln.w, ln.b, y16, nullptr, s); }
    GEMM_S(c, a, a.K);
}

// ---- ggml's arithmetic for quantised files (skw_kernels_q8.hip): quantise the f32 rows once, then any number of products with them
static bool use_q8(const skw_ctx* c) { return c->m->quant != 0 && c->precision == SKW_PRECISION_EXACT; }
static void Q8_ROWS(skw_ctx* c, const float* act32, long lda, int M, int K, int r0) {
    ProfScope p(c, PC_LAYERNORM, 0, 5.0 * M * K);
    skw_q8_quantize(act32, lda, M, K, c->q8_a + (size_t)r0 * c->q8_kmax, c->q8_d + (size_t)r0 * (c->q8_kmax / 32), c->q8_s + (size_t)r0 * (c->q8_kmax / 32), c->cur);
}
// LayerNorm -> f32 rows -> q8 blocks.  (A LayerNorm kernel that quantises its own rows was measured slower than the two launches, twice: one wave
// then owns a whole row's 24 blocks — 266 - 298 vs 243 ms of decode per batch — where the quantiser has a thread per block.)
static void Q8_LN(skw_ctx* c, const float* x, int M, int d, const DevLN& ln, int r0, float* y32) {
    { ProfScope p_(c, PC_LAYERNORM, 0, 6.0 * M * d); skw_layernorm(x, M, d, ln.w, ln.b, nullptr, y32, c->cur); }
    Q8_ROWS(c, y32, d, M, d, r0);
}
static void Q8_GEMM(skw_ctx* c, SkwGemmArgs a, const DevLin& L, int r0, bool decoder = false) {
    a.K = L.n_in; a.N = L.n_out; a.bias = L.b;
    SkwQ8Args qa{c->q8_a + (size_t)r0 * c->q8_kmax, c->q8_d + (size_t)r0 * (c->q8_kmax / 32), c->q8_s + (size_t)r0 * (c->q8_kmax / 32), L.qw, L.dwT, L.mwT, L.n_pad, L.qform,
                 decoder && !(L.n_in & 127) ? 1 : 0};
    ProfScope p(c, a.M <= 64 ? PC_GEMM_SMALL : PC_GEMM, 2.0 * a.M * a.N * a.K, 1.0 * a.M * a.K + 1.0 * a.N * a.K + 4.0 * a.M * a.N);
    skw_gemm_q8(a, qa, c->cur);
}
static SkwGemmArgs q8_args(int M, void* C, long ldc, int epi) { SkwGemmArgs a{}; a.M = M; a.C = C; a.ldc = ldc; a.epi = epi; a.scale = 1.0f; return a; }

static SkwGemmArgs gemm_args(const half_t* A, long lda, const DevLin& L, int M, void* C, long ldc, int epi) {
    SkwGemmArgs a{}; a.A = A; a.lda = lda; a.W = L.w; a.Wf = L.w_frag; a.ldw = L.k_pad; a.M = M; a.N = L.n_out; a.K = L.k_pad; a.C = C;
    a.ldc = ldc; a.bias = L.b; a.epi = epi; a.scale = 1.0f; return a;
}

// front end for `n` clips already described in c->pcm_off / n_samples / n_len (device): mel + normalisation
static void run_mel(skw_ctx* c, int n) {
    skw_model* m = c->m; SkwMelTables t{m->hann, m->sin_t, m->cos_t, m->filters, m->hp.n_mels, m->n_fft_bins, m->mel_grp_lo, m->mel_grp_hi};
    ProfScope p_(c, PC_MEL, 0, 0);
    skw_mel_frames(c->pcm, c->pcm_off, c->n_samples, c->n_len, n, c->n_len_max, t, c->mel, c->stream);
    skw_mel_normalize(c->mel, c->n_len, n, c->n_len_max, m->hp.n_mels, c->clip_max, c->stream);
}
// conv stem for Bw window slots (clip_idx/seek on device) -> c->x [Bw*nc][d]
// row0: the first window slot to compute (slots before it keep what they hold: temperature retries, see skw_full_batch); the stem's
// buffers are scratch, so the Bw - row0 computed windows sit at their start
// Per-clip audio context: the rows a slot's activations take in the encoder pass.  GEMMs are row-wise, so a pass whose longest window has kmax positions runs over Bw x enc_rows
// rows instead of Bw x n_audio_ctx: kmax rounded to whole 32-key blocks and to at least 256 — the f16 GEMMs' per-clip epilogues step from one slot to the next at most once
// per 256-row tile.  A slot's rows past its own K are don't-care: computed from zero mel frames, read by nothing.
static int enc_rows_for(const skw_ctx* c, int kmax) {
    const int nc = c->m->hp.n_audio_ctx;
    return kmax >= nc ? nc : std::min(nc, std::max(256, (kmax + 31) & ~31));
}
// K of every slot of the pass about to run -> device; returns the rows per slot for run_conv / run_encoder (windows row0 .. are computed)
static int set_slot_k(skw_ctx* c, const int* ks, int Bw, int row0, hipStream_t s) {
    const int nc = c->m->hp.n_audio_ctx; int kmax = 1; bool var = false;
    for (int j = 0; j < Bw; ++j) { var = var || ks[j] < nc; if (j >= row0) kmax = std::max(kmax, ks[j]); }
    c->var_k = var;
    (void)hipMemcpyAsync(c->slot_k, ks, sizeof(int) * Bw, hipMemcpyHostToDevice, s);      // (callers keep ks alive until the stream is synchronised)
    return enc_rows_for(c, kmax);
}
static void run_conv(skw_ctx* c, int Bw_all, int row0 = 0, int rows = 0) {
    skw_model* m = c->m; const int nc = rows > 0 ? rows : m->hp.n_audio_ctx, T = 2 * nc, d = m->hp.n_audio_state; const int Bw = Bw_all - row0;
    if (T != c->h1_T) {      // h1 is [slot][T + 2 rows]: the zero row in front of every slot's block moves with T (conv2's first output reads it; the row behind the block is read by nothing)
        (void)hipMemset2DAsync(c->h1, (size_t)(T + 2) * d * sizeof(half_t), 0, (size_t)d * sizeof(half_t), c->max_batch, c->stream);
        c->h1_T = T;
    }
    c->enc_rows = nc;
    skw_mel_im2col(c->mel, c->clip_idx + row0, c->seek + row0, c->n_len, Bw, c->n_len_max, m->hp.n_mels, T, m->conv1.k_pad, c->im2col, c->stream, c->var_k ? c->slot_k + row0 : nullptr);
    SkwGemmArgs a = gemm_args(c->im2col, m->conv1.k_pad, m->conv1, Bw * T, c->h1, d, EPI_GELU_F16_KPERM_ROWPAD); a.gelu_tab = m->gelu_tab; a.n_ctx = T;
    GEMM(c, a, m->conv1.n_in);
    SkwGemmArgs b = gemm_args(c->h1, 2L * d, m->conv2, Bw * nc, c->x, d, EPI_CONV2); b.a_rows_per_batch = nc; b.a_batch_stride = (long)(T + 2) * d;
    b.gelu_tab = m->gelu_tab; b.pe = m->e_pe; b.n_ctx = nc;
    GEMM(c, b, m->conv2.n_in);
}
// cross_kv = q8_0: the q8 image of window slots slot0 .. slot0 + n - 1, every layer, from their f16 fragment-order images (one launch per layer; the slots' key counts are
// slot_k's, in device memory).  Called behind the cross-K/V GEMMs of an encoder pass, and for the slots a temperature retry moved.  Without the flag: marks the image stale.
static void kv8_refresh(skw_ctx* c, int slot0, int n, bool keep_fresh = false) {
    if (!c->kv8()) { c->kv8_fresh = false; return; }
    const skw_hparams& hp = c->m->hp; const int H = hp.n_text_head;
    ProfScope p_(c, PC_OTHER, 0, (double)hp.n_text_layer * n * (4.0 * hp.n_audio_ctx * hp.n_text_state + (double)c->kv8_slot()));
    for (int l = 0; l < hp.n_text_layer; ++l)
        skw_kv8_quantize(c->crossK + (size_t)l * c->max_batch * c->kclip(), c->crossV + (size_t)l * c->max_batch * H * 64 * c->Tpad, c->crossKV8 + (size_t)l * c->max_batch * c->kv8_slot(),
                         slot0, n, H, hp.n_audio_ctx, c->Tpad, c->var_k ? c->slot_k : nullptr, c->stream);
    if (!keep_fresh) c->kv8_fresh = true;
}
// encoder blocks + ln_post (+ cross K/V) over Bw windows; input c->x
// rows: rows per slot of the activations (enc_rows_for; 0: n_audio_ctx).  Strides of Qh / Kh / Vt and of cross K / V stay those of the full context
static void run_encoder(skw_ctx* c, int Bw_all, bool want_f32_out, bool cross, int row0 = 0, int rows = 0) {
    skw_model* m = c->m; const skw_hparams& hp = m->hp; const int nc = rows > 0 ? rows : hp.n_audio_ctx, d = hp.n_audio_state, H = hp.n_audio_head; const int Bw = Bw_all - row0, M = Bw * nc;
    const int* sk_dev = c->var_k ? c->slot_k + row0 : nullptr;      // per-slot keys / queries of the attention (null: every slot is full length, today's launches)
    c->enc_rows = nc;
    // cross K as rows (exact precision, q8, SKW_XATTN_FRAG=0): a slot's rows are n_audio_ctx apart in the buffer whatever `rows` is, so a shortened pass writes slot by slot
    const bool ck_per_slot = nc != hp.n_audio_ctx && Bw > 1 && !c->kv_frag();
    const size_t xk0 = (size_t)row0 * c->kclip(), xv0 = (size_t)row0 * hp.n_text_head * 64 * c->Tpad;      // cross K / V of the computed windows land in slots row0 ..
    if (use_q8(c)) {
        // Quantised file, exact precision: every weight product is ggml's (rows -> q8 blocks, integer block dots), so what feeds a
        // projection stays f32 and unrounded — LayerNorm, attention and GELU write f32 here — and only the attention operands
        // (Q, K, V^T: ggml casts those to f16 itself) are f16 as before.  The conv stem's kernels are 3-D tensors: never quantised.
        for (int l = 0; l < hp.n_audio_layer; ++l) {
            const EncLayer& L = m->enc[l];
            Q8_LN(c, c->x, M, d, L.attn_ln, 0, c->y32);
            { SkwGemmArgs a = q8_args(M, c->Qh, 0, EPI_HEADS_F16); a.n_ctx = nc; a.H = H; a.Tpad = c->Tpad; Q8_GEMM(c, a, L.q, 0); }
            { SkwGemmArgs a = q8_args(M, c->Kh, 0, EPI_HEADS_F16); a.n_ctx = nc; a.H = H; a.Tpad = c->Tpad; Q8_GEMM(c, a, L.k, 0); }
            { SkwGemmArgs a = q8_args(M, c->Vt, 0, EPI_VT_F16); a.n_ctx = nc; a.H = H; a.Tpad = c->Tpad; Q8_GEMM(c, a, L.v, 0); }
            { ProfScope p_(c, PC_ATTN_ENC, 4.0 * Bw * H * (double)nc * nc * 64, 2.0 * 4 * M * d);
              skw_attn_encoder(c->Qh, c->Kh, c->Vt, (half_t*)c->y32, d, Bw, H, nc, c->Tpad, c->stream, nullptr, nullptr, 1, sk_dev, nc); }
            Q8_ROWS(c, c->y32, d, M, d, 0);
            { SkwGemmArgs a = q8_args(M, c->x, d, EPI_F32); a.res = c->x; a.ldres = d; Q8_GEMM(c, a, L.o, 0); }
            Q8_LN(c, c->x, M, d, L.mlp_ln, 0, c->y32);
            { SkwGemmArgs a = q8_args(M, c->h32, 4L * d, EPI_GELU_F32); a.gelu_tab = m->gelu_tab; Q8_GEMM(c, a, L.fc1, 0); }
            Q8_ROWS(c, c->h32, 4L * d, M, 4 * d, 0);
            { SkwGemmArgs a = q8_args(M, c->x, d, EPI_F32); a.res = c->x; a.ldres = d; Q8_GEMM(c, a, L.fc2, 0); }
        }
        skw_layernorm(c->x, M, d, m->ln_post.w, m->ln_post.b, nullptr, c->encq32, c->stream);
        if (want_f32_out) hipMemcpyAsync(c->enc_out32, c->encq32, sizeof(float) * (size_t)nc * d, hipMemcpyDeviceToDevice, c->stream);
        if (cross) {
            const int dt = hp.n_text_state; const float Kscale = (float)pow((double)((float)dt / hp.n_text_head), -0.25);
            Q8_ROWS(c, c->encq32, d, M, d, 0);
            for (int l = 0; l < hp.n_text_layer; ++l) {
                const DecLayer& L = m->dec[l];
                half_t* ck = c->crossK + (size_t)l * c->max_batch * c->kclip() + xk0; half_t* cv = c->crossV + (size_t)l * c->max_batch * hp.n_text_head * 64 * c->Tpad + xv0;
                if (!ck_per_slot) { SkwGemmArgs a = q8_args(M, ck, dt, EPI_F16_PLAIN); a.scale = Kscale; a.has_scale = 1; Q8_GEMM(c, a, L.ck, 0); }
                { SkwGemmArgs a = q8_args(M, cv, 0, EPI_VT_F16); a.n_ctx = nc; a.H = hp.n_text_head; a.Tpad = c->Tpad; Q8_GEMM(c, a, L.cv, 0); }
            }
            // a shortened pass: cross K slot by slot.  The q8 blocks' scales are stored [block][row of the launch], so a slot's rows are quantised again as a launch of their own
            // (row-wise: the same blocks)
            for (int j = 0; ck_per_slot && j < Bw; ++j) {
                Q8_ROWS(c, c->encq32 + (size_t)j * nc * d, d, nc, d, 0);
                for (int l = 0; l < hp.n_text_layer; ++l) {
                    half_t* ck = c->crossK + (size_t)l * c->max_batch * c->kclip() + xk0 + (size_t)j * c->kclip();
                    SkwGemmArgs a = q8_args(nc, ck, dt, EPI_F16_PLAIN); a.scale = Kscale; a.has_scale = 1; Q8_GEMM(c, a, m->dec[l].ck, 0);
                }
            }
        }
        c->last_enc_B = Bw_all;
        return;
    }
    for (int l = 0; l < hp.n_audio_layer; ++l) {
        const EncLayer& L = m->enc[l];
        { ProfScope p_(c, PC_LAYERNORM, 0, 6.0 * M * d); skw_layernorm(c->x, M, d, L.attn_ln.w, L.attn_ln.b, c->y16, nullptr, c->stream); }
        if (l == 0) tap(c, "l0.ln1", c->y16, nc, d, TAP_F16_KPERM);
        { SkwGemmArgs a = gemm_args(c->y16, d, L.q, M, c->Qh, 0, EPI_HEADS_F16); a.n_ctx = nc; a.H = H; a.Tpad = c->Tpad; GEMM(c, a, d); }
        { SkwGemmArgs a = gemm_args(c->y16, d, L.k, M, c->Kh, 0, EPI_HEADS_F16); a.n_ctx = nc; a.H = H; a.Tpad = c->Tpad; GEMM(c, a, d); }
        { // V^T via the swapped product: rows = features (weights as the A operand), columns = tokens
            SkwGemmArgs a{}; a.A = L.v.w; a.lda = L.v.k_pad; a.W = c->y16; a.ldw = d; a.M = L.v.n_out; a.N = M; a.K = L.v.k_pad; a.C = c->Vt;
            a.bias = L.v.b; a.epi = EPI_VT_F16; a.n_ctx = nc; a.H = H; a.Tpad = c->Tpad; a.scale = 1.0f;
            // the f16 kernel takes V^T in the natural orientation (tokens x features)
            if (c->precision == SKW_PRECISION_F16_MFMA) { a.A = c->y16; a.lda = d; a.W = L.v.w; a.Wf = L.v.w_frag; a.ldw = L.v.k_pad; a.M = M; a.N = L.v.n_out; }
            GEMM(c, a, d);
        }
        if (l == 0) { tap(c, "l0.q", c->Qh, nc, d, TAP_HEADS); tap(c, "l0.k", c->Kh, nc, d, TAP_HEADS); tap(c, "l0.v", c->Vt, nc, d, TAP_VT); }
        float* dbg = nullptr;
        if (l == 0 && g_taps_on) { hipMalloc((void**)&dbg, sizeof(float) * ((size_t)nc * d + 2 * (size_t)H * nc + 64)); hipMemset(dbg, 0, sizeof(float) * ((size_t)nc * d + 2 * (size_t)H * nc)); }
        float* dbg2 = nullptr;
        if (dbg) { hipMalloc((void**)&dbg2, sizeof(float) * 64 * c->Tpad); hipMemset(dbg2, 0, sizeof(float) * 64 * c->Tpad); }
        { ProfScope p_(c, PC_ATTN_ENC, 4.0 * Bw * H * (double)nc * nc * 64, 2.0 * 4 * M * d);
          if (c->precision == SKW_PRECISION_F16_MFMA && !dbg) skw_attn_encoder16(c->Qh, c->Kh, c->Vt, c->y16, d, Bw, H, nc, c->Tpad, c->stream, sk_dev, nc);
          else skw_attn_encoder(c->Qh, c->Kh, c->Vt, c->y16, d, Bw, H, nc, c->Tpad, c->stream, dbg, dbg2, 0, sk_dev, nc); }
        if (dbg2) { tap(c, "l0.SP", dbg2, 64, c->Tpad, TAP_F32); hipFree(dbg2); }
        if (dbg) { tap(c, "l0.att32", dbg, nc, d, TAP_F32); tap(c, "l0.rmax", dbg + (size_t)nc * d, H, nc, TAP_F32);
        tap(c, "l0.rinv", dbg + (size_t)nc * d + (size_t)H * nc, H, nc, TAP_F32); hipFree(dbg); }
        if (l == 0) tap(c, "l0.att", c->y16, nc, d, TAP_F16_KPERM);
        { SkwGemmArgs a = gemm_args(c->y16, d, L.o, M, c->x, d, EPI_F32); a.res = c->x; a.ldres = d; GEMM(c, a, d); }
        if (l == 0) tap(c, "l0.x1", c->x, nc, d, TAP_F32);
        { ProfScope p_(c, PC_LAYERNORM, 0, 6.0 * M * d); skw_layernorm(c->x, M, d, L.mlp_ln.w, L.mlp_ln.b, c->y16, nullptr, c->stream); }
        if (l == 0) tap(c, "l0.ln2", c->y16, nc, d, TAP_F16_KPERM);
        { SkwGemmArgs a = gemm_args(c->y16, d, L.fc1, M, c->hbuf, 4L * d, EPI_GELU_F16_KPERM); a.gelu_tab = m->gelu_tab; GEMM(c, a, d); }
        if (l == 0) tap(c, "l0.h", c->hbuf, nc, 4 * d, TAP_F16_KPERM);
        { SkwGemmArgs a = gemm_args(c->hbuf, 4L * d, L.fc2, M, c->x, d, EPI_F32); a.res = c->x; a.ldres = d; GEMM(c, a, 4 * d); }
        if (l == 0) tap(c, "l0.x2", c->x, nc, d, TAP_F32);
    }
    skw_layernorm(c->x, M, d, m->ln_post.w, m->ln_post.b, c->y16, want_f32_out ? c->enc_out32 : nullptr, c->stream);
    if (cross) {
        const int dt = hp.n_text_state; const float Kscale = (float)pow((double)((float)dt / hp.n_text_head), -0.25);
        for (int l = 0; l < hp.n_text_layer; ++l) {
            const DecLayer& L = m->dec[l];
            half_t* ck = c->crossK + (size_t)l * c->max_batch * c->kclip() + xk0; half_t* cv = c->crossV + (size_t)l * c->max_batch * hp.n_text_head * 64 * c->Tpad + xv0;
            for (int j = 0; j < (ck_per_slot ? Bw : 1); ++j) {
                SkwGemmArgs a = gemm_args(c->y16 + (size_t)j * nc * d, d, L.ck, ck_per_slot ? nc : M, ck + (size_t)j * c->kclip(), dt, EPI_F16_PLAIN); a.scale = Kscale; a.has_scale = 1;
                if (c->kv_frag()) { a.frag = 1; a.n_ctx = nc; a.H = hp.n_text_head; a.Tpad = c->Tpad; }
                GEMM(c, a, d);
            }
            { // cross V^T through the operand-swapped product (rows = features, columns = tokens), as for the encoder's V
                SkwGemmArgs a{}; a.A = L.cv.w; a.lda = L.cv.k_pad; a.W = c->y16; a.ldw = d; a.M = L.cv.n_out; a.N = M; a.K = L.cv.k_pad; a.C = cv;
                a.bias = L.cv.b; a.epi = EPI_VT_F16; a.n_ctx = nc; a.H = hp.n_text_head; a.Tpad = c->Tpad; a.scale = 1.0f;
                if (c->precision == SKW_PRECISION_F16_MFMA) { a.A = c->y16; a.lda = d; a.W = L.cv.w; a.ldw = L.cv.k_pad; a.M = M; a.N = L.cv.n_out; a.Wf = L.cv.w_frag; a.frag = c->kv_frag(); }
                GEMM(c, a, d);
            }
        }
        kv8_refresh(c, row0, Bw);
    }
    c->last_enc_B = Bw_all;
}

// one decoder step for Bw sequences: token/pos taken from the device state; logits computed when want_logits
// slot_k: the rows' cross-attention key counts (row i decodes window slot i)
__global__ void k_set_tokens(SkwSeqState* st, int tok, int pos, const int* slot_k) {
    st[blockIdx.x].cur_token = tok; st[blockIdx.x].cur_pos = pos; st[blockIdx.x].active = 1; st[blockIdx.x].n_keys = slot_k[blockIdx.x];
}
// whisper_lang_auto_detect_with_state: the language whose token has the largest logit after the [sot] step (lowest id on a tie)
__global__ void k_lang_argmax(const float* logits, int n_vocab, int tok_sot, int n_lang, int* out) {
    const float* lg = logits + (long)blockIdx.x * n_vocab; float bv = -INFINITY; int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n_lang; i += 64) { float v = lg[tok_sot + 1 + i]; if (v > bv) { bv = v; bi = i; } }
    for (int o = 32; o > 0; o >>= 1) { float ov = __shfl_xor(bv, o, 64); int oi = __shfl_xor(bi, o, 64); if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; } }
    if (threadIdx.x == 0) out[blockIdx.x] = bi;
}
// The alignment pass's hook (align_window): right after decoder layer l's cross-query GEMM, when l holds alignment heads — dq16 then holds exactly the f16 queries the cross
// attention is about to read, and ck is the layer's cross K as this context stores it (rows, or the fragment-order image).  Step 1 for the layer's heads into the capture, then
// steps 2-5 into the chunk's matrices: only one layer's capture is ever live.  Launches nothing outside an alignment pass.
static void align_hook(skw_ctx* c, int l, const half_t* dq16, const half_t* ck, hipStream_t s) {
    if (!c->al_on || !c->al_mask[l]) return;
    const skw_hparams& hp = c->m->hp; const int nh = skw_align_popcount(c->al_mask[l]);
    // taps, one set per SEQUENCE of the call (s = the sequence's number in the order the call aligns them; "align_seq_s<s>" says which clip and window it is): the sequence's
    // alignment rows of this layer's queries and its slot's cross K, both as f16 bit patterns in natural order — what the evaluator needs to restate the pass
    if (g_taps_on) {
        const int nc = hp.n_audio_ctx, dt = hp.n_text_state; char name[40];
        std::vector<uint16_t> h; hipStreamSynchronize(s);
        for (int i = 0; i < c->al_nseq; ++i) {
            const SkwAlignSeq& a = c->al_h_seqs[i]; const int sn = c->al_tap_base + i;
            snprintf(name, sizeof name, "align_dq16_l%d_s%d", l, sn); tap(c, name, dq16 + (size_t)a.qrow0 * dt, a.n, dt, TAP_F16_PLAIN);
            h.resize(c->kclip()); hipMemcpy(h.data(), ck + (size_t)a.slot * c->kclip(), h.size() * 2, hipMemcpyDeviceToHost);
            snprintf(name, sizeof name, "align_ck_l%d_s%d", l, sn); std::vector<float>& o = g_taps[name]; o.assign((size_t)nc * dt, 0.f);
            for (int k = 0; k < nc; ++k) for (int f = 0; f < dt; ++f)
                o[(size_t)k * dt + f] = (float)h[c->kv_frag() ? (size_t)skw_kfrag_off(0, hp.n_text_head, c->Tpad, k, f & ~7) + (f & 7) : (size_t)k * dt + f];
        }
    }
    { ProfScope p_(c, PC_ALIGN_QK, 2.0 * c->al_rows_now * nh * 64.0 * hp.n_audio_ctx, 0);
      skw_align_qk(dq16, hp.n_text_state, ck, c->al_seqs, c->al_nseq, c->al_rows_now, c->al_mask[l], hp.n_text_head, hp.n_audio_ctx, c->Tpad, c->kv_frag(), c->al_P, c->al_rows_now,
                   hp.n_audio_ctx, s); }
    if (g_taps_on) {      // the capture of this layer, per sequence: [head][row][key]
        const int nc = hp.n_audio_ctx; char name[40]; hipStreamSynchronize(s);
        for (int i = 0; i < c->al_nseq; ++i) {
            const SkwAlignSeq& a = c->al_h_seqs[i];
            snprintf(name, sizeof name, "align_P_l%d_s%d", l, c->al_tap_base + i); std::vector<float>& o = g_taps[name]; o.assign((size_t)nh * a.n * nc, 0.f);
            for (int hl = 0; hl < nh; ++hl) hipMemcpy(o.data() + (size_t)hl * a.n * nc, c->al_P + ((size_t)hl * c->al_rows_now + a.prow0) * nc, sizeof(float) * a.n * nc, hipMemcpyDeviceToHost);
        }
    }
    { ProfScope p_(c, PC_ALIGN_REDUCE, 0, 0);
      skw_align_reduce(c->al_P, c->al_rows_now, hp.n_audio_ctx, c->al_seqs, c->al_nseq, c->al_kw_max, nh, c->al_width, l == c->al_l_first, l == c->al_l_last, c->al_n_heads, c->al_acc,
                       c->al_x, s); }
}
// rows [r0, r0 + Bw) of the window batch on stream s: sequences are independent, so groups of rows can run on their own streams
// prefill: the rows are prompt tokens (c->pf_st, scratch from row 0), several per sequence: the K / V caches are addressed through the row's sequence (pad) and cache row (seek)
static void run_decoder_step(skw_ctx* c, int r0, int Bw, int pos, bool want_logits, hipStream_t s, bool prefill = false) {
    skw_model* m = c->m; const skw_hparams& hp = m->hp; const int dt = hp.n_text_state, H = hp.n_text_head, nc = hp.n_audio_ctx, ntc = hp.n_text_ctx;
    const float KQscale = (float)pow((double)((float)dt / H), -0.25);
    const int live = c->live_rows_hint >= 0 ? std::min(c->live_rows_hint, Bw) : Bw;      // rows whose attention kernels do work (algorithmic-byte booking of the profile)
    c->cur = s;
    float* dx = c->dx + (size_t)r0 * dt; half_t* dy16 = c->dy16 + (size_t)r0 * dt; half_t* dq16 = c->dq16 + (size_t)r0 * dt; half_t* datt16 = c->datt16 + (size_t)r0 * dt;
    half_t* dh16 = c->dh16 + (size_t)r0 * 4 * dt; SkwSeqState* st = prefill ? c->pf_st : c->st + r0;
    const int* seqp = prefill ? &st[0].pad : nullptr;                                  // row -> sequence for the attention kernels
    // where the QKV epilogue appends a row's K / V: absolute cache row (prefill) or position inside the row's own cache
    const int* kvpos = prefill ? &st[0].seek : &st[0].cur_pos;
    // per-clip audio context: the rows' key counts sit next to `active` in device memory, so a captured step holds none; null while every slot is full length (today's launches)
    const int* nkeys = c->var_k ? &st[0].n_keys : nullptr;
    const long kv_ld = prefill ? 0 : (long)ntc * dt;
    // The prompt pass in the exact precision: one read of a sequence's cross K / V^T per 16 of its prompt tokens (k_xattn_prefill_exact) instead of one per token.  Every output is
    // the single-query kernel's, bit for bit, so the cut below is a speed choice alone: passes whose longest prompt is shorter keep the single-query kernel on every row.
    const bool xq_mq = prefill && c->precision == SKW_PRECISION_EXACT && c->prompt_xattn_mq_on && c->pf_nseq > 0 && c->pf_nq_max >= SKW_XATTN_MQ_MIN_NQ;
    if (use_q8(c)) {   // quantised file, exact precision: ggml's arithmetic (see run_encoder); the row group's q8 scratch starts at its first row
        float* dy32 = c->dy32 + (size_t)r0 * dt; float* datt32 = c->datt32 + (size_t)r0 * dt; float* dh32 = c->dh32 + (size_t)r0 * 4 * dt;
        skw_dec_embed_f32(m->te32, m->d_pe, &st[0].cur_token, &st[0].cur_pos, Bw, dt, dx, s);
        for (int l = 0; l < hp.n_text_layer; ++l) {
            const DecLayer& L = m->dec[l];
            half_t* sk = c->selfK + ((size_t)l * c->max_batch + r0) * ntc * dt; half_t* sv = c->selfV + ((size_t)l * c->max_batch + r0) * ntc * dt;
            half_t* ck = c->crossK + ((size_t)l * c->max_batch + r0) * c->kclip(); half_t* cv = c->crossV + ((size_t)l * c->max_batch + r0) * H * 64 * c->Tpad;
            Q8_LN(c, dx, Bw, dt, L.attn_ln, r0, dy32);
            { SkwGemmArgs a = q8_args(Bw, dq16, dt, EPI_DEC_QKV); a.scale = KQscale; a.has_scale = 1; a.n_ctx = dt; a.C2 = sk; a.C3 = sv; a.ldc2 = kv_ld;
            a.pos_ptr = kvpos; a.pos_stride = (int)(sizeof(SkwSeqState) / sizeof(int)); Q8_GEMM(c, a, L.qkv, r0, true); }
            { ProfScope p_(c, PC_DEC_ATTN, 0, 4.0 * live * (pos + 1) * dt);
              SkwQ8Out qo{c->q8_a + (size_t)r0 * c->q8_kmax, c->q8_d + (size_t)r0 * (c->q8_kmax / 32), c->q8_s + (size_t)r0 * (c->q8_kmax / 32), Bw};
              skw_dec_self_attn(dq16, sk, sv, &st[0].cur_pos, Bw, H, dt, ntc, nullptr, &st[0].active, s, 0, qo, seqp); }
            { SkwGemmArgs a = q8_args(Bw, dx, dt, EPI_F32); a.res = dx; a.ldres = dt; Q8_GEMM(c, a, L.o, r0, true); }
            Q8_LN(c, dx, Bw, dt, L.cross_ln, r0, dy32);
            { SkwGemmArgs a = q8_args(Bw, dq16, dt, EPI_F16_PLAIN); a.scale = KQscale; a.has_scale = 1; Q8_GEMM(c, a, L.cq, r0, true); }
            align_hook(c, l, dq16, ck, s);
            { ProfScope p_(c, PC_DEC_XATTN, 4.0 * live * (double)nc * dt, 4.0 * live * (double)nc * dt);
            if (!(xq_mq && skw_xattn_prefill_exact(dq16, ck, cv, (half_t*)datt32, c->pf_nseq, c->pf_nq_max, c->pf_meta, c->pf_meta + c->max_batch, c->pf_meta + 2 * c->max_batch, H, dt, nc,
                                                   c->Tpad, s, 1, c->var_k ? c->slot_k : nullptr)))
            skw_dec_cross_attn_vt(dq16, ck, cv, Bw, H, dt, nc, c->Tpad, (half_t*)datt32, &st[0].active, s, 1, 0, seqp, nullptr, nullptr, 0, nullptr, nkeys); }
            Q8_ROWS(c, datt32, dt, Bw, dt, r0);
            { SkwGemmArgs a = q8_args(Bw, dx, dt, EPI_F32); a.res = dx; a.ldres = dt; Q8_GEMM(c, a, L.co, r0, true); }
            Q8_LN(c, dx, Bw, dt, L.mlp_ln, r0, dy32);
            { SkwGemmArgs a = q8_args(Bw, dh32, 4L * dt, EPI_GELU_F32); a.gelu_tab = m->gelu_tab; Q8_GEMM(c, a, L.fc1, r0, true); }
            Q8_ROWS(c, dh32, 4L * dt, Bw, 4 * dt, r0);
            { SkwGemmArgs a = q8_args(Bw, dx, dt, EPI_F32); a.res = dx; a.ldres = dt; Q8_GEMM(c, a, L.fc2, r0, true); }
        }
        if (want_logits) {
            Q8_LN(c, dx, Bw, dt, m->d_ln, r0, dy32);
            SkwGemmArgs a = q8_args(Bw, c->logits + (size_t)r0 * hp.n_vocab, hp.n_vocab, EPI_F32); Q8_GEMM(c, a, m->te, r0, true);
        }
        c->cur = c->stream;
        return;
    }
    // The first layer's LayerNorm rides on the embedding kernel (same bits: skw_ln_rows).  (The others riding on the GEMM that completes x — the last workgroup to arrive per
    // 16-row block normalises it — measured 15.6 us for GEMM + tail against 5.1 + 5.0 for the two launches, profiles/r02c: a launch boundary is cheaper on this part than a
    // hand-over inside a kernel.  Removed in round 5.)
    const bool embed_ln = dt <= 1536;
    // LayerNorm without a launch (f16_mfma): the GEMM that consumes LayerNorm(x) loads the f32 rows, takes their statistics from its own
    // registers and normalises on the way into the MFMA.  35 of the step's 136 launches go.  SKW_DEC_LN_STATS=0 restores the LayerNorm kernels.
    const bool lnA = c->ln_stats_on && embed_ln && c->precision == SKW_PRECISION_F16_MFMA && (dt & 127) == 0 && m->dec[0].qkv.w_nat && m->dec[0].cq.w_nat
        && m->dec[0].fc1.w_nat && m->dec[0].cq.k_pad == dt;
    // the prompt pass of a long-form batch is thousands of rows: there the projections are the encoder's big-tile GEMM (f16_mfma; the small-M kernels stream the
    // weights once per 16 rows and reach ~50 TF/s at M = 4096, the big kernel 600).  The QKV product keeps the decode form: its epilogue appends to the K / V caches.
    const bool bigM = prefill && c->precision == SKW_PRECISION_F16_MFMA && Bw >= 256 && !skw_sw(SW_PROMPT_SMALL_GEMM);
    const bool afrag_on = skw_sw(SW_DEC_AFRAG) != 0;
    // the attention kernels leave their rows as the fragment-order A image the out-projections read (f16_mfma, small-M kernels on both sides; the cross attention: the one-pass
    //  kernel / its multi-query prompt form)
    const bool sa_frag = afrag_on && c->precision == SKW_PRECISION_F16_MFMA && !bigM && (dt & 127) == 0, xa_frag = sa_frag && c->kv_frag();
    auto gemm_s = [&](const SkwGemmArgs& a) { if (bigM) GEMM(c, a, a.K); else GEMM_S(c, a, a.K); };
    // a GEMM fed by LayerNorm(dx): the normalising form (site >= 0), else LayerNorm kernel + GEMM
    auto gemm_ln = [&](SkwGemmArgs a, const DevLin& Lw, const DevLN& ln, int site, bool normalised) {
        if (bigM && a.epi != EPI_DEC_QKV && !normalised) {
            { ProfScope p_(c, PC_LAYERNORM, 0, 6.0 * a.M * a.K); skw_layernorm(dx, a.M, a.K, ln.w, ln.b, dy16, nullptr, s); }
            GEMM(c, a, a.K); return;
        }
        if (lnA && site >= 0) {
            a.W = Lw.w_nat; a.Wf = Lw.w_nat_frag; a.ln_x = dx; a.ln_w = ln.w; a.ln_b = ln.b;
            {   // (the scope ends before the fall-back below books the same product a second time: ADVICE r3)
                ProfScope p(c, PC_GEMM_SMALL, 2.0 * a.M * a.N * a.K, 4.0 * a.M * a.K + 2.0 * a.N * a.K + 2.0 * a.M * a.N);
                if (skw_gemm16_small_lnA(a, c->cur)) return;
                p.cancel();
            }
            a.W = Lw.w; a.Wf = Lw.w_frag; a.ln_x = nullptr;
        }
        GEMM_LN(c, a, dx, ln, dy16, s, normalised);
    };
    if (embed_ln) skw_dec_embed_ln(m->te.w, m->d_pe, &st[0].cur_token, &st[0].cur_pos, Bw, dt, dx, m->dec[0].attn_ln.w, m->dec[0].attn_ln.b, dy16, s);
    else skw_dec_embed(m->te.w, m->d_pe, &st[0].cur_token, &st[0].cur_pos, Bw, dt, dx, s);
    for (int l = 0; l < hp.n_text_layer; ++l) {
        const DecLayer& L = m->dec[l];
        half_t* sk = c->selfK + ((size_t)l * c->max_batch + r0) * ntc * dt; half_t* sv = c->selfV + ((size_t)l * c->max_batch + r0) * ntc * dt;
        half_t* ck = c->crossK + ((size_t)l * c->max_batch + r0) * c->kclip(); half_t* cv = c->crossV + ((size_t)l * c->max_batch + r0) * H * 64 * c->Tpad;
        { SkwGemmArgs a = gemm_args(dy16, dt, L.qkv, Bw, dq16, dt, EPI_DEC_QKV); a.scale = KQscale; a.has_scale = 1; a.n_ctx = dt;
          a.C2 = sk; a.C3 = sv; a.ldc2 = kv_ld; a.pos_ptr = kvpos; a.pos_stride = (int)(sizeof(SkwSeqState) / sizeof(int));
          gemm_ln(a, L.qkv, L.attn_ln, l > 0 ? 3 * (l - 1) + 2 : -1, l == 0 && embed_ln); }
        { ProfScope p_(c, PC_DEC_ATTN, 0, 4.0 * live * (pos + 1) * dt);
        skw_dec_self_attn(dq16, sk, sv, &st[0].cur_pos, Bw, H, dt, ntc, datt16, &st[0].active, s, 0, SkwQ8Out{nullptr, nullptr, nullptr, 0}, seqp, c->precision == SKW_PRECISION_F16_MFMA, sa_frag);
        }
        { SkwGemmArgs a = gemm_args(datt16, dt, L.o, Bw, dx, dt, EPI_F32); a.res = dx; a.ldres = dt; a.a_frag = sa_frag; gemm_s(a); }
        {
            { SkwGemmArgs a = gemm_args(dy16, dt, L.cq, Bw, dq16, dt, EPI_F16_PLAIN); a.scale = KQscale; a.has_scale = 1; gemm_ln(a, L.cq, L.cross_ln, 3 * l, false); }
            align_hook(c, l, dq16, ck, s);
            const bool xp_mq = skw_sw(SW_PROMPT_XATTN_MQ) != 0;
            if (prefill && xp_mq && c->precision == SKW_PRECISION_F16_MFMA && c->pf_nseq > 0) {
                // the prompt pass in the tolerance precision: one read of a sequence's cross K / V^T for up to 128 of its prompt tokens (the encoder attention kernel with the
                // prompt tokens as queries) instead of one per token — 4.6 MB per row per layer otherwise.  The exact precision keeps the single-query kernel: bit-identical to stepping.
                ProfScope p_(c, PC_DEC_XATTN, 4.0 * Bw * (double)nc * 64.0 * H, 4.0 * c->pf_nseq * (double)nc * dt);
                skw_xattn_prefill16(dq16, ck, cv, datt16, c->pf_nseq, c->pf_nq_max, c->pf_meta, c->pf_meta + c->max_batch, c->pf_meta + 2 * c->max_batch, H, dt, nc, c->Tpad, s, c->kv_frag(), xa_frag,
                                    c->var_k ? c->slot_k : nullptr);
            } else if (xq_mq && skw_xattn_prefill_exact(dq16, ck, cv, datt16, c->pf_nseq, c->pf_nq_max, c->pf_meta, c->pf_meta + c->max_batch, c->pf_meta + 2 * c->max_batch, H, dt, nc,
                                                        c->Tpad, s, 0, c->var_k ? c->slot_k : nullptr)) {
            } else
            if (c->kv8_step()) {      // cross_kv = q8_0: every launch of the single-query kernel reads the q8 image (2 x 1.0625 bytes per key and channel)
                ProfScope p_(c, PC_DEC_XATTN, 4.0 * live * (double)nc * dt, 2.125 * live * (double)nc * dt, true);
                skw_dec_cross_attn_kv8(dq16, c->crossKV8 + ((size_t)l * c->max_batch + r0) * c->kv8_slot(), Bw, H, dt, nc, c->Tpad, datt16, &st[0].active, s, 0, seqp, p_.ev_a(), p_.ev_b(), xa_frag,
                                       prefill ? nullptr : kclk_node(c, c->cur_group, l), nkeys);
            } else
            { ProfScope p_(c, PC_DEC_XATTN, 4.0 * live * (double)nc * dt, 4.0 * live * (double)nc * dt, true);
            skw_dec_cross_attn_vt(dq16, ck, cv, Bw, H, dt, nc, c->Tpad, datt16, &st[0].active, s, 0, c->kv_frag() ? 2 : c->precision == SKW_PRECISION_F16_MFMA, seqp, p_.ev_a(), p_.ev_b(), xa_frag,
                                  prefill ? nullptr : kclk_node(c, c->cur_group, l), nkeys);
            }
        }
        { SkwGemmArgs a = gemm_args(datt16, dt, L.co, Bw, dx, dt, EPI_F32); a.res = dx; a.ldres = dt; a.a_frag = xa_frag; gemm_s(a); }
        // f16_mfma, small-M kernels on both sides: fc1 leaves its output as the fragment-order A image fc2 reads (fc2 7.4 -> 6.5 us per launch); the prompt pass's big-tile GEMMs keep rows
        const bool h_frag = afrag_on && c->precision == SKW_PRECISION_F16_MFMA && !bigM && (dt & 127) == 0;
        { SkwGemmArgs a = gemm_args(dy16, dt, L.fc1, Bw, dh16, 4L * dt, EPI_GELU_F16_KPERM); a.gelu_tab = m->gelu_tab; a.c_frag = h_frag; gemm_ln(a, L.fc1, L.mlp_ln, 3 * l + 1, false); }
        { SkwGemmArgs a = gemm_args(dh16, 4L * dt, L.fc2, Bw, dx, dt, EPI_F32); a.res = dx; a.ldres = dt; a.a_frag = h_frag; gemm_s(a); }
    }
    if (want_logits) {
        // (the vocabulary kernel's 256 workgroups would each normalise all 64 rows: measured +6.4 us against this 5.0 us launch)
        { ProfScope p_(c, PC_LAYERNORM, 0, 6.0 * Bw * dt); skw_layernorm(dx, Bw, dt, m->d_ln.w, m->d_ln.b, dy16, nullptr, s); }
        SkwGemmArgs a = gemm_args(dy16, dt, m->te, Bw, c->logits + (size_t)r0 * hp.n_vocab, hp.n_vocab, EPI_F32); GEMM_S(c, a, a.K);
    }
    c->cur = c->stream;
}

// One generation step of a row group as an executable graph: decoder step (positions and tokens read from the device state),
// logit filters + sampling, and the read-back of the group's active count.  Captured once per (group, rows, filter params).
// rows: the per-row form of the sampler (skw_full_batch_mixed) — lp then holds model constants and any_sampled only, so one graph serves every parameter mix of its shape
// cons: some clip of the call has decoding constraints (skw_full_batch_rules): k_dec_constrain sits between the logits GEMM and the sampler; the rows' records are device memory,
//  so that graph too serves every mix.  Calls without constraints key cons = 0 and replay the graphs they always did
// gram: some clip of the call has a grammar (skw_full_batch_grammar): k_dec_grammar follows k_dec_constrain; keyed and served from device records the same way
static hipGraphExec_t step_graph(skw_ctx* c, int g, int r0, int n, const SkwLogitParams& lp, bool rows, bool cons, bool gram) {
    for (size_t i = 0; i < c->step_graphs.size(); ++i) {
        auto& sg = c->step_graphs[i];
        if (sg.g == g && sg.r0 == r0 && sg.n == n && sg.precision == c->precision && sg.ln_stats == c->ln_stats_on && sg.kclk == c->kclk_on && sg.sw_epoch == skw_sw_epoch() &&
            sg.var_k == (int)c->var_k && sg.kv8 == (int)c->kv8_step() && sg.rows == (int)rows && sg.cons == (int)cons && sg.gram == (int)gram && memcmp(&sg.lp, &lp, sizeof lp) == 0) {
            if (i + 1 != c->step_graphs.size()) { auto hit = sg; c->step_graphs.erase(c->step_graphs.begin() + i); c->step_graphs.push_back(hit); }   // most recently used last
            return c->step_graphs.back().exec;
        }
    }
    const int NV = c->m->hp.n_vocab; hipStream_t s = c->gstream[g]; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) return nullptr;
    c->cur_group = g;
    run_decoder_step(c, r0, n, 0, true, s);
    c->cur_group = 0;
    if (cons) skw_dec_constrain(c->logits + (size_t)r0 * NV, NV, lp.tok_eot, c->row_cons + r0, c->st + r0, c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, s);
    if (gram) skw_dec_grammar(c->logits + (size_t)r0 * NV, NV, lp.tok_eot, c->row_gram + r0, c->st + r0, c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->gr_voc_off, c->gr_voc_bytes, s);
    if (rows) skw_dec_sample_rows(c->logits + (size_t)r0 * NV, c->static_mask_pair, lp, c->row_rules + r0, c->st + r0, c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->d_row_live + r0,
        c->probs + (size_t)r0 * skw_probs_row_floats(NV), c->rng, c->clip_idx + r0, c->prompt_buf + (size_t)r0 * SKW_PROMPT_CAP, s);
    else skw_dec_sample(c->logits + (size_t)r0 * NV, c->static_mask, lp, c->st + r0, c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->d_row_live + r0,
        c->probs + (size_t)r0 * skw_probs_row_floats(NV), c->rng, c->clip_idx + r0, c->prompt_buf + (size_t)r0 * SKW_PROMPT_CAP, s);
    if (hipStreamEndCapture(s, &graph) != hipSuccess || !graph) return nullptr;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) exec = nullptr;
    hipGraphDestroy(graph);
    if (exec) {
        // bounded: a long-lived server with ragged batches would otherwise keep one executable graph per (group, rows, params) forever
        if (c->step_graphs.size() >= 24) { hipGraphExecDestroy(c->step_graphs.front().exec); c->step_graphs.erase(c->step_graphs.begin()); }
        skw_ctx::StepGraph sg; sg.g = g; sg.r0 = r0; sg.n = n; sg.precision = c->precision; sg.ln_stats = c->ln_stats_on; sg.kclk = c->kclk_on; sg.var_k = (int)c->var_k; sg.kv8 = (int)c->kv8_step();
         sg.sw_epoch = skw_sw_epoch(); sg.lp = lp; sg.rows = (int)rows; sg.cons = (int)cons; sg.gram = (int)gram; sg.exec = exec; c->step_graphs.push_back(sg);
    }
    return exec;
}

// the always-suppressed tokens (specials, languages, the non-speech list when asked for), packed for both sampler forms
static std::vector<uint8_t> packed_static_mask(const skw_model* m, bool nst) {
    std::vector<uint8_t> mask(m->hp.n_vocab, 0);
    mask[m->tok_not] = 1; mask[m->tok_sot] = 1; mask[m->tok_nosp] = 1; mask[m->tok_solm] = 1; mask[m->tok_translate] = 1; mask[m->tok_transcribe] = 1; mask[m->tok_prev] = 1;
    for (int i = 0; i < m->n_lang; ++i) mask[m->tok_sot + 1 + i] = 1;
    if (nst) { for (int id : m->nst_ids) mask[id] = 1; if (m->tok_sp_dash >= 0) mask[m->tok_sp_dash] = 1; if (m->tok_sp_quote >= 0) mask[m->tok_sp_quote] = 1; }
    std::vector<uint8_t> packed(skw_static_mask_bytes(m->hp.n_vocab)); skw_static_mask_pack(mask.data(), m->hp.n_vocab, packed.data());
    return packed;
}
static void build_static_mask(skw_ctx* c, const skw_full_params* p) {
    if (c->static_mask_nst == (p->suppress_nst ? 1 : 0)) return;
    const std::vector<uint8_t> packed = packed_static_mask(c->m, p->suppress_nst != 0);
    hipMemcpyAsync(c->static_mask, packed.data(), packed.size(), hipMemcpyHostToDevice, c->stream); hipStreamSynchronize(c->stream);
    c->static_mask_nst = p->suppress_nst ? 1 : 0;
}
// the per-row sampler's pair: [0] without, [1] with the non-speech list (a row picks by its own suppress_nst); written once per context
static void build_static_mask_pair(skw_ctx* c) {
    if (c->static_mask_pair_built) return;
    for (int k = 0; k < 2; ++k) {
        const std::vector<uint8_t> packed = packed_static_mask(c->m, k == 1);
        hipMemcpyAsync(c->static_mask_pair + (size_t)k * packed.size(), packed.data(), packed.size(), hipMemcpyHostToDevice, c->stream); hipStreamSynchronize(c->stream);
    }
    c->static_mask_pair_built = 1;
}

// the sampler's view of the model's special tokens and of the whisper_full_params that shape whisper_process_logits
static SkwLogitParams make_logit_params(const skw_model* m, const skw_full_params* p) {
    const skw_hparams& hp = m->hp;
    SkwLogitParams lp{};
    lp.n_vocab = hp.n_vocab;
    lp.tok_eot = m->tok_eot; lp.tok_sot = m->tok_sot; lp.tok_translate = m->tok_translate; lp.tok_transcribe = m->tok_transcribe; lp.tok_solm = m->tok_solm;
    lp.tok_prev = m->tok_prev; lp.tok_nosp = m->tok_nosp; lp.tok_not = m->tok_not; lp.tok_beg = m->tok_beg;
    lp.n_lang = m->n_lang; lp.tok_space = m->tok_space; lp.tok_sp_dash = m->tok_sp_dash; lp.tok_sp_quote = m->tok_sp_quote;
    lp.suppress_blank = p->suppress_blank; lp.suppress_nst = p->suppress_nst; lp.no_timestamps = p->no_timestamps; lp.single_segment = p->single_segment; lp.max_tokens = p->max_tokens;
    lp.tid0_initial = -1;
    if (p->max_initial_ts > 0.0f) { const float precision = (float)WHISPER_CHUNK_SIZE / hp.n_audio_ctx; lp.tid0_initial = (int)roundf(p->max_initial_ts / precision); }
    lp.n_max = hp.n_text_ctx / 2 - 4;
    return lp;
}
// the same six request fields as one row's record for the per-row sampler; mixed_logit_params: what is left in the launch's block (model constants)
static SkwRowRules make_row_rules(const skw_model* m, const skw_full_params* p) {
    const SkwLogitParams lp = make_logit_params(m, p);
    SkwRowRules r{}; r.suppress_blank = lp.suppress_blank; r.suppress_nst = lp.suppress_nst; r.no_timestamps = lp.no_timestamps; r.single_segment = lp.single_segment;
    r.max_tokens = lp.max_tokens; r.tid0_initial = lp.tid0_initial;
    return r;
}
// skw_decode_rules is SkwRowConstraints, field for field (NULL: the default record)
static_assert(sizeof(skw_decode_rules) == sizeof(SkwRowConstraints) && offsetof(skw_decode_rules, bias_id) == offsetof(SkwRowConstraints, bias_id) &&
              offsetof(skw_decode_rules, bias) == offsetof(SkwRowConstraints, bias) && SKW_BIAS_MAX == SKW_CONSTRAIN_BIAS_MAX, "skw_decode_rules is SkwRowConstraints");
static SkwRowConstraints make_row_constraints(const skw_decode_rules* r) {
    SkwRowConstraints o; skw_decode_rules d; if (!r) { skw_decode_rules_set_default(&d); r = &d; }
    memcpy(&o, r, sizeof o); o.pad = 0;
    return o;
}
static SkwLogitParams mixed_logit_params(const skw_model* m) {
    skw_full_params z{};      // (no request: the six fields stay 0 / -1 and the per-row form never reads them)
    return make_logit_params(m, &z);
}

static int load_clips(skw_ctx* c, const float* const* pcm, const int32_t* n_samples, int n, int on_device, std::vector<int>& n_len, std::vector<int>& n_len_org) {
    char* errbuf = c->errbuf;
    std::vector<long> off(n); std::vector<int> ns(n); n_len.resize(n); n_len_org.resize(n);
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] < 0 || n_samples[i] > c->max_samples) { snprintf(errbuf, 512, "clip %d has %d samples; context was created for at most %d", i, n_samples[i], c->max_samples); return -1; }
        off[i] = (long)i * c->max_samples; ns[i] = n_samples[i];
        n_len[i] = (int)(((long)n_samples[i] + WHISPER_SAMPLE_RATE * 30 + 2 * (WHISPER_N_FFT / 2) - WHISPER_N_FFT) / WHISPER_HOP);
        n_len_org[i] = 1 + (n_samples[i] + WHISPER_N_FFT / 2 - WHISPER_N_FFT) / WHISPER_HOP;
        if (n_samples[i] > 0) HIPCHK(hipMemcpyAsync(c->pcm + off[i], pcm[i], sizeof(float) * n_samples[i], on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(c->pcm_off, off.data(), sizeof(long) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->n_samples, ns.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->n_len, n_len.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // host vectors go out of scope
    return 0;
}

// cross K/V of window slots src_slot[r] -> dst_slot[r], every layer, 16 bytes per thread (temperature retries keep their encoder pass)
__global__ void k_slot_copy(const half_t* src, long src_layer_stride, half_t* dst, long dst_layer_stride, const int* src_slot, const int* dst_slot, long slot_elems) {
    const int r = blockIdx.y, l = blockIdx.z;
    const uint4* s4 = (const uint4*)(src + (long)l * src_layer_stride + (long)src_slot[r] * slot_elems);
    uint4* d4 = (uint4*)(dst + (long)l * dst_layer_stride + (long)dst_slot[r] * slot_elems);
    const long n16 = slot_elems >> 3;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) d4[i] = s4[i];
}
// The windows in `old_slots` (ascending new slot order 0 .. R-1) are decoded again at the next temperature: their cross K/V move to slots
// 0 .. R-1 through a staging copy (a direct move could overwrite another retry's source), instead of running the encoder on them again.
static bool retry_slots_in_place(const std::vector<int>& old_slots) { for (size_t k = 0; k < old_slots.size(); ++k) if (old_slots[k] != (int)k) return false; return true; }
static int move_retry_slots(skw_ctx* c, const std::vector<int>& old_slots) {
    char* errbuf = c->errbuf; const skw_hparams& hp = c->m->hp; const int R = (int)old_slots.size(), L = hp.n_text_layer;
    if (retry_slots_in_place(old_slots)) return 0;
    const long ke = (long)c->kclip(), ka = (long)c->Tpad * hp.n_text_state, ve = (long)hp.n_text_head * 64 * c->Tpad;      // ka: the staging buffer is sized like crossK (Tpad rows per slot)
    if (!c->stageK || !c->stageV || !c->slot_map) {      // all three or none: a partial failure must not leave a later retry launching k_slot_copy on a null buffer
        half_t *sk = nullptr, *sv = nullptr; int* sm = nullptr;
        if (hipMalloc((void**)&sk, (size_t)L * c->max_batch * ka * 2) != hipSuccess || hipMalloc((void**)&sv, (size_t)L * c->max_batch * ve * 2) != hipSuccess
            || hipMalloc((void**)&sm, sizeof(int) * 2 * c->max_batch) != hipSuccess) {
            hipFree(sk); hipFree(sv); hipFree(sm); snprintf(errbuf, 512, "temperature retry: staging buffers for the cross K/V move could not be allocated"); return -1;
        }
        poison_floats(sk, (size_t)L * c->max_batch * ka * 2); poison_floats(sv, (size_t)L * c->max_batch * ve * 2);
        hipFree(c->stageK); hipFree(c->stageV); hipFree(c->slot_map); c->stageK = sk; c->stageV = sv; c->slot_map = sm;
    }
    std::vector<int> h(2 * (size_t)c->max_batch, 0);
    for (int k = 0; k < R; ++k) { h[k] = old_slots[k]; h[c->max_batch + k] = k; }
    HIPCHK(hipMemcpyAsync(c->slot_map, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                                   // (h is a local; retries are rare)
    const int* olds = c->slot_map; const int* news = c->slot_map + c->max_batch;
    const dim3 grid(64, R, L);
    hipLaunchKernelGGL(k_slot_copy, grid, dim3(256), 0, c->stream, c->crossK, (long)c->max_batch * ke, c->stageK, (long)c->max_batch * ke, olds, news, ke);
    hipLaunchKernelGGL(k_slot_copy, grid, dim3(256), 0, c->stream, c->crossV, (long)c->max_batch * ve, c->stageV, (long)c->max_batch * ve, olds, news, ve);
    hipLaunchKernelGGL(k_slot_copy, grid, dim3(256), 0, c->stream, c->stageK, (long)c->max_batch * ke, c->crossK, (long)c->max_batch * ke, news, news, ke);
    hipLaunchKernelGGL(k_slot_copy, grid, dim3(256), 0, c->stream, c->stageV, (long)c->max_batch * ve, c->crossV, (long)c->max_batch * ve, news, news, ve);
    return 0;
}

// ---- skw_full_batch*: one call = validate, load, detect languages, then window batches (plan, stage, prompt pass, step loop, collect) until no clip has audio left, finish.
// The rules of whisper_full_with_state a window is decided by (ladder, prompt, verdict, prompt_past, segment cut, seek advance, contexts) are skw_window_rules.h; what is here
// is the GPU orchestration around them.

// What an entry point asks for: the public skw_full_request (include/skw_engine.h) and what validate_request derives from it.  Everything a request decides is read through
// P(clip); the sampler takes the rows' rules from device memory (skw_dec_sample_rows).  With params_per_clip = 0 every P(clip) is *params and the launches are the uniform ones.
static_assert(sizeof(skw_full_request) == SKW_FULL_REQUEST_MIN, "SKW_FULL_REQUEST_MIN is the struct as first published: a new field goes to the END and leaves the constant alone");
namespace {      // (internal linkage: none of this reaches the library's symbol table)
struct FullRequest : skw_full_request {
    bool constrained = false;      // rules: some clip's record is not the default
    bool aligned = false;          // align: some clip asked (a NULL / not enabled record: the clip is not aligned)
    bool grammared = false;        // grammar: some clip has one
    std::vector<std::vector<SkwTraceStep>> trace_steps;      // tracing / teacher forcing: per clip the records collect_window gathers, finish_call hands out
    explicit FullRequest(const skw_full_request& q) : skw_full_request(q) {}
    bool wants_align(int ci) const { return align && align[ci] && align[ci]->enabled; }
    bool mixed() const { return params_per_clip != 0; }
    bool tracing() const { return traces != nullptr; }
    const skw_full_params& P(int ci) const { return params_per_clip ? params[ci] : *params; }
    int K_of(int ci, const skw_hparams& hp) const { return P(ci).audio_ctx > 0 ? P(ci).audio_ctx : hp.n_audio_ctx; }      // the clip's audio context, every window of it
};
// The call's host state, per clip unless said otherwise
struct CallState {
    explicit CallState(int n) : seek(n, 0), acc(n), temps(n), tidx(n, 0), retry_slot(n, -1), prompt_past(n), last_take(n, 0), lang(n), f_cursor(n, 0), tt0(n), tt1(n) {}
    std::vector<int> n_len, n_len_org, seek; std::vector<SeqAcc> acc;
    std::vector<std::vector<float>> temps; std::vector<int> tidx;      // the clip's temperature ladder and the index its current window is decoded at
    std::vector<int> retry_slot;                                      // the window slot whose cross K/V a retrying clip left behind (-1: not retrying)
    std::vector<std::vector<int>> prompt_past; std::vector<int> last_take;      // text already produced conditions the next window of the same clip; what the last prompt took of it
    std::vector<int> lang, f_cursor;                                  // f_cursor (tracing): decisions of the clip made so far (= its position in forced_ids[i])
    // word timestamps: per clip the times of its result tokens (parallel to acc.tok; -1: none), and the windows collect_window accepted for alignment in this round
    struct AlignJob { int ci, slot, seek, n_keys; std::vector<int> text, idx; };      // text: the window's text tokens; idx: where each one's times go in tt0 / tt1
    std::vector<std::vector<int64_t>> tt0, tt1; std::vector<AlignJob> align_jobs;
    SkwLogitParams lp;
    float enc_ms = 0.f, dec_ms = 0.f; int tot_windows = 0, tot_steps = 0; long tot_row_steps = 0; int used_groups = 1, used_group_rows = 0;
};
// One window batch.  Every vector here is the source of an asynchronous copy: the batch lives until collect_window has synchronised the stream.
struct WindowBatch {
    std::vector<int> act, retry_old;      // the clips of the rows; the slots the first R of them (retries) left their cross K/V in
    int R = 0, Bw = 0, enc_rows = 0, prefill_passes = 0;
    std::vector<int> sk, ks, pbuf, np_row, fbuf; std::vector<SkwRowRules> rules;      // per row: seek, key count, prompt (SKW_PROMPT_CAP ids) and its length, forced tokens, request rules
    std::vector<SkwRowConstraints> cons;      // per row: decoding constraints (constrained calls only)
    std::vector<SkwRowGrammar> gram;          // per row: the grammar record, its walk at the start (calls with a grammar only)
};
struct RowGroups { int G = 0; int r0[skw_ctx::MAX_GROUPS], n[skw_ctx::MAX_GROUPS]; bool live[skw_ctx::MAX_GROUPS]; };
}

// finish_call copies the accumulators into the results as bytes: SkwSegment is skw_segment and SkwTokenOut is skw_token, field for field
#define SAME_FIELD(A, B, f) (offsetof(A, f) == offsetof(B, f) && sizeof(A::f) == sizeof(B::f))
static_assert(sizeof(SkwSegment) == sizeof(skw_segment) && SAME_FIELD(SkwSegment, skw_segment, t0) && SAME_FIELD(SkwSegment, skw_segment, t1) &&
              SAME_FIELD(SkwSegment, skw_segment, tok_begin) && SAME_FIELD(SkwSegment, skw_segment, tok_end) && SAME_FIELD(SkwSegment, skw_segment, text_off) &&
              SAME_FIELD(SkwSegment, skw_segment, text_len), "SkwSegment is skw_segment");
static_assert(sizeof(SkwTokenOut) == sizeof(skw_token) && SAME_FIELD(SkwTokenOut, skw_token, id) && SAME_FIELD(SkwTokenOut, skw_token, tid) && SAME_FIELD(SkwTokenOut, skw_token, p) &&
              SAME_FIELD(SkwTokenOut, skw_token, plog) && SAME_FIELD(SkwTokenOut, skw_token, pt) && SAME_FIELD(SkwTokenOut, skw_token, ptsum) &&
              SAME_FIELD(SkwTokenOut, skw_token, margin), "SkwTokenOut is skw_token");
#undef SAME_FIELD

static int ensure_trace_buffers(skw_ctx* c) {
    if (c->trace_dev) return 0;
    int* f = nullptr; SkwTraceStep* t = nullptr;
    if (hipMalloc((void**)&f, sizeof(int) * (size_t)c->max_batch * c->max_tok) != hipSuccess || hipMalloc((void**)&t, sizeof(SkwTraceStep) * (size_t)c->max_batch * c->max_tok) != hipSuccess) {
        hipFree(f); snprintf(c->errbuf, 512, "trace buffers: device allocation failed"); return -1; }
    c->forced_dev = f; c->trace_dev = t;
    return 0;
}

static int validate_request(skw_ctx* c, FullRequest& rq) {
    char* errbuf = c->errbuf; const skw_hparams& hp = c->m->hp;
    if (rq.n_clips < 1 || rq.n_clips > c->max_batch) { snprintf(errbuf, 512, "n_clips %d outside [1, %d]", rq.n_clips, c->max_batch); return -1; }
    // combinations no entry point offers (only skw_full_batch_request can ask for them)
    if (rq.traces && (rq.params_per_clip || rq.rng_state || rq.rules || rq.align || rq.grammar)) {
        snprintf(errbuf, 512, "traces cannot be combined with params_per_clip, rng_state, rules, align or grammar (they are not part of the traced entries)"); return -3; }
    if (rq.text_tokens && (rq.rng_state || rq.context || rq.rules || rq.grammar || rq.traces)) {
        snprintf(errbuf, 512, "text_tokens (forced alignment: nothing is decoded) cannot be combined with rng_state, context, rules, grammar or traces"); return -3; }
    if (rq.forced_ids && (!rq.n_forced || !rq.traces)) { snprintf(errbuf, 512, "forced_ids needs n_forced and traces"); return -3; }
    if (rq.text_tokens && !rq.n_text) { snprintf(errbuf, 512, "text_tokens needs n_text"); return -3; }
    if (rq.text_tokens) for (int i = 0; i < rq.n_clips; ++i) if (!rq.text_tokens[i]) { snprintf(errbuf, 512, "clip %d: no text tokens", i); return -3; }
    for (int i = 0; i < rq.n_clips; ++i) if (rq.P(i).audio_ctx < 0 || rq.P(i).audio_ctx > hp.n_audio_ctx) {
        snprintf(errbuf, 512, "clip %d: audio_ctx %d outside [0, %d] (0 = the model's n_audio_ctx)", i, rq.P(i).audio_ctx, hp.n_audio_ctx); return -3; }
    // contexts handed in (skw_full_batch_context) are checked before anything is launched: a refused call leaves every context, like every generator state, as it was
    if (rq.context) for (int i = 0; i < rq.n_clips; ++i) if (rq.context[i] && !skw_context_check(rq.context[i], SKW_CONTEXT_WORDS - 1, hp.n_vocab, i, errbuf, 512)) return -3;
    rq.constrained = false;
    if (rq.rules) for (int i = 0; i < rq.n_clips; ++i) {
        char who[32]; snprintf(who, sizeof who, "clip %d", i);
        if (!skw_decode_rules_check(rq.rules[i], hp.n_vocab, who, errbuf, 512)) return -3;
        if (!skw_decode_rules_is_default(rq.rules[i])) rq.constrained = true;
    }
    rq.grammared = false;
    if (rq.grammar) for (int i = 0; i < rq.n_clips; ++i) {
        char who[32]; snprintf(who, sizeof who, "clip %d", i);
        bool checked = false; for (int k = 0; k < i && !checked; ++k) checked = rq.grammar[k] == rq.grammar[i];      // (one record handed in for several clips is read once)
        if (!checked && !skw_grammar_check(rq.grammar[i], who, errbuf, 512)) return -3;
        if (rq.grammar[i]) rq.grammared = true;
    }
    rq.aligned = false;
    if (rq.align) for (int i = 0; i < rq.n_clips; ++i) {
        if (!skw_align_check_params(rq.align[i], hp.n_text_layer, hp.n_text_head, i, errbuf, 512)) return -3;
        if (rq.wants_align(i)) rq.aligned = true;
    }
    if (rq.aligned && !rq.times) { snprintf(errbuf, 512, "alignment asked for without a place for the token times"); return -3; }
    if (rq.text_tokens) for (int i = 0; i < rq.n_clips; ++i) {
        if (!rq.wants_align(i)) { snprintf(errbuf, 512, "clip %d: skw_align_batch needs an enabled alignment record", i); return -3; }
        if (rq.n_text[i] < 1 || rq.n_text[i] > hp.n_text_ctx / 2) { snprintf(errbuf, 512, "clip %d: %d text tokens outside [1, %d]", i, rq.n_text[i], hp.n_text_ctx / 2); return -3; }
        for (int k = 0; k < rq.n_text[i]; ++k) if (rq.text_tokens[i][k] < 0 || rq.text_tokens[i][k] >= c->m->tok_eot) {
            snprintf(errbuf, 512, "clip %d: text token %d (id %d) is not a text token", i, k, rq.text_tokens[i][k]); return -3; }
        if (rq.n_samples[i] > WHISPER_SAMPLE_RATE * 30) { snprintf(errbuf, 512, "clip %d: skw_align_batch aligns one window (at most 30 s of audio)", i); return -3; }
    }
    return 0;
}

// clips to the device, the static mask(s), log-mel; the call's per-clip host state
static int load_call(skw_ctx* c, const FullRequest& rq, CallState& cs) {
    char* errbuf = c->errbuf; const int n_clips = rq.n_clips;
    for (int i = 0; i < n_clips; ++i) { memset(&rq.results[i], 0, sizeof(skw_result)); rq.results[i].min_margin = INFINITY; }
    if (c->kclk_on && kclk_reset(c)) return -1;
    HIPCHK(hipEventRecord(c->ev[0], c->stream));
    if (load_clips(c, rq.pcm, rq.n_samples, n_clips, rq.pcm_on_device, cs.n_len, cs.n_len_org)) return -1;
    if (rq.mixed()) build_static_mask_pair(c); else build_static_mask(c, rq.params);
    run_mel(c, n_clips);
    HIPCHK(hipEventRecord(c->ev[1], c->stream));
    for (int ci = 0; ci < n_clips; ++ci) cs.temps[ci] = skw_temperature_ladder(rq.P(ci).temperature, rq.P(ci).temperature_inc);      // (a clip's own ladder)
    // a clip's context (skw_full_batch_context) is its prompt_past as whisper_full_with_state's window loop finds it: the first window takes from it under the rules of every later one
    if (rq.context) for (int i = 0; i < n_clips; ++i) if (rq.context[i]) cs.prompt_past[i].assign(rq.context[i] + 1, rq.context[i] + 1 + rq.context[i][0]);
    // the sampled passes' generator: whisper.cpp keeps ONE std::mt19937 per state (decoder 0, seeded with 0 when the state is created) and lets it run on across calls.  A caller
    // that owns such a stream per clip (the plugin: one per instance, lib.rs:377-379) hands its state in and gets it back (skw_full_batch_rng); without one the stream starts at
    // seed 0 in every call (D2': what a batch of unrelated clips can do)
    skw_rng_seed(c->rng, n_clips, 0u, c->stream);
    if (rq.rng_state) for (int i = 0; i < n_clips; ++i) if (rq.rng_state[i]) {
        if (rq.rng_state[i][624] > 624u) { snprintf(errbuf, 512, "clip %d: the generator state handed in is not a std::mt19937 state (index %u)", i, rq.rng_state[i][624]); return -1; }
        HIPCHK(hipMemcpyAsync(c->rng + (size_t)i * SKW_RNG_WORDS, rq.rng_state[i], sizeof(uint32_t) * SKW_RNG_WORDS, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

// language: fixed by the caller, or (lang_id < 0, whisper.cpp's "auto") detected per clip from the [sot] step on the first window
static int detect_languages(skw_ctx* c, const FullRequest& rq, CallState& cs) {
    char* errbuf = c->errbuf; skw_model* m = c->m; const int NV = m->hp.n_vocab, n_clips = rq.n_clips; std::vector<int>& lang = cs.lang;
    bool any_auto = false;
    for (int i = 0; i < n_clips; ++i) { lang[i] = rq.P(i).lang_id; rq.results[i].lang_id = lang[i]; if (lang[i] < 0 && !any_auto) { any_auto = true;
        if (NV < 51865) { if (rq.mixed()) snprintf(errbuf, 512, "failed to auto-detect language: the model is not multilingual (clip %d)", i);
                          else snprintf(errbuf, 512, "failed to auto-detect language: the model is not multilingual");
                          return -3; } } }
    if (!any_auto) return 0;
    // the detection pass runs on the rows that asked for it
    std::vector<int> act, zero(n_clips, 0); for (int i = 0; i < n_clips; ++i) if (lang[i] < 0 && cs.n_len_org[i] > 0) act.push_back(i);
    const int Bd = (int)act.size();
    if (Bd > 0) {
        HIPCHK(hipMemcpyAsync(c->clip_idx, act.data(), sizeof(int) * Bd, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->seek, zero.data(), sizeof(int) * Bd, hipMemcpyHostToDevice, c->stream));
        std::vector<int> kd(Bd); for (int j = 0; j < Bd; ++j) kd[j] = rq.K_of(act[j], m->hp);      // detection sees the first window as the clip's own audio_ctx shapes it
        const int rows_d = set_slot_k(c, kd.data(), Bd, 0, c->stream);
        run_conv(c, Bd, 0, rows_d); run_encoder(c, Bd, false, true, 0, rows_d);
        hipLaunchKernelGGL(k_set_tokens, dim3(Bd), dim3(1), 0, c->stream, c->st, m->tok_sot, 0, c->slot_k);
        run_decoder_step(c, 0, Bd, 0, true, c->stream);
        hipLaunchKernelGGL(k_lang_argmax, dim3(Bd), dim3(64), 0, c->stream, c->logits, NV, m->tok_sot, m->n_lang, c->row_tok);
        std::vector<int> det(Bd); HIPCHK(hipMemcpyAsync(det.data(), c->row_tok, sizeof(int) * Bd, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
        for (int j = 0; j < Bd; ++j) { lang[act[j]] = det[j]; rq.results[act[j]].lang_id = det[j]; }
    }
    for (int i = 0; i < n_clips; ++i) if (lang[i] < 0) { lang[i] = 0; rq.results[i].lang_id = 0; }
    return 0;
}

// sot, language, task (, notimestamps): the tail of a row's prompt, from its clip's request
static int prompt_tail(const skw_model* m, const skw_full_params& q, int lang, int32_t* out) {
    int n = 0;
    out[n++] = m->tok_sot;
    if (m->hp.n_vocab >= 51865) { out[n++] = m->tok_sot + 1 + lang; out[n++] = q.translate ? m->tok_translate : m->tok_transcribe; }
    if (q.no_timestamps) out[n++] = m->tok_not;
    return n;
}

// The clips that still have audio to decode ("if only 100ms left, then stop"; "input is too short": delta_min = 10 frames, whisper.cpp #2065).  Windows that are decoded again at
// the next temperature come first: their cross K/V are still in HBM (at last round's slot) and move to slots 0 .. R-1; the encoder then runs only on the new windows, slots
// R .. Bw-1.  false: nothing is left.
static bool plan_window(const FullRequest& rq, const CallState& cs, WindowBatch& w) {
    for (int i = 0; i < rq.n_clips; ++i) if (cs.retry_slot[i] >= 0) { w.act.push_back(i); w.retry_old.push_back(cs.retry_slot[i]); }
    w.R = (int)w.act.size();
    for (int i = 0; i < rq.n_clips; ++i) if (cs.retry_slot[i] < 0 && cs.n_len_org[i] >= SKW_DELTA_MIN && cs.seek[i] + SKW_DELTA_MIN < cs.n_len_org[i]) w.act.push_back(i);
    w.Bw = (int)w.act.size();
    return w.Bw > 0;
}

// retried slots moved, the rows' seeks / key counts / prompts / rules / forced tokens uploaded, the encoder on the new windows, the rows' decoder state (host side)
static int stage_window(skw_ctx* c, const FullRequest& rq, CallState& cs, WindowBatch& w) {
    char* errbuf = c->errbuf; skw_model* m = c->m; const skw_hparams& hp = m->hp; const int Bw = w.Bw, R = w.R; const std::vector<int>& act = w.act;
    if (R > 0 && move_retry_slots(c, w.retry_old)) return -1;
    for (int j = 0; j < Bw; ++j) cs.retry_slot[act[j]] = -1;
    w.sk.resize(Bw); for (int j = 0; j < Bw; ++j) w.sk[j] = cs.seek[act[j]];
    HIPCHK(hipMemcpyAsync(c->clip_idx, act.data(), sizeof(int) * Bw, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->seek, w.sk.data(), sizeof(int) * Bw, hipMemcpyHostToDevice, c->stream));
    // the slots' audio contexts: a retried window (slots 0 .. R-1) keeps its clip's K with the cross K/V it moved
    w.ks.resize(Bw); for (int j = 0; j < Bw; ++j) w.ks[j] = rq.K_of(act[j], hp);
    w.enc_rows = set_slot_k(c, w.ks.data(), Bw, R, c->stream);
    w.pbuf.assign((size_t)Bw * SKW_PROMPT_CAP, 0); w.np_row.assign(Bw, 0);
    for (int j = 0; j < Bw; ++j) {
        const int ci = act[j]; int32_t tail[8]; const int n_tail = prompt_tail(m, rq.P(ci), cs.lang[ci], tail);
        w.np_row[j] = skw_row_prompt(cs.prompt_past[ci], cs.temps[ci][cs.tidx[ci]], tail, n_tail, hp.n_text_ctx, cs.lp.n_max, m->tok_prev, w.pbuf.data() + (size_t)j * SKW_PROMPT_CAP,
                                     &cs.last_take[ci]);
    }
    HIPCHK(hipMemcpyAsync(c->prompt_buf, w.pbuf.data(), sizeof(int) * w.pbuf.size(), hipMemcpyHostToDevice, c->stream));
    if (rq.mixed()) {
        w.rules.resize(Bw); for (int j = 0; j < Bw; ++j) w.rules[j] = make_row_rules(m, &rq.P(act[j]));
        HIPCHK(hipMemcpyAsync(c->row_rules, w.rules.data(), sizeof(SkwRowRules) * Bw, hipMemcpyHostToDevice, c->stream));
    }
    if (rq.constrained) {      // the rows' constraints, like their rules: a clip without a record gets the default, which k_dec_constrain leaves alone
        w.cons.resize(Bw); for (int j = 0; j < Bw; ++j) w.cons[j] = make_row_constraints(rq.rules[act[j]]);
        HIPCHK(hipMemcpyAsync(c->row_cons, w.cons.data(), sizeof(SkwRowConstraints) * Bw, hipMemcpyHostToDevice, c->stream));
    }
    if (rq.grammared) {      // the rows' grammars: the walk starts over in every window and every temperature pass
        w.gram.resize(Bw); for (int j = 0; j < Bw; ++j) w.gram[j] = c->gr_clip[act[j]];
        HIPCHK(hipMemcpyAsync(c->row_gram, w.gram.data(), sizeof(SkwRowGrammar) * Bw, hipMemcpyHostToDevice, c->stream));
    }
    cs.lp.any_sampled = 0; for (int j = 0; j < Bw; ++j) if (cs.temps[act[j]][cs.tidx[act[j]]] > 0.0f) cs.lp.any_sampled = 1;      // (part of the step graph's key: greedy passes run the lean sampler)
    if (rq.tracing()) {      // this pass's forced tokens per row: the clip's sequence from its cursor on (-1 = none: the row feeds its own choices)
        w.fbuf.assign((size_t)Bw * c->max_tok, -1);
        if (rq.forced_ids) for (int j = 0; j < Bw; ++j) { const int ci = act[j]; if (!rq.forced_ids[ci]) continue;
            for (int k = 0; k < c->max_tok && cs.f_cursor[ci] + k < rq.n_forced[ci]; ++k) w.fbuf[(size_t)j * c->max_tok + k] = rq.forced_ids[ci][cs.f_cursor[ci] + k]; }
        HIPCHK(hipMemcpyAsync(c->forced_dev, w.fbuf.data(), sizeof(int) * w.fbuf.size(), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipEventRecord(c->ev[2], c->stream));
    // the retried windows' q8 image, from the f16 images that moved with them (nothing moved: the image of slots 0 .. R-1 still stands)
    if (R > 0 && c->kv8_step() && !retry_slots_in_place(w.retry_old)) kv8_refresh(c, 0, R, true);
    if (R < Bw) { run_conv(c, Bw, R, w.enc_rows); run_encoder(c, Bw, false, true, R, w.enc_rows); }
    HIPCHK(hipEventRecord(c->ev[3], c->stream));
    // decoder state
    for (int j = 0; j < Bw; ++j) {
        SkwSeqState& s = c->h_st[j]; memset(&s, 0, sizeof s);
        s.active = 1; s.seek_delta = SKW_WINDOW_FRAMES; s.seek = w.sk[j];
        s.seek_end = cs.n_len_org[act[j]]; s.n_prompt = w.np_row[j]; s.min_margin = INFINITY; s.cur_token = w.pbuf[(size_t)j * SKW_PROMPT_CAP]; s.cur_pos = 0;
        s.temperature = cs.temps[act[j]][cs.tidx[act[j]]]; s.n_keys = w.ks[j];
    }
    return 0;
}

// The prompt in one pass (whisper.cpp evaluates it in one whisper_decode call): every prompt token but a row's last becomes a row of ONE decoder pass —
// the step's own kernels, a row per (sequence, position), the caches addressed through the row's sequence — which fills the self-attention K / V
// of those positions in every layer; the rows then start at their last prompt token, whose logits the first sampling step needs.  A window of a long
// file carries up to 224 tokens of previous text in its prompt: 225 steps of 1.4 ms become one pass.  Per-row arithmetic does not depend on what else is
// in the batch, so the results are the stepped ones, bit for bit (tests/test_gpu_parity.py).  Ends with the rows' decoder state on the device.
static int prompt_pass(skw_ctx* c, WindowBatch& w) {
    char* errbuf = c->errbuf; const int Bw = w.Bw;
    if (c->prompt_pass_on) {
        const int ntc = c->m->hp.n_text_ctx;
        std::vector<SkwSeqState> pf; std::vector<int> row_end;      // row_end: cumulative rows after each sequence (chunks are whole sequences)
        for (int j = 0; j < Bw; ++j) {
            for (int k = 0; k + 1 < w.np_row[j]; ++k) { SkwSeqState t; memset(&t, 0, sizeof t);
            t.active = 1; t.cur_token = w.pbuf[(size_t)j * SKW_PROMPT_CAP + k]; t.cur_pos = k; t.pad = j; t.seek = j * ntc + k; t.n_keys = w.ks[j]; pf.push_back(t); }
            row_end.push_back((int)pf.size());
            c->h_st[j].cur_token = w.pbuf[(size_t)j * SKW_PROMPT_CAP + w.np_row[j] - 1]; c->h_st[j].cur_pos = w.np_row[j] - 1;
        }
        size_t lo = 0; int jlo = 0;
        while (lo < pf.size()) {
            int jhi = jlo; while (jhi < Bw && row_end[jhi] - (int)lo <= c->rows_cap) ++jhi;      // sequences jlo .. jhi-1 fit (a prompt is at most SKW_PROMPT_CAP - 1 <= rows_cap rows)
            const size_t hi = row_end[jhi - 1]; const int n = (int)(hi - lo);
            if (n > 0) {
                HIPCHK(hipMemcpyAsync(c->pf_st, pf.data() + lo, sizeof(SkwSeqState) * n, hipMemcpyHostToDevice, c->stream));
                std::vector<int> meta((size_t)3 * c->max_batch, 0); int ns = 0, nqmax = 0;
                for (int j = jlo; j < jhi; ++j) { const int r0j = (j ? row_end[j - 1] : 0) - (int)lo, nqj = row_end[j] - (j ? row_end[j - 1] : 0); if (nqj <= 0) continue;
                    meta[ns] = r0j; meta[c->max_batch + ns] = nqj; meta[2 * c->max_batch + ns] = j; nqmax = std::max(nqmax, nqj); ++ns; }
                HIPCHK(hipMemcpyAsync(c->pf_meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, c->stream));
                c->pf_nseq = ns; c->pf_nq_max = nqmax;
                run_decoder_step(c, 0, n, 0, false, c->stream, true);
                c->pf_nseq = 0;
                HIPCHK(hipStreamSynchronize(c->stream));      // (pf and meta are host vectors and pf_st is reused by the next chunk)
                ++w.prefill_passes;
            }
            lo = hi; jlo = jhi;
        }
    }
    HIPCHK(hipMemcpyAsync(c->st, c->h_st, sizeof(SkwSeqState) * Bw, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// row groups: G contiguous ranges of the window batch, each on its own stream (one group while profiling, so kernel times do not overlap)
// Default: ONE row group in both precisions.  Rounds 3-4 shipped two groups for f16_mfma at >= 64 rows (+1.3 % on the step in a same-box A/B, profiles/r04g).  Round 5's in-kernel
// launch clock (skw_ctx_kernel_clock) showed what that bought and cost: the groups' cross-attention launches overlap for 27 % of their time and stretch each other from 28 to
// 35-37 us, a profiler serialises the two streams (its per-kernel averages then describe launches that never ran: decode 129 -> 197 ms under rocprofv3), and the dispatch
// front end is a serial resource — two chains of small kernels on two streams gain ~20 % over one (tools/probe/probe_stream_overlap.hip) while the launch count doubles.
// Same-box, round 5 (profiles/r05d): 167.13 ms (two groups) vs 167.59 ms (one) per 64-clip step — inside the +-1.5 % two builds differ by — with the dominant kernel at
// 0.47 of HBM peak per launch (0.66 while any launch is in flight) against 0.77 as one group.  One group: clock, HIP events and rocprofv3 agree on every launch within 2 %.
// The exact precision loses 3 % with two groups, smaller batches more (16-row launches).  SKW_DECODE_GROUPS=n overrides.
// Groups are cut at multiples of 16 rows: the f16_mfma step keeps its attention / FC1 outputs as fragment-order images (skw_afrag_off), which
// scatter a group's rows over whole 16-row tiles of its scratch — two groups sharing a tile would overwrite each other.
static RowGroups cut_row_groups(const skw_ctx* c, int Bw) {
    RowGroups rg; const int n_groups = c->n_groups > 0 ? c->n_groups : 1;
    const int Gw = std::max(1, std::min(n_groups, Bw / 8));
    int prev = 0;
    for (int g = 1; g <= Gw; ++g) {
        const int cut = g == Gw ? Bw : std::min(Bw, (int)(((long)Bw * g / Gw + 8) & ~15L));
        if (cut > prev) { rg.r0[rg.G] = prev; rg.n[rg.G] = cut - prev; rg.live[rg.G] = true; ++rg.G; prev = cut; }
    }
    return rg;
}

// one group's sampler launch (eager steps: profiling, tracing, or no graph)
static void sample_group(skw_ctx* c, const FullRequest& rq, const SkwLogitParams& lp, const RowGroups& rg, int g) {
    const int NV = c->m->hp.n_vocab, r0 = rg.r0[g], n = rg.n[g]; const bool tracing = rq.tracing();
    c->cur = c->gstream[g];
    if (rq.constrained) { ProfScope p_(c, PC_DEC_CONSTRAIN, 0, 0);
      skw_dec_constrain(c->logits + (size_t)r0 * NV, NV, lp.tok_eot, c->row_cons + r0, c->st + r0, c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->gstream[g]); }
    if (rq.grammared) { ProfScope p_(c, PC_DEC_GRAMMAR, 0, 8.0 * n * NV);      // (a pass over the rows to read and one to write; the table's touched rows are noise beside it)
      skw_dec_grammar(c->logits + (size_t)r0 * NV, NV, lp.tok_eot, c->row_gram + r0, c->st + r0, c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->gr_voc_off, c->gr_voc_bytes,
                      c->gstream[g]); }
    { ProfScope p_(c, PC_DEC_SAMPLE, 0, 4.0 * n * NV);
      if (rq.mixed()) skw_dec_sample_rows(c->logits + (size_t)r0 * NV, c->static_mask_pair, lp, c->row_rules + r0, c->st + r0,
        c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->d_row_live + r0, c->probs + (size_t)r0 * skw_probs_row_floats(NV), c->rng,
        c->clip_idx + r0, c->prompt_buf + (size_t)r0 * SKW_PROMPT_CAP, c->gstream[g]);
      else skw_dec_sample(c->logits + (size_t)r0 * NV, c->static_mask, lp, c->st + r0,
        c->toks + (size_t)r0 * c->max_tok, c->max_tok, n, c->d_row_live + r0, c->probs + (size_t)r0 * skw_probs_row_floats(NV), c->rng,
        c->clip_idx + r0, c->prompt_buf + (size_t)r0 * SKW_PROMPT_CAP, c->gstream[g],
        tracing ? c->forced_dev + (size_t)r0 * c->max_tok : nullptr, tracing ? c->trace_dev + (size_t)r0 * c->max_tok : nullptr); }
    c->cur = c->stream;
}

// every step = decoder step (token and position from the device state) + k_dec_sample, which feeds the next prompt token
// while a row is still inside its prompt and samples afterwards; rows have prompts of different lengths
static int step_loop(skw_ctx* c, const FullRequest& rq, CallState& cs, const WindowBatch& w) {
    char* errbuf = c->errbuf; const int Bw = w.Bw; const SkwLogitParams& lp = cs.lp;
    const bool profiling = c->prof && c->prof->on, tracing = rq.tracing();
    // (f16_mfma, one group: eager launches 8 steps ahead measure the same 179 ms; the graph leaves the host idle, which matters with eight ranks on one node)
    const bool use_graphs = c->use_graphs >= 0 ? c->use_graphs != 0 : true;
    RowGroups rg = cut_row_groups(c, Bw); const int G = rg.G;
    cs.used_groups = G; cs.used_group_rows = rg.n[0];
    for (int j = 0; j < Bw; ++j) c->h_row_live[j] = 1;      // (every kernel of the previous window has drained: c->stream was synchronised at its end)
    HIPCHK(hipEventRecord(c->ev[5], c->stream));
    for (int g = 0; g < G; ++g) HIPCHK(hipStreamWaitEvent(c->gstream[g], c->ev[5], 0));
    hipGraphExec_t gexec[skw_ctx::MAX_GROUPS] = {};
    if (use_graphs && !profiling && !tracing) for (int g = 0; g < G; ++g) gexec[g] = step_graph(c, g, rg.r0[g], rg.n[g], lp, rq.mixed(), rq.constrained, rq.grammared);   // nullptr -> eager launches
    // The host learns whether a group still has live rows only by waiting for its stream, and a wait + relaunch per step leaves the
    // GPU idle for the turnaround.  So steps are enqueued `ahead` at a time and the count is read once per block: a step that
    // runs after the last row of its group has finished changes nothing (its attention and sampling kernels return at once for
    // finished rows; what the GEMMs write for them is scratch), it only costs its launches.
    const int step_cap = SKW_PROMPT_CAP + lp.n_max + 2;
    const int ahead = profiling ? 1 : 8;
    for (int i = 0; i < step_cap; i += ahead) {
        const int nstep = std::min(ahead, step_cap - i);
        for (int k = 0; k < nstep; ++k)
            for (int g = 0; g < G; ++g) if (rg.live[g]) {
                if (gexec[g]) HIPCHK(hipGraphLaunch(gexec[g], c->gstream[g]));
                else {
                    // (ahead == 1: the previous step has drained)
                    if (profiling) { int lv = 0; for (int j = rg.r0[g]; j < rg.r0[g] + rg.n[g]; ++j) lv += ((volatile int*)c->h_row_live)[j] != 0; c->live_rows_hint = lv; }
                    c->cur_group = g;
                    run_decoder_step(c, rg.r0[g], rg.n[g], i + k, true, c->gstream[g]); c->live_rows_hint = -1; c->cur_group = 0; sample_group(c, rq, lp, rg, g);
                }
            }
        bool any = false;
        for (int g = 0; g < G; ++g) if (rg.live[g]) { HIPCHK(hipStreamSynchronize(c->gstream[g]));
            int live = 0; for (int j = rg.r0[g]; j < rg.r0[g] + rg.n[g]; ++j) live += ((volatile int*)c->h_row_live)[j] != 0;
            if (live <= 0) rg.live[g] = false; else any = true; }
        if (!any) break;
    }
    for (int g = 0; g < G; ++g) { HIPCHK(hipEventRecord(c->gev[g], c->gstream[g])); HIPCHK(hipStreamWaitEvent(c->stream, c->gev[g], 0)); }
    return 0;
}

// The rows' state and tokens come back and the stream drains (the batch's host vectors may go after this); then per row the pass's verdict — this window again at the next
// temperature, or its output and the advance of seek (whisper_full_with_state's tail, skw_window_rules.h)
static int collect_window(skw_ctx* c, FullRequest& rq, CallState& cs, const WindowBatch& w) {
    char* errbuf = c->errbuf; const skw_model* m = c->m; const int Bw = w.Bw; const std::vector<int>& act = w.act;
    HIPCHK(hipMemcpyAsync(c->h_st, c->st, sizeof(SkwSeqState) * Bw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_toks, c->toks, sizeof(SkwTokenOut) * Bw * c->max_tok, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->ev[4], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (rq.tracing()) {
        std::vector<SkwTraceStep> tb((size_t)Bw * c->max_tok);
        HIPCHK(hipMemcpy(tb.data(), c->trace_dev, sizeof(SkwTraceStep) * tb.size(), hipMemcpyDeviceToHost));
        for (int j = 0; j < Bw; ++j) {
            const int ci = act[j], n = std::min(c->h_st[j].n_tokens, c->max_tok);
            if (rq.forced_ids && rq.forced_ids[ci] && cs.f_cursor[ci] + n > rq.n_forced[ci]) { snprintf(errbuf, 512,
                "clip %d: forced token sequence exhausted (%d given, decision %d reached): the runs' control flow diverged", ci, rq.n_forced[ci], cs.f_cursor[ci] + n);
            return -4; }
            rq.trace_steps[ci].insert(rq.trace_steps[ci].end(), tb.begin() + (size_t)j * c->max_tok, tb.begin() + (size_t)j * c->max_tok + n);
            cs.f_cursor[ci] += n;
        }
    }
    { float a = 0, b = 0; hipEventElapsedTime(&a, c->ev[2], c->ev[3]); hipEventElapsedTime(&b, c->ev[3], c->ev[4]); cs.enc_ms += a; cs.dec_ms += b; }
    cs.tot_windows += Bw;
    // decoder passes until the last row finished (the prompt pass counts as one); row-steps: (row, token) pairs that streamed cross K / V, prompt tokens included
    { int mx = 0; for (int j = 0; j < Bw; ++j) { const int rs = c->h_st[j].n_prompt - 1 + c->h_st[j].n_tokens;
    mx = std::max(mx, c->prompt_pass_on ? c->h_st[j].n_tokens : rs); cs.tot_row_steps += rs; } cs.tot_steps += mx + w.prefill_passes; }
    for (int j = 0; j < Bw; ++j) {
        const int ci = act[j]; const SkwSeqState& s = c->h_st[j]; const SkwTokenOut* tk = c->h_toks + (size_t)j * c->max_tok; skw_result& res = rq.results[ci];
        const skw_full_params& q = rq.P(ci);      // the clip's own request
        if (cs.tidx[ci] == 0) res.n_windows++;
        res.n_decode_steps += 1 + std::max(0, s.n_tokens - 1);     // the prompt is one decode call in whisper.cpp, then one per sampled token but the last
        const SkwVerdict v = skw_pass_verdict(s, tk, q.entropy_thold, q.logprob_thold, q.no_speech_thold);
        if (s.min_margin < res.min_margin) res.min_margin = s.min_margin;
        if (v.fallback) {
            res.fallback_requested++;
            // this window again, at the next temperature, on the cross K/V it already has (slot j)
            if (cs.tidx[ci] + 1 < (int)cs.temps[ci].size()) { cs.tidx[ci]++; cs.retry_slot[ci] = j; continue; }
        }
        cs.tidx[ci] = 0;
        skw_prompt_past_update(cs.prompt_past[ci], cs.last_take[ci], tk, s.result_len, v.no_speech);
        const int tok0 = (int)cs.acc[ci].tok.size(), seek0 = cs.seek[ci];
        cs.seek[ci] += skw_window_output(tk, v.n_tok, cs.seek[ci], s.seek_delta, cs.n_len_org[ci], m->tok_beg, m->tok_eot, q.single_segment, v.no_speech, m->tok_str.data(),
                                         cs.acc[ci]);
        if (rq.wants_align(ci)) {      // an accepted window that is speech: its text tokens (what the output step kept, below <|endoftext|>) are aligned by align_window
            CallState::AlignJob job{ci, j, seek0, w.ks[j], {}, {}};
            for (int k = tok0; k < (int)cs.acc[ci].tok.size(); ++k) if (cs.acc[ci].tok[k].id < m->tok_eot) { job.text.push_back(cs.acc[ci].tok[k].id); job.idx.push_back(k); }
            if (!job.text.empty()) cs.align_jobs.push_back(job);
        }
    }
    return 0;
}

// ---- word timestamps: the phase after collect_window (include/skw_align.h is the arithmetic; DESIGN.md section 3 "Word timestamps")
// The capture of one layer for one chunk: al_rows alignment rows x every head x n_audio_ctx keys, f32, cut to SKW_ALIGN_P_BYTES — but never below one sequence
// (SKW_ALIGN_MAX_ROWS rows) — whatever the batch size.  With it: f64 sums and f32 matrix per cell of the chunk, the sequences' records, jump / t0 / t1 per row.
#define SKW_ALIGN_P_BYTES ((size_t)128 << 20)
static int ensure_align_ws(skw_ctx* c) {
    if (c->al_P) return 0;
    char* errbuf = c->errbuf; const skw_hparams& hp = c->m->hp;
    const size_t per_row = (size_t)hp.n_text_head * hp.n_audio_ctx * sizeof(float);
    const int rows = (int)std::min<size_t>((size_t)c->rows_cap, std::max<size_t>(SKW_ALIGN_MAX_ROWS, SKW_ALIGN_P_BYTES / per_row));
    float* P = nullptr; double* acc = nullptr; float* x = nullptr; SkwAlignSeq* sq = nullptr; int* tm = nullptr;
    if (hipMalloc((void**)&P, per_row * rows) != hipSuccess || hipMalloc((void**)&acc, sizeof(double) * rows * hp.n_audio_ctx) != hipSuccess ||
        hipMalloc((void**)&x, sizeof(float) * rows * hp.n_audio_ctx) != hipSuccess || hipMalloc((void**)&sq, sizeof(SkwAlignSeq) * c->max_batch) != hipSuccess ||
        hipMalloc((void**)&tm, sizeof(int) * 3 * rows) != hipSuccess) {
        hipFree(P); hipFree(acc); hipFree(x); hipFree(sq); hipFree(tm); snprintf(errbuf, 512, "alignment workspace: device allocation failed"); return -1; }
    poison_floats(P, per_row * rows); poison_floats(acc, sizeof(double) * rows * hp.n_audio_ctx); poison_floats(x, sizeof(float) * rows * hp.n_audio_ctx);
    c->al_P = P; c->al_acc = acc; c->al_x = x; c->al_seqs = sq; c->al_times = tm; c->al_rows = rows;
    return 0;
}
// The windows collect_window accepted (cs.align_jobs: not retried, not no-speech, at least one text token, clip asked) get their token times: the teacher-forced sequence
// S = sot (, language, task), notimestamps, text — no [prev] context, from position 0 — runs as ONE prefill pass per chunk of whole sequences, exactly as prompt_pass chunks
// (whatever SKW_PROMPT_PASS says, no logits); the hook in run_decoder_step captures and reduces every alignment layer on the way; then the DTW.  The pass overwrites the
// slots' self-attention caches and the step's scratch, which the next window pass rebuilds from position 0 anyway; it only reads the slots' cross K.
// Jobs whose records differ (head mask, median width) run in passes of their own.
static int align_window(skw_ctx* c, const FullRequest& rq, CallState& cs) {
    char* errbuf = c->errbuf; skw_model* m = c->m; const skw_hparams& hp = m->hp; const int ntc = hp.n_text_ctx;
    std::vector<CallState::AlignJob> jobs; jobs.swap(cs.align_jobs);
    if (jobs.empty()) return 0;
    if (ensure_align_ws(c)) return -1;
    std::vector<bool> done(jobs.size(), false);
    for (size_t g0 = 0; g0 < jobs.size(); ++g0) {
        if (done[g0]) continue;
        const skw_align_params& ap = *rq.align[jobs[g0].ci];
        std::vector<size_t> grp;      // the jobs under the same record as job g0, in order
        for (size_t k = g0; k < jobs.size(); ++k) if (!done[k]) { const skw_align_params& bp = *rq.align[jobs[k].ci];
            if (bp.median_width == ap.median_width && memcmp(bp.head_mask, ap.head_mask, sizeof ap.head_mask) == 0) { grp.push_back(k); done[k] = true; } }
        int l_first = -1, l_last = -1; for (int l = 0; l < hp.n_text_layer; ++l) if (ap.head_mask[l]) { if (l_first < 0) l_first = l; l_last = l; }
        size_t at = 0;
        while (at < grp.size()) {
            // one chunk: whole sequences while the pass's rows fit the step's scratch, the alignment rows the capture, the sequences the records
            std::vector<SkwSeqState> pf; std::vector<SkwAlignSeq> sq; std::vector<int> meta((size_t)3 * c->max_batch, 0);
            int arows = 0, nq_max = 0, kw_max = 0, n_max = 0; long cells = 0; size_t hi = at;
            for (; hi < grp.size() && (int)sq.size() < c->max_batch; ++hi) {
                const CallState::AlignJob& jb = jobs[grp[hi]];
                int32_t S[8 + SKW_ALIGN_MAX_ROWS]; skw_full_params q = rq.P(jb.ci); q.no_timestamps = 1;
                int np = prompt_tail(m, q, cs.lang[jb.ci], S);
                const int T = (int)jb.text.size(), N = T + 1, rows = np + T;
                if (N > SKW_ALIGN_MAX_ROWS || rows > ntc || rows > c->rows_cap || N > c->al_rows) {
                    snprintf(errbuf, 512, "clip %d: a window of %d text tokens cannot be aligned", jb.ci, T); return -1; }
                if (hi > at && ((int)pf.size() + rows > c->rows_cap || arows + N > c->al_rows)) break;
                for (int k = 0; k < T; ++k) S[np + k] = jb.text[k];
                SkwAlignSeq a; memset(&a, 0, sizeof a);
                a.qrow0 = (int)pf.size() + np - 1; a.n = N; a.slot = jb.slot; a.n_keys = jb.n_keys; a.kw = skw_align_kw(cs.n_len_org[jb.ci], jb.seek, jb.n_keys); a.prow0 = arows;
                a.seek_cs = jb.seek; a.xoff = cells;
                meta[sq.size()] = (int)pf.size(); meta[c->max_batch + sq.size()] = rows; meta[2 * c->max_batch + sq.size()] = jb.slot;
                for (int k = 0; k < rows; ++k) { SkwSeqState t; memset(&t, 0, sizeof t);
                    t.active = 1; t.cur_token = S[k]; t.cur_pos = k; t.pad = jb.slot; t.seek = jb.slot * ntc + k; t.n_keys = jb.n_keys; pf.push_back(t); }
                sq.push_back(a); arows += N; cells += (long)N * a.kw; nq_max = std::max(nq_max, rows); kw_max = std::max(kw_max, a.kw); n_max = std::max(n_max, N);
            }
            const int n = (int)pf.size(), ns = (int)sq.size();
            HIPCHK(hipMemcpyAsync(c->pf_st, pf.data(), sizeof(SkwSeqState) * n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->pf_meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->al_seqs, sq.data(), sizeof(SkwAlignSeq) * ns, hipMemcpyHostToDevice, c->stream));
            c->pf_nseq = ns; c->pf_nq_max = nq_max;
            c->al_on = true; c->al_mask = ap.head_mask; c->al_width = ap.median_width; c->al_nseq = ns; c->al_h_seqs = sq.data(); c->al_tap_base = c->al_tap_next;
             c->al_rows_now = arows; c->al_kw_max = kw_max;
            c->al_n_heads = skw_align_n_heads(ap.head_mask); c->al_l_first = l_first; c->al_l_last = l_last;
            run_decoder_step(c, 0, n, 0, false, c->stream, true);
            c->al_on = false; c->al_mask = nullptr; c->pf_nseq = 0;
            if (g_taps_on) {      // per sequence: its matrix, which clip and window it is, and which of the clip's result tokens its rows time
                char name[40];
                for (int i = 0; i < ns; ++i) { const CallState::AlignJob& jb = jobs[grp[at + i]]; const int sn = c->al_tap_base + i;
                    snprintf(name, sizeof name, "align_x_s%d", sn); tap(c, name, c->al_x + sq[i].xoff, sq[i].n, sq[i].kw, TAP_F32);
                    snprintf(name, sizeof name, "align_seq_s%d", sn);
                    g_taps[name] = {(float)jb.ci, (float)jb.seek, (float)jb.n_keys, (float)sq[i].kw, (float)sq[i].n, (float)jb.slot, (float)cs.n_len_org[jb.ci]};
                    snprintf(name, sizeof name, "align_idx_s%d", sn); std::vector<float>& o = g_taps[name]; o.clear(); for (int ix : jb.idx) o.push_back((float)ix); }
                g_taps["align_n"] = {(float)(c->al_tap_base + ns)};
            }
            c->al_tap_next += ns; c->al_h_seqs = nullptr;
            int *jump = c->al_times, *t0 = c->al_times + c->al_rows, *t1 = c->al_times + 2 * c->al_rows;
            { ProfScope p_(c, PC_ALIGN_DTW, 0, 0);
              if (!skw_align_dtw(c->al_x, c->al_seqs, ns, n_max, kw_max, jump, t0, t1, c->stream)) { snprintf(errbuf, 512, "alignment: the DTW launcher refused %d rows x %d keys", n_max, kw_max);
                                                                                                   return -1; } }
            std::vector<int> h0(arows), h1(arows);
            HIPCHK(hipMemcpyAsync(h0.data(), t0, sizeof(int) * arows, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(h1.data(), t1, sizeof(int) * arows, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));      // (the chunk's host vectors are sources of the copies above, and pf_st / al_seqs are reused by the next chunk)
            for (int i = 0; i < ns; ++i) { const CallState::AlignJob& jb = jobs[grp[at + i]];
                std::vector<int64_t>& a0 = cs.tt0[jb.ci]; std::vector<int64_t>& a1 = cs.tt1[jb.ci];
                for (size_t k = 0; k < jb.idx.size(); ++k) { const size_t ix = (size_t)jb.idx[k]; if (a0.size() <= ix) { a0.resize(ix + 1, -1); a1.resize(ix + 1, -1); }
                    a0[ix] = h0[sq[i].prow0 + k]; a1[ix] = h1[sq[i].prow0 + k]; } }
            at = hi;
        }
    }
    return 0;
}

// generator states and contexts go back to their owners, the clips' accumulators become the results, the call's timing
static int finish_call(skw_ctx* c, const FullRequest& rq, CallState& cs) {
    char* errbuf = c->errbuf; const int n_clips = rq.n_clips; int tot_tokens = 0;
    HIPCHK(hipEventRecord(c->ev[5], c->stream));
    if (rq.rng_state) for (int i = 0; i < n_clips; ++i) if (rq.rng_state[i])
        HIPCHK(hipMemcpyAsync(rq.rng_state[i], c->rng + (size_t)i * SKW_RNG_WORDS, sizeof(uint32_t) * SKW_RNG_WORDS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());          // a launch that failed (bad configuration, lost device) must not look like a transcript
    if (rq.context) for (int i = 0; i < n_clips; ++i) if (rq.context[i]) skw_context_write(cs.prompt_past[i], SKW_CONTEXT_WORDS - 1, rq.context[i]);
    for (int i = 0; i < n_clips; ++i) {
        skw_result& res = rq.results[i]; SeqAcc& A = cs.acc[i];
        res.n_segments = (int)A.seg.size(); res.n_tokens = (int)A.tok.size(); res.text_len = (int)A.text.size();
        res.segments = (skw_segment*)malloc(sizeof(skw_segment) * std::max<size_t>(1, A.seg.size())); memcpy(res.segments, A.seg.data(), sizeof(skw_segment) * A.seg.size());
        res.tokens = (skw_token*)malloc(sizeof(skw_token) * std::max<size_t>(1, A.tok.size())); memcpy(res.tokens, A.tok.data(), sizeof(skw_token) * A.tok.size());
        res.text = (char*)malloc(A.text.size() + 1); memcpy(res.text, A.text.data(), A.text.size()); res.text[A.text.size()] = 0;
        tot_tokens += res.n_tokens;
    }
    if (rq.times) for (int i = 0; i < n_clips; ++i) {      // per result token (skw_align_batch: per given text token); -1 where no time was computed
        const size_t nt = rq.text_tokens ? (size_t)rq.n_text[i] : cs.acc[i].tok.size();
        cs.tt0[i].resize(nt, -1); cs.tt1[i].resize(nt, -1);
        skw_token_times& tt = rq.times[i]; tt.n = (int32_t)nt;
        tt.t0 = (int64_t*)malloc(sizeof(int64_t) * std::max<size_t>(1, nt)); tt.t1 = (int64_t*)malloc(sizeof(int64_t) * std::max<size_t>(1, nt));
        memcpy(tt.t0, cs.tt0[i].data(), sizeof(int64_t) * nt); memcpy(tt.t1, cs.tt1[i].data(), sizeof(int64_t) * nt);
    }
    if (rq.traces) for (int i = 0; i < n_clips; ++i) {      // every sampling decision of the clip, in execution order
        const std::vector<SkwTraceStep>& tr = rq.trace_steps[i];
        rq.traces[i].n = (int32_t)tr.size(); rq.traces[i].steps = (skw_trace_step*)malloc(sizeof(skw_trace_step) * std::max<size_t>(1, tr.size()));
        memcpy(rq.traces[i].steps, tr.data(), sizeof(skw_trace_step) * tr.size());
    }
    prof_collect(c);
    { float a = 0, t = 0; hipEventElapsedTime(&a, c->ev[0], c->ev[1]); hipEventElapsedTime(&t, c->ev[0], c->ev[5]);
      c->timing.mel_ms = a; c->timing.encode_ms = cs.enc_ms; c->timing.decode_ms = cs.dec_ms;
      c->timing.total_ms = t; c->timing.n_windows = cs.tot_windows; c->timing.n_decode_steps = cs.tot_steps;
      c->timing.n_tokens = tot_tokens; c->timing.n_row_steps = (int32_t)cs.tot_row_steps; c->timing.decode_groups = cs.used_groups; c->timing.decode_group_rows = cs.used_group_rows; }
    return 0;
}

// ---- grammars on the device (skw_full_batch_grammar, the debug hook)
// the text tokens' bytes, once per context: offsets [tok_eot + 1] and the bytes behind them in one allocation
static int grammar_vocab_ensure(skw_ctx* c) {
    if (c->gr_voc_off) return 0;
    char* errbuf = c->errbuf; const skw_model* m = c->m; const int n = m->tok_eot;
    std::vector<int32_t> off((size_t)n + 1, 0); std::vector<uint8_t> bytes;
    for (int t = 0; t < n; ++t) { const std::string& tx = m->tok_str[t]; bytes.insert(bytes.end(), tx.begin(), tx.end()); off[t + 1] = (int32_t)bytes.size(); }
    const size_t ob = sizeof(int32_t) * off.size(); void* p = nullptr;
    if (hipMalloc(&p, ob + std::max<size_t>(1, bytes.size())) != hipSuccess || !p) { snprintf(errbuf, 512, "grammar: the vocabulary image could not be allocated"); return -1; }
    c->gr_voc_off = (int32_t*)p; c->gr_voc_bytes = (uint8_t*)p + ob;
    HIPCHK(hipMemcpy(c->gr_voc_off, off.data(), ob, hipMemcpyHostToDevice));
    if (!bytes.empty()) HIPCHK(hipMemcpy(c->gr_voc_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    ++c->gr_uploads;
    return 0;
}
// gr_clip[i] = clip i's record (checked already; NULL: none).  Equal tables are one upload — within the call and, through the cache, across calls
static int grammar_upload(skw_ctx* c, const skw_grammar* const* gv, int n) {
    char* errbuf = c->errbuf; static const size_t CACHE_MAX = 8;
    if (grammar_vocab_ensure(c)) return -1;
    const long call = ++c->gr_stamp;
    c->gr_clip.assign(n, SkwRowGrammar{nullptr, nullptr, 0.0f, 0, 0, 0u});
    for (int i = 0; i < n; ++i) {
        const skw_grammar* g = gv[i]; if (!g) continue;
        // (the same tables handed in for several clips — one node instance's segments, a caller's shared grammar — are recognised by address before anything is hashed)
        int same = -1; for (int k = 0; k < i && same < 0; ++k) if (gv[k] && gv[k]->next == g->next && gv[k]->accept == g->accept && gv[k]->n_states == g->n_states) same = k;
        if (same >= 0) { c->gr_clip[i] = c->gr_clip[same]; c->gr_clip[i].penalty = g->penalty; continue; }
        const size_t nn = (size_t)g->n_states * 256; uint64_t h = 1469598103934665603ull;      // FNV-1a over the tables
        for (size_t k = 0; k < nn; ++k) { h = (h ^ g->next[k]) * 1099511628211ull; }
        for (int k = 0; k < g->n_states; ++k) { h = (h ^ g->accept[k]) * 1099511628211ull; }
        skw_ctx::GrammarImage* hit = nullptr;
        for (auto& gi : c->gr_cache) if (gi.hash == h && gi.n_states == g->n_states && memcmp(gi.next.data(), g->next, nn * 2) == 0 && memcmp(gi.accept.data(), g->accept, g->n_states) == 0) {
            hit = &gi; break; }
        if (!hit) {
            // room: the least recently used table that no clip of this call holds goes first
            while (c->gr_cache.size() >= CACHE_MAX) {
                size_t old = c->gr_cache.size();
                for (size_t k = 0; k < c->gr_cache.size(); ++k) if (c->gr_cache[k].stamp != call && (old == c->gr_cache.size() || c->gr_cache[k].stamp < c->gr_cache[old].stamp)) old = k;
                if (old == c->gr_cache.size()) break;      // (every cached table is in use by this call: the cache grows for its duration)
                HIPCHK(hipStreamSynchronize(c->stream)); hipFree(c->gr_cache[old].d_next); c->gr_cache.erase(c->gr_cache.begin() + old);
            }
            void* p = nullptr;
            if (hipMalloc(&p, nn * 2 + g->n_states) != hipSuccess || !p) { snprintf(errbuf, 512, "clip %d: grammar: the table could not be allocated on the device", i); return -1; }
            skw_ctx::GrammarImage gi; gi.hash = h; gi.n_states = g->n_states; gi.next.assign(g->next, g->next + nn); gi.accept.assign(g->accept, g->accept + g->n_states);
            gi.d_next = (uint16_t*)p; gi.d_accept = (uint8_t*)p + nn * 2; gi.stamp = call;
            if (hipMemcpy(gi.d_next, g->next, nn * 2, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(gi.d_accept, g->accept, g->n_states, hipMemcpyHostToDevice) != hipSuccess) {
                hipFree(p); snprintf(errbuf, 512, "clip %d: grammar: the table could not be copied to the device", i); return -1; }
            ++c->gr_uploads; c->gr_cache.push_back(std::move(gi)); hit = &c->gr_cache.back();
        }
        hit->stamp = call;
        c->gr_clip[i] = SkwRowGrammar{hit->d_next, hit->d_accept, g->penalty, g->n_states, 0, 0u};
    }
    return 0;
}

static int full_batch_impl(skw_ctx* c, FullRequest& rq) {
    char* errbuf = c->errbuf; errbuf[0] = 0;
    WS_READY(c);
    if (int rc = validate_request(c, rq)) return rc;
    HIPCHK(hipSetDevice(c->m->device));
    if (rq.tracing() && ensure_trace_buffers(c)) return -1;
    if (rq.grammared) if (int rc = grammar_upload(c, rq.grammar, rq.n_clips)) return rc;
    CallState cs(rq.n_clips); c->al_tap_next = 0;
    if (int rc = load_call(c, rq, cs)) return rc;
    if (int rc = detect_languages(c, rq, cs)) return rc;
    cs.lp = rq.mixed() ? mixed_logit_params(c->m) : make_logit_params(c->m, rq.params);
    while (true) {
        WindowBatch w;      // (alive until collect_window has synchronised the stream)
        if (!plan_window(rq, cs, w)) break;
        if (int rc = stage_window(c, rq, cs, w)) return rc;
        if (rq.text_tokens) {      // skw_align_batch: the encoder has run on the clips' one window; the given text stands where a decoded window's would
            HIPCHK(hipStreamSynchronize(c->stream));
            for (int j = 0; j < w.Bw; ++j) { const int ci = w.act[j]; CallState::AlignJob job{ci, j, 0, w.ks[j], {}, {}};
                for (int k = 0; k < rq.n_text[ci]; ++k) { job.text.push_back(rq.text_tokens[ci][k]); job.idx.push_back(k); }
                cs.align_jobs.push_back(job); }
            if (int rc = align_window(c, rq, cs)) return rc;
            break;
        }
        if (int rc = prompt_pass(c, w)) return rc;
        if (int rc = step_loop(c, rq, cs, w)) return rc;
        if (int rc = collect_window(c, rq, cs, w)) return rc;
        if (rq.aligned) if (int rc = align_window(c, rq, cs)) return rc;
    }
    return finish_call(c, rq, cs);
}

// the entry points' guard: nothing may unwind across the C ABI
template <typename F> static int guarded(skw_ctx* c, const char* entry, F&& body) {
    try { return body(); }
    catch (const std::exception& e) { snprintf(c->errbuf, 512, "%s: %s", entry, e.what()); return -5; }
}
// The one function behind every entry point; entry: the caller's name, for the guard's message.  times[i] and traces[i] are zeroed first: they are defined after a failed call.
// Forced alignment decodes nothing: a caller without results gets the phases' bookkeeping on scratch ones, freed with the call.
static int full_batch_call(skw_ctx* c, const char* entry, const skw_full_request& q) {
    static_assert(sizeof(skw_trace_step) == sizeof(SkwTraceStep), "skw_trace_step is SkwTraceStep");
    return guarded(c, entry, [&] {
        FullRequest rq(q);
        if (rq.times) for (int i = 0; i < rq.n_clips; ++i) { rq.times[i].n = 0; rq.times[i].t0 = rq.times[i].t1 = nullptr; }
        if (rq.traces) { for (int i = 0; i < rq.n_clips; ++i) { rq.traces[i].n = 0; rq.traces[i].steps = nullptr; } rq.trace_steps.resize(std::max(0, rq.n_clips)); }
        std::vector<skw_result> scratch;
        if (rq.text_tokens && !rq.results) { scratch.resize(std::max(1, rq.n_clips)); memset((void*)scratch.data(), 0, sizeof(skw_result) * scratch.size()); rq.results = scratch.data(); }
        const int rc = full_batch_impl(c, rq);
        for (skw_result& r : scratch) skw_result_free(&r);
        return rc; });
}

extern "C" int skw_full_batch_request(skw_ctx* c, const skw_full_request* in) {
    skw_full_request q; memset(&q, 0, sizeof q);
    if (!in || in->size < SKW_FULL_REQUEST_MIN || in->size > sizeof q) {
        snprintf(c->errbuf, 512, "skw_full_batch_request: size %u outside [%d, %zu] (sizeof(skw_full_request) as the caller compiled it)", in ? in->size : 0u, SKW_FULL_REQUEST_MIN, sizeof q);
        return -1; }
    memcpy(&q, in, std::min<size_t>(in->size, sizeof q));
    if (!q.params || (!q.results && !q.text_tokens)) { snprintf(c->errbuf, 512, "skw_full_batch_request: params and results must be given (results may be NULL with text_tokens)"); return -1; }
    return full_batch_call(c, "skw_full_batch_request", q);
}
// ---- the entry points of before the request: each is its own argument check and the fields it sets
static skw_full_request request_of(int per_clip, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device, skw_result* results) {
    skw_full_request q; memset(&q, 0, sizeof q);
    q.size = sizeof q; q.params_per_clip = per_clip; q.params = params; q.pcm = pcm; q.n_samples = n_samples; q.n_clips = n_clips; q.pcm_on_device = pcm_on_device; q.results = results;
    return q;
}
static bool params_given(skw_ctx* c, const char* entry, const skw_full_params* params) {
    if (!params) snprintf(c->errbuf, 512, "%s: params is NULL (one skw_full_params per clip)", entry);
    return params != nullptr;
}
extern "C" int skw_full_batch(skw_ctx* c, const skw_full_params* p, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device, skw_result* results) {
    return full_batch_call(c, "skw_full_batch", request_of(0, p, pcm, n_samples, n_clips, pcm_on_device, results));
}
extern "C" void skw_rng_state_init(uint32_t* state) {      // std::mt19937(0), as whisper_init_state leaves decoder 0's generator
    state[0] = 0u; for (int i = 1; i < 624; ++i) state[i] = 1812433253u * (state[i - 1] ^ (state[i - 1] >> 30)) + (uint32_t)i;
    state[624] = 624u;
}
extern "C" int skw_full_batch_rng(skw_ctx* c, const skw_full_params* p, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                  uint32_t* const* rng_state, skw_result* results) {
    skw_full_request q = request_of(0, p, pcm, n_samples, n_clips, pcm_on_device, results); q.rng_state = rng_state;
    return full_batch_call(c, "skw_full_batch_rng", q);
}
extern "C" int skw_full_batch_mixed(skw_ctx* c, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                    uint32_t* const* rng_state, skw_result* results) {
    if (!params_given(c, "skw_full_batch_mixed", params)) return -1;
    skw_full_request q = request_of(1, params, pcm, n_samples, n_clips, pcm_on_device, results); q.rng_state = rng_state;
    return full_batch_call(c, "skw_full_batch_mixed", q);
}
extern "C" int skw_full_batch_context(skw_ctx* c, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                      uint32_t* const* rng_state, int32_t* const* context, skw_result* results) {
    if (!params_given(c, "skw_full_batch_context", params)) return -1;
    skw_full_request q = request_of(1, params, pcm, n_samples, n_clips, pcm_on_device, results); q.rng_state = rng_state; q.context = context;
    return full_batch_call(c, "skw_full_batch_context", q);
}
extern "C" void skw_decode_rules_default(skw_decode_rules* r) { skw_decode_rules_set_default(r); }
extern "C" int skw_full_batch_rules(skw_ctx* c, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                    uint32_t* const* rng_state, int32_t* const* context, const skw_decode_rules* const* rules, skw_result* results) {
    if (!params_given(c, "skw_full_batch_rules", params)) return -1;
    skw_full_request q = request_of(1, params, pcm, n_samples, n_clips, pcm_on_device, results); q.rng_state = rng_state; q.context = context; q.rules = rules;
    return full_batch_call(c, "skw_full_batch_rules", q);
}
extern "C" int skw_full_batch_aligned(skw_ctx* c, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                      uint32_t* const* rng_state, int32_t* const* context, const skw_decode_rules* const* rules, const skw_align_params* const* align,
                                      skw_token_times* times, skw_result* results) {
    if (!params_given(c, "skw_full_batch_aligned", params)) return -1;
    skw_full_request q = request_of(1, params, pcm, n_samples, n_clips, pcm_on_device, results); q.rng_state = rng_state; q.context = context; q.rules = rules;
    q.align = align; q.times = times;
    return full_batch_call(c, "skw_full_batch_aligned", q);
}
extern "C" int skw_full_batch_grammar(skw_ctx* c, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                      uint32_t* const* rng_state, int32_t* const* context, const skw_decode_rules* const* rules, const skw_align_params* const* align,
                                      skw_token_times* times, const skw_grammar* const* grammar, skw_result* results) {
    if (!params_given(c, "skw_full_batch_grammar", params)) return -1;
    skw_full_request q = request_of(1, params, pcm, n_samples, n_clips, pcm_on_device, results); q.rng_state = rng_state; q.context = context; q.rules = rules;
    q.align = align; q.times = times; q.grammar = grammar;
    return full_batch_call(c, "skw_full_batch_grammar", q);
}
extern "C" int skw_grammar_compile(const char* pattern, size_t len, int flags, float penalty, skw_grammar** out, char* err, size_t errlen) {
    return skw_grammar_compile_impl(pattern, len, flags, penalty, out, err, errlen);
}
extern "C" void skw_grammar_free(skw_grammar* g) { skw_grammar_free_impl(g); }
extern "C" long skw_debug_grammar_uploads(const skw_ctx* c) { return c->gr_uploads; }      // tests: device allocations made for grammars so far (the vocabulary image, then one per cache miss)
extern "C" int skw_align_batch(skw_ctx* c, const skw_full_params* params, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                               const int32_t* const* text_tokens, const int32_t* n_text, const skw_align_params* const* align, skw_token_times* times) {
    if (!params || !text_tokens || !n_text || !align || !times) { snprintf(c->errbuf, 512, "skw_align_batch: params, text_tokens, n_text, align and times must all be given"); return -1; }
    skw_full_request q = request_of(1, params, pcm, n_samples, n_clips, pcm_on_device, nullptr); q.align = align; q.times = times; q.text_tokens = text_tokens; q.n_text = n_text;
    return full_batch_call(c, "skw_align_batch", q);
}
extern "C" void skw_token_times_free(skw_token_times* t) { if (!t) return; free(t->t0); free(t->t1); t->t0 = t->t1 = nullptr; t->n = 0; }
extern "C" int skw_full_batch_traced_context(skw_ctx* c, const skw_full_params* p, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                             const int32_t* const* forced_ids, const int32_t* n_forced, skw_trace* traces, int32_t* const* context, skw_result* results) {
    if (!traces || (forced_ids && !n_forced)) { snprintf(c->errbuf, 512, "skw_full_batch_traced: bad arguments"); return -1; }
    skw_full_request q = request_of(0, p, pcm, n_samples, n_clips, pcm_on_device, results); q.forced_ids = forced_ids; q.n_forced = n_forced; q.traces = traces; q.context = context;
    return full_batch_call(c, "skw_full_batch_traced", q);      // (both traced entry points report under this name)
}
extern "C" int skw_full_batch_traced(skw_ctx* c, const skw_full_params* p, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                     const int32_t* const* forced_ids, const int32_t* n_forced, skw_trace* traces, skw_result* results) {
    return skw_full_batch_traced_context(c, p, pcm, n_samples, n_clips, pcm_on_device, forced_ids, n_forced, traces, nullptr, results);
}
extern "C" void skw_trace_free(skw_trace* t) { if (!t) return; free(t->steps); t->steps = nullptr; t->n = 0; }
extern "C" void skw_result_free(skw_result* r) { if (!r) return; free(r->segments); free(r->tokens); free(r->text); memset(r, 0, sizeof *r); }

// ================================================================== test and measurement hooks that drive the engine's own phases
// (the hooks that run one kernel on caller-supplied operands are skw_hooks.hip's)
// ------------------------------------------------------------------ debug taps (encoder layer 0, natural layouts; enabled by skw_debug_enable)
// tests: f16_mfma cross K / V^T as fragment-order images (one-pass cross attention) / as rows (two-phase kernel); takes effect at the next encoder pass
extern "C" void skw_debug_set_kv_frag(skw_ctx* c, int on) { c->kv_frag_on = on != 0; }
extern "C" void skw_debug_set_prompt_pass(skw_ctx* c, int on) { c->prompt_pass_on = on != 0; }     // tests: the prompt as one pass / one token per step
// tests / tools: the exact precision's prompt pass with the multi-query cross attention (default) or the single-query kernel on every prompt row
extern "C" void skw_debug_set_prompt_xattn_mq(skw_ctx* c, int on) { c->prompt_xattn_mq_on = on != 0; }
extern "C" void skw_debug_set_ln_stats(skw_ctx* c, int on) { c->ln_stats_on = on != 0; }      // tests: the decode step with / without the LayerNorm launches (f16_mfma)
extern "C" void skw_debug_enable(int on) { g_taps_on = on != 0; g_taps.clear(); }
extern "C" long skw_debug_get(const char* name, float* out, size_t cap) {
    auto it = g_taps.find(name); if (it == g_taps.end()) return -1; if (out && cap >= it->second.size()) memcpy(out, it->second.data(), it->second.size() * 4); return (long)it->second.size();
}
static void tap(skw_ctx* c, const char* name, const void* dev, int rows, int cols, TapLayout lay) {
    if (!g_taps_on) return;
    hipStreamSynchronize(c->stream);
    std::vector<float>& o = g_taps[name]; o.assign((size_t)rows * cols, 0.f);
    const int H = c->m->hp.n_audio_head, Tpad = c->Tpad;
    if (lay == TAP_F32) { hipMemcpy(o.data(), dev, o.size() * 4, hipMemcpyDeviceToHost); return; }
    if (lay == TAP_F16_PLAIN) {      // f16 rows in natural order; the tap holds the BIT PATTERNS as floats (exact: every value is below 2^16)
        std::vector<uint16_t> h((size_t)rows * cols); hipMemcpy(h.data(), dev, h.size() * 2, hipMemcpyDeviceToHost);
        for (size_t i = 0; i < h.size(); ++i) o[i] = (float)h[i];
        return;
    }
    if (lay == TAP_F16_KPERM) {
        std::vector<uint16_t> h((size_t)rows * cols); hipMemcpy(h.data(), dev, h.size() * 2, hipMemcpyDeviceToHost);
        for (int r = 0; r < rows; ++r) for (int i = 0; i < cols; ++i) o[(size_t)r * cols + i] = skw_f16_to_f32(h[(size_t)r * cols + skw_kperm(i)]);
    } else if (lay == TAP_HEADS) {   // [(h)*Tpad + i][kperm(d)] for batch 0
        std::vector<uint16_t> h((size_t)H * Tpad * 64); hipMemcpy(h.data(), dev, h.size() * 2, hipMemcpyDeviceToHost);
        for (int r = 0; r < rows; ++r) for (int n = 0; n < cols; ++n) o[(size_t)r * cols + n] = skw_f16_to_f32(h[((size_t)(n >> 6) * Tpad + r) * 64 + skw_kperm(n & 63)]);
    } else {                          // V^T: [(h*64 + c)][kperm(key)] row stride Tpad
        std::vector<uint16_t> h((size_t)H * 64 * Tpad); hipMemcpy(h.data(), dev, h.size() * 2, hipMemcpyDeviceToHost);
        for (int r = 0; r < rows; ++r) for (int n = 0; n < cols; ++n) o[(size_t)r * cols + n] = skw_f16_to_f32(h[((size_t)n) * Tpad + skw_kperm(r)]);
    }
}

// Test hook (tests/test_gpu_logit_rules.py): K11 on its own.  n_rows decoders whose tokens sampled so far in their window are hist[r][0 .. n_hist[r]) meet
// caller-supplied logits; ONE launch of the sampler (form 0: the one the decode step uses; form 1: the streaming kernel, which leaves the filtered row in
// memory) makes each row's next decision.  has_ts / seek_delta / result_len are replayed from the history by the token loop's update rule, as
// oracle/skwo_debug_process_logits does.  Outputs per row: the decision (skw_token), its trace record, and (form 1, optional) the filtered logits.
// params_per_row (skw_debug_sample_rows_mixed): one skw_full_params per row — the launch is the per-row form of the sampler, each row under its own rules and its own static mask.
// rules (skw_debug_sample_rows_rules): one skw_decode_rules (or NULL) per row — k_dec_constrain runs on the rows' logits ahead of the sampler, as in the decode step.
// the fields skw_debug_sample_rows_ex fills (from its skw_sample_rows_ex): per-row temperatures and generator states, the launch with or without the trace buffers, and what
// else the sampler leaves behind:
//  temperature [n_rows] (null: 0 everywhere) — lp.any_sampled is 1 iff some row's is > 0; rng_state [n_rows][625], in and out (null: every row on generator 0, untouched
//  memory of the context): row r draws from generator r (clip_idx[r] = r), an index above 624 is refused like skw_full_batch_rng's; trace = 0: forced = trace = nullptr
//  reach the launcher (k_dec_sample<false, any_sampled, ROWS>), trace_out is left alone; probs_out [n_rows][n_vocab]: the f32 probabilities of rows at a temperature > 0
//  (other rows' entries are left alone); no_speech_prob / n_tokens / cur_token / active_out [n_rows]: the row's state after the launch; kernel_id: SKW_SMPK_* bits of the
//  kernel the launcher picked (skw_dec_sample_kernel, the function it branches on).
struct skw_sample_rows_ex { const float* temperature; uint32_t* rng_state; int32_t trace; int32_t kernel_id; float* probs_out; float* no_speech_prob;
                            int32_t* n_tokens; int32_t* cur_token; int32_t* active; };
// The hook behind all of them (skw_sample_rows_request, include/skw_engine.h); entry: the caller's name, for the guard's message
static int sample_rows_impl(skw_ctx* c, const char* entry, skw_sample_rows_request& q) {
  return guarded(c, entry, [&] {
    char* errbuf = c->errbuf; errbuf[0] = 0;
    const skw_full_params* p = q.params; const skw_full_params* pv = q.params_per_row ? q.params : nullptr; const int n_rows = q.n_rows, hist_stride = q.hist_stride, form = q.form;
    const int32_t* hist = q.hist; const int32_t* n_hist = q.n_hist; const skw_decode_rules* const* rv = q.rules; const skw_grammar* const* gv = q.grammar;
    const bool want_state = q.no_speech_prob || q.n_tokens || q.cur_token || q.active_out;
    WS_READY(c);
    if (n_rows < 1 || n_rows > c->max_batch) { snprintf(errbuf, 512, "n_rows %d outside [1, %d]", n_rows, c->max_batch); return -1; }
    if ((rv || gv) && (q.temperature || q.rng_state || !q.trace || q.probs_out || want_state)) {      // (what no hook offers)
        snprintf(errbuf, 512, "rules and grammar go with the plain launch only: no temperature, rng_state, trace = 0, probs_out or row state"); return -3; }
    if (q.rng_state) for (int r = 0; r < n_rows; ++r) if (q.rng_state[(size_t)r * SKW_RNG_WORDS + 624] > 624u) {
        snprintf(errbuf, 512, "row %d: the generator state handed in is not a std::mt19937 state (index %u)", r, q.rng_state[(size_t)r * SKW_RNG_WORDS + 624]); return -1; }
    if (q.temperature && !q.rng_state) for (int r = 0; r < n_rows; ++r) if (q.temperature[r] > 0.0f) {
        snprintf(errbuf, 512, "row %d: a temperature > 0 needs rng_state (one generator per row)", r); return -1; }
    const bool with_trace = q.trace != 0;
    HIPCHK(hipSetDevice(c->m->device));
    const skw_model* m = c->m; const int NV = m->hp.n_vocab, MT = c->max_tok;
    for (int r = 0; r < n_rows; ++r) if (n_hist[r] < 0 || n_hist[r] >= MT || n_hist[r] > hist_stride) { snprintf(errbuf, 512, "row %d: history of %d tokens (at most %d)", r, n_hist[r], MT - 1);
    return -1; }
    if (ensure_trace_buffers(c)) return -1;
    SkwLogitParams lp; std::vector<SkwRowRules> rules; std::vector<SkwRowConstraints> cons;
    if (rv) {
        for (int r = 0; r < n_rows; ++r) { char who[32]; snprintf(who, sizeof who, "row %d", r); if (!skw_decode_rules_check(rv[r], NV, who, errbuf, 512)) return -3; }
        cons.resize(n_rows); for (int r = 0; r < n_rows; ++r) cons[r] = make_row_constraints(rv[r]);
        HIPCHK(hipMemcpyAsync(c->row_cons, cons.data(), sizeof(SkwRowConstraints) * n_rows, hipMemcpyHostToDevice, c->stream));
    }
    if (gv) {
        for (int r = 0; r < n_rows; ++r) { char who[32]; snprintf(who, sizeof who, "row %d", r); if (!skw_grammar_check(gv[r], who, errbuf, 512)) return -3; }
        if (int rc = grammar_upload(c, gv, n_rows)) return rc;
        HIPCHK(hipMemcpyAsync(c->row_gram, c->gr_clip.data(), sizeof(SkwRowGrammar) * n_rows, hipMemcpyHostToDevice, c->stream));
    }
    if (pv) {
        build_static_mask_pair(c); lp = mixed_logit_params(m);
        rules.resize(n_rows); for (int r = 0; r < n_rows; ++r) rules[r] = make_row_rules(m, &pv[r]);
        HIPCHK(hipMemcpyAsync(c->row_rules, rules.data(), sizeof(SkwRowRules) * n_rows, hipMemcpyHostToDevice, c->stream));
    } else { build_static_mask(c, p); lp = make_logit_params(m, p); }
    lp.any_sampled = 0;
    if (q.temperature) for (int r = 0; r < n_rows; ++r) if (q.temperature[r] > 0.0f) lp.any_sampled = 1;
    std::vector<SkwTokenOut> toks((size_t)n_rows * MT); memset(toks.data(), 0, toks.size() * sizeof(SkwTokenOut));
    std::vector<int> forced((size_t)n_rows * MT, -1), zero(n_rows, 0);
    if (q.rng_state) for (int r = 0; r < n_rows; ++r) zero[r] = r;      // (row r on generator r)
    for (int r = 0; r < n_rows; ++r) {
        SkwSeqState& s = c->h_st[r]; memset(&s, 0, sizeof s);
        s.active = 1; s.seek_delta = SKW_WINDOW_FRAMES; s.seek = 0; s.n_prompt = 1; s.min_margin = INFINITY;
        s.cur_pos = n_hist[r]; s.n_tokens = n_hist[r];
        if (q.temperature) s.temperature = q.temperature[r];
        // the history's timestamps through the token loop's update (as the parent of this hook, oracle/skwo_debug_process_logits, replays them): how has_ts / seek_delta /
        // result_len follow them, and the one failure a history can show.  No stop rule can fire: no budget, no loop bound, the audio without end, and <|endoftext|> is no timestamp
        s.seek_end = INT32_MAX;
        for (int i = 0; i < n_hist[r]; ++i) {
            const int id = hist[(size_t)r * hist_stride + i]; toks[(size_t)r * MT + i].id = id;
            if (id > m->tok_beg && skw_token_loop_update(s, id, i, m->tok_beg, m->tok_eot, 0, 0, 0, INT32_MAX)) {
                snprintf(errbuf, 512, "row %d: the token loop cannot produce this history (timestamp goes backwards at %d)", r, i); return -1; }
        }
        s.seek_end = SKW_WINDOW_FRAMES;
        if (q.active && !q.active[r]) s.active = 0;
        c->h_row_live[r] = 1;
    }
    HIPCHK(hipMemcpyAsync(c->st, c->h_st, sizeof(SkwSeqState) * n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->toks, toks.data(), sizeof(SkwTokenOut) * toks.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->forced_dev, forced.data(), sizeof(int) * forced.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->clip_idx, zero.data(), sizeof(int) * n_rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->logits, q.logits, sizeof(float) * (size_t)n_rows * NV, hipMemcpyHostToDevice, c->stream));
    if (q.rng_state) HIPCHK(hipMemcpyAsync(c->rng, q.rng_state, sizeof(uint32_t) * SKW_RNG_WORDS * n_rows, hipMemcpyHostToDevice, c->stream));
    const int* forced_dev = with_trace ? c->forced_dev : nullptr; SkwTraceStep* trace_dev = with_trace ? c->trace_dev : nullptr;
    if (rv) skw_dec_constrain(c->logits, NV, lp.tok_eot, c->row_cons, c->st, c->toks, MT, n_rows, c->stream);
    if (gv) skw_dec_grammar(c->logits, NV, lp.tok_eot, c->row_gram, c->st, c->toks, MT, n_rows, c->gr_voc_off, c->gr_voc_bytes, c->stream);
    skw_debug_force_stream_sampler(form == 1);
    q.kernel_id = skw_dec_sample_kernel(lp, trace_dev != nullptr, pv != nullptr);
    if (pv) skw_dec_sample_rows(c->logits, c->static_mask_pair, lp, c->row_rules, c->st, c->toks, MT, n_rows, c->d_row_live, c->probs, c->rng, c->clip_idx, c->prompt_buf, c->stream,
                                forced_dev, trace_dev);
    else skw_dec_sample(c->logits, c->static_mask, lp, c->st, c->toks, MT, n_rows, c->d_row_live, c->probs, c->rng, c->clip_idx, c->prompt_buf, c->stream, forced_dev, trace_dev);
    skw_debug_force_stream_sampler(0);
    HIPCHK(hipGetLastError());
    std::vector<SkwTraceStep> tr((size_t)n_rows * MT);
    HIPCHK(hipMemcpyAsync(toks.data(), c->toks, sizeof(SkwTokenOut) * toks.size(), hipMemcpyDeviceToHost, c->stream));
    if (with_trace) HIPCHK(hipMemcpyAsync(tr.data(), c->trace_dev, sizeof(SkwTraceStep) * tr.size(), hipMemcpyDeviceToHost, c->stream));
    if (q.filtered_out) HIPCHK(hipMemcpyAsync(q.filtered_out, c->logits, sizeof(float) * (size_t)n_rows * NV, hipMemcpyDeviceToHost, c->stream));
    std::vector<SkwSeqState> st_after(want_state ? n_rows : 0);
    if (want_state) HIPCHK(hipMemcpyAsync(st_after.data(), c->st, sizeof(SkwSeqState) * n_rows, hipMemcpyDeviceToHost, c->stream));
    if (q.rng_state) HIPCHK(hipMemcpyAsync(q.rng_state, c->rng, sizeof(uint32_t) * SKW_RNG_WORDS * n_rows, hipMemcpyDeviceToHost, c->stream));
    if (q.probs_out && q.temperature) for (int r = 0; r < n_rows; ++r) if (q.temperature[r] > 0.0f)
        HIPCHK(hipMemcpyAsync(q.probs_out + (size_t)r * NV, c->probs + (size_t)r * skw_probs_row_floats(NV), sizeof(float) * NV, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int r = 0; r < n_rows; ++r) {
        const SkwTokenOut& t = toks[(size_t)r * MT + n_hist[r]];
        if (q.tok_out) { skw_token o; o.id = t.id; o.tid = t.tid; o.p = t.p; o.plog = t.plog; o.pt = t.pt; o.ptsum = t.ptsum; o.margin = t.margin; q.tok_out[r] = o; }
        if (q.trace_out && with_trace) memcpy(&q.trace_out[r], &tr[(size_t)r * MT + n_hist[r]], sizeof(skw_trace_step));
        if (q.no_speech_prob) q.no_speech_prob[r] = st_after[r].no_speech_prob;
        if (q.n_tokens) q.n_tokens[r] = st_after[r].n_tokens;
        if (q.cur_token) q.cur_token[r] = st_after[r].cur_token;
        if (q.active_out) q.active_out[r] = st_after[r].active;
    }
    return 0; });
}
extern "C" int skw_debug_sample_rows_request(skw_ctx* c, skw_sample_rows_request* q) {
    if (!q || !q->params) { snprintf(c->errbuf, 512, "skw_debug_sample_rows_request: the request and its params are required"); return -1; }
    return sample_rows_impl(c, "skw_debug_sample_rows_request", *q);
}
static skw_sample_rows_request sample_rows_of(int per_row, const skw_full_params* p, int n_rows, const int32_t* hist, int hist_stride, const int32_t* n_hist, const float* logits_host, int form,
                                              float* filtered_out, skw_token* tok_out, skw_trace_step* trace_out) {
    skw_sample_rows_request q; memset(&q, 0, sizeof q);
    q.params_per_row = per_row; q.params = p; q.n_rows = n_rows; q.hist = hist; q.hist_stride = hist_stride; q.n_hist = n_hist; q.logits = logits_host; q.form = form;
    q.filtered_out = filtered_out; q.tok_out = tok_out; q.trace_out = trace_out; q.trace = 1;
    return q;
}
extern "C" int skw_debug_sample_rows(skw_ctx* c, const skw_full_params* p, int n_rows, const int32_t* hist, int hist_stride, const int32_t* n_hist, const float* logits_host, int form,
                                     float* filtered_out, skw_token* tok_out, skw_trace_step* trace_out) {
    skw_sample_rows_request q = sample_rows_of(0, p, n_rows, hist, hist_stride, n_hist, logits_host, form, filtered_out, tok_out, trace_out);
    return sample_rows_impl(c, "skw_debug_sample_rows", q);
}
extern "C" int skw_debug_sample_rows_mixed(skw_ctx* c, const skw_full_params* params /* [n_rows] */, int n_rows, const int32_t* hist, int hist_stride, const int32_t* n_hist,
                                           const float* logits_host, int form, float* filtered_out, skw_token* tok_out, skw_trace_step* trace_out) {
    if (!params) { snprintf(c->errbuf, 512, "skw_debug_sample_rows_mixed: params is NULL (one skw_full_params per row)"); return -1; }
    skw_sample_rows_request q = sample_rows_of(1, params, n_rows, hist, hist_stride, n_hist, logits_host, form, filtered_out, tok_out, trace_out);
    return sample_rows_impl(c, "skw_debug_sample_rows_mixed", q);
}
extern "C" int skw_debug_sample_rows_rules(skw_ctx* c, const skw_full_params* params /* [n_rows] */, int n_rows, const int32_t* hist, int hist_stride, const int32_t* n_hist,
                                           const float* logits_host, int form, float* filtered_out, skw_token* tok_out, skw_trace_step* trace_out,
                                           const skw_decode_rules* const* rules /* [n_rows], entries may be NULL */) {
    if (!params || !rules) { snprintf(c->errbuf, 512, "skw_debug_sample_rows_rules: params and rules are one per row (rules entries may be NULL)"); return -1; }
    skw_sample_rows_request q = sample_rows_of(1, params, n_rows, hist, hist_stride, n_hist, logits_host, form, filtered_out, tok_out, trace_out); q.rules = rules;
    return sample_rows_impl(c, "skw_debug_sample_rows_rules", q);
}
// constrain -> grammar -> sampler, as in the decode step: rules as above (NULL: no row has a record), grammar one skw_grammar (or NULL) per row.  active [n_rows] (or NULL):
// 0 marks a row as finished before the launch — every kernel leaves it alone
extern "C" int skw_debug_sample_rows_grammar(skw_ctx* c, const skw_full_params* params /* [n_rows] */, int n_rows, const int32_t* hist, int hist_stride, const int32_t* n_hist,
                                             const float* logits_host, int form, float* filtered_out, skw_token* tok_out, skw_trace_step* trace_out,
                                             const skw_decode_rules* const* rules, const skw_grammar* const* grammar, const int32_t* active) {
    if (!params || !grammar) { snprintf(c->errbuf, 512, "skw_debug_sample_rows_grammar: params and grammar are one per row (grammar entries may be NULL)"); return -1; }
    skw_sample_rows_request q = sample_rows_of(1, params, n_rows, hist, hist_stride, n_hist, logits_host, form, filtered_out, tok_out, trace_out);
    q.rules = rules; q.grammar = grammar; q.active = active;
    return sample_rows_impl(c, "skw_debug_sample_rows_grammar", q);
}
// per_row: p is one skw_full_params per row (the per-row form of the sampler, as skw_debug_sample_rows_mixed), else one block for the launch
extern "C" int skw_debug_sample_rows_ex(skw_ctx* c, const skw_full_params* p, int per_row, int n_rows, const int32_t* hist, int hist_stride, const int32_t* n_hist,
                                        const float* logits_host, int form, float* filtered_out, skw_token* tok_out, skw_trace_step* trace_out, skw_sample_rows_ex* ex) {
    if (!p || !ex) { snprintf(c->errbuf, 512, "skw_debug_sample_rows_ex: params and ex are required"); return -1; }
    skw_sample_rows_request q = sample_rows_of(per_row != 0, p, n_rows, hist, hist_stride, n_hist, logits_host, form, filtered_out, tok_out, trace_out);
    q.temperature = ex->temperature; q.rng_state = ex->rng_state; q.trace = ex->trace; q.probs_out = ex->probs_out; q.no_speech_prob = ex->no_speech_prob; q.n_tokens = ex->n_tokens;
    q.cur_token = ex->cur_token; q.active_out = ex->active;
    const int rc = sample_rows_impl(c, "skw_debug_sample_rows_ex", q);
    if (rc == 0) ex->kernel_id = q.kernel_id;
    return rc;
}

// ------------------------------------------------------------------ stage taps
__global__ void k_transpose_mel(const float* mel, int n_len, int n_mel, float* out) {   // [frame][mel] -> [mel][frame]
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x; if (i >= (long)n_len * n_mel) return; int fr = (int)(i / n_mel), j = (int)(i % n_mel); out[(long)j * n_len + fr] = mel[i];
}
extern "C" int skw_log_mel(skw_ctx* c, const float* pcm_host, int n_samples, float* mel_out, size_t cap, int* n_len_o, int* n_len_org_o) {
    char* errbuf = c->errbuf;
    WS_READY(c);
    HIPCHK(hipSetDevice(c->m->device));
    std::vector<int> n_len, n_len_org; const float* pp[1] = {pcm_host}; int32_t ns[1] = {n_samples};
    if (load_clips(c, pp, ns, 1, 0, n_len, n_len_org)) return -1;
    run_mel(c, 1);
    const size_t n = (size_t)n_len[0] * c->m->hp.n_mels;
    if (cap < n) { snprintf(errbuf, 512, "mel_out too small: need %zu floats", n); return -1; }
    float* tmp = nullptr; HIPCHK(hipMalloc((void**)&tmp, n * sizeof(float)));
    hipLaunchKernelGGL(k_transpose_mel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->mel, n_len[0], c->m->hp.n_mels, tmp);
    HIPCHK(hipMemcpyAsync(mel_out, tmp, n * sizeof(float), hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); hipFree(tmp);
    *n_len_o = n_len[0]; *n_len_org_o = n_len_org[0]; return 0;
}
// audio_ctx: 0 = the model's n_audio_ctx; the tap's one window slot gets that many positions (returned through *K)
static int tap_prepare(skw_ctx* c, const float* pcm_host, int n_samples, int seek, int audio_ctx, int* K) {
    char* errbuf = c->errbuf;
    WS_READY(c);
    if (audio_ctx < 0 || audio_ctx > c->m->hp.n_audio_ctx) { snprintf(errbuf, 512, "audio_ctx %d outside [0, %d] (0 = the model's n_audio_ctx)", audio_ctx, c->m->hp.n_audio_ctx); return -1; }
    *K = audio_ctx > 0 ? audio_ctx : c->m->hp.n_audio_ctx;
    HIPCHK(hipSetDevice(c->m->device));
    std::vector<int> n_len, n_len_org; const float* pp[1] = {pcm_host}; int32_t ns[1] = {n_samples};
    if (load_clips(c, pp, ns, 1, 0, n_len, n_len_org)) return -1;
    run_mel(c, 1);
    int zero = 0; HIPCHK(hipMemcpyAsync(c->clip_idx, &zero, sizeof(int), hipMemcpyHostToDevice, c->stream)); HIPCHK(hipMemcpyAsync(c->seek, &seek, sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int rows = set_slot_k(c, K, 1, 0, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    run_conv(c, 1, 0, rows); return 0;
}
extern "C" int skw_conv_stem_actx(skw_ctx* c, const float* pcm_host, int n_samples, int seek, int audio_ctx, float* x0) {
    char* errbuf = c->errbuf; int K = 0; if (tap_prepare(c, pcm_host, n_samples, seek, audio_ctx, &K)) return -1;
    HIPCHK(hipMemcpyAsync(x0, c->x, sizeof(float) * K * c->m->hp.n_audio_state, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return 0;
}
extern "C" int skw_conv_stem(skw_ctx* c, const float* pcm_host, int n_samples, int seek, float* x0) { return skw_conv_stem_actx(c, pcm_host, n_samples, seek, 0, x0); }
// cross V^T [(h*64 + c)][Tpad kperm] of batch slot 0 -> natural [key][d] f32
__global__ void k_vt2f_copy(const half_t* src, float* dst, int nc, int dt, int Tpad) { long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
if (i >= (long)nc * dt) return; int key = (int)(i / dt), n = (int)(i % dt); dst[i] = (float)src[(long)n * Tpad + skw_kperm(key)]; }
// the same exports from the fragment-order images
__global__ void k_kfrag2f_copy(const half_t* src, float* dst, int nc, int dt, int H, int Tpad) { long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
if (i >= (long)nc * dt) return; int key = (int)(i / dt), n = (int)(i % dt); dst[i] = (float)src[skw_kfrag_off(0, H, Tpad, key, n & ~7) + (n & 7)]; }
__global__ void k_vtfrag2f_copy(const half_t* src, float* dst, int nc, int dt, int H, int Tpad) { long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
if (i >= (long)nc * dt) return; int key = (int)(i / dt), n = (int)(i % dt);
const int p = skw_kperm(key); dst[i] = (float)src[skw_vtfrag_off(0, H, Tpad, n, p & ~7) + (p & 7)]; }
__global__ void k_h2f_copy(const half_t* src, float* dst, long n) { long i = (long)blockIdx.x * blockDim.x + threadIdx.x; if (i < n) dst[i] = (float)src[i]; }
extern "C" int skw_encode(skw_ctx* c, const float* pcm_host, int n_samples, int seek, float* enc_out, float* cross_k, float* cross_v) {
    return skw_encode_actx(c, pcm_host, n_samples, seek, 0, enc_out, cross_k, cross_v);
}
extern "C" int skw_encode_actx(skw_ctx* c, const float* pcm_host, int n_samples, int seek, int audio_ctx, float* enc_out, float* cross_k, float* cross_v) {
    char* errbuf = c->errbuf; int K = 0; if (tap_prepare(c, pcm_host, n_samples, seek, audio_ctx, &K)) return -1;
    const skw_hparams& hp = c->m->hp; const int nc = K, d = hp.n_audio_state, dt = hp.n_text_state;      // (nc: the K positions exported)
    run_encoder(c, 1, true, true, 0, c->enc_rows);
    HIPCHK(hipMemcpyAsync(enc_out, c->enc_out32, sizeof(float) * nc * d, hipMemcpyDeviceToHost, c->stream));
    if (cross_k && cross_v) {
        const long n = (long)nc * dt; float* tmp = nullptr; HIPCHK(hipMalloc((void**)&tmp, n * sizeof(float)));
        for (int l = 0; l < hp.n_text_layer; ++l) for (int kv = 0; kv < 2; ++kv) {
            const half_t* vsrc = c->crossV + (size_t)l * c->max_batch * hp.n_text_head * 64 * c->Tpad; const half_t* ksrc = c->crossK + (size_t)l * c->max_batch * c->kclip();
            if (kv && c->kv_frag()) hipLaunchKernelGGL(k_vtfrag2f_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, vsrc, tmp, nc, dt, hp.n_text_head, c->Tpad);
            else if (kv) hipLaunchKernelGGL(k_vt2f_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, vsrc, tmp, nc, dt, c->Tpad);
            else if (c->kv_frag()) hipLaunchKernelGGL(k_kfrag2f_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, ksrc, tmp, nc, dt, hp.n_text_head, c->Tpad);
            else hipLaunchKernelGGL(k_h2f_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, ksrc, tmp, n);
            HIPCHK(hipMemcpyAsync((kv ? cross_v : cross_k) + (size_t)l * n, tmp, n * sizeof(float), hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
        }
        hipFree(tmp);
    }
    HIPCHK(hipStreamSynchronize(c->stream)); return 0;
}
extern "C" int skw_decode_logits(skw_ctx* c, const int32_t* tokens, int n_tokens, float* logits) {
    char* errbuf = c->errbuf;
    WS_READY(c);
    HIPCHK(hipSetDevice(c->m->device));
    if (n_tokens < 1 || n_tokens > c->m->hp.n_text_ctx) { snprintf(errbuf, 512, "bad n_tokens"); return -1; }
    for (int t = 0; t < n_tokens; ++t) {
        hipLaunchKernelGGL(k_set_tokens, dim3(1), dim3(1), 0, c->stream, c->st, tokens[t], t, c->slot_k);      // (slot 0's K: the last encode's)
        run_decoder_step(c, 0, 1, t, t == n_tokens - 1, c->stream);
    }
    HIPCHK(hipMemcpyAsync(logits, c->logits, sizeof(float) * c->m->hp.n_vocab, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return 0;
}

// a clip's alignment record checked the way the entry points will check it (include/skw_align.h): 0 good; -1 bad, skw_ctx_last_error names the clip.  Needs no device.
extern "C" int skw_align_params_check(skw_ctx* c, const skw_align_params* p, int clip) {
    return skw_align_check_params(p, c->m->hp.n_text_layer, c->m->hp.n_text_head, clip, c->errbuf, 512) ? 0 : -1;
}

// the launch clock's records (SkwKClk, skw_kernels.h): one clock per (row group, decoder layer) graph node
static const int KCLK_CAP = 1024;                                      // launches recorded per node and call (a 30 s window is <= 466 steps)
static size_t kclk_node_bytes() { return sizeof(SkwKClk) + sizeof(SkwKClkRec) * SKW_KCLK_SHARDS * (KCLK_CAP - 1); }
// one launch's record: the maxima over its shards; false when no live workgroup stamped it
static bool kclk_launch(const SkwKClk* k, int j, unsigned long long* t0, unsigned long long* t1, unsigned* live) {
    unsigned long long a = 0, b = 0; unsigned l = 0;
    for (int s = 0; s < SKW_KCLK_SHARDS; ++s) { const SkwKClkRec& r = k->rec[j][s]; a = std::max(a, r.t0_inv); b = std::max(b, r.t1); l += r.live_rows; }
    if (!a || !b) return false;
    *t0 = ~a; *t1 = b; *live = l; return true;
}
static SkwKClk* kclk_node(const skw_ctx* c, int g, int l) {
    return c->kclk_on ? (SkwKClk*)((char*)c->kclk + kclk_node_bytes() * ((size_t)g * c->m->hp.n_text_layer + l)) : nullptr;
}
static int kclk_reset(skw_ctx* c) {
    char* errbuf = c->errbuf;
    const size_t nb = kclk_node_bytes(), n_nodes = (size_t)skw_ctx::MAX_GROUPS * c->m->hp.n_text_layer;
    HIPCHK(hipMemsetAsync(c->kclk, 0, nb * n_nodes, c->stream));
    static const unsigned hdr[4] = {(unsigned)KCLK_CAP, 0, 0, 0};
    for (size_t i = 0; i < n_nodes; ++i) HIPCHK(hipMemcpyAsync((char*)c->kclk + nb * i, hdr, 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
// Arms / disarms the in-kernel launch clock of the decode step's cross attention (f16_mfma, fragment-order images).  Armed, the step graphs are captured with the clock's
// pointers (their key carries the flag) and every skw_full_batch starts from zeroed records; skw_ctx_kernel_clock_get sums what the last call recorded.
extern "C" int skw_ctx_kernel_clock(skw_ctx* c, int on) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    if (on && !c->kclk) {
        HIPCHK(hipMalloc((void**)&c->kclk, kclk_node_bytes() * skw_ctx::MAX_GROUPS * c->m->hp.n_text_layer));
        int khz = 0; HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->m->device));
        if (khz <= 0) { snprintf(errbuf, 512, "device reports no wall clock rate"); return -1; }
        c->kclk_khz = khz;
    }
    c->kclk_on = on ? 1 : 0;
    return on ? kclk_reset(c) : 0;
}
// launches recorded by the last skw_full_batch: count, summed first-wave-in -> last-wave-out microseconds, summed live rows (the launch's algorithmic bytes are
// 4 B x live rows x n_audio_ctx x n_text_state), shortest and longest launch
extern "C" int skw_ctx_kernel_clock_get(skw_ctx* c, long* launches, double* sum_us, double* sum_live_rows, double* min_us, double* max_us, int* clock_khz) {
    char* errbuf = c->errbuf;
    if (!c->kclk) { snprintf(errbuf, 512, "the kernel clock was never armed"); return -1; }
    HIPCHK(hipSetDevice(c->m->device));
    const size_t nb = kclk_node_bytes(), n_nodes = (size_t)skw_ctx::MAX_GROUPS * c->m->hp.n_text_layer;
    std::vector<char> h(nb * n_nodes);
    HIPCHK(hipMemcpy(h.data(), c->kclk, h.size(), hipMemcpyDeviceToHost));
    long n = 0; double su = 0, sl = 0, mn = 1e30, mx = 0;
    for (size_t i = 0; i < n_nodes; ++i) {
        const SkwKClk* k = (const SkwKClk*)(h.data() + nb * i);
        for (int j = 0; j < KCLK_CAP; ++j) {
            unsigned long long t0, t1; unsigned live;
            if (!kclk_launch(k, j, &t0, &t1, &live)) continue;
            const double us = (double)(t1 - t0) * 1000.0 / c->kclk_khz;
            ++n; su += us; sl += live; mn = std::min(mn, us); mx = std::max(mx, us);
        }
    }
    *launches = n; *sum_us = su; *sum_live_rows = sl; *min_us = n ? mn : 0; *max_us = mx; *clock_khz = c->kclk_khz;
    return 0;
}

// the keys the recorded launches walked, summed over their live rows (per-clip audio context: a launch's algorithmic bytes = 4 B x its rows' walked keys x n_text_state)
extern "C" int skw_ctx_kernel_clock_keys(skw_ctx* c, double* sum_keys) {
    char* errbuf = c->errbuf;
    if (!c->kclk) { snprintf(errbuf, 512, "the kernel clock was never armed"); return -1; }
    HIPCHK(hipSetDevice(c->m->device));
    const size_t nb = kclk_node_bytes(), n_nodes = (size_t)skw_ctx::MAX_GROUPS * c->m->hp.n_text_layer;
    std::vector<char> h(nb * n_nodes);
    HIPCHK(hipMemcpy(h.data(), c->kclk, h.size(), hipMemcpyDeviceToHost));
    double sk = 0;
    for (size_t i = 0; i < n_nodes; ++i) { const SkwKClk* k = (const SkwKClk*)(h.data() + nb * i);
        for (int j = 0; j < KCLK_CAP; ++j) for (int sh = 0; sh < SKW_KCLK_SHARDS; ++sh) sk += k->rec[j][sh].keys; }
    *sum_keys = sk;
    return 0;
}
// every recorded launch of the last call as (begin us, end us, live rows), times relative to the earliest begin; returns the count written (<= cap), < 0 on error.  Launches of
// different row groups overlap in time: the union of the intervals is the time the kernel was in flight at all.
extern "C" long skw_ctx_kernel_clock_records(skw_ctx* c, double* out /* [cap][3] */, long cap) {
    char* errbuf = c->errbuf;
    if (!c->kclk) { snprintf(errbuf, 512, "the kernel clock was never armed"); return -1; }
    HIPCHK(hipSetDevice(c->m->device));
    const size_t nb = kclk_node_bytes(), n_nodes = (size_t)skw_ctx::MAX_GROUPS * c->m->hp.n_text_layer;
    std::vector<char> h(nb * n_nodes);
    HIPCHK(hipMemcpy(h.data(), c->kclk, h.size(), hipMemcpyDeviceToHost));
    unsigned long long t_min = ~0ull;
    unsigned long long t0, t1; unsigned live;
    for (size_t i = 0; i < n_nodes; ++i) { const SkwKClk* k = (const SkwKClk*)(h.data() + nb * i);
        for (int j = 0; j < KCLK_CAP; ++j) if (kclk_launch(k, j, &t0, &t1, &live)) t_min = std::min(t_min, t0); }
    long n = 0;
    for (size_t i = 0; i < n_nodes; ++i) { const SkwKClk* k = (const SkwKClk*)(h.data() + nb * i);
        for (int j = 0; j < KCLK_CAP && n < cap; ++j) { if (!kclk_launch(k, j, &t0, &t1, &live)) continue;
            out[3 * n] = (double)(t0 - t_min) * 1000.0 / c->kclk_khz; out[3 * n + 1] = (double)(t1 - t_min) * 1000.0 / c->kclk_khz; out[3 * n + 2] = live; ++n; } }
    return n;
}

// The decode step's cross attention alone, B rows, launched back to back over `layers` different K / V^T images (so no launch re-reads what a previous one left in a cache).
// Every launch is stamped twice: by HIP events at the kernel's own begin and end (hipExtLaunchKernelGGL: what rocprofv3 reports as the duration) and — the one-pass kernel — by its
// in-kernel clock (first wave in to last wave out).  us_per_launch: the event average; us_per_launch_clock (may be null): the clock's average, 0 where the kernel has no clock.
extern "C" int skw_debug_xattn(skw_ctx* c, int B, int layers, int probe, int iters, float* us_per_launch, float* us_per_launch_clock) {
    char* errbuf = c->errbuf; HIPCHK(hipSetDevice(c->m->device));
    if (probe) { snprintf(errbuf, 512, "skw_debug_xattn: the parts-off probe launches were removed with round 5's pruning (results: profiles/r02f, r03b)"); return -1; }
    const skw_hparams& hp = c->m->hp; const int d = hp.n_text_state, H = hp.n_text_head, nc = hp.n_audio_ctx, Tpad = c->Tpad;
    const size_t kn = (size_t)B * Tpad * d, vn = (size_t)B * H * 64 * Tpad;
    half_t *K = nullptr, *V = nullptr, *q = nullptr, *out = nullptr; SkwKClk* clk = nullptr;
    iters = std::max(1, std::min(iters, KCLK_CAP));
    HIPCHK(hipMalloc((void**)&K, kn * 2 * layers)); HIPCHK(hipMalloc((void**)&V, vn * 2 * layers));
    HIPCHK(hipMalloc((void**)&q, (size_t)B * d * 2)); HIPCHK(hipMalloc((void**)&out, (size_t)B * d * 4));
    HIPCHK(hipMalloc((void**)&clk, kclk_node_bytes()));
    { std::vector<uint16_t> h(std::max(kn, vn)); uint32_t x = 777; for (auto& v : h) { x = x * 1664525u + 1013904223u; v = skw_f32_to_f16((((x >> 8) & 0xffff) / 65536.0f - 0.5f) * 0.25f); }
      for (int l = 0; l < layers; ++l) { HIPCHK(hipMemcpy(K + kn * l, h.data(), kn * 2, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(V + vn * l, h.data(), vn * 2, hipMemcpyHostToDevice)); }
      HIPCHK(hipMemcpy(q, h.data(), (size_t)B * d * 2, hipMemcpyHostToDevice)); }
    const int pv16 = c->kv_frag() ? 2 : c->precision == SKW_PRECISION_F16_MFMA;       // (timing only: the images are random bytes in either layout; Tpad * d elements per slot are allocated above)
    for (int i = 0; i < layers; ++i) skw_dec_cross_attn_vt(q, K + kn * (i % layers), V + vn * (i % layers), B, H, d, nc, Tpad, out, nullptr, c->stream, 0, pv16);
    HIPCHK(hipMemsetAsync(clk, 0, kclk_node_bytes(), c->stream));
    { static const unsigned hdr[4] = {(unsigned)KCLK_CAP, 0, 0, 0}; HIPCHK(hipMemcpyAsync(clk, hdr, 16, hipMemcpyHostToDevice, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); }
    float ms = 0;
    std::vector<hipEvent_t> ev(2 * (size_t)iters);
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    for (int i = 0; i < iters; ++i)
        skw_dec_cross_attn_vt(q, K + kn * (i % layers), V + vn * (i % layers), B, H, d, nc, Tpad, out, nullptr, c->stream, 0, pv16, nullptr, ev[2 * i], ev[2 * i + 1], 0, pv16 == 2 ? clk : nullptr);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < iters; ++i) { float t = 0; if (hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) ms += t; }
    for (auto& e : ev) hipEventDestroy(e);
    *us_per_launch = 1000.0f * ms / iters;
    if (us_per_launch_clock) {
        *us_per_launch_clock = 0.0f;
        if (pv16 == 2) {
            int khz = 0; HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->m->device));
            std::vector<char> h(kclk_node_bytes()); HIPCHK(hipMemcpy(h.data(), clk, h.size(), hipMemcpyDeviceToHost));
            const SkwKClk* k = (const SkwKClk*)h.data(); double su = 0; int n = 0; unsigned long long t0, t1; unsigned live;
            for (int j = 0; j < iters; ++j) if (kclk_launch(k, j, &t0, &t1, &live)) { su += (double)(t1 - t0) * 1000.0 / std::max(1, khz); ++n; }
            if (n) *us_per_launch_clock = (float)(su / n);
        }
    }
    hipFree(K); hipFree(V); hipFree(q); hipFree(out); hipFree(clk);
    return 0;
}

