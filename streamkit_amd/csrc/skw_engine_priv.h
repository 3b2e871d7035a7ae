// skw_engine_priv.h — what the translation units of libskw_engine.so share behind the C ABI (skw_engine.hip, skw_model.hip, skw_hooks.hip, skw_dsp.hip): the model and
// context structs, the error helpers, and the few functions that cross a file.  Nothing here is exported: the cross-file functions are hidden from the dynamic symbol table.
#pragma once
#include "../../include/skw_engine.h"
#include "../../include/skw_math.h"
#include "../../include/skw_ggml_quant.h"
#include "skw_kernels.h"
#include "skw_tokenizer.h"
#include "skw_decode_rules.h"
#include "skw_grammar_compile.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define SKW_HIDDEN __attribute__((visibility("hidden")))
#define WHISPER_SAMPLE_RATE 16000
#define WHISPER_N_FFT 400
#define WHISPER_HOP 160
#define WHISPER_CHUNK_SIZE 30

static void set_err(char* err, size_t n, const char* fmt, ...) {
    if (!err || !n) return;
    va_list ap; va_start(ap, fmt); vsnprintf(err, n, fmt, ap); va_end(ap);
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(errbuf, 512, "HIP error '%s' at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

struct DevLin { half_t* w = nullptr; float* b = nullptr; int n_out = 0, n_in = 0, k_pad = 0;
                half_t* w_nat = nullptr;   // the same weight with the contraction axis in natural order (decoder projections fed by a LayerNorm: skw_gemm16_small_lnA)
                half_t* w_frag = nullptr; half_t* w_nat_frag = nullptr;   // fragment-order images of w / w_nat for the f16 decode kernels (SkwGemmArgs::Wf; decoder layers only)
                // ggml's arithmetic for a block-quantised weight (skw_kernels_q8.hip): int8 [n_out][n_in], scales / offsets [n_in / 32][n_pad]; null for f16 weights
                int8_t* qw = nullptr; float* dwT = nullptr; float* mwT = nullptr; int n_pad = 0, qform = 0; };
struct HostQ { std::vector<int8_t> q; std::vector<float> d, m; int n_out = 0, K = 0; };      // a quantised weight in the common integer form, host side
struct DevLN { float* w = nullptr; float* b = nullptr; };
struct EncLayer { DevLN attn_ln, mlp_ln; DevLin q, k, v, o, fc1, fc2; };
struct DecLayer { DevLN attn_ln, cross_ln, mlp_ln; DevLin q, k, v, o, cq, ck, cv, co, fc1, fc2; DevLin qkv; /* q|k|v rows concatenated for the fused decode projection */ };

struct skw_model {
    skw_hparams hp{};
    int device = 0;
    std::vector<std::string> tok_str;
    SkwTokenizer tokz;      // text -> ids (skw_model_tokenize): the entries below <|endoftext|>
    int tok_eot, tok_sot, tok_translate, tok_transcribe, tok_solm, tok_prev, tok_nosp, tok_not, tok_beg;
    int tok_space = -1, tok_sp_dash = -1, tok_sp_quote = -1; std::vector<int> nst_ids; int n_lang = 99;
    // device
    float *filters = nullptr, *hann = nullptr, *sin_t = nullptr, *cos_t = nullptr; int n_fft_bins = 201; int *mel_grp_lo = nullptr, *mel_grp_hi = nullptr;
    uint16_t* gelu_tab = nullptr;
    float* e_pe = nullptr; DevLin conv1, conv2; DevLN ln_post; std::vector<EncLayer> enc;
    float* d_pe = nullptr; DevLin te; DevLN d_ln; std::vector<DecLayer> dec;
    int quant = 0;             // ggml type of the matmul weights when the file is uniformly block-quantised and ggml's q8 arithmetic is available (exact precision runs it)
    float* te32 = nullptr;     // quant: the token embedding dequantised to f32 [n_vocab][d] (get_rows does not round to f16)
    std::vector<void*> allocs;
};

struct ProfState;
struct skw_ctx {
    int precision = SKW_PRECISION_EXACT;             // SKW_PRECISION_*: which form of the contractions runs (skw_ctx_set_precision)
    int kv_frag_on = 1;                              // f16_mfma: cross K / V^T as fragment-order images (skw_kernels.h, skw_kfrag_off); SKW_XATTN_FRAG=0 keeps the row layouts
    bool kv_frag() const { return kv_frag_on && precision == SKW_PRECISION_F16_MFMA; }
    // cross_kv = q8_0 (skw_ctx_set_cross_kv; include/skw_kv8.h): the single-query cross attention of the f16_mfma precision reads the q8 image the encoder pass leaves beside the
    // f16 fragment-order images.  Effective only with those images (kv8()): the exact precision owes the oracle its bits and ignores the flag.  kv8_fresh: the image holds the
    // slots of the last encoder pass (false after a pass that ran without the flag) — what the decode step asks, so a flag flipped between an encode and a step changes nothing.
    int cross_kv = SKW_CROSS_KV_F16; uint8_t* crossKV8 = nullptr; bool kv8_fresh = false;
    bool kv8() const { return cross_kv == SKW_CROSS_KV_Q8_0 && kv_frag() && crossKV8; }
    bool kv8_step() const { return kv8() && kv8_fresh; }
    size_t kv8_slot() const { return (size_t)skw_kv8_slot_bytes(m->hp.n_text_head, Tpad); }
    size_t kclip() const { return (size_t)(kv_frag() ? Tpad : m->hp.n_audio_ctx) * m->hp.n_text_state; }      // cross-K elements per window slot (the buffer is sized for the larger: Tpad rows)
    ProfState* prof = nullptr;                       // per-kernel-class event timing (skw_ctx_profile); per context: contexts run on different host threads
    skw_model* m = nullptr; int max_batch = 0, max_samples = 0, n_len_max = 0, Tpad = 0;
    hipStream_t stream = nullptr; hipEvent_t ev[6] = {};
    hipStream_t cur = nullptr;                       // stream the launch helpers enqueue on (== stream outside the decode groups)
    static const int MAX_GROUPS = 8; hipStream_t gstream[MAX_GROUPS] = {}; hipEvent_t gev[MAX_GROUPS] = {}; int n_groups = 1;
    struct StepGraph { int g, r0, n, precision, ln_stats, kclk, var_k, kv8; unsigned sw_epoch; SkwLogitParams lp; int rows, cons, gram; hipGraphExec_t exec; };
    std::vector<StepGraph> step_graphs; int use_graphs = 1;
    char errbuf[512] = {0};
    std::vector<void*> allocs;
    // front end
    float* pcm = nullptr; long* pcm_off = nullptr; int* n_samples = nullptr; int* n_len = nullptr; float* mel = nullptr; float* clip_max = nullptr;
    int *clip_idx = nullptr, *seek = nullptr;
    // per-clip audio context (skw_full_params.audio_ctx): slot_k[slot] = the positions of the window in that slot, travelling with clip_idx / seek.  var_k: some slot of the
    // current pass is shorter than n_audio_ctx — the attention kernels then take their extents from slot_k / SkwSeqState.n_keys (device memory); otherwise the launches are today's.
    // enc_rows: rows per slot of the encoder's activations in the last pass (dense: the largest K of the pass, rounded — enc_rows_for); h1_T: the conv1 rows per slot whose pad
    // rows are currently zero in h1
    int* slot_k = nullptr; bool var_k = false; int enc_rows = 0, h1_T = 0;
    half_t* im2col = nullptr; half_t* h1 = nullptr;
    // encoder
    float* x = nullptr; half_t* y16 = nullptr; half_t *Qh = nullptr, *Kh = nullptr, *Vt = nullptr; half_t* hbuf = nullptr; float* enc_out32 = nullptr;
    half_t *crossK = nullptr, *crossV = nullptr;
    // decoder
    // ggml q8 arithmetic (quantised files, exact precision): unrounded f32 activations and their q8 blocks
    float* dx = nullptr; half_t *dy16 = nullptr, *dq16 = nullptr, *datt16 = nullptr, *dh16 = nullptr;
    half_t *selfK = nullptr, *selfV = nullptr; float* logits = nullptr;
    float *y32 = nullptr, *h32 = nullptr, *encq32 = nullptr, *dy32 = nullptr, *datt32 = nullptr, *dh32 = nullptr;
    int8_t* q8_a = nullptr; float *q8_d = nullptr, *q8_s = nullptr; int q8_kmax = 0;
    // allocated at the first temperature retry (move_retry_slots)
    half_t *stageK = nullptr, *stageV = nullptr; int* slot_map = nullptr;
    int* prompt_buf = nullptr;                       // [B][SKW_PROMPT_CAP] per-row prompts
    int* row_tok = nullptr;                          // per-row prompt token / detected language scratch
    float* probs = nullptr; uint32_t* rng = nullptr;   // sampled (t > 0) passes: probability workspace, std::mt19937 state per clip
    SkwSeqState* st = nullptr; SkwTokenOut* toks = nullptr; uint8_t* static_mask = nullptr; int static_mask_nst = -1;
    // skw_full_batch_mixed: both static masks back to back ([0] without, [1] with the non-speech list; written at the first mixed call) and the rows' own rules, per window
    uint8_t* static_mask_pair = nullptr; int static_mask_pair_built = 0; SkwRowRules* row_rules = nullptr;
    SkwRowConstraints* row_cons = nullptr;           // skw_full_batch_rules: the rows' decoding constraints, per window (read by k_dec_constrain, which only constrained calls launch)
    // skw_full_batch_grammar (include/skw_grammar.h): the rows' grammar records, per window (read and advanced by k_dec_grammar_state / k_dec_grammar, which only calls with a
    // grammar launch); the text tokens' bytes on the device (offsets + bytes, built at the first such call: grammar_vocab_ensure); a small content-keyed cache of uploaded
    // tables, so a node instance's grammar is uploaded once and not per segment (most recently used last; entries of the call in flight are never evicted); and the call's
    // record per clip (next == nullptr: the clip has none)
    SkwRowGrammar* row_gram = nullptr; int32_t* gr_voc_off = nullptr; uint8_t* gr_voc_bytes = nullptr;
    struct GrammarImage { uint64_t hash; int n_states; std::vector<uint16_t> next; std::vector<uint8_t> accept; uint16_t* d_next; uint8_t* d_accept; long stamp; };
    std::vector<GrammarImage> gr_cache; long gr_stamp = 0, gr_uploads = 0; std::vector<SkwRowGrammar> gr_clip;
    SkwSeqState* h_st = nullptr; SkwTokenOut* h_toks = nullptr; // pinned
    int* h_row_live = nullptr; int* d_row_live = nullptr;      // per-row live flags in pinned host memory and their device-side address: k_dec_sample clears a row's flag itself,
                                                               // so a step ends with no 4-byte copy kernel (4.2 us in the chain of every step) — the host reads the flags after the stream drains
    int max_tok = 0;
    // the prompt ([prev] + past text + sot / language / task) in one multi-row pass instead of one token per step; SKW_PROMPT_PASS=0 or skw_debug_set_prompt_pass(ctx, 0)
    int prompt_pass_on = 1;
    int prompt_xattn_mq_on = 1;      // the exact precision's prompt pass: the 16-queries-per-workgroup cross attention (skw_debug_set_prompt_xattn_mq; same bits either way)
    int* pf_meta = nullptr; int pf_nseq = 0, pf_nq_max = 0;      // the pass's sequences on the device: [row0 | nq | slot] x max_batch (the multi-query cross attention of the f16_mfma prompt pass)
    int rows_cap = 0; SkwSeqState* pf_st = nullptr;  // decode-step scratch rows (>= max_batch: the prompt pass runs one row per prompt token) and the prompt pass's per-token pseudo-states
    int ln_stats_on = 1;                             // LayerNorm folded into the decode GEMMs (f16_mfma); SKW_DEC_LN_STATS=0 or skw_debug_set_ln_stats(ctx, 0): LayerNorm kernels
    // profiling: rows of the step about to be launched that are still decoding (finished rows return at once in the attention kernels: their bytes are not booked)
    int live_rows_hint = -1;
    // the in-kernel launch clock of the decode step's cross attention (skw_ctx_kernel_clock): one SkwKClk per (row group, layer); cur_group: the group run_decoder_step is enqueuing
    void* kclk = nullptr; int kclk_on = 0, kclk_khz = 0, cur_group = 0;
    int* forced_dev = nullptr; SkwTraceStep* trace_dev = nullptr;   // [max_batch][max_tok], allocated by the first skw_full_batch_traced
    skw_timing timing{};
    int last_enc_B = 0;
    // word timestamps (align_window, include/skw_align.h).  The workspace is allocated by the first call that aligns a clip (ensure_align_ws): P holds ONE layer's capture for a
    // chunk of al_rows alignment rows — every head, n_audio_ctx keys, f32 — so its size does not depend on the batch; acc / x: the chunk's matrices (f64 sums, f32 result).
    float* al_P = nullptr; double* al_acc = nullptr; float* al_x = nullptr; SkwAlignSeq* al_seqs = nullptr; int* al_times = nullptr; int al_rows = 0;      // al_times: jump | t0 | t1
    // the alignment pass in flight (al_on: only inside align_window): what run_decoder_step's hook captures after an alignment layer's cross-query GEMM
    bool al_on = false; const uint32_t* al_mask = nullptr;
    const SkwAlignSeq* al_h_seqs = nullptr; int al_tap_base = 0, al_tap_next = 0;      // taps: the chunk's records on the host, the call's sequence numbering
    int al_width = 7, al_nseq = 0, al_rows_now = 0, al_kw_max = 0, al_n_heads = 0, al_l_first = 0, al_l_last = 0;
    struct WsEntry { const char* name; void** slot; size_t bytes; bool zero; bool is_float; };      // one workspace buffer: the field it fills and its size (skw_ctx_create)
    std::vector<WsEntry> ws_table;
};
// name of the first workspace buffer whose pointer is null, or nullptr when every entry of the table is allocated
static const char* ws_first_null(const skw_ctx* c) {
    if (c->ws_table.empty()) return "(empty workspace table)";
    for (const skw_ctx::WsEntry& e : c->ws_table) if (!*e.slot) return e.name;
    return nullptr;
}
// every entry point that launches kernels starts here: a context whose table holds a null buffer never reaches a launch
#define WS_READY(c) do { if (const char* nb_ = ws_first_null(c)) { snprintf((c)->errbuf, 512, "workspace buffer '%s' is not allocated", nb_); return -1; } } while (0)

// ---- the functions that cross a file
namespace skw_priv {
// skw_model.hip: the loader's repack of a block-quantised weight (blocks: n_out rows of K / 32 blocks of ggml type qtype, as the file holds them), and its upload into L and m->allocs
SKW_HIDDEN void host_q(int qtype, const uint8_t* blocks, int n_out, int K, HostQ* h);
SKW_HIDDEN bool up_q(skw_model* m, const HostQ& h, int qtype, DevLin* L);
// skw_engine.hip: the NaN fill of a floating-point buffer the engine does not zero (a no-op unless skw_debug_alloc_poison armed it)
SKW_HIDDEN void poison_floats(void* p, size_t bytes);
// skw_engine.hip: a row of the switchboard held at a value for a scope (the kernel hooks force GEMM16W / GEMM16W_NGROUPS in-process); the value from before comes back on every path
struct SKW_HIDDEN SwOverride {
    int id, was;
    SwOverride(int id, int value);
    ~SwOverride();
    void set(int value);
    SwOverride(const SwOverride&) = delete; SwOverride& operator=(const SwOverride&) = delete;
};
}
using namespace skw_priv;
