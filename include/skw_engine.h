/*
 * skw_engine.h — C ABI of the MI355X Whisper engine (libskw_engine.so).
 *
 * This is the drop-in boundary for the arithmetic the reference reaches through
 * whisper-rs (FFI over whisper.cpp's C API).  Each entry point names the
 * reference call it replaces; a Rust host binds these with a ~40-line
 * `extern "C"` block (INTEGRATION.md shows it next to the whisper-rs calls it
 * displaces).  Plain pointers and sizes only — no torch, no C++ types.
 *
 *   reference (plugins/native/whisper/src/lib.rs)            this library
 *   ---------------------------------------------            ----------------------------
 *   WhisperContext::new_with_params(path, params)  :354-363  skw_model_load(path, gpu_device)
 *   context.create_state()                         :377-379  skw_ctx_create(model, max_batch, ...)
 *   FullParams::new(Greedy{best_of:1}) + setters   :624-641  skw_full_params (skw_full_default_params)
 *   whisper_state.full(params, &samples)           :644-646  skw_full_batch(ctx, params, pcm[], n[], n_clips)
 *   state.as_iter() / segment.to_str() /
 *     start_timestamp() / end_timestamp()          :650-660  skw_result.segments[i].{text,t0,t1}
 *
 * skw_full_batch is the batched form of `full`: n_clips independent calls of
 * whisper_full_with_state (greedy strategy, best_of 1, temperature fallback ladder) executed together on one GPU.
 * The kernels fail loudly (non-zero return + message) when no gfx950 device is
 * present; there is no CPU fallback in this library.
 */
#ifndef SKW_ENGINE_H
#define SKW_ENGINE_H
#include <stddef.h>
#include <stdint.h>
#include "skw_align_params.h"      /* skw_align_params; the arithmetic and its helpers: skw_align.h */
#include "skw_grammar.h"           /* skw_grammar: the table, the rule it applies to a row of logits, its check and CPU evaluator */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct skw_model skw_model;
typedef struct skw_ctx skw_ctx;

typedef struct {
    int32_t n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, ftype;
} skw_hparams;

/* the whisper_full_params fields the reference sets (lib.rs:624-641) + the whisper.cpp defaults that shape greedy decoding */
typedef struct {
    int32_t lang_id;          /* whisper_lang_id(language); "en" = 0; < 0 = whisper.cpp's "auto": detected per clip from the first window (multilingual models) */
    int32_t translate;
    int32_t suppress_blank;
    int32_t suppress_nst;
    int32_t no_timestamps;
    int32_t single_segment;
    int32_t max_tokens;
    float   max_initial_ts;
    float   entropy_thold;
    float   logprob_thold;
    float   no_speech_thold;
    int32_t n_threads;        /* accepted for ABI parity with the reference param; unused on the GPU */
    float   temperature;      /* whisper_full_params.temperature, default 0.0: the first pass of a window is greedy argmax */
    float   temperature_inc;  /* default 0.2: a window that fails (entropy / logprob / repetition rules) is decoded again at +0.2 .. 1.0,
                                 sampling with std::discrete_distribution semantics from a per-clip std::mt19937(0); <= 0 disables the ladder */
    int32_t audio_ctx;        /* whisper_full_params.audio_ctx (last field; the struct grew by four bytes with it): 0 = the model's n_audio_ctx (the default: today's behaviour, bit for bit);
                                 K in 1 .. n_audio_ctx: every window of the clip is encoded and attended over K positions — the conv stem sees mel frames [seek, seek + 2 K) and zeros
                                 beyond, the positional embedding is its first K rows, encoder, cross K / V and the decoder's cross attention have K positions.  What the host decides
                                 (seek advance, the 30 s window, segment assembly, the 0.02 s timestamp precision behind max_initial_ts) stays on the model's constants.  Per clip in
                                 skw_full_batch_mixed.  Outside [0, n_audio_ctx]: the call fails, naming the clip.  With lang_id < 0 the detection pass uses the same K. */
} skw_full_params;

typedef struct {
    int64_t t0, t1;             /* centiseconds: whisper_full_get_segment_t0/t1 */
    int32_t tok_begin, tok_end; /* [begin,end) into skw_result.tokens */
    int32_t text_off, text_len; /* into skw_result.text */
} skw_segment;

typedef struct { int32_t id, tid; float p, plog, pt, ptsum;
                 float margin;   /* top1 - top2 admissible logit when this token was chosen (+inf on sampled passes): distance from a tie (diagnostic) */
} skw_token;

typedef struct {
    int32_t n_segments, n_tokens, n_windows, n_decode_steps;
    int32_t fallback_requested; /* decoding passes that failed whisper.cpp's acceptance rules (each but the last temperature's is retried) */
    float   min_margin;         /* smallest top1-top2 admissible-logit margin seen (diagnostic) */
    skw_segment* segments;
    skw_token* tokens;
    char* text;                 /* concatenated segment texts, NUL terminated */
    int32_t text_len;
    int32_t lang_id;            /* the language decoded with: params.lang_id, or the detected one when that was < 0 */
} skw_result;

/* ---- lifetime ---- */
int  skw_device_count(void);
/* page-locked host memory for PCM handed to skw_full_batch: the engine's H2D copies of such buffers are asynchronous DMA (64 x 30 s clips: ~2.3 ms) instead of the driver's
 * staged copy out of pageable memory (~6 ms).  NULL when the allocation fails (callers fall back to ordinary memory). */
void* skw_host_alloc(size_t bytes);
void skw_host_free(void* p);
skw_model* skw_model_load(const char* ggml_path, int device, char* err, size_t errlen);
/* Block-quantised files (q4_0 / q4_1 / q5_0 / q5_1 / q8_0; the reference's default model is a q5_1 file, lib.rs:114-116):
 *   SKW_QUANT_GGML (default)  a context in the exact precision multiplies the way ggml does — activation rows to q8_0 / q8_1 blocks,
 *                             integer block dots, f32 scales (include/skw_ggml_quant.h (a)); a context in the f16_mfma precision runs the
 *                             file's dequantised f16 twin (both representations are resident)
 *   SKW_QUANT_F16_TWIN        the twin in both precisions (round-1 behaviour; also forced by the environment variable SKW_QUANT_TWIN)
 * skw_model_quant_type: the ggml tensor type running in ggml's arithmetic (2, 3, 6, 7, 8), or 0. */
enum { SKW_QUANT_F16_TWIN = 0, SKW_QUANT_GGML = 1 };
skw_model* skw_model_load_ex(const char* ggml_path, int device, int quant_mode, char* err, size_t errlen);
int skw_model_quant_type(const skw_model* m);
void skw_model_free(skw_model*);
void skw_model_get_hparams(const skw_model*, skw_hparams* out);
const char* skw_model_token_text(const skw_model*, int id, int* len);
/* whisper_tokenize: text -> token ids with whisper.cpp's tokenizer (a regex split into words, then inside each word the longest vocabulary entry at every position; only ids
 * below <|endoftext|> take part).  Returns the count, or -needed when cap is too small (ids then holds nothing meaningful).  Nothing is put in front of the text: openai's
 * reference prepends a space to an initial prompt (" " + prompt.strip()), whisper.cpp and this function do not.  Host code (streamkit_amd/csrc/skw_tokenizer.h); needs no device. */
int skw_model_tokenize(const skw_model*, const char* text, int32_t* ids, int cap);
int  skw_model_lang_id(const char* lang); /* whisper_lang_id; -1 if unknown */

skw_ctx* skw_ctx_create(skw_model*, int max_batch, int max_samples_per_clip, char* err, size_t errlen);
void skw_ctx_free(skw_ctx*);
const char* skw_ctx_last_error(const skw_ctx*);

/* Which form of the dense contractions (K2, K4-K6 and, in decode, K8-K10) a context runs.  Additive: the reference has no such knob.
 *   SKW_PRECISION_EXACT     f16 values widened to f32 and chained in k order on the f32-input MFMA: every tensor is bit-identical
 *                           to oracle/ (the checker mode; 1/16 of the f16 matrix rate);
 *   SKW_PRECISION_F16_MFMA  the same f16 operands fed to v_mfma_f32_16x16x32_f16 (f32 accumulate, hardware summation order):
 *                           intermediate tensors agree with the exact mode's to the tolerances tests/test_gpu_f16.py states, and every
 *                           greedy decision equals the exact mode's given the same history unless the exact mode's own top1 - top2
 *                           logit margin at that step is below twice the measured logit error (checked step by step under teacher
 *                           forcing, skw_full_batch_traced).  A free-running transcript is therefore identical to the exact mode's
 *                           up to its first such near-tie and may differ after it (on the synthetic benchmark model about a quarter
 *                           of the 30 s clips contain one; bench.py reports the count).  log-mel and the logit rules are the exact
 *                           kernels in both modes, and so are the encoder's LayerNorms; GELU is evaluated (exp2 / rcp) instead of looked
 *                           up, and the DECODE step folds its LayerNorms into the consuming GEMMs (k_gemm16_small_lnA: one-pass
 *                           E[x^2] - mean^2 statistics in f64, f32 rstd — within the mode's tolerance of k_layernorm's two-pass
 *                           arithmetic, not identical to it; SKW_DEC_LN_STATS=0 restores the LayerNorm kernels). */
#define SKW_PRECISION_EXACT 0
#define SKW_PRECISION_F16_MFMA 1
int skw_ctx_set_precision(skw_ctx*, int precision);   /* 0 on success; takes effect from the next call on this context */
int skw_ctx_get_precision(const skw_ctx*);

/* How a context stores the cross K / V its decode steps stream (additive; llama.cpp's --cache-type-k / --cache-type-v q8_0).  Not a third precision: a flag beside it.
 *   SKW_CROSS_KV_F16   (default) the f16 images; every launch is the one it was before this knob existed;
 *   SKW_CROSS_KV_Q8_0  the encoder pass also leaves cross K and V^T as ggml q8_0 blocks of 32 (include/skw_kv8.h: format, byte order, the bit-exact score chain), and every launch
 *                      of the single-query cross attention — decode steps, the language-detection step, prompt rows that take the single-query kernel — streams those, 1.0625 bytes
 *                      per element instead of 2.  The multi-query prompt pass and the word-timestamp capture keep reading the f16 images, which stay.  Costs another 1.0625 bytes
 *                      per element of memory (2.45 MB per slot and layer at Whisper-small), allocated when the flag is q8_0 AND the precision is f16_mfma for the first time
 *                      (whichever of the two setters completes the pair; a context that stays exact never allocates it).
 * Effective only while the context runs SKW_PRECISION_F16_MFMA with its fragment-order images: the exact precision owes the oracle its bits and ignores the flag (no bit changes). */
#define SKW_CROSS_KV_F16  0
#define SKW_CROSS_KV_Q8_0 1
int skw_ctx_set_cross_kv(skw_ctx*, int type);   /* 0 on success; from the next call on this context */
int skw_ctx_get_cross_kv(const skw_ctx*);

void skw_full_default_params(skw_full_params*);
/* The "auto" rule for skw_full_params.audio_ctx, stated once: clips of at least 480 000 samples (30 s) get n_audio_ctx; shorter ones
 * min(n_audio_ctx, 32 * ceil((ceil(n_samples / 320) + 25) / 32)) — the 20 ms positions the audio covers, half a second of margin, whole 32-key blocks.  Needs no device. */
int  skw_audio_ctx_for_samples(int n_samples, int n_audio_ctx);

/* ---- the hot path ---- */
/* One call, one request: skw_full_batch_request(ctx, &skw_full_request) — the struct stands further down, behind the types it names.  Every skw_full_batch* function and
 * skw_align_batch below is skw_full_batch_request with these fields set: its arguments go to the fields of the same name, everything else stays zero.  Each keeps its place here
 * because its comment is the contract of the field it introduced.
 * pcm[i]: 16 kHz mono f32, n_samples[i] samples; host pointers (pcm_on_device = 0) or device pointers (= 1).
 * results[i] is filled and must be released with skw_result_free. n_clips <= max_batch. Returns 0 on success. */
int  skw_full_batch(skw_ctx*, const skw_full_params*, const float* const* pcm, const int32_t* n_samples, int n_clips,
                    int pcm_on_device, skw_result* results);
void skw_result_free(skw_result*);
/* The temperature ladder's generator as the reference keeps it.  whisper.cpp owns ONE std::mt19937 per whisper_state (decoder 0's, seeded with 0 by whisper_init_state) and lets
 * it run on across calls of whisper_full_with_state; the reference node creates one state per instance (plugins/native/whisper/src/lib.rs:377-379), so an instance's n-th segment
 * that needs a sampled pass draws from where its earlier segments left the stream.  skw_full_batch_rng is skw_full_batch with that stream handed in and out per clip:
 * rng_state[i] = NULL (seed 0 for this call, what skw_full_batch does) or SKW_RNG_STATE_WORDS words — mt[624] and the index, initialised once by skw_rng_state_init — which the
 * call advances exactly as the reference's generator would advance on this clip.  Rows of a batch never share a stream, so in the exact precision the result does not
 * depend on batch composition (f16_mfma: under that precision's own contract for batch composition). */
#define SKW_RNG_STATE_WORDS 625
void skw_rng_state_init(uint32_t* state /* [SKW_RNG_STATE_WORDS] */);
int  skw_full_batch_rng(skw_ctx*, const skw_full_params*, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                        uint32_t* const* rng_state /* [n_clips], entries may be NULL */, skw_result* results);
/* Clips with different parameters in one batch: params[i] is clip i's own skw_full_params (every field may differ: language or auto-detection, task, no_timestamps,
 * single_segment, max_tokens, max_initial_ts, the suppress_* rules, the thresholds, temperature and temperature_inc).  results[i] is what skw_full_batch_rng returns for
 * clip i alone with params[i] and the same generator state: bit for bit in the exact precision, and in f16_mfma under that precision's contract for batch composition.
 * An array whose entries are all equal gives exactly what skw_full_batch_rng gives.  rng_state as above (may be NULL).  The node's scheduler batches its instances'
 * segments through this call whatever their parameters (the reference sets language and the suppress_* flags per instance, lib.rs:624-641). */
int  skw_full_batch_mixed(skw_ctx*, const skw_full_params* params /* [n_clips] */, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                          uint32_t* const* rng_state /* NULL, or [n_clips] with entries that may be NULL */, skw_result* results);
/* Text that conditions decoding: an initial prompt (whisper_full_params.initial_prompt / prompt_tokens) and the context whisper.cpp carries from one whisper_full_with_state call
 * of a state to the next (no_context = false: the state's prompt_past survives the call).  skw_full_batch_context is skw_full_batch_mixed with that token list handed in and out
 * per clip, the way rng_state hands the generator in and out.
 *   in   context[i][0] = n in 0 .. 512, context[i][1 .. n] = token ids, oldest first: whisper_state::prompt_past as it stands when whisper_full_with_state enters its window loop
 *        (the host has done the no_context clear and has put the initial prompt's tokens in front).  Every window — the first included — then follows the engine's one rule:
 *        a pass at temperature < 0.5 decodes behind [prev] + the last min(n_text_ctx / 2, n, room) tokens; the language-detection pass takes none.
 *   out  prompt_past as the call leaves it: what the last window's prompt took, then that window's kept tokens unless it was classed no-speech.  A clip too short to transcribe
 *        leaves its context as it was.
 * context = NULL or context[i] = NULL: an empty context that is not returned; such rows are skw_full_batch_mixed's, bit for bit and launch for launch.  n outside 0 .. 512 or an id
 * outside [0, n_vocab) fails the call (naming the clip) before anything runs; a failed call writes no context back. */
#define SKW_CONTEXT_WORDS 513   /* [0] = n in 0..512, [1..n] = token ids, oldest first: whisper_state::prompt_past */
int  skw_full_batch_context(skw_ctx*, const skw_full_params* params /* [n_clips] */, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                            uint32_t* const* rng_state /* as skw_full_batch_mixed */, int32_t* const* context /* NULL, or [n_clips] with entries that may be NULL */, skw_result* results);

/* Decoding constraints per clip, applied to the f32 logits row of every sampling decision before the sampler (k_dec_constrain), in this order:
 *   1. bias                  x[bias_id[k]] += bias[k] for k < n_bias: distinct ids in [0, n_vocab), each bias finite or -inf (-inf: the token is suppressed)
 *   2. repetition_penalty t  (finite, > 0; 1 = off) for each DISTINCT text token id of the pass so far: x[id] = x[id] < 0 ? x[id] * t : x[id] / t — once, however often it occurred
 *   3. no_repeat_ngram_size N (>= 0; 0 = off) with T = the pass's text tokens, m of them: for every i in 0 .. m - N with T[i .. i+N-1) == T[m-N+1 .. m), x[T[i+N-1]] = -inf
 * "the pass so far": the ids sampled in the current temperature pass of the current window that are below <|endoftext|> — timestamps, <|endoftext|> and specials neither count nor
 * are touched by 2 and 3, and the prompt ([prev] + carried context + sot / language / task) is not part of it.  The sampler then takes the row exactly where it took the decoder's:
 * no_speech_prob of a window's first decision is computed from the biased row (2 and 3 cannot move it: the history is empty there).  Not applied in the language-detection pass.
 * skw_full_batch_rules is skw_full_batch_context with one such record per clip: rules == NULL, a NULL entry or a default entry is skw_full_batch_context for that clip, bit for bit,
 * and a call whose clips are all default is that call launch for launch.  A bad record (t not finite or <= 0, N < 0, n_bias outside 0 .. SKW_BIAS_MAX, an id outside the vocabulary
 * or given twice, a bias that is +inf or NaN) fails the call before anything runs, naming the clip. */
#define SKW_BIAS_MAX 256
typedef struct { float repetition_penalty; int32_t no_repeat_ngram_size; int32_t n_bias; int32_t pad;
                 int32_t bias_id[SKW_BIAS_MAX]; float bias[SKW_BIAS_MAX]; } skw_decode_rules;
void skw_decode_rules_default(skw_decode_rules*);            /* 1.0, 0, 0 */
int  skw_full_batch_rules(skw_ctx*, const skw_full_params* params /* [n_clips] */, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                          uint32_t* const* rng_state, int32_t* const* context, const skw_decode_rules* const* rules /* NULL, or [n_clips] with entries that may be NULL */,
                          skw_result* results);

/* Word timestamps: a time per text token from the cross-attention weights of a set of alignment heads, warped against the token axis (openai-whisper word_timestamps,
 * whisper.cpp dtw_token_timestamps).  include/skw_align.h states the arithmetic, step by step, as one contract the kernels and a CPU evaluator evaluate to the same bits.
 * skw_full_batch_aligned is skw_full_batch_rules with one skw_align_params per clip: align == NULL, a NULL entry or enabled == 0 is skw_full_batch_rules for that clip, bit for
 * bit, and a call with no aligned clip is that call launch for launch (nothing is allocated either).  For an aligned clip every window that is accepted, is speech and holds
 * text is run once more, teacher-forced and without [prev] context, and its text tokens receive their times; tokens, text, segments and log-probabilities are what the
 * unaligned call returns.  times[i] (release with skw_token_times_free): n = results[i].n_tokens, t0 / t1 per result token in centiseconds from the clip's start, -1 for
 * timestamp tokens and for clips that did not ask.  t1 of a token is t0 of the window's next text token (the last one's: where <|endoftext|> aligns).
 * A bad record (empty head mask, a head or layer outside the model, median_width even, below 1 or above SKW_ALIGN_MEDIAN_MAX) fails the call before anything runs, naming the clip.
 * skw_align_batch is forced alignment of GIVEN text: clip i (at most 30 s: one window) against text_tokens[i][0 .. n_text[i]) (ids below <|endoftext|>, 1 .. n_text_ctx / 2 of
 * them); nothing is decoded.  times[i].n = n_text[i].  Language and task come from params[i] (lang_id < 0: detected); every align entry must be enabled. */
typedef struct { int32_t n; int64_t* t0; int64_t* t1; } skw_token_times;
int  skw_full_batch_aligned(skw_ctx*, const skw_full_params* params /* [n_clips] */, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                            uint32_t* const* rng_state, int32_t* const* context, const skw_decode_rules* const* rules, const skw_align_params* const* align /* as rules */,
                            skw_token_times* times /* [n_clips] out */, skw_result* results);
int  skw_align_batch(skw_ctx*, const skw_full_params* params /* [n_clips] */, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                     const int32_t* const* text_tokens, const int32_t* n_text, const skw_align_params* const* align, skw_token_times* times /* [n_clips] out */);
void skw_token_times_free(skw_token_times*);

/* Grammar-constrained decoding: a clip may bring a grammar — a byte-level DFA the transcript's text has to match in full (include/skw_grammar.h states the table, the rule and
 * its limits: REGULAR languages only, where whisper.cpp's grammar_rules are GBNF; per temperature pass and per window, so it is meant for utterances of one window; timestamps
 * are transparent to the match; the penalty is finite, so where the sampler's own masks remove every fitting token the best non-fitting one wins).  The rule is stage 4 on the
 * f32 logits row, after skw_decode_rules' three and ahead of the sampler (k_dec_grammar); not applied in the language-detection pass nor while a row feeds its prompt.
 * skw_full_batch_grammar is skw_full_batch_aligned with one grammar per clip: grammar == NULL or a NULL entry is skw_full_batch_aligned for that clip, bit for bit, and a call
 * in which no clip has a grammar launches exactly what that call launches (no new kernel, no allocation, the same step graphs).  Every clip may bring its own grammar; equal
 * tables are uploaded once, and the context keeps the last few it saw (keyed by content), so a caller that hands in the same grammar segment after segment uploads it once.
 * A bad record (skw_grammar_check) fails the call before anything runs, naming the clip.  Not part of the traced / teacher-forced entries.
 * skw_grammar_compile makes a grammar from a pattern (the regular-expression subset of streamkit_amd/csrc/skw_grammar_compile.h; flags: SKW_GRAMMAR_IGNORE_CASE = 1):
 * 0 and *out (release with skw_grammar_free), or -1 and the compiler's message in err.  A table made any other way is as good: fill in the struct. */
int  skw_full_batch_grammar(skw_ctx*, const skw_full_params* params /* [n_clips] */, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                            uint32_t* const* rng_state, int32_t* const* context, const skw_decode_rules* const* rules, const skw_align_params* const* align,
                            skw_token_times* times, const skw_grammar* const* grammar /* NULL, or [n_clips] with entries that may be NULL */, skw_result* results);
int  skw_grammar_compile(const char* pattern, size_t len, int flags, float penalty, skw_grammar** out, char* err, size_t errlen);
void skw_grammar_free(skw_grammar*);

/* ---- decision trace / teacher forcing (parity instrumentation of the hot path; the reference has no counterpart) ----
 * skw_full_batch_traced is skw_full_batch that also returns, per clip, one record for EVERY sampling decision it made, in execution order
 * over all windows and temperature passes (discarded tokens included).  With forced_ids[i] == NULL the run is free (forced_id == chosen_id).
 * With forced_ids[i] = the chosen_id sequence of another run (another precision of the same model on the same audio), the decoder is fed
 * those tokens instead of its own choices, so every step sees exactly the history the other run saw and the two runs' decisions can be
 * compared step by step: chosen_id is what THIS precision's argmax picked, top1 / top2 the two largest admissible logits, forced_logit
 * the logit of the fed token.  A forced sequence that runs out before the decoder stops is an error (the runs' control flow diverged).
 * The decode steps are launched eagerly in this mode (same kernels as the captured step graph, plus the trace form of the sampler). */
typedef struct { int32_t chosen_id, forced_id, top1_id, top2_id; float top1, top2, forced_logit, lse;
                 float temperature;   /* of the pass this decision belongs to; > 0: chosen_id is a std::discrete_distribution draw (not an argmax) and the logits here are the row's divided by it */
                 int32_t pad; } skw_trace_step;
typedef struct { int32_t n; skw_trace_step* steps; } skw_trace;
int  skw_full_batch_traced(skw_ctx*, const skw_full_params*, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                           const int32_t* const* forced_ids /* [n_clips] or NULL */, const int32_t* n_forced /* [n_clips] or NULL */,
                           skw_trace* traces /* [n_clips] out; release with skw_trace_free */, skw_result* results);
/* the same with each clip's context handed in and out as skw_full_batch_context does (context NULL, or [n_clips] with entries that may be NULL): teacher forcing of clips that decode
 * behind carried text */
int  skw_full_batch_traced_context(skw_ctx*, const skw_full_params*, const float* const* pcm, const int32_t* n_samples, int n_clips, int pcm_on_device,
                                   const int32_t* const* forced_ids, const int32_t* n_forced, skw_trace* traces, int32_t* const* context, skw_result* results);
void skw_trace_free(skw_trace*);

/* ---- the request: what every entry above fills in ----
 * A field left zero asks for nothing, and a feature's array in which no clip asks is that call without the array, launch for launch (the paragraphs above, field by field).
 * size is what lets the struct grow at its end: a caller compiled against an older header hands in its own sizeof, the fields it does not know stay zero.  A size below
 * SKW_FULL_REQUEST_MIN (the struct as it was first published) or above this library's sizeof fails with -1 and a message.
 * params_per_clip picks the launches, not just the reading of params: 0 is the uniform form (skw_full_batch, _rng, _traced*), 1 the per-row form (_mixed and every entry after it,
 * skw_align_batch) even where all blocks are equal — same results, different kernels.
 * Combinations no entry above offers are refused with -3 before anything runs: traces with params_per_clip, rng_state, rules, align or grammar; text_tokens with rng_state,
 * context, rules, grammar or traces; forced_ids without n_forced or without traces.  A refused call writes back no generator state and no context; times[i] and traces[i] are
 * zeroed before anything is checked, so they are defined after a failed call. */
typedef struct {
    uint32_t size;              /* sizeof(skw_full_request) as the caller compiled it */
    int32_t  params_per_clip;   /* 0: params is ONE block (the uniform launches); 1: params[n_clips] (the per-row launches) */
    const skw_full_params* params;
    const float* const* pcm; const int32_t* n_samples; int32_t n_clips; int32_t pcm_on_device;
    uint32_t* const* rng_state;                 /* NULL, or [n_clips], entries may be NULL */
    int32_t* const* context;                    /* as skw_full_batch_context */
    const skw_decode_rules* const* rules;       /* as skw_full_batch_rules */
    const skw_align_params* const* align; skw_token_times* times;      /* as skw_full_batch_aligned */
    const skw_grammar* const* grammar;          /* as skw_full_batch_grammar */
    const int32_t* const* text_tokens; const int32_t* n_text;          /* forced alignment, as skw_align_batch: nothing is decoded; results may be NULL */
    const int32_t* const* forced_ids; const int32_t* n_forced; skw_trace* traces;   /* traces != NULL: as skw_full_batch_traced_context */
    skw_result* results;
} skw_full_request;
#define SKW_FULL_REQUEST_MIN 136
int skw_full_batch_request(skw_ctx*, const skw_full_request*);

/* Test hook: one sampler launch (constrain -> grammar -> sampler, as in the decode step) on caller-supplied logits; skw_engine.hip states it next to the code.  The five
 * skw_debug_sample_rows* hooks are this request with their arguments filled in.  trace = 0, temperature, rng_state and the pointers behind them are not offered together with
 * rules or grammar (-3 before the launch). */
typedef struct {
    int32_t  params_per_row;    /* 0: params is ONE block (the uniform launch); 1: params[n_rows] (the per-row launch) */
    int32_t  n_rows;
    const skw_full_params* params;
    const int32_t* hist; int32_t hist_stride; int32_t form; const int32_t* n_hist; const float* logits;      /* hist [n_rows][hist_stride], logits [n_rows][n_vocab] on the host */
    float* filtered_out; skw_token* tok_out; skw_trace_step* trace_out;
    const skw_decode_rules* const* rules; const skw_grammar* const* grammar;      /* NULL, or [n_rows] with entries that may be NULL */
    const int32_t* active;      /* NULL, or [n_rows]: 0 marks a row as finished before the launch */
    const float* temperature; uint32_t* rng_state;      /* [n_rows] / [n_rows][SKW_RNG_STATE_WORDS], in and out */
    int32_t trace;              /* 1: the launch with the trace buffers (what every hook but _ex runs); 0: without, trace_out is left alone */
    int32_t kernel_id;          /* out: SKW_SMPK_* bits of the kernel the launcher picked */
    float* probs_out; float* no_speech_prob; int32_t* n_tokens; int32_t* cur_token; int32_t* active_out;      /* the rows' state after the launch */
} skw_sample_rows_request;
int skw_debug_sample_rows_request(skw_ctx*, skw_sample_rows_request*);

/* timing of the last skw_full_batch (milliseconds, GPU events on the engine's stream) */
typedef struct { float mel_ms, encode_ms, decode_ms, total_ms; int32_t n_windows, n_decode_steps, n_tokens;
                 /* n_row_steps: sum over rows of the decode steps the row was live in (a finished row's attention kernels return at once:
                    the HBM bytes of a step scale with its live rows) */
                 int32_t n_row_steps;
                 /* how the decode step of the call's last window pass ran: row groups (each a step graph on its own stream) and rows in the first group — what a per-launch
                    roofline of the decode kernels has to be booked against (bench.py reads these instead of restating the engine's default) */
                 int32_t decode_groups, decode_group_rows;
} skw_timing;
void skw_ctx_last_timing(const skw_ctx*, skw_timing* out);
/* per-kernel-class event timing (adds an event pair around every launch; use for roofline accounting, not for the timed run).
 * classes: 0 k_gemm, 1 k_gemm_smallm, 2 k_attn_encoder, 3 k_layernorm, 4 k_mel, 5 k_dec_self_attn, 6 k_dec_sample, 7 other, 8 k_dec_cross_attn, 9 k_dec_constrain,
 *          10 k_align_qk, 11 k_align_reduce, 12 k_align_dtw (word timestamps), 13 k_dec_grammar (both of its launches) */
void skw_ctx_profile(skw_ctx*, int on);
int  skw_ctx_profile_get(skw_ctx*, int cls, char* name, size_t name_len, long* count, double* ms, double* algorithmic_flops, double* algorithmic_bytes);
/* In-kernel launch clock of the decode step's dominant kernel (the f16_mfma cross attention).  HIP events cannot sit between the kernels of a captured step graph, and an eager,
 * event-stamped step is not the timed configuration (two row groups interleave differently): armed, the kernel itself records first-wave-in and last-wave-out of every launch on the
 * device's constant-rate clock while the step graphs run as in any other call.  skw_ctx_kernel_clock_get: the launches the last skw_full_batch recorded — count, summed microseconds,
 * summed live rows (a launch's algorithmic bytes = 4 B x live rows x n_audio_ctx x n_text_state), shortest / longest launch, the clock's rate in kHz.  Diagnostic; off by default. */
int  skw_ctx_kernel_clock(skw_ctx*, int on);
int  skw_ctx_kernel_clock_get(skw_ctx*, long* launches, double* sum_us, double* sum_live_rows, double* min_us, double* max_us, int* clock_khz);
/* the keys those launches walked, summed over their live rows: with per-clip audio contexts a launch's algorithmic bytes are 4 B x (its rows' walked keys) x n_text_state */
int  skw_ctx_kernel_clock_keys(skw_ctx*, double* sum_keys);
/* every recorded launch as (begin us, end us, live rows), relative to the earliest begin; returns the count written.  Row groups run on their own streams, so launches overlap:
 * the union of the intervals is the time the kernel was in flight at all. */
long skw_ctx_kernel_clock_records(skw_ctx*, double* out /* [cap][3] */, long cap);
/* the HIP stream the engine launches on (opaque hipStream_t) */
void* skw_ctx_stream(const skw_ctx*);

/* ---- stage taps (used by the parity tests and by hosts that only need a front end) ---- */
/* K1: log-mel of one clip; mel_out [n_mel][n_len] f32 (whisper.cpp layout); caller provides cap floats */
int skw_log_mel(skw_ctx*, const float* pcm_host, int n_samples, float* mel_out, size_t cap, int* n_len, int* n_len_org);
/* K2: conv stem + positional embedding for the window at `seek`; x0 [n_audio_ctx][n_state] f32 */
int skw_conv_stem(skw_ctx*, const float* pcm_host, int n_samples, int seek, float* x0);
/* K2-K6: encoder output (after ln_post) [n_audio_ctx][n_state] f32 and, when non-null, cross K/V [n_text_layer][n_audio_ctx][n_state] f32 */
int skw_encode(skw_ctx*, const float* pcm_host, int n_samples, int seek, float* enc_out, float* cross_k, float* cross_v);
/* the same taps at an audio context of K = audio_ctx positions (0 = n_audio_ctx): x0 [K][n_state]; enc_out [K][n_state], cross K/V [n_text_layer][K][n_state] */
int skw_conv_stem_actx(skw_ctx*, const float* pcm_host, int n_samples, int seek, int audio_ctx, float* x0);
int skw_encode_actx(skw_ctx*, const float* pcm_host, int n_samples, int seek, int audio_ctx, float* enc_out, float* cross_k, float* cross_v);
/* K7-K10: after skw_encode / skw_encode_actx (whose K it follows), run the decoder on tokens[0..n) from position 0 and return the last token's logits [n_vocab] */
int skw_decode_logits(skw_ctx*, const int32_t* tokens, int n_tokens, float* logits);

/* ---- resampler front end: the arithmetic of the reference's audio::resampler node on the GPU ----
 * reference: crates/nodes/src/audio/filters/resampler.rs:231-244 (FastFixedIn::new(ratio, 1.0, Linear, chunk_frames, channels)),
 *            :384-514 (per-chunk process), :543-688 (remainder with a fresh resampler). */
typedef struct skw_dsp skw_dsp;                 /* model-free device context (stream + scratch) */
skw_dsp* skw_dsp_create(int device, char* err, size_t errlen);
void skw_dsp_free(skw_dsp*);
const char* skw_dsp_last_error(const skw_dsp*);
typedef struct { double last_index; double ratio; int32_t chunk_frames; int32_t channels; float hist[32]; } skw_resampler_state; /* rubato's carried state: fractional index + 16-frame history */
void skw_resampler_init(skw_resampler_state*, double ratio /* out/in */, int chunk_frames, int channels);
/* n_chunks full chunks of interleaved f32 input -> interleaved output (host pointers); bit-exact with rubato's Linear interpolation */
int skw_resample_linear(skw_dsp*, skw_resampler_state*, const float* in, int n_chunks, float* out, int out_cap_frames, int* out_frames);
/* how the last skw_resample_linear obtained its index sequence: 0 = the closed-form per-chunk proposal was proven equal to rubato's
 * sequential f64 walk on the device (48 / 32 / 96 kHz sources), 1 = a second proposal was (44.1 kHz family and every other ratio met so
 * far: chunk starts walked by the host for long calls, stepped binade by binade on the device for short ones), 2 = neither: the
 * single-lane walk ran */
int skw_dsp_last_scan_fallback(const skw_dsp*);
/* additive quality mode: polyphase Kaiser-windowed sinc (32 taps/phase), whole buffer */
int skw_resample_polyphase(skw_dsp*, const float* in, long n_in_frames, int channels, int in_rate, int out_rate, float* out, long out_cap_frames, long* out_frames);
/* the same filter over a stream, packet by packet: the input tail later outputs need stays in HBM; results identical to the whole-buffer call */
typedef struct skw_pp_stream skw_pp_stream;
skw_pp_stream* skw_polyphase_stream_create(skw_dsp*, int channels, int in_rate, int out_rate);
int  skw_polyphase_stream_push(skw_pp_stream*, const float* in, long n_frames, int final_call, float* out, long out_cap_frames, long* out_frames);
void skw_polyphase_stream_free(skw_pp_stream*);

#ifdef __cplusplus
}
#endif
#endif
