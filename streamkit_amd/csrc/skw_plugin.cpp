// skw_plugin.cpp — libwhisper.so: the StreamKit native plugin `whisper` (registered by the host as
// plugin::native::whisper) on top of the MI355X engine.  Drop-in for the reference cdylib:
//   /root/reference/plugins/native/whisper/src/lib.rs        (this file restates it function by function)
//   /root/reference/sdks/plugin-sdk/native/src/lib.rs:426-856 (the six extern "C" entry points the macro generates)
// ABI: include/streamkit_native_abi.h.
//
// Params beyond the reference's are ADDITIVE (unknown keys are ignored by the reference's serde config, lib.rs:66-104):
// vad_mode, batch_window_ms, max_batch, mixed_batch, flush_tail, precision, gpu_device: "auto", initial_prompt, carry_context, repetition_penalty,
// no_repeat_ngram_size, suppress_tokens, logit_bias (decoding constraints per instance, skw_full_batch_rules), grammar / grammar_choices / grammar_ignore_case /
// grammar_penalty (a pattern the transcript has to match, skw_full_batch_grammar), and input_sample_rate / input_resample_mode (the
// audio::resampler node's arithmetic run inside this plugin, skw_resampler_core.h: a 48 kHz Opus source then needs no node in between).
// One BEHAVIOURAL difference remains and is not additive: with the default vad_mode "auto" the Silero model at `vad_model_path`
// gates what Whisper sees exactly as in the reference (skw_silero.h) only when that file exists; when it does not, the
// reference fails ("Failed to initialize VAD: ...") while this build logs a warning and falls back to an RMS energy gate
// (p = rms / (rms + 0.01), so vad_threshold then means a level, not a speech probability).  `vad_mode: "silero"` restores the
// reference's hard failure.  INTEGRATION.md section D lists this with the other observable differences.
#include "../../include/streamkit_native_abi.h"
#include "../../include/skw_engine.h"
#include "../../include/skw_align.h"
#include "skw_decode_rules.h"
#include "skw_words.h"
#include "skw_segmenter.h"
#include "../../include/skw_vad_batch.h"
#include "skw_silero.h"
#include "skw_resampler_core.h"
#include <sys/stat.h>
#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

// ------------------------------------------------------------------ error strings (conversions.rs:441-461: thread-local, borrowed)
thread_local std::string g_last_error;
CResult ok_result() { CResult r; r.success = true; r.error_message = nullptr; return r; }
CResult err_result(const std::string& msg) {
    g_last_error = msg; for (auto& ch : g_last_error) if (ch == '\0') ch = ' ';
    CResult r; r.success = false; r.error_message = g_last_error.c_str(); return r;
}
CResult err_null() { CResult r; r.success = false; r.error_message = nullptr; return r; }
// Nothing may unwind into the host's Rust frames (SURVEY.md section 8b "Errors": panics / C++ exceptions must not cross): every entry point
// body runs under this — std::bad_alloc / length_error from the buffers, std::system_error from the worker thread, std::future_error ...
template <typename F> CResult guarded(const char* what, F&& f) {
    try { return f(); }
    catch (const std::exception& e) { return err_result(std::string(what) + ": " + e.what()); }
    catch (...) { return err_result(std::string(what) + ": unknown C++ exception"); }
}

// ------------------------------------------------------------------ configuration (lib.rs:25-157)
struct WhisperConfig {
    std::string model_path = "models/ggml-base.en-q5_1.bin";
    std::string language = "en";
    std::string vad_model_path = "models/silero_vad.onnx";
    float vad_threshold = 0.5f;
    uint64_t min_silence_duration_ms = 700;
    float max_segment_duration_secs = 30.0f;
    uint64_t n_threads = 0;
    bool use_gpu = false; int gpu_device = 0; bool gpu_device_auto = false;
    bool suppress_blank = true, suppress_non_speech_tokens = true;
    bool emit_vad_events = false;
    // additive
    std::string vad_mode = "auto";   // auto | silero | energy | always
    int batch_window_ms = 2; int max_batch = 64; bool flush_tail = false;
    bool mixed_batch = true;         // segments of differently configured instances share a GPU batch (skw_full_batch_mixed); false: a batch is cut at the first job whose parameters differ
    std::string precision = "exact"; // exact | f16_mfma  (include/skw_engine.h, SKW_PRECISION_*)
    std::string cross_kv = "f16";    // f16 | q8_0  (include/skw_engine.h, SKW_CROSS_KV_*): how the decode steps' cross K / V is stored; q8_0 needs precision f16_mfma
    // skw_full_params.audio_ctx of this instance's segments: 0 (the model's context, the reference's behaviour), an integer 1 .. n_audio_ctx, or "auto" (skw_audio_ctx_for_samples per
    // segment).  An integer out of range is the engine's refusal, per request: it stays with the segment that carries it
    int audio_ctx = 0; bool audio_ctx_auto = false;
    std::string vad_device = "cpu";  // cpu (the libm Silero gate, frame by frame) | gpu (Silero in the contract arithmetic of include/skw_silero_net.h on gpu_device's GPU)
    int vad_batch_frames = 1;        // complete 512-sample frames held back before the gate is asked for their probabilities in one call
    // Text that conditions decoding (skw_full_batch_context).  The defaults are the reference's behaviour: whisper-rs leaves no_context = true and sets no prompt (lib.rs:624-641).
    std::string initial_prompt;      // whisper_full_params.initial_prompt: tokenised with whisper.cpp's tokenizer (nothing is put in front of it), in front of every segment's context
    bool carry_context = false;      // whisper_full_params.no_context = false: the text of this instance's segment n conditions its segment n + 1
    uint32_t input_sample_rate = 16000; std::string input_resample_mode = "linear";   // linear (the audio::resampler node's rubato arithmetic, bit for bit) | polyphase
    // Decoding constraints of this instance's segments (skw_full_batch_rules): repetition_penalty, no_repeat_ngram_size, and suppress_tokens (a -inf bias each) + logit_bias as the
    // record's pairs, at most SKW_BIAS_MAX distinct ids together.  The default record asks for nothing.  max_suppress_id / max_bias_id: the largest id each key named (-1: none),
    // so that the check against the loaded model's vocabulary can name the key
    skw_decode_rules rules; int max_suppress_id = -1, max_bias_id = -1;
    // (additive) timestamp_granularity: "segment" (the reference's output, byte for byte) | "word" (one segment per word: skw_words.h on the token times of skw_full_batch_aligned).
    // alignment_heads: "top:N" (every head of the top N decoder layers; N = 0: half of them, the default) or explicit [layer, head] pairs in align.head_mask
    bool word_timestamps = false; int align_top = 0; bool align_explicit = false; skw_align_params align;
    // (additive) grammar | grammar_choices, grammar_ignore_case, grammar_penalty: the pattern this instance's transcripts have to match (include/skw_grammar.h: a regular
    // expression compiled to a byte DFA — the regular subset of whisper.cpp's grammar_rules), compiled when the parameters are parsed; null: none
    std::shared_ptr<skw_grammar> grammar;
    WhisperConfig() { skw_decode_rules_set_default(&rules); memset(&align, 0, sizeof align); align.median_width = 7; }
};

// repetition_penalty, no_repeat_ngram_size, suppress_tokens, logit_bias -> cfg->rules; every refusal names its key
bool parse_decode_rules(const skw::JsonValue& v, WhisperConfig* cfg, std::string* err) {
    skw_decode_rules& r = cfg->rules;
    auto bad = [&](const std::string& m) { *err = "Invalid config: " + m; return false; };
    auto whole = [](const skw::JsonValue& x, double lo, double hi) { return x.type == skw::JsonValue::Number && x.num == std::floor(x.num) && x.num >= lo && x.num <= hi; };
    if (const skw::JsonValue* x = v.get("repetition_penalty")) {
        if (x->type != skw::JsonValue::Number || !std::isfinite((float)x->num) || !((float)x->num > 0.0f)) return bad("repetition_penalty must be a number > 0 (1.0 = off)");
        r.repetition_penalty = (float)x->num;
    }
    if (const skw::JsonValue* x = v.get("no_repeat_ngram_size")) {
        if (!whole(*x, 0, 1e6)) return bad("no_repeat_ngram_size must be an integer >= 0 (0 = off)");
        r.no_repeat_ngram_size = (int32_t)x->num;
    }
    // suppression first, then the biases: an id under both keys is suppressed (x + b, then -inf, is -inf)
    auto add = [&](const char* key, int id, float b) {
        for (int k = 0; k < r.n_bias; ++k) if (r.bias_id[k] == id) {
            if (std::isinf(r.bias[k]) && !std::isinf(b)) return true;
            if (std::isinf(b)) return true;      // (listed twice under suppress_tokens: once is enough)
            return bad(std::string(key) + ": token id " + std::to_string(id) + " is given twice");
        }
        if (r.n_bias >= SKW_BIAS_MAX) return bad("suppress_tokens and logit_bias together allow at most " + std::to_string(SKW_BIAS_MAX) + " distinct token ids");
        r.bias_id[r.n_bias] = id; r.bias[r.n_bias] = b; ++r.n_bias;
        return true;
    };
    if (const skw::JsonValue* x = v.get("suppress_tokens")) {
        if (x->type != skw::JsonValue::Array) return bad("suppress_tokens must be an array of token ids");
        for (const skw::JsonValue& e : x->arr) {
            if (!whole(e, 0, 1e9)) return bad("suppress_tokens must be an array of token ids (integers >= 0)");
            if (!add("suppress_tokens", (int)e.num, -INFINITY)) return false;
            cfg->max_suppress_id = std::max(cfg->max_suppress_id, (int)e.num);
        }
    }
    if (const skw::JsonValue* x = v.get("logit_bias")) {
        if (x->type != skw::JsonValue::Array) return bad("logit_bias must be an array of [token id, bias] pairs");
        for (const skw::JsonValue& e : x->arr) {
            if (e.type != skw::JsonValue::Array || e.arr.size() != 2 || !whole(e.arr[0], 0, 1e9) || e.arr[1].type != skw::JsonValue::Number || !std::isfinite((float)e.arr[1].num))
                return bad("logit_bias must be an array of [token id, bias] pairs (an integer >= 0 and a finite number; suppress_tokens is the -inf bias)");
            if (!add("logit_bias", (int)e.arr[0].num, (float)e.arr[1].num)) return false;
            cfg->max_bias_id = std::max(cfg->max_bias_id, (int)e.arr[0].num);
        }
    }
    return true;
}
// grammar (a pattern) | grammar_choices (strings: " ?(c1|c2|...)[.!?]?" with each choice escaped), grammar_ignore_case, grammar_penalty -> cfg->grammar.  The default penalty
// is 100, whisper.cpp's grammar_penalty default as recalled (it could not be checked against its source here).
bool parse_grammar(const skw::JsonValue& v, WhisperConfig* cfg, std::string* err) {
    auto bad = [&](const std::string& m) { *err = "Invalid config: " + m; return false; };
    const skw::JsonValue* gp = v.get("grammar"); const skw::JsonValue* gc = v.get("grammar_choices");
    bool icase = false; float penalty = 100.0f;
    if (const skw::JsonValue* x = v.get("grammar_ignore_case")) { if (x->type != skw::JsonValue::Bool) return bad("grammar_ignore_case must be a boolean"); icase = x->b; }
    if (const skw::JsonValue* x = v.get("grammar_penalty")) {
        if (x->type != skw::JsonValue::Number || !std::isfinite((float)x->num) || !((float)x->num > 0.0f)) return bad("grammar_penalty must be a finite number > 0");
        penalty = (float)x->num;
    }
    cfg->grammar.reset();
    if (gp && gc) return bad("grammar and grammar_choices cannot both be given");
    std::string pattern;
    if (gp) {
        if (gp->type != skw::JsonValue::String) return bad("grammar must be a string (a pattern)");
        if (gp->str.empty()) return true;      // (the default: no grammar)
        pattern = gp->str;
    } else if (gc) {
        if (gc->type != skw::JsonValue::Array) return bad("grammar_choices must be an array of strings");
        if (gc->arr.empty()) return true;
        pattern = " ?(";
        for (size_t k = 0; k < gc->arr.size(); ++k) {
            const skw::JsonValue& e = gc->arr[k];
            if (e.type != skw::JsonValue::String || e.str.empty()) return bad("grammar_choices must be an array of non-empty strings");
            if (k) pattern += "|";
            for (unsigned char ch : e.str) {      // every ASCII character that is not a letter or a digit is escaped: the choice is matched literally
                if (ch < 0x80 && !std::isalnum(ch)) pattern += '\\';
                pattern += (char)ch;
            }
        }
        pattern += ")[.!?]?";
    } else return true;
    skw_grammar* g = nullptr; char e[256] = {0};
    if (skw_grammar_compile(pattern.data(), pattern.size(), icase ? 1 : 0, penalty, &g, e, sizeof e) != 0) return bad(std::string(gp ? "grammar: " : "grammar_choices: ") + e);
    cfg->grammar = std::shared_ptr<skw_grammar>(g, skw_grammar_free);
    return true;
}
// the ids against the loaded model's vocabulary (create_instance and update_params, once the engine is known)
bool check_rule_ids(const WhisperConfig& cfg, int n_vocab, std::string* err) {
    for (int pass = 0; pass < 2; ++pass) {
        const int mx = pass ? cfg.max_bias_id : cfg.max_suppress_id;
        if (mx >= n_vocab) { *err = std::string("Invalid config: ") + (pass ? "logit_bias" : "suppress_tokens") + ": token id " + std::to_string(mx) + " outside the model's vocabulary [0, " +
                                    std::to_string(n_vocab) + ")"; return false; }
    }
    char e[512];
    if (!skw_decode_rules_check(&cfg.rules, n_vocab, "decoding rules", e, sizeof e)) { *err = std::string("Invalid config: ") + e; return false; }      // (nothing the parser lets through)
    return true;
}

bool parse_config(const char* json, WhisperConfig* cfg, std::string* err) {
    if (!json || !*json) return true;
    skw::JsonValue v; std::string perr;
    if (!skw::json_parse(json, &v, &perr)) { *err = "Invalid config: " + perr; return false; }
    if (v.type == skw::JsonValue::Null) return true;
    if (v.type != skw::JsonValue::Object) { *err = "Invalid config: expected a JSON object"; return false; }
    auto str = [&](const char* k, std::string* dst) { const skw::JsonValue* x = v.get(k);
    if (!x) return true; if (x->type != skw::JsonValue::String) { *err = std::string("Invalid config: invalid type for `") + k + "`, expected a string";
    return false; } *dst = x->str; return true; };
    auto num = [&](const char* k, double* dst) { const skw::JsonValue* x = v.get(k);
    if (!x) return true; if (x->type != skw::JsonValue::Number) { *err = std::string("Invalid config: invalid type for `") + k + "`, expected a number";
    return false; } *dst = x->num; return true; };
    auto boo = [&](const char* k, bool* dst) { const skw::JsonValue* x = v.get(k);
    if (!x) return true; if (x->type != skw::JsonValue::Bool) { *err = std::string("Invalid config: invalid type for `") + k + "`, expected a boolean";
    return false; } *dst = x->b; return true; };
    double d;
    if (!str("model_path", &cfg->model_path) || !str("language", &cfg->language) || !str("vad_model_path", &cfg->vad_model_path) || !str("vad_mode", &cfg->vad_mode)
        || !str("precision", &cfg->precision)) return false;
    if (cfg->precision != "exact" && cfg->precision != "f16_mfma") { *err = "Invalid config: precision must be \"exact\" or \"f16_mfma\""; return false; }
    if (!str("cross_kv", &cfg->cross_kv)) return false;
    if (cfg->cross_kv != "f16" && cfg->cross_kv != "q8_0") { *err = "Invalid config: cross_kv must be \"f16\" or \"q8_0\""; return false; }
    if (cfg->cross_kv == "q8_0" && cfg->precision != "f16_mfma") {
        *err = "Invalid config: cross_kv \"q8_0\" needs precision \"f16_mfma\": the exact precision reproduces the reference bit for bit and cannot read quantised cross K/V";
        return false;
    }
    if (!str("vad_device", &cfg->vad_device) || !str("initial_prompt", &cfg->initial_prompt)) return false;
    if (cfg->vad_device != "cpu" && cfg->vad_device != "gpu") { *err = "Invalid config: vad_device must be \"cpu\" or \"gpu\""; return false; }
    d = cfg->vad_batch_frames; if (!num("vad_batch_frames", &d)) return false;
    if (d < 1 || d > 65536 || d != std::floor(d)) { *err = "Invalid config: vad_batch_frames must be an integer between 1 and 65536"; return false; }
    cfg->vad_batch_frames = (int)d;
    if (!str("input_resample_mode", &cfg->input_resample_mode)) return false;
    if (cfg->input_resample_mode != "linear" && cfg->input_resample_mode != "polyphase") { *err = "Invalid config: input_resample_mode must be \"linear\" or \"polyphase\""; return false; }
    d = cfg->input_sample_rate; if (!num("input_sample_rate", &d)) return false;
    if (d < 1000 || d > 768000 || d != std::floor(d)) { *err = "Invalid config: input_sample_rate must be an integer between 1000 and 768000";
    return false; } cfg->input_sample_rate = (uint32_t)d;
    d = cfg->vad_threshold; if (!num("vad_threshold", &d)) return false; cfg->vad_threshold = (float)d;
    d = (double)cfg->min_silence_duration_ms; if (!num("min_silence_duration_ms", &d)) return false;
    if (d < 0 || d != std::floor(d)) { *err = "Invalid config: min_silence_duration_ms must be a non-negative integer";
    return false; } cfg->min_silence_duration_ms = (uint64_t)d;
    d = cfg->max_segment_duration_secs; if (!num("max_segment_duration_secs", &d)) return false; cfg->max_segment_duration_secs = (float)d;
    d = (double)cfg->n_threads; if (!num("n_threads", &d)) return false;
    if (d < 0 || d != std::floor(d)) { *err = "Invalid config: n_threads must be a non-negative integer"; return false; } cfg->n_threads = (uint64_t)d;
    {   // gpu_device: an integer as in the reference (lib.rs:31-33), or (additive) the string "auto": instances are dealt round-robin over the visible GPUs
        const skw::JsonValue* x = v.get("gpu_device");
        if (x && x->type == skw::JsonValue::String) { if (x->str != "auto") { *err = "Invalid config: gpu_device must be an integer or \"auto\""; return false; } cfg->gpu_device_auto = true; }
        else { d = cfg->gpu_device; if (!num("gpu_device", &d)) return false; if (d != std::floor(d)) { *err = "Invalid config: gpu_device must be an integer";
        return false; } cfg->gpu_device = (int)d; }
    }
    {   // audio_ctx: an integer, or the string "auto"
        const skw::JsonValue* x = v.get("audio_ctx");
        if (x && x->type == skw::JsonValue::String) { if (x->str != "auto") { *err = "Invalid config: audio_ctx must be an integer or \"auto\""; return false; } cfg->audio_ctx_auto = true; }
        else { d = cfg->audio_ctx; if (!num("audio_ctx", &d)) return false;
               if (d != std::floor(d) || std::fabs(d) > 1e6) { *err = "Invalid config: audio_ctx must be an integer or \"auto\""; return false; } cfg->audio_ctx = (int)d; }
    }
    d = cfg->batch_window_ms; if (!num("batch_window_ms", &d)) return false; cfg->batch_window_ms = (int)d;
    d = cfg->max_batch; if (!num("max_batch", &d)) return false; cfg->max_batch = std::max(1, (int)d);
    if (!boo("use_gpu", &cfg->use_gpu) || !boo("suppress_blank", &cfg->suppress_blank) || !boo("suppress_non_speech_tokens", &cfg->suppress_non_speech_tokens) ||
        !boo("emit_vad_events", &cfg->emit_vad_events) || !boo("flush_tail", &cfg->flush_tail) || !boo("mixed_batch", &cfg->mixed_batch) || !boo("carry_context", &cfg->carry_context)) return false;
    if (const skw::JsonValue* x = v.get("timestamp_granularity")) {
        if (x->type != skw::JsonValue::String || (x->str != "segment" && x->str != "word")) { *err = "Invalid config: timestamp_granularity must be \"segment\" or \"word\""; return false; }
        cfg->word_timestamps = x->str == "word";
    }
    if (const skw::JsonValue* x = v.get("alignment_heads")) {
        const char* msg = "Invalid config: alignment_heads must be \"top:N\" (N >= 1) or an array of [layer, head] pairs (layer 0 .. 31, head 0 .. 31)";
        memset(cfg->align.head_mask, 0, sizeof cfg->align.head_mask); cfg->align_explicit = false; cfg->align_top = 0;
        if (x->type == skw::JsonValue::String) {
            char* end = nullptr; const long n = x->str.compare(0, 4, "top:") == 0 ? strtol(x->str.c_str() + 4, &end, 10) : 0;
            if (n < 1 || n > 32 || !end || *end) { *err = msg; return false; }
            cfg->align_top = (int)n;
        } else if (x->type == skw::JsonValue::Array && !x->arr.empty()) {
            for (const skw::JsonValue& pr : x->arr) {
                if (pr.type != skw::JsonValue::Array || pr.arr.size() != 2 || pr.arr[0].type != skw::JsonValue::Number || pr.arr[1].type != skw::JsonValue::Number) { *err = msg; return false; }
                const double l = pr.arr[0].num, h = pr.arr[1].num;
                if (l != std::floor(l) || h != std::floor(h) || l < 0 || l > 31 || h < 0 || h > 31) { *err = msg; return false; }
                cfg->align.head_mask[(int)l] |= 1u << (int)h;
            }
            cfg->align_explicit = true;
        } else { *err = msg; return false; }
    }
    if (!parse_grammar(v, cfg, err)) return false;
    return parse_decode_rules(v, cfg, err);
}

// ------------------------------------------------------------------ shared engine: model cache + batch scheduler
// One per (model_path, use_gpu, gpu_device) — the key of the reference's WHISPER_CONTEXT_CACHE (lib.rs:175-180, 330).
// Instances submit finished speech segments; a worker thread forms batches and runs skw_full_batch.
// A segment's samples in page-locked memory, so that the engine's H2D copy of the batch is asynchronous DMA (64 x 30 s: ~2.3 ms) and not the driver's staged copy out of pageable
// memory (~6 ms, all of it in front of the first kernel).  Buffers are recycled through a process-wide pool (page-locking is not free: one allocation per first use of a slot).
struct PinnedPool {
    struct Buf { float* p; size_t cap; };
    std::mutex mu; std::vector<Buf> free_; size_t pooled_bytes = 0;
    static PinnedPool& get() { static PinnedPool* pool = new PinnedPool(); return *pool; }      // (leaked on purpose: instances may outlive static destruction order)
    Buf acquire(size_t n) {
        {   std::lock_guard<std::mutex> l(mu); int best = -1;
            for (int i = 0; i < (int)free_.size(); ++i) if (free_[i].cap >= n && (best < 0 || free_[i].cap < free_[best].cap)) best = i;
            if (best >= 0) { Buf b = free_[best]; free_.erase(free_.begin() + best); pooled_bytes -= b.cap * sizeof(float); return b; } }
        const size_t cap = std::max<size_t>((n + 65535) & ~(size_t)65535, 491520);      // at least a 30.72 s segment: the common size comes back from the pool
        return Buf{(float*)skw_host_alloc(cap * sizeof(float)), cap};
    }
    void release(Buf b) {
        if (!b.p) return;
        {   std::lock_guard<std::mutex> l(mu);
            if (pooled_bytes + b.cap * sizeof(float) <= ((size_t)512 << 20)) { free_.push_back(b); pooled_bytes += b.cap * sizeof(float); return; } }
        skw_host_free(b.p);
    }
};
struct Job {
    std::vector<float> pcm_pageable; PinnedPool::Buf pinned{nullptr, 0}; size_t n = 0;
    skw_full_params params; std::promise<int> done; skw_result result{}; std::string error;
    uint32_t* rng = nullptr;      // the owning instance's std::mt19937 stream (WhisperPlugin::rng): continued by this segment's sampled passes, if it needs any
    // the text this segment decodes behind (prompt_past as whisper_full_with_state's window loop finds it: the instance's initial prompt, then what it carries) and, after the call,
    // what the call leaves.  want_ctx: the instance has a prompt or carries context (an instance that carries hands in its context even while it is empty: that is how it gets the
    // first one back); without it the job takes no part in a context call
    int32_t ctx[SKW_CONTEXT_WORDS] = {0}; bool want_ctx = false;
    int32_t* context() { return want_ctx ? ctx : nullptr; }
    skw_decode_rules rules; bool constrained = false;      // the owning instance's decoding constraints when the segment was queued; constrained: they are not the default record
    const skw_decode_rules* decode_rules() const { return constrained ? &rules : nullptr; }
    skw_align_params align; bool want_align = false; skw_token_times times{0, nullptr, nullptr};      // timestamp_granularity "word": the instance's alignment record, the token times
    const skw_align_params* align_params() const { return want_align ? &align : nullptr; }
    std::shared_ptr<skw_grammar> grammar;      // the owning instance's grammar when the segment was queued (null: none); shared, so update_params cannot free it under a batch
    void set_samples(const std::vector<float>& v) {
        n = v.size(); pinned = PinnedPool::get().acquire(n);
        if (pinned.p) memcpy(pinned.p, v.data(), n * sizeof(float)); else pcm_pageable = v;      // (no page-locked memory to be had: the ordinary copy path)
    }
    const float* data() const { return pinned.p ? pinned.p : pcm_pageable.data(); }
    ~Job() { PinnedPool::get().release(pinned); skw_token_times_free(&times); }
};
std::atomic<long> g_engine_calls{0}, g_batch_jobs{0}, g_mixed_calls{0};      // skw_whisper_plugin_batch_stats
std::atomic<long> g_align_calls{0};      // engine calls that aligned at least one job (skw_full_batch_aligned)
std::atomic<long> g_grammar_calls{0};    // engine calls in which at least one job had a grammar (skw_full_batch_grammar)
std::atomic<long> g_context_calls{0}, g_rules_calls{0};                                        // skw_whisper_plugin_context_stats: engine calls that carried at least one context
struct SharedEngine {
    skw_model* model = nullptr;
    skw_ctx* ctx = nullptr;
    int max_batch = 0;          // rows the workspace was created for
    int max_samples = 0;        // samples per row the workspace was created for
    int batch_limit = 64;       // scheduler: largest batch formed (the max_batch param of the instance created most recently; under mu)
    int window_ms = 2;          // scheduler: how long a batch waits for more jobs (batch_window_ms of the instance created most recently; under mu)
    bool multilingual = true;   // the model has language tokens (n_vocab >= 51865); set once at load
    int n_audio_ctx = 1500;     // the model's encoder positions (what audio_ctx "auto" is capped at); set once at load
    int n_text_ctx = 448;       // the model's decoder positions (a prompt takes at most half of them); set once at load
    int n_text_layer = 4, n_text_head = 6;      // the model's decoder geometry (what alignment_heads is resolved against); set once at load
    int n_vocab = 51865;        // the model's vocabulary (what suppress_tokens / logit_bias ids are checked against); set once at load
    bool mixed = true;          // scheduler: jobs join a batch whatever their parameters (mixed_batch of the instance created most recently; under mu)
    int precision = SKW_PRECISION_EXACT;
    int cross_kv = SKW_CROSS_KV_F16;
    // precision and cross_kv of this engine on a workspace just created; false (with the engine's message) when the q8 image cannot be allocated
    bool configure(skw_ctx* c, std::string* err) {
        skw_ctx_set_precision(c, precision);
        if (skw_ctx_set_cross_kv(c, cross_kv) != 0) { if (err) *err = std::string("Failed to create Whisper state: ") + skw_ctx_last_error(c); return false; }
        return true;
    }
    static const int kMaxSamples = 16000 * 121;   // schema maximum of max_segment_duration_secs (120 s) + one VAD frame of slack: no segment is longer
    static int samples_for(float max_segment_secs) { const double s = std::min(120.0, std::max(1.0, (double)max_segment_secs)); return std::min(kMaxSamples, (int)std::ceil(s * 16000.0) + 1024); }
    // The workspace is sized for the longest segment an instance of this engine can cut (its max_segment_duration_secs) and the largest batch one asked
    // for, not for the schema's maxima: 31 s by default instead of 121 (0.2 GB instead of 0.8 at 64 rows).  An instance that allows longer segments or
    // larger batches grows it, between batches (the engine outlives its instances: lib.rs:170-180).
    // Grows to max(configured floor, what was held, what is needed), rounded up (whole seconds, multiples of 8 rows) so that a run of slightly longer segments does not
    // re-create it batch after batch.  When the larger workspace cannot be had, the previous size — or the floor — is restored and only the oversize batch fails.
    int floor_samples = 0, floor_batch = 0;      // what the instances of this engine were configured for (get_engine); the workspace is never smaller while one is alive
    std::mutex ws_mu;                            // the workspace is in use (a batch is running) or being re-created / released
    int live_instances = 0;                      // under ws_mu: plugin instances holding this engine; the last one to go releases the workspace (the MODEL stays, lib.rs:170-180)
    bool ensure_workspace(int need_samples, int need_batch, std::string* err) {
        if (ctx && need_samples <= max_samples && need_batch <= max_batch) return true;
        const int was_s = max_samples, was_b = max_batch;
        const int ns = std::min(kMaxSamples, (std::max(std::max(need_samples, max_samples), floor_samples) + 15999) / 16000 * 16000);
        const int nb = (std::max(std::max(need_batch, max_batch), floor_batch) + 7) & ~7;
        char ebuf[512] = {0};
        if (ctx) { skw_ctx_free(ctx); ctx = nullptr; max_samples = 0; max_batch = 0; }      // release first: two workspaces need not fit side by side
        skw_ctx* nc = skw_ctx_create(model, nb, ns, ebuf, sizeof ebuf);
        if (!nc) {
            *err = std::string("Failed to create Whisper state: ") + ebuf;
            const int rs = std::max(was_s, floor_samples), rb = std::max(was_b, floor_batch);
            if (rs > 0 && rb > 0 && (rs < ns || rb < nb)) {      // back to what there was: later batches of the usual size must not pay for this one
                char e2[512] = {0};
                if (skw_ctx* oc = skw_ctx_create(model, rb, rs, e2, sizeof e2)) {
                    if (configure(oc, nullptr)) { ctx = oc; max_samples = rs; max_batch = rb; } else skw_ctx_free(oc);
                }
            }
            return false;
        }
        if (!configure(nc, err)) { skw_ctx_free(nc); return false; }
        ctx = nc; max_samples = ns; max_batch = nb;
        return true;
    }
    void instance_added() { std::lock_guard<std::mutex> l(ws_mu); ++live_instances; }
    // The reference keeps the CONTEXT (weights) for the life of the process and drops each instance's WhisperState with the instance (lib.rs:160-180, 376-380).  Here the
    // batch workspace plays the state's part for all instances at once: when the last one goes — the prewarm node, or every session after a quiet spell — its device memory
    // (cross / self K-V caches for max_batch rows: 6.6 GB at 64 rows of Whisper-small) is returned; the next batch re-creates it (~3-20 ms, logged by get_engine).
    void instance_gone() {
        std::lock_guard<std::mutex> l(ws_mu);
        if (--live_instances <= 0) { live_instances = 0; if (ctx) { skw_ctx_free(ctx); ctx = nullptr; max_samples = 0; max_batch = 0; } }
    }
    std::mutex mu; std::condition_variable cv; std::deque<std::shared_ptr<Job>> queue; bool stop = false; std::thread worker;
    ~SharedEngine() {
        { std::lock_guard<std::mutex> l(mu); stop = true; } cv.notify_all(); if (worker.joinable()) worker.join();
        if (ctx) skw_ctx_free(ctx); if (model) skw_model_free(model);
    }
    void run() {
        for (;;) {
            std::vector<std::shared_ptr<Job>> batch;
            {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return stop || !queue.empty(); });
                if (stop && queue.empty()) return;
                // batch formation: give concurrent instances a short window to join
                auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(window_ms);
                while ((int)queue.size() < batch_limit && !stop) { if (cv.wait_until(l, deadline) == std::cv_status::timeout) break; }
                while (!queue.empty() && (int)batch.size() < batch_limit) {
                    // arrival order, whatever the jobs' params: every row of skw_full_batch_mixed decodes under its own.  mixed_batch: false cuts at the first job that differs
                    if (!mixed && !batch.empty() && (memcmp(&batch[0]->params, &queue.front()->params, sizeof(skw_full_params)) != 0 ||
                                                     memcmp(&batch[0]->rules, &queue.front()->rules, sizeof(skw_decode_rules)) != 0 ||
                                                     batch[0]->grammar.get() != queue.front()->grammar.get())) break;      // (and where the rules or the grammar differ)
                    batch.push_back(queue.front()); queue.pop_front();
                }
            }
            const int n = (int)batch.size();
            int rc = -1; std::string why;
            try {
                std::vector<const float*> ptrs(n); std::vector<int32_t> ns(n); std::vector<skw_result> res(n); int need = 0;
                for (int i = 0; i < n; ++i) { ptrs[i] = batch[i]->data(); ns[i] = (int32_t)batch[i]->n; need = std::max(need, (int)ns[i]); }
                std::lock_guard<std::mutex> wl(ws_mu);
                if (ensure_workspace(need, n, &why)) {
                    std::vector<uint32_t*> rngs(n); for (int i = 0; i < n; ++i) rngs[i] = batch[i]->rng;
                    std::vector<skw_full_params> pv(n); bool differ = false;
                    for (int i = 0; i < n; ++i) { pv[i] = batch[i]->params; differ = differ || memcmp(&pv[0], &pv[i], sizeof(skw_full_params)) != 0; }
                    // a batch in which no job has a prompt or carries context makes exactly the calls it made before contexts existed; otherwise ONE context call serves it (jobs without
                    // text hand in NULL: their rows are skw_full_batch_mixed's)
                    std::vector<int32_t*> cxs(n); for (int i = 0; i < n; ++i) cxs[i] = batch[i]->context();
                    // (jobs that all share one parameter block run the uniform call: the same launches as before mixed batches existed)
                    // decoding constraints: a batch in which some job has them hands its rules in (jobs without hand in NULL: their rows are the context call's); otherwise as before
                    std::vector<const skw_decode_rules*> rls(n); bool rules_differ = false;
                    for (int i = 0; i < n; ++i) { rls[i] = batch[i]->decode_rules(); rules_differ = rules_differ || memcmp(&batch[0]->rules, &batch[i]->rules, sizeof(skw_decode_rules)) != 0; }
                    // word timestamps: a batch in which some job asks hands its records in (jobs that do not ask hand in NULL: their rows are the rules call's); otherwise as before
                    std::vector<const skw_align_params*> als(n); std::vector<skw_token_times> tms(n, skw_token_times{0, nullptr, nullptr});
                    for (int i = 0; i < n; ++i) als[i] = batch[i]->align_params();
                    // grammars: a batch in which some job has one hands them in (jobs without hand in NULL: their rows are the aligned call's); otherwise as before
                    std::vector<const skw_grammar*> grs(n); for (int i = 0; i < n; ++i) grs[i] = batch[i]->grammar.get();
                    // ONE engine call for jobs [i0, i0 + m) — the whole batch, or one job alone: a feature's array goes in where some job of the span uses it (NULL otherwise; the
                    // generators always), and the launches are the uniform ones exactly where no job of the span uses any and the span shares one parameter block
                    auto used = [](const auto& v, int i0, int m) { for (int i = i0; i < i0 + m; ++i) if (v[i]) return true; return false; };
                    auto call = [&](int i0, int m, bool one_block, skw_result* out, skw_token_times* times) {
                        const bool cx = used(cxs, i0, m), rl = used(rls, i0, m), al = used(als, i0, m), gr = used(grs, i0, m);
                        skw_full_request q{}; q.size = sizeof q; q.params_per_clip = (cx || rl || al || gr || !one_block) ? 1 : 0;
                        q.params = &pv[i0]; q.pcm = &ptrs[i0]; q.n_samples = &ns[i0]; q.n_clips = m; q.rng_state = &rngs[i0]; q.results = out;
                        q.context = cx ? &cxs[i0] : nullptr; q.rules = rl ? &rls[i0] : nullptr; q.align = al ? &als[i0] : nullptr; q.times = al ? times : nullptr;
                        q.grammar = gr ? &grs[i0] : nullptr;
                        return skw_full_batch_request(ctx, &q);
                    };
                    const bool any_ctx = used(cxs, 0, n), any_rules = used(rls, 0, n), any_align = used(als, 0, n), any_gram = used(grs, 0, n);
                    rc = call(0, n, !differ, res.data(), tms.data());
                    g_engine_calls.fetch_add(1); g_batch_jobs.fetch_add(n); if (differ) g_mixed_calls.fetch_add(1); if (any_ctx) g_context_calls.fetch_add(1);
                    if (any_rules) g_rules_calls.fetch_add(1);
                    if (any_align) g_align_calls.fetch_add(1);
                    if (any_gram) g_grammar_calls.fetch_add(1);
                    if (rc == 0) for (int i = 0; i < n; ++i) { batch[i]->result = res[i]; batch[i]->times = tms[i]; } else why = skw_ctx_last_error(ctx);
                    if (rc != 0 && (differ || rules_differ || (any_align && n > 1))) {
                        // A refusal must stay with the request that earned it: jobs of differently configured instances share this call, and one of them being refused
                        // (the engine fails the whole call and hands no generator state back) is no reason for the others to fail.  Each job again, alone, under its own
                        // parameters; every job gets its own outcome.  (Jobs with equal blocks share their configuration, and shared the call before mixed batches too.)
                        for (int i = 0; i < n; ++i) {
                            // (the refused call wrote no context back: each job's own, as it was queued; its rules, alignment record and grammar go with it into its own call)
                            skw_result one{}; skw_token_times tm{0, nullptr, nullptr};
                            int r1 = call(i, 1, true, &one, &tm);
                            g_engine_calls.fetch_add(1);
                            if (r1 == 0) { batch[i]->result = one; batch[i]->times = tm; }
                            else { try { batch[i]->error = skw_ctx_last_error(ctx); } catch (const std::exception&) { r1 = -1; } }      // (a promise is satisfied once)
                            batch[i]->done.set_value(r1);
                        }
                        continue;
                    }
                }
            } catch (const std::exception& e) { rc = -1; why = e.what(); }     // the worker thread must not die with waiters blocked on it
            for (int i = 0; i < n; ++i) { if (rc != 0) batch[i]->error = why; batch[i]->done.set_value(rc); }
        }
    }
};
// WHISPER_CONTEXT_CACHE (lib.rs:170-180): process-global, STRONG references — an entry lives until the library is unloaded or the process exits, so a
// prewarmed model (apps/skit/src/plugins.rs:265-306: "Node is dropped immediately, but ... model loading via Arc persist") and every Oneshot request after
// the first find it loaded.  What is cached here is the whole SharedEngine: the weights with their device images, the batch workspace (the reference's
// per-instance WhisperState has no counterpart: instances share one batched context) and the scheduler thread.
// The map is a function-local static constructed after the HIP runtime is up (skw_device_count makes the first HIP call), so that at process exit it is
// destroyed — workers joined, device memory released — before the runtime's own teardown; a dlclose of the plugin runs the same destructor.
struct EngineCache {
    std::mutex mu;
    std::map<std::string, std::shared_ptr<SharedEngine>> map;
};
EngineCache& engine_cache() { (void)skw_device_count(); static EngineCache c; return c; }
std::atomic<int> g_model_loads{0}, g_cache_hits{0};

struct WhisperPlugin;
std::shared_ptr<SharedEngine> get_engine(const WhisperConfig& cfg, WhisperPlugin* who, std::string* err);
// gpu_device: "auto" (additive): instance k of the process runs on GPU k mod n_gpus — one SharedEngine (model copy + batch scheduler)
// per device, which is how the reference's docs spread pipelines over GPUs by hand (docs/.../deployment/gpu.md:64-66)
std::atomic<unsigned> g_auto_rr{0};
void resolve_auto_device(WhisperConfig* cfg) {
    if (!cfg->gpu_device_auto) return;
    const int n = skw_device_count();
    cfg->gpu_device = n > 0 ? (int)(g_auto_rr.fetch_add(1) % (unsigned)n) : 0;
}

// ------------------------------------------------------------------ the plugin instance (lib.rs:199-221)
struct WhisperPlugin {
    WhisperConfig config; std::shared_ptr<SharedEngine> engine; skw::Segmenter seg; std::unique_ptr<skw::Vad> vad;
    // the engine this instance holds, counted (SharedEngine::live_instances): the last holder to let go returns the batch workspace
    // whisper.cpp keeps one std::mt19937 per whisper_state (seeded with 0 at whisper_init_state) for the temperature ladder's draws and lets it run on across calls; the
    // reference creates one state per instance (lib.rs:377-379) and a new one when update_params swaps the context (lib.rs:520-535).  This is that generator: every segment of
    // this instance continues it (skw_full_batch_rng), whichever batch the segment lands in.
    uint32_t rng[SKW_RNG_STATE_WORDS];
    // whisper.cpp's other per-state memory: prompt_past, the text a call leaves for the next one when no_context is false.  context[0] = n, then n ids, oldest first — what this
    // instance's last segment handed back (carry_context), WITHOUT the initial prompt, which goes in front of it again for every segment as whisper_full_with_state does.
    // An instance never has two segments in flight: plugin_process_packet (and plugin_flush) run transcribe_and_emit on the caller's thread and wait there on the job's promise
    // before the segmenter hands over the next cut, and the host serialises the calls on one instance.  Segment n + 1 therefore always sees what segment n left.
    int32_t context[SKW_CONTEXT_WORDS] = {0};
    std::vector<int32_t> prompt_tokens; bool prompt_ready = false;      // initial_prompt tokenised with this instance's model: once, and again when either changes
    void hold(std::shared_ptr<SharedEngine> e) {
        if (e) e->instance_added(); if (engine) engine->instance_gone(); engine = std::move(e); skw_rng_state_init(rng);
        context[0] = 0; prompt_ready = false;      // a new state starts with no text, and another model may tokenise the prompt differently
    }
    ~WhisperPlugin() { if (engine) engine->instance_gone(); }
    std::unique_ptr<skw::ResamplerCore> front;      // input_sample_rate != 16000: the audio::resampler node's arithmetic on the GPU, feeding the segmenter
    CLogCallback log_cb = nullptr; void* log_ud = nullptr;
    void log(CLogLevel lv, const char* fmt, ...) {
        if (!log_cb) return; char buf[1024]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        log_cb(lv, "whisper_plugin_native", buf, log_ud);
    }
};

// initial_prompt -> tokens (whisper_tokenize); a prompt longer than half the decoder's context keeps its END, as whisper_full_with_state's own cut of prompt_past would
void ensure_prompt_tokens(WhisperPlugin* self) {
    if (self->prompt_ready) return;
    self->prompt_tokens.clear(); self->prompt_ready = true;
    if (self->config.initial_prompt.empty()) return;
    std::vector<int32_t> ids(64);
    int n = skw_model_tokenize(self->engine->model, self->config.initial_prompt.c_str(), ids.data(), (int)ids.size());
    if (n < 0) { ids.resize((size_t)-n); n = skw_model_tokenize(self->engine->model, self->config.initial_prompt.c_str(), ids.data(), (int)ids.size()); }
    if (n < 0) n = 0;
    ids.resize((size_t)n);
    const int cap = self->engine->n_text_ctx / 2;
    if (n > cap) {
        self->log(SK_LOG_WARN, "initial_prompt is %d tokens; only its last %d (half the model's text context) condition decoding", n, cap);
        ids.erase(ids.begin(), ids.end() - cap);
    }
    self->prompt_tokens = ids;
}
// The context a segment is queued with (whisper_full_with_state before its window loop): no carry -> the carried part is cleared (no_context); then the prompt's tokens go to the
// FRONT (whisper.cpp: push_back + rotate); when the total exceeds what the engine takes, the oldest tokens behind the prompt go.
void build_job_context(WhisperPlugin* self, int32_t* out) {
    ensure_prompt_tokens(self);
    const int cap = SKW_CONTEXT_WORDS - 1, np = (int)self->prompt_tokens.size();
    int nc = self->config.carry_context ? self->context[0] : 0;
    if (np + nc > cap) nc = cap - np;
    out[0] = np + nc;
    for (int i = 0; i < np; ++i) out[1 + i] = self->prompt_tokens[i];
    for (int i = 0; i < nc; ++i) out[1 + np + i] = self->context[1 + self->context[0] - nc + i];
}

std::shared_ptr<SharedEngine> get_engine(const WhisperConfig& cfg, WhisperPlugin* who, std::string* err) {
    char keybuf[96];
    // the reference's key (path, use_gpu, gpu_device) + the additive precision and cross_kv
    snprintf(keybuf, sizeof keybuf, "|%d|%d|%s|%s", cfg.use_gpu ? 1 : 0, cfg.gpu_device, cfg.precision.c_str(), cfg.cross_kv.c_str());
    const std::string key = cfg.model_path + keybuf;
    EngineCache& cache = engine_cache();
    std::unique_lock<std::mutex> l(cache.mu);
    auto it = cache.map.find(key);
    if (it != cache.map.end()) {
        g_cache_hits.fetch_add(1);
        // ws_mu is held for the whole of a running batch: the cache's mutex is let go first, so that creating an instance of ANOTHER engine (or reading the statistics)
        // does not wait behind this engine's batch (entries are never removed from the map: the pointer stays good)
        const std::shared_ptr<SharedEngine> e = it->second;
        l.unlock();
        // additive scheduler params: the most recent instance's
        { std::lock_guard<std::mutex> le(e->mu); e->batch_limit = cfg.max_batch; e->window_ms = cfg.batch_window_ms; e->mixed = cfg.mixed_batch; }
        { std::lock_guard<std::mutex> lw(e->ws_mu);      // the floor follows the largest configuration seen; the workspace itself grows (or comes back) with the next batch
          e->floor_samples = std::max(e->floor_samples, SharedEngine::samples_for(cfg.max_segment_duration_secs));
          e->floor_batch = std::max(e->floor_batch, cfg.max_batch);
          // an engine whose last instance had gone gets its workspace back here, at instance creation — where the reference creates a WhisperState (lib.rs:377-379) — not inside the first batch
          if (!e->ctx && !e->ensure_workspace(e->floor_samples, e->floor_batch, err)) return nullptr; }
        if (who) who->log(SK_LOG_INFO, "CACHE HIT: Reusing cached Whisper context (model_path=%s, gpu_device=%d, precision=%s)", cfg.model_path.c_str(), cfg.gpu_device, cfg.precision.c_str());
        return e;
    }
    if (who) who->log(SK_LOG_INFO, "CACHE MISS: Loading Whisper model (model_path=%s, gpu_device=%d, precision=%s)", cfg.model_path.c_str(), cfg.gpu_device, cfg.precision.c_str());
    char ebuf[512] = {0};
    auto eng = std::make_shared<SharedEngine>();
    const auto t0 = std::chrono::steady_clock::now();
    eng->model = skw_model_load(cfg.model_path.c_str(), cfg.gpu_device, ebuf, sizeof ebuf);
    if (!eng->model) { *err = ebuf[0] ? ebuf : ("Failed to load Whisper model from '" + cfg.model_path + "'"); return nullptr; }
    g_model_loads.fetch_add(1);
    { skw_hparams hp{}; skw_model_get_hparams(eng->model, &hp); eng->multilingual = hp.n_vocab >= 51865; eng->n_audio_ctx = hp.n_audio_ctx; eng->n_text_ctx = hp.n_text_ctx;
      eng->n_text_layer = hp.n_text_layer; eng->n_text_head = hp.n_text_head;
      eng->n_vocab = hp.n_vocab; }
    const auto t1 = std::chrono::steady_clock::now();
    eng->batch_limit = cfg.max_batch;
    eng->window_ms = cfg.batch_window_ms; eng->mixed = cfg.mixed_batch;
    eng->precision = cfg.precision == "f16_mfma" ? SKW_PRECISION_F16_MFMA : SKW_PRECISION_EXACT;
    eng->cross_kv = cfg.cross_kv == "q8_0" ? SKW_CROSS_KV_Q8_0 : SKW_CROSS_KV_F16;
    eng->floor_samples = SharedEngine::samples_for(cfg.max_segment_duration_secs); eng->floor_batch = cfg.max_batch;
    if (!eng->ensure_workspace(eng->floor_samples, eng->floor_batch, err)) return nullptr;
    const auto t2 = std::chrono::steady_clock::now();
    eng->worker = std::thread([e = eng.get()] { e->run(); });
    cache.map[key] = eng;
    if (who) who->log(SK_LOG_INFO, "Whisper model loaded and cached (model_load_ms=%.1f, ctx_create_ms=%.1f, max_batch=%d)",
                      std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(), cfg.max_batch);
    return eng;
}

// Silero gate behind the segmenter's Vad interface; the weights of one file are shared by every instance that names it and, like the Whisper
// context, stay cached for the life of the process
struct SileroGate : skw::Vad {
    skw::SileroVad v;
    explicit SileroGate(std::shared_ptr<const skw::SileroWeights> w) : v(std::move(w)) {}
    float process_chunk(const float* f) override { return v.process_chunk(f); }
    void reset() override { v.reset(); }
};
// vad_device "gpu": the same network in the contract arithmetic.  Calls of at least kGpuMinFrames frames go to the device context of (file, device) — one per
// process, shared by every instance, serialised inside skw_vad_gpu_process — smaller ones to the CPU contract evaluator, which gives the same bits: where a
// call is evaluated is invisible in the result.  The stream's state lives in the CPU evaluator and travels with each GPU call.
constexpr size_t kGpuMinFrames = 8;
struct SileroGpuGate : skw::Vad {
    skw::SileroContractVad v; skw_vad_gpu* gpu;
    SileroGpuGate(std::shared_ptr<const skw::SileroWeights> w, skw_vad_gpu* g) : v(std::move(w)), gpu(g) {}
    float process_chunk(const float* f) override { return v.process_chunk(f); }
    void process_chunks(const float* frames, size_t n, float* probs) override {
        if (n < kGpuMinFrames) { v.process_chunks(frames, n, probs); return; }
        float st[320]; v.get_state(st);
        const float* fp[1] = {frames}; const int32_t nf[1] = {(int32_t)n}; float* sp[1] = {st}; float* pp[1] = {probs};
        if (skw_vad_gpu_process(gpu, 1, fp, nf, sp, pp) != 0)
            throw std::runtime_error(std::string("Silero VAD on the GPU failed: ") + skw_vad_gpu_last_error(gpu));   // no fall-back; guarded() reports it
        v.set_state(st);
    }
    void reset() override { v.reset(); }
};
std::mutex g_vad_mu;
std::map<std::string, std::shared_ptr<const skw::SileroWeights>> g_vad_cache;
std::map<std::string, skw_vad_gpu*> g_vad_gpu_cache;      // (file, device) -> device context, kept for the life of the process like the Whisper contexts
skw_vad_gpu* get_silero_gpu(const std::string& path, int device, std::string* err) {
    std::lock_guard<std::mutex> l(g_vad_mu);
    const std::string key = path + "|" + std::to_string(device);
    auto it = g_vad_gpu_cache.find(key);
    if (it != g_vad_gpu_cache.end()) return it->second;
    char ebuf[512] = {0};
    skw_vad_gpu* g = skw_vad_gpu_create(path.c_str(), device, ebuf, sizeof ebuf);
    if (!g) { *err = ebuf; return nullptr; }
    g_vad_gpu_cache[key] = g;
    return g;
}
std::shared_ptr<const skw::SileroWeights> get_silero(const std::string& path, std::string* err) {
    std::lock_guard<std::mutex> l(g_vad_mu);
    auto it = g_vad_cache.find(path);
    if (it != g_vad_cache.end()) return it->second;
    auto w = std::make_shared<skw::SileroWeights>();
    try { if (!skw::SileroVad::load_weights(path, w.get(), err)) return nullptr; }
    catch (const std::exception& e) { *err = "Failed to load VAD model from '" + path + "': " + e.what(); return nullptr; }     // a malformed file must not unwind across the C ABI
    g_vad_cache[path] = w;
    return w;
}

// SileroVAD::new at lib.rs:382-383 ("Failed to initialize VAD: {e}") / :557-560 ("Failed to reload VAD: {e}", added by the caller)
std::unique_ptr<skw::Vad> make_silero_gate(const WhisperConfig& cfg, std::shared_ptr<const skw::SileroWeights> w, std::string* err) {
    if (cfg.vad_device != "gpu") return std::unique_ptr<skw::Vad>(new SileroGate(w));
    skw_vad_gpu* g = get_silero_gpu(cfg.vad_model_path, cfg.gpu_device, err);
    if (!g) return nullptr;                                                        // a gate that was asked to run on the GPU and cannot is an error, never a quiet CPU gate
    return std::unique_ptr<skw::Vad>(new SileroGpuGate(w, g));
}
std::unique_ptr<skw::Vad> make_vad(const WhisperConfig& cfg, WhisperPlugin* p, std::string* err) {
    std::string mode = cfg.vad_mode;
    if (mode == "auto") {
        struct stat sb;
        if (stat(cfg.vad_model_path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) {
            // The file is there: run it — unless this build cannot read it (the graph is restated from the published v5 layout and has only ever
            // seen files of tools/make_synth_silero.py's making; the reference names v6, vad.rs:5).  In auto mode that is a warning and the energy
            // gate, not a node that fails to start; `vad_mode: "silero"` keeps the reference's hard failure.
            std::string e; auto w = get_silero(cfg.vad_model_path, &e);
            if (w) {
                if (p) p->log(SK_LOG_INFO, "Silero VAD: %s", w->bound.c_str());
                auto gate = make_silero_gate(cfg, w, &e);
                if (!gate) *err = "Failed to initialize VAD: " + e;
                return gate;
            }
            if (p) p->log(SK_LOG_WARN, "%s; using vad_mode=energy (set vad_mode to \"silero\" to make this an error)", e.c_str());
            mode = "energy";
        } else {
            // the reference fails here; this build keeps running on an energy gate and says so (header comment)
            if (p) p->log(SK_LOG_WARN, "Silero VAD model '%s' not found; using vad_mode=energy (set vad_mode to \"silero\" to make this an error)", cfg.vad_model_path.c_str());
            mode = "energy";
        }
    }
    if ((mode == "always" || mode == "energy") && cfg.vad_device == "gpu" && p)
        p->log(SK_LOG_INFO, "vad_device \"gpu\" is unused with vad_mode=%s (only the Silero gate runs on the GPU)", mode.c_str());
    if (mode == "always") return std::unique_ptr<skw::Vad>(new skw::AlwaysSpeechVad());
    if (mode == "energy") return std::unique_ptr<skw::Vad>(new skw::EnergyVad());
    if (mode == "silero") {
        std::string e; auto w = get_silero(cfg.vad_model_path, &e);
        if (!w) { *err = "Failed to initialize VAD: " + e; return nullptr; }
        if (p) p->log(SK_LOG_INFO, "Silero VAD: %s", w->bound.c_str());
        auto gate = make_silero_gate(cfg, w, &e);
        if (!gate) *err = "Failed to initialize VAD: " + e;
        return gate;
    }
    *err = "Failed to initialize VAD: unknown vad_mode '" + mode + "'"; return nullptr;
}

struct Emit {
    COutputCallback out_cb; void* out_ud; CTelemetryCallback tel_cb; void* tel_ud;
    // OutputSender::send (sdk lib.rs:200-223)
    bool send_transcription(const std::string& json, std::string* err) const {
        CPacket pk; pk.packet_type = SK_PACKET_TRANSCRIPTION; pk.data = json.data(); pk.len = json.size();
        CResult r = out_cb("out", &pk, out_ud);
        if (r.success) return true;
        *err = r.error_message ? std::string(r.error_message) : std::string("Unknown error"); return false;
    }
    // OutputSender::emit_telemetry (sdk lib.rs:237-283): best effort, errors ignored by the caller (lib.rs:438 `let _ =`)
    void telemetry(const char* event, const std::string& json) const { if (tel_cb) (void)tel_cb(event, (const uint8_t*)json.data(), json.size(), nullptr, tel_ud); }
};

// transcribe_and_emit (lib.rs:582-702)
bool transcribe_and_emit(WhisperPlugin* self, const Emit& em, const skw::SegmentCut& cut, std::string* err) {
    if (cut.samples.empty()) return true;
    if (self->config.emit_vad_events && !cut.segment_id.empty()) {
        std::string j = "{\"duration_ms\":" + std::to_string(cut.end_time_ms >= cut.start_time_ms ? cut.end_time_ms - cut.start_time_ms : 0) +
                        ",\"end_time_ms\":" + std::to_string(cut.end_time_ms) + ",\"reason\":" + skw::json_quote(cut.reason) + ",\"segment_id\":" + skw::json_quote(cut.segment_id) +
                        ",\"silence_duration_ms\":" + (cut.has_silence_duration ? std::to_string(cut.silence_duration_ms) : std::string("null")) +
                        ",\"start_time_ms\":" + std::to_string(cut.start_time_ms) + "}";
        em.telemetry("vad.speech_end", j);
    }
    auto job = std::make_shared<Job>();
    job->set_samples(cut.samples);
    skw_full_default_params(&job->params);
    int lang = self->config.language == "auto" ? -1 : skw_model_lang_id(self->config.language.c_str());     // "auto": whisper.cpp detects it from the first window
    if (lang < 0 && self->config.language != "auto") { *err = "Whisper inference failed: unknown language '" + self->config.language + "'"; return false; }
    // an English-only model cannot detect a language (whisper.cpp: "failed to auto-detect language"): this request's own error, raised before its segment joins a batch
    if (lang < 0 && !self->engine->multilingual) { *err = "Whisper inference failed: failed to auto-detect language: the model is not multilingual"; return false; }
    job->params.lang_id = lang; job->params.translate = 0;
    job->params.suppress_blank = self->config.suppress_blank ? 1 : 0; job->params.suppress_nst = self->config.suppress_non_speech_tokens ? 1 : 0;
    job->params.n_threads = (int32_t)self->config.n_threads;
    // (additive) the segment's audio context: what its instance is configured for now (update_params takes effect from the next segment); "auto" = the exported rule on its length
    job->params.audio_ctx = self->config.audio_ctx_auto ? skw_audio_ctx_for_samples((int)job->n, self->engine->n_audio_ctx) : self->config.audio_ctx;
    job->rng = self->rng;
    job->rules = self->config.rules; job->constrained = !skw_decode_rules_is_default(&job->rules);      // (additive) what the instance is configured for now, like audio_ctx
    job->grammar = self->config.grammar;      // (additive) the instance's grammar as it is configured now: update_params takes effect from the next segment
    if (self->config.word_timestamps) {      // (additive) the instance's alignment record as it is configured now; "top:N" is resolved against the loaded model
        job->align = self->config.align; job->align.enabled = 1; job->want_align = true;
        if (!self->config.align_explicit) { const int L = self->engine->n_text_layer;
            skw_align_heads_top(L, self->engine->n_text_head, self->config.align_top > 0 ? self->config.align_top : std::max(1, L / 2), job->align.head_mask); }
    }
    build_job_context(self, job->ctx); job->want_ctx = self->config.carry_context || job->ctx[0] > 0;
    if ((int)job->n > SharedEngine::kMaxSamples) { *err = "Whisper inference failed: segment longer than the engine workspace"; return false; }
    std::future<int> fut = job->done.get_future();
    { std::lock_guard<std::mutex> l(self->engine->mu); self->engine->queue.push_back(job); }
    self->engine->cv.notify_all();
    int rc = fut.get();
    if (rc != 0) { *err = "Whisper inference failed: " + job->error; return false; }
    // what the call left is this instance's carried text from here on (a failed call hands nothing back: the carried part stays as it was); without carry nothing is kept
    if (self->config.carry_context) memcpy(self->context, job->ctx, sizeof self->context); else self->context[0] = 0;
    // segments with absolute timestamps (lib.rs:648-677)
    struct Seg { std::string text; uint64_t t0, t1; };
    std::vector<Seg> segs;
    const skw_result& R = job->result;
    std::vector<Seg> words;      // timestamp_granularity "word": one segment per word (skw_words.h) — a host deserialising TranscriptionSegment would drop any extra key
    const bool words_ok = job->want_align && job->times.n == R.n_tokens;
    if (job->want_align && !words_ok) self->log(SK_LOG_WARN, "Word timestamps: %d token times for %d tokens; emitting segments", (int)job->times.n, (int)R.n_tokens);
    if (words_ok) {
        std::vector<SkwWordTok> wt; std::vector<std::string> keep; keep.reserve((size_t)R.n_tokens);
        bool after_ts = true;
        for (int k = 0; k < R.n_tokens; ++k) {
            if (job->times.t0[k] < 0) { after_ts = true; continue; }      // (a timestamp token, or a token of a window that was not aligned: the next text token starts a word)
            int len = 0; const char* tx = skw_model_token_text(self->engine->model, R.tokens[k].id, &len);
            keep.emplace_back(tx ? tx : "", tx ? (size_t)len : 0);
            wt.push_back(SkwWordTok{keep.back().data(), (int)keep.back().size(), job->times.t0[k], job->times.t1[k], after_ts});
            after_ts = false;
        }
        for (const SkwWord& w : skw_words_cut(wt.data(), (int)wt.size())) {
            if (!skw::utf8_valid(w.text)) continue;
            words.push_back(Seg{w.text, cut.start_time_ms + (uint64_t)(w.start * 10), cut.start_time_ms + (uint64_t)(w.end * 10)});
        }
    }
    for (int i = 0; i < R.n_segments; ++i) {
        std::string text(R.text + R.segments[i].text_off, (size_t)R.segments[i].text_len);
        if (!skw::utf8_valid(text)) { self->log(SK_LOG_WARN, "Failed to get segment text: invalid UTF-8"); continue; }
        std::string trimmed = skw::utf8_trim(text);
        if (trimmed.empty()) continue;
        const uint64_t rel0 = (uint64_t)(R.segments[i].t0 * 10), rel1 = (uint64_t)(R.segments[i].t1 * 10);   // `as u64` of an i64
        segs.push_back(Seg{trimmed, cut.start_time_ms + rel0, cut.start_time_ms + rel1});
    }
    if (segs.empty()) self->log(SK_LOG_WARN, "Whisper inference produced no segments");
    else {
        std::string full; for (size_t i = 0; i < segs.size(); ++i) { if (i) full += " "; full += segs[i].text; }
        // serde_json::to_vec(TranscriptionData) (crates/core/src/types.rs:150-175): field order of the structs
        std::string j = "{\"text\":" + skw::json_quote(full) + ",\"segments\":[";
        if (words_ok) segs.swap(words);      // (text stays the full text of the segments)
        for (size_t i = 0; i < segs.size(); ++i) {
            if (i) j += ",";
            j += "{\"text\":" + skw::json_quote(segs[i].text) + ",\"start_time_ms\":" + std::to_string(segs[i].t0) + ",\"end_time_ms\":" + std::to_string(segs[i].t1) + ",\"confidence\":null}";
        }
        j += "],\"language\":" + skw::json_quote(self->config.language) + ",\"metadata\":null}";
        skw_result_free(&job->result);
        if (!em.send_transcription(j, err)) return false;
        return true;
    }
    skw_result_free(&job->result);
    return true;
}

void emit_speech_start(WhisperPlugin* self, const Emit& em, const skw::SpeechStart& s) {
    if (!self->config.emit_vad_events) return;
    std::string j = "{\"segment_id\":" + skw::json_quote(s.segment_id) + ",\"speech_probability\":" + skw::json_f32(s.probability) +
                    ",\"start_time_ms\":" + std::to_string(s.start_time_ms) + ",\"threshold\":" + skw::json_f32(s.threshold) + "}";
    em.telemetry("vad.speech_start", j);
}

// ------------------------------------------------------------------ metadata (lib.rs:224-320)
const char* const kDescription =
    "Real-time speech-to-text transcription using OpenAI's Whisper model. Features VAD-based segmentation for natural speech boundaries, "
    "GPU acceleration support, and streaming output. Requires 16kHz mono audio input.";
const char* const kSchema =
    "{\"type\":\"object\",\"properties\":{"
    "\"model_path\":{\"type\":\"string\",\"description\":\"Path to Whisper GGML model file (relative to repo root). IMPORTANT: Input audio must be 16kHz mono f32.\",\"default\":\"models/ggml-base.en-q5_1.bin\"},"
    "\"language\":{\"type\":\"string\",\"description\":\"Language code (e.g., 'en', 'es', 'fr')\",\"default\":\"en\"},"
    "\"vad_model_path\":{\"type\":\"string\",\"description\":\"Path to Silero VAD ONNX model file\",\"default\":\"models/silero_vad.onnx\"},"
    "\"vad_threshold\":{\"type\":\"number\",\"description\":\"VAD speech probability threshold (0.0-1.0)\",\"default\":0.5,\"minimum\":0.0,\"maximum\":1.0},"
    "\"min_silence_duration_ms\":{\"type\":\"integer\",\"description\":\"Minimum silence duration before transcription (milliseconds)\",\"default\":700,\"minimum\":100,\"maximum\":5000},"
    "\"max_segment_duration_secs\":{\"type\":\"number\",\"description\":\"Maximum segment duration before forced transcription (seconds)\",\"default\":30.0,\"minimum\":5.0,\"maximum\":120.0},"
    "\"n_threads\":{\"type\":\"integer\",\"description\":\"Number of threads for decoding (0 = auto: min(4, num_cores), 8-12 recommended for modern CPUs)\",\"default\":0,\"minimum\":0,\"maximum\":32},"
    "\"use_gpu\":{\"type\":\"boolean\",\"description\":\"Enable GPU acceleration (this build always runs on the MI355X selected by gpu_device)\",\"default\":false},"
    "\"gpu_device\":{\"type\":[\"integer\",\"string\"],\"description\":\"GPU device ID to use (0 = first GPU, 1 = second GPU, etc.); (additive) \\\"auto\\\" deals instances round-robin over the visible GPUs\",\"default\":0,\"minimum\":0,\"maximum\":7},"
    "\"suppress_blank\":{\"type\":\"boolean\",\"description\":\"Suppress blank/silent audio segments\",\"default\":true},"
    "\"suppress_non_speech_tokens\":{\"type\":\"boolean\",\"description\":\"Suppress non-speech tokens like [BLANK_AUDIO], [MUSIC], [APPLAUSE], etc.\",\"default\":true},"
    "\"emit_vad_events\":{\"type\":\"boolean\",\"description\":\"Emit VAD speech start/end out-of-band to the telemetry bus (does not flow through graph pins).\",\"default\":false},"
    "\"vad_mode\":{\"type\":\"string\",\"description\":\"(additive) auto (Silero when vad_model_path exists, else an energy gate) | silero | energy | always\",\"default\":\"auto\"},"
    "\"vad_device\":{\"type\":\"string\",\"description\":\"(additive) cpu (the Silero gate frame by frame on the host) | gpu (the Silero gate in the bit-exact contract arithmetic on the GPU of gpu_device; unused with the energy / always gates)\",\"default\":\"cpu\"},"
    "\"vad_batch_frames\":{\"type\":\"integer\",\"description\":\"(additive) complete 512-sample frames held back before the VAD gate evaluates them in one call; cuts, ids and timestamps do not depend on it, a cut is handed over up to N-1 frames (32 ms each) later; file transcription sets 64 or more\",\"default\":1,\"minimum\":1,\"maximum\":65536},"
    "\"precision\":{\"type\":\"string\",\"description\":\"(additive) exact (f32-chain contractions, bit-reproducible; block-quantised model files run ggml's q8 arithmetic) | f16_mfma (f16 matrix cores; quantised files as their f16 twin)\",\"default\":\"exact\"},"
    "\"cross_kv\":{\"type\":\"string\",\"description\":\"(additive) f16 | q8_0: the decode steps read the window's cross K/V as ggml q8_0 blocks, half the bytes of every step; needs precision f16_mfma\",\"default\":\"f16\"},"
    "\"batch_window_ms\":{\"type\":\"integer\",\"description\":\"(additive) how long the per-GPU scheduler waits for concurrent instances before launching a batch\",\"default\":2},"
    "\"max_batch\":{\"type\":\"integer\",\"description\":\"(additive) largest number of segments transcribed in one GPU batch\",\"default\":64},"
    "\"audio_ctx\":{\"type\":[\"integer\",\"string\"],\"description\":\"(additive) whisper.cpp's audio_ctx per segment: 0 = the model's 1500 positions (30 s); N = encode and attend only N positions (20 ms each: the audio beyond N/50 s is not heard); \\\"auto\\\" = the positions the segment covers + 0.5 s, in 32-position blocks. Segments with different values share a batch\",\"default\":0},"
    "\"mixed_batch\":{\"type\":\"boolean\",\"description\":\"(additive) segments of instances with different language / suppress_* settings share one GPU batch; false cuts a batch at the first differing job\",\"default\":true},"
    "\"initial_prompt\":{\"type\":\"string\",\"description\":\"(additive) whisper.cpp's initial_prompt: text (domain vocabulary, spellings) every segment is decoded behind; tokenised with whisper.cpp's tokenizer, which puts nothing in front of it (start it with a space to match openai's reference); at most half the model's text context (224 tokens), longer prompts keep their end\",\"default\":\"\"},"
    "\"carry_context\":{\"type\":\"boolean\",\"description\":\"(additive) whisper.cpp's no_context = false: the text of this instance's previous segment conditions the next one; cleared when model_path, language or initial_prompt change\",\"default\":false},"
    "\"timestamp_granularity\":{\"type\":\"string\",\"description\":\"(additive) segment: the reference's output; word: one segment per word, timed by cross-attention DTW (whisper.cpp dtw_token_timestamps, openai word_timestamps); text stays the full text\",\"default\":\"segment\",\"enum\":[\"segment\",\"word\"]},"
    "\"alignment_heads\":{\"description\":\"(additive) the cross-attention heads word timestamps are read from: top:N (every head of the top N decoder layers; default: half the layers) or an array of [layer, head] pairs\",\"default\":\"top:half\"},"
    "\"repetition_penalty\":{\"type\":\"number\",\"description\":\"(additive) repetition penalty on the text tokens the current window has already produced (timestamps and the prompt are exempt): a logit x becomes x / p when positive, x * p when negative, once per distinct token; 1.0 = off. As in faster-whisper / transformers\",\"default\":1.0,\"exclusiveMinimum\":0.0},"
    "\"no_repeat_ngram_size\":{\"type\":\"integer\",\"description\":\"(additive) no n-gram of this many text tokens occurs twice within a window (timestamps in between are skipped); 0 = off\",\"default\":0,\"minimum\":0},"
    "\"suppress_tokens\":{\"type\":\"array\",\"items\":{\"type\":\"integer\",\"minimum\":0},\"description\":\"(additive) token ids that are never produced (the id-level form of whisper.cpp's suppress_regex); with logit_bias at most 256 distinct ids, each below the model's vocabulary size\",\"default\":[]},"
    "\"logit_bias\":{\"type\":\"array\",\"items\":{\"type\":\"array\",\"minItems\":2,\"maxItems\":2},\"description\":\"(additive) [token id, bias] pairs: the bias is added to the token's logit at every sampling decision; an id also under suppress_tokens stays suppressed. Segments with different decoding rules share a batch\",\"default\":[]},"
    "\"grammar\":{\"type\":\"string\",\"description\":\"(additive) a pattern every segment's text has to match in full (whisper.cpp's grammar_rules, restricted to REGULAR languages: a regular expression over bytes — literals, escapes, \\\\d \\\\w \\\\s, ., [...], groups, |, ? * + {m,n}). Tokens that cannot continue a match lose grammar_penalty logits, the end of the text loses it while the match is incomplete. The match restarts in every 30 s window and ignores timestamps: meant for short utterances. Not with grammar_choices. Segments with and without grammars share a batch\",\"default\":\"\"},"
    "\"grammar_choices\":{\"type\":\"array\",\"items\":{\"type\":\"string\"},\"description\":\"(additive) the grammar as a list of allowed utterances (commands, names, yes / no): compiled as ' ?(c1|c2|...)[.!?]?' with each choice matched literally\",\"default\":[]},"
    "\"grammar_ignore_case\":{\"type\":\"boolean\",\"description\":\"(additive) ASCII letters of the grammar match either case\",\"default\":false},"
    "\"grammar_penalty\":{\"type\":\"number\",\"description\":\"(additive) whisper.cpp's grammar_penalty: what a token that does not fit the grammar loses; finite on purpose (a token the grammar dislikes can still win when nothing that fits is left)\",\"default\":100.0,\"exclusiveMinimum\":0.0},"
    "\"flush_tail\":{\"type\":\"boolean\",\"description\":\"(additive) transcribe buffered speech when the input stream ends (the reference drops it)\",\"default\":false},"
    "\"input_sample_rate\":{\"type\":\"integer\",\"description\":\"(additive) sample rate of the mono f32 packets fed to this node; anything but 16000 is resampled to 16 kHz on the GPU with the audio::resampler node's arithmetic (chunk_frames 960) before VAD segmentation\",\"default\":16000,\"minimum\":1000,\"maximum\":768000},"
    "\"input_resample_mode\":{\"type\":\"string\",\"description\":\"(additive) linear (rubato FastFixedIn/Linear, bit for bit what audio::resampler gives) | polyphase (Kaiser-windowed sinc)\",\"default\":\"linear\"}"
    "}}";

const CAudioFormat kInFormat = {16000, 1, SK_SAMPLE_F32};
// the reference's one accepted type first; (additive) mono f32 at any rate (0 = wildcard, packet_meta.rs:97-109) so that a graph with
// `input_sample_rate: 48000` passes the host's connection check — the rate is validated per packet either way (lib.rs:183-197)
const CAudioFormat kInAnyRate = {0, 1, SK_SAMPLE_F32};
const CPacketTypeInfo kInTypes[2] = {{SK_PACKET_RAW_AUDIO, &kInFormat, nullptr}, {SK_PACKET_RAW_AUDIO, &kInAnyRate, nullptr}};
const CInputPin kInputs[1] = {{"in", kInTypes, 2}};
const COutputPin kOutputs[1] = {{"out", {SK_PACKET_TRANSCRIPTION, nullptr, nullptr}}};
const char* const kCategories[3] = {"ml", "speech", "transcription"};
const CNodeMetadata kMetadata = {"whisper", kDescription, kInputs, 1, kOutputs, 1, kSchema, kCategories, 3};

// ------------------------------------------------------------------ the six entry points (sdk lib.rs:462-854)
const CNodeMetadata* plugin_get_metadata() { return &kMetadata; }

CPluginHandle create_instance_impl(const char* params, CLogCallback log_cb, void* log_ud) {
    auto p = std::unique_ptr<WhisperPlugin>(new WhisperPlugin()); p->log_cb = log_cb; p->log_ud = log_ud;
    std::string err;
    if (!parse_config(params, &p->config, &err)) { p->log(SK_LOG_ERROR, "%s", err.c_str()); return nullptr; }
    resolve_auto_device(&p->config);
    p->hold(get_engine(p->config, p.get(), &err));
    if (!p->engine) { p->log(SK_LOG_ERROR, "%s", err.c_str()); return nullptr; }
    if (!check_rule_ids(p->config, p->engine->n_vocab, &err)) { p->log(SK_LOG_ERROR, "%s", err.c_str()); return nullptr; }
    p->vad = make_vad(p->config, p.get(), &err);
    if (!p->vad) { p->log(SK_LOG_ERROR, "%s", err.c_str()); return nullptr; }
    p->seg.configure(p->config.vad_threshold, p->config.min_silence_duration_ms, p->config.max_segment_duration_secs);
    p->seg.set_batch_frames((size_t)p->config.vad_batch_frames);
    if (p->config.input_sample_rate != 16000) {
        p->front.reset(new skw::ResamplerCore());
        p->front->target = 16000; p->front->chunk_frames = 960; p->front->out_frame = 0;
        p->front->gpu_device = p->config.gpu_device; p->front->polyphase = p->config.input_resample_mode == "polyphase";
    }
    return (CPluginHandle)p.release();
}
CPluginHandle plugin_create_instance(const char* params, CLogCallback log_cb, void* log_ud) {
    auto fail = [&](const std::string& m) -> CPluginHandle { if (log_cb) log_cb(SK_LOG_ERROR, "whisper_plugin_native", m.c_str(), log_ud); return nullptr; };
    try { return create_instance_impl(params, log_cb, log_ud); }          // NULL = "Plugin failed to create instance" at the host (wrapper.rs:184-188)
    catch (const std::exception& e) { return fail(std::string("Failed to create Whisper plugin instance: ") + e.what()); }
    catch (...) { return fail("Failed to create Whisper plugin instance: unknown C++ exception"); }
}

// 16 kHz mono samples into the VAD segmenter (lib.rs:411-493)
bool feed_segmenter(WhisperPlugin* self, const Emit& em, const float* samples, size_t n, std::string* err) {
    bool failed = false;
    self->seg.push(samples, n, *self->vad,
                   [&](const skw::SpeechStart& s) { emit_speech_start(self, em, s); },
                   [&](const skw::SegmentCut& cut) { if (!transcribe_and_emit(self, em, cut, err)) { failed = true; return false; } return true; }, err);
    return !failed && err->empty();
}

CResult plugin_process_packet(CPluginHandle handle, const char* input_pin, const CPacket* packet, COutputCallback out_cb, void* out_ud,
                              CTelemetryCallback tel_cb, void* tel_ud) {
    if (!handle || !input_pin || !packet) return err_null();
    return guarded("Whisper plugin", [&]() -> CResult {
        WhisperPlugin* self = (WhisperPlugin*)handle;
        if (!packet->data) return err_result("Invalid packet: Null packet data pointer");
        if (packet->packet_type != SK_PACKET_RAW_AUDIO) {
            if (packet->packet_type == SK_PACKET_TEXT || packet->packet_type == SK_PACKET_TRANSCRIPTION || packet->packet_type == SK_PACKET_CUSTOM || packet->packet_type == SK_PACKET_BINARY)
                return err_result("Whisper plugin only accepts audio packets");
            return err_result("Invalid packet: Unsupported packet type");
        }
        const CAudioFrame* fr = (const CAudioFrame*)packet->data;
        if (!fr->samples) return err_result("Invalid packet: Null samples pointer in audio frame");
        // validate_audio_format (lib.rs:183-197); with the additive input_sample_rate the expected rate is the configured one
        const uint32_t want = self->config.input_sample_rate;
        if (fr->sample_rate != want) {
            if (want == 16000) return err_result("Whisper requires 16kHz audio, got " + std::to_string(fr->sample_rate) + "Hz. Please add an audio_resample node upstream.");
            return err_result("Whisper plugin is configured for " + std::to_string(want) + "Hz input (input_sample_rate), got " + std::to_string(fr->sample_rate) + "Hz.");
        }
        if (fr->channels != 1) return err_result("Whisper requires mono audio, got " + std::to_string(fr->channels) + " channels. Please add an audio_resample node upstream.");
        Emit em{out_cb, out_ud, tel_cb, tel_ud};
        std::string err;
        if (self->front) {
            if (!self->front->push(fr->samples, fr->sample_count, fr->sample_rate, fr->channels,
                                   [&](const float* d, size_t n, std::string* e) { return feed_segmenter(self, em, d, n, e); }, &err)) return err_result(err);
        } else if (!feed_segmenter(self, em, fr->samples, fr->sample_count, &err)) return err_result(err);
        return ok_result();
    });
}

CResult plugin_update_params(CPluginHandle handle, const char* params) {
    if (!handle) return err_result("Invalid handle (null)");
    return guarded("Whisper plugin", [&]() -> CResult {
        WhisperPlugin* self = (WhisperPlugin*)handle;
        if (!params || !*params) return ok_result();
        WhisperConfig nc;   // serde deserialises a fresh config from the new JSON (defaults for missing keys), lib.rs:498-499
        std::string err;
        if (!parse_config(params, &nc, &err)) return err_result(err);
        if (nc.gpu_device_auto) nc.gpu_device = self->config.gpu_device;        // an "auto" instance stays on the device it was dealt
        if (nc.model_path != self->config.model_path || nc.precision != self->config.precision || nc.cross_kv != self->config.cross_kv || nc.use_gpu != self->config.use_gpu ||
            nc.gpu_device != self->config.gpu_device) {
            auto eng = get_engine(nc, self, &err);
            if (!eng) return err_result("Failed to reload Whisper model: " + err);
            if (!check_rule_ids(nc, eng->n_vocab, &err)) return err_result(err);      // (before the instance lets go of the engine it has)
            self->hold(eng);
        } else if (!check_rule_ids(nc, self->engine->n_vocab, &err)) return err_result(err);
        if (nc.vad_model_path != self->config.vad_model_path || nc.vad_threshold != self->config.vad_threshold || nc.vad_mode != self->config.vad_mode || nc.vad_device != self->config.vad_device ||
            (nc.vad_device == "gpu" && nc.gpu_device != self->config.gpu_device)) {
            auto v = make_vad(nc, self, &err);
            if (!v) { const std::string pre = "Failed to initialize VAD: "; return err_result("Failed to reload VAD: " + (err.compare(0, pre.size(), pre) == 0 ? err.substr(pre.size()) : err)); }
            // frames held back (vad_batch_frames > 1) belong to the gate and the threshold they arrived under: judged now, consumed by the next packet or flush
            self->seg.judge_pending(*self->vad);
            self->vad = std::move(v);
        }
        self->seg.set_batch_frames((size_t)nc.vad_batch_frames);
        if (nc.min_silence_duration_ms != self->config.min_silence_duration_ms) self->seg.set_min_silence_ms(nc.min_silence_duration_ms);
        self->seg.set_threshold(nc.vad_threshold); self->seg.set_max_duration_secs(nc.max_segment_duration_secs);
        // another model, language or prompt: what was carried belongs to the old ones (hold() has already cleared it for a new model); the prompt is tokenised again
        if (nc.model_path != self->config.model_path || nc.language != self->config.language || nc.initial_prompt != self->config.initial_prompt) { self->context[0] = 0; self->prompt_ready = false; }
        nc.input_sample_rate = self->config.input_sample_rate; nc.input_resample_mode = self->config.input_resample_mode;   // the front end's rate is fixed at creation (a stream does not change rate)
        self->config = nc;
        return ok_result();
    });
}

CResult plugin_flush(CPluginHandle handle, COutputCallback out_cb, void* out_ud, CTelemetryCallback tel_cb, void* tel_ud) {
    if (!handle) return err_result("Invalid handle (null)");
    return guarded("Whisper plugin", [&]() -> CResult {
        WhisperPlugin* self = (WhisperPlugin*)handle;
        Emit em{out_cb, out_ud, tel_cb, tel_ud}; std::string err;
        // the resampler front end's remainder belongs to the stream whether or not the tail is then transcribed (resampler.rs:543-730 runs on input close)
        if (self->front && !self->front->finish([&](const float* d, size_t n, std::string* e) { return feed_segmenter(self, em, d, n, e); }, &err)) return err_result(err);
        // frames held back by vad_batch_frames > 1 are part of the stream: evaluated and consumed here (with the default of 1 there are none)
        bool failed = false;
        self->seg.drain(*self->vad, [&](const skw::SpeechStart& s) { emit_speech_start(self, em, s); },
                        [&](const skw::SegmentCut& cut) { if (!transcribe_and_emit(self, em, cut, &err)) { failed = true; return false; } return true; });
        if (failed || !err.empty()) return err_result(err);
        if (!self->config.flush_tail) return ok_result();   // trait default (sdk lib.rs:324-326): buffered tail is dropped
        skw::SegmentCut cut;
        if (self->seg.take_tail(&cut) && !transcribe_and_emit(self, em, cut, &err)) return err_result(err);
        return ok_result();
    });
}

void plugin_destroy_instance(CPluginHandle handle) { try { if (handle) delete (WhisperPlugin*)handle; } catch (...) {} }

const CNativePluginAPI kApi = {STREAMKIT_NATIVE_PLUGIN_API_VERSION, plugin_get_metadata, plugin_create_instance, plugin_process_packet,
                               plugin_update_params, plugin_flush, plugin_destroy_instance};
}  // namespace

extern "C" const CNativePluginAPI* streamkit_native_plugin_api(void) { return &kApi; }
// additive, for tests and bench.py: how often this library loaded a model file / found one cached since it was loaded itself (W5)
extern "C" void skw_whisper_plugin_cache_stats(int* model_loads, int* cache_hits) {
    if (model_loads) *model_loads = g_model_loads.load();
    if (cache_hits) *cache_hits = g_cache_hits.load();
}
// additive, for tests and tools/bench_plugin.py: engine calls made by the schedulers of this process, the jobs (segments) they carried, and how many of the calls carried jobs that
// did not all share one parameter block (skw_full_batch_mixed) — what tells a joined batch from several sequential ones.  Plain counters: no GPU is touched.
extern "C" void skw_whisper_plugin_batch_stats(long* engine_calls, long* jobs, long* mixed_calls) {
    if (engine_calls) *engine_calls = g_engine_calls.load();
    if (jobs) *jobs = g_batch_jobs.load();
    if (mixed_calls) *mixed_calls = g_mixed_calls.load();
}
// additive, for tests: engine calls that carried at least one context (skw_full_batch_context); a process whose instances set neither initial_prompt nor carry_context stays at 0
extern "C" void skw_whisper_plugin_context_stats(long* context_calls) { if (context_calls) *context_calls = g_context_calls.load(); }
// additive, for tests: engine calls that carried at least one job with decoding constraints (skw_full_batch_rules); a process whose instances set none of the four keys stays at 0
extern "C" void skw_whisper_plugin_rules_stats(long* rules_calls) { if (rules_calls) *rules_calls = g_rules_calls.load(); }
// additive, for tests: engine calls in which at least one job had a grammar (skw_full_batch_grammar); a process whose instances set neither grammar key stays at 0
extern "C" long skw_whisper_plugin_grammar_calls(void) { return g_grammar_calls.load(); }
// additive, for tests: engine calls that aligned at least one job (skw_full_batch_aligned); a process whose instances all keep timestamp_granularity "segment" stays at 0
extern "C" void skw_whisper_plugin_align_stats(long* align_calls) { if (align_calls) *align_calls = g_align_calls.load(); }
// additive, for tests: the node's own parsing of repetition_penalty / no_repeat_ngram_size / suppress_tokens / logit_bias out of a parameter object, and the check of the ids against
// a vocabulary of n_vocab entries (what create_instance and update_params apply once the model is known).  0 and the record, or -1 and the message.  No GPU is touched.
extern "C" int skw_whisper_plugin_parse_rules(const char* params_json, int n_vocab, skw_decode_rules* out, char* err, size_t errlen) {
    try {
        WhisperConfig cfg; std::string e;
        if (!parse_config(params_json, &cfg, &e) || !check_rule_ids(cfg, n_vocab, &e)) { snprintf(err, errlen, "%s", e.c_str()); return -1; }
        if (out) *out = cfg.rules;
        return 0;
    } catch (const std::exception& ex) { snprintf(err, errlen, "%s", ex.what()); return -1; }
}
// additive, for tests: cached engines (models resident), how many of them hold a batch workspace right now, and live plugin instances over all of them
extern "C" void skw_whisper_plugin_workspace_stats(int* engines, int* workspaces, int* instances) {
    EngineCache& cache = engine_cache();
    std::lock_guard<std::mutex> l(cache.mu);
    int e = 0, w = 0, n = 0;
    for (auto& kv : cache.map) { std::lock_guard<std::mutex> lw(kv.second->ws_mu); ++e; w += kv.second->ctx != nullptr; n += kv.second->live_instances; }
    if (engines) *engines = e; if (workspaces) *workspaces = w; if (instances) *instances = n;
}
