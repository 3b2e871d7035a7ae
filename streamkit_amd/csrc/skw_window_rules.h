// skw_window_rules.h — the decision rules of whisper_full_with_state that need no device: plain integer and double arithmetic on one window's tokens and bookkeeping.
//
// The token loop's update is the one function here that also runs on the device (the tail of both samplers, smp_commit in skw_kernels_sample.hip); everything else is host code the engine's window
// loop calls between GPU phases (skw_engine.hip).  Nothing here knows the model, the context or HIP beyond SKW_HD, so g++ compiles the header alone:
// tests/cpp/window_rules_main.cpp drives every function of it (tests/test_cpu_window_rules.py, plain and under the host sanitizers), against the fixture and the oracle's
// statement of the same rules (oracle/skw_oracle.c: token_loop_update, window_output).
#pragma once
#include <stdint.h>
#include "../../include/skw_math.h"

// per-sequence decoding state kept on the device (whisper_decoder + the bits of whisper_full_with_state's loop that depend on it)
struct SkwSeqState {
    int32_t active;        // still decoding
    int32_t failed, completed;
    int32_t has_ts, seek_delta, result_len;
    int32_t n_tokens;      // sampled tokens so far (i)
    int32_t seek, seek_end;
    int32_t n_prompt;
    float no_speech_prob;
    float min_margin;
    int32_t cur_token;     // token to feed next
    int32_t cur_pos;       // its position
    float temperature;     // 0: argmax; > 0: logits / t, then a std::discrete_distribution draw from the clip's mt19937
    int32_t pad;
    int32_t n_keys;        // cross-attention keys of this row (the clip's audio_ctx); 0: the model's n_audio_ctx
};
// The prompt pass (skw_engine.hip, prefill): one SkwSeqState per PROMPT TOKEN, so every kernel of the decode step takes it as a row —
//   active = 1, cur_token / cur_pos = the token and its position, pad = the sequence (window slot) it belongs to, seek = slot * n_text_ctx + position (its K / V cache row).
// whisper_full_with_state: `const int delta_min = 10` mel frames (100 ms) - shortest input transcribed, the loop's stop rule and the decoder's end-of-audio test
#define SKW_DELTA_MIN 10
#define SKW_PROMPT_CAP 240   // [prev] + n_text_ctx/2 past tokens + sot, language, task, notimestamps
#define SKW_WINDOW_FRAMES 3000   // one 30 s chunk in 10 ms mel frames (100 * WHISPER_CHUNK_SIZE): seek_delta of a window nothing has shortened
struct SkwTokenOut { int32_t id, tid; float p, plog, pt, ptsum, margin; };

// ---- (a) the token loop's update, host and device
// One sampled token's effect on the row's bookkeeping — the body of whisper_full_with_state's token loop between sampling and the next decoder step ("timestamp token - update
// sliding window" down to the "failed" / "completed" tests).  seek_delta / result_len follow the last timestamp above <|0.00|>; a timestamp that steps BACK fails the pass
// (whisper.cpp #2065); the pass completes at <|endoftext|>, past max_tokens, or when the timestamps reach the end of the audio, and at the loop bound n_max; it fails when that
// bound comes before half a window is covered.  id: the sampled token, i: its index in the window.  Sets st.failed / st.completed and returns non-zero when either one ends the row's loop.
SKW_HD int skw_token_loop_update(SkwSeqState& st, int id, int i, int tok_beg, int tok_eot, int max_tokens, int no_timestamps, int single_segment, int n_max) {
    int failed = 0, completed = 0;
    if (id > tok_beg) {
        const int sd_new = 2 * (id - tok_beg);
        if (st.has_ts && st.seek_delta > sd_new && st.result_len < i) failed = 1;
        else { st.seek_delta = sd_new; st.result_len = i + 1; st.has_ts = 1; }
    }
    if (!failed && (id == tok_eot || (max_tokens > 0 && i >= max_tokens) || (st.has_ts && st.seek + st.seek_delta + SKW_DELTA_MIN >= st.seek_end))) {
        if (st.result_len == 0 && !no_timestamps) {
            if (st.seek + st.seek_delta + SKW_DELTA_MIN >= st.seek_end) st.result_len = i + 1; else failed = 1;
        }
        if (!failed) {
            if (single_segment || no_timestamps) { st.result_len = i + 1; st.seek_delta = SKW_WINDOW_FRAMES; }
            completed = 1;
        }
    }
    if (!failed && !completed && i == n_max - 1 && (st.result_len == 0 || st.seek_delta < SKW_WINDOW_FRAMES / 2)) failed = 1;
    if (!failed && !completed && i + 1 >= n_max) completed = 1;   // loop bound reached (whisper.cpp leaves the for loop)
    st.failed = failed; st.completed = completed;
    return failed | completed;
}

// ---- (b) host rules (the kernel files define SKW_WINDOW_RULES_DEVICE_PART before they include this header: they need none of what follows, nor its standard headers)
#ifndef SKW_WINDOW_RULES_DEVICE_PART
#include <math.h>
#include <stdio.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

// The temperature ladder of one request ("temperatures" at the top of whisper_full_with_state): temperature, then + temperature_inc while below 1.0 (+ 1e-6), in float as
// whisper.cpp's loop runs it; temperature_inc <= 0 leaves the one entry.  At most 16 entries.
static inline std::vector<float> skw_temperature_ladder(float temperature, float temperature_inc) {
    std::vector<float> tl; tl.push_back(temperature);
    if (temperature_inc > 0.0f) for (float t = temperature + temperature_inc; t < 1.0f + 1e-6f && tl.size() < 16; t += temperature_inc) tl.push_back(t);
    return tl;
}

// One row's prompt ("init prompt and kv cache for the current iteration"): [prev] + the last min(n_text_ctx / 2, n, room) tokens of prompt_past — on passes at t < 0.5 only, and
// only when there is a past — then the tail (sot, language, task (, notimestamps)).  room = n_text_ctx - n_max - n_tail - 1 keeps every position of the window inside
// n_text_ctx; it only binds with notimestamps in the tail.  out: SKW_PROMPT_CAP ids.  Returns the prompt's length; *take: how many tokens of prompt_past it took.
static inline int skw_row_prompt(const std::vector<int>& prompt_past, float t, const int32_t* tail, int n_tail, int n_text_ctx, int n_max, int tok_prev, int* out, int* take) {
    int n = 0; *take = 0;
    if (!prompt_past.empty() && t < 0.5f) {
        *take = std::min(std::min(n_text_ctx / 2, (int)prompt_past.size()), n_text_ctx - n_max - n_tail - 1);
        out[n++] = tok_prev; for (int i = 0; i < *take; ++i) out[n++] = prompt_past[prompt_past.size() - *take + i];
    }
    for (int k = 0; k < n_tail; ++k) out[n++] = tail[k];
    return n;
}

// whisper_sequence_score: avg_logprobs + entropy of the last 32 tokens
static inline void skw_sequence_score(const SkwTokenOut* tk, int result_len, double* avg_logprobs, double* entropy) {
    *avg_logprobs = -INFINITY; *entropy = 0.0; if (result_len == 0) return;
    double result = 0.0; for (int i = 0; i < result_len; ++i) result += tk[i].plog;
    *avg_logprobs = result / result_len;
    std::map<int, int> cnts; int cnt = 0; for (int i = std::max(0, result_len - 32); i < result_len; ++i) { cnts[tk[i].id]++; cnt++; }
    double e = 0.0; for (auto& kv : cnts) { double pp = kv.second / (double)cnt; e -= pp * log(pp); } *entropy = e;
}

// One pass's verdict ("rank the resulting sequences" down to the fallback test, and is_no_speech of the output step): a pass the token loop did not fail is scored over its
// first result_len tokens and fails when more than 32 of them have an entropy below entropy_thold; a fallback is requested for a failed pass and for one whose avg_logprobs is
// below logprob_thold unless no_speech_prob reaches no_speech_thold; the window is no-speech when no_speech_prob is above its threshold AND avg_logprobs below its own.
// n_tok: the tokens the output step is handed — every sampled one of a pass the token loop failed, the first result_len otherwise.
struct SkwVerdict { bool failed, fallback, no_speech; int n_tok; double avg_logprobs, entropy; };
static inline SkwVerdict skw_pass_verdict(const SkwSeqState& s, const SkwTokenOut* tk, float entropy_thold, float logprob_thold, float no_speech_thold) {
    SkwVerdict v; v.failed = s.failed != 0; v.n_tok = s.n_tokens; v.avg_logprobs = -INFINITY; v.entropy = 0.0;
    if (!v.failed) { v.n_tok = s.result_len; skw_sequence_score(tk, s.result_len, &v.avg_logprobs, &v.entropy); if (s.result_len > 32 && v.entropy < entropy_thold) v.failed = true; }
    v.fallback = v.failed || (v.avg_logprobs < logprob_thold && s.no_speech_prob < no_speech_thold);
    v.no_speech = s.no_speech_prob > no_speech_thold && v.avg_logprobs < logprob_thold;
    return v;
}

// "update prompt_past": what this window's prompt took from it is always kept; the window's first result_len tokens are appended only when it is speech
static inline void skw_prompt_past_update(std::vector<int>& prompt_past, int take, const SkwTokenOut* tk, int result_len, bool is_no_speech) {
    std::vector<int> keep(prompt_past.end() - take, prompt_past.end());
    prompt_past = keep;
    if (!is_no_speech) for (int i = 0; i < result_len; ++i) prompt_past.push_back(tk[i].id);
}

// a clip's output so far: segments, their tokens and their text (SkwSegment is skw_segment of include/skw_engine.h, SkwTokenOut its skw_token)
struct SkwSegment { int64_t t0, t1; int32_t tok_begin, tok_end, text_off, text_len; };
struct SeqAcc { std::vector<SkwSegment> seg; std::vector<SkwTokenOut> tok; std::string text; };

// The window's output step (whisper_full_with_state after the temperature ladder, "if (!tokens_cur.empty() ...)" to "seek += seek_delta"): tk[0 .. n_tok) are cut into segments
// at timestamp tokens above <|0.00|> — a run of timestamps closes one segment, a segment without text is dropped, a trailing piece of text ends at seek + seek_delta — and
// appended to A, unless the window is no-speech.  Returns the advance of seek: seek_delta, or, when the tokens end "text, timestamp" (single_timestamp_ending: nothing spoken
// after the last timestamp), what is left of the chunk.  tok_str: the text of ids below tok_eot.  Frames of 10 ms; seek_end: the frames the clip has.
static inline int skw_window_output(const SkwTokenOut* tk, int n_tok, int seek, int seek_delta, int seek_end, int tok_beg, int tok_eot, int single_segment, bool is_no_speech,
                                    const std::string* tok_str, SeqAcc& A) {
    if (n_tok > 0 && !is_no_speech) {
        int i0 = 0; int64_t t0 = seek + 2 * (tk[0].tid - tok_beg); std::string text;
        auto push = [&](int64_t a, int64_t b, int from, int to) {
            SkwSegment sg{}; sg.t0 = a; sg.t1 = b; sg.tok_begin = (int)A.tok.size();
            for (int q = from; q < to; ++q) A.tok.push_back(tk[q]);
            sg.tok_end = (int)A.tok.size(); sg.text_off = (int)A.text.size(); sg.text_len = (int)text.size(); A.text += text; A.seg.push_back(sg);
        };
        for (int i = 0; i < n_tok; ++i) {
            if (tk[i].id < tok_eot) text += tok_str[tk[i].id];
            if (tk[i].id > tok_beg && !single_segment) {
                const int64_t t1 = seek + 2 * (tk[i].tid - tok_beg);
                if (!text.empty()) push(t0, t1, i0, i + 1);
                text.clear();
                while (i < n_tok && tk[i].id > tok_beg) i++;
                i--; t0 = t1; i0 = i + 1;
            }
        }
        if (!text.empty()) push(t0, seek + seek_delta, i0, n_tok);
    }
    const bool single_timestamp_ending = n_tok > 1 && tk[n_tok - 2].id < tok_beg && tk[n_tok - 1].id > tok_beg;
    if (single_timestamp_ending) seek_delta = std::min(seek_end - seek, SKW_WINDOW_FRAMES);
    return seek_delta;
}

// A context handed in (cx[0] = n, cx[1 .. n] = ids, oldest first: prompt_past as the window loop finds it) is refused unless n is in 0 .. n_cap and every id in [0, n_vocab).
// Returns true when it stands; otherwise err says why, naming the clip.
static inline bool skw_context_check(const int32_t* cx, int n_cap, int n_vocab, int clip, char* err, size_t errlen) {
    const int n = cx[0];
    if (n < 0 || n > n_cap) { snprintf(err, errlen, "clip %d: context of %d tokens outside [0, %d]", clip, n, n_cap); return false; }
    for (int k = 0; k < n; ++k) if (cx[1 + k] < 0 || cx[1 + k] >= n_vocab) {
        snprintf(err, errlen, "clip %d: context token %d (id %d) outside [0, %d)", clip, k, cx[1 + k], n_vocab); return false; }
    return true;
}
// prompt_past as the call leaves it goes back to its owner: the newest n_cap tokens (kept prompt + one window is below that for every n_text_ctx <= 512)
static inline void skw_context_write(const std::vector<int>& prompt_past, int n_cap, int32_t* cx) {
    const int n = std::min((int)prompt_past.size(), n_cap);
    cx[0] = n; for (int k = 0; k < n; ++k) cx[1 + k] = prompt_past[prompt_past.size() - n + k];
}
#endif
