// skw_decode_rules (include/skw_engine.h) on the host: the default record, the test for it, and the ONE check of a record that the engine (per clip, before anything runs) and
// the Whisper node (per instance, at create_instance / update_params) both apply.  Host code only; needs no device.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/skw_engine.h"

static inline void skw_decode_rules_set_default(skw_decode_rules* r) { memset(r, 0, sizeof *r); r->repetition_penalty = 1.0f; }
// NULL and (1.0, 0, 0) ask for nothing: such a clip is skw_full_batch_context's, and a call of such clips launches no constraint kernel
static inline bool skw_decode_rules_is_default(const skw_decode_rules* r) { return !r || (r->repetition_penalty == 1.0f && r->no_repeat_ngram_size == 0 && r->n_bias == 0); }
// who: "clip 3" / "row 3" — the message names it.  false: err holds why the record is refused
static inline bool skw_decode_rules_check(const skw_decode_rules* r, int n_vocab, const char* who, char* err, size_t errlen) {
    if (!r) return true;
    if (!std::isfinite(r->repetition_penalty) || !(r->repetition_penalty > 0.0f)) {
        snprintf(err, errlen, "%s: repetition_penalty %g must be finite and > 0 (1 = off)", who, (double)r->repetition_penalty); return false; }
    if (r->no_repeat_ngram_size < 0) { snprintf(err, errlen, "%s: no_repeat_ngram_size %d must be >= 0 (0 = off)", who, r->no_repeat_ngram_size); return false; }
    if (r->n_bias < 0 || r->n_bias > SKW_BIAS_MAX) { snprintf(err, errlen, "%s: n_bias %d outside [0, %d]", who, r->n_bias, SKW_BIAS_MAX); return false; }
    std::vector<bool> seen;
    for (int k = 0; k < r->n_bias; ++k) {
        const int id = r->bias_id[k]; const float b = r->bias[k];
        if (id < 0 || id >= n_vocab) { snprintf(err, errlen, "%s: bias %d: token id %d outside [0, %d)", who, k, id, n_vocab); return false; }
        if (seen.empty()) seen.assign((size_t)n_vocab, false);
        if (seen[id]) { snprintf(err, errlen, "%s: bias %d: token id %d is given twice", who, k, id); return false; }
        seen[id] = true;
        if (std::isnan(b) || (std::isinf(b) && b > 0.0f)) { snprintf(err, errlen, "%s: bias %d (token %d): %g is not finite or -inf", who, k, id, (double)b); return false; }
    }
    return true;
}
