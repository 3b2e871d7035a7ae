/*
 * skw_grammar.h — the CONTRACT of grammar-constrained decoding: a grammar as a dense byte-level DFA, the rule it applies to one sampling decision of one row, the check of a
 * record, and a sequential CPU evaluator of the rule.  The HIP side is streamkit_amd/csrc/skw_kernels_grammar.hip (k_dec_grammar), which evaluates skw_grammar_walk — the one
 * function below that decides whether a token fits — on the device; the compiler that makes such a table from a pattern is streamkit_amd/csrc/skw_grammar_compile.h.
 * Plain C, host/device, no libm.
 *
 * WHAT A GRAMMAR IS.  whisper.cpp's whisper_full_params carries grammar_rules / grammar_penalty: at every step the tokens whose text cannot continue a match lose grammar_penalty
 * logits, and <|endoftext|> loses it while the match is incomplete.  Its grammars are GBNF (pushdown).  This one is the REGULAR subset: a DFA over bytes, anchored at both ends
 * (a full match).  State 0 is the start; next[s][b] is the state after byte b, or SKW_GRAMMAR_DEAD when no match can begin with the bytes read so far; accept[s] = 1 where a
 * complete match ends.  A table made by skw_grammar_compile is trimmed: every state that is not DEAD can still reach an accepting one, so "not DEAD" means "a match is still
 * possible".  A table made by hand need not be; the rule below is stated on the table as it is.
 *
 * THE RULE, for one sampling decision of one row.  x is the row's f32 logits after the three stages of skw_decode_rules (include/skw_engine.h); this is stage 4, ahead of the
 * sampler.  T[0 .. m) is the pass's text tokens exactly as skw_decode_rules defines them: the ids below <|endoftext|> sampled in the current temperature pass of the current
 * window — timestamps, specials and the prompt are not part of it (timestamps are transparent to the match).  bytes(t) is skw_model_token_text(t).
 *   1. s = state 0 walked over bytes(T[0]) ... bytes(T[m-1]).  If the walk reaches DEAD an earlier choice left the language: the row is LEFT UNTOUCHED for the rest of the
 *      pass (whisper.cpp leaves a row alone once no grammar stack survives).
 *   2. every text token t < tok_eot: t FITS iff bytes(t) is non-empty and the walk from s over it does not reach DEAD.  A token that does not fit gets
 *      x[t] = x[t] - penalty — one f32 subtraction.
 *   3. if accept[s] == 0: x[tok_eot] = x[tok_eot] - penalty.
 *   4. every other id (specials, timestamps) is untouched.
 * Not applied in the language-detection pass nor while a row still feeds its prompt; the walk restarts at state 0 in every temperature pass and every window (a grammar is meant
 * for an utterance of one window).  The penalty is finite on purpose, as whisper.cpp's is: no row becomes all -inf because of the grammar, and where the sampler's own masks
 * remove every fitting token the best non-fitting one wins — the documented escape, not an error.
 */
#ifndef SKW_GRAMMAR_H
#define SKW_GRAMMAR_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKW_GR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SKW_GR_HD static inline
#endif

#define SKW_GRAMMAR_MAX_STATES 4096          /* next[] is then 4096 x 256 x 2 B = 2 MiB */
#define SKW_GRAMMAR_DEAD 0xFFFFu
typedef struct { int32_t n_states;          /* 1 .. SKW_GRAMMAR_MAX_STATES; state 0 is the start */
                 const uint16_t* next;      /* [n_states][256]: next state or SKW_GRAMMAR_DEAD */
                 const uint8_t*  accept;    /* [n_states]: 1 = a complete match ends here */
                 float penalty;             /* finite, > 0 */ } skw_grammar;

/* The text of the vocabulary's text tokens as one image: bytes(t) = bytes[off[t] .. off[t + 1]) for t in [0, n_text), n_text >= tok_eot.  The engine builds it from
 * skw_model_token_text once per model and keeps a copy on the device. */
typedef struct { int32_t n_text; const int32_t* off /* [n_text + 1] */; const uint8_t* bytes; } skw_grammar_vocab;

/* state s (not DEAD) walked over n bytes: the state reached, or DEAD as soon as the table says so.  THE function host and device share. */
SKW_GR_HD uint32_t skw_grammar_walk(const uint16_t* next, uint32_t s, const uint8_t* b, int n) {
    for (int i = 0; i < n; ++i) { s = next[(size_t)s * 256 + b[i]]; if (s == SKW_GRAMMAR_DEAD) return SKW_GRAMMAR_DEAD; }
    return s;
}
/* step 2's predicate */
SKW_GR_HD int skw_grammar_fits(const uint16_t* next, uint32_t s, const uint8_t* b, int n) { return n > 0 && skw_grammar_walk(next, s, b, n) != SKW_GRAMMAR_DEAD; }

/* false: err holds why the record is refused; who ("clip 3" / "row 3") is named.  NULL asks for nothing and passes. */
static inline int skw_grammar_check(const skw_grammar* g, const char* who, char* err, size_t errlen) {
    if (!g) return 1;
    if (g->n_states < 1 || g->n_states > SKW_GRAMMAR_MAX_STATES) {
        snprintf(err, errlen, "%s: grammar: n_states %d outside [1, %d]", who, g->n_states, SKW_GRAMMAR_MAX_STATES); return 0; }
    if (!g->next || !g->accept) { snprintf(err, errlen, "%s: grammar: next / accept table is NULL", who); return 0; }
    if (!(g->penalty > 0.0f) || !(g->penalty <= 3.4028234663852886e38f)) {      /* (NaN fails the first test, +inf the second) */
        snprintf(err, errlen, "%s: grammar: penalty %g must be finite and > 0", who, (double)g->penalty); return 0; }
    for (int s = 0; s < g->n_states; ++s) if (g->accept[s] > 1) {
        snprintf(err, errlen, "%s: grammar: accept[%d] = %d is neither 0 nor 1", who, s, (int)g->accept[s]); return 0; }
    for (long i = 0; i < (long)g->n_states * 256; ++i) if (g->next[i] != SKW_GRAMMAR_DEAD && g->next[i] >= (uint32_t)g->n_states) {
        snprintf(err, errlen, "%s: grammar: next[%ld][%ld] = %u is neither a state below %d nor DEAD", who, i / 256, i % 256, (unsigned)g->next[i], g->n_states); return 0; }
    return 1;
}

/* ---- the sequential evaluator ---- */
/* step 1: the state after the pass's text tokens (hist: every id sampled in the pass so far, timestamps and all), or DEAD */
static inline uint32_t skw_grammar_state_ref(const skw_grammar* g, const skw_grammar_vocab* v, int tok_eot, const int32_t* hist, int n_hist) {
    uint32_t s = 0;
    for (int i = 0; i < n_hist && s != SKW_GRAMMAR_DEAD; ++i) {
        const int t = hist[i];
        if (t < 0 || t >= tok_eot) continue;
        s = skw_grammar_walk(g->next, s, v->bytes + v->off[t], v->off[t + 1] - v->off[t]);
    }
    return s;
}
/* steps 1 - 4 on the row x[0 .. n_vocab), in place; returns the state of step 1 */
static inline uint32_t skw_grammar_apply_ref(const skw_grammar* g, const skw_grammar_vocab* v, int tok_eot, const int32_t* hist, int n_hist, float* x) {
    const uint32_t s = skw_grammar_state_ref(g, v, tok_eot, hist, n_hist);
    if (s == SKW_GRAMMAR_DEAD) return s;
    for (int t = 0; t < tok_eot; ++t) if (!skw_grammar_fits(g->next, s, v->bytes + v->off[t], v->off[t + 1] - v->off[t])) x[t] = x[t] - g->penalty;
    if (!g->accept[s]) x[tok_eot] = x[tok_eot] - g->penalty;
    return s;
}

#endif
