// Grammar-constrained decoding on the device (include/skw_grammar.h states the rule; skw_full_batch_grammar): stage 4 of the logits row, after k_dec_constrain and ahead of
// the sampler.  Two launches per step, both tiny next to the logits GEMM in front of them:
//   k_dec_grammar_state   one wave per row, lane 0: the row's DFA state after the pass's text tokens.  The state is CARRIED in the row's record (n_seen, state) and advanced by the
//                         tokens that arrived since — one token per step — instead of re-walked from token 0 (224 tokens x their bytes, every load depending on the one before).
//                         The record is written by the host per window and per temperature pass with n_seen = 0, state = 0, and a row whose n_tokens is below n_seen starts
//                         over, so what the kernel computes is the stateless contract's state on every path: prompt pass (rows that still feed their prompt return), ladder
//                         retries on moved slots (restaged records), graph replays past a row's end (finished rows return), the debug hook (n_seen = 0: the whole walk).
//   k_dec_grammar         one thread per (row, id in [0, tok_eot]): a text token walks its bytes from the row's state through skw_grammar_walk — the contract's own function —
//                         and loses `penalty` when the walk dies or the token has no text; the thread of <|endoftext|> subtracts it while the state does not accept.
// Rows without a grammar, finished rows, rows that still feed their prompt and rows whose state is DEAD return at once without touching their logits.
// WHERE THE TABLE LIVES: in global memory, read through the vector L1 / L2 — not staged in LDS.  A launch touches a handful of table rows (the row of the state itself for every
// token's first byte, which kills most tokens, then the few states the survivors pass through): a few KiB that stay in the 32 KiB L1 however many states the table has, while
// staging would have every one of the ~200 workgroups of a row copy up to 64 KiB before its first lookup.  Measured: profiles/grammar/README.md (a 4096-state table costs the
// launch the same as a 10-state one).
#include "skw_kernels.h"
#include "../../include/skw_grammar.h"
#include <hip/hip_runtime.h>

#define GRAMMAR_NT 256

// what a row is doing, as k_dec_constrain asks it: nullptr = leave the row alone
static __device__ __forceinline__ const SkwRowGrammar* grammar_row(const SkwRowGrammar* gr, const SkwSeqState* st_all, int b) {
    const SkwSeqState* st = &st_all[b];
    if (!st->active) return nullptr;
    if (st->cur_pos < st->n_prompt - 1) return nullptr;      // still feeding the prompt: the sampler does not sample either
    return gr[b].next ? &gr[b] : nullptr;
}

__global__ __launch_bounds__(64) void k_dec_grammar_state(SkwRowGrammar* gr, const SkwSeqState* st_all, const SkwTokenOut* toks_all, int max_tok, int tok_eot,
                                                          const int32_t* voc_off, const uint8_t* voc_bytes) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const SkwRowGrammar* r = grammar_row(gr, st_all, b);
    if (!r) return;
    const int n = min(st_all[b].n_tokens, max_tok);
    int seen = r->n_seen; uint32_t s = r->state;
    if (seen > n || seen < 0) { seen = 0; s = 0; }
    const SkwTokenOut* toks = toks_all + (long)b * max_tok;
    for (int i = seen; i < n && s != SKW_GRAMMAR_DEAD; ++i) {
        const int t = toks[i].id;
        if (t < 0 || t >= tok_eot) continue;
        const int o0 = voc_off[t], o1 = voc_off[t + 1];
        s = skw_grammar_walk(r->next, s, voc_bytes + o0, o1 - o0);
    }
    gr[b].n_seen = n; gr[b].state = s;
}

__global__ __launch_bounds__(GRAMMAR_NT) void k_dec_grammar(float* logits_all, int n_vocab, int tok_eot, const SkwRowGrammar* gr, const SkwSeqState* st_all,
                                                            const int32_t* voc_off, const uint8_t* voc_bytes) {
    const int b = blockIdx.y, t = blockIdx.x * GRAMMAR_NT + threadIdx.x;
    const SkwRowGrammar* r = grammar_row(gr, st_all, b);      // (uniform per workgroup)
    if (!r) return;
    const uint32_t s = r->state;
    if (s == SKW_GRAMMAR_DEAD || s >= (uint32_t)r->n_states) return;
    if (t > tok_eot || t >= n_vocab) return;
    float* x = logits_all + (long)b * n_vocab + t;
    if (t == tok_eot) { if (!r->accept[s]) *x = *x - r->penalty; return; }
    const int o0 = voc_off[t], o1 = voc_off[t + 1];
    if (!skw_grammar_fits(r->next, s, voc_bytes + o0, o1 - o0)) *x = *x - r->penalty;
}

void skw_dec_grammar(float* logits, int n_vocab, int tok_eot, SkwRowGrammar* gr, const SkwSeqState* st, const SkwTokenOut* toks, int max_tok, int B,
                     const int32_t* voc_off, const uint8_t* voc_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_dec_grammar_state, dim3(B), dim3(64), 0, s, gr, st, toks, max_tok, tok_eot, voc_off, voc_bytes);
    hipLaunchKernelGGL(k_dec_grammar, dim3((tok_eot + 1 + GRAMMAR_NT - 1) / GRAMMAR_NT, B), dim3(GRAMMAR_NT), 0, s, logits, n_vocab, tok_eot, gr, st, voc_off, voc_bytes);
}
