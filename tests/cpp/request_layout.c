/* The layout of the request structs as a C compiler sees include/skw_engine.h (tests/test_cpu_request.py compares it with the ctypes structures of streamkit_amd/engine.py).
 * One line per fact: "<struct> sizeof <n>", "<struct> <field> <offset>", "SKW_FULL_REQUEST_MIN <n>". */
#include <stddef.h>
#include <stdio.h>
#include "skw_engine.h"

#define SIZE(S) printf(#S " sizeof %zu\n", sizeof(S))
#define OFF(S, f) printf(#S " " #f " %zu\n", offsetof(S, f))

int main(void) {
    SIZE(skw_full_request);
    OFF(skw_full_request, size); OFF(skw_full_request, params_per_clip); OFF(skw_full_request, params);
    OFF(skw_full_request, pcm); OFF(skw_full_request, n_samples); OFF(skw_full_request, n_clips); OFF(skw_full_request, pcm_on_device);
    OFF(skw_full_request, rng_state); OFF(skw_full_request, context); OFF(skw_full_request, rules);
    OFF(skw_full_request, align); OFF(skw_full_request, times); OFF(skw_full_request, grammar);
    OFF(skw_full_request, text_tokens); OFF(skw_full_request, n_text);
    OFF(skw_full_request, forced_ids); OFF(skw_full_request, n_forced); OFF(skw_full_request, traces); OFF(skw_full_request, results);
    printf("SKW_FULL_REQUEST_MIN %d\n", (int)SKW_FULL_REQUEST_MIN);
    SIZE(skw_sample_rows_request);
    OFF(skw_sample_rows_request, params_per_row); OFF(skw_sample_rows_request, n_rows); OFF(skw_sample_rows_request, params);
    OFF(skw_sample_rows_request, hist); OFF(skw_sample_rows_request, hist_stride); OFF(skw_sample_rows_request, form);
    OFF(skw_sample_rows_request, n_hist); OFF(skw_sample_rows_request, logits);
    OFF(skw_sample_rows_request, filtered_out); OFF(skw_sample_rows_request, tok_out); OFF(skw_sample_rows_request, trace_out);
    OFF(skw_sample_rows_request, rules); OFF(skw_sample_rows_request, grammar); OFF(skw_sample_rows_request, active);
    OFF(skw_sample_rows_request, temperature); OFF(skw_sample_rows_request, rng_state); OFF(skw_sample_rows_request, trace); OFF(skw_sample_rows_request, kernel_id);
    OFF(skw_sample_rows_request, probs_out); OFF(skw_sample_rows_request, no_speech_prob); OFF(skw_sample_rows_request, n_tokens);
    OFF(skw_sample_rows_request, cur_token); OFF(skw_sample_rows_request, active_out);
    return 0;
}
