/*
 * skw_align_params.h — what a clip asks of skw_full_batch_aligned / skw_align_batch (include/skw_engine.h), and the limits that go with it.  Plain C, nothing else:
 * the arithmetic these parameters select, its evaluator and the helpers that fill and check a record (skw_align_heads_top, skw_align_check_params) are include/skw_align.h.
 */
#ifndef SKW_ALIGN_PARAMS_H
#define SKW_ALIGN_PARAMS_H
#include <stdint.h>

#define SKW_ALIGN_MEDIAN_MAX 15     /* widest median filter the kernels hold in registers */
#define SKW_ALIGN_MAX_ROWS 256      /* rows of one alignment matrix: a DTW thread owns a row (n_text_ctx / 2 + 2 = 226 in every Whisper) */
#define SKW_ALIGN_MAX_LAYERS 32

/* head_mask: bit h of word l = head h of decoder layer l; median_width: odd, 1 .. SKW_ALIGN_MEDIAN_MAX (7: openai's and transformers') */
typedef struct { int32_t enabled; int32_t median_width; uint32_t head_mask[SKW_ALIGN_MAX_LAYERS]; } skw_align_params;

#endif /* SKW_ALIGN_PARAMS_H */
