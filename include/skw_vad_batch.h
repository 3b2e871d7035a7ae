/*
 * skw_vad_batch.h — the additive half of the Silero gate's C ABI (include/skw_vad.h holds the five calls that mirror the reference):
 * the choice of arithmetic, many frames per call and the whole carried state on the CPU (libskw_vad.so, no GPU dependency), and the
 * same gate on the GPU, batched over frames and streams (libskw_engine.so).
 *
 * In a Rust host these take the place of the `ort` session calls of plugins/native/whisper/src/vad.rs: INTEGRATION.md section C.
 */
#ifndef SKW_VAD_BATCH_H
#define SKW_VAD_BATCH_H
#include <stddef.h>
#include <stdint.h>
#include "skw_vad.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- libskw_vad.so: the choice of arithmetic, many frames per call, the whole carried state */
#define SKW_VAD_ARITH_LIBM 0
#define SKW_VAD_ARITH_CONTRACT 1
#define SKW_VAD_STATE_FLOATS 320                      /* context[64], h[128], c[128] */
skw_vad* skw_vad_create_ex(const char* onnx_path, int arithmetic, char* err, size_t errlen);
int  skw_vad_arithmetic(const skw_vad*);
/* n consecutive 512-sample frames of one stream: exactly n calls of skw_vad_process_chunk */
int  skw_vad_process_chunks(skw_vad*, const float* frames, size_t n, float* probabilities);
void skw_vad_get_state_ex(const skw_vad*, float* out320);
void skw_vad_set_state_ex(skw_vad*, const float* in320);
/* tests: the feed-forward half of one frame in the contract arithmetic, from the carried context, without touching the state:
 * STFT magnitudes [129][4], conv outputs [128][4], [64][2], [64][1], [128][1], and b_ih + W_ih.x [512]; any pointer may be NULL */
int  skw_vad_debug_feed_forward(const skw_vad*, const float* frame512, float* mag, float* c1, float* c2, float* c3, float* c4, float* gin);
/* tests: the contract's sigmoid (kind 0) and tanh (kind 1), element by element */
void skw_vad_debug_math(int kind, const float* in, float* out, size_t n);

/* ---- the same gate on the GPU (libskw_engine.so, include/skw_silero_net.h arithmetic), batched over frames and streams.
 * One skw_vad_gpu per device holds the weights, a HIP stream of its own (never a Whisper context's) and grow-only work
 * buffers.  skw_vad_gpu_process may be called from any number of host threads: calls on one object are serialised by a
 * mutex inside it (a call is a few launches; the streams of one call run side by side on different compute units).
 *
 * Stream s brings n_frames[s] consecutive frames (frames[s]: n_frames[s] * 512 floats, may be NULL when n_frames[s] == 0) and
 * its state block state[s] (320 floats, read and overwritten); probs[s] receives n_frames[s] probabilities.  Returns 0, or
 * non-zero with a message in skw_vad_gpu_last_error.  No exception crosses this boundary. */
typedef struct skw_vad_gpu skw_vad_gpu;
skw_vad_gpu* skw_vad_gpu_create(const char* onnx_path, int device, char* err, size_t errlen);
int  skw_vad_gpu_process(skw_vad_gpu*, int n_streams, const float* const* frames, const int32_t* n_frames, float* const* state, float* const* probs);
const char* skw_vad_gpu_last_error(const skw_vad_gpu*);
/* milliseconds of the last call on the device, by events: host-to-device copies, kernels, device-to-host copies */
void skw_vad_gpu_last_timing(const skw_vad_gpu*, float* out3);
void skw_vad_gpu_free(skw_vad_gpu*);
/* tests: the feed-forward taps of n <= 8192 consecutive frames of one stream (layouts as skw_vad_debug_feed_forward, frame-major) */
int  skw_vad_gpu_debug_feed_forward(skw_vad_gpu*, const float* frames, int n, const float* state320, float* mag, float* c1, float* c2, float* c3, float* c4, float* gin);
/* tests: while on, every work buffer is filled with NaNs before each call, so a kernel that reads what none wrote changes a result */
void skw_vad_gpu_debug_alloc_poison(int on);
#ifdef __cplusplus
}
#endif
#endif
