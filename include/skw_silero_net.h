/*
 * skw_silero_net.h — the arithmetic CONTRACT of the Silero VAD gate (16 kHz branch), in the style of skw_math.h.
 *
 * The gate of streamkit_amd/csrc/skw_silero.h (class SileroVad) uses libm's expf / tanhf and whatever the host
 * compiler makes of `s += w * x`; no GPU kernel can be held to that bit for bit.  This header states a second
 * arithmetic for the SAME network that gcc on x86-64 and hipcc on gfx950 evaluate to the same bits under
 * -ffp-contract=off (every fma is explicit; nothing else can contract).  It is the specification: the CPU
 * evaluator (SileroContractVad, skw_silero.h) calls these functions as they stand, the HIP kernels
 * (streamkit_amd/csrc/skw_vad_gpu.hip) tile the same chains over frames and streams, one chain per thread.
 *
 * The network (shapes as in skw_silero.h):
 *   window   x[640]: 64 carried context samples, the 512-sample frame, then 64 reflected samples x[576+j] = x[574-j]
 *   STFT     re/im[bin][fr] = sum_k basis[bin | 129+bin][k] * x[128 fr + k], k = 0..255 ascending, from 0
 *            mag = sqrtf(fmaf(im, im, re * re))                                        -> [129][4]
 *   conv l   four Conv1d(kernel 3, padding 1) + ReLU: 129->128 s1, 128->64 s2, 64->64 s2, 64->128 s1
 *            one chain from the bias over (c ascending, tap k ascending); a tap that falls into the padding is
 *            SKIPPED, not multiplied by zero                                            -> [128][4], [64][2], [64][1], [128][1]
 *   LSTM     s[r] = chain from b_ih[r] over W_ih[r][k] * x[k];  u[r] = chain from b_hh[r] over W_hh[r][k] * h[k];
 *            gates[r] = s[r] + u[r]   (gate blocks i, f, g, o of 128 rows each)
 *            c = fmaf(sigmoid(f), c, sigmoid(i) * tanh(g));  h = sigmoid(o) * tanh(c)
 *   output   p = sigmoid(chain from ob over ow[j] * max(h[j], 0)), j ascending
 *   every chain step is acc = fmaf(w, x, acc); sqrtf and the divisions are IEEE (correctly rounded).
 *
 *   sigmoid(v) = 1 / (1 + skw_expf(-v))
 *   tanh(v)    = sign(v) * (1 - e) / (1 + e),  e = skw_expf(-2 |v|)
 *                absolute error against the real tanh: below 2.5e-7 for every finite v (tests/test_cpu_vad_contract.py
 *                sweeps it against float64).  skw_expf is accurate to about 1.5 ulp and e <= 1, so e is off by at most
 *                ~1e-7 absolutely; d/de of (1-e)/(1+e) is -2/(1+e)^2, between -2 and -1/2, and the subtraction, the
 *                addition and the division each add half an ulp of a value <= 2.  The RELATIVE error is not small
 *                near 0 (1 - e cancels); the LSTM needs the absolute one, its outputs are bounded by 1.
 *
 * The carried state of one stream is 320 floats: context[64], h[128], c[128] (SKW_SILERO_STATE).
 */
#ifndef SKW_SILERO_NET_H
#define SKW_SILERO_NET_H
#include "skw_math.h"

#define SKW_SILERO_FRAME 512
#define SKW_SILERO_CONTEXT 64
#define SKW_SILERO_BINS 129
#define SKW_SILERO_HIDDEN 128
#define SKW_SILERO_GATES 512
#define SKW_SILERO_STATE 320

/* x[640] from the carried context and the frame */
SKW_HD void skw_silero_window(const float* ctx64, const float* frame512, float* x640) {
    for (int i = 0; i < 64; ++i) x640[i] = ctx64[i];
    for (int i = 0; i < 512; ++i) x640[64 + i] = frame512[i];
    for (int j = 0; j < 64; ++j) x640[576 + j] = x640[574 - j];
}

/* basis [258][256]; one STFT magnitude */
SKW_HD float skw_silero_stft_mag(const float* basis, const float* x640, int bin, int fr) {
    const float* br = basis + (size_t)bin * 256; const float* bi = basis + (size_t)(129 + bin) * 256; const float* xs = x640 + 128 * fr;
    float re = 0.0f, im = 0.0f;
    for (int k = 0; k < 256; ++k) { re = __builtin_fmaf(br[k], xs[k], re); im = __builtin_fmaf(bi[k], xs[k], im); }
    return __builtin_sqrtf(__builtin_fmaf(im, im, re * re));
}

/* cw [co][ci][3], in [ci][T]; output element (o, t) of Conv1d(kernel 3, padding 1, stride st) + ReLU */
SKW_HD float skw_silero_conv_relu(const float* cw, const float* cb, const float* in, int ci, int T, int st, int o, int t) {
    float s = cb[o];
    for (int c = 0; c < ci; ++c)
        for (int k = 0; k < 3; ++k) { const int p = t * st - 1 + k; if (p >= 0 && p < T) s = __builtin_fmaf(cw[((size_t)o * ci + c) * 3 + k], in[c * T + p], s); }
    return s > 0.0f ? s : 0.0f;
}

SKW_HD float skw_silero_dot128(float bias, const float* w, const float* x) {
    float s = bias;
    for (int k = 0; k < 128; ++k) s = __builtin_fmaf(w[k], x[k], s);
    return s;
}

SKW_HD float skw_silero_sigmoid(float v) { return 1.0f / (1.0f + skw_expf(-v)); }

SKW_HD float skw_silero_tanh(float v) {
    const uint32_t b = skw_f32_bits(v);
    const float e = skw_expf(-2.0f * skw_bits_f32(b & 0x7fffffffu));
    const float t = (1.0f - e) / (1.0f + e);
    return skw_bits_f32(skw_f32_bits(t) | (b & 0x80000000u));
}

/* one LSTM unit from its four gate pre-activations; updates *c, returns h */
SKW_HD float skw_silero_cell(float gi, float gf, float gg, float go, float* c) {
    const float i = skw_silero_sigmoid(gi), f = skw_silero_sigmoid(gf), g = skw_silero_tanh(gg), o = skw_silero_sigmoid(go);
    const float cn = __builtin_fmaf(f, *c, i * g);
    *c = cn;
    return o * skw_silero_tanh(cn);
}

SKW_HD float skw_silero_output(float ob, const float* ow, const float* h) {
    float acc = ob;
    for (int j = 0; j < 128; ++j) acc = __builtin_fmaf(ow[j], h[j] > 0.0f ? h[j] : 0.0f, acc);
    return skw_silero_sigmoid(acc);
}

#endif /* SKW_SILERO_NET_H */
