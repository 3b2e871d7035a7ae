/*
 * skw_kokoro_ops.h — TEST HOOKS: one Kokoro operator at a time, from host arrays, through either backend of include/skw_kokoro_net.h.
 *
 * The product (streamkit_amd/csrc/skw_tts.hip, skw_tts_debug_op_*) and its checker (oracle/skw_kokoro_oracle.cpp, skwo_kokoro_op_*) both export the SAME seven entries,
 * generated from this one file, so that the two hook sets cannot drift: what differs is the `Side` — how a host array becomes a backend buffer, what a weight needs attached
 * before the backend can read it (the product: the device images of upload_weights; the checker: nothing), and how a result comes back.
 *
 * A Side provides:   Backend& be();  Buf in(const float*, int T, int C);  bool attach(Tensor&, Role);  long out(const Buf&, float* dst, long cap);
 *                    bool begin_lstm(int H);  void end_lstm();      (the product's multi-workgroup LSTM needs exchange words and an LDS size for THIS H)
 * Every entry returns the element count of the result (copying min(count, cap) floats), -1 when the side failed (allocation), -2 for arguments no layer could have.
 */
#ifndef SKW_KOKORO_OPS_H
#define SKW_KOKORO_OPS_H
#include "skw_kokoro_net.h"

namespace skw { namespace kokoro {

/* which image a weight's consumer reads (skw_tts.hip attach_images): as it is; [k / 4][Co16][4] for the conv / linear kernels; ConvTranspose1d's [tap][ci][co] plus one
 * conv image per output phase; a recurrent LSTM weight transposed */
enum Role { ROLE_PLAIN = 0, ROLE_CONV = 1, ROLE_CONVTR = 2, ROLE_HH = 3 };

inline Tensor op_tensor(const float* p, std::initializer_list<int64_t> dims) {
    Tensor t; t.dims = dims; long n = 1; for (int64_t d : dims) n *= d; t.host.assign(p, p + n); return t;
}

template <class S> long op_conv(S& s, const float* x, int T, int Ci, const float* w, int Co, int K, const float* bias, int stride, int dil, int pad, float* out, long cap) {
    if (T < 1 || Ci < 1 || Co < 1 || K < 1 || stride < 1 || dil < 1 || pad < 0 || T + 2 * pad - dil * (K - 1) - 1 < 0) return -2;
    Tensor tw = op_tensor(w, {Co, Ci, K}), tb; if (bias) tb = op_tensor(bias, {Co});
    if (!s.attach(tw, ROLE_CONV) || (bias && !s.attach(tb, ROLE_PLAIN))) return -1;
    return s.out(s.be().conv(s.in(x, T, Ci), tw, bias ? &tb : nullptr, K, stride, dil, pad), out, cap);
}
/* w: [Ci][Co][K], or [C][1][K] when depthwise */
template <class S> long op_convtr(S& s, const float* x, int T, const float* w, int Ci, int Co, int K, const float* bias, int stride, int pad, int out_pad, int depthwise, float* out, long cap) {
    if (T < 1 || Ci < 1 || Co < 1 || K < 1 || stride < 1 || pad < 0 || out_pad < 0 || (T - 1) * stride - 2 * pad + K + out_pad < 1 || (depthwise && Co != Ci)) return -2;
    Tensor tw = depthwise ? op_tensor(w, {Ci, 1, K}) : op_tensor(w, {Ci, Co, K}), tb; if (bias) tb = op_tensor(bias, {Co});
    if (!s.attach(tw, depthwise ? ROLE_PLAIN : ROLE_CONVTR) || (bias && !s.attach(tb, ROLE_PLAIN))) return -1;
    return s.out(s.be().convtr(s.in(x, T, Ci), tw, bias ? &tb : nullptr, K, stride, pad, out_pad, depthwise != 0), out, cap);
}
template <class S> long op_layernorm(S& s, const float* x, int T, int C, const float* gamma, const float* beta, float eps, float* out, long cap) {
    if (T < 1 || C < 1) return -2;
    Tensor tg = op_tensor(gamma, {C}), tb = op_tensor(beta, {C});
    if (!s.attach(tg, ROLE_PLAIN) || !s.attach(tb, ROLE_PLAIN)) return -1;
    auto b = s.in(x, T, C); s.be().layernorm(b, tg, tb, eps);
    return s.out(b, out, cap);
}
/* gb: [2 C] = gamma | beta of the style projection */
template <class S> long op_ada_ln(S& s, const float* x, int T, int C, const float* gb, float* out, long cap) {
    if (T < 1 || C < 1) return -2;
    auto b = s.in(x, T, C); s.be().ada_ln(b, s.in(gb, 1, 2 * C));
    return s.out(b, out, cap);
}
/* act: ACT_LEAKY02 / 01 / 001 or ACT_GELU (Snake needs an alpha tensor and the platform's sinf: the stage tests hold it) */
template <class S> long op_ada_in_act(S& s, const float* x, int T, int C, const float* gb, int act, float* out, long cap) {
    if (T < 1 || C < 1 || act < ACT_LEAKY02 || act > ACT_GELU) return -2;
    auto b = s.in(x, T, C); s.be().ada_in_act(b, s.in(gb, 1, 2 * C), (Act)act, nullptr);
    return s.out(b, out, cap);
}
template <class S> long op_attention(S& s, const float* q, const float* k, const float* v, int T, int heads, float* out, long cap) {
    if (T < 1 || heads < 1 || T > 8192) return -2;
    const int C = 64 * heads;
    return s.out(s.be().attention(s.in(q, T, C), s.in(k, T, C), s.in(v, T, C), heads), out, cap);
}
/* ws[8]: per direction (forward, reverse) weight_ih [4H][In], weight_hh [4H][H], bias_ih [4H], bias_hh [4H] */
template <class S> long op_lstm_bi(S& s, const float* x, int T, int In, int H, const float* const* ws, float* out, long cap) {
    if (T < 1 || In < 1 || H < 1 || H > 256 || T >= 4096) return -2;
    Tensor t[8]; const Tensor* p[8];
    for (int d = 0; d < 2; ++d) {
        t[4 * d] = op_tensor(ws[4 * d], {4 * H, In}); t[4 * d + 1] = op_tensor(ws[4 * d + 1], {4 * H, H});
        t[4 * d + 2] = op_tensor(ws[4 * d + 2], {4 * H}); t[4 * d + 3] = op_tensor(ws[4 * d + 3], {4 * H});
        if (!s.attach(t[4 * d], ROLE_CONV) || !s.attach(t[4 * d + 1], ROLE_HH) || !s.attach(t[4 * d + 2], ROLE_PLAIN) || !s.attach(t[4 * d + 3], ROLE_PLAIN)) return -1;
    }
    for (int i = 0; i < 8; ++i) p[i] = &t[i];
    if (!s.begin_lstm(H)) return -1;
    auto o = s.be().lstm_bi(s.in(x, T, In), p);
    const long n = s.out(o, out, cap);
    s.end_lstm();
    return n;
}

}}  // namespace skw::kokoro

/* the seven exported entries, PREFIX##conv ... PREFIX##lstm_bi.  HANDLE is the first parameter's type (the product: its engine; the checker: an unused pointer);
 * SIDE is constructed from it for the length of one call. */
#define SKW_KOKORO_OP_EXPORTS(PREFIX, HANDLE, SIDE) \
extern "C" long PREFIX##conv(HANDLE h, const float* x, int T, int Ci, const float* w, int Co, int K, const float* bias, int stride, int dil, int pad, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_conv(s, x, T, Ci, w, Co, K, bias, stride, dil, pad, out, cap); } catch (...) { return -1; } } \
extern "C" long PREFIX##convtr(HANDLE h, const float* x, int T, const float* w, int Ci, int Co, int K, const float* bias, int stride, int pad, int out_pad, int depthwise, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_convtr(s, x, T, w, Ci, Co, K, bias, stride, pad, out_pad, depthwise, out, cap); } catch (...) { return -1; } } \
extern "C" long PREFIX##layernorm(HANDLE h, const float* x, int T, int C, const float* gamma, const float* beta, float eps, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_layernorm(s, x, T, C, gamma, beta, eps, out, cap); } catch (...) { return -1; } } \
extern "C" long PREFIX##ada_ln(HANDLE h, const float* x, int T, int C, const float* gb, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_ada_ln(s, x, T, C, gb, out, cap); } catch (...) { return -1; } } \
extern "C" long PREFIX##ada_in_act(HANDLE h, const float* x, int T, int C, const float* gb, int act, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_ada_in_act(s, x, T, C, gb, act, out, cap); } catch (...) { return -1; } } \
extern "C" long PREFIX##attention(HANDLE h, const float* q, const float* k, const float* v, int T, int heads, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_attention(s, q, k, v, T, heads, out, cap); } catch (...) { return -1; } } \
extern "C" long PREFIX##lstm_bi(HANDLE h, const float* x, int T, int In, int H, const float* const* ws, float* out, long cap) { \
    try { SIDE s(h); return skw::kokoro::op_lstm_bi(s, x, T, In, H, ws, out, cap); } catch (...) { return -1; } }

#endif
