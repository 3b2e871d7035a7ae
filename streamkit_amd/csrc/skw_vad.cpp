// libskw_vad.so — the C ABI of include/skw_vad.h over the header-only Silero implementation (skw_silero.h).
#include "../../include/skw_vad_batch.h"
#include "skw_silero.h"

struct skw_vad {
    std::shared_ptr<const skw::SileroWeights> w; int arith; skw::SileroVad v; skw::SileroContractVad cv;
    skw_vad(std::shared_ptr<const skw::SileroWeights> ww, int a) : w(ww), arith(a), v(ww), cv(ww) {}
};

extern "C" skw_vad* skw_vad_create_ex(const char* path, int arithmetic, char* err, size_t errlen) {
    try {
        if (arithmetic != SKW_VAD_ARITH_LIBM && arithmetic != SKW_VAD_ARITH_CONTRACT) { if (err && errlen) snprintf(err, errlen, "Failed to load VAD model from '%s': unknown arithmetic %d",
            path ? path : "", arithmetic); return nullptr; }
        auto w = std::make_shared<skw::SileroWeights>(); std::string e;
        if (!path || !skw::SileroVad::load_weights(path, w.get(), &e)) { if (err && errlen) snprintf(err, errlen, "%s", path ? e.c_str() : "Failed to load VAD model from '': no path");
        return nullptr; }
        return new skw_vad(w, arithmetic);
    } catch (const std::exception& ex) { if (err && errlen) snprintf(err, errlen, "Failed to load VAD model from '%s': %s", path ? path : "", ex.what()); return nullptr; }
}
extern "C" skw_vad* skw_vad_create(const char* path, char* err, size_t errlen) { return skw_vad_create_ex(path, SKW_VAD_ARITH_LIBM, err, errlen); }
extern "C" int skw_vad_process_chunk(skw_vad* v, const float* frame512, float* probability) {
    if (!v || !frame512 || !probability) return -1;
    *probability = v->arith == SKW_VAD_ARITH_CONTRACT ? v->cv.process_chunk(frame512) : v->v.process_chunk(frame512); return 0;
}
extern "C" int skw_vad_process_chunks(skw_vad* v, const float* frames, size_t n, float* probs) {
    if (!v || (n && (!frames || !probs))) return -1;
    if (v->arith == SKW_VAD_ARITH_CONTRACT) v->cv.process_chunks(frames, n, probs); else for (size_t i = 0; i < n; ++i) probs[i] = v->v.process_chunk(frames + i * 512);
    return 0;
}
extern "C" void skw_vad_reset(skw_vad* v) { if (v) { v->v.reset(); v->cv.reset(); } }
extern "C" void skw_vad_state(const skw_vad* v, float* out256) {
    if (v->arith == SKW_VAD_ARITH_CONTRACT) { float s[320]; v->cv.get_state(s); memcpy(out256, s + 64, sizeof(float) * 256); return; }
    memcpy(out256, v->v.state_h(), sizeof(float) * 128); memcpy(out256 + 128, v->v.state_c(), sizeof(float) * 128);
}
extern "C" int skw_vad_arithmetic(const skw_vad* v) { return v ? v->arith : -1; }
extern "C" void skw_vad_get_state_ex(const skw_vad* v, float* out320) { if (v->arith == SKW_VAD_ARITH_CONTRACT) v->cv.get_state(out320); else v->v.get_state(out320); }
extern "C" void skw_vad_set_state_ex(skw_vad* v, const float* in320) { if (v->arith == SKW_VAD_ARITH_CONTRACT) v->cv.set_state(in320); else v->v.set_state(in320); }
extern "C" int skw_vad_debug_feed_forward(const skw_vad* v, const float* frame512, float* mag, float* c1, float* c2, float* c3, float* c4, float* gin) {
    if (!v || !frame512) return -1;
    float s[320]; v->cv.get_state(s); if (v->arith != SKW_VAD_ARITH_CONTRACT) v->v.get_state(s);
    skw::SileroTaps t; v->cv.feed_forward(s, frame512, &t);
    if (mag) memcpy(mag, t.mag, sizeof t.mag); if (c1) memcpy(c1, t.c1, sizeof t.c1); if (c2) memcpy(c2, t.c2, sizeof t.c2);
    if (c3) memcpy(c3, t.c3, sizeof t.c3); if (c4) memcpy(c4, t.c4, sizeof t.c4); if (gin) memcpy(gin, t.gin, sizeof t.gin);
    return 0;
}
extern "C" void skw_vad_debug_math(int kind, const float* in, float* out, size_t n) {   // tests: 0 sigmoid, 1 tanh of the contract
    for (size_t i = 0; i < n; ++i) out[i] = kind == 1 ? skw_silero_tanh(in[i]) : skw_silero_sigmoid(in[i]);
}
extern "C" void skw_vad_free(skw_vad* v) { delete v; }
