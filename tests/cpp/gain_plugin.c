/*
 * A third-party native plugin in plain C, for tests/test_cpu_abi.py: a gain node ("gain_c", params {"gain": <number>},
 * RawAudio in -> every sample times the gain -> RawAudio out), the shape of the C example StreamKit publishes for its
 * native-plugin ABI.  Written against include/streamkit_native_abi.h alone: it shares no code with the mini-host or
 * the product plugins, so loading it proves the mini-host drives any plugin that follows the header.
 */
#include <stdlib.h>
#include <string.h>

#include "streamkit_native_abi.h"

typedef struct {
    float gain;
    float* buf;
    size_t cap;
} GainNode;

static float parse_gain(const char* json) {
    const char* k = json ? strstr(json, "\"gain\"") : NULL;
    if (!k) return 1.0f;
    k = strchr(k + 6, ':');
    return k ? strtof(k + 1, NULL) : 1.0f;
}

static CResult ok(void) { CResult r = {true, NULL}; return r; }
static CResult fail(const char* msg) { CResult r = {false, msg}; return r; }

static const CAudioFormat any_f32 = {0, 0, SK_SAMPLE_F32};     /* 0 = the host's wildcard */
static const CPacketTypeInfo in_types[] = {{SK_PACKET_RAW_AUDIO, &any_f32, NULL}};
static const CInputPin inputs[] = {{"in", in_types, 1}};
static const COutputPin outputs[] = {{"out", {SK_PACKET_RAW_AUDIO, &any_f32, NULL}}};
static const char* const categories[] = {"audio", "filters"};
static const CNodeMetadata metadata = {
    "gain_c", "Audio gain (volume) filter in C", inputs, 1, outputs, 1,
    "{\"type\":\"object\",\"properties\":{\"gain\":{\"type\":\"number\",\"default\":1.0,\"minimum\":0.0}}}",
    categories, 2};

static const CNodeMetadata* get_metadata(void) { return &metadata; }

static CPluginHandle create_instance(const char* params_json, CLogCallback log, void* log_ud) {
    GainNode* n = (GainNode*)calloc(1, sizeof(GainNode));
    if (!n) return NULL;
    n->gain = parse_gain(params_json);
    if (log) log(SK_LOG_INFO, "gain_c", "instance created", log_ud);
    return n;
}

static CResult process_packet(CPluginHandle h, const char* pin, const CPacket* pk, COutputCallback out, void* out_ud,
                              CTelemetryCallback tel, void* tel_ud) {
    (void)pin; (void)tel; (void)tel_ud;
    GainNode* n = (GainNode*)h;
    if (!n || !pk) return ok();
    if (pk->packet_type != SK_PACKET_RAW_AUDIO || !pk->data) return fail("gain_c: expected RawAudio");
    const CAudioFrame* in = (const CAudioFrame*)pk->data;
    if (in->sample_count > n->cap) {
        float* b = (float*)realloc(n->buf, in->sample_count * sizeof(float));
        if (!b) return fail("gain_c: out of memory");
        n->buf = b; n->cap = in->sample_count;
    }
    for (size_t i = 0; i < in->sample_count; ++i) n->buf[i] = in->samples[i] * n->gain;
    CAudioFrame f = {in->sample_rate, in->channels, n->buf, in->sample_count};
    CPacket o = {SK_PACKET_RAW_AUDIO, &f, sizeof f};
    return out("out", &o, out_ud);
}

static CResult update_params(CPluginHandle h, const char* params_json) {
    if (h) ((GainNode*)h)->gain = parse_gain(params_json);
    return ok();
}

static CResult flush(CPluginHandle h, COutputCallback out, void* out_ud, CTelemetryCallback tel, void* tel_ud) {
    (void)h; (void)out; (void)out_ud; (void)tel; (void)tel_ud;
    return ok();
}

static void destroy_instance(CPluginHandle h) {
    GainNode* n = (GainNode*)h;
    if (n) { free(n->buf); free(n); }
}

static const CNativePluginAPI api = {STREAMKIT_NATIVE_PLUGIN_API_VERSION, get_metadata, create_instance, process_packet,
                                     update_params, flush, destroy_instance};

const CNativePluginAPI* streamkit_native_plugin_api(void) { return &api; }
