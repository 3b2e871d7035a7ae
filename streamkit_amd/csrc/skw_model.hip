// skw_model.hip — GGML model loading for libskw_engine.so: the file parser, the repack of f16 and block-quantised weights into what the kernels read, the tokenizer
// accessors and the language / non-speech tables.  Depends on skw_model only.
//
// Reference call site this replaces: /root/reference/plugins/native/whisper/src/lib.rs:354-363 model load.
#include "skw_engine_priv.h"

static const char* const g_lang[] = {"en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it", "id", "hi", "fi", "vi",
    "he", "uk", "el", "ms", "cs", "ro", "da", "hu", "ta", "no", "th", "ur", "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk", "te", "fa", "lv", "bn", "sr", "az",
    "sl", "kn", "et", "mk", "br", "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw", "gl", "mr", "pa", "si", "km", "sn", "yo", "so", "af", "oc", "ka", "be",
    "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo", "ht", "ps", "tk", "nn", "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha", "ba", "jw", "su", "yue"};
static const int g_n_lang = (int)(sizeof(g_lang) / sizeof(g_lang[0]));
// whisper.cpp's g_lang also maps the full language names; whisper_lang_id accepts either spelling
static const char* const g_lang_name[] = {"english", "chinese", "german", "spanish", "russian", "korean", "french", "japanese", "portuguese", "turkish", "polish", "catalan", "dutch",
    "arabic", "swedish", "italian", "indonesian", "hindi", "finnish", "vietnamese", "hebrew", "ukrainian", "greek", "malay", "czech", "romanian", "danish", "hungarian", "tamil", "norwegian",
    "thai", "urdu", "croatian", "bulgarian", "lithuanian", "latin", "maori", "malayalam", "welsh", "slovak", "telugu", "persian", "latvian", "bengali", "serbian", "azerbaijani", "slovenian",
    "kannada", "estonian", "macedonian", "breton", "basque", "icelandic", "armenian", "nepali", "mongolian", "bosnian", "kazakh", "albanian", "swahili", "galician", "marathi", "punjabi",
    "sinhala", "khmer", "shona", "yoruba", "somali", "afrikaans", "occitan", "georgian", "belarusian", "tajik", "sindhi", "gujarati", "amharic", "yiddish", "lao", "uzbek", "faroese",
    "haitian creole", "pashto", "turkmen", "nynorsk", "maltese", "sanskrit", "luxembourgish", "myanmar", "tibetan", "tagalog", "malagasy", "assamese", "tatar", "hawaiian", "lingala", "hausa",
    "bashkir", "javanese", "sundanese", "cantonese"};
static_assert(sizeof(g_lang_name) / sizeof(g_lang_name[0]) == sizeof(g_lang) / sizeof(g_lang[0]), "one name per code");

static const char* const NST_LIST[] = {"\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
    "\xe3\x80\x8c", "\xe3\x80\x8d", "\xe3\x80\x8e", "\xe3\x80\x8f", "<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))",
    "[[", "]]", "{{", "}}", "\xe2\x99\xaa\xe2\x99\xaa", "\xe2\x99\xaa\xe2\x99\xaa\xe2\x99\xaa", "\xe2\x99\xa9", "\xe2\x99\xaa", "\xe2\x99\xab", "\xe2\x99\xac",
        "\xe2\x99\xad", "\xe2\x99\xae", "\xe2\x99\xaf"};
static const int N_NST_LIST = (int)(sizeof(NST_LIST) / sizeof(NST_LIST[0]));

// qblk: the file's blocks of a quantised tensor (data: its f16 twin)
struct RawT { std::string name; int n_dims = 0; int ne[4] = {1, 1, 1, 1}; int type = 0; std::vector<uint8_t> data; size_t n = 0; std::vector<uint8_t> qblk; int qtype = 0; };
template <typename T> static T* dev_upload(skw_model* m, const T* h, size_t n) {
    T* d = nullptr; if (hipMalloc((void**)&d, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) return nullptr;
    if (n && hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return nullptr; }
    m->allocs.push_back(d); return d;
}
static RawT* find_t(std::vector<RawT>& ts, const std::string& name) { for (auto& t : ts) if (t.name == name) return &t; return nullptr; }
static const float* as_f32(RawT* t, std::vector<float>& tmp) {
    if (t->type == 0) return (const float*)t->data.data();
    tmp.resize(t->n); const uint16_t* h = (const uint16_t*)t->data.data(); for (size_t i = 0; i < t->n; ++i) tmp[i] = skw_f16_to_f32(h[i]); return tmp.data();
}
static bool is_matmul_weight(const RawT& t) {
    const std::string& n = t.name;
    return t.n_dims == 2 && n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0 && n.find("positional_embedding") == std::string::npos && n.find("ln") == std::string::npos;
}
// blocks: n_out rows of K / 32 blocks of ggml type qtype, as the file holds them
void skw_priv::host_q(int qtype, const uint8_t* blocks, int n_out, int K, HostQ* h) {
    const int nb = K / 32; const size_t bb = skw_ggml_block_bytes(qtype);
    h->n_out = n_out; h->K = K; h->q.resize((size_t)n_out * K); h->d.resize((size_t)n_out * nb); h->m.resize((size_t)n_out * nb);
    for (size_t i = 0; i < (size_t)n_out * nb; ++i) skw_ggml_unpack_block(qtype, blocks + i * bb, h->q.data() + i * 32, &h->d[i], &h->m[i]);
}
static void host_q(const RawT& w, HostQ* h) { host_q(w.qtype, w.qblk.data(), w.ne[1], w.ne[0], h); }
// int8 rows as they are; scales and offsets transposed to [block][n_pad] so that a lane's four adjacent features are one 16-byte load
bool skw_priv::up_q(skw_model* m, const HostQ& h, int qtype, DevLin* L) {
    const int nb = h.K / 32, n_pad = (h.n_out + 63) & ~63;
    std::vector<float> dT((size_t)nb * n_pad, 0.0f), mT((size_t)nb * n_pad, 0.0f);
    for (int n = 0; n < h.n_out; ++n) for (int b = 0; b < nb; ++b) { dT[(size_t)b * n_pad + n] = h.d[(size_t)n * nb + b]; mT[(size_t)b * n_pad + n] = h.m[(size_t)n * nb + b]; }
    L->qw = dev_upload(m, h.q.data(), h.q.size()); L->dwT = dev_upload(m, dT.data(), dT.size()); L->mwT = dev_upload(m, mT.data(), mT.size());
    L->n_pad = n_pad; L->qform = skw_ggml_dot_form(qtype);
    return L->qw && L->dwT && L->mwT;
}
// f16 weight [n_out][n_in] (or conv [oc][ic][kw]) -> device [n_out][k_pad] with the contraction axis in kperm order
static bool up_lin(skw_model* m, std::vector<RawT>& ts, const std::string& wname, const char* bname, DevLin* L, char* err, size_t errlen, bool want_nat = false) {
    RawT* w = find_t(ts, wname);
    if (!w) { set_err(err, errlen, "missing tensor %s", wname.c_str()); return false; }
    if (w->type != 1) { set_err(err, errlen, "tensor %s: only f16 matmul weights are supported (ggml type %d)", wname.c_str(), w->type); return false; }
    int n_in, n_out, kw = 1, ic = 0;
    if (w->n_dims == 2) { n_in = w->ne[0]; n_out = w->ne[1]; }
    else if (w->n_dims == 3) { kw = w->ne[0]; ic = w->ne[1]; n_in = kw * ic; n_out = w->ne[2]; }
    else { set_err(err, errlen, "tensor %s: bad dims", wname.c_str()); return false; }
    const int k_pad = (n_in + 31) & ~31;
    std::vector<uint16_t> h((size_t)n_out * k_pad, 0);
    const uint16_t* src = (const uint16_t*)w->data.data();
    for (int o = 0; o < n_out; ++o) {
        uint16_t* dst = h.data() + (size_t)o * k_pad;
        if (w->n_dims == 2) for (int i = 0; i < n_in; ++i) dst[skw_kperm(i)] = src[(size_t)o * n_in + i];
        else for (int c = 0; c < ic; ++c) for (int t = 0; t < kw; ++t) dst[skw_kperm(t * ic + c)] = src[((size_t)o * ic + c) * kw + t];
    }
    L->n_in = n_in; L->n_out = n_out; L->k_pad = k_pad;
    L->w = (half_t*)dev_upload(m, h.data(), h.size());
    if (!L->w) { set_err(err, errlen, "device allocation failed for %s", wname.c_str()); return false; }
    if (want_nat && w->n_dims == 2 && k_pad == n_in) { L->w_nat = (half_t*)dev_upload(m, src, (size_t)n_out * n_in);
    if (!L->w_nat) { set_err(err, errlen, "device allocation failed for %s", wname.c_str()); return false; } }
    if (m->quant && !w->qblk.empty()) { HostQ h; host_q(*w, &h); if (!up_q(m, h, w->qtype, L)) { set_err(err, errlen, "device allocation failed for %s", wname.c_str()); return false; } }
    L->b = nullptr;
    if (bname) {
        RawT* b = find_t(ts, bname);
        if (!b) { set_err(err, errlen, "missing tensor %s", bname); return false; }
        std::vector<float> tmp; L->b = dev_upload(m, as_f32(b, tmp), b->n);
    }
    return true;
}
static bool up_ln(skw_model* m, std::vector<RawT>& ts, const std::string& wname, const std::string& bname, DevLN* L, char* err, size_t errlen) {
    RawT* w = find_t(ts, wname); RawT* b = find_t(ts, bname);
    if (!w || !b) { set_err(err, errlen, "missing tensor %s / %s", wname.c_str(), bname.c_str()); return false; }
    std::vector<float> t1, t2; L->w = dev_upload(m, as_f32(w, t1), w->n); L->b = dev_upload(m, as_f32(b, t2), b->n); return L->w && L->b;
}

extern "C" int skw_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
extern "C" void* skw_host_alloc(size_t bytes) { void* p = nullptr;
if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
extern "C" void skw_host_free(void* p) { if (p) (void)hipHostFree(p); }
extern "C" int skw_model_lang_id(const char* lang) {
    if (!lang) return -1;
    for (int i = 0; i < g_n_lang; ++i) if (!strcmp(g_lang[i], lang)) return i;
    for (int i = 0; i < g_n_lang; ++i) if (!strcmp(g_lang_name[i], lang)) return i;
    return -1;
}

static skw_model* model_load_impl(const char* path, int device, int quant_mode, char* err, size_t errlen);
extern "C" skw_model* skw_model_load_ex(const char* path, int device, int quant_mode, char* err, size_t errlen) {
    try { return model_load_impl(path, device, quant_mode, err, errlen); }
    catch (const std::exception& e) { set_err(err, errlen, "Failed to load Whisper model from '%s': %s", path ? path : "", e.what()); return nullptr; }   // nothing may unwind across the C ABI
}
extern "C" skw_model* skw_model_load(const char* path, int device, char* err, size_t errlen) { return skw_model_load_ex(path, device, SKW_QUANT_GGML, err, errlen); }
extern "C" int skw_model_quant_type(const skw_model* m) { return m->quant; }
static skw_model* model_load_impl(const char* path, int device, int quant_mode, char* err, size_t errlen) {
    int ndev = skw_device_count();
    if (ndev <= 0) { set_err(err, errlen, "no HIP device available: libskw_engine requires an MI355X (gfx950); there is no CPU fallback"); return nullptr; }
    if (device < 0 || device >= ndev) { set_err(err, errlen, "gpu_device %d out of range (%d devices)", device, ndev); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_err(err, errlen, "hipSetDevice(%d) failed", device); return nullptr; }
    FILE* f = fopen(path, "rb");
    if (!f) { set_err(err, errlen, "Failed to load Whisper model from '%s': cannot open file", path); return nullptr; }
    int32_t magic = 0;
    if (fread(&magic, 4, 1, f) != 1 || magic != 0x67676d6c) { fclose(f); set_err(err, errlen, "Failed to load Whisper model from '%s': bad magic", path); return nullptr; }
    skw_model* m = new skw_model(); m->device = device;
    auto fail = [&](const char* msg) -> skw_model* { set_err(err, errlen, "Failed to load Whisper model from '%s': %s", path, msg); fclose(f); skw_model_free(m); return nullptr; };
    if (fread(&m->hp, 4, 11, f) != 11) return fail("short hparams");
    {   // a corrupt header must fail here, not as std::bad_alloc across the C ABI
        const skw_hparams& h = m->hp;
        auto in = [](int v, int lo, int hi) { return v >= lo && v <= hi; };
        if (!in(h.n_vocab, 1000, 200000) || !in(h.n_audio_ctx, 1, 4096) || !in(h.n_audio_state, 64, 1536) || !in(h.n_audio_head, 1, 32) || !in(h.n_audio_layer, 1, 64) ||
            !in(h.n_text_ctx, 8, 4096) || !in(h.n_text_state, 64, 1536) || !in(h.n_text_head, 1, 32) || !in(h.n_text_layer, 1, 64) || !in(h.n_mels, 1, 256)) return fail("implausible hparams");
    }
    int32_t nm = 0, nf = 0;
    if (fread(&nm, 4, 1, f) != 1 || fread(&nf, 4, 1, f) != 1) return fail("short mel filter header");
    if (nm < 1 || nm > 256 || nf < 1 || nf > 4096) return fail("implausible mel filter header");
    std::vector<float> filt((size_t)nm * nf);
    if (fread(filt.data(), 4, filt.size(), f) != filt.size()) return fail("short mel filters");
    m->n_fft_bins = nf;
    if (nm != m->hp.n_mels) return fail("mel filter count differs from n_mels");
    int32_t nv = 0; if (fread(&nv, 4, 1, f) != 1) return fail("short vocab");
    if (nv < 0 || nv > 200000) return fail("implausible vocabulary size");
    const int NV = m->hp.n_vocab; m->tok_str.assign(NV, std::string());
    for (int i = 0; i < nv; ++i) {
        uint32_t len = 0; if (fread(&len, 4, 1, f) != 1) return fail("short vocab");
        if (len > 4096) return fail("implausible token length");
        std::string s(len, '\0'); if (len && fread(&s[0], 1, len, f) != len) return fail("short vocab");
        if (i < NV) m->tok_str[i] = s;
    }
    m->tok_eot = 50256; m->tok_sot = 50257; m->tok_translate = 50357; m->tok_transcribe = 50358; m->tok_solm = 50359;
    m->tok_prev = 50360; m->tok_nosp = 50361; m->tok_not = 50362; m->tok_beg = 50363;
    if (NV >= 51865) {
        m->tok_eot++; m->tok_sot++; const int dt = NV - 51865;
        m->tok_translate += 1 + dt; m->tok_transcribe += 1 + dt; m->tok_solm += 1 + dt; m->tok_prev += 1 + dt; m->tok_nosp += 1 + dt; m->tok_not += 1 + dt; m->tok_beg += 1 + dt;
        m->n_lang = 99 + dt;
    }
    for (int i = nv; i < NV; ++i) {
        char buf[64];
        if (i > m->tok_beg) snprintf(buf, sizeof buf, "[_TT_%d]", i - m->tok_beg);
        else if (i == m->tok_eot) snprintf(buf, sizeof buf, "[_EOT_]");
        else if (i == m->tok_sot) snprintf(buf, sizeof buf, "[_SOT_]");
        else if (i == m->tok_translate) snprintf(buf, sizeof buf, "[_TRANSLATE_]");
        else if (i == m->tok_transcribe) snprintf(buf, sizeof buf, "[_TRANSCRIBE_]");
        else if (i == m->tok_solm) snprintf(buf, sizeof buf, "[_SOLM_]");
        else if (i == m->tok_prev) snprintf(buf, sizeof buf, "[_PREV_]");
        else if (i == m->tok_nosp) snprintf(buf, sizeof buf, "[_NOSP_]");
        else if (i == m->tok_not) snprintf(buf, sizeof buf, "[_NOT_]");
        else if (i == m->tok_beg) snprintf(buf, sizeof buf, "[_BEG_]");
        else if (i > m->tok_sot && i <= m->tok_sot + m->n_lang) snprintf(buf, sizeof buf, "[_LANG_%s]", g_lang[std::min(i - m->tok_sot - 1, g_n_lang - 1)]);
        else snprintf(buf, sizeof buf, "[_extra_token_%d]", i);
        m->tok_str[i] = buf;
    }
    m->tokz.build(m->tok_str, m->tok_eot);
    { // token_to_id lookups performed by whisper_process_logits (a later duplicate string wins, as std::map::operator[] does)
        std::map<std::string, int> t2i; for (int i = 0; i < NV; ++i) t2i[m->tok_str[i]] = i;
        auto get = [&](const std::string& s) { auto it = t2i.find(s); return it == t2i.end() ? -1 : it->second; };
        m->tok_space = get(" "); m->tok_sp_dash = get(" -"); m->tok_sp_quote = get(" '");
        for (int j = 0; j < N_NST_LIST; ++j) for (int sp = 0; sp < 2; ++sp) { int id = get(std::string(sp ? " " : "") + NST_LIST[j]); if (id >= 0) m->nst_ids.push_back(id); }
    }
    std::vector<RawT> ts;
    for (;;) {
        int32_t nd, len, tt; if (fread(&nd, 4, 1, f) != 1) break;
        if (fread(&len, 4, 1, f) != 1 || fread(&tt, 4, 1, f) != 1) return fail("short tensor header");
        RawT t; t.n_dims = nd; t.type = tt; t.n = 1;
        if (nd < 1 || nd > 4 || len < 0 || len > 255) return fail("corrupt tensor header");
        for (int i = 0; i < nd; ++i) { int32_t e; if (fread(&e, 4, 1, f) != 1) return fail("short tensor header");
        if (e < 1 || e > (1 << 24)) return fail("corrupt tensor header"); t.ne[i] = e; t.n *= (size_t)e; }
        if (t.n > ((size_t)1 << 31)) return fail("corrupt tensor header");
        t.name.resize(len); if (len && fread(&t.name[0], 1, len, f) != (size_t)len) return fail("short tensor name");
        size_t esz = tt == 0 ? 4 : tt == 1 ? 2 : 0;
        if (!esz) {   // block-quantised 2-D weights: decoded to f16 here (include/skw_ggml_quant.h, DEVIATION D4)
            const size_t bb = skw_ggml_block_bytes(tt);
            if (!bb || t.ne[0] % 32) { std::string msg = "tensor " + t.name + ": unsupported ggml type " + std::to_string(tt) + " (f32, f16, q4_0, q4_1, q5_0, q5_1, q8_0 are read)";
            return fail(msg.c_str()); }
            std::vector<uint8_t> blocks(t.n / 32 * bb); if (fread(blocks.data(), 1, blocks.size(), f) != blocks.size()) return fail("short tensor data");
            t.data.resize(t.n * 2); skw_ggml_dequant_to_f16(tt, blocks.data(), t.n, (uint16_t*)t.data.data()); t.type = 1; t.qtype = tt; t.qblk = std::move(blocks);
            ts.push_back(std::move(t)); continue;
        }
        t.data.resize(t.n * esz); if (fread(t.data.data(), 1, t.data.size(), f) != t.data.size()) return fail("short tensor data");
        ts.push_back(std::move(t));
    }
    fclose(f); f = nullptr;
    {   // ggml's q8 arithmetic needs every matmul weight in one block type (what whisper.cpp's quantize writes); anything else runs as the f16 twin
        int qt = 0; bool uniform = quant_mode != 0 && !skw_sw(SW_QUANT_TWIN);
        for (auto& t : ts) if (is_matmul_weight(t)) { if (t.qblk.empty()) uniform = false; else if (!qt) qt = t.qtype; else if (qt != t.qtype) uniform = false; }
        m->quant = (uniform && qt) ? qt : 0;
    }
    auto fail2 = [&]() -> skw_model* { skw_model_free(m); return nullptr; };
    // tables
    m->filters = dev_upload(m, filt.data(), filt.size());
    {   // per mel filter: the range of 4-bin groups with a non-zero tap (the filterbank comes from the model file; Slaney filters are narrow)
        std::vector<int> lo(nm, 0), hi(nm, 0);
        for (int j = 0; j < nm; ++j) { int a = nf, b = -1; for (int k = 0; k < nf; ++k) if (filt[(size_t)j * nf + k] != 0.0f) { a = std::min(a, k);
        b = std::max(b, k); } if (b >= 0) { lo[j] = a / 4; hi[j] = b / 4 + 1; } }
        m->mel_grp_lo = dev_upload(m, lo.data(), lo.size()); m->mel_grp_hi = dev_upload(m, hi.data(), hi.size());
    }
    {
        std::vector<float> sn(WHISPER_N_FFT), cs(WHISPER_N_FFT), hn(WHISPER_N_FFT);
        for (int i = 0; i < WHISPER_N_FFT; ++i) { double theta = (2 * M_PI * i) / WHISPER_N_FFT;
        sn[i] = sinf(theta); cs[i] = cosf(theta); hn[i] = 0.5 * (1.0 - cosf((2.0 * M_PI * i) / (WHISPER_N_FFT))); }
        m->sin_t = dev_upload(m, sn.data(), sn.size()); m->cos_t = dev_upload(m, cs.data(), cs.size()); m->hann = dev_upload(m, hn.data(), hn.size());
        std::vector<uint16_t> gt(65536); for (int i = 0; i < 65536; ++i) gt[i] = skw_gelu_table_entry((uint16_t)i);
        m->gelu_tab = dev_upload(m, gt.data(), gt.size());
    }
    std::vector<float> tmp;
    RawT* t;
    if (!(t = find_t(ts, "encoder.positional_embedding"))) { set_err(err, errlen, "missing encoder.positional_embedding"); return fail2(); }
    m->e_pe = dev_upload(m, as_f32(t, tmp), t->n);
    if (!(t = find_t(ts, "decoder.positional_embedding"))) { set_err(err, errlen, "missing decoder.positional_embedding"); return fail2(); }
    m->d_pe = dev_upload(m, as_f32(t, tmp), t->n);
    bool ok = true;
    // fragment-order images of the decoder projections (SkwGemmArgs::Wf); =0: the f16 decode kernels read weight rows
    const bool wfrag_on = skw_sw(SW_DEC_WFRAG) != 0;
    ok = ok && up_lin(m, ts, "encoder.conv1.weight", "encoder.conv1.bias", &m->conv1, err, errlen);
    // conv1 runs as a product over the im2col image [frames][3 n_mels padded]: the f16 GEMMs step K by 64 (80 bands: 240 -> 256, large-v3's 128: 384)
    if (ok && ((m->conv1.k_pad & 63) || m->conv1.n_in != 3 * m->hp.n_mels || m->hp.n_mels > 128)) {
        set_err(err, errlen, "encoder.conv1.weight: 3 x n_mels = %d taps do not pad to a multiple of 64 (n_mels 80 and 128 are supported)", m->conv1.n_in); ok = false;
    }
    ok = ok && up_lin(m, ts, "encoder.conv2.weight", "encoder.conv2.bias", &m->conv2, err, errlen);
    ok = ok && up_ln(m, ts, "encoder.ln_post.weight", "encoder.ln_post.bias", &m->ln_post, err, errlen);
    m->enc.resize(m->hp.n_audio_layer);
    for (int l = 0; l < m->hp.n_audio_layer && ok; ++l) {
        EncLayer& L = m->enc[l]; std::string p = "encoder.blocks." + std::to_string(l) + ".";
        ok = ok && up_ln(m, ts, p + "attn_ln.weight", p + "attn_ln.bias", &L.attn_ln, err, errlen);
        ok = ok && up_lin(m, ts, p + "attn.query.weight", (p + "attn.query.bias").c_str(), &L.q, err, errlen);
        ok = ok && up_lin(m, ts, p + "attn.key.weight", nullptr, &L.k, err, errlen);
        ok = ok && up_lin(m, ts, p + "attn.value.weight", (p + "attn.value.bias").c_str(), &L.v, err, errlen);
        ok = ok && up_lin(m, ts, p + "attn.out.weight", (p + "attn.out.bias").c_str(), &L.o, err, errlen);
        ok = ok && up_ln(m, ts, p + "mlp_ln.weight", p + "mlp_ln.bias", &L.mlp_ln, err, errlen);
        ok = ok && up_lin(m, ts, p + "mlp.0.weight", (p + "mlp.0.bias").c_str(), &L.fc1, err, errlen);
        ok = ok && up_lin(m, ts, p + "mlp.2.weight", (p + "mlp.2.bias").c_str(), &L.fc2, err, errlen);
    }
    ok = ok && up_lin(m, ts, "decoder.token_embedding.weight", nullptr, &m->te, err, errlen);
    if (ok && m->quant) {   // get_rows on the quantised token embedding: q * d (+ m) in f32, not rounded to f16
        RawT* te = find_t(ts, "decoder.token_embedding.weight"); const size_t bb = skw_ggml_block_bytes(te->qtype); std::vector<float> e32(te->n);
        for (size_t i = 0; i < te->n / 32; ++i) skw_ggml_dequant_block(te->qtype, te->qblk.data() + i * bb, e32.data() + i * 32);
        m->te32 = dev_upload(m, e32.data(), e32.size()); ok = m->te32 != nullptr;
    }
    ok = ok && up_ln(m, ts, "decoder.ln.weight", "decoder.ln.bias", &m->d_ln, err, errlen);
    m->dec.resize(m->hp.n_text_layer);
    for (int l = 0; l < m->hp.n_text_layer && ok; ++l) {
        DecLayer& L = m->dec[l]; std::string p = "decoder.blocks." + std::to_string(l) + ".";
        ok = ok && up_ln(m, ts, p + "attn_ln.weight", p + "attn_ln.bias", &L.attn_ln, err, errlen);
        ok = ok && up_lin(m, ts, p + "attn.query.weight", (p + "attn.query.bias").c_str(), &L.q, err, errlen, true);
        ok = ok && up_lin(m, ts, p + "attn.key.weight", nullptr, &L.k, err, errlen, true);
        ok = ok && up_lin(m, ts, p + "attn.value.weight", (p + "attn.value.bias").c_str(), &L.v, err, errlen, true);
        ok = ok && up_lin(m, ts, p + "attn.out.weight", (p + "attn.out.bias").c_str(), &L.o, err, errlen);
        ok = ok && up_ln(m, ts, p + "cross_attn_ln.weight", p + "cross_attn_ln.bias", &L.cross_ln, err, errlen);
        ok = ok && up_lin(m, ts, p + "cross_attn.query.weight", (p + "cross_attn.query.bias").c_str(), &L.cq, err, errlen, true);
        ok = ok && up_lin(m, ts, p + "cross_attn.key.weight", nullptr, &L.ck, err, errlen);
        ok = ok && up_lin(m, ts, p + "cross_attn.value.weight", (p + "cross_attn.value.bias").c_str(), &L.cv, err, errlen);
        ok = ok && up_lin(m, ts, p + "cross_attn.out.weight", (p + "cross_attn.out.bias").c_str(), &L.co, err, errlen);
        ok = ok && up_ln(m, ts, p + "mlp_ln.weight", p + "mlp_ln.bias", &L.mlp_ln, err, errlen);
        ok = ok && up_lin(m, ts, p + "mlp.0.weight", (p + "mlp.0.bias").c_str(), &L.fc1, err, errlen, true);
        ok = ok && up_lin(m, ts, p + "mlp.2.weight", (p + "mlp.2.bias").c_str(), &L.fc2, err, errlen);
        if (ok) {   // fused q|k|v weight [3d][k_pad] and bias [3d] (k has no bias: zeros; adding 0.0f is exact)
            const int d = L.q.n_out, kp = L.q.k_pad; L.qkv.n_in = L.q.n_in; L.qkv.n_out = 3 * d; L.qkv.k_pad = kp;
            half_t* w = nullptr; float* b = nullptr;
            if (hipMalloc((void**)&w, (size_t)3 * d * kp * 2) != hipSuccess || hipMalloc((void**)&b, (size_t)3 * d * 4) != hipSuccess) { set_err(err, errlen, "device allocation failed"); ok = false; }
            else {
                m->allocs.push_back(w); m->allocs.push_back(b);
                hipMemcpy(w, L.q.w, (size_t)d * kp * 2, hipMemcpyDeviceToDevice);
                hipMemcpy(w + (size_t)d * kp, L.k.w, (size_t)d * kp * 2, hipMemcpyDeviceToDevice);
                hipMemcpy(w + (size_t)2 * d * kp, L.v.w, (size_t)d * kp * 2, hipMemcpyDeviceToDevice);
                hipMemset(b, 0, (size_t)3 * d * 4); hipMemcpy(b, L.q.b, (size_t)d * 4, hipMemcpyDeviceToDevice); hipMemcpy(b + 2 * d, L.v.b, (size_t)d * 4, hipMemcpyDeviceToDevice);
                L.qkv.w = w; L.qkv.b = b;
                if (L.q.w_nat && L.k.w_nat && L.v.w_nat) {      // the concatenation again in natural k order
                    half_t* wn = nullptr;
                    if (hipMalloc((void**)&wn, (size_t)3 * d * kp * 2) == hipSuccess) {
                        m->allocs.push_back(wn);
                        hipMemcpy(wn, L.q.w_nat, (size_t)d * kp * 2, hipMemcpyDeviceToDevice);
                        hipMemcpy(wn + (size_t)d * kp, L.k.w_nat, (size_t)d * kp * 2, hipMemcpyDeviceToDevice);
                        hipMemcpy(wn + (size_t)2 * d * kp, L.v.w_nat, (size_t)d * kp * 2, hipMemcpyDeviceToDevice);
                        L.qkv.w_nat = wn;
                    }
                }
            }
            // fragment-order images for the f16 decode kernels (skw_make_wfrag): every decoder projection the small-M kernels multiply by; fc1's rows in its GELU epilogue's order
            if (ok && wfrag_on) {
                auto mk = [&](DevLin& X, int perm) {
                    if ((X.n_out & 15) || (X.k_pad & 31)) return;
                    for (int nat = 0; nat < 2; ++nat) {
                        const half_t* src = nat ? X.w_nat : X.w; if (!src) continue;
                        half_t* img = nullptr; if (hipMalloc((void**)&img, (size_t)X.n_out * X.k_pad * 2) != hipSuccess) continue;      // (no image: the kernels read the rows)
                        m->allocs.push_back(img); skw_make_wfrag(src, X.k_pad, X.n_out, X.k_pad, perm, img, nullptr);
                        (nat ? X.w_nat_frag : X.w_frag) = img;
                    }
                };
                mk(L.qkv, 0); mk(L.o, 0); mk(L.cq, 0); mk(L.co, 0); mk(L.fc1, 1); mk(L.fc2, 0);
                mk(L.ck, 0); mk(L.cv, 0);      // the encoder pass's cross K / V^T products (k_gemm16w streams its weights from these images)
            }
            if (ok && m->quant) {   // the same concatenation in the integer form
                HostQ hq, hk, hv, all; host_q(*find_t(ts, p + "attn.query.weight"), &hq); host_q(*find_t(ts, p + "attn.key.weight"), &hk); host_q(*find_t(ts, p + "attn.value.weight"), &hv);
                all.n_out = 3 * d; all.K = hq.K;
                for (const HostQ* h : {&hq, &hk, &hv}) { all.q.insert(all.q.end(), h->q.begin(), h->q.end());
                all.d.insert(all.d.end(), h->d.begin(), h->d.end()); all.m.insert(all.m.end(), h->m.begin(), h->m.end()); }
                ok = up_q(m, all, m->quant, &L.qkv);
            }
        }
    }
    // Encoder weights as fragment-order images too (k_gemm16w, the f16_mfma precision's big GEMM: weights go from these straight into MFMA operands).  Rows in the
    // order of the epilogue that consumes the product: the kperm'ed-output epilogues (Q / K heads, FC1 and conv1 GELU) want strip row p = logical feature kperm^-1(p).
    if (ok) {
        auto mke = [&](DevLin& X, int perm) {
            if ((X.n_out & 15) || (X.k_pad & 63) || !X.w) return;
            half_t* img = nullptr;
            if (hipMalloc((void**)&img, (size_t)X.n_out * X.k_pad * 2) != hipSuccess) return;      // (no image: k_gemm16 stages the rows through LDS)
            m->allocs.push_back(img);
            skw_make_wfrag(X.w, X.k_pad, X.n_out, X.k_pad, perm, img, nullptr);
            X.w_frag = img;
        };
        mke(m->conv1, 1);
        mke(m->conv2, 0);
        for (EncLayer& L : m->enc) {
            mke(L.q, 1);
            mke(L.k, 1);
            mke(L.v, 0);
            mke(L.o, 0);
            mke(L.fc1, 1);
            mke(L.fc2, 0);
        }
        if (hipDeviceSynchronize() != hipSuccess) ok = false;
    }
    if (!ok) return fail2();
    if ((m->hp.n_audio_state / m->hp.n_audio_head) != 64 || (m->hp.n_text_state / m->hp.n_text_head) != 64 || m->hp.n_audio_state % 128 || m->hp.n_text_state % 128 || m->hp.n_audio_state > 1536) {
        // (a multiple of 128: the decoder's contractions are four contiguous K segments, D3'; every Whisper width — 384, 512, 768, 1024, 1280 — is one)
        set_err(err, errlen, "unsupported model geometry (head dim must be 64, state a multiple of 128 and <= 1536)"); return fail2();
    }
    hipDeviceSynchronize();
    return m;
}
extern "C" void skw_model_free(skw_model* m) { if (!m) return; hipSetDevice(m->device); for (void* p : m->allocs) hipFree(p); delete m; }
extern "C" void skw_model_get_hparams(const skw_model* m, skw_hparams* out) { *out = m->hp; }
extern "C" const char* skw_model_token_text(const skw_model* m, int id, int* len) {
    if (id < 0 || id >= m->hp.n_vocab) { if (len) *len = 0; return ""; }
    if (len) *len = (int)m->tok_str[id].size(); return m->tok_str[id].c_str();
}
extern "C" int skw_model_tokenize(const skw_model* m, const char* text, int32_t* ids, int cap) {
    try { return m->tokz.tokenize_into(text, ids, (ids && cap > 0) ? cap : 0); } catch (const std::exception&) { return 0; }      // (nothing may unwind across the C ABI)
}
