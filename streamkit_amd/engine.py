"""ctypes binding of libskw_engine.so (include/skw_engine.h) — the MI355X Whisper engine.

The library is the product; this module is plumbing for tests and bench.py.  It refuses to run
without the compiled HIP library: there is no Python / CPU fallback for any kernel.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SKW_ENGINE_SO") or os.path.join(_HERE, "libskw_engine.so")      # (SKW_ENGINE_SO: A/B runs against another build of the same library, tools only)
_LIB = None


class HParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_vocab", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                                         "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer", "n_mels", "ftype")]


class FullParams(C.Structure):
    _fields_ = [("lang_id", C.c_int32), ("translate", C.c_int32), ("suppress_blank", C.c_int32), ("suppress_nst", C.c_int32),
                ("no_timestamps", C.c_int32), ("single_segment", C.c_int32), ("max_tokens", C.c_int32),
                ("max_initial_ts", C.c_float), ("entropy_thold", C.c_float), ("logprob_thold", C.c_float),
                ("no_speech_thold", C.c_float), ("n_threads", C.c_int32),
                ("temperature", C.c_float), ("temperature_inc", C.c_float),
                ("audio_ctx", C.c_int32)]      # 0 = the model's n_audio_ctx; K: the clip is encoded and attended over K positions (whisper_full_params.audio_ctx)


BIAS_MAX = 256      # SKW_BIAS_MAX


class DecodeRules(C.Structure):
    """skw_decode_rules: a clip's decoding constraints, applied to the logits of every sampling decision ahead of the sampler (include/skw_engine.h) —
    bias (+ suppression as a -inf bias), then the repetition penalty over the pass's distinct text tokens, then the no-repeat n-gram ban.
    DecodeRules(repetition_penalty=1.1, no_repeat_ngram_size=3, bias={id: b}, suppress=[ids]); no argument: the default record (1.0, 0, no pairs), which asks for nothing."""
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32), ("n_bias", C.c_int32), ("pad", C.c_int32),
                ("bias_id", C.c_int32 * BIAS_MAX), ("bias", C.c_float * BIAS_MAX)]

    def __init__(self, repetition_penalty=1.0, no_repeat_ngram_size=0, bias=None, suppress=None):
        super().__init__()
        self.repetition_penalty = float(repetition_penalty)
        self.no_repeat_ngram_size = _as_int32(no_repeat_ngram_size, "no_repeat_ngram_size")
        pairs = [(int(i), float(b)) for i, b in (bias.items() if hasattr(bias, "items") else (bias or ()))]
        pairs += [(int(i), float("-inf")) for i in (suppress or ())]
        if len(pairs) > BIAS_MAX:
            raise ValueError("DecodeRules: %d biased / suppressed ids, at most %d" % (len(pairs), BIAS_MAX))
        self.n_bias = len(pairs)
        for k, (i, b) in enumerate(pairs):
            self.bias_id[k] = _as_int32(i, "bias id")
            self.bias[k] = b

    def is_default(self):
        return self.repetition_penalty == 1.0 and self.no_repeat_ngram_size == 0 and self.n_bias == 0

    def check(self, n_vocab, who="rules"):
        """The engine's own validation (skw_decode_rules_check), restated so that it needs no device: raises ValueError naming `who`"""
        t = self.repetition_penalty
        if not (np.isfinite(t) and t > 0.0):
            raise ValueError("%s: repetition_penalty %r must be finite and > 0 (1 = off)" % (who, t))
        if self.no_repeat_ngram_size < 0:
            raise ValueError("%s: no_repeat_ngram_size %d must be >= 0 (0 = off)" % (who, self.no_repeat_ngram_size))
        if not 0 <= self.n_bias <= BIAS_MAX:
            raise ValueError("%s: n_bias %d outside [0, %d]" % (who, self.n_bias, BIAS_MAX))
        seen = set()
        for k in range(self.n_bias):
            i, b = self.bias_id[k], self.bias[k]
            if not 0 <= i < n_vocab:
                raise ValueError("%s: bias %d: token id %d outside [0, %d)" % (who, k, i, n_vocab))
            if i in seen:
                raise ValueError("%s: bias %d: token id %d is given twice" % (who, k, i))
            seen.add(i)
            if np.isnan(b) or b == float("inf"):
                raise ValueError("%s: bias %d (token %d): %r is not finite or -inf" % (who, k, i, b))


def _as_int32(v, what):
    v = int(v)
    if not -2**31 <= v < 2**31:
        raise ValueError("DecodeRules: %s %d does not fit an int32" % (what, v))
    return v


def rules_array(rules, n, n_vocab, who):
    """[DecodeRules | None] * n -> (the checked records kept alive, (c_void_p * n) of their addresses, NULL where None)"""
    if len(rules) != n:
        raise ValueError("%d rule records for %d %ss" % (len(rules), n, who))
    for i, r in enumerate(rules):
        if r is not None:
            if not isinstance(r, DecodeRules):
                raise ValueError("%s %d: rules must be DecodeRules or None" % (who, i))
            r.check(n_vocab, "%s %d" % (who, i))
    return list(rules), _ptr_array(rules, C.addressof)


GRAMMAR_MAX_STATES = 4096      # SKW_GRAMMAR_MAX_STATES
GRAMMAR_DEAD = 0xFFFF          # SKW_GRAMMAR_DEAD
GRAMMAR_IGNORE_CASE = 1        # SKW_GRAMMAR_IGNORE_CASE


class GrammarRec(C.Structure):      # skw_grammar (include/skw_grammar.h)
    _fields_ = [("n_states", C.c_int32), ("next", C.c_void_p), ("accept", C.c_void_p), ("penalty", C.c_float)]


class Grammar:
    """A grammar for grammar-constrained decoding (include/skw_grammar.h): a dense byte-level DFA — next uint16 [n_states][256] (GRAMMAR_DEAD: no match can continue), accept
    uint8 [n_states], state 0 the start — and the finite penalty > 0 that tokens which cannot continue a match lose.  Regular languages only (whisper.cpp's GBNF is a pushdown
    grammar; this is its regular subset).  Grammar.compile(pattern) builds the tables from a regular expression (full match over bytes; the subset of
    streamkit_amd/csrc/skw_grammar_compile.h); Grammar.from_tables(next, accept, penalty) takes them as they are — the engine checks them when they are used."""

    def __init__(self, nxt, accept, penalty):
        self.next = np.ascontiguousarray(nxt, dtype=np.uint16).reshape(-1, 256)
        self.accept = np.ascontiguousarray(accept, dtype=np.uint8).reshape(-1)
        self.penalty = float(penalty)
        self.rec = GrammarRec(self.accept.size, self.next.ctypes.data, self.accept.ctypes.data, self.penalty)

    @classmethod
    def from_tables(cls, nxt, accept, penalty=100.0):
        return cls(nxt, accept, penalty)

    @classmethod
    def compile(cls, pattern, ignore_case=False, penalty=100.0):
        """pattern: str (taken as its UTF-8 bytes) or bytes.  Raises ValueError with the compiler's message."""
        pat = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        out = C.c_void_p(); err = C.create_string_buffer(256)
        if lib().skw_grammar_compile(pat, len(pat), GRAMMAR_IGNORE_CASE if ignore_case else 0, float(penalty), C.byref(out), err, 256) != 0:
            raise ValueError(err.value.decode(errors="replace"))
        try:
            rec = GrammarRec.from_address(out.value)
            n = rec.n_states
            nxt = np.frombuffer((C.c_uint16 * (n * 256)).from_address(rec.next), dtype=np.uint16).copy()
            acc = np.frombuffer((C.c_uint8 * n).from_address(rec.accept), dtype=np.uint8).copy()
        finally:
            lib().skw_grammar_free(out)
        return cls(nxt, acc, penalty)

    @property
    def n_states(self):
        return int(self.accept.size)

    def walk(self, data, state=0):
        """the state after `data` from `state`, or GRAMMAR_DEAD"""
        s = int(state)
        for b in bytes(data):
            if s == GRAMMAR_DEAD:
                break
            s = int(self.next[s, b])
        return s

    def matches(self, data):
        s = self.walk(data)
        return s != GRAMMAR_DEAD and bool(self.accept[s])


def grammars_array(grammars, n, who):
    """[Grammar | None] * n -> (c_void_p * n) of the records' addresses, NULL where None (the Grammar objects keep the tables alive: hold on to the list)"""
    if len(grammars) != n:
        raise ValueError("%d grammars for %d %ss" % (len(grammars), n, who))
    for i, g in enumerate(grammars):
        if g is not None and not isinstance(g, Grammar):
            raise ValueError("%s %d: grammars must be Grammar or None" % (who, i))
    return _ptr_array(grammars, lambda g: C.addressof(g.rec))


class Segment(C.Structure):
    _fields_ = [("t0", C.c_int64), ("t1", C.c_int64), ("tok_begin", C.c_int32), ("tok_end", C.c_int32),
                ("text_off", C.c_int32), ("text_len", C.c_int32)]


class Token(C.Structure):
    _fields_ = [("id", C.c_int32), ("tid", C.c_int32), ("p", C.c_float), ("plog", C.c_float), ("pt", C.c_float), ("ptsum", C.c_float), ("margin", C.c_float)]


class Result(C.Structure):
    _fields_ = [("n_segments", C.c_int32), ("n_tokens", C.c_int32), ("n_windows", C.c_int32), ("n_decode_steps", C.c_int32),
                ("fallback_requested", C.c_int32), ("min_margin", C.c_float),
                ("segments", C.POINTER(Segment)), ("tokens", C.POINTER(Token)), ("text", C.c_void_p), ("text_len", C.c_int32), ("lang_id", C.c_int32)]


class Timing(C.Structure):
    _fields_ = [("mel_ms", C.c_float), ("encode_ms", C.c_float), ("decode_ms", C.c_float), ("total_ms", C.c_float),
                ("n_windows", C.c_int32), ("n_decode_steps", C.c_int32), ("n_tokens", C.c_int32), ("n_row_steps", C.c_int32),
                ("decode_groups", C.c_int32), ("decode_group_rows", C.c_int32)]


class Trace(C.Structure):
    _fields_ = [("n", C.c_int32), ("steps", C.c_void_p)]


TRACE_DT = np.dtype([("chosen_id", "<i4"), ("forced_id", "<i4"), ("top1_id", "<i4"), ("top2_id", "<i4"),
                     ("top1", "<f4"), ("top2", "<f4"), ("forced_logit", "<f4"), ("lse", "<f4"), ("temperature", "<f4"), ("pad", "<i4")])      # skw_trace_step


class ResamplerState(C.Structure):
    _fields_ = [("last_index", C.c_double), ("ratio", C.c_double), ("chunk_frames", C.c_int32), ("channels", C.c_int32), ("hist", C.c_float * 32)]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libskw_engine.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                               "the engine has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.skw_device_count.restype = C.c_int
        L.skw_model_load.restype = C.c_void_p
        L.skw_model_load.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
        L.skw_model_load_ex.restype = C.c_void_p
        L.skw_model_load_ex.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        L.skw_model_quant_type.argtypes = [C.c_void_p]
        L.skw_model_free.argtypes = [C.c_void_p]
        L.skw_model_get_hparams.argtypes = [C.c_void_p, C.POINTER(HParams)]
        L.skw_model_token_text.restype = C.c_void_p
        L.skw_model_token_text.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.skw_model_lang_id.argtypes = [C.c_char_p]
        L.skw_ctx_create.restype = C.c_void_p
        L.skw_ctx_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        L.skw_ctx_free.argtypes = [C.c_void_p]
        L.skw_ctx_last_error.restype = C.c_char_p
        L.skw_ctx_last_error.argtypes = [C.c_void_p]
        L.skw_ctx_set_precision.argtypes = [C.c_void_p, C.c_int]
        L.skw_ctx_get_precision.argtypes = [C.c_void_p]
        L.skw_ctx_set_cross_kv.argtypes = [C.c_void_p, C.c_int]
        L.skw_ctx_get_cross_kv.argtypes = [C.c_void_p]
        for name in ("kq", "kd", "vq", "vd"):
            f = getattr(L, "skw_layout_kv8_%s_off" % name); f.restype = C.c_long; f.argtypes = [C.c_int] * 5
        L.skw_layout_kv8_slot_bytes.restype = C.c_long
        L.skw_layout_kv8_slot_bytes.argtypes = [C.c_int, C.c_int]
        L.skw_debug_kv8_quantize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.skw_debug_attn_kv8.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
        L.skw_ctx_stream.restype = C.c_void_p
        L.skw_ctx_stream.argtypes = [C.c_void_p]
        L.skw_ctx_last_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
        L.skw_full_default_params.argtypes = [C.POINTER(FullParams)]
        L.skw_full_batch.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(Result)]
        L.skw_full_batch_rng.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(Result)]
        L.skw_full_batch_mixed.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(Result)]
        L.skw_full_batch_context.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(Result)]
        L.skw_decode_rules_default.argtypes = [C.POINTER(DecodeRules)]
        L.skw_full_batch_rules.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(Result)]
        L.skw_debug_sample_rows_rules.argtypes = [C.c_void_p, C.POINTER(FullParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_void_p)]
        L.skw_model_tokenize.argtypes =[C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]
        L.skw_debug_set_prompt_pass.argtypes = [C.c_void_p, C.c_int]
        L.skw_debug_set_prompt_xattn_mq.argtypes = [C.c_void_p, C.c_int]
        L.skw_debug_xattn_exact.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        L.skw_rng_state_init.argtypes = [C.c_void_p]
        L.skw_result_free.argtypes = [C.POINTER(Result)]
        L.skw_full_batch_traced.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(Trace), C.POINTER(Result)]
        L.skw_full_batch_traced_context.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(Trace), C.POINTER(C.c_void_p), C.POINTER(Result)]
        L.skw_trace_free.argtypes = [C.POINTER(Trace)]
        L.skw_log_mel.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.skw_conv_stem.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.skw_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_decode_logits.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.skw_conv_stem_actx.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.skw_encode_actx.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_audio_ctx_for_samples.argtypes = [C.c_int, C.c_int]
        L.skw_ctx_kernel_clock_keys.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.skw_dsp_create.restype = C.c_void_p
        L.skw_dsp_create.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        L.skw_dsp_free.argtypes = [C.c_void_p]
        L.skw_dsp_last_error.restype = C.c_char_p
        L.skw_dsp_last_error.argtypes = [C.c_void_p]
        L.skw_resampler_init.argtypes = [C.POINTER(ResamplerState), C.c_double, C.c_int, C.c_int]
        L.skw_resample_linear.argtypes = [C.c_void_p, C.POINTER(ResamplerState), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.skw_resample_polyphase.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
        L.skw_dsp_last_scan_fallback.argtypes = [C.c_void_p]
        L.skw_polyphase_stream_create.restype = C.c_void_p
        L.skw_polyphase_stream_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.skw_polyphase_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
        L.skw_polyphase_stream_free.argtypes = [C.c_void_p]
        L.skw_ctx_profile.argtypes = [C.c_void_p, C.c_int]
        L.skw_ctx_profile_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.skw_debug_math.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
        L.skw_debug_sample_rows.argtypes = [C.c_void_p, C.POINTER(FullParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_debug_sample_rows_mixed.argtypes = [C.c_void_p, C.POINTER(FullParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_debug_sample_rows_ex.argtypes = [C.c_void_p, C.POINTER(FullParams), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(SampleRowsEx)]
        L.skw_debug_enable.argtypes = [C.c_int]
        L.skw_debug_get.restype = C.c_long
        L.skw_debug_get.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
        L.skw_ctx_kernel_clock.argtypes = [C.c_void_p, C.c_int]
        L.skw_ctx_kernel_clock_get.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.skw_ctx_kernel_clock_records.restype = C.c_long; L.skw_ctx_kernel_clock_records.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
        L.skw_debug_xattn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.skw_debug_switch_name.restype = C.c_char_p; L.skw_debug_switch_name.argtypes = [C.c_int]
        L.skw_debug_switch_what.restype = C.c_char_p; L.skw_debug_switch_what.argtypes = [C.c_int]
        L.skw_debug_switch_default.argtypes = [C.c_int]
        L.skw_debug_switch_get.argtypes = [C.c_char_p]
        L.skw_debug_switch_set.argtypes = [C.c_char_p, C.c_int]
        L.skw_debug_attn16.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
        L.skw_debug_attn_exact.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.skw_debug_gemm_q8.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.POINTER(C.c_int)])
        L.skw_debug_q8_quantize.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_debug_self_attn_q8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 10
        L.skw_debug_gemm16_epi.argtypes = [C.c_void_p, C.POINTER(Gemm16EpiArgs)]
        L.skw_debug_align_qk.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_int] + [C.c_void_p] * 5
        L.skw_debug_align_reduce.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.skw_debug_align_dtw.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.skw_align_params_check.argtypes = [C.c_void_p, C.POINTER(AlignParams), C.c_int]
        L.skw_full_batch_aligned.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(TokenTimes), C.POINTER(Result)]
        L.skw_align_batch.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_void_p), C.POINTER(TokenTimes)]
        L.skw_token_times_free.argtypes = [C.POINTER(TokenTimes)]
        L.skw_full_batch_grammar.argtypes = [C.c_void_p, C.POINTER(FullParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(TokenTimes), C.POINTER(C.c_void_p), C.POINTER(Result)]
        L.skw_grammar_compile.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
        L.skw_grammar_free.argtypes = [C.c_void_p]
        L.skw_debug_grammar_uploads.restype = C.c_long; L.skw_debug_grammar_uploads.argtypes = [C.c_void_p]
        L.skw_full_batch_request.argtypes = [C.c_void_p, C.POINTER(FullRequest)]
        L.skw_debug_sample_rows_request.argtypes = [C.c_void_p, C.POINTER(SampleRowsRequest)]
        L.skw_debug_sample_rows_grammar.argtypes = [C.c_void_p, C.POINTER(FullParams), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
        _LIB = L
    return _LIB


class AlignParams(C.Structure):        # skw_align_params (include/skw_align.h)
    _fields_ = [("enabled", C.c_int32), ("median_width", C.c_int32), ("head_mask", C.c_uint32 * 32)]


class TokenTimes(C.Structure):         # skw_token_times
    _fields_ = [("n", C.c_int32), ("t0", C.POINTER(C.c_int64)), ("t1", C.POINTER(C.c_int64))]


def align_params(head_mask=None, median_width=7, top=None, hp=None):
    """An enabled skw_align_params.  head_mask: one uint32 per decoder layer (bit h = head h), or [(layer, head), ...]; or top=N with hp: every head of the top N decoder layers
    (whisper.cpp's N_TOP_MOST; N = n_text_layer // 2 is openai's default for a model that names no heads)."""
    p = AlignParams(enabled=1, median_width=int(median_width))
    if top is not None:
        head_mask = [((1 << hp.n_text_head) - 1 if hp.n_text_layer - min(top, hp.n_text_layer) <= l < hp.n_text_layer else 0) for l in range(hp.n_text_layer)]
    if head_mask and isinstance(head_mask[0], (tuple, list)):
        for l, h in head_mask:
            p.head_mask[l] |= 1 << h
    else:
        for l, w in enumerate(head_mask or []):
            p.head_mask[l] = int(w)
    return p


def _times_out(tt):
    out = [(int(tt.t0[k]), int(tt.t1[k])) for k in range(tt.n)]
    lib().skw_token_times_free(C.byref(tt))
    return out


class Gemm16EpiArgs(C.Structure):      # struct skw_gemm16_epi_args (skw_hooks.hip)
    _fields_ = [("launcher", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("epi", C.c_int32),
                ("A", C.c_void_p), ("a_halves", C.c_int64), ("lda", C.c_int64), ("a_rows_per_batch", C.c_int32), ("a_batch_stride", C.c_int64), ("a_frag", C.c_int32),
                ("ln_x", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p),
                ("W", C.c_void_p), ("use_wf", C.c_int32),
                ("bias", C.c_void_p), ("res", C.c_void_p), ("ldres", C.c_int64), ("res_alias", C.c_int32),
                ("scale", C.c_float), ("has_scale", C.c_int32),
                ("pe", C.c_void_p), ("n_ctx", C.c_int32), ("H", C.c_int32), ("Tpad", C.c_int32), ("frag", C.c_int32), ("c_frag", C.c_int32),
                ("pos", C.c_void_p), ("force_small", C.c_int32),
                ("C", C.c_void_p), ("c_bytes", C.c_int64), ("ldc", C.c_int64), ("C2", C.c_void_p), ("C3", C.c_void_p), ("c2_bytes", C.c_int64), ("ldc2", C.c_int64),
                ("kernel_id", C.c_int32)]


class SampleRowsEx(C.Structure):      # skw_sample_rows_ex (skw_engine.hip)
    _fields_ = [("temperature", C.c_void_p), ("rng_state", C.c_void_p), ("trace", C.c_int32), ("kernel_id", C.c_int32), ("probs_out", C.c_void_p), ("no_speech_prob", C.c_void_p),
                ("n_tokens", C.c_void_p), ("cur_token", C.c_void_p), ("active", C.c_void_p)]


class FullRequest(C.Structure):      # skw_full_request (include/skw_engine.h): what every full_batch / align_batch call is
    _fields_ = [("size", C.c_uint32), ("params_per_clip", C.c_int32), ("params", C.POINTER(FullParams)),
                ("pcm", C.POINTER(C.c_void_p)), ("n_samples", C.POINTER(C.c_int32)), ("n_clips", C.c_int32), ("pcm_on_device", C.c_int32),
                ("rng_state", C.POINTER(C.c_void_p)), ("context", C.POINTER(C.c_void_p)), ("rules", C.POINTER(C.c_void_p)),
                ("align", C.POINTER(C.c_void_p)), ("times", C.POINTER(TokenTimes)), ("grammar", C.POINTER(C.c_void_p)),
                ("text_tokens", C.POINTER(C.c_void_p)), ("n_text", C.POINTER(C.c_int32)),
                ("forced_ids", C.POINTER(C.c_void_p)), ("n_forced", C.POINTER(C.c_int32)), ("traces", C.POINTER(Trace)), ("results", C.POINTER(Result))]


FULL_REQUEST_MIN = 136      # SKW_FULL_REQUEST_MIN


class SampleRowsRequest(C.Structure):      # skw_sample_rows_request (include/skw_engine.h): what every sample_rows call is
    _fields_ = [("params_per_row", C.c_int32), ("n_rows", C.c_int32), ("params", C.POINTER(FullParams)),
                ("hist", C.c_void_p), ("hist_stride", C.c_int32), ("form", C.c_int32), ("n_hist", C.c_void_p), ("logits", C.c_void_p),
                ("filtered_out", C.c_void_p), ("tok_out", C.c_void_p), ("trace_out", C.c_void_p),
                ("rules", C.POINTER(C.c_void_p)), ("grammar", C.POINTER(C.c_void_p)), ("active", C.c_void_p),
                ("temperature", C.c_void_p), ("rng_state", C.c_void_p), ("trace", C.c_int32), ("kernel_id", C.c_int32),
                ("probs_out", C.c_void_p), ("no_speech_prob", C.c_void_p), ("n_tokens", C.c_void_p), ("cur_token", C.c_void_p), ("active_out", C.c_void_p)]


def _ptr_array(items, address):
    """[object | None] * n -> (c_void_p * n) of address(object), NULL where None (the caller keeps the objects alive)"""
    return (C.c_void_p * len(items))(*[None if x is None else address(x) for x in items])


def _params_for(p, per, n):
    """the request's params: a list as an array, one block repeated n times where the launch is the per-clip / per-row one (per), else the block itself"""
    if isinstance(p, (list, tuple)):
        return (FullParams * len(p))(*p)
    return (FullParams * n)(*([p] * n)) if per else C.pointer(p)


# what a sampler launch ran (SKW_SMPK_* of skw_kernels.h): k_dec_sample<TRACE, DRAW, ROWS> or k_dec_sample_stream<ROWS>
def sampler_kernel_name(kernel_id):
    b = lambda m: "true" if kernel_id & m else "false"
    return "k_dec_sample_stream<%s>" % b(1) if kernel_id & 8 else "k_dec_sample<%s, %s, %s>" % (b(4), b(2), b(1))


_TOKEN_DT = np.dtype([("id", "<i4"), ("tid", "<i4"), ("p", "<f4"), ("plog", "<f4"), ("pt", "<f4"), ("ptsum", "<f4"), ("margin", "<f4")])      # struct Token
_SEGMENT_DT = np.dtype([("t0", "<i8"), ("t1", "<i8"), ("tok_begin", "<i4"), ("tok_end", "<i4"), ("text_off", "<i4"), ("text_len", "<i4")])      # struct Segment
assert _TOKEN_DT.itemsize == C.sizeof(Token) and _SEGMENT_DT.itemsize == C.sizeof(Segment)


def _result_to_dict(r):
    text = C.string_at(r.text, r.text_len) if r.text else b""
    if r.n_tokens > 0:      # one structured view of the token array instead of five ctypes field reads per token (5 ms per 64 results in the bench's timed step)
        a = np.frombuffer((C.c_char * (r.n_tokens * C.sizeof(Token))).from_address(C.addressof(r.tokens.contents)), dtype=_TOKEN_DT)
        toks = list(zip(a["id"].tolist(), a["tid"].tolist(), a["p"].tolist(), a["plog"].tolist(), a["margin"].tolist()))
    else:
        toks = []
    segs = []
    if r.n_segments > 0:
        sg = np.frombuffer((C.c_char * (r.n_segments * C.sizeof(Segment))).from_address(C.addressof(r.segments.contents)), dtype=_SEGMENT_DT).tolist()
        segs = [dict(t0=t0, t1=t1, tokens=[t[0] for t in toks[b:e]], text=text[o:o + n]) for (t0, t1, b, e, o, n) in sg]
    return dict(segments=segs, tokens=toks, n_windows=r.n_windows, n_decode_steps=r.n_decode_steps,
                fallback_requested=r.fallback_requested, min_margin=r.min_margin, lang_id=r.lang_id)


def audio_ctx_for_samples(n_samples, n_audio_ctx=1500):
    """The "auto" rule for FullParams.audio_ctx (skw_audio_ctx_for_samples): the positions the audio covers, half a second of margin, whole 32-key blocks.  No GPU needed."""
    return lib().skw_audio_ctx_for_samples(int(n_samples), int(n_audio_ctx))


CONTEXT_WORDS = 513      # SKW_CONTEXT_WORDS


def context_new(ids=()):
    """A clip owner's carried text (whisper_state::prompt_past) as an int32[513]: [0] = n, [1 .. n] = token ids, oldest first (at most 512)"""
    ids = [int(x) for x in ids]
    assert len(ids) <= CONTEXT_WORDS - 1
    a = np.zeros(CONTEXT_WORDS, np.int32)
    a[0] = len(ids)
    a[1:1 + len(ids)] = ids
    return a


def context_ids(a):
    return [int(x) for x in a[1:1 + int(a[0])]]


def rng_state_new():
    """std::mt19937(0) as a uint32[625] (mt + index): the generator a freshly created whisper_state owns"""
    s = np.zeros(625, np.uint32)
    lib().skw_rng_state_init(s.ctypes.data)
    return s


class Model:
    def __init__(self, path, device=0, quant_mode=1):
        """quant_mode (block-quantised files): 1 = ggml's q8 arithmetic in the exact precision (SKW_QUANT_GGML), 0 = the dequantised f16 twin everywhere"""
        L = lib()
        err = C.create_string_buffer(512)
        self.h = L.skw_model_load_ex(path.encode(), device, int(quant_mode), err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())
        self.quant = L.skw_model_quant_type(self.h)
        self.hp = HParams()
        L.skw_model_get_hparams(self.h, C.byref(self.hp))

    def token_bytes(self, i):
        n = C.c_int()
        p = lib().skw_model_token_text(self.h, i, C.byref(n))
        return C.string_at(p, n.value)

    def tokenize(self, text):
        """whisper_tokenize (skw_model_tokenize): whisper.cpp's tokenizer on `text` (str or bytes) -> list of ids.  Nothing is put in front of the text."""
        b = text.encode() if isinstance(text, str) else bytes(text)
        n = lib().skw_model_tokenize(self.h, b, None, 0)
        if n == 0:
            return []
        ids = np.zeros(-n, np.int32)
        n = lib().skw_model_tokenize(self.h, b, ids.ctypes.data, ids.size)
        assert n == ids.size
        return ids.tolist()

    def close(self):
        if self.h:
            lib().skw_model_free(self.h)
            self.h = None


class Context:
    def __init__(self, model, max_batch=1, max_samples=0):
        err = C.create_string_buffer(512)
        self.model = model
        self.h = lib().skw_ctx_create(model.h, max_batch, max_samples, err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError("skw engine: " + lib().skw_ctx_last_error(self.h).decode())

    def last_error(self):
        return lib().skw_ctx_last_error(self.h).decode()

    PRECISIONS = {"exact": 0, "f16_mfma": 1}

    def set_precision(self, name):
        """'exact' (f32-chain contractions, bit-identical to the oracle) or 'f16_mfma' (f16 matrix cores: every greedy decision equals the exact
        mode's given the same history unless that step was a near-tie; a free-running transcript is identical up to its first near-tie)."""
        self._check(lib().skw_ctx_set_precision(self.h, self.PRECISIONS[name]))

    def get_precision(self):
        v = lib().skw_ctx_get_precision(self.h)
        return [k for k, x in self.PRECISIONS.items() if x == v][0]

    CROSS_KV = {"f16": 0, "q8_0": 1}

    def set_cross_kv(self, name):
        """'f16' (default) or 'q8_0': the decode steps' cross attention streams cross K / V as ggml q8_0 blocks (include/skw_kv8.h) — half the bytes of every step.  Effective
        only with precision 'f16_mfma'; the exact precision ignores it.  From the next call on this context."""
        self._check(lib().skw_ctx_set_cross_kv(self.h, self.CROSS_KV[name]))

    def get_cross_kv(self):
        v = lib().skw_ctx_get_cross_kv(self.h)
        return [k for k, x in self.CROSS_KV.items() if x == v][0]

    def default_params(self):
        p = FullParams()
        lib().skw_full_default_params(C.byref(p))
        return p

    def full_batch(self, clips, params=None, device_ptrs=None, n_samples=None, trace=False, forced=None, rng_states=None, contexts=None, rules=None, align=None,
                   grammars=None):
        """clips: list of 1-D float32 numpy arrays (host), or device_ptrs + n_samples for HBM-resident PCM.
        trace=True (or forced=[per-clip int32 id sequences]): skw_full_batch_traced — returns (results, traces), traces[i] a structured
        array (TRACE_DT) with one record per sampling decision of clip i; with `forced` the decoder is fed those ids (teacher forcing).
        rng_states=[uint32[625] or None per clip] (rng_state_new()): the temperature ladder's std::mt19937 stream of each clip's OWNER, continued and updated in place
        (skw_full_batch_rng: whisper.cpp keeps one generator per state and lets it run on across calls).
        params=[FullParams per clip]: skw_full_batch_mixed — every clip decodes under its own parameters in the one batch (rng_states allowed with it).  Tracing / teacher
        forcing takes one FullParams and no rng_states: either combination raises ValueError.
        contexts=[int32[513] or None per clip] (context_new()): skw_full_batch_context — each clip decodes behind its owner's carried text (prompt_past: [0] = n, then n ids,
        an initial prompt's tokens in front) and the array is updated in place to what the call leaves, like rng_states.  One FullParams is repeated per clip.  With trace / forced:
        skw_full_batch_traced_context.
        rules=[DecodeRules or None per clip]: skw_full_batch_rules — each clip's decoding constraints (repetition penalty, no-repeat n-gram, bias / suppression); None or a default
        record leaves the clip as it is without.  May be combined with per-clip params, rng_states and contexts; with trace / forced it raises ValueError.  The records are checked
        here as the engine checks them (ValueError naming the clip).
        align=[AlignParams or None per clip] (align_params()): skw_full_batch_aligned — the clips that ask get word timestamps: each result gains "token_times", one (t0, t1) in
        centiseconds per token of "tokens", (-1, -1) for timestamp tokens and for clips that did not ask.  May be combined with per-clip params, rng_states, contexts and rules; not
        with trace / forced.
        grammars=[Grammar or None per clip]: skw_full_batch_grammar — the clips that bring one are decoded under it (tokens whose text cannot continue a match lose the
        grammar's penalty, <|endoftext|> loses it while the match is incomplete); None leaves the clip as it is without.  May be combined with everything align may."""
        per_clip = isinstance(params, (list, tuple))
        tracing = trace or forced is not None
        if grammars is not None and tracing:
            raise ValueError("full_batch: grammars cannot be combined with trace / forced (grammars are not part of the traced entries)")
        if align is not None and tracing:
            raise ValueError("full_batch: align cannot be combined with trace / forced")
        rq = FullRequest(size=C.sizeof(FullRequest))
        if rules is not None:
            if tracing:
                raise ValueError("full_batch: rules cannot be combined with trace / forced (there is no traced entry point with decoding constraints)")
            n_in = len(device_ptrs) if device_ptrs is not None else len(clips)
            rules_keep, rq.rules = rules_array(rules, n_in, self.model.hp.n_vocab, "clip")
        if tracing:      # (checked before anything touches the library or the device)
            if per_clip:
                raise ValueError("full_batch: trace / forced take one FullParams, not a list (tracing with per-clip parameters is not supported)")
            if rng_states is not None:
                raise ValueError("full_batch: rng_states cannot be combined with trace / forced (the traced call starts every generator at seed 0)")
        if device_ptrs is not None:
            n = len(device_ptrs)
            rq.pcm = (C.c_void_p * n)(*device_ptrs)
            rq.n_samples = (C.c_int32 * n)(*n_samples)
            rq.pcm_on_device = 1
        else:
            clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
            n = len(clips)
            rq.pcm = _ptr_array(clips, lambda c: c.ctypes.data)
            rq.n_samples = (C.c_int32 * n)(*[c.size for c in clips])
        if per_clip and len(params) != n:
            raise ValueError("full_batch: %d parameter blocks for %d clips" % (len(params), n))
        # the per-clip launches as soon as a per-clip feature is asked for (the traced call takes contexts and stays uniform), the uniform ones otherwise
        rq.params_per_clip = 1 if per_clip or grammars is not None or align is not None or rules is not None or (contexts is not None and not tracing) else 0
        rq.params = _params_for(params or self.default_params(), rq.params_per_clip, n)
        rq.n_clips = n
        res = (Result * n)()
        rq.results = res
        if contexts is not None:
            if len(contexts) != n:
                raise ValueError("full_batch: %d contexts for %d clips" % (len(contexts), n))
            assert all(x is None or (x.dtype == np.int32 and x.size == CONTEXT_WORDS and x.flags["C_CONTIGUOUS"]) for x in contexts)
            rq.context = _ptr_array(contexts, lambda x: x.ctypes.data)
        if grammars is not None:
            rq.grammar = grammars_array(grammars, n, "clip")
        times = None
        if align is not None:
            if len(align) != n:
                raise ValueError("full_batch: %d alignment records for %d clips" % (len(align), n))
            rq.align = _ptr_array(align, C.addressof)
            times = (TokenTimes * n)()
            rq.times = times
        if rng_states is not None:
            assert len(rng_states) == n and all(s is None or (s.dtype == np.uint32 and s.size == 625 and s.flags["C_CONTIGUOUS"]) for s in rng_states)
            rq.rng_state = _ptr_array(rng_states, lambda s: s.ctypes.data)
        if tracing:
            tr = (Trace * n)()
            rq.traces = tr
            if forced is not None:
                keep = [np.ascontiguousarray(f, dtype=np.int32) for f in forced]
                rq.forced_ids = _ptr_array(keep, lambda k: k.ctypes.data)
                rq.n_forced = (C.c_int32 * n)(*[k.size for k in keep])
        self._check(lib().skw_full_batch_request(self.h, C.byref(rq)))
        out = [_result_to_dict(res[i]) for i in range(n)]
        for i in range(n):
            lib().skw_result_free(C.byref(res[i]))
        if times is not None:
            for i in range(n):
                out[i]["token_times"] = _times_out(times[i])
        if tracing:
            traces = []
            for i in range(n):
                a = np.frombuffer((C.c_char * (tr[i].n * TRACE_DT.itemsize)).from_address(tr[i].steps), dtype=TRACE_DT).copy() if tr[i].n else np.zeros(0, TRACE_DT)
                traces.append(a)
                lib().skw_trace_free(C.byref(tr[i]))
            return out, traces
        return out

    def align_batch(self, clips, texts, align, params=None):
        """skw_align_batch: forced alignment of given text — clips[i] (at most 30 s) against the text token ids texts[i]; nothing is decoded.
        -> per clip a list of (t0, t1) in centiseconds, one per given token."""
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        n = len(clips)
        keep = [np.ascontiguousarray(t, dtype=np.int32) for t in texts]
        times = (TokenTimes * n)()
        rq = FullRequest(size=C.sizeof(FullRequest), params_per_clip=1, params=_params_for(params or self.default_params(), 1, n), n_clips=n,
                         pcm=_ptr_array(clips, lambda c: c.ctypes.data), n_samples=(C.c_int32 * n)(*[c.size for c in clips]),
                         text_tokens=_ptr_array(keep, lambda k: k.ctypes.data), n_text=(C.c_int32 * n)(*[k.size for k in keep]),
                         align=_ptr_array(align, C.addressof), times=times)
        self._check(lib().skw_full_batch_request(self.h, C.byref(rq)))
        return [_times_out(times[i]) for i in range(n)]

    def set_prompt_pass(self, on):
        """test hook (skw_debug_set_prompt_pass): 0 = the prompt is stepped token by token instead of evaluated in one pass"""
        lib().skw_debug_set_prompt_pass(self.h, 1 if on else 0)

    def set_prompt_xattn_mq(self, on):
        """test hook (skw_debug_set_prompt_xattn_mq): 0 = the exact precision's prompt pass keeps the single-query cross attention (same bits, one K / V^T read per prompt row)"""
        lib().skw_debug_set_prompt_xattn_mq(self.h, 1 if on else 0)

    def timing(self):
        t = Timing()
        lib().skw_ctx_last_timing(self.h, C.byref(t))
        return {f: getattr(t, f) for f, _ in t._fields_}

    def profile(self, on=True):
        lib().skw_ctx_profile(self.h, 1 if on else 0)

    def profile_get(self):
        out = {}
        for cls in range(14):
            name = C.create_string_buffer(64); cnt = C.c_long(); ms = C.c_double(); fl = C.c_double(); by = C.c_double()
            if lib().skw_ctx_profile_get(self.h, cls, name, 64, C.byref(cnt), C.byref(ms), C.byref(fl), C.byref(by)) == 0:
                out[name.value.decode()] = dict(count=cnt.value, ms=ms.value, flops=fl.value, bytes=by.value)
        return out

    def kernel_clock(self, on=True):
        """Arms / disarms the in-kernel launch clock of the decode step's cross attention (include/skw_engine.h, skw_ctx_kernel_clock)."""
        self._check(lib().skw_ctx_kernel_clock(self.h, 1 if on else 0))

    def kernel_clock_get(self):
        n = C.c_long(); su = C.c_double(); sl = C.c_double(); mn = C.c_double(); mx = C.c_double(); khz = C.c_int()
        self._check(lib().skw_ctx_kernel_clock_get(self.h, C.byref(n), C.byref(su), C.byref(sl), C.byref(mn), C.byref(mx), C.byref(khz)))
        return dict(launches=n.value, sum_us=su.value, sum_live_rows=sl.value, min_us=mn.value, max_us=mx.value, clock_khz=khz.value)

    def kernel_clock_keys(self):
        """keys walked by the recorded launches, summed over their live rows (algorithmic bytes = 4 B x this x n_text_state)"""
        sk = C.c_double()
        self._check(lib().skw_ctx_kernel_clock_keys(self.h, C.byref(sk)))
        return sk.value

    def kernel_clock_records(self, cap=65536):
        """[(begin us, end us, live rows)] of every launch the last call recorded"""
        out = np.zeros((cap, 3), np.float64)
        n = lib().skw_ctx_kernel_clock_records(self.h, out.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("skw engine: " + self.last_error())
        return out[:n].copy()

    def stream(self):
        return lib().skw_ctx_stream(self.h)

    def log_mel(self, pcm):
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        hp = self.model.hp
        cap = hp.n_mels * ((pcm.size + 480000) // 160 + 8)
        out = np.empty(cap, dtype=np.float32)
        n_len, n_org = C.c_int(), C.c_int()
        self._check(lib().skw_log_mel(self.h, pcm.ctypes.data, pcm.size, out.ctypes.data, cap, C.byref(n_len), C.byref(n_org)))
        return out[:hp.n_mels * n_len.value].reshape(hp.n_mels, n_len.value).copy(), n_org.value

    def conv_stem(self, pcm, seek=0, audio_ctx=None):
        """audio_ctx=K (skw_conv_stem_actx; 0 = n_audio_ctx): the stem at K positions, [K][n_state]; None: the existing tap"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        hp = self.model.hp
        if audio_ctx is None:
            out = np.empty((hp.n_audio_ctx, hp.n_audio_state), dtype=np.float32)
            self._check(lib().skw_conv_stem(self.h, pcm.ctypes.data, pcm.size, seek, out.ctypes.data))
            return out
        K = audio_ctx if 0 < audio_ctx <= hp.n_audio_ctx else hp.n_audio_ctx      # (the buffer's size; the library refuses what is out of range)
        out = np.empty((K, hp.n_audio_state), dtype=np.float32)
        self._check(lib().skw_conv_stem_actx(self.h, pcm.ctypes.data, pcm.size, seek, int(audio_ctx), out.ctypes.data))
        return out

    def encode(self, pcm, seek=0, cross=True, audio_ctx=None):
        """audio_ctx=K (skw_encode_actx; 0 = n_audio_ctx): encoder output [K][n_state] and cross K / V [n_text_layer][K][n_state]; decode_logits then follows that K"""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        hp = self.model.hp
        K = hp.n_audio_ctx if audio_ctx is None or not 0 < audio_ctx <= hp.n_audio_ctx else audio_ctx
        enc = np.empty((K, hp.n_audio_state), dtype=np.float32)
        ck = cv = None
        if cross:
            ck = np.empty((hp.n_text_layer, K, hp.n_text_state), dtype=np.float32)
            cv = np.empty_like(ck)
        if audio_ctx is None:
            self._check(lib().skw_encode(self.h, pcm.ctypes.data, pcm.size, seek, enc.ctypes.data,
                                         ck.ctypes.data if cross else None, cv.ctypes.data if cross else None))
        else:
            self._check(lib().skw_encode_actx(self.h, pcm.ctypes.data, pcm.size, seek, int(audio_ctx), enc.ctypes.data,
                                              ck.ctypes.data if cross else None, cv.ctypes.data if cross else None))
        return enc, ck, cv

    def decode_logits(self, tokens):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.model.hp.n_vocab, dtype=np.float32)
        self._check(lib().skw_decode_logits(self.h, t.ctypes.data, t.size, out.ctypes.data))
        return out

    def sample_rows(self, hists, logits, params=None, form=0, want_filtered=False, rules=None, temperature=None, rng_state=None, trace=True, extras=False,
                    grammars=None, active=None):
        """K11 on its own (skw_debug_sample_rows): one sampler launch decides the next token of len(hists) decoders whose sampled tokens so far are
        hists[r], on caller-supplied logits [rows][n_vocab].  form 0: the decode step's sampler; 1: the streaming kernel (leaves the filtered row
        in memory: want_filtered).  -> (tokens structured array, trace records, filtered logits or None)
        params=[FullParams per row]: the per-row form of the sampler (skw_debug_sample_rows_mixed) — every row under its own rules and its own static mask.
        rules=[DecodeRules or None per row]: skw_debug_sample_rows_rules — k_dec_constrain on the rows' logits, then the per-row form of the sampler.
        grammars=[Grammar or None per row] (with rules= or without; active=[0 / 1 per row]: 0 marks a row as finished before the launch): skw_debug_sample_rows_grammar —
        k_dec_constrain (when rules are given), k_dec_grammar, then the per-row form of the sampler, as in the decode step.
        temperature=[per row], rng_state=uint32 [rows][625] (updated in place: row r draws from generator r), trace=False (the launch without trace buffers) or extras=True:
        skw_debug_sample_rows_ex — a fourth element is returned, a dict of kernel (the instantiation the launcher picked), probs [rows][n_vocab] (rows at a temperature > 0;
        NaN elsewhere), no_speech_prob, n_tokens, cur_token, active [rows] (the rows' state after the launch)."""
        per_row = isinstance(params, (list, tuple))
        R = len(hists)
        rq = SampleRowsRequest(n_rows=R, form=int(form), trace=1 if trace else 0, kernel_id=-1)
        if rules is not None:
            rules_keep, rq.rules = rules_array(rules, R, self.model.hp.n_vocab, "row")
        if per_row and len(params) != R:
            raise ValueError("sample_rows: %d parameter blocks for %d rows" % (len(params), R))
        stride = max(1, max(len(h) for h in hists))
        hb = np.zeros((R, stride), dtype=np.int32)
        for r, h in enumerate(hists):
            hb[r, :len(h)] = h
        nh = np.array([len(h) for h in hists], dtype=np.int32)
        lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(R, self.model.hp.n_vocab)
        filt = np.empty_like(lg) if want_filtered else None
        toks = np.zeros(R, dtype=_TOKEN_DT)
        tr = np.zeros(R, dtype=TRACE_DT)
        rq.hist, rq.hist_stride, rq.n_hist, rq.logits = hb.ctypes.data, stride, nh.ctypes.data, lg.ctypes.data
        rq.filtered_out, rq.tok_out, rq.trace_out = filt.ctypes.data if want_filtered else None, toks.ctypes.data, tr.ctypes.data
        ex = temperature is not None or rng_state is not None or not trace or extras      # (what skw_debug_sample_rows_ex added: a fourth element comes back)
        if grammars is not None:
            if ex:
                raise ValueError("sample_rows: grammars= goes with the plain call only")
            rq.grammar = grammars_array(grammars, R, "row")
            act = None if active is None else np.ascontiguousarray(active, dtype=np.int32).reshape(R)
            rq.active = None if act is None else act.ctypes.data
        elif ex:
            if rules is not None:
                raise ValueError("sample_rows: rules= goes with the plain call only")
            t = np.zeros(R, np.float32) if temperature is None else np.ascontiguousarray(temperature, dtype=np.float32).reshape(R)
            if rng_state is not None:
                assert rng_state.dtype == np.uint32 and rng_state.shape == (R, 625) and rng_state.flags["C_CONTIGUOUS"]
                rq.rng_state = rng_state.ctypes.data
            out = dict(probs=np.full((R, self.model.hp.n_vocab), np.nan, np.float32), no_speech_prob=np.zeros(R, np.float32), n_tokens=np.zeros(R, np.int32),
                       cur_token=np.zeros(R, np.int32), active=np.zeros(R, np.int32))
            rq.temperature, rq.probs_out, rq.no_speech_prob = t.ctypes.data, out["probs"].ctypes.data, out["no_speech_prob"].ctypes.data
            rq.n_tokens, rq.cur_token, rq.active_out = out["n_tokens"].ctypes.data, out["cur_token"].ctypes.data, out["active"].ctypes.data
        # rules and grammars run the per-row form of the sampler whatever the parameters; otherwise a list of parameters does
        rq.params_per_row = 1 if per_row or grammars is not None or rules is not None else 0
        rq.params = _params_for(params or self.default_params(), rq.params_per_row, R)
        self._check(lib().skw_debug_sample_rows_request(self.h, C.byref(rq)))
        if grammars is None and ex:
            out["kernel"] = sampler_kernel_name(rq.kernel_id)
            return toks, tr, filt, out
        return toks, tr, filt

    ATTN16_FORMS = {"encoder": 0, "prefill": 1, "cross16": 2, "cross2p": 3, "self": 4}

    def attn16(self, form, H, n_ctx, Q, K, V, fill_from, k_pad=0x7E00, v_pad=0x7E00, frag=0, ofrag=0, slot_k=None, out_rows=0, row0=None, nq=None, slot=None,
               active=None, seq=None, count=None, sentinel=0x5A5A):
        """One f16_mfma attention launcher on caller-supplied operands (skw_debug_attn16, skw_hooks.hip).  Q [rows][H*64], K / V [slots][n_ctx][H*64] as float16 (or their
        uint16 bit patterns) in natural order; every K / V position of slot s from fill_from[s] up holds the bit pattern k_pad / v_pad when the kernel runs; the output buffer
        starts as `sentinel` in every half.  form: "encoder" (slot_k, out_rows), "prefill" (row0, nq, slot per sequence; frag, ofrag, slot_k), "cross16" / "cross2p" (the one-pass
        and the two-phase decode kernels; active, seq, count = n_keys per row; ofrag) or "self" (count = pos per row; active, seq; ofrag).  -> f32 [rows][H*64], natural order."""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        ints = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        Q = bits(Q); K = bits(K); V = bits(V)
        n_slots = K.shape[0]
        assert K.shape == (n_slots, n_ctx, d) and V.shape == K.shape and Q.shape[-1] == d
        f = self.ATTN16_FORMS[form]
        rows = 1 if f == 0 else Q.shape[0]
        if f == 0:
            assert Q.shape == K.shape
            orows = n_slots * (out_rows if (slot_k is not None and out_rows) else n_ctx)
        else:
            orows = rows
        fill_from, slot_k, row0, nq, slot, active, seq, count = (ints(a) for a in (fill_from, slot_k, row0, nq, slot, active, seq, count))
        assert fill_from.size == n_slots and (slot_k is None or slot_k.size == n_slots)
        for a in (active, seq, count):
            assert a is None or a.size == rows
        n_seq = 0 if row0 is None else row0.size
        assert n_seq == 0 or (nq.size == n_seq and slot.size == n_seq)
        out = np.empty((orows, d), dtype=np.float32)
        self._check(lib().skw_debug_attn16(self.h, f, H, n_ctx, n_slots, rows, (1 if frag else 0) | (2 if ofrag else 0), int(out_rows), Q.ctypes.data, K.ctypes.data, V.ctypes.data,
                                           fill_from.ctypes.data, int(k_pad), int(v_pad), ptr(slot_k), n_seq, ptr(row0), ptr(nq), ptr(slot), ptr(active), ptr(seq), ptr(count),
                                           int(sentinel), out.ctypes.data))
        return out

    def kv8_quantize(self, H, n_ctx, K, V, fill_from, k_pad=0x7E00, v_pad=0x7E00, slot_k=None):
        """k_kv8_quantize on caller-supplied K / V [slots][n_ctx][H*64] (float16 or uint16 bit patterns, natural order; positions from fill_from[s] up hold the pad patterns);
        slot_k: the slots' key counts (None: n_ctx).  -> the q8 image as uint8 [slots][slot bytes], 0xEE where the kernel wrote nothing (byte order: the exported skw_layout_kv8_* functions)."""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        K = bits(K); V = bits(V); n_slots = K.shape[0]
        assert K.shape == (n_slots, n_ctx, d) and V.shape == K.shape
        fill_from = np.ascontiguousarray(fill_from, dtype=np.int32); assert fill_from.size == n_slots
        sk = None if slot_k is None else np.ascontiguousarray(slot_k, dtype=np.int32)
        img = np.empty((n_slots, kv8_slot_bytes(H, (n_ctx + 31) & ~31)), np.uint8)
        self._check(lib().skw_debug_kv8_quantize(self.h, H, n_ctx, n_slots, K.ctypes.data, V.ctypes.data, fill_from.ctypes.data, int(k_pad), int(v_pad),
                                                 None if sk is None else sk.ctypes.data, img.ctypes.data))
        return img

    def attn_kv8(self, H, n_ctx, Q, K, V, fill_from, k_pad=0x7E00, v_pad=0x7E00, slot_k=None, active=None, seq=None, count=None, ofrag=0, f32_out=0, raw=0, sentinel=0x5A5A):
        """The quantise kernel, then the q8 cross attention through its launcher (skw_debug_attn_kv8), on operands as attn16's "cross16" form takes them; slot_k: the quantiser's
        key count per slot (None: n_ctx).  -> f32 [rows][H*64] in natural order (f32_out: unrounded), or with raw the kernel's f32 scores [rows][H][n_ctx], NaN where unwritten."""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        ints = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        Q = bits(Q); K = bits(K); V = bits(V); n_slots, rows = K.shape[0], Q.shape[0]
        assert K.shape == (n_slots, n_ctx, d) and V.shape == K.shape and Q.shape == (rows, d)
        fill_from, slot_k, active, seq, count = (ints(a) for a in (fill_from, slot_k, active, seq, count))
        assert fill_from.size == n_slots and (slot_k is None or slot_k.size == n_slots)
        for a in (active, seq, count):
            assert a is None or a.size == rows
        out = np.empty((rows, H, n_ctx) if raw else (rows, d), dtype=np.float32)
        self._check(lib().skw_debug_attn_kv8(self.h, H, n_ctx, n_slots, rows, (2 if ofrag else 0) | (4 if f32_out else 0) | (8 if raw else 0), Q.ctypes.data, K.ctypes.data, V.ctypes.data,
                                             fill_from.ctypes.data, int(k_pad), int(v_pad), ptr(slot_k), ptr(active), ptr(seq), ptr(count), int(sentinel), out.ctypes.data))
        return out

    def xattn_exact(self, mq, H, n_ctx, Q, K, V, fill_from, row0, nq, slot, slot_k=None, f32_out=False, k_pad=0x7E00, v_pad=0x7E00, sentinel=0x5A5A):
        """The exact precision's prompt-pass cross attention on caller-supplied operands (skw_debug_xattn_exact).  Q [rows][H*64], K / V [slots][n_ctx][H*64] as float16 (or uint16
        bit patterns), natural order; sequences (row0, nq, slot); slot_k None or a key count per slot.  mq=0: the single-query kernel on every owned row, mq=1: the
        16-queries-per-workgroup kernel.  -> the raw output buffer as uint16 [rows][H*64 * (2 if f32_out else 1)] (f16 rows are in kperm order), `sentinel` where nothing was written."""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        ints = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        Q = bits(Q); K = bits(K); V = bits(V)
        n_slots, rows = K.shape[0], Q.shape[0]
        assert K.shape == (n_slots, n_ctx, d) and V.shape == K.shape and Q.shape == (rows, d)
        fill_from, row0, nq, slot, slot_k = (ints(a) for a in (fill_from, row0, nq, slot, slot_k))
        assert fill_from.size == n_slots and (slot_k is None or slot_k.size == n_slots) and row0.size == nq.size == slot.size
        out = np.empty((rows, d * (2 if f32_out else 1)), dtype=np.uint16)
        self._check(lib().skw_debug_xattn_exact(self.h, int(mq), H, n_ctx, n_slots, rows, 1 if f32_out else 0, Q.ctypes.data, K.ctypes.data, V.ctypes.data, fill_from.ctypes.data,
                                                int(k_pad), int(v_pad), None if slot_k is None else slot_k.ctypes.data, row0.size, row0.ctypes.data, nq.ctypes.data, slot.ctypes.data,
                                                int(sentinel), out.ctypes.data))
        return out

    ATTN_EXACT_FORMS = {"encoder": 0, "self": 1}
    ATTN_ENC_KERNELS = {0: "k_attn_encoder", 1: "k_attn_encoder_v3"}

    def attn_exact(self, form, H, n_ctx, Q, K, V, fill_from, f32_out=False, raw=False, k_pad=0x7E00, v_pad=0x7E00, slot_k=None, out_rows=0, active=None, seq=None, pos=None,
                   sentinel=0x5A5A):
        """The exact precision's encoder attention or decoder self attention on caller-supplied operands (skw_debug_attn_exact, skw_hooks.hip), through the public launcher.
        Operands, fill_from, the pads and the sentinel as attn16.  form "encoder": Q [slots][n_ctx][H*64] (slot_k, out_rows); "self": Q [rows][H*64], K / V the caches
        [slots][n_text_ctx][H*64], pos per row (active, seq).  -> (out, kernel): out uint16 [rows][H*64] (f16 bits; kperm order when raw, else natural) or, f32_out, uint32
        [rows][H*64] (the f32 rows' bits); kernel: the encoder kernel the launcher chose (ATTN_ENC_KERNELS), None for "self"."""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        ints = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        Q = bits(Q); K = bits(K); V = bits(V)
        n_slots = K.shape[0]
        assert K.shape == (n_slots, n_ctx, d) and V.shape == K.shape and Q.shape[-1] == d
        f = self.ATTN_EXACT_FORMS[form]
        fill_from, slot_k, active, seq, pos = (ints(a) for a in (fill_from, slot_k, active, seq, pos))
        assert fill_from.size == n_slots and (slot_k is None or slot_k.size == n_slots)
        if f == 0:
            assert Q.shape == K.shape and active is None and seq is None and pos is None
            rows = 1; orows = n_slots * (int(out_rows) if out_rows else n_ctx)
        else:
            rows = orows = Q.shape[0]
            assert Q.shape == (rows, d) and pos is not None and slot_k is None and not out_rows
            for a in (active, seq, pos):
                assert a is None or a.size == rows
        out = np.empty((orows, d), dtype=np.uint32 if f32_out else np.uint16)
        kid = C.c_int(-1)
        self._check(lib().skw_debug_attn_exact(self.h, f, H, n_ctx, n_slots, rows, 1 if f32_out else 0, 1 if raw else 0, int(out_rows), Q.ctypes.data, K.ctypes.data, V.ctypes.data,
                                               fill_from.ctypes.data, int(k_pad), int(v_pad), ptr(slot_k), ptr(active), ptr(seq), ptr(pos), int(sentinel), out.ctypes.data, C.byref(kid)))
        return out, (self.ATTN_ENC_KERNELS[kid.value] if f == 0 else None)

    def gemm_q8(self, qtype, blocks, N, K, A, segmented, epi, C_buf, ldc=0, bias=None, res_alias=False, scale=1.0, has_scale=0, n_ctx=0, H=0, Tpad=0, pos=None,
                C2_buf=None, C3_buf=None, ldc2=0):
        """One product of ggml's arithmetic for quantised files on caller-supplied operands (skw_debug_gemm_q8, skw_hooks.hip): `blocks` (bytes: N rows of K / 32 blocks of ggml
        type qtype) go through the model loader's repack, A (f32 [M][lda >= K]: the first K columns are the rows) through skw_q8_quantize, then skw_gemm_q8 — the public
        launchers, dispatch included.  C_buf (and C2_buf / C3_buf for EPI_DEC_QKV) are flat arrays holding what the output buffers hold BEFORE the launch: the caller's sentinel
        with its margin (res_alias: the residual in C's M x N region); they are not modified.  -> (kernel id, C, C2, C3): the buffers after the launch."""
        Ah = np.ascontiguousarray(A, dtype=np.float32); M, lda = Ah.shape
        blocks = np.frombuffer(blocks, np.uint8)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        bias = f32(bias); pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        Cb = np.ascontiguousarray(C_buf).copy(); C2 = None if C2_buf is None else np.ascontiguousarray(C2_buf).copy(); C3 = None if C3_buf is None else np.ascontiguousarray(C3_buf).copy()
        assert bias is None or bias.size == N
        assert (C2 is None) == (C3 is None) and (C2 is None or C2.nbytes == C3.nbytes)
        kid = C.c_int(-1)
        self._check(lib().skw_debug_gemm_q8(self.h, int(qtype), blocks.ctypes.data, N, K, Ah.ctypes.data, lda, M, 1 if segmented else 0, int(epi), int(n_ctx), int(H), int(Tpad), ptr(bias),
                                            1 if res_alias else 0, float(scale), int(has_scale), ptr(pos), Cb.ctypes.data, Cb.nbytes, int(ldc), ptr(C2), ptr(C3),
                                            0 if C2 is None else C2.nbytes, int(ldc2), C.byref(kid)))
        return kid.value, Cb, C2, C3

    def gemm16_epi(self, launcher, N, K, epi, W, C_buf, A=None, lda=0, a_rows_per_batch=0, a_batch_stride=0, a_frag=False, M=None, ln=None, use_wf=False, bias=None, res=None,
                   res_alias=False, scale=1.0, has_scale=0, pe=None, n_ctx=0, H=0, Tpad=0, frag=False, c_frag=False, pos=None, force_small=False, ldc=0, C2_buf=None, C3_buf=None, ldc2=0):
        """One f16_mfma product on caller-supplied operands through the public launchers (skw_debug_gemm16_epi, skw_hooks.hip).  launcher: 0 skw_gemm16 as k_gemm16w, 1 as k_gemm16,
        2 skw_gemm16_small, 3 skw_gemm16_small_lnA.  A: flat uint16 array of f16 bits (rows at lda, the batch-strided rows of conv2, or the fragment-order image) or, launcher 3,
        ln = (x f32 [M][K], gain [K], bias [K]); W uint16 [N][K].  C_buf (C2_buf / C3_buf) hold what the output buffers hold BEFORE the launch — the caller's sentinel with its
        margins, the residual when res_alias — and are not modified.  -> (rc, kernel id, C, C2, C3): rc 0, or -2 when the launcher refuses the arguments; -1 raises."""
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        W = np.ascontiguousarray(W, dtype=np.uint16); assert W.shape == (N, K)
        A = None if A is None else np.ascontiguousarray(A, dtype=np.uint16).reshape(-1)
        lx, lw, lb = (f32(v) for v in ln) if ln is not None else (None, None, None)
        if M is None:
            M = lx.shape[0]
        bias, res, pe = f32(bias), f32(res), f32(pe)
        pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
        assert (bias is None or bias.size == N) and (pos is None or pos.size == M) and (lx is None or (lx.shape == (M, K) and lw.size == K and lb.size == K))
        assert res is None or res.ndim == 2 and res.shape[0] == M
        assert pe is None or pe.shape == (n_ctx, N)
        Cb = np.ascontiguousarray(C_buf).copy(); C2 = None if C2_buf is None else np.ascontiguousarray(C2_buf).copy(); C3 = None if C3_buf is None else np.ascontiguousarray(C3_buf).copy()
        assert (C2 is None) == (C3 is None) and (C2 is None or C2.nbytes == C3.nbytes)
        a = Gemm16EpiArgs(launcher=int(launcher), M=int(M), N=int(N), K=int(K), epi=int(epi), A=ptr(A), a_halves=0 if A is None else A.size, lda=int(lda),
                          a_rows_per_batch=int(a_rows_per_batch), a_batch_stride=int(a_batch_stride), a_frag=1 if a_frag else 0, ln_x=ptr(lx), ln_w=ptr(lw), ln_b=ptr(lb),
                          W=W.ctypes.data, use_wf=1 if use_wf else 0, bias=ptr(bias), res=ptr(res), ldres=0 if res is None else res.shape[1], res_alias=1 if res_alias else 0,
                          scale=float(scale), has_scale=int(has_scale), pe=ptr(pe), n_ctx=int(n_ctx), H=int(H), Tpad=int(Tpad), frag=1 if frag else 0, c_frag=1 if c_frag else 0,
                          pos=ptr(pos), force_small=1 if force_small else 0, C=Cb.ctypes.data, c_bytes=Cb.nbytes, ldc=int(ldc), C2=ptr(C2), C3=ptr(C3),
                          c2_bytes=0 if C2 is None else C2.nbytes, ldc2=int(ldc2), kernel_id=-1)
        rc = lib().skw_debug_gemm16_epi(self.h, C.byref(a))
        if rc not in (0, -2):
            self._check(rc)
        return rc, a.kernel_id, Cb, C2, C3

    def q8_quantize(self, x, K):
        """k_q8_quantize on f32 rows x [M][ldx >= K] (skw_debug_q8_quantize) -> q int8 [M][K], d and s f32 [K/32][M]"""
        x = np.ascontiguousarray(x, dtype=np.float32); M, ldx = x.shape
        q = np.empty((M, K), np.int8); dT = np.empty((K // 32, M), np.float32); sT = np.empty((K // 32, M), np.float32)
        self._check(lib().skw_debug_q8_quantize(self.h, x.ctypes.data, ldx, M, K, q.ctypes.data, dT.ctypes.data, sT.ctypes.data))
        return q, dT, sT

    def self_attn_q8(self, H, n_text_ctx, Q, K, V, pos, active=None, seq=None, sentinel=0x5A):
        """The decoder's exact self attention twice on the same operands (skw_debug_self_attn_q8): with f32 output and leaving its rows as q8 blocks.  Q [rows][H*64], K / V
        [rows][n_text_ctx][H*64] float16; pos / active / seq per row.  Every byte of the four outputs starts as `sentinel`.
        -> (out f32 [rows][H*64], q int8 [rows][H*64], d, s f32 [2H][rows])"""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        ints = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        Q = bits(Q); K = bits(K); V = bits(V); rows = Q.shape[0]
        assert Q.shape == (rows, d) and K.shape == (rows, n_text_ctx, d) and V.shape == K.shape
        pos, active, seq = ints(pos), ints(active), ints(seq)
        for a in (pos, active, seq):
            assert a is None or a.size == rows
        out = np.full((rows, d), sentinel, np.uint8).repeat(4, axis=1).view(np.float32); q = np.full((rows, d), sentinel, np.uint8).view(np.int8)
        dT = np.full((2 * H, rows * 4), sentinel, np.uint8).view(np.float32); sT = dT.copy()
        self._check(lib().skw_debug_self_attn_q8(self.h, H, n_text_ctx, rows, Q.ctypes.data, K.ctypes.data, V.ctypes.data, pos.ctypes.data, ptr(active), ptr(seq),
                                                 out.ctypes.data, q.ctypes.data, dT.ctypes.data, sT.ctypes.data))
        return out, q, dT, sT

    # ---- word timestamps: the three kernels of skw_kernels_align.hip on caller-supplied arrays (include/skw_align.h is what they evaluate)
    def align_qk(self, H, n_ctx, Q, K, head_mask, qrow0, n, slot, n_keys, frag=False, k_pad=0x7E00, sentinel=np.float32(-7.0)):
        """k_align_qk (skw_debug_align_qk).  Q [rows][H*64], K [slots][n_ctx][H*64] float16, natural order; head_mask: the layer's alignment heads (bit h); sequence i: rows
        qrow0[i] .. + n[i] of Q, cross K of slot[i], n_keys[i] keys (0: n_ctx).  -> P f32 [heads][sum n][n_ctx], `sentinel` where nothing was written."""
        d = H * 64
        bits = lambda a: np.ascontiguousarray(a.view(np.uint16) if a.dtype == np.float16 else a, dtype=np.uint16)
        Q = bits(Q); K = bits(K)
        qrow0, n, slot, n_keys = (np.ascontiguousarray(a, dtype=np.int32) for a in (qrow0, n, slot, n_keys))
        assert K.shape[1:] == (n_ctx, d) and Q.shape[1] == d and qrow0.size == n.size == slot.size == n_keys.size
        P = np.full((bin(head_mask).count("1"), int(n.sum()), n_ctx), sentinel, np.float32)
        self._check(lib().skw_debug_align_qk(self.h, H, n_ctx, K.shape[0], Q.shape[0], 1 if frag else 0, Q.ctypes.data, K.ctypes.data, int(k_pad), int(head_mask), n.size,
                                             qrow0.ctypes.data, n.ctypes.data, slot.ctypes.data, n_keys.ctypes.data, P.ctypes.data))
        return P

    def align_reduce(self, P_layers, n, kw, width=7, sentinel=np.float32(-7.0)):
        """k_align_reduce (skw_debug_align_reduce), one launch per layer.  P_layers: per layer f32 [heads][sum n][keys]; sequences of n[i] rows cropped to kw[i] keys.
        -> the sequences' N x Kw matrices back to back, flat f32."""
        P_layers = [np.ascontiguousarray(P, dtype=np.float32) for P in P_layers]
        n, kw = np.ascontiguousarray(n, dtype=np.int32), np.ascontiguousarray(kw, dtype=np.int32)
        rows, stride = P_layers[0].shape[1:]
        assert all(P.shape[1:] == (rows, stride) for P in P_layers) and rows == int(n.sum()) and n.size == kw.size
        nh = np.array([P.shape[0] for P in P_layers], np.int32)
        Pall = np.concatenate([P.reshape(-1) for P in P_layers])
        x = np.full(int((n.astype(np.int64) * kw).sum()), sentinel, np.float32)
        self._check(lib().skw_debug_align_reduce(self.h, len(P_layers), nh.ctypes.data, Pall.ctypes.data, stride, int(width), n.size, n.ctypes.data, kw.ctypes.data, x.ctypes.data))
        return x

    def align_dtw(self, xs, seek_cs=None, sentinel=-77):
        """k_align_dtw (skw_debug_align_dtw): one launch over the f32 matrices xs (each [N][Kw]).  -> (jump, t0, t1), int32 [sum N]"""
        xs = [np.ascontiguousarray(x, dtype=np.float32) for x in xs]
        n = np.array([x.shape[0] for x in xs], np.int32); kw = np.array([x.shape[1] for x in xs], np.int32)
        seek = np.zeros(len(xs), np.int32) if seek_cs is None else np.ascontiguousarray(seek_cs, dtype=np.int32)
        flat = np.concatenate([x.reshape(-1) for x in xs])
        jump, t0, t1 = (np.full(int(n.sum()), sentinel, np.int32) for _ in range(3))
        self._check(lib().skw_debug_align_dtw(self.h, len(xs), n.ctypes.data, kw.ctypes.data, seek.ctypes.data, flat.ctypes.data, jump.ctypes.data, t0.ctypes.data, t1.ctypes.data))
        return jump, t0, t1

    def align_params_check(self, enabled, median_width, head_mask, clip=0):
        """a clip's alignment record against this context's model (skw_align_params_check): None when good, else the message"""
        p = AlignParams(enabled=int(enabled), median_width=int(median_width))
        for l, w in enumerate(head_mask):
            p.head_mask[l] = int(w)
        return None if lib().skw_align_params_check(self.h, C.byref(p), int(clip)) == 0 else lib().skw_ctx_last_error(self.h).decode()

    def math(self, kind, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        self._check(lib().skw_debug_math(self.h, kind, x.ctypes.data, out.ctypes.data, x.size))
        return out

    def close(self):
        if self.h:
            lib().skw_ctx_free(self.h)
            self.h = None


def switches():
    """The engine's switchboard (skw_kernels.h SkwSw / skw_engine.hip g_sw_defs): {name: (default, current, what)}.  No GPU needed."""
    L = lib()
    return {L.skw_debug_switch_name(i).decode(): (L.skw_debug_switch_default(i), L.skw_debug_switch_get(L.skw_debug_switch_name(i)), L.skw_debug_switch_what(i).decode())
            for i in range(L.skw_debug_switch_count())}


class switch:
    """`with engine.switch("GEMM16W", 0): ...` — flips one row of the switchboard in-process (what the environment variable SKW_GEMM16W=0 selects at start-up) and restores it."""
    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        self.old = lib().skw_debug_switch_get(self.name)
        if lib().skw_debug_switch_set(self.name, self.value) != 0:
            raise KeyError("no such switch: %s" % self.name.decode())
        return self

    def __exit__(self, *exc):
        lib().skw_debug_switch_set(self.name, self.old)
        return False


def debug_enable(on=True):
    lib().skw_debug_enable(1 if on else 0)


def debug_get(name):
    n = lib().skw_debug_get(name.encode(), None, 0)
    if n < 0:
        return None
    out = np.empty(n, dtype=np.float32)
    lib().skw_debug_get(name.encode(), out.ctypes.data, n)
    return out


class Dsp:
    """Model-free device context for the resampler kernels (include/skw_engine.h, R1-R3)."""

    def __init__(self, device=0):
        err = C.create_string_buffer(512)
        self.h = lib().skw_dsp_create(device, err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())

    def linear_stream(self, ratio, chunk_frames, channels):
        st = ResamplerState()
        lib().skw_resampler_init(C.byref(st), ratio, chunk_frames, channels)
        return st

    def resample_linear(self, st, interleaved, n_chunks):
        x = np.ascontiguousarray(interleaved, dtype=np.float32)
        cap = int(n_chunks * st.chunk_frames * st.ratio) + 64
        out = np.empty(cap * st.channels, dtype=np.float32)
        n = C.c_int()
        if lib().skw_resample_linear(self.h, C.byref(st), x.ctypes.data, n_chunks, out.ctypes.data, cap, C.byref(n)) != 0:
            raise RuntimeError(lib().skw_dsp_last_error(self.h).decode())
        return out[:n.value * st.channels].copy()

    def last_scan_fallback(self):
        """1 when the last resample_linear needed the single-lane index walk (the parallel proposal failed its on-device check)."""
        return lib().skw_dsp_last_scan_fallback(self.h)

    def polyphase_stream(self, channels, in_rate, out_rate):
        return PolyphaseStream(self, channels, in_rate, out_rate)

    def resample_polyphase(self, interleaved, channels, in_rate, out_rate):
        x = np.ascontiguousarray(interleaved, dtype=np.float32)
        n_in = x.size // channels
        cap = n_in * out_rate // in_rate + 64
        out = np.empty(cap * channels, dtype=np.float32)
        n = C.c_long()
        if lib().skw_resample_polyphase(self.h, x.ctypes.data, n_in, channels, in_rate, out_rate, out.ctypes.data, cap, C.byref(n)) != 0:
            raise RuntimeError(lib().skw_dsp_last_error(self.h).decode())
        return out[:n.value * channels].copy()

    def close(self):
        if self.h:
            lib().skw_dsp_free(self.h)
            self.h = None


class PolyphaseStream:
    """Streaming polyphase resampler with its input tail resident on the device (skw_polyphase_stream_*)."""

    def __init__(self, dsp, channels, in_rate, out_rate):
        self.dsp, self.ch, self.in_rate, self.out_rate = dsp, channels, in_rate, out_rate
        self.h = lib().skw_polyphase_stream_create(dsp.h, channels, in_rate, out_rate)
        if not self.h:
            raise RuntimeError(lib().skw_dsp_last_error(dsp.h).decode())

    def push(self, interleaved, final=False):
        x = np.ascontiguousarray(interleaved if interleaved is not None else np.zeros(0, np.float32), dtype=np.float32)
        n_in = x.size // self.ch
        cap = (n_in + 4096) * self.out_rate // self.in_rate + 4096
        out = np.empty(cap * self.ch, dtype=np.float32)
        n = C.c_long()
        if lib().skw_polyphase_stream_push(self.h, x.ctypes.data if n_in else None, n_in, 1 if final else 0, out.ctypes.data, cap, C.byref(n)) != 0:
            raise RuntimeError(lib().skw_dsp_last_error(self.dsp.h).decode())
        return out[:n.value * self.ch].copy()

    def close(self):
        if self.h:
            lib().skw_polyphase_stream_free(self.h); self.h = None


def kv8_slot_bytes(H, Tpad):
    """bytes of one window slot of the q8 cross K / V image (include/skw_kv8.h)"""
    return int(lib().skw_layout_kv8_slot_bytes(H, Tpad))
