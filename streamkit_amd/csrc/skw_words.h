// skw_words.h — the word rule of `timestamp_granularity: "word"`: cuts a window's text tokens, with the token times of include/skw_align.h, into words.  Host code only.
//
// whisper.cpp's split_on_word rule, and nothing more:
//   - a word starts at the window's first text token (and at a text token that follows a timestamp token: `first`), and at any token whose text begins with a space while the
//     bytes accumulated in the current word are valid UTF-8;
//   - a token that is not valid UTF-8 on its own (a piece of a multi-byte character) stays with the current word, whatever it begins with;
//   - start = t0 of the word's first token; end = t1 of its last token — which is t0 of the next word's first token in the window, else the window's eot time; end >= start;
//   - a word whose text trims (ASCII white space) to nothing is skipped — the word after it still begins where its own first token begins.
// No punctuation merging and no script-specific splitting: text without spaces (CJK) comes out as one word per stretch between two `first` tokens.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "skw_segmenter.h"      // skw::utf8_valid: the node's one UTF-8 validator

// one text token: its bytes, its times (include/skw_align.h step 7); first: it opens a window or follows a timestamp token
struct SkwWordTok { const char* text; int len; int64_t t0, t1; bool first; };
struct SkwWord { int tok_begin, tok_end; int64_t start, end; std::string text; };             // tokens [tok_begin, tok_end) of the window; text trimmed

inline std::vector<SkwWord> skw_words_cut(const SkwWordTok* toks, int n) {
    std::vector<SkwWord> all;
    for (int i = 0; i < n; ++i) {
        const bool own_valid = skw::utf8_valid(std::string(toks[i].text, (size_t)toks[i].len));
        const bool starts = all.empty() || toks[i].first || (toks[i].len > 0 && toks[i].text[0] == ' ' && own_valid && skw::utf8_valid(all.back().text));
        if (starts) all.push_back(SkwWord{i, i, toks[i].t0, toks[i].t1, std::string()});
        all.back().text.append(toks[i].text, (size_t)toks[i].len);
        all.back().tok_end = i + 1; all.back().end = toks[i].t1;
    }
    std::vector<SkwWord> out;
    for (SkwWord& w : all) {
        const char* ws = " \t\n\r\f\v";
        const size_t a = w.text.find_first_not_of(ws);
        if (a == std::string::npos) continue;
        w.text = w.text.substr(a, w.text.find_last_not_of(ws) - a + 1);
        if (w.end < w.start) w.end = w.start;
        out.push_back(w);
    }
    return out;
}
