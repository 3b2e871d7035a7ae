// skw_tokenizer.h — whisper.cpp's tokenize(): text -> token ids.  Header-only host code (no device, no engine types): the engine wraps it as skw_model_tokenize,
// tests/cpp/tokenize_main.cpp compiles it on its own.
//
// RECALLED from whisper.cpp (whisper.cpp: `static std::vector<whisper_vocab::id> tokenize(const whisper_vocab&, const std::string&)`, what whisper_tokenize calls); stated here,
// not copied:
//   split   the text is cut into words by repeated std::regex_search over the remaining suffix with
//             's|'t|'re|'ve|'m|'ll|'d| ?[[:alpha:]]+| ?[[:digit:]]+| ?[^\s[:alpha:][:digit:]]+|\s+(?!\S)|\s+
//           (bytes the pattern cannot match at the front of the suffix are passed over by the search; an empty match ends nothing because none is possible);
//   match   inside a word, at position i, the LONGEST vocabulary entry that starts there wins (j = n down to i + 1); if no entry starts at i, that one byte is skipped;
//   vocab   the map is token_to_id; only ids below <|endoftext|> are in it here (the specials are never produced from text), and where two ids carry the same string the
//           higher id wins (the map's last assignment, as the loader fills it in id order).
// Nothing is put in front of the text (openai's reference decodes behind " " + prompt.strip(); whisper.cpp does not, and neither does this).
#pragma once
#include <cstdint>
#include <regex>
#include <string>
#include <unordered_map>
#include <vector>

struct SkwTokenizer {
    std::unordered_map<std::string, int32_t> token_to_id;
    size_t max_len = 0;      // longest entry in bytes: no candidate longer than this is looked up

    // tok[i] = the string of id i; ids >= n_text (<|endoftext|> and above) stay out
    void build(const std::vector<std::string>& tok, int n_text) {
        token_to_id.clear(); max_len = 0;
        for (int i = 0; i < n_text && i < (int)tok.size(); ++i) { token_to_id[tok[i]] = i; if (tok[i].size() > max_len) max_len = tok[i].size(); }
    }

    std::vector<int32_t> tokenize(const std::string& text) const {
        static const std::regex re(R"('s|'t|'re|'ve|'m|'ll|'d| ?[[:alpha:]]+| ?[[:digit:]]+| ?[^\s[:alpha:][:digit:]]+|\s+(?!\S)|\s+)");
        std::vector<std::string> words;
        {
            std::string::const_iterator at = text.begin(); std::smatch mt;
            while (at != text.end() && std::regex_search(at, text.end(), mt, re)) {
                if (mt.length(0) == 0) { ++at; continue; }      // (the pattern has no empty alternative; guards the loop all the same)
                words.push_back(mt.str(0)); at = mt[0].second;
            }
        }
        std::vector<int32_t> out;
        for (const std::string& w : words) {
            const size_t n = w.size(); size_t i = 0;
            while (i < n) {
                size_t j = n; bool found = false;
                if (j - i > max_len) j = i + max_len;      // longer candidates cannot be entries: the first hit is still the longest one
                for (; j > i; --j) {
                    auto it = token_to_id.find(w.substr(i, j - i));
                    if (it != token_to_id.end()) { out.push_back(it->second); i = j; found = true; break; }
                }
                if (!found) ++i;      // whisper.cpp logs "unknown token" and moves on by one byte
            }
        }
        return out;
    }

    // whisper_tokenize's return convention: the count, or -needed when cap is too small
    int tokenize_into(const char* text, int32_t* ids, int cap) const {
        const std::vector<int32_t> t = tokenize(text ? std::string(text) : std::string());
        if ((int)t.size() > cap) return -(int)t.size();
        for (size_t i = 0; i < t.size(); ++i) ids[i] = t[i];
        return (int)t.size();
    }
};
