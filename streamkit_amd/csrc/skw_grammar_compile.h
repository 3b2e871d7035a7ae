// Pattern -> skw_grammar (include/skw_grammar.h): a regular expression over BYTES, anchored at both ends (a full match), compiled to a trimmed dense DFA.
// Host code only; needs no device.  The supported subset, with Python's `re` on a bytes pattern as the meaning of every construct (tests/test_cpu_grammar.py holds it to that):
//   literals (UTF-8 as its bytes), `\` + a punctuation character (the character itself), \n \t \r \f \v
//   \d \w \s \D \W \S (ASCII), `.` (any byte but \n), [...] with ranges, escapes and a leading ^
//   ( ) groups, |, and the quantifiers ? * + {m} {m,} {m,n} (greedy: for a full match lazy ones would accept the same strings)
//   SKW_GRAMMAR_IGNORE_CASE: ASCII letters match either case
// Anything else — (?...) groups, anchors, back-references, \b, lazy / possessive quantifiers, a `{` that is no quantifier — is refused with a message, as are an empty
// pattern, unbalanced brackets and a pattern whose DFA has more than SKW_GRAMMAR_MAX_STATES states: the node feeds this from user JSON, so it never crashes and never
// recurses or allocates without a bound.
// How: recursive descent to a small syntax tree, Thompson construction (counted repetitions are copies), subset construction, then removal of the states that cannot reach an
// accepting one — their transitions become DEAD, so "not DEAD" means "a match is still possible" (include/skw_grammar.h).
#pragma once
#include <algorithm>
#include <bitset>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <vector>
#include "../../include/skw_grammar.h"

#define SKW_GRAMMAR_IGNORE_CASE 1

namespace skw_grammar_cc {
typedef std::bitset<256> ByteSet;
struct Node { enum Kind { SET, CAT, ALT, REP } kind = CAT; ByteSet set; std::vector<std::unique_ptr<Node>> kids; int lo = 0, hi = 0; };      // REP: hi < 0 = unbounded; CAT of nothing = empty
struct Fail { char msg[200]; };
static const int MAX_DEPTH = 64, MAX_COUNT = 1000, MAX_NFA = 50000;

[[noreturn]] static inline void fail(const char* fmt, ...) {
    Fail f; va_list ap; va_start(ap, fmt); vsnprintf(f.msg, sizeof f.msg, fmt, ap); va_end(ap); throw f;
}
static inline ByteSet range_set(int a, int b) { ByteSet s; for (int c = a; c <= b; ++c) s.set(c); return s; }
static inline ByteSet class_set(char c) {      // d w s (the caller complements for D W S)
    ByteSet s;
    if (c == 'd') s = range_set('0', '9');
    else if (c == 'w') { s = range_set('0', '9') | range_set('a', 'z') | range_set('A', 'Z'); s.set('_'); }
    else { for (const char* p = " \t\n\r\f\v"; *p; ++p) s.set((unsigned char)*p); }
    return s;
}
static inline ByteSet fold_case(ByteSet s) {
    for (int c = 'a'; c <= 'z'; ++c) { const int u = c - 32; if (s[c] || s[u]) { s.set(c); s.set(u); } }
    return s;
}

struct Parser {
    const unsigned char* p; size_t n, i = 0; bool icase;
    Parser(const char* pat, size_t len, bool ic) : p((const unsigned char*)pat), n(len), icase(ic) {}
    bool more() const { return i < n; }
    // an escape after the backslash: a class (is_class, with its set) or one byte
    int escape(bool* is_class, ByteSet* cls) {
        if (!more()) fail("pattern ends in a backslash");
        const unsigned char c = p[i++]; *is_class = false;
        switch (c) {
            case 'd': case 'w': case 's': *is_class = true; *cls = class_set((char)c); return 0;
            case 'D': case 'W': case 'S': *is_class = true; *cls = ~class_set((char)(c + 32)); return 0;
            case 'n': return '\n'; case 't': return '\t'; case 'r': return '\r'; case 'f': return '\f'; case 'v': return '\v';
            default: break;
        }
        if (c < 0x80 && !((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) return c;      // punctuation (and space): itself
        if (c >= 0x80) return c;
        fail("unsupported escape \\%c at byte %zu", c, i - 2);
    }
    std::unique_ptr<Node> leaf(ByteSet s) { std::unique_ptr<Node> nd(new Node); nd->kind = Node::SET; nd->set = icase ? fold_case(s) : s; return nd; }
    std::unique_ptr<Node> bracket() {      // after '['
        bool neg = false; ByteSet s; const size_t open = i - 1;
        if (more() && p[i] == '^') { neg = true; ++i; }
        bool first = true;
        for (;;) {
            if (!more()) fail("unbalanced '[' at byte %zu", open);
            unsigned char c = p[i++];
            if (c == ']' && !first) break;
            first = false;
            int lo; bool is_class = false; ByteSet cls;
            if (c == '\\') lo = escape(&is_class, &cls); else lo = c;
            if (is_class) { s |= cls; continue; }
            if (i + 1 < n && p[i] == '-' && p[i + 1] != ']') {      // a range lo-hi
                i += 1; unsigned char d = p[i++]; int hi; bool hc = false; ByteSet hcls;
                if (d == '\\') hi = escape(&hc, &hcls); else hi = d;
                if (hc) fail("a character class cannot end a range (byte %zu)", i - 1);
                if (hi < lo) fail("bad character range %c-%c at byte %zu", lo, hi, i - 1);
                s |= range_set(lo, hi);
            } else s.set(lo);
        }
        if (icase) s = fold_case(s);
        if (neg) s = ~s;
        std::unique_ptr<Node> nd(new Node); nd->kind = Node::SET; nd->set = s;
        return nd;
    }
    std::unique_ptr<Node> atom(int depth) {
        const unsigned char c = p[i++];
        if (c == '(') {
            if (more() && p[i] == '?') fail("unsupported group (?...) at byte %zu", i - 1);
            const size_t open = i - 1;
            std::unique_ptr<Node> in = alt(depth + 1);
            if (!more() || p[i] != ')') fail("unbalanced '(' at byte %zu", open);
            ++i; return in;
        }
        if (c == '[') return bracket();
        if (c == '.') { ByteSet s; s.set(); s.reset('\n'); std::unique_ptr<Node> nd(new Node); nd->kind = Node::SET; nd->set = s; return nd; }
        if (c == '\\') { bool is_class; ByteSet cls; const int b = escape(&is_class, &cls);
            if (is_class) { std::unique_ptr<Node> nd(new Node); nd->kind = Node::SET; nd->set = cls; return nd; }
            ByteSet s; s.set(b); return leaf(s); }
        if (c == '*' || c == '+' || c == '?' || c == '{') fail("nothing to repeat at byte %zu", i - 1);
        if (c == '^' || c == '$') fail("unsupported anchor '%c' at byte %zu (the match is anchored at both ends)", c, i - 1);
        if (c == ']' || c == '}') { ByteSet s; s.set(c); return leaf(s); }      // (literal when unpaired, as in re)
        ByteSet s; s.set(c); return leaf(s);
    }
    int number() {
        if (!more() || p[i] < '0' || p[i] > '9') return -1;
        long v = 0; while (more() && p[i] >= '0' && p[i] <= '9') { v = v * 10 + (p[i++] - '0'); if (v > MAX_COUNT) fail("repetition count above %d", MAX_COUNT); }
        return (int)v;
    }
    std::unique_ptr<Node> repeat(int depth) {
        std::unique_ptr<Node> a = atom(depth);
        bool quantified = false;
        while (more()) {
            const unsigned char c = p[i]; int lo, hi;
            if (c == '?') { lo = 0; hi = 1; ++i; }
            else if (c == '*') { lo = 0; hi = -1; ++i; }
            else if (c == '+') { lo = 1; hi = -1; ++i; }
            else if (c == '{') {
                const size_t at = i; ++i; lo = number();
                if (lo < 0) fail("unsupported '{' at byte %zu (only {m}, {m,} and {m,n} are quantifiers; escape a literal brace)", at);
                if (more() && p[i] == ',') { ++i; hi = number(); } else hi = lo;
                if (!more() || p[i] != '}') fail("unbalanced '{' at byte %zu", at);
                ++i;
                if (hi >= 0 && hi < lo) fail("bad repetition {%d,%d} at byte %zu", lo, hi, at);
            } else break;
            if (quantified) fail("unsupported quantifier on a quantifier at byte %zu (lazy and possessive forms are not supported)", i - 1);
            quantified = true;
            std::unique_ptr<Node> r(new Node); r->kind = Node::REP; r->lo = lo; r->hi = hi; r->kids.push_back(std::move(a)); a = std::move(r);
        }
        return a;
    }
    std::unique_ptr<Node> cat(int depth) {
        std::unique_ptr<Node> c(new Node); c->kind = Node::CAT;
        while (more() && p[i] != '|' && p[i] != ')') c->kids.push_back(repeat(depth));
        return c;
    }
    std::unique_ptr<Node> alt(int depth) {
        if (depth > MAX_DEPTH) fail("groups nested deeper than %d", MAX_DEPTH);
        std::unique_ptr<Node> a(new Node); a->kind = Node::ALT;
        a->kids.push_back(cat(depth));
        while (more() && p[i] == '|') { ++i; a->kids.push_back(cat(depth)); }
        return a;
    }
};

struct Nfa {
    struct St { std::vector<int> eps; ByteSet on; int to = -1; };
    std::vector<St> st;
    int add() { if ((int)st.size() >= MAX_NFA) fail("pattern too large (more than %d NFA states)", MAX_NFA); st.emplace_back(); return (int)st.size() - 1; }
    // builds the fragment of nd between a new entry state and a new exit state
    void build(const Node* nd, int* in, int* out) {
        *in = add(); *out = add();
        switch (nd->kind) {
        case Node::SET: st[*in].on = nd->set; st[*in].to = *out; break;
        case Node::CAT: { int cur = *in;
            for (const auto& k : nd->kids) { int a, b; build(k.get(), &a, &b); st[cur].eps.push_back(a); cur = b; }
            st[cur].eps.push_back(*out); break; }
        case Node::ALT: for (const auto& k : nd->kids) { int a, b; build(k.get(), &a, &b); st[*in].eps.push_back(a); st[b].eps.push_back(*out); } break;
        case Node::REP: { int cur = *in; const Node* k = nd->kids[0].get();
            for (int r = 0; r < nd->lo; ++r) { int a, b; build(k, &a, &b); st[cur].eps.push_back(a); cur = b; }
            if (nd->hi < 0) { int a, b; build(k, &a, &b); st[cur].eps.push_back(a); st[b].eps.push_back(cur); }      // cur -> k -> cur, any number of times
            else for (int r = nd->lo; r < nd->hi; ++r) { int a, b; build(k, &a, &b); st[cur].eps.push_back(*out); st[cur].eps.push_back(a); cur = b; }
            st[cur].eps.push_back(*out); break; }
        }
    }
    void closure(std::vector<int>& set, std::vector<char>& mark) const {      // set: grows to its epsilon closure, sorted; mark: all zero in and out
        std::vector<int> stack(set);
        for (int s : set) mark[s] = 1;
        while (!stack.empty()) { const int s = stack.back(); stack.pop_back(); for (int t : st[s].eps) if (!mark[t]) { mark[t] = 1; set.push_back(t); stack.push_back(t); } }
        for (int s : set) mark[s] = 0;
        std::sort(set.begin(), set.end());
    }
};

struct Tables { std::vector<uint16_t> next; std::vector<uint8_t> accept; };

static inline Tables compile(const char* pat, size_t len, int flags) {
    if (!pat || len == 0) fail("empty pattern");
    Parser ps(pat, len, (flags & SKW_GRAMMAR_IGNORE_CASE) != 0);
    std::unique_ptr<Node> root = ps.alt(0);
    if (ps.more()) fail("unbalanced ')' at byte %zu", ps.i);
    Nfa nfa; int in, out; nfa.build(root.get(), &in, &out);
    // subset construction; the empty set is DEAD and is never a state
    std::vector<char> mark(nfa.st.size(), 0);
    std::map<std::vector<int>, int> ids; std::vector<std::vector<int>> sets;
    std::vector<int> s0{in}; nfa.closure(s0, mark); ids[s0] = 0; sets.push_back(s0);
    std::vector<int> nx;      // [state][256], -1 = DEAD
    for (size_t d = 0; d < sets.size(); ++d) {
        nx.resize((d + 1) * 256, -1);
        std::vector<int> movers; for (int s : sets[d]) if (nfa.st[s].to >= 0) movers.push_back(s);
        for (int b = 0; b < 256; ++b) {
            std::vector<int> to; for (int s : movers) if (nfa.st[s].on[b]) to.push_back(nfa.st[s].to);
            if (to.empty()) continue;
            std::sort(to.begin(), to.end()); to.erase(std::unique(to.begin(), to.end()), to.end());
            nfa.closure(to, mark);
            auto it = ids.find(to);
            if (it == ids.end()) {
                if ((int)sets.size() >= SKW_GRAMMAR_MAX_STATES) fail("the pattern needs more than %d DFA states", SKW_GRAMMAR_MAX_STATES);
                it = ids.emplace(to, (int)sets.size()).first; sets.push_back(to);
            }
            nx[d * 256 + b] = it->second;
        }
    }
    const int nd = (int)sets.size();
    std::vector<char> acc(nd, 0); for (int d = 0; d < nd; ++d) acc[d] = std::binary_search(sets[d].begin(), sets[d].end(), out);
    // trim: live = can reach an accepting state (backwards from the accepting ones over the reversed edges)
    std::vector<std::vector<int>> rev(nd); for (int d = 0; d < nd; ++d) for (int b = 0; b < 256; ++b) if (nx[d * 256 + b] >= 0) rev[nx[d * 256 + b]].push_back(d);
    std::vector<char> live(nd, 0); std::vector<int> stack; for (int d = 0; d < nd; ++d) if (acc[d]) { live[d] = 1; stack.push_back(d); }
    while (!stack.empty()) { const int d = stack.back(); stack.pop_back(); for (int q : rev[d]) if (!live[q]) { live[q] = 1; stack.push_back(q); } }
    if (!live[0]) fail("the pattern matches nothing");
    std::vector<int> renum(nd, -1); int k = 0; for (int d = 0; d < nd; ++d) if (live[d]) renum[d] = k++;      // (0 stays 0)
    Tables t; t.next.assign((size_t)k * 256, (uint16_t)SKW_GRAMMAR_DEAD); t.accept.assign(k, 0);
    for (int d = 0; d < nd; ++d) if (live[d]) {
        t.accept[renum[d]] = acc[d] ? 1 : 0;
        for (int b = 0; b < 256; ++b) { const int q = nx[d * 256 + b]; if (q >= 0 && live[q]) t.next[(size_t)renum[d] * 256 + b] = (uint16_t)renum[q]; }
    }
    return t;
}
}      // namespace skw_grammar_cc

// 0: *out is a new grammar (release with skw_grammar_free_impl); -1: err holds the compiler's message.  Nothing is thrown across this function.
static inline int skw_grammar_compile_impl(const char* pattern, size_t len, int flags, float penalty, skw_grammar** out, char* err, size_t errlen) {
    if (out) *out = nullptr;
    if (err && errlen) err[0] = 0;
    try {
        if (!out) skw_grammar_cc::fail("no place for the grammar");
        if (!(penalty > 0.0f) || !(penalty <= 3.4028234663852886e38f)) skw_grammar_cc::fail("penalty %g must be finite and > 0", (double)penalty);
        skw_grammar_cc::Tables t = skw_grammar_cc::compile(pattern, len, flags);
        const size_t nb = t.next.size() * sizeof(uint16_t);
        char* blk = (char*)malloc(sizeof(skw_grammar) + nb + t.accept.size());
        if (!blk) skw_grammar_cc::fail("out of memory");
        skw_grammar* g = (skw_grammar*)blk; uint16_t* nx = (uint16_t*)(blk + sizeof(skw_grammar)); uint8_t* ac = (uint8_t*)(blk + sizeof(skw_grammar) + nb);
        memcpy(nx, t.next.data(), nb); memcpy(ac, t.accept.data(), t.accept.size());
        g->n_states = (int32_t)t.accept.size(); g->next = nx; g->accept = ac; g->penalty = penalty;
        *out = g; return 0;
    } catch (const skw_grammar_cc::Fail& f) { if (err && errlen) snprintf(err, errlen, "grammar: %s", f.msg); return -1;
    } catch (const std::exception& e) { if (err && errlen) snprintf(err, errlen, "grammar: %s", e.what()); return -1; }
}
static inline void skw_grammar_free_impl(skw_grammar* g) { free(g); }
