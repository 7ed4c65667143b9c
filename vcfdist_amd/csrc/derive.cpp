// derive.cpp -- the text in front of the derived strata (include/vcfdist_derive.h): one compiler for both command lines.
// vpr_derive_compile turns NAME=EXPR into the postfix program k_derive_mask runs (pr_derive.hip), vpr_derive_cross turns LIST:LIST
// into its pairs.  Host code; the messages are made here alone, so the two drivers cannot differ in them.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vcfdist_derive.h"

namespace {

thread_local std::string g_err;

int fail(const std::string &entry, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = "entry '" + entry + "': " + buf;
    return -1;
}

const char *const DELIMITERS = " \t()&|!=,:";
bool is_blank(char c) { return c == ' ' || c == '\t'; }
bool is_name_char(char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '.' || c == '+' || c == '-'; }

// '*' matches any run of characters, the empty one included; every other character matches itself
bool glob_match(const char *g, const char *s) {
    const char *star = nullptr, *back = nullptr;
    while (*s) {
        if (*g == '*') { star = g++; back = s; }
        else if (*g == *s) { g++; s++; }
        else if (star) { g = star + 1; s = ++back; }
        else return false;
    }
    while (*g == '*') g++;
    return !*g;
}

int find(const char *const *names, int32_t n, const std::string &name) {
    for (int32_t k = 0; k < n; k++) if (name == names[k]) return k;
    return -1;
}

// the strata an operand or a glob stands for, in table order (an operand: the one of that name)
enum Lookup { FOUND, UNKNOWN, NO_MATCH };
Lookup lookup(const std::string &tok, const char *const *names, int32_t n, std::vector<int32_t> &out) {
    if (tok.find('*') == std::string::npos) {
        const int k = find(names, n, tok);
        if (k < 0) return UNKNOWN;
        out.push_back(k);
        return FOUND;
    }
    const size_t before = out.size();
    for (int32_t k = 0; k < n; k++) if (glob_match(tok.c_str(), names[k])) out.push_back(k);
    return out.size() > before ? FOUND : NO_MATCH;
}

// NAME=EXPR by recursive descent: or := and ('|' and)*, and := unary ('&' unary)*, unary := '!'* primary, primary := '(' or ')' | operand
struct Compiler {
    const std::string &entry, &own;
    const char *const *names; int32_t n_names;
    const char *p;                     // the rest of the expression
    std::vector<int32_t> code;
    int depth = 0, parens = 0;
    char last = 0;                     // the token in front: an operator, '(' or ')', 'x' for an operand, 0 at the start

    void blanks() { while (is_blank(*p)) p++; }
    int push(int32_t c) {
        code.push_back(c);
        if (++depth > VPR_DV_MAX_DEPTH) return fail(entry, "nesting deeper than %d", VPR_DV_MAX_DEPTH);
        return 0;
    }
    int binary(int32_t op) { code.push_back(op); depth--; return 0; }

    int operand() {
        const size_t n = strcspn(p, DELIMITERS);
        const std::string tok(p, n);
        p += n; last = 'x';
        if (tok == own) return fail(entry, "'%s' is the entry itself", tok.c_str());
        std::vector<int32_t> ks;
        switch (lookup(tok, names, n_names, ks)) {
        case UNKNOWN: return fail(entry, "unknown stratum '%s' (an entry names the strata in front of it)", tok.c_str());
        case NO_MATCH: return fail(entry, "glob '%s' matches no stratum in front of the entry", tok.c_str());
        default: break;
        }
        for (size_t i = 0; i < ks.size(); i++) {        // the union, left-associated: a stack of 2
            if (push(ks[i])) return -1;
            if (i) binary(VPR_DV_OR);
        }
        return 0;
    }
    int primary() {
        blanks();
        const char c = *p;
        if (c == '(') {
            if (++parens > VPR_DV_MAX_DEPTH) return fail(entry, "nesting deeper than %d", VPR_DV_MAX_DEPTH);
            p++; last = '(';
            if (alternatives()) return -1;
            blanks();
            if (*p != ')') return fail(entry, "unbalanced parenthesis: a '(' is never closed");
            p++; last = ')'; parens--;
            return 0;
        }
        if (c == '&' || c == '|') return fail(entry, "dangling operator '%c'", c);
        if (!c || c == ')') {
            if (last == '&' || last == '|' || last == '!') return fail(entry, "dangling operator '%c'", last);
            if (last == '(' && c == ')') return fail(entry, "empty parentheses");
            if (c == ')') return fail(entry, "unbalanced parenthesis: a ')' closes nothing");
            return fail(entry, last == '(' ? "unbalanced parenthesis: a '(' is never closed" : "empty expression");
        }
        if (strchr(DELIMITERS, c)) return fail(entry, "unexpected character '%c' in the expression", c);
        return operand();
    }
    int unary() {
        int n_not = 0;
        for (blanks(); *p == '!'; blanks()) { p++; n_not++; last = '!'; }
        if (primary()) return -1;
        for (int i = 0; i < n_not; i++) code.push_back(VPR_DV_NOT);
        return 0;
    }
    int conjunction() {
        if (unary()) return -1;
        for (blanks(); *p == '&'; blanks()) {
            p++; last = '&';
            if (unary()) return -1;
            binary(VPR_DV_AND);
        }
        return 0;
    }
    int alternatives() {
        if (conjunction()) return -1;
        for (blanks(); *p == '|'; blanks()) {
            p++; last = '|';
            if (conjunction()) return -1;
            binary(VPR_DV_OR);
        }
        return 0;
    }
    int run() {
        if (alternatives()) return -1;
        blanks();
        if (!*p) return 0;
        if (*p == ')') return fail(entry, "unbalanced parenthesis: a ')' closes nothing");
        if (*p == '(' || *p == '!' || !strchr(DELIMITERS, *p)) {
            const size_t n = *p == '(' || *p == '!' ? 1 : strcspn(p, DELIMITERS);
            return fail(entry, "missing operator in front of '%s'", std::string(p, n).c_str());
        }
        return fail(entry, "unexpected character '%c' in the expression", *p);
    }
};

// one side of a cross: glob[,glob...] -> the matching strata in table order, each once
int cross_side(const std::string &entry, const std::string &list, const char *which, const char *const *names, int32_t n_names, std::vector<int32_t> &out) {
    if (list.find_first_not_of(" \t") == std::string::npos) return fail(entry, "empty %s side", which);
    std::vector<char> in(size_t(n_names), 0);
    size_t at = 0;
    while (true) {
        const size_t comma = list.find(',', at);
        std::string tok = list.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        while (!tok.empty() && is_blank(tok.back())) tok.pop_back();
        while (!tok.empty() && is_blank(tok.front())) tok.erase(0, 1);
        if (tok.empty()) return fail(entry, "empty glob on the %s side", which);
        const size_t bad = tok.find_first_of(DELIMITERS);
        if (bad != std::string::npos) return fail(entry, "unexpected character '%c' in '%s'", tok[bad], tok.c_str());
        std::vector<int32_t> ks;
        switch (lookup(tok, names, n_names, ks)) {
        case UNKNOWN: return fail(entry, "unknown stratum '%s' (an entry names the strata in front of it)", tok.c_str());
        case NO_MATCH: return fail(entry, "glob '%s' matches no stratum in front of the entry", tok.c_str());
        default: break;
        }
        for (int32_t k : ks) in[size_t(k)] = 1;
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    for (int32_t k = 0; k < n_names; k++) if (in[size_t(k)]) out.push_back(k);
    return 0;
}

}  // namespace

extern "C" {

const char *vpr_derive_last_error(void) { return g_err.c_str(); }

int vpr_derive_compile(const char *entry_text, const char *const *names, int32_t n_names, char *name_out, size_t name_cap, int32_t *code,
                       int32_t code_cap, int32_t *n_code) {
    if (!entry_text || n_names < 0 || (n_names && !names) || !name_out || !code || code_cap < 0 || !n_code) {
        g_err = "vpr_derive_compile: bad argument";
        return -1;
    }
    const std::string entry = entry_text;
    const size_t eq = entry.find('=');
    if (eq == std::string::npos) return fail(entry, "missing '=' (an entry is NAME=EXPR)");
    std::string name = entry.substr(0, eq);
    while (!name.empty() && is_blank(name.back())) name.pop_back();
    while (!name.empty() && is_blank(name.front())) name.erase(0, 1);
    if (name.empty()) return fail(entry, "empty name");
    for (char c : name)
        if (!is_name_char(c)) return fail(entry, "bad name '%s' (a name is [A-Za-z0-9_.+-]+)", name.c_str());
    if (find(names, n_names, name) >= 0) return fail(entry, "name '%s' is already a stratum", name.c_str());
    if (name.size() + 1 > name_cap) return fail(entry, "name '%s' is longer than %zu characters", name.c_str(), name_cap - 1);
    const std::string expr = entry.substr(eq + 1);
    if (expr.find_first_not_of(" \t") == std::string::npos) return fail(entry, "empty expression");
    Compiler c{entry, name, names, n_names, expr.c_str(), {}};
    if (c.run()) return -1;
    if (c.code.size() > size_t(code_cap)) return fail(entry, "code longer than %d", code_cap);
    memcpy(name_out, name.c_str(), name.size() + 1);
    memcpy(code, c.code.data(), 4 * c.code.size());
    *n_code = int32_t(c.code.size());
    return 0;
}

int vpr_derive_cross(const char *entry_text, const char *const *names, int32_t n_names, int32_t *pairs, int32_t pairs_cap, int32_t *n_pairs) {
    if (!entry_text || n_names < 0 || (n_names && !names) || !pairs || pairs_cap < 0 || !n_pairs) {
        g_err = "vpr_derive_cross: bad argument";
        return -1;
    }
    const std::string entry = entry_text;
    const size_t colon = entry.find(':');
    if (colon == std::string::npos) return fail(entry, "missing ':' (an entry is LIST:LIST)");
    if (entry.find(':', colon + 1) != std::string::npos) return fail(entry, "more than one ':'");
    std::vector<int32_t> left, right;
    if (cross_side(entry, entry.substr(0, colon), "left", names, n_names, left) || cross_side(entry, entry.substr(colon + 1), "right", names, n_names, right))
        return -1;
    int32_t n = 0;
    for (int32_t a : left)
        for (int32_t b : right) {
            if (a == b) continue;
            const std::string name = std::string(names[a]) + "&" + names[b];
            if (find(names, n_names, name) >= 0) return fail(entry, "name '%s' is already a stratum", name.c_str());
            if (n == pairs_cap) return fail(entry, "more than %d pairs", pairs_cap);
            pairs[2 * n] = a; pairs[2 * n + 1] = b;
            n++;
        }
    if (!n) return fail(entry, "the cross yields no pair");
    *n_pairs = n;
    return 0;
}

}  // extern "C"
