"""The derived strata of include/vcfdist_derive.h, stated twice without any project code: an evaluator of the TEXT (NAME=EXPR, and
LIST:LIST crosses) over a boolean matrix member[n_strata][n_var], written from the definition -- precedence, globs, unions -- and
not from the postfix; and an evaluator of a raw postfix program."""
import re

import numpy as np

AND, OR, NOT = -1, -2, -3
DELIMITERS = " \t()&|!=,:"


def glob_matches(glob, names):
    """the indices of the names a glob matches, in table order: '*' is any run of characters, every other character itself"""
    rx = re.compile("".join(".*" if c == "*" else re.escape(c) for c in glob), re.S)
    return [k for k, n in enumerate(names) if rx.fullmatch(n)]


def operand_strata(tok, names):
    """the strata an operand stands for: the one of that name, or with a '*' everything the glob matches"""
    return glob_matches(tok, names) if "*" in tok else [names.index(tok)]


def tokens(expr):
    out, i = [], 0
    while i < len(expr):
        c = expr[i]
        if c in " \t":
            i += 1
        elif c in "()&|!":
            out.append(c); i += 1
        else:
            j = i
            while j < len(expr) and expr[j] not in DELIMITERS:
                j += 1
            assert j > i, expr
            out.append(expr[i:j]); i = j
    return out


def eval_expr(expr, names, member):
    """the members of EXPR, a bool vector: member[k] is the bool vector of names[k]'s members"""
    toks = tokens(expr)
    at = [0]

    def peek():
        return toks[at[0]] if at[0] < len(toks) else None

    def take():
        at[0] += 1
        return toks[at[0] - 1]

    def primary():
        t = take()
        if t == "!":
            return ~primary()
        if t == "(":
            x = union()
            assert take() == ")"
            return x
        ks = operand_strata(t, names)
        assert ks, t
        x = np.zeros(member.shape[1], bool)
        for k in ks:            # a glob is the union of what it matches
            x = x | member[k]
        return x

    def conjunction():
        x = primary()
        while peek() == "&":
            take()
            x = x & primary()
        return x

    def union():
        x = conjunction()
        while peek() == "|":
            take()
            x = x | conjunction()
        return x
    x = union()
    assert at[0] == len(toks), expr
    return x


def derive(entries, names, member):
    """NAME=EXPR entries one after the other, each against the names in front of it -> (all names, the matrix with their rows appended)"""
    names, member = list(names), np.asarray(member, bool)
    for e in entries:
        name, expr = e.split("=", 1)
        row = eval_expr(expr, names, member)
        names.append(name.strip(" \t"))
        member = np.vstack([member, row[None]])
    return names, member


def cross_pairs(entry, names):
    """LIST:LIST -> the pairs (a, b), a != b, left-major; each side the matching strata in table order, each once"""
    left, right = entry.split(":")
    side = lambda text: sorted({k for g in text.split(",") for k in operand_strata(g.strip(" \t"), names)})
    return [(a, b) for a in side(left) for b in side(right) if a != b]


def cross(entries, names, member):
    names, member = list(names), np.asarray(member, bool)
    for e in entries:
        pairs = cross_pairs(e, names)
        member = np.vstack([member] + [(member[a] & member[b])[None] for a, b in pairs])
        names += [names[a] + "&" + names[b] for a, b in pairs]
    return names, member


def run_postfix(code, member):
    """a raw program over member[n_strata][n_var] -> the bool vector it leaves"""
    st = []
    for c in code:
        if c >= 0:
            st.append(member[c].copy())
        elif c == NOT:
            st[-1] = ~st[-1]
        else:
            b, a = st.pop(), st.pop()
            st.append(a & b if c == AND else a | b)
    assert len(st) == 1
    return st[0]


def run_programs(code_off, code, member):
    """the entries of one call: entry j sees the rows in front of it, earlier entries included -> the matrix with their rows appended"""
    member = np.asarray(member, bool)
    for j in range(len(code_off) - 1):
        member = np.vstack([member, run_postfix(code[code_off[j]:code_off[j + 1]], member)[None]])
    return member


def words_of(member):
    """member[n_strata][n_var] -> uint64 [n_words][n_var], bit k & 63 of word k >> 6"""
    n, nv = member.shape
    w = np.zeros(((n + 63) // 64, nv), np.uint64)
    for k in range(n):
        w[k >> 6] |= member[k].astype(np.uint64) << np.uint64(k & 63)
    return w


def bits_of(words, n_strata):
    """the inverse: uint64 [n_words][n_var] -> bool [n_strata][n_var]"""
    return np.stack([((words[k >> 6] >> np.uint64(k & 63)) & np.uint64(1)).astype(bool) for k in range(n_strata)]) if n_strata else \
        np.zeros((0, words.shape[1]), bool)
