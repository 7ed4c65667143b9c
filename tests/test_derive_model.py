"""The derived strata's compiler without a GPU (include/vcfdist_derive.h, vcfdist_amd/csrc/derive.cpp): the program the library
emits for a text, run by the postfix evaluator of tests/derive_model.py, gives what the model's evaluator of the TEXT gives -- on
the cases of tests/derive_cases.py and on random expressions --, the emitted programs are the expected ones where the cases state
them, the crosses give their pairs, and every malformed entry is refused with its message."""
import numpy as np
import pytest

import derive_cases as DC
import derive_model as DM
from vcfdist_amd import _abi as A, api

MEMBER = DC.random_members(len(DC.NAMES), 257, 3)


def test_the_model_evaluates_the_definition():
    """the text evaluator on hand-made bits: precedence, negation as the complement within the slot, a glob as a union"""
    names = ["a", "b", "c"]
    mem = np.array([[1, 1, 0, 0, 1], [1, 0, 1, 0, 0], [0, 0, 1, 1, 1]], bool)
    a, b, c = mem
    ev = lambda e: DM.eval_expr(e, names, mem)
    assert np.array_equal(ev("a|b&c"), a | (b & c)) and not np.array_equal(ev("a|b&c"), (a | b) & c)
    assert np.array_equal(ev("!a&b"), ~a & b) and not np.array_equal(ev("!a&b"), ~(a & b))
    assert np.array_equal(ev("*"), a | b | c) and np.array_equal(ev("!*"), ~(a | b | c)) and np.array_equal(ev("!!a"), a)
    assert np.array_equal(ev("a") ^ ev("!a"), np.ones(5, bool))                 # x and !x partition the variants
    assert np.array_equal(DM.run_postfix([0, 1, 2, DM.AND, DM.OR], mem), a | (b & c))
    assert np.array_equal(DM.run_postfix([0, DM.NOT, 1, DM.AND], mem), ~a & b)
    assert np.array_equal(DM.bits_of(DM.words_of(mem), 3), mem)
    assert DM.cross_pairs("a,b:b,c", names) == [(0, 1), (0, 2), (1, 2)]
    assert (A.DV_AND, A.DV_OR, A.DV_NOT) == (DM.AND, DM.OR, DM.NOT) == (DC.AND, DC.OR, DC.NOT)


def test_the_cases_name_the_default_strata():
    assert api.context_default()[0] == DC.CONTEXT and api.varstrata_default()[0] == DC.VARIANT


def valid_program(code, n_front):
    depth = top = 0
    for c in code:
        assert c in (DM.AND, DM.OR, DM.NOT) or 0 <= c < n_front
        depth += 1 if c >= 0 else -1 if c != DM.NOT else 0
        assert depth >= 1
        top = max(top, depth)
    assert depth == 1
    return top


@pytest.mark.parametrize("entry,equivalent,program", DC.PARSES, ids=[p[0] for p in DC.PARSES])
def test_a_case_compiles_to_its_parse(entry, equivalent, program):
    name, code = api.derive_compile(entry, DC.NAMES)
    assert name == entry.split("=")[0].strip(" \t")
    assert list(code) == program
    assert valid_program(code, len(DC.NAMES)) <= (2 if "(" not in entry and "&" not in entry and "|" not in entry else A.DV_MAX_DEPTH)    # a glob alone: a stack of 2
    want = DM.eval_expr(entry.split("=", 1)[1], DC.NAMES, MEMBER)
    assert np.array_equal(want, DM.eval_expr(equivalent, DC.NAMES, MEMBER))      # the parse the case states
    assert np.array_equal(DM.run_postfix(code, MEMBER), want)


def test_a_sequence_of_entries_sees_the_entries_in_front():
    names, member = list(DC.NAMES), MEMBER
    for entry, equivalent in zip(DC.SEQUENCE, DC.SEQUENCE_EQUIV):
        name, code = api.derive_compile(entry, names)
        row = DM.run_postfix(code, member)
        assert np.array_equal(row, DM.eval_expr(equivalent, names, member)), entry
        names.append(name)
        member = np.vstack([member, row[None]])
    model_names, model_member = DM.derive(DC.SEQUENCE, DC.NAMES, MEMBER)
    assert model_names == names and np.array_equal(model_member, member)
    assert member[names.index("any")].all() and member[names.index("hp_long")].any()      # (any takes in easy, the complement of the rest)


def test_random_expressions_equal_the_model():
    rng = np.random.RandomState(11)
    n_glob = top = 0
    for _ in range(400):
        expr = DC.random_expression(rng, DC.NAMES)
        try:
            want = DM.eval_expr(expr, DC.NAMES, MEMBER)
        except AssertionError:          # (a random glob that matches nothing)
            with pytest.raises(api.VprError):
                api.derive_compile("r=" + expr, DC.NAMES)
            continue
        name, code = api.derive_compile("r=" + expr, DC.NAMES)
        top = max(top, valid_program(code, len(DC.NAMES)))
        n_glob += "*" in expr
        assert np.array_equal(DM.run_postfix(code, MEMBER), want), expr
    assert n_glob > 20 and top >= 4


def test_the_stack_limit_itself_compiles():
    name, code = api.derive_compile(DC.STACK32, DC.NAMES)
    assert valid_program(code, len(DC.NAMES)) == A.DV_MAX_DEPTH
    name, code = api.derive_compile("x=" + "(" * 32 + "hom" + ")" * 32, DC.NAMES)
    assert list(code) == [DC.K["hom"]]
    name, code = api.derive_compile("x=" + "!" * 65535 + "hom", DC.NAMES)          # the code limit itself
    assert len(code) == A.DV_MAX_CODE
    many = [f"s{k}" for k in range(700)]                                          # a glob over hundreds of strata: a stack of 2
    name, code = api.derive_compile("x=!s*", many)
    assert valid_program(code, 700) == 2 and len(code) == 2 * 700


@pytest.mark.parametrize("entry,pairs", DC.CROSSES, ids=[c[0] for c in DC.CROSSES])
def test_a_cross_gives_its_pairs(entry, pairs):
    got = api.derive_cross(entry, DC.NAMES)
    assert [(DC.NAMES[a], DC.NAMES[b]) for a, b in got] == pairs
    assert got == DM.cross_pairs(entry, DC.NAMES)
    names, member = DM.cross([entry], DC.NAMES, MEMBER)
    for i, (a, b) in enumerate(got):
        assert names[len(DC.NAMES) + i] == f"{DC.NAMES[a]}&{DC.NAMES[b]}"
        assert np.array_equal(member[len(DC.NAMES) + i], DM.run_postfix([a, b, DM.AND], MEMBER))


def test_a_cross_may_name_a_derived_stratum_and_no_pair_twice():
    names = DC.NAMES + ["hp_long"]
    assert api.derive_cross("hp_long:hom", names) == [(len(DC.NAMES), DC.K["hom"])]
    assert len(api.derive_cross("ins_*,del_*,snp_*,hom,het,iso_50,near_10:hp_*,tr_*,gc_*", DC.NAMES)) == 154
    with pytest.raises(api.VprError) as e:
        api.derive_cross("hom:het", names + ["hom&het"])
    assert str(e.value) == "entry 'hom:het': name 'hom&het' is already a stratum"
    with pytest.raises(api.VprError) as e:
        api.derive_cross("hom,het:snp_*", DC.NAMES, pairs_cap=3)
    assert str(e.value) == "entry 'hom,het:snp_*': more than 3 pairs"
    assert len(api.derive_cross("hom,het:snp_*", DC.NAMES, pairs_cap=4)) == 4


@pytest.mark.parametrize("entry,what", DC.MALFORMED, ids=[m[0][:40] for m in DC.MALFORMED])
def test_a_malformed_entry_is_refused(entry, what):
    with pytest.raises(api.VprError) as e:
        api.derive_compile(entry, DC.NAMES)
    assert str(e.value) == f"entry '{entry}': {what}"


@pytest.mark.parametrize("entry,what", DC.MALFORMED_CROSS, ids=[m[0] for m in DC.MALFORMED_CROSS])
def test_a_malformed_cross_is_refused(entry, what):
    with pytest.raises(api.VprError) as e:
        api.derive_cross(entry, DC.NAMES)
    assert str(e.value) == f"entry '{entry}': {what}"


def test_a_small_code_buffer_is_refused():
    with pytest.raises(api.VprError) as e:
        api.derive_compile("x=hom|het", DC.NAMES, code_cap=2)
    assert str(e.value) == "entry 'x=hom|het': code longer than 2"
    assert list(api.derive_compile("x=hom|het", DC.NAMES, code_cap=3)[1]) == [DC.K["hom"], DC.K["het"], DC.OR]
    # a later entry is not known where the earlier one is compiled; with it in front the same text compiles
    with pytest.raises(api.VprError) as e:
        api.derive_compile("p=q", DC.NAMES)
    assert str(e.value) == "entry 'p=q': unknown stratum 'q'" + DC.U
    assert list(api.derive_compile("p=q", DC.NAMES + ["q"])[1]) == [len(DC.NAMES)]
