"""The Python driver's totals (vcfdist_amd/__main__.py): the vector that is summed over the ranks is packed and unpacked without a
process group, and the default strata of the four families have names of their own, so one loop can refuse a duplicate for all four."""
import itertools

import numpy as np
import pytest

from vcfdist_amd import __main__ as CLI, _abi as A, api

INPUTS = ["q.vcf", "t.vcf", "ref.fa"]          # (never opened)


def _totals(options, names=(), n_variant=0):
    args = CLI.parse(INPUTS + ["-mn", "0", "-mx", "1"] + options)
    plan = None
    if names:
        plan = CLI.StrataPlan(names=list(names))
        plan.vs.specs = [None] * n_variant
    return CLI.Totals(args, plan)


def _every_section():
    """nq = 2, three strata of which two are variant strata, two replicates, both label passes and their cuts, every entry distinct"""
    tot = _totals(["--stratify-variants", "--bootstrap", "2", "--classify-errors", "--classify-matches", "--cut-classes"], "abc", 2)
    at = 1
    for a in tot.tally:
        a[...] = np.arange(at, at + a.size).reshape(a.shape)
        at += a.size
    return tot


def test_layout():
    tot = _every_section()
    e, m = tot.passes
    want = [tot.total, tot.strat, tot.seen_none, tot.vs_members, tot.boot, tot.boot_strat, e.counts, m.counts, e.strata, e.boot, m.strata, m.boot]
    assert len(tot.tally) == len(want) and all(a is b for a, b in zip(tot.tally, want))
    assert [a.shape for a in want] == [(2, 4, 3, 2), (3, 2, 4, 3, 2), (2,), (2, 2), (2, 2, 4, 3, 2), (3, 2, 2, 4, 3, 2),
                                       (2, 4, A.EC_CLASSES, 2), (2, 4, A.MK_KINDS, 2), (3, 2, 4, A.EC_CLASSES, 2), (2, 2, 4, A.EC_CLASSES, 2),
                                       (3, 2, 4, A.MK_KINDS, 2), (2, 2, 4, A.MK_KINDS, 2)]
    vec = CLI.pack(tot.tally)
    assert vec.dtype == np.int64 and vec.shape == (sum(a.size for a in want),)
    assert np.array_equal(vec[:tot.total.size], tot.total.ravel())
    assert np.array_equal(vec, np.arange(1, vec.size + 1))          # (filled in the vector's order: every section lies where it is expected)


def test_round_trip():
    tot = _every_section()
    before = [(a, a.copy()) for a in tot.tally]
    CLI.unpack(tot.tally, CLI.pack(tot.tally) * 2)
    for a, was in before:
        assert a.shape == was.shape and a.dtype == was.dtype == np.int64 and np.array_equal(a, 2 * was)
    e, m = tot.passes
    assert tot.tally[0] is tot.total and tot.tally[-1] is m.boot and tot.tally[-4] is e.strata          # (the owners hold the sums)


def test_total_alone():
    tot = _totals([])
    tot.total[...] = np.arange(1, 49).reshape(2, 4, 3, 2)
    assert tot.passes == [] and len(tot.tally) == 1 and np.array_equal(CLI.pack(tot.tally), np.arange(1, 49))
    CLI.unpack(tot.tally, np.arange(48, 0, -1))
    assert np.array_equal(tot.total.ravel(), np.arange(48, 0, -1))


DEFAULTS = (("--stratify-repeats", "repeat", api.repeats_default), ("--stratify-long-repeats", "long repeat", api.longrepeats_default),
            ("--stratify-context", "sequence-context", api.context_default), ("--stratify-variants", "variant", api.varstrata_default))


def test_default_names_are_distinct():
    """the one loop checks a default name against every name in front of it, the list's and the earlier families': no two families
    share a name, so it refuses what the four separate checks refused"""
    assert [(f["option"], f["word"], f["defaults"]) for f in CLI.FAMILIES] == list(DEFAULTS)
    names = [list(defaults()[0]) for _, _, defaults in DEFAULTS]
    assert all(len(n) >= 3 and len(set(n)) == len(n) for n in names)
    for a, b in itertools.combinations(names, 2):
        assert not set(a) & set(b), (a, b)


@pytest.mark.parametrize("option,word,defaults", DEFAULTS)
def test_a_default_name_in_the_list_is_refused(tmp_path, option, word, defaults):
    name = defaults()[0][-1]
    (tmp_path / "a.bed").write_text("chr1\t10\t20\n")
    lst = tmp_path / "list.tsv"
    lst.write_text(f"whole\ta.bed\n{name}\ta.bed\n")
    missing = [str(tmp_path / "no_query.vcf"), str(tmp_path / "no_truth.vcf"), str(tmp_path / "no.fa")]
    every = [o for o, _, _ in DEFAULTS]
    for options in ([option], every):               # (alone, and behind the families in front of it)
        with pytest.raises(SystemExit) as e:
            CLI.main(missing + ["--stratify", str(lst)] + options)
        assert str(e.value) == f"ERROR: strata list '{lst}': duplicate stratum name '{name}' (a {word} stratum of {option})"
    with pytest.raises(Exception) as e:             # (without the family the list is fine: the first input does not exist)
        CLI.main(missing + ["--stratify", str(lst)] + [o for o in every if o != option])
    assert "no_query" in str(e.value)
