"""The model of the near-repeat strata (tests/nearrepeats_model.py) against itself: `fast`, the pigeonhole, is held to `brute`, the
definition, on every planted case that brute can do and on random genomes; every case of tests/nearrepeats_cases.py is what it
declares; m = 0 is the exact family; the strata are nested."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import nearrepeats_cases as NC
import nearrepeats_model as NM
import repeats_model as RM

Spec = namedtuple("Spec", "k m slop")
BRUTE_MAX = 3000
KM = [(16, 1), (24, 1), (25, 1), (32, 1), (24, 2), (31, 2), (32, 2), (32, 3)]


@functools.lru_cache(maxsize=None)
def cases():
    return NC.all_cases()


def n_valid(case, k):
    return sum(int(NM.strands(NM.as_bytes(c), k)[0].sum()) for c in case.contigs)


def test_fast_equals_brute_on_the_small_cases():
    done = 0
    for case in cases():
        for k, m in case.specs:
            if n_valid(case, k) > BRUTE_MAX:
                continue
            a, b = NM.brute(case.contigs, k, m), NM.fast(case.contigs, k, m)
            assert a[1:] == b[1:] and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])), (case.name, k, m)
            done += 1
    assert done > 100


@pytest.mark.parametrize("k,m", KM)
def test_fast_equals_brute_on_random_genomes(k, m):
    """mutated forward and reverse-complemented copies, a copy on a second contig, an N, an empty contig and one of k - 1 bases"""
    rng = np.random.default_rng(1000 * k + m)
    for _ in range(3):
        g = NC.Genome(rng, flank=30)
        for d in range(m + 3):
            pos = tuple(int(p) for p in rng.choice(k, d, replace=False))
            g.pair(k, pos, bool(d % 2))
            g.pair(k, pos, not d % 2)
        c0 = bytearray(g.done())
        c0[len(c0) // 2] = ord("N")
        src = int(rng.integers(0, len(c0) // 3))
        c2 = NC.rnd(rng, 50) + NC.mutate(bytes(c0[src:src + k]).replace(b"N", b"A"), [k // 2]) + NC.rnd(rng, 50)
        contigs = [bytes(c0), b"", c2, NC.rnd(rng, k - 1)]
        a, b = NM.brute(contigs, k, m), NM.fast(contigs, k, m)
        assert a[1] <= BRUTE_MAX and a[2] > 0
        assert a[1:] == b[1:] and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        # the long-run path of `fast` too
        c = NM.fast(contigs, k, m, small=2, chunk=3)
        assert a[1:] == c[1:] and all(np.array_equal(x, y) for x, y in zip(a[0], c[0]))


@pytest.mark.parametrize("k", NC.MONO_M0_K)
def test_m0_is_the_exact_family(k):
    contigs, _ = NC.mono_genome()
    contigs = contigs + [contigs[0][100:400]]
    a, b = RM.repeated(contigs, k), NM.fast(contigs, k, 0)
    assert a[1:] == b[1:] and a[2] > 0 and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    rows_a = RM.all_intervals(contigs, [Spec(k, 0, 2)])[0]
    rows_b = NM.all_intervals(contigs, [Spec(k, 0, 2)])[0]
    assert not NM.same(rows_a, rows_b)


def test_every_case_is_what_it_declares():
    names = [c.name for c in cases()]
    assert len(set(names)) == len(names)
    for prefix in ("pos_", "over_", "self_", "shift_", "run_", "strand_", "seam_", "n_", "edge_", "mono_"):
        assert any(n.startswith(prefix) for n in names), prefix
    for case in cases():
        assert 2 <= len(case.specs) <= NM.MAX_SPEC and sum(len(c) for c in case.contigs) <= 320_000, case.name
        memo = {}
        for k, m in case.specs:
            assert 0 <= m <= NM.MAX_M and 8 * (m + 1) <= k <= NM.MAX_K
            memo[(k, m)] = NM.fast(case.contigs, k, m)
        for k, m, c, i in case.near:
            assert memo[(k, m)][0][c][i], (case.name, "near", k, m, c, i)
        for k, m, c, i in case.clean:
            assert not memo[(k, m)][0][c][i], (case.name, "clean", k, m, c, i)
        for (k, m), n in case.total.items():
            assert memo[(k, m)][2] == n, (case.name, "total", k, m, memo[(k, m)][2], n)
        assert case.near or case.clean or case.total, case.name


def test_the_strata_are_nested():
    case = [c for c in cases() if c.name == "mono_k32"][0]
    last = None
    for m in range(4):
        near, _, n = NM.fast(case.contigs, 32, m)
        if last is not None:
            assert all((a <= b).all() for a, b in zip(last[0], near)) and n > last[1]
        last = (near, n)


def test_blocks_and_names():
    assert NM.blocks(32, 1) == [(0, 16), (16, 32)] and NM.blocks(31, 1) == [(0, 15), (15, 31)]
    assert NM.blocks(25, 1) == [(0, 12), (12, 25)] and NM.blocks(31, 2) == [(0, 10), (10, 20), (20, 31)]
    assert NM.blocks(32, 3) == [(0, 8), (8, 16), (16, 24), (24, 32)] and NM.blocks(32, 0) == [(0, 32)]
    assert all(b - a <= 16 for k in range(16, 33) for m in range(1, 4) if k >= 8 * (m + 1) for a, b in NM.blocks(k, m))
    assert NM.name(32, 1) == "near_k32_m1"
