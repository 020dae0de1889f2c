"""The host reference of the null-group draws (tests/null_sampler_ref.py), checked on the CPU.

(a) its Philox against the published known-answer vectors of Random123;
(b) the draw rule is exact: over all 2^48 values of (16 bits, 32 tie bits) a column joins A in exactly ceil(needA 2^48 / rem) of
    them and A or B in ceil(needAB 2^48 / rem) -- P differs from need / rem by less than 2^-48 -- and what 16 bits alone decide
    is what every 48-bit value with those 16 bits gives;
(c) the whole-row law: chi-square of 400 000 draws of one row against the exact multivariate hypergeometric pmf of (oA, oB);
(d) the digests of tests/golden/null_draws.json, which a device recorded, are those of the reference: all 144."""
import functools
import json
from fractions import Fraction
from math import comb

import numpy as np
import pytest

from tests import null_sampler_ref as ref


# ------------------------------------------------------------------------------------------------ (a) Philox
KAT = [  # Random123 kat_vectors, philox4x32-10: counter, key, result
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_known_answers():
    for counter, key, want in KAT:
        assert tuple(int(x) for x in ref.philox4x32_10(counter, key)) == want
    # vectorised over rows: the three at once
    got = ref.philox4x32_10([np.array([k[0][i] for k in KAT]) for i in range(4)], [np.array([k[1][i] for k in KAT]) for i in range(2)])
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]


# ------------------------------------------------------------------------------------------------ (b) the draw rule
def _ceil_div(a, b):
    return -(-a // b)


def _words_below(v, rem, need):
    """How many of the 2^32 tie words w give tie_pick(v, w, rem) < need: pick < need <=> (v 2^32 + w) rem < need 2^48.  The two
    tie_pick calls at the boundary prove the count, since the pick is monotone in w."""
    c = min(max(_ceil_div(need << 48, rem) - (v << 32), 0), 1 << 32)
    assert c == 0 or ref.tie_pick(v, c - 1, rem) < need
    assert c == 1 << 32 or ref.tie_pick(v, c, rem) >= need
    return c


@pytest.mark.parametrize("rem", range(1, 25))
def test_draw_rule_is_exact(rem):
    v = np.arange(65536, dtype=np.int64)
    lo = ((v << 32) * rem) >> 48                                            # the pick with the smallest and the largest tie word
    hi = (((v << 32) | 0xFFFFFFFF) * rem) >> 48                             # (< 2^53: exact in int64)
    for needA in range(rem + 1):
        for needAB in range(needA, rem + 1):
            dec = ref.decide16(v, rem, needA, needAB)
            # 16 bits never contradict 48
            assert (hi[dec == ref.A] < needA).all()
            assert (lo[dec == ref.B] >= needA).all() and (hi[dec == ref.B] < needAB).all()
            assert (lo[dec == ref.NEITHER] >= needAB).all()
            ties = [int(x) for x in v[dec == ref.TIE]]
            assert len(ties) <= 2
            inA, inAB = int((dec == ref.A).sum()) << 32, int((dec != ref.NEITHER).sum() - len(ties)) << 32
            for t in ties:                                                  # a tie is a value whose 32 more bits matter
                assert ref.from_pick(int(lo[t]), needA, needAB) != ref.from_pick(int(hi[t]), needA, needAB)
                inA += _words_below(t, rem, needA)
                inAB += _words_below(t, rem, needAB)
            assert inA == _ceil_div(needA << 48, rem) and inAB == _ceil_div(needAB << 48, rem)
            assert 0 <= Fraction(inA, 1 << 48) - Fraction(needA, rem) < Fraction(1, 1 << 48)
            assert 0 <= Fraction(inAB, 1 << 48) - Fraction(needAB, rem) < Fraction(1, 1 << 48)


def test_equality_edge_is_not_a_tie():
    """(v + 1) rem == need << 16: the interval ends AT the threshold, the column joins A; one more column needed by B: B."""
    assert int(ref.decide16(32767, 64, 32, 64)) == ref.A and int(ref.decide16(32768, 64, 32, 64)) == ref.B
    assert int(ref.decide16(65535, 64, 32, 64)) == ref.B and int(ref.decide16(49151, 64, 32, 48)) == ref.B
    assert int(ref.decide16(49152, 64, 32, 48)) == ref.NEITHER
    assert int(ref.decide16(21845, 3, 1, 3)) == ref.TIE                     # 65536 / 3 lies inside [21845, 21846)


# ------------------------------------------------------------------------------------------------ (c) the whole-row law
N_DRAWS = 400000


def mvhg_pmf(h, stateless, ga, gb):
    """{(oA, oB) as a tuple of 2 S counts: probability}: the per-state counts of the first ga and the next gb columns of a uniform
    permutation of a row with h[s] columns of state s and `stateless` columns without one (which take places, unreported)."""
    n = sum(h) + stateless
    total = comb(n, ga) * comb(n - ga, gb)
    cells = {}

    def walk(s, a_left, b_left, ways, oa, ob):
        if s == len(h):
            if a_left + b_left <= stateless:
                key = tuple(oa) + tuple(ob)
                cells[key] = cells.get(key, 0) + ways * comb(stateless, a_left) * comb(stateless - a_left, b_left)
            return
        for a in range(min(h[s], a_left) + 1):
            for b in range(min(h[s] - a, b_left) + 1):
                walk(s + 1, a_left - a, b_left - b, ways * comb(h[s], a) * comb(h[s] - a, b), oa + [a], ob + [b])

    walk(0, ga, gb, 1, [], [])
    assert sum(cells.values()) == total
    return {k: Fraction(w, total) for k, w in cells.items()}


def chi_square_p(oA, oB, pmf):
    """The p-value of the observed rows of (oA, oB) against the pmf; cells with expectation < 5 are pooled into one."""
    from scipy.stats import chi2
    n = oA.shape[0]
    seen, counts = np.unique(np.concatenate([oA, oB], axis=1).astype(np.int64), axis=0, return_counts=True)
    observed = {tuple(int(x) for x in k): int(c) for k, c in zip(seen, counts)}
    assert set(observed) <= set(pmf), "an outcome of probability 0"
    stat, cells, pool_e, pool_o = 0.0, 0, 0.0, 0
    for k, p in pmf.items():
        e, o = float(p * n), observed.get(k, 0)
        if e < 5:
            pool_e, pool_o = pool_e + e, pool_o + o
        else:
            stat, cells = stat + (o - e) ** 2 / e, cells + 1
    if pool_e > 0:
        stat, cells = stat + (pool_o - pool_e) ** 2 / pool_e, cells + 1
    return float(chi2.sf(stat, cells - 1)), cells


LAW_ROWS = [  # h, columns without a state, ga, gb, seed
    ((8, 6, 7), 0, 12, 9, ref.SEEDS[0]),
    ((5, 5, 3, 2), 0, 4, 6, ref.SEEDS[1]),
    ((4, 3, 2, 1), 2, 3, 2, ref.SEEDS[0]),
    ((6, 6, 4), 0, 9, 7, ref.SEEDS[1]),                                      # two equal maxima, default sizes
]


@pytest.mark.parametrize("h,stateless,ga,gb,seed", LAW_ROWS)
def test_hist_sampler_law(h, stateless, ga, gb, seed):
    n = sum(h) + stateless
    hA = np.tile(np.array([x // 2 for x in h], dtype=np.uint16), (N_DRAWS, 1))     # any split of h between the real groups
    hB = np.tile(np.array([x - x // 2 for x in h], dtype=np.uint16), (N_DRAWS, 1))
    oA, oB, _info = ref.sample_from_hist(hA, hB, n, ga, gb, seed, ref.KEYS[0])
    p, cells = chi_square_p(oA, oB, mvhg_pmf(h, stateless, ga, gb))
    print("h=%s stateless=%d ga=%d gb=%d: %d cells, p=%.4g" % (h, stateless, ga, gb, cells, p))
    assert p >= 1e-6


def test_matrix_sampler_law():
    """sample_from_matrix on one row of 7 + 6 columns, one of them without a state, -g 4 + 5."""
    xa, xb = np.array([0, 2, 1, 0, -1, 3, 0], dtype=np.int8), np.array([1, 0, 0, 2, 1, 0], dtype=np.int8)
    S, ga, gb = 4, 4, 5
    oA, oB = ref.sample_from_matrix(np.tile(xa, (N_DRAWS, 1)), np.tile(xb, (N_DRAWS, 1)), S, ga, gb, ref.SEEDS[0], ref.KEYS[0])
    h = tuple(int(((xa == s).sum() + (xb == s).sum())) for s in range(S))
    p, cells = chi_square_p(oA, oB, mvhg_pmf(h, 1, ga, gb))
    print("matrix h=%s: %d cells, p=%.4g" % (h, cells, p))
    assert p >= 1e-6


# ------------------------------------------------------------------------------------------------ (d) the recorded digests
@functools.lru_cache(maxsize=2)
def _inputs(na, nb, S, rows):
    parts = ref._parts(na, nb, S, rows)
    return parts, [ref._hist(a, S) for a, _b in parts], [ref._hist(b, S) for _a, b in parts]


@functools.lru_cache(maxsize=None)
def _null_groups(na, nb, S, rows, ga, gb, seed):
    """(OAs, OBs, ties) of the reference for a case: part by part, every part under its own key."""
    _parts, HAs, HBs = _inputs(na, nb, S, rows)
    OAs, OBs, ties = [], [], 0
    for hA, hB, key in zip(HAs, HBs, ref._keys(rows)):
        oA, oB, info = ref.sample_from_hist(hA, hB, na + nb, ga, gb, seed, key)
        OAs.append(oA)
        OBs.append(oB)
        ties += info["ties_A"] + info["ties_AB"]
    return OAs, OBs, ties


@pytest.fixture(scope="module")
def recorded():
    return json.loads(ref.FIXTURE.read_text())["digests"]


def test_every_recorded_digest_has_a_case(recorded):
    labels = [ref.hist_label(na, nb, S, rows, ga, gb, force, seed) for na, nb, S, rows in ref.HIST_CASES
              for ga, gb in ref.hist_group_sizes(na, nb) for force in (0, 1) for seed in ref.SEEDS]
    labels += [ref.fused_label(na, nb, S, rows, seed) for na, nb, S, rows in ref.FUSED_CASES for seed in ref.SEEDS]
    assert len(labels) == len(set(labels)) == 144 and set(labels) == set(recorded)


@pytest.mark.parametrize("na,nb,S,rows", ref.HIST_CASES, ids=lambda x: ref._rows_label(x) if isinstance(x, tuple) else str(x))
def test_recorded_hist_digests_are_the_references(recorded, na, nb, S, rows):
    """One reference run serves the library's own choice of kernel and the column-by-column one: the draws do not depend on it."""
    ties = 0
    for ga, gb in ref.hist_group_sizes(na, nb):
        for seed in ref.SEEDS:
            OAs, OBs, t = _null_groups(na, nb, S, rows, ga, gb, seed)
            ties += t
            for force in (0, 1):
                label = ref.hist_label(na, nb, S, rows, ga, gb, force, seed)
                assert ref.digest_arrays((OAs, OBs)) == recorded[label], label
    print("ties taken:", ties)


@pytest.mark.parametrize("na,nb,S,rows", ref.FUSED_CASES, ids=lambda x: ref._rows_label(x) if isinstance(x, tuple) else str(x))
def test_recorded_fused_digests_are_the_references(recorded, na, nb, S, rows):
    """epg_pair_count_null_parts: the real groups' histograms, the state counts (int64) and the null groups."""
    _parts, HAs, HBs = _inputs(na, nb, S, rows)
    counts = sum(h.sum(axis=0, dtype=np.int64) for h in HAs + HBs)
    for seed in ref.SEEDS:
        OAs, OBs, _t = _null_groups(na, nb, S, rows, na, nb, seed)
        label = ref.fused_label(na, nb, S, rows, seed)
        assert ref.digest_arrays((HAs, HBs, [counts], OAs, OBs)) == recorded[label], label
