"""GPU: the paired-mode null groups equal the host reference (tests/null_sampler_ref.py) bit for bit.

tests/test_null_sampler_ref.py shows on the CPU that the reference's draw rule is exact and that it reproduces the recorded
digests of tests/golden/null_draws.json.  Here the shapes those cases never reach go through every way into the sampler that
takes them:

  hist   epg_null_hist_from_binhist, the library's own choice of sampler
  seq    the same with the column-by-column sampler forced
  fused  epg_pair_count_null_parts (count pass + draw; default group sizes, S = 15 / 18 / 25)
  draws  epg_null_dist_draws_parts: its floats against epg_pair_scores_s1_parts on the REFERENCE's null groups

and the matrix-scanning epg_null_hist against sample_from_matrix."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import null_sampler_ref as ref

pytestmark = pytest.mark.gpu
S18 = 18
HIGH_KEY = (3 << 40) + 17                                                    # a row key with a non-zero high word

# name -> (NA, NB, S, [(ga, gb, ways)], seeds); the rows of a case: _inputs
CASES = {
    # ties wherever a kernel can meet one: in a speculative call of eight, in a row's last 1 .. 7 draws, at either threshold
    "ties": (379, 342, S18, [(379, 342, "hist seq fused draws"), (100, 100, "hist seq draws")], ref.SEEDS),
    # uniform states, need << 16 a multiple of rem again and again: (v + 1) rem == need << 16 must give A, not a tie
    "edge32": (32, 32, S18, [(32, 32, "hist seq fused draws"), (8, 8, "hist seq draws")], ref.SEEDS),
    "edge64": (64, 64, S18, [(64, 64, "hist seq fused draws"), (8, 8, "hist seq draws")], ref.SEEDS),
    # rows shorter than one Philox call: only the tail path runs
    "short9": (5, 4, 5, [(5, 4, "hist seq draws"), (2, 2, "hist seq draws")], ref.SEEDS),
    "short21": (12, 9, S18, [(12, 9, "hist seq fused draws"), (4, 4, "hist seq draws")], ref.SEEDS),
    # -g at the limit of two bit strings: 1536 columns take them, 1537 go column by column (and are beyond the draws kernel)
    "two1536": (768, 768, S18, [(100, 100, "hist seq draws")], ref.SEEDS),
    "two1537": (769, 768, S18, [(100, 100, "hist seq")], ref.SEEDS),
    # the widest row the entry point takes: the u32 arithmetic of the column-by-column sampler at its end
    "widest": (32768, 32767, S18, [(32768, 32767, "hist"), (40000, 25000, "hist")], ref.SEEDS[1:]),
    # rows without a state, of one state, with two equal maxima; groups of one column, groups that leave one column out
    "degenerate": (20, 17, S18, [(20, 17, "hist seq fused draws"), (1, 1, "hist seq draws"), (18, 18, "hist seq draws"),
                                 (36, 1, "hist seq draws")], ref.SEEDS),
    # the flagship width under a key with a non-zero high word
    "highkey": (379, 342, S18, [(379, 342, "hist seq fused draws"), (100, 100, "hist seq draws")], ref.SEEDS),
}
TIE_GENERIC, TIE_SHORT = 7000, 80000                                         # rows of the tie case: see _tie_rows
EDGE_ROWS = 20000                                                            # an equality edge takes one v in 65536, too


def _tie_rows(rng, NA, NB, S):
    """A tie takes one value of v in 65536 per threshold and draw, so ties need draws: TIE_GENERIC rows as in the recorded cases
    (~200 draws each, nearly all in full calls) and TIE_SHORT rows of the modal state with 1 .. 7 other columns (seven in three
    rows of four), whose every draw is a tail draw."""
    n = NA + NB
    x = np.full((TIE_SHORT, n), S - 1, dtype=np.int8)
    pos, st = rng.integers(0, n, size=(TIE_SHORT, 7)), rng.integers(0, S - 1, size=(TIE_SHORT, 7)).astype(np.int8)
    rows = np.arange(TIE_SHORT)
    others = np.where(rows % 4, 7, 1 + (rows // 4) % 7)
    for k in range(7):
        some = rows[others > k]
        x[some, pos[some, k]] = st[some, k]
    return (np.concatenate([ref._states(rng, TIE_GENERIC, NA, S), x[:, :NA]]),
            np.concatenate([ref._states(rng, TIE_GENERIC, NB, S), x[:, NA:]]))


def _degenerate_rows(rng, NA, NB, S):
    xa, xb = ref._states(rng, 140, NA, S), ref._states(rng, 140, NB, S)
    for r in range(0, 140, 7):                                               # spread over the waves' lanes
        k = (r // 7) % 4
        if k == 0:                                                           # no column holds a state: every position is drawn
            xa[r], xb[r] = -1, -1
        elif k == 1:                                                         # two equal maxima: the first one is modal
            xa[r, :NA // 2], xa[r, NA // 2:] = 9, 4
            xb[r], xb[r, :5], xb[r, 5:10] = 2, 4, 9
            h = ref._hist(xa[r:r + 1], S)[0].astype(int) + ref._hist(xb[r:r + 1], S)[0]
            assert h[4] == h[9] == h.max() and NA % 2 == 0
        elif k == 2:                                                         # one state only
            xa[r], xb[r] = 6, 6
        else:                                                                # one state and columns without one
            xa[r], xb[r] = 0, -1
    return xa, xb


@functools.lru_cache(maxsize=2)
def _inputs(name):
    """(hA, hB uint16 [R, S], xa, xb int8 state matrices or None, key of the first row)."""
    NA, NB, S = CASES[name][:3]
    rng = np.random.default_rng([NA, NB, S, len(name)])
    if name == "widest":                                                     # histograms only: ~90 % of a row in one state
        h = np.stack([rng.multinomial(NA + NB, [0.9 if s == (5 * r) % S else 0.1 / (S - 1) for s in range(S)]) for r in range(8)])
        hA = rng.binomial(h, NA / (NA + NB))
        return hA.astype(np.uint16), (h - hA).astype(np.uint16), None, None, HIGH_KEY
    if name == "ties":
        xa, xb = _tie_rows(rng, NA, NB, S)
    elif name == "degenerate":
        xa, xb = _degenerate_rows(rng, NA, NB, S)
    elif name.startswith(("edge", "short")):
        R = EDGE_ROWS if name.startswith("edge") else 300
        xa, xb = rng.integers(0, S, size=(R, NA)).astype(np.int8), rng.integers(0, S, size=(R, NB)).astype(np.int8)
    else:
        xa, xb = ref._states(rng, 130, NA, S), ref._states(rng, 130, NB, S)
    return ref._hist(xa, S), ref._hist(xb, S), xa, xb, ref.KEYS[0] if name in ("ties", "two1536") else HIGH_KEY


@functools.lru_cache(maxsize=4)
def _reference(name, ga, gb, seed):
    hA, hB, _xa, _xb, key0 = _inputs(name)
    NA, NB = CASES[name][:2]
    # (rows draw independently of one another: the short rows of the tie case go separately, not through the long rows' steps)
    cuts = [0, TIE_GENERIC, hA.shape[0]] if name == "ties" else [0, hA.shape[0]]
    blocks = [ref.sample_from_hist(hA[a:b], hB[a:b], NA + NB, ga, gb, seed, key0 + a) for a, b in zip(cuts, cuts[1:])]
    oA, oB = np.concatenate([blk[0] for blk in blocks]), np.concatenate([blk[1] for blk in blocks])
    info = {k: sum(blk[2][k] for blk in blocks) for k in blocks[0][2]}
    print("%s ga=%d gb=%d seed=%d: rows=%d %s" % (name, ga, gb, seed, hA.shape[0], info))
    return oA, oB, info


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


def _dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16)).cuda()


def _tables(S, widths):
    from epilogos_amd.scores import s1ScoreTable
    q = np.random.default_rng(S).random(S).astype(np.float32) + 0.05
    q /= q.sum()
    return {w: torch.from_numpy(s1ScoreTable(q, w)[1]).cuda() for w in set(widths)}


def _run(eng, way, name, ga, gb, seed):
    """-> (got, want) pairs of host arrays that must be equal."""
    NA, NB, S = CASES[name][:3]
    hA, hB, xa, xb, key0 = _inputs(name)
    oA, oB, _info = _reference(name, ga, gb, seed)
    if way in ("hist", "seq"):
        eng._abi.call("epg_test_force", 0, 1 if way == "seq" else 0)
        try:
            OA, OB = eng.null_hist_from_binhist(_dev(hA), _dev(hB), NA + NB, S, ga, gb, seed, key0)
        finally:
            eng._abi.call("epg_test_force", 0, 0)
        return [(eng.hist_to_numpy(OA), oA), (eng.hist_to_numpy(OB), oB)]
    if way == "fused":
        assert (ga, gb) == (NA, NB)
        HAs, HBs, OAs, OBs = eng.pair_count_null_parts([eng.states_to_device(xa)], [eng.states_to_device(xb)], NA, NB, S, seed, [key0])
        return [(eng.hist_to_numpy(HAs[0]), hA), (eng.hist_to_numpy(HBs[0]), hB), (eng.hist_to_numpy(OAs[0]), oA), (eng.hist_to_numpy(OBs[0]), oB)]
    assert way == "draws"
    T = _tables(S, (ga, gb))
    got = eng.null_dist_draws_parts([_dev(hA)], [_dev(hB)], [key0], S, NA, NB, ga, gb, T[ga], T[gb], [seed])
    # the null distance is a function of the null groups and their tables alone: score the reference's groups as both pairs
    RA, RB = _dev(oA), _dev(oB)
    want = eng.pair_scores_s1_parts([(RA, RB, RA, RB)], S, ga, gb, ga, gb, T[ga], T[gb], T[ga], T[gb])[0]["null"]
    assert tuple(got[0].shape) == (1, hA.shape[0])
    return [(got[0][0].cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))]


PARAMS = [(name, ga, gb, seed, way) for name, (_na, _nb, _s, sizes, seeds) in CASES.items() for ga, gb, ways in sizes for seed in seeds
          for way in ways.split()]


@pytest.mark.parametrize("name,ga,gb,seed,way", PARAMS, ids=["%s-%d+%d-%x-%s" % p for p in PARAMS])
def test_sampler_equals_reference(eng, name, ga, gb, seed, way):
    for k, (got, want) in enumerate(_run(eng, way, name, ga, gb, seed)):
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, "output %d: %d rows differ, first %s" % (k, bad.size, bad[:8])


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_tie_case_reaches_every_tie_path(seed):
    """A condition on the INPUTS, from the reference alone: the tie case holds ties at the A threshold and (-g) at the A-or-B
    threshold, in full calls of eight draws and in the last 1 .. 7 draws of a row."""
    NA, NB, _S, sizes, _seeds = CASES["ties"]
    info = _reference("ties", NA, NB, seed)[2]
    assert info["ties_A"] >= 20 and info["tail_A"] >= 3 and info["full_A"] >= 3 and info["ties_AB"] == 0
    info = _reference("ties", sizes[1][0], sizes[1][1], seed)[2]
    assert info["ties_A"] >= 20 and info["ties_AB"] >= 20
    assert min(info["tail_A"], info["tail_AB"], info["full_A"], info["full_AB"]) >= 3


@pytest.mark.parametrize("name", ["edge32", "edge64"])
def test_edge_cases_reach_the_equality_edge(name):
    """A condition on the INPUTS, from the reference alone: (v + 1) rem == need << 16 occurs in the edge cases' draws, at the A
    threshold and (-g) at the A-or-B threshold."""
    _NA, _NB, _S, sizes, seeds = CASES[name]
    default, g = ([_reference(name, ga, gb, seed)[2] for seed in seeds] for ga, gb, _ways in sizes)
    assert sum(i["edge_A"] for i in default) >= 3
    assert sum(i["edge_A"] for i in g) >= 1 and sum(i["edge_AB"] for i in g) >= 1


# ------------------------------------------------------------------------------------------------ the matrix-scanning kernel
def _junk_states(rng, R, N, S):
    """States with bytes that are none: -1, S and 127."""
    x = ref._states(rng, R, N, S)
    junk = rng.random((R, N))
    x[junk < 0.05] = -1
    x[(junk >= 0.05) & (junk < 0.07)] = S
    x[(junk >= 0.07) & (junk < 0.08)] = 127
    return x


@pytest.mark.parametrize("R", [130, 257])
@pytest.mark.parametrize("g", [None, 20])
@pytest.mark.parametrize("pitch", ["packed", "padded"])
@pytest.mark.parametrize("NA,NB", [(37, 29), (379, 342)])
def test_null_hist_equals_matrix_reference(eng, NA, NB, pitch, g, R):
    S, row0 = S18, ref.KEYS[0]
    rng = np.random.default_rng([NA, NB, R])
    xa, xb = _junk_states(rng, R, NA, S), _junk_states(rng, R, NB, S)
    ga, gb = (NA, NB) if g is None else (g, g)
    up = (lambda x: torch.from_numpy(x).cuda()) if pitch == "packed" else eng.states_to_device
    XA, XB = up(xa), up(xb)
    assert (XA.stride(0) == NA) == (pitch == "packed")
    for seed in ref.SEEDS:
        wantA, wantB = ref.sample_from_matrix(xa, xb, S, ga, gb, seed, row0)
        HA, HB = eng.null_hist(XA, NA, XB, NB, S, ga, gb, seed, row0)
        assert np.array_equal(eng.hist_to_numpy(HA), wantA) and np.array_equal(eng.hist_to_numpy(HB), wantB), seed
