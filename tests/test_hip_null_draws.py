"""The paired-mode null-group draws, pinned bit for bit.

tests/test_hip_s3_null.py checks the sampler's law, its determinism and that its kernels agree with one another; none of that
says WHICH groups a seed gives.  Paired outputs must not depend on the library version, the GPU count, the batch shape or the
kernel a width selects, so tests/golden/null_draws.json records a SHA-256 of what epg_null_hist_from_binhist_parts and
epg_pair_count_null_parts return for a fixed list of cases (tests/golden/make_golden_null_draws.py wrote it), and this test
recomputes them.  The cases reach every sampler and every way into it: row widths at the word boundaries of the bit strings, at
their 3072-column limit and beyond it, models of 5 .. 40 states, default group sizes and -g, the column-by-column kernel forced,
rows of one state, rows with columns that hold no state, tiles that are not full, several parts with an empty one among them and
keys of their own, more parts than one launch takes, two seeds."""
import hashlib
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
FIXTURE = GOLDEN / "null_draws.json"
SEEDS = (77, 0x9E3779B97F4A7C15)
KEYS = (123456789012, 5, 40000000)             # row0 of the three parts (the second one is empty)

# histogram path: (NA, NB, S, rows of the parts); every entry runs with the default group sizes and with -g, with the library's
# own choice of kernel and with the column-by-column kernel forced, under both seeds
WIDTHS = ((16, 16), (17, 16), (379, 342), (1500, 1572), (1600, 1600), (3000, 3001), (2000, 1200))
HIST_CASES = [(na, nb, 18, (20011, 0, 71) if (na, nb) == (379, 342) else (130, 0, 71)) for na, nb in WIDTHS]
HIST_CASES += [(na, nb, s, (130, 0, 71)) for s in (5, 15, 25, 40) for na, nb in ((17, 16), (379, 342))]
HIST_CASES += [(379, 342, 18, (9,) * 50)]      # more parts than one launch takes
# fused count + draw: its own shapes only (one and four 128-byte groups per row for every S, the flagship's three)
FUSED_CASES = [(na, nb, s, (130, 0, 71)) for s in (15, 18, 25) for na, nb in ((100, 120), (400, 500))]
FUSED_CASES += [(379, 342, 18, (20011, 0, 71)), (379, 342, 18, (70,) * 40)]
FUSED_REFUSED = (100, 300, 18)                 # one and three groups per row: not the fused kernel's


def _states(rng, R, N, S):
    """[R, N] int8 states, one dominant state as in real data; row 3 is all one state, row 5 has columns without a state."""
    p = 1.0 / (1.0 + np.arange(S)[::-1]) ** 2
    x = np.searchsorted(np.cumsum(p / p.sum()), rng.random((R, N))).clip(0, S - 1).astype(np.int8)
    if R > 5:
        x[3, :] = 1
        x[5, ::3] = -1
    return x


def _hist(x, S):
    h = np.zeros((x.shape[0], S), dtype=np.uint16)
    for s in range(S):
        h[:, s] = (x == s).sum(axis=1)
    return h


def _parts(na, nb, S, rows):
    rng = np.random.default_rng([na, nb, S, len(rows)])
    return [(_states(rng, r, na, S), _states(rng, r, nb, S)) for r in rows]


def _keys(rows):
    return [KEYS[i] if len(rows) == len(KEYS) else 1000 * i for i in range(len(rows))]


def _rows_label(rows):
    return "+".join(map(str, rows)) if len(rows) <= 3 else "%dx%d" % (len(rows), rows[0])


def _digest(groups):
    h = hashlib.sha256()
    for ts in groups:
        for t in ts:
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def compute_digests(eng):
    """case description -> SHA-256 of the outputs, parts in order."""
    out = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
    for na, nb, S, rows in HIST_CASES:
        parts = _parts(na, nb, S, rows)
        HAs, HBs = [dev(_hist(a, S)) for a, _b in parts], [dev(_hist(b, S)) for _a, b in parts]
        g = 6 if na + nb < 100 else 100
        for ga, gb in ((na, nb), (g, g)):
            for force in (0, 1):
                for seed in SEEDS:
                    eng._abi.call("epg_test_force", 0, force)
                    try:
                        OAs, OBs = eng.null_hist_from_binhist_parts(HAs, HBs, na + nb, S, ga, gb, seed, _keys(rows))
                    finally:
                        eng._abi.call("epg_test_force", 0, 0)
                    out["hist NA=%d NB=%d S=%d rows=%s ga=%d gb=%d force_seq=%d seed=%d" % (
                        na, nb, S, _rows_label(rows), ga, gb, force, seed)] = _digest((OAs, OBs))
    for na, nb, S, rows in FUSED_CASES:
        parts = _parts(na, nb, S, rows)
        XAs, XBs = [eng.states_to_device(a) for a, _b in parts], [eng.states_to_device(b) for _a, b in parts]
        for seed in SEEDS:
            counts = eng.zeros_counts(S)
            HAs, HBs, OAs, OBs = eng.pair_count_null_parts(XAs, XBs, na, nb, S, seed, _keys(rows), counts=counts)
            out["fused NA=%d NB=%d S=%d rows=%s seed=%d" % (na, nb, S, _rows_label(rows), seed)] = _digest((HAs, HBs, [counts], OAs, OBs))
    return out


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


def test_null_draws_are_the_recorded_ones(eng):
    want = json.loads(FIXTURE.read_text())["digests"]
    got = compute_digests(eng)
    assert sorted(got) == sorted(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, wrong


def test_fused_call_refuses_other_shapes(eng):
    na, nb, S = FUSED_REFUSED
    rng = np.random.default_rng(1)
    XA, XB = eng.states_to_device(_states(rng, 70, na, S)), eng.states_to_device(_states(rng, 70, nb, S))
    with pytest.raises(eng._abi.EpilogosHipError) as e:
        eng.pair_count_null_parts([XA], [XB], na, nb, S, SEEDS[0], [0])
    assert e.value.code == -2 and "pair_count_null: S=18, widths 100 + 300 are not the fused kernel's" in str(e.value)
