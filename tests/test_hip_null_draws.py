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

from tests.null_sampler_ref import (FIXTURE, FUSED_CASES, FUSED_REFUSED, HIST_CASES, KEYS, SEEDS, WIDTHS, _hist, _keys, _parts,  # noqa: F401
                                    _rows_label, _states, fused_label, hist_group_sizes, hist_label)

pytestmark = pytest.mark.gpu


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
        for ga, gb in hist_group_sizes(na, nb):
            for force in (0, 1):
                for seed in SEEDS:
                    eng._abi.call("epg_test_force", 0, force)
                    try:
                        OAs, OBs = eng.null_hist_from_binhist_parts(HAs, HBs, na + nb, S, ga, gb, seed, _keys(rows))
                    finally:
                        eng._abi.call("epg_test_force", 0, 0)
                    out[hist_label(na, nb, S, rows, ga, gb, force, seed)] = _digest((OAs, OBs))
    for na, nb, S, rows in FUSED_CASES:
        parts = _parts(na, nb, S, rows)
        XAs, XBs = [eng.states_to_device(a) for a, _b in parts], [eng.states_to_device(b) for _a, b in parts]
        for seed in SEEDS:
            counts = eng.zeros_counts(S)
            HAs, HBs, OAs, OBs = eng.pair_count_null_parts(XAs, XBs, na, nb, S, seed, _keys(rows), counts=counts)
            out[fused_label(na, nb, S, rows, seed)] = _digest((HAs, HBs, [counts], OAs, OBs))
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
