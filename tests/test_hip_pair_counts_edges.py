"""GPU: the S2 pair counts that epg_bin_hist_s2 folds into the count pass (k_bin_hist_s2), at their edges.

A wave re-packs the 32 staged histogram rows of a super-tile as 16 words of bin PAIRS per state, a lane owns one 3 x 3 block of state
pairs (a "role") and every PSLICE-th pair word, and the block's lanes meet in an LDS copy of the S x S matrix.  The cases walk
  * the three compile-time models: 15, 18 and 25 states = 15, 21 and 45 roles, so 4, 3 and 1 lanes per role (25: two padded state rows);
  * rows of one column, of one 128-byte group plus a byte, and of the widest fused shape (eight groups);
  * one bin, a ragged half-empty super-tile with an odd row count, and a second super-tile of one row (a pair word whose upper half,
    and pair words that are entirely, past the last row must not be multiplied);
  * on the one-CU grid of tests/grid_cap.py a row count that gives every wave three super-tiles and more, the last one ragged with an
    odd row count: the per-lane 64-bit sums carried from tile to tile.
Everything is exact: counts2 must equal h.T @ h - diag(h.sum(0)) of the ORACLE's histograms (expected.py:146-158) after one call and
twice that after a second call into the same array."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as onp
from tests.grid_cap import cdiv, count_grid, one_cu, tiles_of_waves

pytestmark = pytest.mark.gpu

R_CAPPED = 24 * 32 + 13


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def states():
    """(S, N, R) -> (x, oracle histograms, pair counts), computed once and shared"""
    made = {}

    def get(S, N, R):
        if (S, N, R) not in made:
            x = np.random.default_rng([S, N, R]).integers(0, S, size=(R, N)).astype(np.int8)
            if R * N > 3:
                x[R // 2, N // 2] = -1                                   # a byte that is no state
            x[R - 1, N - 1] = S - 1                                      # the last state in the last byte of the last row
            h = onp.bin_hist(x, S).astype(np.int64)
            for a in (x, h):
                a.setflags(write=False)
            made[S, N, R] = (x, h, h.T @ h - np.diag(h.sum(axis=0)))
        return made[S, N, R]
    return get


def _check(eng, states, S, N, R):
    x, h, want = states(S, N, R)
    X = eng.states_to_device(x)
    c1, c2 = eng.zeros_counts(S), eng.zeros_counts(S * S)
    H, _ = eng.bin_hist_s2(X, N, S, counts2=c2, counts=c1)
    assert np.array_equal(eng.hist_to_numpy(H), h.astype(np.uint16))
    assert np.array_equal(c1.cpu().numpy(), h.sum(axis=0))
    assert np.array_equal(c2.cpu().numpy().reshape(S, S), want), (S, N, R)
    eng.bin_hist_s2(X, N, S, counts2=c2, H=H)                            # the same array again: it accumulates
    assert np.array_equal(c2.cpu().numpy().reshape(S, S), 2 * want), (S, N, R)


@pytest.mark.parametrize("R", [1, 31, 33])
@pytest.mark.parametrize("N", [1, 129, 1024])
@pytest.mark.parametrize("S", [15, 18, 25])
def test_fused_pair_counts_at_the_edges(eng, states, S, N, R):
    _check(eng, states, S, N, R)


@pytest.mark.parametrize("N", [1, 129, 1024])
@pytest.mark.parametrize("S", [15, 18, 25])
def test_fused_pair_counts_over_several_super_tiles(eng, states, S, N):
    R = R_CAPPED
    blocks = count_grid(R, 1)
    few, _most = tiles_of_waves(cdiv(R, 32), blocks * 4)
    assert blocks == 2 and few >= 3 and R % 32 == 13                     # every wave: three super-tiles or more; the last: 13 rows
    with one_cu(eng._abi):
        _check(eng, states, S, N, R)
