"""GPU: the count pass's two sources of state words -- the LDS-DMA stream (DmaHalfTile, csrc/epg_count.h; the default for the
15-, 18- and 25-state models on rows of up to 1024 columns) and the plain loads it replaces (epg_test_force(6, 1)).

Both must give the numpy oracle's histograms and state counts bit for bit, and each other's, at the smallest shapes where the
loader can go wrong:
  R     1, 15, 16, 17, 31, 32, 33, 95: a half tile of 16 rows and a super-tile of 32, one row less and one more (rows past R are
        asked for at X's first chunk instead), and 785 = 3 x 256 + 17 rows on the one-CU grid (tests/grid_cap.py): 8 waves, 25
        super-tiles, so every wave refills its slot for a second and a third tile and the last one is ragged;
  N     1, 16, 17, 127, 128, 129, 833, 1023, 1024: one chunk, a full and a started chunk, the group boundary (128 bytes), the
        flagship width (53 chunks: the last DMA instruction of a half tile is a partial one), the widest row and one byte less;
  ldx   the padded width (pad bytes -1, as engine.states_to_device leaves them) and 48 bytes more (pad bytes a VALID state: a
        loader that takes pad bytes for columns, or the next row's bytes for this one's, counts them);
  S     15, 18, 25;
  bytes random states, every byte the same state (the packed 16-bit counts at their largest), the last columns -1.
A case is one (S, N): its rows are drawn, uploaded and counted by the oracle once, and every R is the first R rows of them.
The arena cases (tests/abi_arena.py) put X so that its last byte is the last byte before a guard band of valid states."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as onp
from tests.abi_arena import Arena
from tests.grid_cap import cdiv, count_grid, forced, one_cu, tiles_of_waves

gpu = pytest.mark.gpu
FORCE_PLAIN_LOADS = 6
ROWS = (1, 15, 16, 17, 31, 32, 33, 95)
R_WRAP = 3 * 256 + 17
WIDTHS = (1, 16, 17, 127, 128, 129, 833, 1023, 1024)
MODELS = (15, 18, 25)
KINDS = ("random", "one state", "-1 columns")


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


def test_wrap_case_arithmetic():
    """R_WRAP on the one-CU grid: 2 workgroups = 8 waves, every wave three super-tiles or four, the last super-tile ragged."""
    assert count_grid(R_WRAP, 1) == 2
    few, most = tiles_of_waves(cdiv(R_WRAP, 32), 2 * 4)
    assert few >= 3 and most > few and R_WRAP % 32 not in (0, 16)
    assert all(count_grid(r, 256) * 4 * 32 >= r for r in ROWS)           # the device's grid: one super-tile per wave


def states(kind, R, N, S, seed):
    rng = np.random.default_rng([seed, R, N, S])
    if kind == "one state":
        return np.full((R, N), S - 1, dtype=np.int8)
    x = rng.integers(0, S, size=(R, N)).astype(np.int8)
    if kind == "-1 columns":
        x[:, N - max(N // 5, 1):] = -1
    return x


def device_matrix(x, ldx, pad):
    host = np.full((x.shape[0], ldx), pad, dtype=np.int8)
    host[:, :x.shape[1]] = x
    return torch.from_numpy(host).cuda()


def both_loaders(eng, X, R, N, S):
    """-> (H, counts) of the first R rows of X; asserts that the two loaders agree."""
    got = []
    for plain in (0, 1):
        with forced(eng._abi, FORCE_PLAIN_LOADS, plain):
            H, c = eng.bin_hist(X[:R], N, S)
            got.append((eng.hist_to_numpy(H), c.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), "DMA and plain loads differ"
    return got[0]


@gpu
@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("S", MODELS)
def test_count_dma_equals_oracle_and_plain_loads(eng, S, N):
    padded = eng.padded_width(N)
    for kind in KINDS:
        x = states(kind, R_WRAP, N, S, 7)
        want = onp.bin_hist(x, S).astype(np.uint16)
        for ldx, pad in ((padded, -1), (padded + 48, 1)):
            X = device_matrix(x, ldx, pad)
            assert X.data_ptr() % 16 == 0 and X.stride(0) == ldx and ldx % 16 == 0      # what the DMA loads are taken for
            for R in ROWS + (R_WRAP,):
                H, c = both_loaders(eng, X, R, N, S)
                assert np.array_equal(H, want[:R]), (kind, ldx, R)
                assert np.array_equal(c, want[:R].sum(axis=0, dtype=np.int64)), (kind, ldx, R)
            with one_cu(eng._abi):                                                       # second and third tiles: the slot is refilled
                H, c = both_loaders(eng, X, R_WRAP, N, S)
            assert np.array_equal(H, want), (kind, ldx, "one CU")
            assert np.array_equal(c, want.sum(axis=0, dtype=np.int64)), (kind, ldx, "one CU")


@gpu
@pytest.mark.parametrize("S,N,ldx,R", [(18, 833, 848, 95), (25, 1024, 1024, 33), (15, 17, 32, 785)])
def test_count_dma_stays_inside_x(eng, S, N, ldx, R):
    """X ends exactly where a guard band of valid states begins (and starts behind one): a request past either end that is
    counted shows in H or in the counts; a write outside H and the counts shows in the arena."""
    x = states("random", R, N, S, 11)
    host = np.full((R, ldx), 2, dtype=np.int8)
    host[:, :N] = x
    want = onp.bin_hist(x, S).astype(np.uint16)
    arena = Arena("cuda", guard_byte=1)
    arena.add("X", R * ldx, role="in")
    arena.add("H", R * S * 2, role="out", align=16)
    arena.add("counts", S * 8, role="out", align=8)
    arena.build()
    for plain in (0, 1):
        arena.reset()
        arena.write("X", host)
        arena.fill("H", 0xFF)
        arena.fill("counts", 0)
        arena.snapshot()
        with forced(eng._abi, FORCE_PLAIN_LOADS, plain), one_cu(eng._abi):
            eng._abi.call("epg_bin_hist", arena.ptr("X"), R, N, ldx, S, arena.ptr("H"), arena.ptr("counts"), eng._stream())
            torch.cuda.synchronize()
        arena.check()
        assert np.array_equal(arena.read("H", np.uint16).reshape(R, S), want), plain
        assert np.array_equal(arena.read("counts", np.int64), want.sum(axis=0, dtype=np.int64)), plain
