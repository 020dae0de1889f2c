"""The kernels of `simsearch -b --step1 gpu` (include/epilogos_simsearch_pick.h) against tests/simsearch_pick_ref.py, exact equality
everywhere: the centre scores, the rolling maximum, the rank and the pick at the smallest shapes where they can go wrong (around the
window, around the pick tile T, several tiles), and one call of each inside the guarded arena of tests/abi_arena.py.  No grid of
these kernels is sized by the compute-unit count, so there is no one-CU case.  Two loops take a second turn only beyond those shapes and
have cases of their own: k_compact_offsets beyond 256 tiles, the halo load of k_pick_sweep beyond W = 257."""
import ctypes

import numpy as np
import pytest

from epilogos_amd import _abi
from tests import simsearch_pick_ref as ref
from tests.abi_arena import Arena

pytestmark = pytest.mark.gpu
T = _abi.header_constant("simsearch_pick", "EPG_PICK_TILE")
WINDOWS = [1, 2, 5, 24, 25, 124, 125]


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset) if t.numel() else None


def _stream():
    from epilogos_amd import engine
    return engine._stream()


def _ws(nbytes):
    import torch
    assert nbytes >= 0
    return torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")


# ---- rowscore ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 3, 15, 18, 25, 100])
def test_rowscore_is_the_left_to_right_float_sum(S):
    import torch
    rng = np.random.default_rng(S)
    for R in (1, 63, 64, 65, 1000):
        x = rng.integers(-300000, 900000, size=(R, S)).astype(np.int32)
        x[rng.random((R, S)) < 0.3] = 0
        edge = rng.random((R, S)) < 0.1                          # values near +-2^31 / 1e5
        x[edge] = np.where(rng.random(int(edge.sum())) < 0.5, 2 ** 31 - 1 - rng.integers(0, 50, int(edge.sum())),
                           -2 ** 31 + rng.integers(0, 50, int(edge.sum()))).astype(np.int32)
        x[0, 0], x[-1, -1] = 2 ** 31 - 1, -2 ** 31
        out = torch.full((R + 2,), -7.0, dtype=torch.float64, device="cuda")
        xd = _cuda(x)                                            # (held: a temporary's memory would be handed out again)
        _abi.call("epg_simsearch_rowscore", _ptr(xd), R, S, _ptr(out, 8), _stream())
        got = out.cpu().numpy()
        assert got[0] == -7.0 and got[-1] == -7.0, "wrote outside its output"
        want = ref.row_scores(x)
        assert got[1:-1].tobytes() == want.tobytes(), (R, S)


# ---- rolling max ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINDOWS)
def test_rolling_max_is_pandas(W):
    import torch
    from epilogos_amd import _io
    rng = np.random.default_rng(W)
    for n in sorted({W - 1, W, W + 1, 1000, 4099} - {0}):
        v = np.round(rng.normal(size=n), 1)                      # rounded: equal maxima inside a window are the rule
        v[n // 3:n // 3 + 2 * W] = -1.5
        out = torch.full((n + 2,), -7.0, dtype=torch.float64, device="cuda")
        vd = _cuda(v)
        _abi.call("epg_simsearch_rolling_max", _ptr(vd), n, W, _ptr(out, 8), _stream())
        got = out.cpu().numpy()
        assert got[0] == -7.0 and got[-1] == -7.0, "wrote outside its output"
        want = _io.rolling_max(v, W)
        assert np.array_equal(np.isnan(got[1:-1]), np.isnan(want)), (W, n)
        assert np.array_equal(got[1:-1], want, equal_nan=True), (W, n)
        assert np.array_equal(want, ref.rolling_max(v, W), equal_nan=True)


# ---- rank ----------------------------------------------------------------------------------------------------------------------

def _rank(rmax, rmean, score):
    import torch
    n = len(rmax)
    rank = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    ws = _ws(_abi.call("epg_simsearch_rank_ws_bytes", n))
    keys = [_cuda(rmax), _cuda(rmean), _cuda(score)]
    _abi.call("epg_simsearch_rank", _ptr(keys[0]), _ptr(keys[1]), _ptr(keys[2]), n, _ptr(rank, 4), _ptr(ws), ws.numel(), _stream())
    got = rank.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7, "wrote outside its output"
    return got[1:-1].astype(np.int64)


KEYS = ["distinct", "ties_max", "ties_max_mean", "ties_all", "zeros", "negative"]


@pytest.mark.parametrize("kind", KEYS)
def test_rank_is_the_lexsort(kind):
    rng = np.random.default_rng(KEYS.index(kind))
    for n in (1, 2, 255, 256, 257, 70001):
        few = lambda k: rng.integers(-k, k + 1, size=n) / 8.0                # noqa: E731 -- a few values: massive ties
        rmax, rmean, score = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
        if kind == "ties_max":
            rmax = few(2)                                        # equal maxima, different means
        elif kind == "ties_max_mean":
            rmax, rmean = few(1), few(2)
        elif kind == "ties_all":
            rmax, rmean, score = few(1), few(1), few(1)
        elif kind == "zeros":                                    # -0.0 beside +0.0 in every column: equal keys, index order
            rmax, rmean, score = few(1), few(1), few(2)
            for col in (rmax, rmean, score):
                col[(col == 0) & (rng.random(n) < 0.5)] = -0.0
            assert n < 255 or (np.signbit(rmax) & (rmax == 0)).any()
        elif kind == "negative":
            rmax, rmean, score = -np.abs(few(3)) - 1.0, -np.abs(rmean) * 1e-300, -np.abs(score) * 1e300
        want = ref.lexsort_rank(rmax, rmean, score)
        assert np.array_equal(_rank(rmax, rmean, score), want), (kind, n)


# ---- pick ----------------------------------------------------------------------------------------------------------------------

def _pick(rank, W, cap):
    """-> (picked positions, launches); the outputs sit between guard entries that must stay untouched."""
    import torch
    n = len(rank)
    room = -(-n // W)
    r = _cuda(np.asarray(rank).astype(np.uint32).view(np.int32))
    picked = torch.full((room + 2,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    launches = ctypes.c_int32(-7)
    ws = _ws(_abi.call("epg_simsearch_pick_ws_bytes", n, W))
    _abi.call("epg_simsearch_pick", _ptr(r), n, W, cap, _ptr(picked, 8), _ptr(count, 8), ctypes.byref(launches), _ptr(ws), ws.numel(),
              _stream())
    torch.cuda.synchronize()
    picked, count = picked.cpu().numpy(), count.cpu().numpy()
    assert picked[0] == -7 and count[0] == -7 and count[2] == -7, "wrote outside its outputs"
    k = int(count[1])
    assert 0 <= k <= room and (picked[1 + k:] == -7).all(), "entries behind n_picked were written"
    return picked[1:1 + k], launches.value


def _sizes(W):
    return sorted({1, W - 1, W, W + 1, T - 1, T, T + 1, 3 * T + 7} - {0})


@pytest.mark.parametrize("name", ref.PATTERNS)
@pytest.mark.parametrize("W", WINDOWS)
def test_pick_is_the_walk(W, name):
    for n in _sizes(W):
        rank = ref.pattern(name, n, W, T, seed=W)
        full = ref.pick(rank, W, n)
        for cap in sorted({1, 3, len(full), len(full) + 1, n}):
            got, launches = _pick(rank, W, cap)
            want = ref.pick(rank, W, cap)
            assert np.array_equal(got, want), (W, name, n, cap)                  # ascending, n_picked exact
            assert 1 <= launches <= -(-n // T) if name in ("identity", "reversed") else launches >= 1, (W, name, n, launches)


@pytest.mark.parametrize("W", WINDOWS)
def test_a_plateau_costs_a_sweep_per_tile_not_one_per_window(W):
    """Ranks by position over 3 T + 7 windows: the header's bound for monotone keys, ceil(n / T) sweeps; one launch per round of the
    rules would need n / W."""
    n = 3 * T + 7
    got, launches = _pick(np.arange(n), W, n)
    assert np.array_equal(got, np.arange(0, n, W))
    assert launches <= -(-n // T) == 4
    assert W > 125 or launches * 10 <= n // W


PK_THREADS = 256                                                 # epg_simsearch_pick.hip: the workgroup of the pick kernels


@pytest.mark.parametrize("n,W", [(PK_THREADS * T + 1, 125), (2 * PK_THREADS * T + T + 5, 25)])
def test_pick_with_more_tiles_than_the_offsets_workgroup_has_threads(n, W):
    """k_compact_offsets scans the tiles' counts in turns of 256 with a carry: 256 tiles and ONE position in the second turn; three
    turns, the last of two tiles, the very last ragged.  (A genome of 15 M bins is 29 turns.)"""
    tiles = -(-n // T)
    assert (-(-tiles // PK_THREADS), tiles - (-(-tiles // PK_THREADS) - 1) * PK_THREADS, n % T) == {125: (2, 1, 1), 25: (3, 2, 5)}[W]
    assert -(-(3 * T + 7) // T) <= PK_THREADS                    # the largest of the sizes above: one turn
    rank = ref.pattern("random", n, W, T, seed=W)
    rank[np.nonzero(rank == 0)[0][0]], rank[n - 1] = rank[n - 1], 0          # the best window is the last: the last tile holds a pick
    full = ref.pick(rank, W, n)
    assert full[-1] == n - 1 and full[0] < T
    got, launches = _pick(rank, W, n)
    assert np.array_equal(got, full) and launches >= 1
    cap = len(full) // 2                                          # ... and with the threshold on the ranks
    assert np.array_equal(_pick(rank, W, cap)[0], ref.pick(rank, W, cap))


@pytest.mark.parametrize("W", [300, 1024])
def test_pick_with_a_halo_wider_than_the_workgroup(W):
    """k_pick_sweep loads the two halos of W - 1 states with j += 256: a second turn beyond W = 257, four at the largest window."""
    assert -(-(W - 1) // PK_THREADS) == {300: 2, 1024: 4}[W] and max(WINDOWS) - 1 <= PK_THREADS
    assert W <= _abi.header_constant("simsearch_pick", "EPG_PICK_MAX_W")
    n = 3 * T + 7
    for name in ("random", "reversed", "saw_window", "best_last_of_tile"):
        rank = ref.pattern(name, n, W, T, seed=W)
        for cap in (3, n):
            got, _launches = _pick(rank, W, cap)
            assert np.array_equal(got, ref.pick(rank, W, cap)), (W, name, cap)


def test_pick_of_nothing():
    got, launches = _pick(np.zeros(0, dtype=np.int64), 25, 10)
    assert len(got) == 0 and launches == 0
    got, launches = _pick(np.arange(100), 25, 0)
    assert len(got) == 0 and launches == 0


# ---- contract: nothing outside the named outputs is written -------------------------------------------------------------------------

def test_entry_points_write_only_their_outputs():
    import torch
    rng = np.random.default_rng(5)
    R, S, W = 3000, 18, 25
    x = rng.integers(-50000, 300000, size=(R, S)).astype(np.int32)
    score = ref.row_scores(x)
    n = 2 * T + 77
    rmax, rmean, sc = np.round(rng.normal(size=n), 1), rng.normal(size=n), rng.normal(size=n)
    rank = ref.lexsort_rank(rmax, rmean, sc)
    room = -(-n // W)
    rank_ws, pick_ws = _abi.call("epg_simsearch_rank_ws_bytes", n), _abi.call("epg_simsearch_pick_ws_bytes", n, W)
    arena = Arena("cuda", guard_byte=1)
    arena.add("X", x.nbytes, role="in")
    arena.add("score", R * 8)
    arena.add("v", R * 8, role="in")
    arena.add("rollmax", R * 8)
    for name in ("rmax", "rmean", "sc"):
        arena.add(name, n * 8, role="in")
    arena.add("rank_out", n * 4)
    arena.add("rank_ws", rank_ws, role="ws")
    arena.add("rank_in", n * 4, role="in")
    arena.add("picked", room * 8)                                 # exactly ceil(n / W) entries
    arena.add("n_picked", 8)
    arena.add("pick_ws", pick_ws, role="ws")
    arena.build()
    arena.write("X", x), arena.write("v", score)
    arena.write("rmax", rmax), arena.write("rmean", rmean), arena.write("sc", sc)
    arena.write("rank_in", rank.astype(np.uint32))
    arena.snapshot()
    launches = ctypes.c_int32(0)
    st = _stream()
    _abi.call("epg_simsearch_rowscore", arena.ptr("X"), R, S, arena.ptr("score"), st)
    _abi.call("epg_simsearch_rolling_max", arena.ptr("v"), R, W, arena.ptr("rollmax"), st)
    _abi.call("epg_simsearch_rank", arena.ptr("rmax"), arena.ptr("rmean"), arena.ptr("sc"), n, arena.ptr("rank_out"), arena.ptr("rank_ws"),
              rank_ws, st)
    _abi.call("epg_simsearch_pick", arena.ptr("rank_in"), n, W, n, arena.ptr("picked"), arena.ptr("n_picked"), ctypes.byref(launches),
              arena.ptr("pick_ws"), pick_ws, st)
    torch.cuda.synchronize()
    arena.check()
    assert arena.read("score", np.float64).tobytes() == score.tobytes()
    from epilogos_amd import _io
    assert np.array_equal(arena.read("rollmax", np.float64), _io.rolling_max(score, W), equal_nan=True)
    assert np.array_equal(arena.read("rank_out", np.uint32), rank)
    want = ref.pick(rank, W, n)
    k = int(arena.read("n_picked", np.int64)[0])
    assert k == len(want) and np.array_equal(arena.read("picked", np.int64)[:k], want) and launches.value >= 1
