"""GPU: the persistent kernels' SECOND AND LATER tiles, at small shapes.

Almost every kernel of the library runs on a persistent grid of num_cus() x k workgroups: a wave walks tiles t, t + waves, ... and
carries state from one to the next -- packed 16-bit running counts with a mid-loop flush (K1, k_pair_count_null), tiles fetched
one iteration ahead (k_s2_hist_wave, k_score_s2_bin, k_pair_fused_s1, k_pair_count_null), a cursor through several parts, LDS
staging areas that are re-used with only wave barriers in between.  On 256 compute units a wave gets a second tile only beyond
65 000 - 524 000 rows, so at the shapes of the other oracle tests none of that runs.  epg_test_force(5, 1) (tests/grid_cap.py)
sizes every grid for ONE compute unit: a few thousand rows then give every wave three and more tiles.

Every case runs once on the one-CU grid and once on the device's, and asks
  * integer outputs to equal the numpy oracle (oracle/oracle_np.py, tests/null_sampler_ref.py) bit for bit,
  * float outputs to meet the tolerance that the entry point's existing test asserts against the float64 oracle,
  * the two runs to agree byte for byte,
and states its own arithmetic -- rows per sweep of the capped grid as the dispatch code computes it, hence tiles per wave (at
least three, the last one ragged) -- in plain asserts; test_case_arithmetic repeats those without a GPU.

The S3 score kernels (k_s3_score, k_s3_score_bl), the LDS-counter kernel k_s3_hist and the matrix-core contraction take one
slice or task per workgroup: their grids are slice counts, not CU multiples, and the switch does not change them.  Their cases here
span several slices with a ragged last one and put the grid-stride helpers around them (finish, table build, reconstruct, one-hot
operand) on the one-CU grid."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as onp
from tests import null_sampler_ref as ref
from tests.grid_cap import (cdiv, capped_and_not, count_grid, flush_every, forced, null_draws_waves, pair_count_null_waves, pair_fused_waves, part_tiles,
                            s1_from_hist_stride, tile_rows, tiles_of_waves)

gpu = pytest.mark.gpu
U16, I64, F32 = np.uint16, np.int64, np.float32


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


def _np(t):
    return t.cpu().numpy()


def _dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16)).cuda()


# ----------------------------------------------------------------------------------------------------------------------------
# count pass: the mid-loop flush
# ----------------------------------------------------------------------------------------------------------------------------
# (S, N, R, flush_every).  Under the cap: 2 workgroups = 8 waves = 256 rows per sweep.
COUNT_CASES = [(18, 833, 10240 + 17, 77), (25, 1024, 8192 + 5, 62), (15, 4097, 2048 + 33, 14), (31, 2500, 16 * 256 + 9, 25), (7, 2500, 16 * 256 + 9, 25)]
ONE_STATE_CASES = [(18, 21845, 3 * 256 + 1, 2), (18, 21846, 3 * 256 + 1, 1), (15, 32767, 3 * 256 + 1, 1), (25, 65535, 3 * 256 + 1, 1)]


def _count_arith(S, N, R, fe):
    assert fe == flush_every(N)
    blocks = count_grid(R, 1)
    assert blocks == 2 and blocks * 4 * 32 == 256                         # rows per sweep
    few, most = tiles_of_waves(cdiv(R, 32), blocks * 4)
    assert few >= 3 and R % 32 != 0                                       # every wave: three tiles and more; the last tile is ragged
    assert 2 * few > fe                                                   # two epilogues per tile: every wave flushes inside its loop
    # a lane whose rows all hold one state adds N per epilogue: with a flush interval twice as long, or none, a half overflows
    assert fe * N <= 65535
    if fe > 1 or 2 * N > 65535:
        assert min(2 * fe, 2 * few) * N > 65535
    assert count_grid(R, 256) * 4 * 32 >= R                               # the device's grid: one tile per wave, what the other tests run


def _lane_state(S, b):
    return (S - 1 - b) % S


def flush_rows(R, N, S, seed):
    """A quad lane b of a wave counts the rows with row % 16 == b, tile after tile.  b < 8: rows of ONE state (that lane's packed
    half reaches flush_every x N); b = 8: two states alternating along the row; b = 9: two states alternating from row to row;
    b = 10: bytes that are no state; the rest: random states."""
    rng = np.random.default_rng([seed, R, N, S])
    x = rng.integers(0, S, size=(R, N)).astype(np.int8)
    b = np.arange(R) % 16
    for k in range(8):
        x[b == k] = _lane_state(S, k)
    x[b == 8, 0::2], x[b == 8, 1::2] = 0, S - 1
    x[b == 9] = np.where((np.arange(R)[b == 9] // 16) % 2, 1, S - 2).astype(np.int8)[:, None]
    x[b == 10] = -1
    if S < 31:
        x[b == 10, ::3] = S
    return x


def one_state_rows(R, N, S):
    return np.repeat(np.array([_lane_state(S, r % 16) for r in range(R)], dtype=np.int8)[:, None], N, axis=1)


def _pair_counts(h):
    h = h.astype(I64)
    return h.T @ h - np.diag(h.sum(axis=0))


def _count_run(eng, x, S, N, want_h, packed):
    R = x.shape[0]
    X = torch.from_numpy(np.ascontiguousarray(x)).cuda() if packed else eng.states_to_device(x)
    assert X.stride(0) == (N if packed else eng.padded_width(N))
    abi = eng._abi

    def fn():
        out = {}
        H, c = eng.bin_hist(X, N, S)
        out["H"], out["counts"] = eng.hist_to_numpy(H), _np(c)
        c1 = eng.zeros_counts(S)
        abi.call("epg_hist_s1", eng._ptr(X), R, N, X.stride(0), S, eng._ptr(c1), eng._stream())     # counts only
        out["counts alone"] = _np(c1)
        H1, _ = eng.bin_hist(X, N, S, want_counts=False)                                             # H only
        out["H alone"] = eng.hist_to_numpy(H1)
        cs = eng.zeros_counts(S)
        H2, c2 = eng.bin_hist_s2(X, N, S, counts=cs)                      # (one launch for 15 / 18 / 25 states and N <= 1024)
        out["H s2"], out["counts s2"], out["counts2"] = eng.hist_to_numpy(H2), _np(cs), _np(c2).reshape(S, S)
        return out

    o = capped_and_not(abi, fn)
    for name in ("H", "H alone", "H s2"):
        assert np.array_equal(o[name], want_h), name
    for name in ("counts", "counts alone", "counts s2"):
        assert np.array_equal(o[name], want_h.sum(axis=0, dtype=I64)), name
    assert np.array_equal(o["counts2"], _pair_counts(want_h))


@gpu
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("S,N,R,fe", COUNT_CASES)
def test_count_pass_flushes_inside_the_loop(eng, S, N, R, fe, packed):
    _count_arith(S, N, R, fe)
    x = flush_rows(R, N, S, 1)
    _count_run(eng, x, S, N, onp.bin_hist(x, S).astype(U16), packed)


@gpu
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("S,N,R,fe", ONE_STATE_CASES)
def test_count_pass_one_bin_fills_a_half(eng, S, N, R, fe, packed):
    """flush_every steps 2 -> 1 between N = 21845 and 21846; at 65535 a single bin fills a 16-bit half."""
    _count_arith(S, N, R, fe)
    x = one_state_rows(R, N, S)
    want = np.zeros((R, S), dtype=U16)
    want[np.arange(R), x[:, 0]] = N
    assert np.array_equal(onp.bin_hist(x[:40], S), want[:40])
    _count_run(eng, x, S, N, want, packed)


# ----------------------------------------------------------------------------------------------------------------------------
# several parts in one launch
# ----------------------------------------------------------------------------------------------------------------------------
PART_ROWS = (40 * 256 + 5, 1, 0, 31, 33, 3 * 256, 700)
# name -> (S, rows, widths, parts whose rows are those of flush_rows).  A launch takes the parts of one load-schedule class
# (128-byte groups per row, 1 .. 8; wider: the any-width loop); nmax = the widest part of the launch.
PARTS_CASES = {
    # one class (seven groups per row): every wave crosses every part boundary; the widest part is the sixth
    "one-class": (18, PART_ROWS, (800, 770, 833, 880, 769, 896, 790), (0, 6)),
    # the parts back to front, eight groups per row: a narrow part comes first, the long part is the widest and the last, every part holds
    # one-state rows.  THE case that tells a flush interval taken from the first part's width (72 epilogues at 897 columns, 62 at 1024) from
    # the right one: _parts_arith walks a wave through the launch with either interval
    "one-class-reversed": (18, PART_ROWS[::-1], (897, 1000, 900, 960, 940, 920, 1024), (0, 1, 2, 3, 5, 6)),
    # across classes: 7 groups, 1, 3, any width, 2, any width, 3; the any-width launch holds a narrow and a wide part of one-state rows
    "classes": (15, PART_ROWS, (833, 40, 379, 1100, 129, 4097, 342), (0, 3, 5)),
    "classes-25": (25, PART_ROWS, (1000, 1025, 16, 1024, 2500, 130, 897), (0, 4)),
}


def _cls(n):
    return cdiv(n, 128) if cdiv(n, 128) <= 8 else 0


def _fullest_half(parts, waves, fe):
    """The largest value a 16-bit half reaches in a launch of `parts` = [(rows, width, one-state rows?)] when the packed counts are
    flushed every `fe` epilogues: a wave takes the super-tiles w, w + waves, ... of the parts in order, a super-tile is two epilogues,
    and an epilogue adds the part's width in a lane of one-state rows (counted for whole super-tiles of such parts only)."""
    tiles = [n if one and 32 * (t + 1) <= r else 0 for r, n, one in parts for t in range(cdiv(r, 32))]
    worst = 0
    for w in range(waves):
        half = since = 0
        for add in tiles[w::waves]:
            for _ in range(2):
                half += add
                worst = max(worst, half)
                since += 1
                if since >= fe:
                    half = since = 0
    return worst


def _parts_arith(S, rows, widths, marked):
    assert sorted(rows) == sorted(PART_ROWS) and len(widths) == len(rows)
    launches = {}
    for k, (r, n) in enumerate(zip(rows, widths)):
        if r:
            launches.setdefault(_cls(n), []).append((r, n, k in marked))
    for parts in launches.values():                                       # with the launch's own interval nothing overflows ...
        nmax = max(n for _r, n, _o in parts)
        assert _fullest_half(parts, 8, flush_every(nmax)) <= 65535
        if any(r == max(rows) and one for r, _n, one in parts):           # ... twice the interval does, in the launch of the long part
            assert _fullest_half(parts, 8, 2 * flush_every(nmax)) > 65535
    if len(launches) == 1 and rows[-1] == max(rows):                      # (one-class-reversed) ... and so does the first part's interval
        parts = launches[_cls(widths[0])]
        assert parts[-1][1] == max(n for _r, n, _o in parts) > parts[0][1]
        assert _fullest_half(parts, 8, flush_every(parts[0][1])) > 1.1 * 65535
    launches = {c: [(r, n) for r, n, _o in parts] for c, parts in launches.items()}
    big = max(rows)
    for c, parts in launches.items():
        nsuper = part_tiles([r for r, _n in parts], 32)
        blocks = count_grid(nsuper * 32, 1)
        assert blocks <= 2                                                # at most 256 rows per sweep
        if any(r == big for r, _n in parts):
            few, _most = tiles_of_waves(nsuper, blocks * 4)
            assert blocks == 2 and few >= 3 and any(r % 32 for r, _n in parts)
            nmax = max(n for _r, n in parts)
            assert 2 * (big // 256) > flush_every(nmax)                   # the long part alone: a flush inside the loop
            if len(parts) > 1:
                assert parts[0][1] != nmax                                # the widest part is not the first


@gpu
@pytest.mark.parametrize("name", list(PARTS_CASES))
def test_count_pass_over_several_parts(eng, name):
    S, rows, widths, marked = PARTS_CASES[name]
    _parts_arith(S, rows, widths, marked)
    rng = np.random.default_rng(len(name))
    xs = [flush_rows(r, n, S, k) if k in marked else rng.integers(0, S, size=(r, n)).astype(np.int8) for k, (r, n) in enumerate(zip(rows, widths))]
    for x in xs:
        if x.shape[0] > 40:
            x[37, ::5] = -1
    # pitches: padded, packed and padded + 3
    Xs = []
    for k, x in enumerate(xs):
        if k % 3 == 1:
            Xs.append(torch.from_numpy(np.ascontiguousarray(x)).cuda())
        else:
            host = np.full((x.shape[0], eng.padded_width(x.shape[1]) + (3 if k % 3 == 2 else 0)), -1, dtype=np.int8)
            host[:, :x.shape[1]] = x
            Xs.append(torch.from_numpy(host).cuda())
    hs = [onp.bin_hist(x, S).astype(U16) for x in xs]

    def fn():
        counts = eng.zeros_counts(S)
        Hs, _ = eng.bin_hist_parts(Xs, list(widths), S, counts=counts)
        out = {"H%d" % k: eng.hist_to_numpy(H) for k, H in enumerate(Hs)}
        out["counts"] = _np(counts)
        c1 = eng.zeros_counts(S)
        eng.bin_hist_parts(Xs, list(widths), S, counts=c1, want_hist=False)
        out["counts alone"] = _np(c1)
        return out

    o = capped_and_not(eng._abi, fn)
    total = sum(h.sum(axis=0, dtype=I64) for h in hs)
    for k, h in enumerate(hs):
        assert np.array_equal(o["H%d" % k], h), "part %d" % k
    assert np.array_equal(o["counts"], total) and np.array_equal(o["counts alone"], total)


GROUPS_CASES = [(18, 833, 3 * 256 + 37, 3), (25, 1100, 3 * 256 + 37, 4), (20, 130, 4 * 256 + 1, 1)]


def _groups_arith(S, N, R, G):
    blocks = count_grid(R, 1)
    assert blocks == 2 and tiles_of_waves(cdiv(R, 32), 8)[0] >= 3 and R % 32


@gpu
@pytest.mark.parametrize("S,N,R,G", GROUPS_CASES)
def test_grouped_count_pass(eng, S, N, R, G):
    """k_bin_hist_groups: the same tile loop with G x S counters per lane and a staging area per group; its column sums are 64-bit."""
    _groups_arith(S, N, R, G)
    rng = np.random.default_rng(S + N)
    x = flush_rows(R, N, S, 3)
    groups = [np.sort(rng.choice(N, size=max(1, N // (g + 2)), replace=False)).astype(I64) for g in range(G)]
    groups[0] = np.arange(N, dtype=I64)
    X = eng.states_to_device(x)

    def fn():
        Hs, counts = eng.bin_hist_groups(X, N, S, groups)
        out = {"H%d" % g: eng.hist_to_numpy(H) for g, H in enumerate(Hs)}
        out["counts"] = _np(counts)
        return out

    o = capped_and_not(eng._abi, fn)
    for g, cols in enumerate(groups):
        want = onp.bin_hist(x[:, cols], S)
        assert np.array_equal(o["H%d" % g], want), g
        assert np.array_equal(o["counts"][g], want.sum(axis=0)), g


# ----------------------------------------------------------------------------------------------------------------------------
# S1 scores
# ----------------------------------------------------------------------------------------------------------------------------
S1_HIST_CASES = [(18, 833, 12001), (15, 379, 12001), (15, 4000, 12001)]


def _s1_hist_arith(S, N, R):
    total, nent = R * S, (N + 1) * S
    assert total % 4 != 0                                                 # block 0 finishes the last one to three counts
    lds = []
    for itemsize in (4, 8):
        stride = s1_from_hist_stride(total, nent, itemsize, 1)
        assert stride <= 2048
        nquads = total // 4
        main = max(0, cdiv(nquads - 3 * stride, 4 * stride))             # thread 0: four quads in flight per turn, while qd + 3 stride < nquads
        assert main >= 3 and main * 4 * stride < nquads                   # ... three turns and more, then the tail loop has work
        assert nquads > 3 * 3 * stride
        lds.append(nent * itemsize <= 150 * 1024)
    return lds


def _s1_hist(S, N, R):
    rng = np.random.default_rng([S, N, R])
    h = rng.integers(0, N + 1, size=(R, S)).astype(U16)
    # 0, N and counts above N all over the array: "anything larger scores 0" is what a batch's flat histogram buffer relies on
    flat = h.reshape(-1)
    at = rng.choice(flat.size, size=3000, replace=False)
    flat[at[:1000]], flat[at[1000:2000]], flat[at[2000:2500]], flat[at[2500:]] = 0, N, N + 1, 65535
    flat[-3:] = (N, 65535, 0)                                             # the tail that is no whole quad
    flat[:4] = (65535, N, 0, N + 1)
    counts = rng.integers(1, 1 << 30, size=S).astype(I64)
    return h, counts


@gpu
@pytest.mark.parametrize("S,N,R", S1_HIST_CASES)
def test_s1_scores_from_histograms(eng, S, N, R):
    from epilogos_amd.scores import s1ScoreTable
    lds32, lds64 = _s1_hist_arith(S, N, R)
    assert (lds32, lds64) == ((True, True) if N < 4000 else (False, False))
    h, counts = _s1_hist(S, N, R)
    q = onp.normalise(counts)
    t64, t32 = s1ScoreTable(q, N)
    H, Q, CNT = _dev(h), torch.from_numpy(q).cuda(), torch.from_numpy(counts).cuda()
    T64, T32 = torch.from_numpy(t64).cuda(), torch.from_numpy(t32).cuda()

    def fn():
        out = {}
        o32, o64 = eng.score_s1_from_binhist(H, N, S, Q, want32=True, want64=True)
        out["f32"], out["f64"] = _np(o32), _np(o64)
        o32, o64 = eng.score_s1_from_binhist_table(H, N, S, T64=T64, T32=T32)
        out["table f32"], out["table f64"] = _np(o32), _np(o64)
        c = CNT.clone()
        q2, o32, o64 = eng.combine_score_s1(c, H, N, S, want32=True, want64=True, rezero=True)
        out["combine f32"], out["combine f64"], out["q"], out["rezeroed"] = _np(o32), _np(o64), _np(q2), _np(c)
        return out

    o = capped_and_not(eng._abi, fn)
    hc = np.where(h <= N, h, 0).astype(I64)                              # a count above N scores 0
    want = onp.kl(hc / N, q[None, :])
    np.testing.assert_allclose(o["f64"], want, rtol=1e-11, atol=1e-15)    # (tests/test_hip_parity.py _s1_check)
    np.testing.assert_allclose(o["f32"], want.astype(F32), rtol=2e-7, atol=0)
    cols = np.arange(S)[None, :]
    assert np.array_equal(o["table f64"], t64[hc, cols]) and np.array_equal(o["table f32"], t32[hc, cols])    # the caller's table: its bits
    assert np.array_equal(o["q"], q) and not o["rezeroed"].any()
    np.testing.assert_allclose(o["combine f64"], want, rtol=1e-11, atol=0)   # (test_hip_abi_contract.py b_combine)
    np.testing.assert_allclose(o["combine f32"], want.astype(F32), rtol=2e-7, atol=0)
    assert (o["f64"][h > N] == 0).all() and (o["f32"][h == 0] == 0).all()


S1_DIRECT_CASES = [(18, 833, 3 * 256 + 37), (18, 1100, 3 * 256 + 5), (15, 379, 3 * 256 + 37)]


@gpu
@pytest.mark.parametrize("S,N,R", S1_DIRECT_CASES)
def test_s1_scores_from_the_matrix(eng, S, N, R):
    """epg_score_s1: k_score_s1 (18 states; the count kernels' tile loop, 256 rows per sweep under the cap), the two passes otherwise."""
    assert count_grid(R, 1) == 2 and tiles_of_waves(cdiv(R, 32), 8)[0] >= 3 and R % 32
    x = flush_rows(R, N, S, 5)
    q = onp.normalise(onp.expected_s1(x, S))
    X, Q = eng.states_to_device(x), torch.from_numpy(q).cuda()

    def fn():
        o32, o64 = eng.score_s1(X, N, S, Q, want32=True, want64=True)
        return {"f32": _np(o32), "f64": _np(o64)}

    o = capped_and_not(eng._abi, fn)
    want = onp.score_s1(x, q, S)
    np.testing.assert_allclose(o["f64"], want, rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(o["f32"], want.astype(F32), rtol=2e-7, atol=0)


# ----------------------------------------------------------------------------------------------------------------------------
# S2
# ----------------------------------------------------------------------------------------------------------------------------
S2_ROWS = 3 * 2048 + 70                      # k_s2_hist_wave under the cap: 8 workgroups x 4 waves x 64 rows = 2048 rows per sweep
S2_HIST_CASES = [(18, 834), (5, 4096), (25, 900), (31, 4095), (30, 70)]     # (S, counts below this) of test_s2_counts_from_arbitrary_histograms


def _s2_hist_arith(R):
    ntiles = cdiv(R, 64)
    waves = min(cdiv(ntiles, 4), 1 * 8) * 4
    assert waves * 64 == 2048
    few, most = tiles_of_waves(ntiles, waves)
    assert few >= 3 and R % 64 != 0
    return ntiles, waves


def _s2_hist(S, hi, R, pair):
    """Tile t of the kernel's walk is rows [64 (ntiles - 1 - t), +64) (it walks H from its end).  A wave takes t = w, w + 32, ...:
    the tiles of every second turn hold counts >= 4096 (the 64-bit path), the others do not (the dot-product path)."""
    ntiles, waves = _s2_hist_arith(R)
    rng = np.random.default_rng([S, hi, int(pair)])
    lim = min(hi, 4096) // 2 if pair else hi                              # (H + H2 stays below 4096 outside the marked tiles)
    ha = rng.integers(0, lim, size=(R, S)).astype(U16)
    hb = rng.integers(0, lim, size=(R, S)).astype(U16) if pair else np.zeros((R, S), dtype=U16)
    big = np.zeros(R, dtype=bool)
    for t in range(ntiles):
        if (t // waves) % 2 == 1:
            d = ntiles - 1 - t
            big[64 * d:64 * d + 64] = True
            r = min(64 * d + int(rng.integers(0, 64)), R - 1)
            if pair:                                                      # neither group reaches 4096, their sum does
                ha[r, t % S], hb[r, t % S] = 4000, 96 + t
            else:
                ha[r, t % S] = 4096 if t % 3 == 0 else 65535 - t
    seq = [bool(big[64 * (ntiles - 1 - t)]) for t in range(0, ntiles, waves)]
    assert seq[:3] == [False, True, False]                                # wave 0's turns
    small = (ha.astype(I64) + hb)[~big]
    assert small.max() < 4096
    return ha, hb


@gpu
@pytest.mark.parametrize("pair", [False, True], ids=["H", "H+H2"])
@pytest.mark.parametrize("S,hi", S2_HIST_CASES)
def test_s2_counts_alternate_paths_from_tile_to_tile(eng, S, hi, pair):
    R = S2_ROWS
    ha, hb = _s2_hist(S, hi, R, pair)
    HA, HB = _dev(ha), _dev(hb)

    def fn():
        c = eng.hist_s2_from_binhist_pair(HA, HB, S) if pair else eng.hist_s2_from_binhist(HA, S)
        once = _np(c).reshape(S, S).copy()
        c = eng.hist_s2_from_binhist_pair(HA, HB, S, counts=c) if pair else eng.hist_s2_from_binhist(HA, S, counts=c)   # accumulates
        return {"counts": once, "twice": _np(c).reshape(S, S)}

    o = capped_and_not(eng._abi, fn)
    want = _pair_counts(ha.astype(I64) + hb)
    assert np.array_equal(o["counts"], want) and np.array_equal(o["twice"], 2 * want)


# (25 states: the log table of the float64 kernel sits in LDS while 256 x 25 x 8 + 16 (N + 1) <= 65536, N <= 895, of the float32 one up
#  to N = 2495; 1791 / 1792 take the same kernels, 895 / 896 the two float64 instantiations; N = 4000: no table in LDS at all)
S2_SCORE_CASES = [(18, 833, None), (25, 1791, None), (25, 1792, None), (25, 895, None), (25, 896, None), (15, 4000, None), (18, 379, 16)]
S2_SCORE_ROWS = 3 * 1024 + 9                 # k_score_s2_bin under the cap: 4 workgroups x 4 waves x 64 rows = 1024 rows per sweep


def _s2_score_arith(S, R):
    waves = min(cdiv(cdiv(R, 64), 4), 1 * 4) * 4
    assert waves * 64 == 1024 and tiles_of_waves(cdiv(R, 64), waves)[0] >= 3 and R % 64
    bpw = 64 // S                                                         # k_score_s2_from_hist (q with zero cells): 8 workgroups
    gwaves = min(cdiv(cdiv(R, bpw), 4), 1 * 8) * 4
    assert tiles_of_waves(cdiv(R, bpw), gwaves)[0] >= 3


@gpu
@pytest.mark.parametrize("S,N,top", S2_SCORE_CASES)
def test_s2_scores(eng, S, N, top):
    """top: only states below it occur, q has zero cells and the general kernel does the work instead of the bin-per-lane one."""
    R = S2_SCORE_ROWS
    _s2_score_arith(S, R)
    rng = np.random.default_rng([S, N])
    x = rng.integers(0, top or S, size=(R, N)).astype(np.int8)
    x[::9, : N // 2] = 3                                                  # skewed rows next to uniform ones
    h = onp.bin_hist(x, S)
    q = onp.normalise(_pair_counts(h))
    H, Q = _dev(h.astype(U16)), torch.from_numpy(np.ascontiguousarray(q.reshape(-1))).cuda()

    def fn():
        o32, o64 = eng.score_s2_from_binhist(H, N, S, Q, want32=True, want64=True)
        return {"f32": _np(o32), "f64": _np(o64)}

    o = capped_and_not(eng._abi, fn)
    want = onp.score_s2(x, q, S)
    np.testing.assert_allclose(o["f64"], want, rtol=1e-6, atol=1e-12)      # (tests/test_hip_parity.py _s2_check)
    np.testing.assert_allclose(o["f32"], want.astype(F32), rtol=3e-7, atol=1e-12)


# ----------------------------------------------------------------------------------------------------------------------------
# paired pass
# ----------------------------------------------------------------------------------------------------------------------------
PAIR_ROWS = (2 * 768 + 5, 1, 130, 768 + 63, 0, 64, 777)
# (S, NA, NB, ga, gb): the compile-time models and a run-time one, the flagship's widths and narrow ones, -g widths of their own
PAIR_CASES = [(18, 379, 342, 379, 342), (18, 379, 342, 100, 100), (15, 40, 33, 40, 33), (25, 40, 33, 20, 20), (21, 40, 33, 40, 33), (15, 379, 342, 379, 342)]
PAIR_SEEDS = (77, 0x9E3779B97F4A7C15)


def _prefetches(rows, waves):
    """k_pair_fused_s1, one workgroup: per wave, for every tile but its last, whether the NEXT tile is prefetched (a whole tile of 64
    rows) and whether it belongs to another part."""
    rows = [r for r in rows if r]
    t0 = np.concatenate([[0], np.cumsum([cdiv(r, 64) for r in rows])])
    out = []
    for w in range(waves):
        seq = list(range(w, int(t0[-1]), waves))
        turns = []
        for t, nt in zip(seq, seq[1:]):
            p, np_ = int(np.searchsorted(t0, t, side="right")) - 1, int(np.searchsorted(t0, nt, side="right")) - 1
            turns.append((rows[np_] - (nt - t0[np_]) * 64 >= 64, p != np_))
        out.append(turns)
    return out


def _pair_arith(S, NA, NB, ga, gb):
    n = NA + NB
    fused = pair_fused_waves(S, NA, NB, ga, gb)
    few, _ = tiles_of_waves(part_tiles(PAIR_ROWS, 64), fused)             # ONE workgroup: `fused` x 64 rows per sweep
    assert fused * 64 <= 768 and few >= 3
    if S in (15, 18, 25):
        turns = _prefetches(PAIR_ROWS, fused)
        flat = [t for w in turns for t in w]
        assert (True, False) in flat and (True, True) in flat and ((False, False) in flat or (False, True) in flat)
        # some wave: prefetch taken, then refused (the next tile is ragged), then taken again across a part boundary
        assert any(w[k][0] and not w[k + 1][0] and w[k + 2] == (True, True) for w in turns for k in range(len(w) - 2))
    rows2 = PAIR_ROWS + PAIR_ROWS                                         # the other kernels' grids are wider: the parts twice
    assert tiles_of_waves(part_tiles(rows2, 64), null_draws_waves(S, n, ga, gb))[0] >= 3
    tr = tile_rows(2 * 2 * S)                                             # k_null_hist_rows: 8 workgroups x 4 waves
    assert tiles_of_waves(part_tiles(rows2, tr), 32)[0] >= 3
    if S in (15, 18, 25) and (ga, gb) == (NA, NB):
        assert tiles_of_waves(part_tiles(rows2, 64), pair_count_null_waves(S, n, 1))[0] >= 3
    assert any(r % 64 for r in PAIR_ROWS)


def _pitched(x, ldx):
    host = np.full((x.shape[0], ldx), -1, dtype=np.int8)
    host[:, :x.shape[1]] = x
    return torch.from_numpy(host).cuda()


def _gather(T, h):
    return T[h.astype(I64), np.arange(h.shape[1])[None, :]]


@functools.lru_cache(maxsize=2)
def _pair_inputs(S, NA, NB):
    rows = PAIR_ROWS + PAIR_ROWS
    rng = np.random.default_rng([S, NA, NB])
    xs = []
    for r in rows:
        xa, xb = ref.dominant_states(rng, r, NA, S), ref.dominant_states(rng, r, NB, S)
        xa[::7], xb[::7] = S - 1, S - 1                                   # quiescent in both groups ...
        xb[::21] = 0                                                      # ... and in one only
        xs.append((xa, xb))
    keys = [(k << 40) + 1000 * k for k in range(len(rows))]
    return rows, xs, keys


@gpu
@pytest.mark.parametrize("S,NA,NB,ga,gb", PAIR_CASES)
def test_paired_pass(eng, S, NA, NB, ga, gb):
    from epilogos_amd.scores import s1ScoreTable
    _pair_arith(S, NA, NB, ga, gb)
    rows, xs, keys = _pair_inputs(S, NA, NB)
    n, n1 = len(rows), len(PAIR_ROWS)
    hs = [(ref.hist(a, S), ref.hist(b, S)) for a, b in xs]
    total = sum(a.sum(axis=0, dtype=I64) + b.sum(axis=0, dtype=I64) for a, b in hs)
    q = onp.normalise(total)
    tabs = {w: s1ScoreTable(q, w)[1] for w in {NA, NB, ga, gb}}
    T = {w: torch.from_numpy(t).cuda() for w, t in tabs.items()}
    fused_count = S in (15, 18, 25) and (ga, gb) == (NA, NB)
    pa, pb = eng.padded_width(NA), eng.padded_width(NB)
    XAs = [_pitched(a, pa + (0, 3, 32)[k % 3]) for k, (a, _b) in enumerate(xs)]
    XBs = [_pitched(b, pb + (32, 0, 3)[k % 3]) for k, (_a, b) in enumerate(xs)]
    HAs, HBs = [_dev(a) for a, _b in hs], [_dev(b) for _a, b in hs]
    qstate = S - 1
    masks = [torch.from_numpy(onp.quiescent_mask(a, b, qstate).astype(np.uint8)).cuda() for a, b in xs]

    def fn():
        out = {}
        if fused_count:
            counts = eng.zeros_counts(S)
            ha, hb, oa, ob = eng.pair_count_null_parts(XAs, XBs, NA, NB, S, PAIR_SEEDS[0], keys, counts=counts)
            out["counts"] = _np(counts)
            for k in range(n):
                out["cHA%d" % k], out["cHB%d" % k] = eng.hist_to_numpy(ha[k]), eng.hist_to_numpy(hb[k])
                out["cOA%d" % k], out["cOB%d" % k] = eng.hist_to_numpy(oa[k]), eng.hist_to_numpy(ob[k])
        OAs, OBs = eng.null_hist_from_binhist_parts(HAs, HBs, NA + NB, S, ga, gb, PAIR_SEEDS[0], keys)
        for k in range(n):
            out["OA%d" % k], out["OB%d" % k] = eng.hist_to_numpy(OAs[k]), eng.hist_to_numpy(OBs[k])
        quads = [(HAs[k], HBs[k], OAs[k], OBs[k]) for k in range(n1)]     # the issue's seven parts
        for tag, qs in (("", qstate), ("nomask ", None)):
            res = eng.pair_scores_s1_parts(quads, S, NA, NB, ga, gb, T[NA], T[NB], T[ga], T[gb], qstate=qs)
            for k, r in enumerate(res):
                for name in ("delta", "null", "rdist", "mdiff") + (("quies",) if qs is not None else ()):
                    out["%s%s%d" % (tag, name, k)] = _np(r[name])
        for tag, mk in (("draws", None), ("masked draws", masks)):
            got = eng.null_dist_draws_parts(HAs, HBs, keys, S, NA, NB, ga, gb, T[ga], T[gb], PAIR_SEEDS, masks=mk)
            for k in range(n):
                out["%s%d" % (tag, k)] = _np(got[k])
        return out

    o = capped_and_not(eng._abi, fn)
    if fused_count:
        assert np.array_equal(o["counts"], total)
    for k, r in enumerate(rows):
        if not r:
            continue
        (xa, xb), (hA, hB) = xs[k], hs[k]
        draws = [ref.sample_from_hist(hA, hB, NA + NB, ga, gb, seed, keys[k])[:2] for seed in PAIR_SEEDS]
        oA, oB = draws[0]
        assert np.array_equal(o["OA%d" % k], oA) and np.array_equal(o["OB%d" % k], oB), "null groups of part %d" % k
        if fused_count:
            assert np.array_equal(o["cHA%d" % k], hA) and np.array_equal(o["cHB%d" % k], hB), "histograms of part %d" % k
            assert np.array_equal(o["cOA%d" % k], oA) and np.array_equal(o["cOB%d" % k], oB), "fused null groups of part %d" % k
        nulls = [onp.pair_finish(_gather(tabs[ga], a), _gather(tabs[gb], b))[1] for a, b in draws]
        qm = onp.quiescent_mask(xa, xb, qstate)
        for j, nd in enumerate(nulls):
            assert np.array_equal(o["draws%d" % k][j].view(np.uint32), nd.view(np.uint32)), "draw %d of part %d" % (j, k)
            md = o["masked draws%d" % k][j]
            assert np.isnan(md[qm]).all() and np.array_equal(md[~qm].view(np.uint32), nd[~qm].view(np.uint32))
        if k < n1:
            delta, _ = onp.pair_finish(_gather(tabs[NA], hA), _gather(tabs[NB], hB))
            dist, md = onp.pair_metrics(delta, True)
            for tag in ("", "nomask "):
                assert np.array_equal(o[tag + "delta%d" % k], delta), "delta of part %d" % k
                assert np.array_equal(o[tag + "null%d" % k], nulls[0]), "null distance of part %d" % k
                assert np.array_equal(o[tag + "rdist%d" % k], dist) and np.array_equal(o[tag + "mdiff%d" % k], md), "STEP 4 of part %d" % k
            assert np.array_equal(o["quies%d" % k].astype(bool), qm), "quiescence mask of part %d" % k
            assert r < 64 or (qm.any() and not qm.all())


PCN_FLUSH = (18, 512, 500, (9 * 768 + 5, 3 * 768, 5 * 768 + 1))


def _pcn_flush_arith():
    S, NA, NB, rows = PCN_FLUSH
    waves = pair_count_null_waves(S, NA + NB, 1)
    assert waves * 64 == 768
    few, _ = tiles_of_waves(part_tiles(rows, 64), waves)
    fe = flush_every(max(NA, NB))
    assert 8 * few > fe                                                   # eight epilogues per tile (four 16-row sub-tiles of A and of B)
    assert min(2 * fe, 8 * few) * min(NA, NB) > 65535 >= fe * max(NA, NB)
    assert any(r % 64 for r in rows)


@gpu
def test_pair_count_null_flushes_inside_the_loop(eng):
    """k_pair_count_null keeps its own packed running counts (both groups of a lane's rows in the same words)."""
    _pcn_flush_arith()
    S, NA, NB, rows = PCN_FLUSH
    xs = [(flush_rows(r, NA, S, k), flush_rows(r, NB, S, k + 10)) for k, r in enumerate(rows)]
    keys = [5, 1 << 33, 40000000]
    pa, pb = eng.padded_width(NA), eng.padded_width(NB)
    XAs = [_pitched(a, pa + (0, 3, 32)[k]) for k, (a, _b) in enumerate(xs)]
    XBs = [_pitched(b, pb + (32, 0, 3)[k]) for k, (_a, b) in enumerate(xs)]

    def fn():
        counts = eng.zeros_counts(S)
        ha, hb, oa, ob = eng.pair_count_null_parts(XAs, XBs, NA, NB, S, PAIR_SEEDS[1], keys, counts=counts)
        out = {"counts": _np(counts)}
        for k in range(len(rows)):
            out["HA%d" % k], out["HB%d" % k] = eng.hist_to_numpy(ha[k]), eng.hist_to_numpy(hb[k])
            out["OA%d" % k], out["OB%d" % k] = eng.hist_to_numpy(oa[k]), eng.hist_to_numpy(ob[k])
        return out

    o = capped_and_not(eng._abi, fn)
    total = 0
    for k, (xa, xb) in enumerate(xs):
        hA, hB = ref.hist(xa, S), ref.hist(xb, S)
        total = total + hA.sum(axis=0, dtype=I64) + hB.sum(axis=0, dtype=I64)
        assert np.array_equal(o["HA%d" % k], hA) and np.array_equal(o["HB%d" % k], hB), k
        oA, oB, _ = ref.sample_from_hist(hA, hB, NA + NB, NA, NB, PAIR_SEEDS[1], keys[k])
        assert np.array_equal(o["OA%d" % k], oA) and np.array_equal(o["OB%d" % k], oB), k
    assert np.array_equal(o["counts"], total)


PAIR_TAIL_CASES = [(18, 3 * 2048 + 70), (15, 3 * 2048 + 7)]               # epg_pair_finish, epg_pair_metrics: 8 x 4 waves x 64 rows


@gpu
@pytest.mark.parametrize("S,R", PAIR_TAIL_CASES)
def test_pair_finish_and_metrics(eng, S, R):
    assert tile_rows(2 * S * 4) == 64 and tile_rows(S * 4) == 64
    assert tiles_of_waves(cdiv(R, 64), 32)[0] >= 3 and R % 64
    rng = np.random.default_rng(S)
    a, b = rng.standard_normal((R, S)).astype(F32), rng.standard_normal((R, S)).astype(F32)
    a[::5] = b[::5]
    a[::4, 1] = a[::4, S - 1] + (b[::4, 1] - b[::4, S - 1])               # ties of |delta|, up to rounding
    A, B = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()

    def fn():
        delta, dist = eng.pair_finish(A, B)
        rd, md = eng.pair_metrics(delta, roundtrip=True)
        rd0, md0 = eng.pair_metrics(delta, roundtrip=False)
        return {"delta": _np(delta), "dist": _np(dist), "rdist": _np(rd), "mdiff": _np(md), "rdist0": _np(rd0), "mdiff0": _np(md0)}

    o = capped_and_not(eng._abi, fn)
    d, dist = onp.pair_finish(a, b)
    assert np.array_equal(o["delta"], d) and np.array_equal(o["dist"], dist)
    for rt, tag in ((True, ""), (False, "0")):
        wd, wx = onp.pair_metrics(d, rt)
        assert np.array_equal(o["rdist" + tag], wd) and np.array_equal(o["mdiff" + tag], wx)


# ----------------------------------------------------------------------------------------------------------------------------
# S3
# ----------------------------------------------------------------------------------------------------------------------------
S3_ROWS = 3 * 1440 + 80                      # three slices of the biosample-lane kernel (BL_SLICE = 1440) and a ragged one; two of k_s3_score's 4096
S3_CASES = [(18, 33), (15, 65), (18, 65), (15, 33)]


def _s3_arith(S, R):
    assert cdiv(R, 1440) >= 4 and R % 1440 and cdiv(R, 4096) >= 2 and R % 4096
    cells = R * S                                                         # k_s3_fix_finish / k_s3_unit_finish: 8 workgroups x 256 cells per sweep
    assert cdiv(cells, 1 * 8 * 256) >= 3 and cells % 256


@functools.lru_cache(maxsize=1)
def _s3_inputs(S, N):
    rng = np.random.default_rng([S, N])
    x = rng.integers(0, S, size=(S3_ROWS, N)).astype(np.int8)
    x[::11, : N // 2] = S - 1
    c = onp.expected_s3(x, S)
    q = onp.normalise(c)
    # the rows compared with the per-row numpy loop: the first and the last row of every slice of either kernel, and every 9th row
    pick = sorted(set(range(0, S3_ROWS, 9)) | {r for k in range(5) for r in (1440 * k, 1440 * k - 1, 4096 * k, 4096 * k - 1) if 0 <= r < S3_ROWS}
                  | {S3_ROWS - 1})
    pick = np.array(pick)
    return x, c, q, pick, onp.score_s3_f64(x[pick], q, S)


@gpu
@pytest.mark.parametrize("S,N", S3_CASES)
def test_s3_counts_and_scores(eng, S, N):
    """What the one-CU grid changes here: k_s3_fix_finish / k_s3_unit_finish (8 workgroups walk the R x S cells), k_s3_tq_max and
    k_s3_tq_build (the lane kernel's table), k_s3_onehot_fp4, k_s3_reconstruct and the split heuristic of the contraction (its
    blockIdx.y).  k_s3_score, k_s3_score_bl, k_s3_hist, the transposes and k_s3_syrk_fp4's task grid are launched as on the device:
    for them the comparison of the two runs says nothing new, the oracle comparison over four slices does."""
    R = S3_ROWS
    _s3_arith(S, R)
    x, c, q, pick, want = _s3_inputs(S, N)
    X, Q = eng.states_to_device(x), torch.from_numpy(np.ascontiguousarray(q.reshape(-1))).cuda()
    abi = eng._abi

    def fn():
        out = {}
        for tag, sw in (("lanes", 0), ("bins", 1)):                       # both score kernels
            with forced(abi, 1, sw):
                o32, o64 = eng.score_s3(X, N, S, Q, want32=True, want64=True)
            out["f32 " + tag], out["f64 " + tag] = _np(o32), _np(o64)
        for tag, sw in (("full", (2, 1)), ("reduced", (2, 2)), ("lds", (3, 1))):      # all three count routes
            with forced(abi, *sw):
                out["counts " + tag] = _np(eng.hist_s3(X, N, S)).reshape(N, N, S, S)
        return out

    o = capped_and_not(abi, fn)
    for tag in ("full", "reduced", "lds"):
        assert np.array_equal(o["counts " + tag], c), tag
    for tag in ("lanes", "bins"):
        np.testing.assert_allclose(o["f64 " + tag][pick], want, rtol=1e-6, atol=1e-9)       # (tests/test_hip_s3_null.py)
        np.testing.assert_allclose(o["f32 " + tag][pick], want.astype(F32), rtol=1e-6, atol=1e-9)


# ----------------------------------------------------------------------------------------------------------------------------
# wide models, exceedance counts
# ----------------------------------------------------------------------------------------------------------------------------
WIDE = (40, 37, 3 * 512 + 37)                # (S, N, R) of tests/test_hip_wide_models.py, grown


def _wide_arith():
    S, N, R = WIDE
    assert cdiv(R, min(cdiv(R, 4), 1 * 32) * 4) >= 3                    # k_bin_hist_safe: 32 workgroups x 4 rows
    assert cdiv(R, min(cdiv(R, 128), 1 * 4) * 128) >= 3 and R % 128     # k_w_hist_s2: 4 workgroups x 128 rows
    assert cdiv(R, min(cdiv(R, 4), 1 * 16) * 4) >= 3                    # k_w_score_s2: 16 workgroups x 4 rows


@gpu
def test_wide_model(eng):
    _wide_arith()
    S, N, R = WIDE
    rng = np.random.default_rng(S * N)
    x = rng.integers(0, S, size=(R, N)).astype(np.int8)
    x[::13, : N // 2] = S - 1
    X = eng.states_to_device(x)
    h = onp.bin_hist(x, S)
    q1, q2 = onp.normalise(h.sum(axis=0)), onp.normalise(_pair_counts(h))
    Q1, Q2 = torch.from_numpy(q1).cuda(), torch.from_numpy(np.ascontiguousarray(q2.reshape(-1))).cuda()

    def fn():
        H, counts = eng.bin_hist(X, N, S)
        c2 = eng.hist_s2_from_binhist(H, S)
        a32, a64 = eng.score_s1_from_binhist(H, N, S, Q1, want32=True, want64=True)
        b32, b64 = eng.score_s2_from_binhist(H, N, S, Q2, want32=True, want64=True)
        return {"H": eng.hist_to_numpy(H), "counts": _np(counts), "counts2": _np(c2).reshape(S, S), "s1 f32": _np(a32), "s1 f64": _np(a64),
                "s2 f32": _np(b32), "s2 f64": _np(b64)}

    o = capped_and_not(eng._abi, fn)
    assert np.array_equal(o["H"], h) and np.array_equal(o["counts"], h.sum(axis=0)) and np.array_equal(o["counts2"], _pair_counts(h))
    want1 = onp.score_s1(x, q1, S)
    np.testing.assert_allclose(o["s1 f64"], want1, rtol=1e-11, atol=0)                         # (tests/test_hip_wide_models.py)
    np.testing.assert_allclose(o["s1 f32"], want1.astype(F32), rtol=2e-7, atol=0)              # (tests/test_hip_parity.py, S1 float32)
    want2 = onp.score_s2(x, q2, S)
    np.testing.assert_allclose(o["s2 f64"], want2, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(o["s2 f32"], want2.astype(F32), rtol=3e-7, atol=1e-12)


WIDE_S3 = (40, 12, 1100)


@gpu
def test_wide_model_s3(eng):
    S, N, R = WIDE_S3
    assert cdiv(R * N, 1 * 16 * 256) >= 3 and (R * N) % 256             # k_w_score_s3: 16 workgroups x 256 (bin, biosample) per sweep
    rng = np.random.default_rng(S + N)
    x = rng.integers(0, S, size=(R, N)).astype(np.int8)
    X = eng.states_to_device(x)
    c = onp.expected_s3(x, S)
    q = onp.normalise(c)
    Q = torch.from_numpy(np.ascontiguousarray(q.reshape(-1))).cuda()

    def fn():
        o32, o64 = eng.score_s3(X, N, S, Q, want32=True, want64=True)
        return {"counts": _np(eng.hist_s3(X, N, S)).reshape(N, N, S, S), "f32": _np(o32), "f64": _np(o64)}

    o = capped_and_not(eng._abi, fn)
    assert np.array_equal(o["counts"], c)
    want = onp.score_s3_f64(x, q, S)
    np.testing.assert_allclose(o["f64"], want, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(o["f32"], want.astype(F32), rtol=1e-6, atol=1e-9)                # (test_hip_abi_contract.py b_score_s3)


EXCEED_N = 3 * 4096 + 77                     # k_null_keys: 16 workgroups x 256 values per sweep


@gpu
def test_null_exceed(eng):
    assert cdiv(EXCEED_N, 1 * 16 * 256) >= 4 and EXCEED_N % 256
    x, d = ref.exceed_inputs(3, EXCEED_N)
    d = np.where(np.isnan(d), np.float32(0.5), d)
    X, D = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()

    def fn():
        e = torch.zeros(len(d), dtype=torch.int64, device="cuda")
        eng.null_exceed(X, D, e)
        return {"exceed": _np(e)}

    o = capped_and_not(eng._abi, fn)
    assert np.array_equal(o["exceed"], ref.exceed_np(x, d))


# ----------------------------------------------------------------------------------------------------------------------------
def test_case_arithmetic():
    """No GPU: the cases' own arithmetic (rows per sweep on the one-CU grid, tiles per wave, what a wrong flush interval would
    overflow), from the restated dispatch code above."""
    for case in COUNT_CASES + ONE_STATE_CASES:
        _count_arith(*case)
    for case in PARTS_CASES.values():
        _parts_arith(*case)
    for case in GROUPS_CASES:
        _groups_arith(*case)
    for case in S1_HIST_CASES:
        _s1_hist_arith(*case)
    _s2_hist_arith(S2_ROWS)
    for S, hi in S2_HIST_CASES:
        for pair in (False, True):
            _s2_hist(S, hi, S2_ROWS, pair)
    for S, _n, _t in S2_SCORE_CASES:
        _s2_score_arith(S, S2_SCORE_ROWS)
    for case in PAIR_CASES:
        _pair_arith(*case)
    _pcn_flush_arith()
    for S, _n in S3_CASES:
        _s3_arith(S, S3_ROWS)
    _wide_arith()
