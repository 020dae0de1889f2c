"""GPU: the p-value stage of paired mode on the device (csrc/epg_pvals.h).

epgf_gennorm_pvals against roiAndVisualPairwise.calculatePVals (scipy) on the inputs of tests/pvals_ref.py -- six sizes, six
parameter sets, every case led by the edge values (loc and its float32 neighbours, both zeros, the largest float32 and infinity of
both signs, denormals, both sides of the series / continued-fraction switch).  The bounds are FACTOR = 4 times what the numpy
restatement of the kernel differs from scipy by (tests/pvals_ref.REL_BELOW, ABS_ABOVE; tests/test_pvals_host.py measures them):
below loc relative plus 1e-300, above loc absolute.  p == 1 at x == loc and p == 0 at both infinities exactly; the flags.

epgf_bh_adjust against roiAndVisualPairwise.benjaminiHochberg BIT FOR BIT: ten sizes around the tile and the wave, six kinds of
input; its flag; two calls, the same bits; argument validation of both entry points in the documented order on device memory.
The host references are computed once per module.

The later turns of the kernels' loops: k_gennorm_pvals on the one-CU grid of tests/grid_cap.py (nine grid-stride turns over 70001 values,
NaN counts carried from turn to turn, byte for byte the device's own grid) and k_bh_carry with two and three tiles per thread (2^21 + 1
and 4 196 357 values); each case restates the kernel's constants and asserts its own turn count."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import roiAndVisualPairwise as rv
from tests import pvals_ref as ref
from tests.grid_cap import capped_and_not, cdiv
from tests.test_pvals_host import host_pvals

pytestmark = pytest.mark.gpu

BH_SIZES = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 70001)
BH_KINDS = ("uniform", "rounded", "equal", "descending", "above_one", "kernel")


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def host():
    """(params, M) -> (x, scipy's p-values), computed once."""
    return {(params, M): (ref.values(M, params),) + (host_pvals(ref.values(M, params), params),) for params in ref.PARAMS for M in ref.SIZES}


def device_pvals(eng, x, params):
    p, flags = eng.gennorm_pvals(torch.from_numpy(x).cuda(), torch.tensor(params, dtype=torch.float64).cuda())
    return p.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("M", ref.SIZES)
@pytest.mark.parametrize("params", ref.PARAMS, ids=["beta%g" % p[0] for p in ref.PARAMS])
def test_pvals_against_scipy(eng, host, params, M):
    x, want = host[params, M]
    p, flags = device_pvals(eng, x, params)
    assert p.dtype == np.float64 and p.shape == (M,) and list(flags) == [0, 0]
    rel, ab = ref.differences(p, want, x, params[1])
    print("beta %g M %d: relative below loc %.3g (bound %.3g), absolute above loc %.3g = %.1f x 2^-52 (bound %.3g)"
          % (params[0], M, rel, ref.FACTOR * ref.REL_BELOW, ab, ab * 2.0 ** 52, ref.FACTOR * ref.ABS_ABOVE))
    xd = x.astype(np.float64)
    assert (p[xd == params[1]] == 1.0).all() and (p[np.isinf(xd)] == 0.0).all()
    assert rel <= ref.FACTOR * ref.REL_BELOW
    assert ab <= ref.FACTOR * ref.ABS_ABOVE


def test_pvals_flags(eng, host):
    params = ref.PARAMS[0]
    x, _want = host[params, 1025]
    base, flags = device_pvals(eng, x, params)
    assert list(flags) == [0, 0]
    again, _ = device_pvals(eng, x, params)
    assert np.array_equal(base.view(np.uint64), again.view(np.uint64))
    y = x.copy()
    y[700] = np.nan
    p, flags = device_pvals(eng, y, params)
    assert list(flags) == [1, 0] and np.isnan(p[700])
    assert np.array_equal(np.delete(p, 700).view(np.uint64), np.delete(base, 700).view(np.uint64))
    for bad in ((0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (1.0, np.nan, 1.0), (1.0, 0.0, np.nan)):
        p, flags = device_pvals(eng, x, bad)
        assert list(flags) == [1025, 0] and np.isnan(p).all(), bad


# ---- the grid-stride turns of k_gennorm_pvals: the one-CU grid ------------------------------------------------------------------------
PV_THREADS, PV_BLOCKS_PER_CU = 256, 32                       # epg_pvals.hip: a workgroup, workgroups per compute unit
M_TURNS = 70001


def pvals_turns(M, cus):
    """(threads of the grid, the most turns of a thread's loop) on a device of `cus` compute units."""
    threads = min(cdiv(M, PV_THREADS), PV_BLOCKS_PER_CU * cus) * PV_THREADS
    return threads, cdiv(M, threads)


@pytest.mark.parametrize("params", ref.PARAMS, ids=["beta%g" % p[0] for p in ref.PARAMS])
def test_pvals_grid_stride_turns_on_the_one_cu_grid(eng, host, params):
    """70001 values on 8192 threads: nine turns, the last one ragged.  scipy with the bounds of test_pvals_against_scipy (the inputs
    are that test's), and the device's own grid, where a thread has one turn, byte for byte."""
    assert pvals_turns(M_TURNS, 1) == (8192, 9) and M_TURNS % 8192 != 0
    assert pvals_turns(M_TURNS, eng._abi.call("epg_device_cus"))[1] == 1
    x, want = host[params, M_TURNS]

    def fn():
        p, flags = device_pvals(eng, x, params)
        return {"p": p, "flags": flags}
    out = capped_and_not(eng._abi, fn)
    p = out["p"]
    assert p.dtype == np.float64 and p.shape == (M_TURNS,) and list(out["flags"]) == [0, 0]
    rel, ab = ref.differences(p, want, x, params[1])
    print("beta %g on one CU: relative below loc %.3g (bound %.3g), absolute above loc %.3g (bound %.3g)"
          % (params[0], rel, ref.FACTOR * ref.REL_BELOW, ab, ref.FACTOR * ref.ABS_ABOVE))
    xd = x.astype(np.float64)
    assert (p[xd == params[1]] == 1.0).all() and (p[np.isinf(xd)] == 0.0).all()
    assert rel <= ref.FACTOR * ref.REL_BELOW
    assert ab <= ref.FACTOR * ref.ABS_ABOVE


def test_pvals_flags_are_carried_across_turns(eng, host):
    """A thread's NaN count lives in a register from turn to turn: thread 700 of the one-CU grid meets NaN in its turns 0 and 1,
    thread 5 in its last turn only, thread 8191 in turn 3, the last value of all (thread 4464, turn 8) is one too."""
    params = ref.PARAMS[0]
    x, _want = host[params, M_TURNS]
    stride, turns = pvals_turns(M_TURNS, 1)
    assert (stride, turns) == (8192, 9)
    planted = [700, 700 + stride, 5 + 8 * stride, 3 * stride + stride - 1, M_TURNS - 1]
    assert len(set(planted)) == 5 and max(planted) == M_TURNS - 1 and np.isfinite(x[planted]).all()
    assert sorted(i % stride for i in planted) == [5, 700, 700, 4464, 8191]
    y = x.copy()
    y[planted] = np.nan
    base, flags = device_pvals(eng, x, params)
    assert list(flags) == [0, 0]

    def fn():
        p, flags = device_pvals(eng, y, params)
        return {"p": p, "flags": flags}
    out = capped_and_not(eng._abi, fn)
    assert list(out["flags"]) == [len(planted), 0] and np.isnan(out["p"][planted]).all()
    assert np.array_equal(np.delete(out["p"], planted).view(np.uint64), np.delete(base, planted).view(np.uint64))


def test_pvals_from_a_device_fit_s_row(eng):
    """params is device memory: a row of gennorm_fit's output feeds the call without a read-back."""
    x = ref.values(1025, ref.PARAMS[3])
    x = x[np.isfinite(x) & (np.abs(x) < 1)]
    xd = torch.from_numpy(x).cuda()
    fitted, _fval, info = eng.gennorm_fit(xd)
    assert int(info[0, 1]) != 2
    p, flags = eng.gennorm_pvals(xd, fitted[0])
    want = host_pvals(x, tuple(np.float64(v) for v in fitted[0].cpu().numpy()))
    rel, ab = ref.differences(p.cpu().numpy(), want, x, float(fitted[0, 1]))
    assert list(flags.cpu().numpy()) == [0, 0] and rel <= ref.FACTOR * ref.REL_BELOW and ab <= ref.FACTOR * ref.ABS_ABOVE


# ---- Benjamini-Hochberg --------------------------------------------------------------------------------------------------------------
def bh_input(kind, M, eng=None):
    rng = np.random.default_rng([M, BH_KINDS.index(kind)])
    if kind == "uniform":
        return rng.random(M)
    if kind == "rounded":                                                       # heavy ties, runs of 0.0 and of 1.0
        p = np.round(rng.random(M), 2)
        p[rng.random(M) < 0.1] = 0.0
        p[rng.random(M) < 0.1] = 1.0
        return p
    if kind == "equal":
        return np.full(M, 0.03125)
    if kind == "descending":
        return np.linspace(1.0, 0.0, M, endpoint=False)
    if kind == "above_one":
        return rng.random(M) * 3.0
    params = ref.PARAMS[M % len(ref.PARAMS)]                                    # the p-values the kernel above produces
    return device_pvals(eng, ref.values(M, params), params)[0]


def device_bh(eng, p):
    adj, flags = eng.bh_adjust(torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)).cuda())
    return adj.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("M", BH_SIZES)
def test_bh_is_the_host_s_bit_for_bit(eng, M):
    for kind in BH_KINDS:
        p = bh_input(kind, M, eng)
        assert p.shape == (M,) and not np.isnan(p).any() and (p >= 0).all()
        want = rv.benjaminiHochberg(p)
        got, flags = device_bh(eng, p)
        assert list(flags) == [0], kind
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), "%s M=%d: %d of %d values differ" % (
            kind, M, int((got.view(np.uint64) != want.view(np.uint64)).sum()), M)
        again, _ = device_bh(eng, p)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64)), kind


def test_bh_flags(eng):
    p = bh_input("uniform", 1025)
    for bad, n in ((np.nan, 1), (-0.25, 1), (-np.inf, 1), (-0.0, 1)):
        q = p.copy()
        q[[3, 1000][:n]] = bad
        assert list(device_bh(eng, q)[1]) == [n], bad
    q = p.copy()
    q[5], q[77], q[1024] = np.nan, -1.0, np.nan
    assert list(device_bh(eng, q)[1]) == [3]
    q = p.copy()
    q[9] = np.inf                                                               # +inf is a p >= +0.0: adjusted to 1, like the host's
    got, flags = device_bh(eng, q)
    assert list(flags) == [0] and np.array_equal(got.view(np.uint64), rv.benjaminiHochberg(q).view(np.uint64))


# ---- k_bh_carry with more than one tile per thread ---------------------------------------------------------------------------------
BH_TILE, BH_CARRY_THREADS = 2048, 1024                       # epg_pvals.hip: sorted values per tile, threads of the ONE carry workgroup
BH_BIG = (2097152, 2097153, 4196357)
BH_BIG_KINDS = ("uniform", "rounded", "descending", "above_one")


def bh_carry_shape(M):
    """(tiles, tiles per carry thread, threads that own a tile, tiles of the last of them)."""
    tiles = cdiv(M, BH_TILE)
    chunk = cdiv(tiles, BH_CARRY_THREADS)
    return tiles, chunk, cdiv(tiles, chunk), tiles - (cdiv(tiles, chunk) - 1) * chunk


def test_bh_big_sizes_give_a_carry_thread_more_than_one_tile():
    assert bh_carry_shape(max(BH_SIZES)) == (35, 1, 35, 1)                      # the largest size of the test above
    assert bh_carry_shape(2097152) == (1024, 1, 1024, 1)                        # the last shape of one tile per thread
    assert bh_carry_shape(2097153) == (1025, 2, 513, 1)                         # threads 513 .. 1023 own nothing, thread 512 one tile of ONE value
    assert bh_carry_shape(4196357) == (2050, 3, 684, 1)                         # thread 683 is ragged, the last tile too
    assert 4196357 % BH_TILE == 5


@pytest.mark.parametrize("kind", BH_BIG_KINDS)
@pytest.mark.parametrize("M", BH_BIG)
def test_bh_with_chunks_of_tiles_is_the_host_s_bit_for_bit(eng, M, kind):
    """("descending": every minimum comes from the far right, a wrong carry between two chunks shows in nearly every value.)"""
    assert bh_carry_shape(M)[1] == {2097152: 1, 2097153: 2, 4196357: 3}[M]
    p = bh_input(kind, M)
    want = rv.benjaminiHochberg(p)
    got, flags = device_bh(eng, p)
    assert list(flags) == [0]
    differ = got.view(np.uint64) != want.view(np.uint64)
    assert not differ.any(), "%s M=%d: %d of %d values differ, the first at %d" % (kind, M, int(differ.sum()), M, int(np.argmax(differ)))


def test_bh_flags_with_chunks_of_tiles(eng):
    M = BH_BIG[-1]
    assert bh_carry_shape(M)[1] == 3
    p = bh_input("uniform", M)
    planted = {3: np.nan, 700 * BH_TILE: -0.0, 1030 * BH_TILE + 7: np.nan, 2049 * BH_TILE: -np.inf, M - 1: -0.25}
    assert len({i // BH_TILE for i in planted}) == 4 and max(planted) < M        # (tiles of the input; sorted, they all go behind +inf)
    for i, v in planted.items():
        p[i] = v
    assert list(device_bh(eng, p)[1]) == [len(planted)]


def test_engine_checks_its_arguments(eng):
    x = torch.zeros(10, dtype=torch.float32, device="cuda")
    th = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64, device="cuda")
    for bad_x in (x.double(), x.cpu(), x[:0], x.view(2, 5), torch.zeros(20, dtype=torch.float32, device="cuda")[::2]):
        with pytest.raises(ValueError):
            eng.gennorm_pvals(bad_x, th)
    for bad_th in (th.float(), th.cpu(), th[:2], torch.zeros(6, dtype=torch.float64, device="cuda")[::2]):
        with pytest.raises(ValueError):
            eng.gennorm_pvals(x, bad_th)
    p = torch.zeros(10, dtype=torch.float64, device="cuda")
    for bad_p in (p.float(), p.cpu(), p[:0], p.view(2, 5), torch.zeros(20, dtype=torch.float64, device="cuda")[::2]):
        with pytest.raises(ValueError):
            eng.bh_adjust(bad_p)
    assert eng.bh_ws_bytes(10) % 256 == 0 and eng.bh_ws_bytes(70001) >= 70001 * 12
    with pytest.raises(eng.EpilogosHipError):
        eng.bh_adjust(p, ws=torch.empty(256, dtype=torch.uint8, device="cuda"))


def test_argument_validation_on_device_memory(eng):
    """The documented order, with real device pointers: shape, unsupported size, pointers, alignment of ws, size of ws."""
    from epilogos_amd import _abi
    lib = _abi.load()
    msg = lib.epg_last_error
    M = 1025
    need = lib.epgf_bh_ws_bytes(M)
    assert need > 0 and need % 256 == 0
    buf = torch.zeros(need + 512, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 255) // 256 * 256
    ws, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 64)
    d = torch.zeros(M, dtype=torch.float64, device="cuda")
    o = torch.zeros(M, dtype=torch.float64, device="cuda")
    f = torch.zeros(2, dtype=torch.int32, device="cuda")
    x = torch.zeros(M, dtype=torch.float32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    bh, pv = lib.epgf_bh_adjust, lib.epgf_gennorm_pvals
    assert bh(P(d), 0, P(o), P(f), ws, need, None) == -1 and b"bad shape" in msg()
    assert bh(None, 1 << 31, P(o), P(f), ws, need, None) == -2 and b"2^31" in msg()
    assert bh(None, M, None, P(f), ws, need, None) == -1 and b"p is NULL" in msg()
    assert bh(P(d), M, None, None, ws, need, None) == -1 and b"adj is NULL" in msg()
    assert bh(P(d), M, P(o), None, None, need, None) == -1 and b"flags is NULL" in msg()
    assert bh(P(d), M, P(o), P(f), None, 0, None) == -1 and b"ws is NULL" in msg()
    assert bh(P(d), M, P(o), P(f), off, 0, None) == -1 and b"aligned" in msg()
    assert bh(P(d), M, P(o), P(f), ws, need - 1, None) == -4 and b"workspace" in msg()
    assert pv(P(x), 0, P(d), P(o), P(f), None) == -1 and pv(None, 1 << 31, P(d), P(o), P(f), None) == -2
    assert pv(None, M, None, P(o), P(f), None) == -1 and b"x is NULL" in msg()
    assert pv(P(x), M, P(d), P(o), None, None) == -1 and b"flags is NULL" in msg()
    torch.cuda.synchronize()
    assert not o.any() and not f.any()                                          # a refused call touches nothing
    assert bh(P(d), M, P(o), P(f), ws, need, None) == 0
    torch.cuda.synchronize()
