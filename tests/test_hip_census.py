"""GPU: epg_state_census (include/epilogos_census.h) against numpy -- np.bincount per column of the matrix's bytes.  Integers
only: census, other and first_bad must match exactly, on both load paths (16-byte loads; the byte path of a base or a row
stride that is no multiple of 16), on the one-CU grid and on the device's, and inside a guarded arena."""
import ctypes as C

import numpy as np
import pytest
import torch

from epilogos_amd import _abi, engine
from tests import grid_cap
from tests.abi_arena import Arena

pytestmark = pytest.mark.gpu

NONE = np.iinfo(np.int64).max
ROWS = (1, 63, 64, 65, 1000)
COLS = (1, 15, 16, 17, 100, 833, 1025)
LAYOUTS = ("padded", "wide", "odd_base", "odd_stride")


def reference(xs, S):
    """xs: uint8 [R, N] -> (census int64 [N, S], other int64 [N], first_bad)."""
    R, N = xs.shape
    census = np.zeros((N, S), dtype=np.int64)
    for n in range(N):
        census[n] = np.bincount(xs[:, n], minlength=256)[:S]
    other = R - census.sum(axis=1)
    bad = np.flatnonzero(xs.reshape(-1) >= S)
    return census, other, (int(bad[0]) if bad.size else NONE)


def make_bytes(rng, R, W, N, S, col0=0):
    """uint8 [R, W]: valid states everywhere, the bytes that are no state (or alias one) at known places inside columns
    col0 .. col0 + N - 1, and outside them -- the row padding -- valid states and 200, which must not be counted."""
    x = rng.integers(0, S, size=(R, W), dtype=np.uint8)
    outside = np.ones(W, dtype=bool)
    outside[col0:col0 + N] = False
    x[:, outside] = np.where(rng.random((R, int(outside.sum()))) < 0.5, 200, x[:, outside])
    specials = [0xFF, S, 31, 32 + int(rng.integers(0, S)), 0x80, 254]
    places = rng.choice(R * N, size=min(len(specials), R * N), replace=False)
    for at, b in zip(places, specials):
        x[at // N, col0 + at % N] = b
    return x


def device_view(x, N, layout, col0):
    """The host bytes as a device int8 matrix view of `layout` -> (X [R, >= N] whose first N columns are x[:, col0:col0 + N])."""
    R, W = x.shape
    if layout in ("padded", "wide", "odd_stride"):
        t = torch.from_numpy(x.view(np.int8)).cuda()
        X = t[:, col0:] if layout != "padded" else t
    else:                                                # the same rows one byte into an allocation
        flat = torch.empty(R * W + 1, dtype=torch.int8, device="cuda")
        flat[1:].copy_(torch.from_numpy(x.view(np.int8).reshape(-1)))
        X = flat[1:].view(R, W)
    return X


def layout_shape(N, layout):
    """(W, col0): the width of the allocation and the first column of the matrix in it."""
    ldx = engine.padded_width(N)
    return {"padded": (ldx, 0), "wide": (ldx + 32, 16), "odd_base": (ldx, 0), "odd_stride": (ldx + 7, 3)}[layout]


def run_case(rng, R, N, S, layout):
    W, col0 = layout_shape(N, layout)
    x = make_bytes(rng, R, W, N, S, col0)
    X = device_view(x, N, layout, col0)
    fast = X.data_ptr() % 16 == 0 and X.stride(0) % 16 == 0
    assert fast == (layout in ("padded", "wide")), layout
    census, other, fb = engine.state_census(X, N, S)
    want = reference(x[:, col0:col0 + N], S)
    where = "R=%d N=%d S=%d %s" % (R, N, S, layout)
    assert np.array_equal(census.cpu().numpy(), want[0]), where
    assert np.array_equal(other.cpu().numpy(), want[1]), where
    assert int(fb.item()) == want[2], where
    assert np.array_equal(X[:, :N].cpu().numpy().view(np.uint8), x[:, col0:col0 + N]), where       # (X is an input)
    return x, X, want


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S", [1, 15, 18, 31, 32, 127])
def test_against_numpy(S, layout):
    rng = np.random.default_rng(1000 * S + LAYOUTS.index(layout))
    for R in ROWS:
        for N in COLS:
            run_case(rng, R, N, S, layout)


@pytest.mark.parametrize("layout", ["padded", "odd_stride"])
def test_two_calls_add_up_and_first_bad_keeps_the_minimum(layout):
    rng = np.random.default_rng(7)
    R, N, S = 300, 100, 18
    W, col0 = layout_shape(N, layout)
    xa = rng.integers(0, S, size=(R, W), dtype=np.uint8)
    xb = xa.copy()
    xa[200, col0 + 5] = 33                               # the later offender first, then the earlier one
    xb[17, col0 + 60] = 0xFF
    XA, XB = device_view(xa, N, layout, col0), device_view(xb, N, layout, col0)
    census, other, fb = engine.state_census(XA, N, S)
    assert int(fb.item()) == 200 * N + 5
    engine.state_census(XB, N, S, census=census, other=other, first_bad=fb)
    wa, wb = reference(xa[:, col0:col0 + N], S), reference(xb[:, col0:col0 + N], S)
    assert np.array_equal(census.cpu().numpy(), wa[0] + wb[0]) and np.array_equal(other.cpu().numpy(), wa[1] + wb[1])
    assert int(fb.item()) == 17 * N + 60
    engine.state_census(XA, N, S, census=census, other=other, first_bad=fb)       # a later offender does not replace it
    assert int(fb.item()) == 17 * N + 60 and int(other.sum().item()) == 3


def test_other_and_first_bad_may_be_null():
    rng = np.random.default_rng(8)
    R, N, S = 130, 33, 18
    x = make_bytes(rng, R, engine.padded_width(N), N, S)
    X = device_view(x, N, "padded", 0)
    want = reference(x[:, :N], S)
    census, other, fb = engine.state_census(X, N, S, want_other=False, want_first_bad=False)
    assert other is None and fb is None and np.array_equal(census.cpu().numpy(), want[0])
    census, other, fb = engine.state_census(X, N, S, want_first_bad=False)
    assert fb is None and np.array_equal(other.cpu().numpy(), want[1]) and np.array_equal(census.cpu().numpy(), want[0])


def test_no_rows_and_no_columns_touch_nothing():
    S = 18
    X = torch.zeros((64, 32), dtype=torch.int8, device="cuda")
    pattern = torch.arange(1, 32 * S + 1, dtype=torch.int64, device="cuda") * 0x0101010101
    for R, N, ldx in ((0, 20, 32), (64, 0, 32), (0, 0, 1)):
        census, other, fb = pattern.clone(), pattern[:32].clone(), pattern[:1].clone()
        _abi.call("epg_state_census", C.c_void_p(X.data_ptr()), R, N, ldx, S, C.c_void_p(census.data_ptr()), C.c_void_p(other.data_ptr()),
                  C.c_void_p(fb.data_ptr()), None)
        torch.cuda.synchronize()
        assert torch.equal(census, pattern) and torch.equal(other, pattern[:32]) and torch.equal(fb, pattern[:1]), (R, N)
    census, other, fb = engine.state_census(X[:0], 20, S)
    assert census.shape == (20, S) and int(census.sum().item()) == 0 and int(other.sum().item()) == 0 and int(fb.item()) == NONE
    census, other, fb = engine.state_census(X, 0, S)
    assert census.shape == (0, S) and other.shape == (0,) and int(fb.item()) == NONE


@pytest.mark.parametrize("capped", [False, True])
def test_narrow_counters_do_not_wrap(capped):
    """70 001 rows of one value: a packed 8- or 16-bit partial counter that is not flushed in time wraps.  On the device's grid
    a block sees few of the rows; on the one-CU grid ONE block walks all of them and must flush on the way."""
    R, N, S = 70001, 17, 18
    abi = _abi
    for value, layout in ((0, "padded"), (0xFF, "padded"), (0, "odd_base"), (0xFF, "odd_base")):
        W, _ = layout_shape(N, layout)
        x = np.full((R, W), value, dtype=np.uint8)
        X = device_view(x, N, layout, 0)

        def go():
            return engine.state_census(X, N, S)
        if capped:
            with grid_cap.one_cu(abi):
                census, other, fb = go()
        else:
            census, other, fb = go()
        census, other = census.cpu().numpy(), other.cpu().numpy()
        if value == 0:
            assert (census[:, 0] == R).all() and census[:, 1:].sum() == 0 and other.sum() == 0 and int(fb.item()) == NONE
        else:
            assert census.sum() == 0 and (other == R).all() and int(fb.item()) == 0


@pytest.mark.parametrize("layout", ["padded", "odd_stride"])
def test_one_cu_grid_equals_the_devices(layout):
    rng = np.random.default_rng(11)
    R, N, S = 5000, 100, 18
    W, col0 = layout_shape(N, layout)
    x = make_bytes(rng, R, W, N, S, col0)
    X = device_view(x, N, layout, col0)

    def fn():
        census, other, fb = engine.state_census(X, N, S)
        return {"census": census.cpu().numpy(), "other": other.cpu().numpy(), "first_bad": fb.cpu().numpy()}
    got = grid_cap.capped_and_not(_abi, fn)
    want = reference(x[:, col0:col0 + N], S)
    assert np.array_equal(got["census"], want[0]) and np.array_equal(got["other"], want[1]) and int(got["first_bad"][0]) == want[2]


@pytest.mark.parametrize("S,N", [(18, 833), (40, 50)])
def test_column_sums_equal_the_count_pass(S, N):
    rng = np.random.default_rng(S)
    R = 777
    X = engine.states_to_device(rng.integers(0, S, size=(R, N)))
    census, other, fb = engine.state_census(X, N, S)
    _H, counts = engine.bin_hist(X, N, S, want_hist=False)
    assert torch.equal(census.sum(0), counts) and int(other.sum().item()) == 0 and int(fb.item()) == NONE
    assert int(counts.sum().item()) == R * N


@pytest.mark.parametrize("R,N,S,mis,ldx", [(333, 100, 18, 0, 112), (333, 100, 18, 5, 112), (70, 1025, 31, 0, 1040), (129, 17, 127, 0, 23),
                                           (2000, 50, 40, 0, 64)])
def test_contract_in_a_guarded_arena(R, N, S, mis, ldx):
    """Outputs between guard bands, every buffer sized exactly: nothing outside census[N * S], other[N] and first_bad[1] is
    written, X is unchanged, and the outputs ACCUMULATE on what they held."""
    rng = np.random.default_rng(R + N)
    x = make_bytes(rng, R, ldx, N, S)
    want = reference(x[:, :N], S)
    for null_other in (False, True):
        ar = Arena("cuda", guard_byte=1)
        ar.add("X", R * ldx, role="in", align=256, misalign=mis)
        ar.add("census", 8 * N * S, role="out", align=8)
        ar.add("other", 8 * N, role="out", align=8)
        ar.add("first_bad", 8, role="out", align=8)
        ar.build()
        ar.write("X", x)
        c0 = rng.integers(0, 1000, size=N * S).astype(np.int64)
        o0 = rng.integers(0, 1000, size=N).astype(np.int64)
        ar.write("census", c0)
        ar.write("other", o0)
        ar.write("first_bad", np.array([NONE], dtype=np.int64))
        ar.snapshot(frozen=("other", "first_bad") if null_other else ())
        _abi.call("epg_state_census", ar.ptr("X"), R, N, ldx, S, ar.ptr("census"), None if null_other else ar.ptr("other"),
                  None if null_other else ar.ptr("first_bad"), None)
        torch.cuda.synchronize()
        ar.check()
        assert np.array_equal(ar.read("census", np.int64), c0 + want[0].reshape(-1))
        if not null_other:
            assert np.array_equal(ar.read("other", np.int64), o0 + want[1]) and int(ar.read("first_bad", np.int64)[0]) == want[2]
