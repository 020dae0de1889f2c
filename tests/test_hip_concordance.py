"""GPU: epg_concordance (include/epilogos_concordance.h) against the numpy restatement of its definition
(tests/test_concordance_host.restatement).  Integers only: agree and both must match exactly, for every plane count, on both
kernels (fewer than 32 bins: the byte kernel), across chunks of the workspace, on the one-CU grid and on the device's, and
inside a guarded arena."""
import numpy as np
import pytest
import torch

from epilogos_amd import _abi, engine
from tests import grid_cap
from tests.abi_arena import Arena
from tests.conftest import synth_states
from tests.test_concordance_host import restatement

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 2049)
# the pair kernel's tiles are 16 columns i x 64 columns j: 63 / 64 / 65 lie below, at and above an edge of both, 130 spans three
# j-blocks and nine i-tiles (tiles on, above and -- skipped, mirrored -- below the diagonal)
COLS = (1, 2, 33, 63, 64, 65, 130)
STATES = (1, 15, 18, 31, 32, 100, 127)


def make_states(R, N, S, seed):
    """uint8 [R, N]: conftest.synth_states with about 5 % of the bytes replaced by those of {-1, S, 31, 32, 200} that are no
    state of the model."""
    x = synth_states(R, N, S, seed=seed).view(np.uint8).copy()
    rng = np.random.default_rng(seed + 1)
    bad = np.array([v for v in (0xFF, S, 31, 32, 200) if v >= S], dtype=np.uint8)
    hit = rng.random((R, N)) < 0.05
    x[hit] = bad[rng.integers(0, len(bad), size=int(hit.sum()))]
    return x


def to_device(x, ldx):
    """uint8 [R, N] -> int8 [R, ldx] on the device; the padding holds 0, a valid state: a kernel that reads past N counts it."""
    host = np.zeros((x.shape[0], ldx), dtype=np.uint8)
    host[:, :x.shape[1]] = x
    return torch.from_numpy(host.view(np.int8)).cuda()


def check(x, S, ldx, where):
    N = x.shape[1]
    X = to_device(x, ldx)
    agree, both = engine.concordance(X, N, S)
    wa, wb = restatement(x, S)
    a, b = agree.cpu().numpy(), both.cpu().numpy()
    assert np.array_equal(a, wa), where
    assert np.array_equal(b, wb), where
    assert np.array_equal(a, a.T) and np.array_equal(b, b.T) and np.array_equal(np.diag(a), (x < S).sum(axis=0)) and \
        np.array_equal(np.diag(a), np.diag(b)), where
    assert np.array_equal(X[:, :N].cpu().numpy().view(np.uint8), x), where                     # (X is an input)


@pytest.mark.parametrize("S", STATES)
def test_shape_grid(S):
    for R in ROWS:
        for N in COLS:
            x = make_states(R, N, S, seed=1000 * S + 10 * N + R % 7)
            for ldx in (engine.padded_width(N), N + 3):
                check(x, S, ldx, "R=%d N=%d S=%d ldx=%d" % (R, N, S, ldx))


@pytest.mark.parametrize("R", [20, 333])
def test_special_columns(R):
    """Two identical columns, a column that is no state anywhere, and a column that differs from another in the last bin only."""
    S, N = 18, 70
    x = make_states(R, N, S, seed=R)
    x[:, 40] = x[:, 3]
    x[:, 17] = 0xFF
    x[:, 66] = x[:, 5]
    x[R - 1, 5] = 0
    x[R - 1, 66] = 1
    X = to_device(x, engine.padded_width(N))
    agree, both = (t.cpu().numpy() for t in engine.concordance(X, N, S))
    wa, wb = restatement(x, S)
    assert np.array_equal(agree, wa) and np.array_equal(both, wb)
    assert agree[3, 40] == agree[40, 3] == both[3, 3] == both[40, 40] > 0
    assert not agree[17].any() and not agree[:, 17].any() and not both[17].any() and not both[:, 17].any()
    assert agree[5, 66] == both[5, 66] - 1 == agree[66, 5]


def test_accumulation_and_null_both():
    S, N = 18, 65
    xa, xb = make_states(300, N, S, seed=1), make_states(77, N, S, seed=2)
    XA, XB = to_device(xa, engine.padded_width(N)), to_device(xb, N + 3)
    agree, both = engine.concordance(XA, N, S)
    a2, b2 = engine.concordance(XB, N, S, agree=agree, both=both)
    assert a2.data_ptr() == agree.data_ptr() and b2.data_ptr() == both.data_ptr()
    wa, wb = restatement(np.concatenate([xa, xb]), S)
    assert np.array_equal(agree.cpu().numpy(), wa) and np.array_equal(both.cpu().numpy(), wb)
    # both = NULL: agree is what it is with both, and nothing else is returned
    only, none = engine.concordance(XA, N, S, want_both=False)
    assert none is None and np.array_equal(only.cpu().numpy(), restatement(xa, S)[0])
    # no rows: nothing is added
    a3, b3 = engine.concordance(XA[:0], N, S, agree=agree, both=both)
    assert np.array_equal(a3.cpu().numpy(), wa) and np.array_equal(b3.cpu().numpy(), wb)


@pytest.mark.parametrize("capped", [False, True])
def test_long_run_of_equal_columns(capped):
    """70 001 bins, 9 columns, every byte the same state: the largest counts a shape of this size has.  The workspace of this call
    is capped at R * N + 2^20 = 1 678 336 bytes = 1092 of its 2188 words of 1536 bytes, so the bins go in three chunks (1092,
    1092 and 4 words, the last holding 17 bins); on the one-CU grid the four tiles of a chunk are cut into 8 segments of words
    that 32 waves walk.  The counters have no flush interval to cross: a lane's u32 counter holds 2^26 words of 32 bins, which
    is the most a segment may have."""
    R, N, S = 70001, 9, 18
    assert engine.concordance_ws_bytes(R, N, S) == 1678336 < (R + 31) // 32 * 1536
    X = to_device(np.full((R, N), 4, dtype=np.uint8), engine.padded_width(N))
    if capped:
        with grid_cap.one_cu(_abi):
            agree, both = engine.concordance(X, N, S)
            torch.cuda.synchronize()
    else:
        agree, both = engine.concordance(X, N, S)
    assert (agree.cpu().numpy() == R).all() and (both.cpu().numpy() == R).all()


@pytest.mark.parametrize("S,N", [(18, 130), (100, 65)])
def test_one_cu_grid_equals_the_devices(S, N):
    R = 5000
    x = make_states(R, N, S, seed=N)
    X = to_device(x, N + 3)

    def fn():
        agree, both = engine.concordance(X, N, S)
        return {"agree": agree.cpu().numpy(), "both": both.cpu().numpy()}
    got = grid_cap.capped_and_not(_abi, fn)
    wa, wb = restatement(x, S)
    assert np.array_equal(got["agree"], wa) and np.array_equal(got["both"], wb)


@pytest.mark.parametrize("R,N,S,mis,ldx", [(333, 70, 18, 0, 80), (333, 70, 18, 5, 73), (20, 33, 18, 1, 33), (129, 17, 127, 0, 17)])
def test_contract_in_a_guarded_arena(R, N, S, mis, ldx):
    """Outputs and workspace between guard bands, every buffer sized exactly (X ends with its last row's ldx bytes; ldx == N in two
    cases, so a read past column N of the last row leaves the buffer): nothing outside agree[N * N], both[N * N] and the
    workspace is written, X is unchanged, and the outputs ACCUMULATE on what they held."""
    rng = np.random.default_rng(R + N)
    x = make_states(R, N, S, seed=R + N)
    host = np.zeros((R, ldx), dtype=np.uint8)
    host[:, :N] = x
    wa, wb = restatement(x, S)
    nws = engine.concordance_ws_bytes(R, N, S)
    for null_both in (False, True):
        ar = Arena("cuda", guard_byte=1)
        ar.add("X", R * ldx, role="in", align=256, misalign=mis)
        ar.add("agree", 8 * N * N, role="out", align=8)
        ar.add("both", 8 * N * N, role="out", align=8)
        ar.add("ws", nws, role="ws", align=256)
        ar.build()
        ar.write("X", host)
        a0 = rng.integers(0, 1000, size=N * N).astype(np.int64)
        b0 = rng.integers(0, 1000, size=N * N).astype(np.int64)
        ar.write("agree", a0)
        ar.write("both", b0)
        ar.snapshot(frozen=("both",) if null_both else ())
        _abi.call("epg_concordance", ar.ptr("X"), R, N, ldx, S, ar.ptr("agree"), None if null_both else ar.ptr("both"), ar.ptr("ws"), nws, None)
        torch.cuda.synchronize()
        ar.check()
        assert np.array_equal(ar.read("agree", np.int64), a0 + wa.reshape(-1))
        if not null_both:
            assert np.array_equal(ar.read("both", np.int64), b0 + wb.reshape(-1))


def test_real_fixture_and_the_trace_of_hist_s3(golden_real):
    """On the real slice: the restatement, and off the diagonal the trace over the state pairs of hist_s3's [N, N, S, S]
    co-occurrence counts -- what tools/concordance_bench.py holds the kernel against."""
    x = np.asarray(golden_real["x"]).astype(np.int8)
    S, N = 18, x.shape[1]
    X = engine.states_to_device(x)
    agree, both = engine.concordance(X, N, S)
    wa, wb = restatement(x.view(np.uint8), S)
    assert np.array_equal(agree.cpu().numpy(), wa) and np.array_equal(both.cpu().numpy(), wb)
    counts = engine.hist_s3(X, N, S).view(N, N, S, S)
    trace = torch.diagonal(counts, dim1=2, dim2=3).sum(-1).cpu().numpy().astype(np.int64)
    off = ~np.eye(N, dtype=bool)
    assert np.array_equal(trace[off], wa[off])
