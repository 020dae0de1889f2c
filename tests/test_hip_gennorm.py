"""GPU: epgf_gennorm_nnlf and epgf_gennorm_fit (include/epilogos_gennorm.h) against scipy.stats.gennorm, straight through the C ABI.

The negative log-likelihood is held against scipy's on float64 within tests/gennorm_ref.nnlf_bound; the fit against scipy's own
fit of the same sub-sample with the one-sided condition of tests/test_gennorm_host.py (scipy's nnlf at the device's parameters is
at most scipy's nnlf at scipy's parameters plus fmin's ftol), on samples and sub-samples for which the numpy restatement of the
algorithm satisfies it (tests/test_gennorm_host.py runs the restatement on FIT_CASES without a GPU).  Two points have no maximum likelihood
(beta grows without bound): scipy's fmin stops at its cap there and so does the kernel, flag 1; every other case must converge.

The later turns of the kernels' loops have cases of their own, each with its arithmetic asserted from constants restated beside it: the
fit's sweeps of 1024 groups of four values (n = 4101, 8195 and the command's default 100000), the nnlf pass's second and later chunk of a
workgroup on the one-CU grid of tests/grid_cap.py, its second and third tile of 256 parameter sets."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gennorm_ref as ref
from tests.grid_cap import capped_and_not, cdiv
from tests.test_gennorm_host import no_worse_than_scipy, refusals, scipy_nnlf

pytestmark = pytest.mark.gpu

M0 = 5000
# family, n, T, idx given, the flag of every trial, the seed of the sub-samples (one for which the restatement satisfies the
# condition in every trial, with a margin; beta < 1 has a local optimum at every data point).  n: below one wave (2), no multiple of the block (257, 3000), one beyond the
# block (1025); idx None: M = n, every trial fits x[0 .. n)
FIT_CASES = [
    ("rounded", 257, 101, True, 0, 0),
    ("signedsq", 1025, 3, True, 0, 2),
    ("gennorm06", 1025, 3, True, 0, 0),
    ("signedsq", 3000, 3, True, 0, 0),
    ("gennorm2", 3000, 1, True, 0, 0),
    ("rounded", 2, 3, True, 1, 0),
    ("gennorm2", 1025, 1, False, 0, 0),
    ("signedsq", 3000, 3, False, 0, 0),
    ("rounded", 257, 101, False, 0, 0),
    ("signedsq", 2, 1, False, 1, 0),
    # sweeps beyond the first: a thread of the fit's workgroup takes group tid, tid + 1024, ... of four values (sweeps_of below).
    # 4097: 1024 groups and a tail of one, the last one-sweep shape; 4101: the smallest n with a tail at which thread 0 takes a second
    # group; 8195: two whole sweeps and a tail of three; 100000: the command's default -z, 25 sweeps (thread 0) and 24 (the others)
    ("signedsq", 4097, 3, True, 0, 3),
    ("rounded", 4097, 1, False, 0, 0),
    ("gennorm06", 4101, 3, True, 0, 0),
    ("gennorm2", 4101, 1, False, 0, 0),
    ("gennorm2", 8195, 3, True, 0, 0),
    ("signedsq", 8195, 1, False, 0, 0),
    ("signedsq", 100000, 2, True, 0, 2),
    ("gennorm06", 100000, 1, False, 0, 0),
]
# the size of the sample a case draws from: M0, and more for the sizes that M0 does not hold twice over
M0_OF = {8195: 20000, 100000: 120000}
IDS = ["%s-n%d-T%d-%s" % (f, n, T, "idx" if i else "all") for f, n, T, i, _flag, _seed in FIT_CASES]


def case_inputs(family, n, T, with_idx, seed=0):
    """-> (x float32 [M], idx int32 [T, n] or None)"""
    M = M0_OF.get(n, M0)
    assert M >= n
    x = ref.sample(family, M)
    return (x, ref.sub_samples(M, T, n, seed)) if with_idx else (x[:n].copy(), None)


GN_THREADS, GN_GROUP = 1024, 4               # k_gennorm_fit: threads of a trial's workgroup, floats of a group (epg_gennorm.hip)


def sweeps_of(n):
    """(groups, tail, turns of the gather / gn_block_sum loop that thread 0 runs, turns of the workgroup's last thread)."""
    groups = n // GN_GROUP
    return groups, n % GN_GROUP, -(-groups // GN_THREADS), groups // GN_THREADS


def case_of(family, n, T, with_idx):
    return FIT_CASES.index(next(c for c in FIT_CASES if c[:4] == (family, n, T, with_idx)))


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_fit(abi, x, idx, T, n):
    """One epgf_gennorm_fit on fresh device buffers filled with dirt -> (params [T, 3], fval [T], info [T, 2]) as numpy."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    idxd = torch.from_numpy(np.ascontiguousarray(idx)).cuda() if idx is not None else None
    M = xd.numel()
    params = torch.full((T, 3), -7.0, dtype=torch.float64, device="cuda")
    fval = torch.full((T,), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((T, 2), -7, dtype=torch.int32, device="cuda")
    need = abi.call("epgf_gennorm_ws_bytes", M, T, n)
    ws = torch.randint(0, 255, (need,), dtype=torch.uint8, device="cuda")
    abi.call("epgf_gennorm_fit", _p(xd), M, _p(idxd), T, n, _p(params), _p(fval), _p(info), _p(ws), need, _st())
    torch.cuda.synchronize()
    return params.cpu().numpy(), fval.cpu().numpy(), info.cpu().numpy()


def raw_nnlf(abi, x, params):
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    pd = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64)).cuda()
    M, T = xd.numel(), pd.shape[0]
    out = torch.full((T,), -7.0, dtype=torch.float64, device="cuda")
    need = abi.call("epgf_gennorm_ws_bytes", M, T, 0)
    ws = torch.randint(0, 255, (need,), dtype=torch.uint8, device="cuda")
    abi.call("epgf_gennorm_nnlf", _p(xd), M, _p(pd), T, _p(out), _p(ws), need, _st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


_FITS = {}


def fitted(abi, k):
    """The device's result of FIT_CASES[k], computed once."""
    if k not in _FITS:
        family, n, T, with_idx, _flag, seed = FIT_CASES[k]
        x, idx = case_inputs(family, n, T, with_idx, seed)
        _FITS[k] = (x, idx) + raw_fit(abi, x, idx, T, n)
    return _FITS[k]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- nnlf ------------------------------------------------------------------------------------------------------------------------
def nnlf_params(x, T):
    """[T, 3]: beta 0.34, 1, 2, 8 in turn, loc and scale varied, loc EQUAL to a data value in every fifth set, one invalid set."""
    rng = np.random.default_rng([x.size, T])
    p = np.empty((T, 3))
    p[:, 0] = np.resize([0.34, 1.0, 2.0, 8.0], T)
    p[:, 1] = rng.normal(scale=0.3, size=T)
    p[:, 2] = rng.uniform(0.05, 3.0, size=T)
    p[::5, 1] = x[rng.integers(0, x.size, size=len(p[::5]))].astype(np.float64)
    return p


INVALID = [(-1.0, 0.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 0.0, -1.0), (np.nan, 0.0, 1.0), (1.0, np.nan, 1.0), (1.0, 0.0, np.nan)]


@pytest.mark.parametrize("T", [1, 101])
@pytest.mark.parametrize("M", [1, 1023, 70001])
def test_nnlf_against_scipy(abi, M, T):
    x = ref.sample("signedsq", M)
    sets = nnlf_params(x, max(T, 8))
    sets[3] = INVALID[M % len(INVALID)]
    worst = 0.0
    for p in ([sets] if T > 1 else [sets[k:k + 1] for k in range(8)]):                  # T = 1: eight calls of one set each
        got = raw_nnlf(abi, x, p)
        for t in range(len(p)):
            if not (p[t, 0] > 0 and p[t, 2] > 0) or np.isnan(p[t]).any():
                assert got[t] == np.inf, (p[t], got[t])
                continue
            want, bound = scipy_nnlf(p[t], x), ref.nnlf_bound(p[t], x)
            worst = max(worst, abs(got[t] - want) / bound)
            assert abs(got[t] - want) <= bound, "set %s: %.17g, scipy %.17g, bound %.3g" % (p[t], got[t], want, bound)
    print("M=%d T=%d: largest |device - scipy| / bound = %.3g" % (M, T, worst))


def test_every_invalid_set_gives_inf_and_leaves_the_others_alone(abi):
    x = ref.sample("gennorm06", 3000)
    good = nnlf_params(x, 4)
    alone = raw_nnlf(abi, x, good)
    mixed = raw_nnlf(abi, x, np.concatenate([np.array(INVALID), good]))
    assert (mixed[:len(INVALID)] == np.inf).all() and np.array_equal(bits(mixed[len(INVALID):]), bits(alone))


def test_nnlf_does_not_depend_on_T_or_the_call(abi):
    x = ref.sample("signedsq", 70001)
    p = nnlf_params(x, 101)
    whole = raw_nnlf(abi, x, p)
    assert np.array_equal(bits(whole), bits(raw_nnlf(abi, x, p)))
    for t in (0, 57, 100):
        assert np.array_equal(bits(raw_nnlf(abi, x, p[t:t + 1])), bits(whole[t:t + 1])), t


# ---- nnlf: a workgroup's second and later chunks, the second and third tile of parameter sets ---------------------------------------
GN_CHUNK, GN_TT, GN_GRID_PER_CU = 1024, 256, 8   # epg_gennorm.hip: values per chunk, sets per LDS tile (and per finish workgroup), workgroups per CU


def nnlf_chunks_per_workgroup(M, cus):
    """(fewest, most) chunks that a workgroup of k_gennorm_nnlf_partial walks with c += gridDim.x on a device of `cus` CUs."""
    chunks = cdiv(M, GN_CHUNK)
    grid = min(chunks, GN_GRID_PER_CU * cus)
    return chunks // grid, cdiv(chunks, grid)


def hold_nnlf_against_scipy(x, p, got):
    """Every valid set of p within ref.nnlf_bound of scipy, every other one +inf -> the largest |device - scipy| / bound."""
    worst = 0.0
    for t in range(len(p)):
        if not (p[t, 0] > 0 and p[t, 2] > 0) or np.isnan(p[t]).any():
            assert got[t] == np.inf, (t, p[t], got[t])
            continue
        want, bound = scipy_nnlf(p[t], x), ref.nnlf_bound(p[t], x)
        worst = max(worst, abs(got[t] - want) / bound)
        assert abs(got[t] - want) <= bound, "set %d %s: %.17g, scipy %.17g, bound %.3g" % (t, p[t], got[t], want, bound)
    return worst


@pytest.mark.parametrize("M", [9217, 70001])
def test_nnlf_chunk_turns_on_the_one_cu_grid(abi, M):
    """c += gridDim.x: 8 workgroups on the one-CU grid.  9217 values are 10 chunks, two workgroups take two and six take one; 70001
    are 69 chunks, eight or nine per workgroup.  The sums are added per chunk, in chunk order: the grid must not change a bit."""
    assert nnlf_chunks_per_workgroup(M, 1) == {9217: (1, 2), 70001: (8, 9)}[M]
    if M == 70001:
        assert nnlf_chunks_per_workgroup(M, 1)[0] >= 3
    assert nnlf_chunks_per_workgroup(M, abi.call("epg_device_cus")) == (1, 1)            # what every other test of this module runs
    x = ref.sample("signedsq", M)
    sets = nnlf_params(x, 8)
    sets[3] = INVALID[M % len(INVALID)]
    got = capped_and_not(abi, lambda: {"nnlf": raw_nnlf(abi, x, sets)})["nnlf"]
    print("M=%d on one CU: largest |device - scipy| / bound = %.3g" % (M, hold_nnlf_against_scipy(x, sets, got)))


@pytest.mark.parametrize("T", [256, 257, 600])
@pytest.mark.parametrize("M", [1023, 9217])
def test_nnlf_tiles_of_parameter_sets(abi, M, T):
    """t0 += GN_TT in k_gennorm_nnlf_partial, and 256 sets per workgroup of k_gennorm_nnlf_finish: one whole tile, a second tile of one
    set, three tiles with a ragged last; 9217 values: the tiles inside the second and later chunk too."""
    tiles = cdiv(T, GN_TT)
    assert tiles == {256: 1, 257: 2, 600: 3}[T] and (T % GN_TT != 0) == (T != 256)
    x = ref.sample("signedsq", M)
    sets = nnlf_params(x, T)
    # invalid sets: the last of the first tile, then one in every later tile that holds a valid set beside it (the second tile of
    # T = 257 is ONE set: it stays valid, so that its value is held against scipy)
    planted = [t for t in (GN_TT - 1, GN_TT + 1, 2 * GN_TT + 3) if t < T]
    assert [t // GN_TT for t in planted] == list(range(tiles if T != GN_TT + 1 else 1))
    for j, t in enumerate(planted):
        sets[t] = INVALID[(M + T + j) % len(INVALID)]
    got = raw_nnlf(abi, x, sets)
    assert (got[planted] == np.inf).all()
    print("M=%d T=%d: largest |device - scipy| / bound = %.3g" % (M, T, hold_nnlf_against_scipy(x, sets, got)))
    for t in sorted({0, GN_TT - 2, GN_TT - 1, GN_TT, GN_TT + 1, 2 * GN_TT - 1, 2 * GN_TT, T - 1} & set(range(T))):
        assert np.array_equal(bits(raw_nnlf(abi, x, sets[t:t + 1])), bits(got[t:t + 1])), t


# ---- fit -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(FIT_CASES)), ids=IDS)
def test_fit_against_scipy(abi, k):
    family, n, T, with_idx, flag, _seed = FIT_CASES[k]
    x, idx, params, fval, info = fitted(abi, k)
    assert np.isfinite(params).all() and np.isfinite(fval).all()
    assert (info[:, 1] == flag).all(), info[:, 1]
    assert (info[:, 0] <= ref.MAXFUN).all() and (info[:, 0] >= 4).all()
    if flag == 1:
        assert (info[:, 0] == ref.MAXFUN).all()
    print("evaluations: %d .. %d" % (info[:, 0].min(), info[:, 0].max()))
    for t in range(T):
        s = x[idx[t]] if with_idx else x
        assert params[t, 0] > 0 and params[t, 2] > 0
        assert abs(fval[t] - scipy_nnlf(params[t], s)) <= ref.nnlf_bound(params[t], s), "trial %d: fval is not scipy's nnlf at the parameters" % t
        if not with_idx and t > 0:                                                      # the same sample: the same bits, scipy asked once
            assert np.array_equal(bits(params[t]), bits(params[0])) and bits(fval[t:t + 1]).tolist() == bits(fval[:1]).tolist()
            continue
        no_worse_than_scipy(params[t], s, "%s n=%d trial %d" % (family, n, t))


def test_the_later_sweep_cases_sweep_more_than_once():
    """The arithmetic of the cases beyond one sweep, from the constants restated above (no GPU work)."""
    assert sweeps_of(3000) == (750, 0, 1, 0)                                            # the largest of the earlier cases: one turn
    assert sweeps_of(4097) == (1024, 1, 1, 1)                                           # every thread one whole turn, thread 0 the tail
    assert sweeps_of(4101) == (1025, 1, 2, 1)                                           # thread 0 alone takes a second group
    assert sweeps_of(8195) == (2048, 3, 2, 2)
    assert sweeps_of(100000) == (25000, 0, 25, 24)
    for n in (4097, 4101, 8195, 100000):
        assert {c[3] for c in FIT_CASES if c[1] == n} == {True, False}, n               # each size with idx and without


def test_a_trial_has_the_same_bits_alone_and_in_a_batch_of_101(abi):
    x, idx, params, fval, info = fitted(abi, 0)
    assert len(idx) == 101
    for t in (0, 50, 100):
        p1, f1, i1 = raw_fit(abi, x, idx[t:t + 1], 1, idx.shape[1])
        assert np.array_equal(bits(p1), bits(params[t:t + 1])) and np.array_equal(bits(f1), bits(fval[t:t + 1])) and np.array_equal(i1, info[t:t + 1]), t
    # ... and a trial of two sweeps and a tail in a batch of 3: the slices of the workspace are 8256 floats apart, not n
    x, idx, params, fval, info = fitted(abi, case_of("gennorm2", 8195, 3, True))
    assert len(idx) == 3 and sweeps_of(idx.shape[1])[2:] == (2, 2)
    for t in (0, 1, 2):
        p1, f1, i1 = raw_fit(abi, x, idx[t:t + 1], 1, idx.shape[1])
        assert np.array_equal(bits(p1), bits(params[t:t + 1])) and np.array_equal(bits(f1), bits(fval[t:t + 1])) and np.array_equal(i1, info[t:t + 1]), t


_TWICE = [0, 3, 7, case_of("gennorm06", 4101, 3, True), case_of("signedsq", 100000, 2, True)]


@pytest.mark.parametrize("k", _TWICE, ids=[IDS[k] for k in _TWICE])
def test_two_identical_calls_give_identical_bits(abi, k):
    family, n, T, _with_idx, _flag, _seed = FIT_CASES[k]
    x, idx, params, fval, info = fitted(abi, k)
    p2, f2, i2 = raw_fit(abi, x, idx, T, n)
    assert np.array_equal(bits(p2), bits(params)) and np.array_equal(bits(f2), bits(fval)) and np.array_equal(i2, info)


def test_a_constant_sub_sample_is_flagged_and_the_other_trials_keep_their_bits(abi):
    n, T = 257, 5
    x = ref.sample("gennorm2", M0)
    x[4000:4000 + n] = np.float32(0.375)
    idx = ref.sub_samples(M0, T, n)
    base = raw_fit(abi, x, idx, T, n)
    assert (base[2][:, 1] == 0).all()
    idx2 = idx.copy()
    idx2[2] = np.arange(4000, 4000 + n)
    params, fval, info = raw_fit(abi, x, idx2, T, n)
    assert info[2].tolist() == [0, 2] and np.isnan(params[2]).all() and np.isnan(fval[2])
    keep = [0, 1, 3, 4]
    assert np.array_equal(bits(params[keep]), bits(base[0][keep])) and np.array_equal(bits(fval[keep]), bits(base[1][keep]))
    assert np.array_equal(info[keep], base[2][keep])
    x[4100] = np.inf                                                                     # a value that is not finite: the same flag
    assert raw_fit(abi, x, idx2, T, n)[2][2].tolist() == [0, 2]
    assert raw_nnlf(abi, x[:4000], params)[2] == np.inf                                  # NaN parameters: +inf


def test_every_documented_error_code_in_the_documented_order(abi):
    lib = abi.load()
    x = torch.zeros(M0, dtype=torch.float32, device="cuda")
    idx = torch.zeros((3, 257), dtype=torch.int32, device="cuda")
    out = torch.full((64,), 5.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    refusals(lib, _p(x), _p(idx), _p(out), _p(ws), ws_bytes=ws.numel())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((ws == 0).all())                             # a refused call touches nothing


def test_the_engine_wrappers(abi):
    from epilogos_amd import engine
    x, idx, params, fval, info = fitted(abi, 1)
    xd, idxd = torch.from_numpy(x).cuda(), torch.from_numpy(idx).cuda()
    p, f, i = engine.gennorm_fit(xd, idxd)
    assert np.array_equal(bits(p.cpu().numpy()), bits(params)) and np.array_equal(bits(f.cpu().numpy()), bits(fval)) and np.array_equal(i.cpu().numpy(), info)
    got = engine.gennorm_nnlf(xd, p)
    assert np.array_equal(bits(got.cpu().numpy()), bits(raw_nnlf(abi, x, params)))
    one = engine.gennorm_fit(xd[:1025])                                                    # idx None: one trial on all of x
    assert one[0].shape == (1, 3) and int(one[2][0, 1]) == 0
    for bad in (-1, M0):
        worse = idxd.clone()
        worse[1, 7] = bad
        with pytest.raises(ValueError, match="outside"):
            engine.gennorm_fit(xd, worse)
    with pytest.raises(ValueError):
        engine.gennorm_fit(xd.double(), idxd)
    with pytest.raises(ValueError):
        engine.gennorm_nnlf(xd, p.float())
