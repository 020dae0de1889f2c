"""The device fit of the paired null distribution, the host side (no GPU): the algorithm of include/epilogos_gennorm.h restated in
numpy (tests/gennorm_ref.py) against scipy's own fit; what the header promises beyond its binding (tests/test_abi_symbols.py); the entry points'
argument checks, made before the first HIP call, in the documented order; --fit on the command line and its way down to _fitParams;
the seeding of the sub-samples.  scipy is the reference throughout."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.stats as st

from epilogos_amd import _abi
from epilogos_amd import roiAndVisualPairwise as rv
from tests import gennorm_ref as ref
from tests.test_null_draws_host import PAIRED, SINGLE, _cli_message, _results, _state_info

SIZES = (257, 3000, 100000)


def scipy_nnlf(params, x):
    """scipy's nnlf on the values widened to float64 (on a float32 array and plain floats scipy's arithmetic would be float32)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(st.gennorm.nnlf(tuple(float(v) for v in params), np.asarray(x, dtype=np.float64)))


def scipy_fit(x):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return st.gennorm.fit(x)


def no_worse_than_scipy(params, x, what=""):
    """The fit-quality condition: scipy's nnlf at `params` is at most scipy's nnlf at scipy's own fit plus fmin's absolute ftol
    (scipy's result is defined no more closely than that).  One-sided: a better optimum passes.  -> the difference."""
    got, want = scipy_nnlf(params, x), scipy_nnlf(scipy_fit(x), x)
    print("%s nnlf - scipy's = %.3g" % (what, got - want))
    assert got <= want + ref.FTOL, "%s: nnlf %.17g is more than 1e-4 above scipy's %.17g" % (what, got, want)
    return got - want


# ---- the algorithm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_the_restatement_is_no_worse_than_scipy(family, n):
    x = ref.sample(family, n)
    assert x.dtype == np.float32 and x.shape == (n,)
    params, fval, evals, flag = ref.fit(x)
    assert evals <= ref.MAXFUN and flag == 0 and np.isfinite(params).all() and np.isfinite(fval)
    assert abs(fval - scipy_nnlf(params, x)) <= ref.nnlf_bound(params, x)          # the objective IS scipy's nnlf
    no_worse_than_scipy(params, x, "%s n=%d" % (family, n))


def test_the_restatement_is_no_worse_than_scipy_on_the_gpu_tests_sub_samples():
    """The cases of tests/test_hip_gennorm.py, every trial: chosen so that the ALGORITHM satisfies the condition and gives the flag
    the GPU test wants, before device arithmetic comes into it."""
    from tests.test_hip_gennorm import FIT_CASES, case_inputs
    for family, n, T, with_idx, flag, seed in FIT_CASES:
        x, idx = case_inputs(family, n, T, with_idx, seed)
        for t in range(T if with_idx else 1):
            s = x[idx[t]] if with_idx else x
            params, _fval, evals, got = ref.fit(s)
            assert got == flag and evals <= ref.MAXFUN, (family, n, t, got, evals)
            no_worse_than_scipy(params, s, "%s n=%d trial %d" % (family, n, t))


def test_the_rounded_family_has_ties_and_the_signed_squares_a_small_beta():
    x = ref.sample("rounded", 3000)
    assert len(np.unique(x)) < 200
    assert 0.25 < ref.fit(ref.sample("signedsq", 100000))[0][0] < 0.45


def test_a_constant_sample_is_flagged():
    params, fval, evals, flag = ref.fit(np.full(300, 0.25, dtype=np.float32))
    assert flag == 2 and evals == 0 and np.isnan(params).all() and np.isnan(fval)
    x = ref.sample("gennorm2", 300)
    x[17] = np.inf
    assert ref.fit(x)[3] == 2
    x[17] = np.nan
    assert ref.fit(x)[3] == 2


def test_two_points_stop_at_the_cap_as_scipy_does():
    """n = 2 has no maximum likelihood (beta grows without bound): scipy's fmin ends at maxfun, and so does the restatement."""
    from scipy import optimize
    x = ref.sample("rounded", 5000)[[3, 11]]
    assert x[0] != x[1]
    params, fval, evals, flag = ref.fit(x)
    assert flag == 1 and evals == ref.MAXFUN and np.isfinite(params).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = optimize.fmin(lambda p: ref.objective(p, x), ref.start(x), full_output=True, disp=False)
    assert out[4] == 1 and out[3] == ref.MAXFUN


def test_the_objective_is_infinite_outside_the_parameter_space():
    x = ref.sample("gennorm2", 257)
    for p in ((0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 0.0, -2.0), (np.nan, 0.0, 1.0), (1.0, np.nan, 1.0), (1.0, 0.0, np.nan)):
        assert ref.objective(p, x) == np.inf


def test_the_median_pick_is_the_existing_rule():
    rng = np.random.default_rng(5)
    for T in (1, 2, 3, 4, 100, 101):
        for _ in range(5):
            nnlf = np.round(rng.normal(size=T), 1)                              # ties
            if T > 3:
                nnlf[rng.integers(0, T)] = np.inf
            want = int(np.argsort(nnlf, kind="stable")[int((T - 1) / 2)])        # (the expression _fitParams always used)
            assert ref.median_pick(nnlf) == want == rv.medianTrial(nnlf)


# ---- the header ------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_take_a_stream_and_keep_their_prefix():
    """(tests/test_abi_symbols.py holds the header against its binding and the library's exports.)"""
    from tests.abi_headers import header_prototypes
    protos = header_prototypes("gennorm")
    assert protos["epgf_gennorm_fit"][1][-1] == "void* stream" and protos["epgf_gennorm_nnlf"][1][-1] == "void* stream"
    # the prefix keeps the entry points out of the table of tests/test_hip_abi_streams.py; tests/test_hip_gennorm_streams.py runs its procedure
    from tests.test_abi_streams_coverage import stream_prototypes
    assert not [n for n in stream_prototypes() if "gennorm" in n]
    assert "epgf_" in _abi.HEADERS["gennorm"].path.read_text().split("#ifndef")[0]


def refusals(lib, x, idx, out, ws, M=5000, T=3, n=257, ws_bytes=1 << 30):
    """Every documented error code of the two entry points, in the documented order, on the pointers given (they are not
    dereferenced: every check comes before the first HIP call).  tests/test_hip_gennorm.py runs it on device memory."""
    ok = dict(x=x, M=M, idx=idx, T=T, n=n, params=out, fval=out, info=out, ws=ws, ws_bytes=ws_bytes, nnlf=out)
    off = ctypes.c_void_p(ws.value + 64)

    def fit(**kw):
        a = dict(ok, **kw)
        return lib.epgf_gennorm_fit(a["x"], a["M"], a["idx"], a["T"], a["n"], a["params"], a["fval"], a["info"], a["ws"], a["ws_bytes"], None)

    def nnlf(**kw):
        a = dict(ok, **kw)
        return lib.epgf_gennorm_nnlf(a["x"], a["M"], a["params"], a["T"], a["nnlf"], a["ws"], a["ws_bytes"], None)
    msg = lib.epg_last_error
    assert fit(T=0) == -1 and b"bad shape" in msg() and fit(n=1) == -1 and b"bad shape" in msg() and fit(n=M + 1) == -1 and b"bad shape" in msg()
    assert fit(M=1 << 31) == -2 and b"2^31" in msg()
    assert fit(idx=None) == -1 and b"idx is NULL" in msg()
    for name in ("x", "params", "fval", "info", "ws"):
        assert fit(**{name: None}) == -1 and (name + " is NULL").encode() in msg(), name
    assert fit(ws=off) == -1 and b"aligned" in msg()
    need = lib.epgf_gennorm_ws_bytes(M, T, n)
    assert need >= T * n * 4 and need % 256 == 0
    assert fit(ws_bytes=need - 1) == -4 and b"workspace" in msg()
    # the order: shape, unsupported size, idx, pointers (x, params, fval, info, ws), alignment, size
    assert fit(T=0, M=1 << 31, x=None) == -1 and b"bad shape" in msg()
    assert fit(M=1 << 31, idx=None, x=None) == -2
    assert fit(idx=None, x=None) == -1 and b"idx is NULL" in msg()
    assert fit(x=None, params=None) == -1 and b"x is NULL" in msg()
    assert fit(params=None, fval=None) == -1 and b"params is NULL" in msg()
    assert fit(fval=None, info=None) == -1 and b"fval is NULL" in msg()
    assert fit(info=None, ws=None) == -1 and b"info is NULL" in msg()
    assert fit(ws=off, ws_bytes=0) == -1 and b"aligned" in msg()
    assert nnlf(T=0) == -1 and b"bad shape" in msg() and nnlf(M=0) == -1 and b"bad shape" in msg()
    assert nnlf(M=1 << 31) == -2 and b"2^31" in msg()
    for name in ("x", "params", "nnlf", "ws"):
        assert nnlf(**{name: None}) == -1 and (name + " is NULL").encode() in msg(), name
    assert nnlf(ws=off) == -1 and b"aligned" in msg()
    assert nnlf(ws_bytes=lib.epgf_gennorm_ws_bytes(M, T, 0) - 1) == -4 and b"workspace" in msg()
    assert nnlf(T=0, M=1 << 31, x=None) == -1 and nnlf(M=1 << 31, x=None) == -2
    assert nnlf(x=None, params=None) == -1 and b"x is NULL" in msg()
    assert nnlf(nnlf=None, ws=None) == -1 and b"nnlf is NULL" in msg()
    assert nnlf(ws=off, ws_bytes=0) == -1 and b"aligned" in msg()


def test_argument_validation_without_gpu():
    lib = _abi.load()
    p = ctypes.c_void_p(1 << 20)
    refusals(lib, p, p, p, p)


def test_workspace_size():
    size = _abi.load().epgf_gennorm_ws_bytes
    for bad in ((0, 1, 0), (1 << 31, 1, 0), (10, 0, 0), (10, 1, 1), (10, 1, 11), (10, 1, -1)):
        assert size(*bad) == -1, bad
    assert size(1, 1, 0) == 256 and size(2, 1, 2) == 256
    assert size(5000, 101, 257) == 101 * 1280                                   # a trial's slice: its floats rounded up to 256 bytes
    assert size(1246253, 101, 100000) == 101 * 400128
    assert size(1246253, 101, 0) == -(-(1218 * 101 * 8) // 256) * 256           # 1218 chunks of 1024 values, a float64 per trial
    assert size(15000000, 101, 100000) == max(101 * 400128, -(-(14649 * 101 * 8) // 256) * 256)
    assert 0 < size((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1) % 256 + 1


# ---- the command line and STEP 4 ---------------------------------------------------------------------------------------------------
def test_the_three_usage_errors(capsys):
    msg = _cli_message(SINGLE + ["-n", "--fit", "gpu"], capsys)
    assert msg is not None and "--fit gpu" in msg and "paired" in msg
    msg = _cli_message(PAIRED + ["--fit", "gpu"], capsys)
    assert msg is not None and "--fit gpu" in msg and "--null-distribution" in msg
    msg = _cli_message(PAIRED + ["-n", "--fit", "gpu", "--null-draws", "4"], capsys)
    assert msg is not None and "--fit gpu" in msg and "--null-draws" in msg


@pytest.mark.parametrize("args", [PAIRED + ["-n", "--fit", "gpu"], PAIRED + ["-n", "--fit", "host"], PAIRED + ["--fit", "host"], SINGLE + ["--fit", "host"],
                                  PAIRED + ["-n", "--fit", "host", "--null-draws", "4"], PAIRED + ["-n", "--fit", "gpu", "--null-seed", "7"]])
def test_cli_accepts(args, capsys):
    msg = _cli_message(args, capsys)
    assert msg is None or "--fit" not in msg


def test_help_names_the_option():
    from click.testing import CliRunner

    from epilogos_amd import run
    out = " ".join(CliRunner().invoke(run.main, ["-h"], terminal_width=200).output.split())
    assert "--fit [host|gpu]" in out and "[default: host]" in out
    assert CliRunner().invoke(run.main, PAIRED + ["-n", "--fit", "cpu"]).exit_code == 2


def test_fit_host_reaches_fitParams_unchanged(tmp_path, monkeypatch):
    """Without the option, and with --fit host, STEP 4 calls _fitParams with the five positional arguments it always had; with
    fit="gpu" the two keywords come on top."""
    res, _M = _results(np.random.default_rng(4), with_exceed=False)
    calls = []

    def five(distanceArrNull, quiescenceArr, numProcesses, numTrials, samplingSize):
        calls.append((len(distanceArrNull), numProcesses, numTrials, samplingSize))
        return (1.5, 0.0, 2.0)
    monkeypatch.setattr(rv, "_fitParams", five)
    for kw in ({}, {"fit": "host"}, {"fit": "host", "seed": 7}):
        np.save(tmp_path / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
        rv.mainFromArrays(res, _state_info(tmp_path), tmp_path, "t", 2, True, 3, 1000, tmp_path / "exp_freq_t.npy", 10, False, **kw)
    assert calls == [(301, 2, 3, 1000)] * 3
    seen = []
    monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: seen.append((len(a), k)) or (1.5, 0.0, 2.0))
    np.save(tmp_path / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
    rv.mainFromArrays(res, _state_info(tmp_path), tmp_path, "t", 2, True, 3, 1000, tmp_path / "exp_freq_t.npy", 10, False, fit="gpu", seed=7)
    assert seen == [(5, {"fit": "gpu", "seed": 7})]


def test_the_host_fit_is_the_default_and_an_unknown_fit_is_refused(monkeypatch):
    data = ref.sample("gennorm2", 400)
    monkeypatch.setattr(rv, "fitOnSubSample", lambda values, samplingSize, rng=None: ((2.0, float(len(values)), 1.0), 3.0))
    assert rv._fitParams(data, np.zeros(400), 1, 3, 100) == (2.0, 400.0, 1.0)
    assert rv._fitParams(data, np.arange(400) < 100, 1, 3, 100, fit="host", seed=5) == (2.0, 300.0, 1.0)
    with pytest.raises(ValueError):
        rv._fitParams(data, np.zeros(400), 1, 3, 100, fit="cpu")


def test_a_degenerate_trial_falls_back_to_the_host_with_one_warning(monkeypatch, capsys):
    data = ref.sample("gennorm2", 400)
    asked = []
    monkeypatch.setattr(rv, "_fitParamsGpu", lambda d, T, n, seed: asked.append((len(d), T, n, seed)))      # -> None: a trial was flagged 2
    monkeypatch.setattr(rv, "fitOnSubSample", lambda values, samplingSize, rng=None: ((2.0, 0.0, 1.0), 3.0))
    assert rv._fitParams(data, np.zeros(400), 1, 3, 100, fit="gpu", seed=9) == (2.0, 0.0, 1.0)
    assert asked == [(400, 3, 100, 9)]
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 1 and out[0].startswith("WARNING:") and "host" in out[0]


def test_the_seed_gives_the_sub_samples():
    a, b = rv.fitIndices(5000, 7, 300, 7), rv.fitIndices(5000, 7, 300, 7)
    assert a.dtype == np.int32 and a.shape == (7, 300) and np.array_equal(a, b)
    assert all(len(np.unique(r)) == 300 for r in a) and a.min() >= 0 and a.max() < 5000          # without replacement
    assert not np.array_equal(a, rv.fitIndices(5000, 7, 300, 8))
    rng = np.random.default_rng([7, 0x666974])                                  # the documented recipe, trial after trial
    assert np.array_equal(a, np.stack([rng.choice(5000, 300, replace=False) for _ in range(7)]))
    assert np.array_equal(a[:3], rv.fitIndices(5000, 3, 300, 7))                # a prefix: trial t does not depend on T
    assert rv.fitIndices(300, 7, 300, 7) is None and rv.fitIndices(299, 7, 300, 7) is None
    assert not np.array_equal(rv.fitIndices(5000, 2, 300, None), rv.fitIndices(5000, 2, 300, None))
    assert np.array_equal(rv.fitIndices(5000, 2, 300, -3), rv.fitIndices(5000, 2, 300, -3))       # any integer --null-seed takes
