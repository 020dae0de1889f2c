"""The p-value stage of paired mode on the device, the host side (no GPU): the kernel's arithmetic restated in numpy
(tests/pvals_ref.py) against roiAndVisualPairwise.calculatePVals on the inputs of tests/test_hip_pvals.py, within the figures that
file records; the internal binding table against csrc/epg_pvals.h, type for type, and the library's exports; --pvals on the
command line and its way down to STEP 4."""
import ctypes
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from epilogos_amd import _abi, build
from epilogos_amd import roiAndVisualPairwise as rv
from tests import pvals_ref as ref
from tests.abi_headers import ctypes_of
from tests.test_null_draws_host import PAIRED, SINGLE, _cli_message, _results, _state_info

NAMES = ["epgf_bh_adjust", "epgf_bh_ws_bytes", "epgf_gennorm_pvals"]


def host_pvals(x, params):
    """calculatePVals as STEP 4 calls it: the float32 distances and np.float64 parameters, as the fit returns them."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return rv.calculatePVals(np.asarray(x, dtype=np.float32), np.float64(params[0]), np.float64(params[1]), np.float64(params[2]))


# ---- (a) the restatement -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    out = {}
    for params in ref.PARAMS:
        for M in ref.SIZES:
            x = ref.values(M, params)
            p, flags = ref.pvals(x, *params)
            want = host_pvals(x, params)
            out[params, M] = (x, p, flags, want) + ref.differences(p, want, x, params[1])
    return out


def test_the_restatement_stays_within_the_recorded_figures(measured):
    rel = max(v[4] for v in measured.values())
    ab = max(v[5] for v in measured.values())
    strings = sum(int(sum(("%.5e" % a) != ("%.5e" % b) for a, b in zip(v[1], v[3]))) for v in measured.values())
    print("restatement against calculatePVals: relative below loc %.3g, absolute above loc %.3g (%.1f x 2^-52), %d %%.5e strings differ"
          % (rel, ab, ab * 2.0 ** 52, strings))
    assert 0 < rel <= ref.REL_BELOW and 0 < ab <= ref.ABS_ABOVE
    assert ref.REL_BELOW < 1e-12 and ref.ABS_ABOVE < 1e-13                    # (the record itself: nobody widened it by orders)
    assert strings == 0
    for (_params, M), v in measured.items():
        assert v[1].shape == (M,) and not v[2][1], "an iteration stopped at the cap"


def test_the_inputs_hold_the_edge_values():
    big = np.finfo(np.float32).max
    for params in ref.PARAMS:
        beta, loc, scale = params
        x = ref.values(63, params)
        assert x.dtype == np.float32 and x.shape == (63,)
        xd = x.astype(np.float64)
        assert (xd <= loc).any() and (xd > loc).any()
        lo, hi = xd[xd < loc].max(), xd[xd > loc].min()
        assert np.nextafter(np.float32(lo), np.float32(np.inf)) in (np.float32(hi), np.float32(loc))      # the float32 neighbours of loc
        assert (float(np.float32(loc)) == loc) == bool((xd == loc).any())
        for v in (big, -big, np.inf, -np.inf, np.float32(1e-45)):
            assert v in x
        assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        with np.errstate(all="ignore"):
            t = np.abs((xd - loc) / scale) ** beta                              # both sides of the switch, left and right of loc
        a1 = 1.0 / beta + 1.0
        for side in (xd < loc, xd > loc):
            assert (t[side] < a1).any() and ((t[side] >= a1) & (t[side] < 1.001 * a1)).any(), params
    assert ref.values(1, ref.PARAMS[3])[0] == 0.0 and ref.values(70001, ref.PARAMS[0]).shape == (70001,)


def test_the_exact_cases_and_the_flags_of_the_restatement():
    for params in ref.PARAMS:
        x = ref.values(65, params)
        p, flags = ref.pvals(x, *params)
        xd = x.astype(np.float64)
        assert (p[xd == params[1]] == 1.0).all() and (p[np.isinf(xd)] == 0.0).all() and list(flags) == [0, 0]
        assert ((p >= 0) & (p <= 1)).all()
        y = x.copy()
        y[7] = np.nan
        q, flags = ref.pvals(y, *params)
        assert list(flags) == [1, 0] and np.isnan(q[7]) and np.array_equal(np.delete(q, 7), np.delete(p, 7))
    for bad in ((0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (1.0, np.nan, 1.0), (1.0, 0.0, np.nan)):
        p, flags = ref.pvals(ref.values(65, ref.PARAMS[2]), *bad)
        assert np.isnan(p).all() and list(flags) == [65, 0]


def test_the_cap_is_counted():
    """A cap of 3 terms is met by nearly every value; the default never is on these inputs (asserted above)."""
    x = ref.values(1025, ref.PARAMS[3])
    old = ref.ITMAX
    try:
        ref.ITMAX = 3
        _p, flags = ref.pvals(x, *ref.PARAMS[3])
    finally:
        ref.ITMAX = old
    assert flags[0] == 0 and flags[1] > 900


# ---- (b) the header and its binding --------------------------------------------------------------------------------------------------
def header_prototypes(path):
    """name -> (return type, [parameter declarations]) of every prototype of a header (the parser of tests/abi_headers.py, on a path)."""
    txt = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    txt = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", txt, flags=re.M)
    protos = {}
    for stmt in txt.split(";"):
        m = re.match(r"\s*(.*?)\b(epg[tf]?_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            args = " ".join(m.group(3).split())
            protos[m.group(2)] = (" ".join(m.group(1).split()), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return protos


@pytest.fixture(scope="module")
def lib():
    if build.is_stale():
        if shutil.which("hipcc") is None:
            pytest.skip("hipcc not available and library not prebuilt")
        build.build_library()
    return _abi.load()


def test_the_internal_table_is_apart_from_the_public_registry():
    assert list(_abi.INTERNAL) == list(build.INTERNAL_HEADERS) == ["pvals"] and "pvals" not in _abi.HEADERS and "pvals" not in build.PUBLIC_HEADERS
    header = _abi.INTERNAL["pvals"]
    assert header.path == build.CSRC / "epg_pvals.h" and header.path in build.HEADERS and "epg_pvals.hip" in build.SOURCES
    assert not list((build.ROOT / "include").glob("*pvals*"))
    for public in _abi.HEADERS.values():
        assert not set(public.prototypes) & set(header.prototypes)
    text = header.path.read_text()
    assert "PACKAGE-INTERNAL" in text and "include/epilogos_pvals.h" in text and "tests/test_abi_symbols.py" in text


def test_header_and_binding_agree():
    header = _abi.INTERNAL["pvals"]
    protos = header_prototypes(header.path)
    assert sorted(protos) == sorted(header.prototypes) == NAMES
    for name, (res, args) in header.prototypes.items():
        ret, params = protos[name]
        assert res is ctypes_of(ret, returned=True), name
        assert len(args) == len(params), name
        for i, (a, p) in enumerate(zip(args, params)):
            assert "double " not in p.replace("double*", "") and a is ctypes_of(p), "%s: parameter %d is `%s` in the header, %s in the binding" % (name, i, p, a.__name__)
    assert protos["epgf_gennorm_pvals"][1][-1] == "void* stream" and protos["epgf_bh_adjust"][1][-1] == "void* stream"


def test_library_exports_every_name(lib):
    fresh = ctypes.CDLL(str(_abi.lib_path()))
    for name in NAMES:
        fn = getattr(lib, name)
        assert hasattr(fresh, name) and fn.argtypes == _abi.INTERNAL["pvals"].prototypes[name][1]
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(_abi.lib_path())], capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(NAMES) <= exported


def test_argument_validation_without_gpu(lib):
    """Every check that needs no device, in the documented order (tests/test_hip_pvals.py runs the rest on device memory)."""
    p = ctypes.c_void_p(1 << 20)
    msg = lib.epg_last_error
    pv, bh = lib.epgf_gennorm_pvals, lib.epgf_bh_adjust
    assert pv(p, 0, p, p, p, None) == -1 and b"bad shape" in msg() and pv(None, 1 << 31, p, p, p, None) == -2 and b"2^31" in msg()
    for k, name in enumerate(("x", "params", "p", "flags")):
        a = [p, 10, p, p, p]
        a[(0, 2, 3, 4)[k]] = None
        assert pv(*a, None) == -1 and (name + " is NULL").encode() in msg(), name
    assert pv(None, 0, None, p, p, None) == -1 and b"bad shape" in msg() and pv(None, 10, None, p, p, None) == -1 and b"x is NULL" in msg()
    assert pv(p, 10, None, None, p, None) == -1 and b"params is NULL" in msg() and pv(p, 10, p, None, None, None) == -1 and b"p is NULL" in msg()
    assert bh(p, 0, p, p, p, 1 << 40, None) == -1 and b"bad shape" in msg() and bh(None, 1 << 31, p, p, p, 1 << 40, None) == -2 and b"2^31" in msg()
    for k, name in enumerate(("p", "adj", "flags", "ws")):
        a = [p, 10, p, p, p, 1 << 40]
        a[(0, 2, 3, 4)[k]] = None
        assert bh(*a, None) == -1 and (name + " is NULL").encode() in msg(), name
    assert bh(p, 10, p, p, ctypes.c_void_p((1 << 20) + 64), 0, None) == -1 and b"aligned" in msg()
    assert bh(None, 10, None, p, p, 0, None) == -1 and b"p is NULL" in msg() and bh(p, 10, None, None, p, 0, None) == -1 and b"adj is NULL" in msg()
    assert bh(p, 10, p, None, None, 0, None) == -1 and b"flags is NULL" in msg()
    assert bh(p, 10, p, p, None, 0, None) == -1 and b"ws is NULL" in msg()
    assert lib.epgf_bh_ws_bytes(0) == -1 and b"bad shape" in msg() and lib.epgf_bh_ws_bytes(1 << 31) == -1 and lib.epgf_bh_ws_bytes(-5) == -1


# ---- (c) the command line and STEP 4 ---------------------------------------------------------------------------------------------------
def test_the_two_usage_errors(capsys):
    msg = _cli_message(SINGLE + ["-n", "--pvals", "gpu"], capsys)
    assert msg is not None and "--pvals gpu" in msg and "paired" in msg
    msg = _cli_message(PAIRED + ["--pvals", "gpu"], capsys)
    assert msg is not None and "--pvals gpu" in msg and "--null-distribution" in msg


@pytest.mark.parametrize("args", [PAIRED + ["-n", "--pvals", "gpu"], PAIRED + ["-n", "--pvals", "host"], PAIRED + ["--pvals", "host"], SINGLE + ["--pvals", "host"],
                                  PAIRED + ["-n", "--pvals", "gpu", "--null-draws", "4"], PAIRED + ["-n", "--pvals", "gpu", "--fit", "gpu", "--null-seed", "7"],
                                  PAIRED + ["-n", "--pvals", "gpu", "--fit", "host"]])
def test_cli_accepts(args, capsys):
    msg = _cli_message(args, capsys)
    assert msg is None or "--pvals" not in msg


def test_help_names_the_option():
    from click.testing import CliRunner

    from epilogos_amd import run
    out = " ".join(CliRunner().invoke(run.main, ["-h"], terminal_width=200).output.split())
    assert "--pvals [host|gpu]" in out
    assert CliRunner().invoke(run.main, PAIRED + ["-n", "--pvals", "cpu"]).exit_code == 2


def _run_step4(tmp_path, res, **kw):
    np.save(tmp_path / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
    rv.mainFromArrays(res, _state_info(tmp_path), tmp_path, "t", 1, True, 3, 1000, tmp_path / "exp_freq_t.npy", 10, False, **kw)


def test_pvals_host_reaches_finish_unchanged(tmp_path, monkeypatch):
    """Without the option, and with pvals="host", _finish is called with the arguments it always had; pvals="gpu" adds one keyword."""
    res, _M = _results(np.random.default_rng(4), with_exceed=False)
    monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: (1.5, 0.0, 2.0))
    seen = []
    monkeypatch.setattr(rv, "_finish", lambda *a, **k: seen.append((len(a), sorted(k))))
    for kw in ({}, {"pvals": "host"}, {"fit": "host", "seed": 7, "pvals": "host"}):
        _run_step4(tmp_path, res, **kw)
    assert seen == [(12, ["empirical"])] * 3
    _run_step4(tmp_path, res, pvals="gpu")
    assert seen[-1] == (12, ["empirical", "pvals"])


def test_the_host_stage_is_the_default_and_an_unknown_one_is_refused(tmp_path, monkeypatch):
    res, _M = _results(np.random.default_rng(4), with_exceed=False)
    monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: (1.5, 0.0, 2.0))
    calls = []
    real_p, real_bh = rv.calculatePVals, rv.benjaminiHochberg
    monkeypatch.setattr(rv, "calculatePVals", lambda d, beta, loc, scale: calls.append(("p", len(d), beta, loc, scale)) or real_p(d, beta, loc, scale))
    monkeypatch.setattr(rv, "benjaminiHochberg", lambda p: calls.append(("bh", len(p))) or real_bh(p))
    monkeypatch.setattr(rv, "_pvalsGpu", lambda *a: (_ for _ in ()).throw(AssertionError("the device stage must not run")))
    _run_step4(tmp_path, res)
    _run_step4(tmp_path, res, pvals="host")
    assert calls == [("p", 301, 1.5, 0.0, 2.0), ("bh", 301)] * 2
    with pytest.raises(ValueError):
        _run_step4(tmp_path, res, pvals="cpu")


def test_a_flag_falls_back_to_the_host_with_one_warning(tmp_path, monkeypatch, capsys):
    res, _M = _results(np.random.default_rng(4), with_exceed=False)
    monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: (1.5, 0.0, 2.0))
    _run_step4(tmp_path, res)
    want = (tmp_path / "pairwiseMetrics_t.txt.gz").read_bytes()[8:]
    host_lines = [l for l in capsys.readouterr().out.splitlines() if "[Done]" in l]
    asked = []
    monkeypatch.setattr(rv, "_pvalsGpu", lambda d, params, empirical: asked.append((len(d), params, empirical)))       # -> None: a flag was set
    _run_step4(tmp_path, res, pvals="gpu")
    assert asked == [(301, (1.5, 0.0, 2.0), None)]
    out = capsys.readouterr().out.splitlines()
    assert len([l for l in out if "WARNING:" in l]) == 1 and "host" in [l for l in out if "WARNING:" in l][0]
    # the stage labels and [Done] marks of the host run, with the warning inside the first of the two stages
    text = "\n".join(out)
    assert text.count("[Done]") == len(host_lines)
    assert [l.split("\t")[0].strip() for l in host_lines] == [l.split("\t")[0].strip() for l in out if l.startswith("    ")]
    assert (tmp_path / "pairwiseMetrics_t.txt.gz").read_bytes()[8:] == want


def test_the_device_stage_s_values_are_what_is_written(tmp_path, monkeypatch):
    """pvals="gpu" with a stand-in for the device: what _pvalsGpu returns goes to the writers, and the host functions do not run;
    with exceedance counts in the results the stand-in is handed the host's empirical p-values."""
    import gzip
    for with_exceed in (False, True):
        res, M = _results(np.random.default_rng(4), with_exceed=with_exceed)
        monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: (1.5, 0.0, 2.0))
        boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the host stage must not run"))
        monkeypatch.setattr(rv, "calculatePVals", boom)
        monkeypatch.setattr(rv, "benjaminiHochberg", boom)
        seen = []

        def device(d, params, empirical):
            seen.append(empirical)
            return np.full(len(d), 0.25), np.full(len(d), 0.5)
        monkeypatch.setattr(rv, "_pvalsGpu", device)
        _run_step4(tmp_path, res, pvals="gpu")
        with gzip.open(tmp_path / "pairwiseMetrics_t.txt.gz", "rt") as fh:
            rows = [l.split("\t") for l in fh.read().splitlines()]
        assert len(rows) == 301 and all(r[6] == "2.50000e-01" and r[7] == "5.00000e-01" for r in rows)
        if with_exceed:
            e = np.concatenate([res[k]["nullExceed"] for k in ("matrix_chr1", "matrix_chr2", "matrix_chrX")])
            assert np.array_equal(seen[0], rv.empiricalPVals(e, M))
        else:
            assert seen == [None]
