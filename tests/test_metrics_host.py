"""`epilogos --roi [host|gpu]` and `--metrics [host|gpu]`, the host side (no GPU): the stand-alone program that holds the device's
"%.5e" arithmetic (csrc/epg_fmt_e5.h) against snprintf under the address and undefined-behaviour sanitizers; csrc/epg_metrics_text.h
against its binding table, type for type, the library's exports and the validation order of its entry point; the options on the
command line, their usage errors and their way down to STEP 4 (nothing is added for `host`); the `--roi gpu` path on CPU tensors with
the numpy restatements of tests/simsearch_pick_ref.py in place of the device steps, on the tie fixtures of tests/golden/roi.npz and
on vectors of two chromosomes."""
import ctypes
import re
import shutil
import subprocess

import numpy as np
import pytest

from epilogos_amd import _abi, build, roiAndVisualPairwise as rv, roiSingle
from tests import metrics_text_ref as mref
from tests import simsearch_pick_ref as pref
from tests.abi_headers import ctypes_of
from tests.conftest import load_golden
from tests.test_null_draws_host import _results, _state_info
from tests.test_writer_host import _build_program, _invoke, _matrix_dir, be  # noqa: F401  (be: the fixture)

NAMES = ["epgm_format_metrics", "epgm_format_ws_bytes", "epgm_text_bytes_max"]
ROOT = build.ROOT


# ---- (a) the stand-alone program -------------------------------------------------------------------------------------------------------
def test_the_e5_arithmetic_is_snprintf_s_under_the_sanitizers(tmp_path):
    exe = _build_program(tmp_path, "fmt_e5_check", [ROOT / "tests" / "fmt_e5_check.cpp"], [])
    res = subprocess.run([str(exe), "10000000"], capture_output=True, text=True)
    assert res.returncode == 0 and " 0 differ" in res.stdout, res.stdout + res.stderr
    m = re.search(r"fmt_e5_check: (\d+) values, (\d+) refused, (\d+) with a three-digit exponent", res.stdout)
    values, refused, three = (int(v) for v in m.groups())
    assert values - refused >= 10 ** 7 + 10 ** 5 and refused >= 14 and three > 10 ** 6, res.stdout


# ---- (b) the header and its binding ----------------------------------------------------------------------------------------------------
def header_prototypes(path):
    """name -> (return type, [parameter declarations]) of every epgm_ prototype of a header (the parser of tests/abi_headers.py, on a
    path and for this prefix)."""
    txt = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    txt = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", txt, flags=re.M)
    protos = {}
    for stmt in txt.split(";"):
        m = re.match(r"\s*(.*?)\b(epgm_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
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


def test_the_metrics_table_is_apart_from_the_other_registries():
    assert list(_abi.METRICS) == list(build.METRICS_HEADERS) == ["metrics_text"] and list(_abi._METRICS_TABLES) == ["metrics_text"]
    for reg in (_abi.HEADERS, _abi.INTERNAL, _abi.WRITER, _abi.READER, _abi._INTERNAL_TABLES, build.PUBLIC_HEADERS, build.INTERNAL_HEADERS,
                build.WRITER_HEADERS, build.READER_HEADERS):
        assert "metrics_text" not in reg
    header = _abi.METRICS["metrics_text"]
    assert header.path == build.CSRC / "epg_metrics_text.h" and header.path in build.HEADERS and "epg_metrics_text.hip" in build.SOURCES
    assert build.CSRC / "epg_fmt_e5.h" in build.HEADERS
    assert not list((build.ROOT / "include").glob("*metrics*"))
    for other in [*_abi.HEADERS.values(), *_abi.INTERNAL.values(), *_abi.WRITER.values(), *_abi.READER.values()]:
        assert not set(other.prototypes) & set(header.prototypes)
    text = header.path.read_text()
    assert "PACKAGE-INTERNAL" in text and "include/epilogos_metrics_text.h" in text and "tests/test_abi_symbols.py" in text
    assert _abi.header_constant_of(header, "EPGM_NAME_MAX") == 4096
    assert [_abi.header_constant_of(header, "EPGM_FLAG_" + k.upper()) for k in ("dist", "pval", "state", "chrom", "coord", "cap")] == list(mref.FLAG.values())


def test_header_and_binding_agree():
    header = _abi.METRICS["metrics_text"]
    protos = header_prototypes(header.path)
    assert sorted(protos) == sorted(header.prototypes) == NAMES
    for name, (res, args) in header.prototypes.items():
        ret, params = protos[name]
        assert res is ctypes_of(ret, returned=True), name
        assert len(args) == len(params), name
        for i, (a, p) in enumerate(zip(args, params)):
            assert a is ctypes_of(p), "%s: parameter %d is `%s` in the header, %s in the binding" % (name, i, p, a.__name__)
    assert protos["epgm_format_metrics"][1][-1] == "void* stream"


def test_library_exports_every_name(lib):
    fresh = ctypes.CDLL(str(_abi.lib_path()))
    for name in NAMES:
        fn = getattr(lib, name)
        assert hasattr(fresh, name) and fn.argtypes == _abi.METRICS["metrics_text"].prototypes[name][1]
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(_abi.lib_path())], capture_output=True, text=True).stdout
        assert set(NAMES) <= {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_argument_validation_in_the_header_s_order_without_gpu(lib):
    mref.check_validation_order(lib)


# ---- (c) the command line --------------------------------------------------------------------------------------------------------------
def test_the_options_and_their_usage_errors(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    log = tmp_path.parent / (tmp_path.name + "_io.log")
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    from click.testing import CliRunner

    from epilogos_amd import run
    out = " ".join(CliRunner().invoke(run.main, ["-h"], terminal_width=200).output.split())
    assert "--roi [host|gpu]" in out and "--metrics [host|gpu]" in out
    for opt in ("--roi", "--metrics"):
        res = _invoke(["-m", "paired", "-a", "x", "-b", "y", "-o", "o", "-j", "j", opt, "cpu"])
        assert res.exit_code == 2 and opt in res.output
    # --metrics gpu: paired mode only, refused before any file is read or any directory made
    for args in (["-i", "x"], ["-i", "x", "--roi", "gpu"], ["-i", "x", "--columns", "1-3"]):
        res = _invoke(args + ["-o", "o", "-j", "j", "--metrics", "gpu"])
        assert res.exit_code == 0 and res.output.strip() == "ERROR: [--metrics gpu] is only valid in paired mode", res.output
    assert not list(tmp_path.iterdir()) and not log.exists()
    # valid: --roi in both modes, --metrics in paired mode with and without -n; host anywhere
    for args in (["-i", "x", "--roi", "gpu"], ["-i", "x", "--roi", "host", "--metrics", "host"],
                 ["-m", "paired", "-a", "x", "-b", "y", "-n", "--metrics", "gpu", "--roi", "gpu"],
                 ["-m", "paired", "-a", "x", "-b", "y", "--metrics", "gpu"],
                 ["-m", "paired", "-a", "x", "-b", "y", "-n", "--null-draws", "3", "--pvals", "gpu", "--metrics", "gpu", "--roi", "gpu"]):
        res = _invoke(args + ["-o", "o", "-j", "j"])
        assert res.exit_code != 2 and "--metrics" not in res.output and "--roi" not in res.output, res.output


class _Stop(Exception):
    pass


@pytest.mark.parametrize("mode", ["single", "paired", "paired-n"])
def test_host_adds_nothing_to_the_calls(tmp_path, be, monkeypatch, mode):  # noqa: F811
    """Default and --roi host --metrics host: STEP 4 gets the arguments it always got and writes the same bytes; gpu adds roi="gpu" /
    metrics="gpu" and nothing else."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    d, states = _matrix_dir(tmp_path)
    args = ["-i", str(d), "-j", str(states), "-w", "3"]
    if mode != "single":
        args += ["-m", "paired", "--columns-a", "1-3", "--columns-b", "4-6", "--null-seed", "7"] + (["-n", "-t", "3"] if mode == "paired-n" else [])
    module, gpu = (roiSingle, ["--roi", "gpu"]) if mode == "single" else (rv, ["--roi", "gpu", "--metrics", "gpu"])
    seen = []
    real = module.mainFromArrays
    monkeypatch.setattr(module, "mainFromArrays", lambda *a, **k: seen.append((len(a), sorted(k))) or real(*a, **k))
    inner = []
    if mode == "single":
        real_txt = roiSingle.createTopScoresTxt
        monkeypatch.setattr(roiSingle, "createTopScoresTxt", lambda *a, **k: inner.append(sorted(k)) or real_txt(*a, **k))
    else:
        real_fin = rv._finish
        monkeypatch.setattr(rv, "_finish", lambda *a, **k: inner.append(sorted(k)) or real_fin(*a, **k))
    for k, extra in enumerate(([], ["--roi", "host"] + ([] if mode == "single" else ["--metrics", "host"]))):
        res = _invoke(args + ["-o", str(tmp_path / ("o%d" % k))] + extra)
        assert res.exit_code == 0 and "ERROR" not in res.output and "WARNING" not in res.output, res.output
    assert len(seen) == 2 and seen[0] == seen[1] and not {"roi", "metrics"} & set(seen[0][1])
    assert len(inner) == 2 and inner[0] == inner[1] and not {"roi", "metrics"} & set(inner[0])
    a, b = tmp_path / "o0", tmp_path / "o1"
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir())
    masked = lambda p: p.read_bytes()[:4] + b"\0\0\0\0" + p.read_bytes()[8:] if p.name.endswith(".gz") else p.read_bytes()      # (gzip MTIME)
    assert all(masked(b / p.name) == masked(p) for p in a.iterdir() if p.is_file())

    def stop(*a, **k):
        seen.append((len(a), sorted(k)))
        raise _Stop()
    monkeypatch.setattr(module, "mainFromArrays", stop)
    res = _invoke(args + ["-o", str(tmp_path / "o2")] + gpu)
    assert isinstance(res.exception, _Stop)
    assert seen[2] == (seen[0][0], sorted(seen[0][1] + ["roi"] + ([] if mode == "single" else ["metrics"])))


def test_step4_refuses_unknown_values(tmp_path):
    with pytest.raises(ValueError, match="roi"):
        roiSingle._maxMeanOn("cpu")
    with pytest.raises(ValueError, match="metrics"):
        rv._writeMetricsOn("cpu")


# ---- (d) --roi gpu on CPU tensors ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def on_cpu(monkeypatch):
    """numpy restatements in place of the device steps of similaritySearch_step1, the CPU in place of the device."""
    import torch

    from epilogos_amd import similaritySearch_max_mean as mm, similaritySearch_step1 as step1
    pref.install(monkeypatch, step1, mm)
    monkeypatch.setattr(step1, "deviceOf", lambda: torch.device("cpu"))
    return step1


@pytest.mark.parametrize("width", [7, 10])
def test_roi_gpu_writes_the_reference_s_tie_fixtures(tmp_path, on_cpu, width):
    r = load_golden("roi.npz")
    tie = r["tie_scores"]
    loc = np.array([["chr2", 200 * i, 200 * i + 200] for i in range(tie.shape[0])], dtype=object)
    for where in ("host", "gpu"):
        roiSingle.createTopScoresTxt(tmp_path / (where + ".txt"), loc, tie, r["state_names"], width, **roiSingle._roiOptions(where))
        assert (tmp_path / (where + ".txt")).read_bytes() == r["roi_tie_w%d" % width].tobytes(), where


def _two_chromosomes(n1, n2, seed, levels=None):
    rng = np.random.default_rng(seed)
    n = n1 + n2
    score = rng.integers(0, levels, size=n).astype(np.float64) if levels else rng.normal(size=n) ** 2
    chrom = np.array(["chr1"] * n1 + ["chr2"] * n2, dtype=object)
    start = np.concatenate([np.arange(n1), np.arange(n2)]) * 200
    return chrom, start, start + 200, score


@pytest.mark.parametrize("W", [2, 5, 50, 125])
@pytest.mark.parametrize("levels", [None, 3])
def test_roi_gpu_on_two_chromosomes_is_the_host_s(on_cpu, W, levels):
    """The boundary windows are masked on the host, the pick runs in the compacted index space: the same five arrays, with many ties
    (three score levels) and without."""
    chrom, start, end, score = _two_chromosomes(700, 450, W, levels)
    want = roiSingle.maxMean(chrom, start, end, score, W, 100)
    got = roiSingle.maxMeanDevice(chrom, start, end, score, W, 100)
    assert len(want[0]) > 0 and len(got) == 5
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    lo, hi = want[4] - W // 2, want[4] + W // 2 + (W % 2) - 1
    assert (chrom[lo] == chrom[hi]).all()                                       # no window spans the boundary
    # too short for one window: five empty arrays, as the host's
    none = roiSingle.maxMeanDevice(chrom[:W - 1], start[:W - 1], end[:W - 1], score[:W - 1], W, 100)
    assert len(none) == 5 and all(len(a) == 0 for a in none)


def test_roi_gpu_falls_back_with_one_warning(on_cpu, capsys):
    chrom, start, end, score = _two_chromosomes(3200, 900, 1)
    assert roiSingle.maxMeanDevice(chrom, start, end, score, 1025, 100) is None
    out = capsys.readouterr().out
    assert out.count("WARNING: [--roi gpu]") == 1 and "1024" in out and "host" in out
    widest = roiSingle.maxMeanDevice(chrom, start, end, score, 1024, 100)
    assert len(widest[0]) >= 1 and all(np.array_equal(a, b) for a, b in zip(widest, roiSingle.maxMean(chrom, start, end, score, 1024, 100)))
    assert capsys.readouterr().out == ""
    bad = score.copy()
    bad[77] = np.nan
    assert roiSingle.maxMeanDevice(chrom, start, end, bad, 50, 100) is None
    out = capsys.readouterr().out
    assert out.count("WARNING: [--roi gpu]") == 1 and "not finite" in out
    want = roiSingle.maxMean(chrom, start, end, score, 1025, 100)
    got = roiSingle._maxMeanOn("gpu")(chrom, start, end, score, 1025, 100)
    assert all(np.array_equal(a, b) for a, b in zip(want, got)) and capsys.readouterr().out.count("WARNING:") == 1


@pytest.mark.parametrize("pvalBool", [True, False])
def test_paired_step4_with_roi_gpu_writes_the_host_s_files(tmp_path, on_cpu, pvalBool):
    """roiAndVisualPairwise.mainFromArrays(roi="gpu") on hand-made arrays of three chromosomes: every file is the host's."""
    wrote = {}
    for where in ("host", "gpu"):
        res, _M = _results(np.random.default_rng(4), with_exceed=pvalBool)
        out = tmp_path / where
        out.mkdir()
        np.save(out / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
        rv.mainFromArrays(res, _state_info(tmp_path), out, "t", 1, pvalBool, 3, 200, out / "exp_freq_t.npy", 10, False, **roiSingle._roiOptions(where))
        wrote[where] = out
    names = sorted(p.name for p in wrote["host"].iterdir())
    assert names == sorted(p.name for p in wrote["gpu"].iterdir()) and "regionsOfInterest_t.txt" in names
    assert (wrote["host"] / "regionsOfInterest_t.txt").read_bytes() == (wrote["gpu"] / "regionsOfInterest_t.txt").read_bytes()
    assert (wrote["host"] / "regionsOfInterest_t.txt").stat().st_size > 0 or pvalBool
    assert (wrote["host"] / "pairwiseMetrics_t.txt.gz").read_bytes() == (wrote["gpu"] / "pairwiseMetrics_t.txt.gz").read_bytes()
