"""`simsearch -b --step1 gpu`, the host side (no GPU; tests/test_abi_symbols.py holds include/epilogos_simsearch_pick.h against
its binding): the header's tile constants, the argument checks made before the first HIP call, cli()'s handling of --step1, the
STEP 1 child of a --gpus N build, and similaritySearch_step1's orchestration -- shifts, masks, compaction, final order,
coordinates -- against similaritySearch_max_mean with numpy restatements (tests/simsearch_pick_ref.py) in place of the device steps."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import _abi
from epilogos_amd import roiSingle
from epilogos_amd import similaritySearch_max_mean as mm
from epilogos_amd import similaritySearch_run as run
from tests import simsearch_pick_ref as ref

ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests" / "golden" / "simsearch.npz")


# ---- the header --------------------------------------------------------------------------------------------------------------------

def test_a_tile_and_its_halos_fit_the_lds():
    """(tests/test_abi_symbols.py holds the header against its binding and the library's exports.)"""
    T, maxW = _abi.header_constant("simsearch_pick", "EPG_PICK_TILE"), _abi.header_constant("simsearch_pick", "EPG_PICK_MAX_W")
    assert T % 256 == 0 and 3 * 4 * (T + 2 * (maxW - 1)) <= 48 * 1024            # key, prefix and suffix of a tile and its halos


def test_argument_validation_without_gpu():
    lib = _abi.load()
    x = ctypes.c_void_p(4096)
    launches = ctypes.c_int32(-5)
    assert lib.epg_simsearch_rowscore(x, -1, 15, x, None) == -1 and b"bad shape" in lib.epg_last_error()
    assert lib.epg_simsearch_rowscore(x, 10, 0, x, None) == -1
    assert lib.epg_simsearch_rowscore(None, 10, 15, x, None) == -1 and b"NULL" in lib.epg_last_error()
    assert lib.epg_simsearch_rowscore(None, 0, 15, None, None) == 0
    assert lib.epg_simsearch_rolling_max(x, -1, 5, x, None) == -1
    assert lib.epg_simsearch_rolling_max(x, 10, 0, x, None) == -1
    assert lib.epg_simsearch_rolling_max(x, 10, 1025, x, None) == -2 and b"1024" in lib.epg_last_error()
    assert lib.epg_simsearch_rolling_max(x, 10, 5, None, None) == -1
    assert lib.epg_simsearch_rolling_max(None, 0, 5, None, None) == 0
    assert lib.epg_simsearch_rank_ws_bytes(-1) == -1 and lib.epg_simsearch_rank_ws_bytes(2 ** 31) == -1
    assert lib.epg_simsearch_rank_ws_bytes(0) >= 0 and lib.epg_simsearch_rank_ws_bytes(1000) >= 24 * 1000
    assert lib.epg_simsearch_rank(x, x, x, -1, x, x, 1 << 20, None) == -1
    assert lib.epg_simsearch_rank(x, None, x, 10, x, x, 1 << 20, None) == -1 and b"NULL" in lib.epg_last_error()
    assert lib.epg_simsearch_rank(x, x, x, 10, x, ctypes.c_void_p(4100), 1 << 20, None) == -1 and b"aligned" in lib.epg_last_error()
    assert lib.epg_simsearch_rank(x, x, x, 10, x, x, 8, None) == -4
    assert lib.epg_simsearch_rank(None, None, None, 0, None, None, 0, None) == 0
    assert lib.epg_simsearch_pick_ws_bytes(-1, 25) == -1 and lib.epg_simsearch_pick_ws_bytes(10, 0) == -1
    assert lib.epg_simsearch_pick_ws_bytes(10, 1025) == -2
    assert lib.epg_simsearch_pick_ws_bytes(1000, 25) >= 3 * 1000
    lb = ctypes.byref(launches)
    assert lib.epg_simsearch_pick(x, -1, 25, 5, x, x, lb, x, 1 << 20, None) == -1
    assert lib.epg_simsearch_pick(x, 10, 0, 5, x, x, lb, x, 1 << 20, None) == -1
    assert lib.epg_simsearch_pick(x, 10, 2000, 5, x, x, lb, x, 1 << 20, None) == -2
    assert lib.epg_simsearch_pick(x, 10, 25, -1, x, x, lb, x, 1 << 20, None) == -1 and b"maxRegions" in lib.epg_last_error()
    assert lib.epg_simsearch_pick(None, 10, 25, 5, x, x, lb, x, 1 << 20, None) == -1 and b"NULL" in lib.epg_last_error()
    assert lib.epg_simsearch_pick(x, 10, 25, 5, x, x, None, x, 1 << 20, None) == -1
    assert lib.epg_simsearch_pick(x, 10, 25, 5, x, x, lb, ctypes.c_void_p(4100), 1 << 20, None) == -1 and b"aligned" in lib.epg_last_error()
    assert lib.epg_simsearch_pick(x, 10, 25, 5, x, x, lb, x, 8, None) == -4
    assert launches.value == -5                                                 # a refused call writes nothing


# ---- the restatement itself --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 2, 5, 24, 25])
def test_restated_walk_rank_and_rolling_max_are_maxmeans(W):
    """maxMean on a vector with ties and a plateau picks what the restatement's rank and walk pick."""
    from epilogos_amd import _io
    rng = np.random.default_rng(W)
    R = 700
    score = np.round(rng.normal(size=R), 1)
    score[300:420] = 0.5
    chrom, start = np.array(["chr1"] * R, dtype=object), np.arange(R) * 200
    h = W // 2
    e_off = h if W % 2 else h - 1
    sc = score[h:R - e_off]
    assert np.array_equal(ref.rolling_max(sc, W), _io.rolling_max(sc, W), equal_nan=True)
    import pandas as pd
    rmax, rmean = ref.rolling_max(sc, W), pd.Series(sc).rolling(W, center=True).mean().to_numpy()
    keep = np.nonzero(~np.isnan(rmax))[0]
    for cap in (3, R):
        *_x, orig = roiSingle.maxMean(chrom, start, start + 200, score, W, cap)
        got = keep[ref.pick(ref.lexsort_rank(rmax[keep], rmean[keep], sc[keep]), W, cap)] + h
        assert np.array_equal(np.sort(orig), got)


def test_rank_patterns_are_permutations():
    T = 64
    for name in ref.PATTERNS:
        for n in (1, 5, T - 1, T, T + 1, 3 * T + 7):
            assert np.array_equal(np.sort(ref.pattern(name, n, 5, T)), np.arange(n)), (name, n)
    assert ref.pattern("best_first_of_tile", 3 * T + 7, 5, T)[T] == 0 and ref.pattern("best_last_of_tile", 3 * T + 7, 5, T)[T - 1] == 0


# ---- cli() ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def captured(monkeypatch):
    calls = []
    monkeypatch.setattr(run, "buildSimSearch", lambda *a, **k: calls.append((a, k)))
    return calls


def test_step1_defaults_to_host_and_gpu_reaches_the_build(tmp_path, captured):
    base = ["-b", "-s", "x.txt", "-o", str(tmp_path)]
    for argv in (base, base + ["--step1", "host"], ["--step1=gpu"] + base, base[:3] + ["--step1", "gpu"] + base[3:],
                 base + ["--gpus", "3", "--step1", "gpu"]):
        with pytest.raises(SystemExit) as e:
            run.cli(argv)
        assert e.value.code == 0
    assert [k["step1"] for _a, k in captured] == ["host", "host", "gpu", "gpu", "gpu"]
    assert [k["gpus"] for _a, k in captured] == [1, 1, 1, 1, 3]
    assert "--step1" not in [o for p in run.main.params for o in p.opts]         # main's options stay the reference's


@pytest.mark.parametrize("value", ["device", "", "GPU", None])
def test_other_step1_values_are_refused(tmp_path, captured, capsys, value):
    argv = ["-b", "-s", "x.txt", "-o", str(tmp_path)] + (["--step1", value] if value is not None else ["--step1"])
    with pytest.raises(SystemExit) as e:
        run.cli(argv)
    assert e.value.code == 2 and "--step1 takes one of host, gpu" in capsys.readouterr().err and not captured


def test_step1_with_query_is_refused(tmp_path, captured, capsys):
    with pytest.raises(SystemExit) as e:
        run.cli(["--step1", "gpu", "-q", "chr1:1-2", "-m", "x.bed.gz", "-o", str(tmp_path)])
    assert e.value.code == 2 and "--step1 applies to -b only" in capsys.readouterr().err and not captured


def test_build_refuses_other_step1_values(tmp_path):
    with pytest.raises(ValueError, match="step1"):
        run.buildSimSearch("x.txt", tmp_path, 25000, 10, 1, 100, -1, -1, gpus=1, step1="device")
    assert not list(tmp_path.iterdir())


def test_three_gpus_run_step1_as_one_child_first(tmp_path, monkeypatch):
    """--gpus 3 --step1 gpu with a recording runChildren: one STEP 1 job on LOCAL_RANK 0, then the three STEP 2 jobs; the parent
    imports neither the device path nor torch's GPU side."""
    from epilogos_amd import _io
    from epilogos_amd import similaritySearch_write as wr
    monkeypatch.setenv("EPILOGOS_DIST_BACKEND", "gloo")
    monkeypatch.setattr(_io, "node_cores", lambda: 16)
    monkeypatch.setattr(wr, "main", lambda *a: None)
    sp = tmp_path / "scores.txt"
    sp.write_bytes(GOLD["s200_scores_txt"].tobytes())
    out = tmp_path / "o"
    out.mkdir()
    handed = []

    def record(jobs, **kw):
        handed.append((jobs, kw, "epilogos_amd.similaritySearch_step1" in sys.modules))
    monkeypatch.setattr(run, "runChildren", record)
    sys.modules.pop("epilogos_amd.similaritySearch_step1", None)
    run.buildSimSearch(sp, out, 25000, 10, 8, 100, 0, 2.5, gpus=3, step1="gpu")
    assert [len(jobs) for jobs, _kw, _imp in handed] == [1, 3]
    (argv, env), = handed[0][0]
    assert argv == [sys.executable, "-m", "epilogos_amd.similaritySearch_step1", str(out.resolve()), str(sp.resolve()), "125", "5", "25000",
                    "0", "2.5"]
    assert env["LOCAL_RANK"] == "0" and env["OMP_NUM_THREADS"] == "8" and env["PYTHONPATH"].split(":")[0] == str(ROOT)
    assert handed[0][1] == {"step": "STEP 1"}
    assert [a[2] for a, _e in handed[1][0]] == ["epilogos_amd.similaritySearch_calc"] * 3
    assert [e["LOCAL_RANK"] for _a, e in handed[1][0]] == ["0", "1", "2"]
    assert not any(imp for _jobs, _kw, imp in handed) and "epilogos_amd.similaritySearch_step1" not in sys.modules


def test_a_failed_step1_child_is_named_as_step1():
    jobs = [([sys.executable, "-c", "import sys; sys.stderr.write('no device\\n'); sys.exit(4)"], None)]
    with pytest.raises(SystemExit) as e:
        run.runChildren(jobs, step="STEP 1")
    assert "STEP 1 child 0 of 1 exited with status 4" in str(e.value.code) and "no device" in str(e.value.code)


# ---- the orchestration against today's STEP 1 ----------------------------------------------------------------------------------------

def _same_arrays(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype == object:
        assert all(x == y and type(x) is type(y) for x, y in zip(a.reshape(-1), b.reshape(-1)))
    else:
        assert a.tobytes() == b.tobytes()                               # the values bit for bit (C order, whatever the layout)


def _both(tmp_path, monkeypatch, sp, windowBP, filterState=-1, filterScore=-1):
    from epilogos_amd import similaritySearch_step1 as step1
    ref.install(monkeypatch, step1, mm)
    windowBP, windowBins, blockSize = run.windowParameters(sp, windowBP)
    dirs = []
    for name, fn in (("host", mm.main), ("dev", step1.main)):
        d = tmp_path / name
        d.mkdir()
        fn(d, sp, windowBins, blockSize, windowBP, filterState, filterScore)
        dirs.append(d)
    assert sorted(p.name for p in dirs[1].iterdir()) == sorted(p.name for p in dirs[0].iterdir()) == \
        ["genome_stats.npz", "reduced_genome.npy", "simsearch_cube.npz"]
    for f in ("genome_stats.npz", "simsearch_cube.npz"):
        a, b = np.load(dirs[0] / f, allow_pickle=True), np.load(dirs[1] / f, allow_pickle=True)
        assert sorted(a.files) == sorted(b.files) == ["coords", "scores"]
        for k in a.files:
            _same_arrays(a[k], b[k])
    assert (dirs[0] / "reduced_genome.npy").read_bytes() == (dirs[1] / "reduced_genome.npy").read_bytes()
    return np.load(dirs[1] / "simsearch_cube.npz", allow_pickle=True)["coords"]


@pytest.mark.parametrize("case", ["s200", "s20"])
def test_orchestration_writes_the_host_arrays_golden(tmp_path, monkeypatch, case):
    sp = tmp_path / "scores.txt"
    sp.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    coords = _both(tmp_path, monkeypatch, sp, int(GOLD[case + "_windowBP"]))
    assert len(coords) == len(GOLD[case + "_cube_coords"])


@pytest.mark.parametrize("filters", [(-1, -1), (0, -1), (3, 1.5)])
def test_orchestration_writes_the_host_arrays_plateau(tmp_path, monkeypatch, filters):
    """6 000 bins by 15 states, two chromosomes, 1 500 identical rows, the chromosome change inside a window."""
    sp = tmp_path / "plateau.txt"
    sp.write_bytes(ref.plateau_scores_text())
    coords = _both(tmp_path, monkeypatch, sp, -1, *filters)
    if filters == (0, -1):
        assert {"chr1", "chr2"} == set(coords[:, 0]) and len(coords) > 20
        ends = coords[coords[:, 0] == "chr1"][:, 2].astype(np.int64)
        assert ends.max() <= 2937 * 200                                        # no window runs over the chromosome change


def test_too_few_bins_for_a_window(tmp_path, monkeypatch):
    sp = tmp_path / "short.txt"
    sp.write_bytes(b"".join(GOLD["s200_scores_txt"].tobytes().splitlines(keepends=True)[:100]))
    assert len(_both(tmp_path, monkeypatch, sp, 25000)) == 0
