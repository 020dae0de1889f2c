"""--null-draws K, the host side (no GPU): the seeds of the K draws, the command line's refusals, the argument checks of
include/epilogos_nulldraws.h (tests/test_abi_symbols.py holds it against its binding), and STEP 4 on exceedance counts -- empirical p-values
(1 + e) / (1 + M), Benjamini-Hochberg of them, today's three files, no fit."""
import gzip
import shutil

import numpy as np
import pytest

from epilogos_amd import _abi, _io, build
from epilogos_amd import roiAndVisualPairwise as rv
from epilogos_amd.helpers import null_draw_seeds


# ---------------------------------------------------------------------------------------------------------- seeds
def _splitmix(seed, k):
    m = (1 << 64) - 1
    z = (seed + k * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_seeds_fixed_values():
    # splitmix64 from the state 0 gives 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F (its published test vector);
    # entry k of seed s is output k of the state s, and the golden-ratio seed's entry k is output k + 1 of the state 0
    a = null_draw_seeds(0, 4)
    assert a.dtype == np.uint64 and a.shape == (4,)
    assert [int(x) for x in a] == [0, 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    b = null_draw_seeds(0x9E3779B97F4A7C15, 3)
    assert [int(x) for x in b] == [0x9E3779B97F4A7C15, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    c = null_draw_seeds(77, 3)
    assert [int(x) for x in c] == [77, 0x6258CBE07C1FF081, 0x7E54A4883A969E54]


@pytest.mark.parametrize("seed", [0, 5, 77, 20240229, (1 << 64) - 1, (1 << 63) + 12345])
def test_seeds_entry_zero_and_distinct(seed):
    s = null_draw_seeds(seed, 100)
    assert int(s[0]) == seed
    assert len(set(int(x) for x in s)) == 100
    assert [int(x) for x in s[1:]] == [_splitmix(seed, k) for k in range(1, 100)]
    assert np.array_equal(null_draw_seeds(seed, 7), s[:7])                 # a prefix: entry k does not depend on K
    assert null_draw_seeds(seed, 1).tolist() == [seed]


# ---------------------------------------------------------------------------------------------------------- command line
def _cli_message(args, capsys):
    """The ERROR line of a command that is refused before any path is looked at, or None when that stage lets it through (the
    command then fails later on its missing directories)."""
    from epilogos_amd import run
    try:
        run.main(args=args, standalone_mode=False)
    except SystemExit:
        pass
    except Exception:
        pass
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("ERROR")]
    return lines[0] if lines else None


PAIRED = ["-m", "paired", "-a", "/nonexistent/a", "-b", "/nonexistent/b", "-o", "/nonexistent/o", "-j", "/nonexistent/j"]
SINGLE = ["-i", "/nonexistent/i", "-o", "/nonexistent/o", "-j", "/nonexistent/j"]


def test_cli_needs_null_distribution(capsys):
    msg = _cli_message(PAIRED + ["--null-draws", "4"], capsys)
    assert msg is not None and "--null-draws" in msg and "--null-distribution" in msg


def test_cli_needs_paired_mode(capsys):
    msg = _cli_message(SINGLE + ["-n", "--null-draws", "4"], capsys)
    assert msg is not None and "--null-draws" in msg and "paired" in msg


def test_cli_refuses_several_gpus(capsys, monkeypatch):
    monkeypatch.setenv("EPILOGOS_LAUNCH_DRYRUN", "1")                       # (were it let through, nothing would be started)
    msg = _cli_message(PAIRED + ["-n", "--null-draws", "4", "--gpus", "2"], capsys)
    assert msg is not None and "--null-draws" in msg and "one GPU" in msg


def test_cli_refuses_less_than_one(capsys):
    msg = _cli_message(PAIRED + ["-n", "--null-draws", "0"], capsys)
    assert msg is not None and "--null-draws" in msg


@pytest.mark.parametrize("args", [PAIRED + ["--null-draws", "1"], PAIRED + ["-n", "--null-draws", "1"], SINGLE + ["--null-draws", "1"],
                                  SINGLE + ["-n", "--null-draws", "1"], PAIRED + ["-n", "--null-draws", "4"],
                                  PAIRED + ["-n", "--null-draws", "4", "-t", "3", "-z", "10"]])
def test_cli_accepts(args, capsys):
    msg = _cli_message(args, capsys)
    assert msg is None or "--null-draws" not in msg


def test_help_names_the_option_and_the_unused_ones():
    from click.testing import CliRunner

    from epilogos_amd import run
    out = " ".join(CliRunner().invoke(run.main, ["-h"], terminal_width=200).output.split())
    assert "--null-draws" in out
    assert out.count("accepted and unused with --null-draws") == 2           # -t and -z


# ---------------------------------------------------------------------------------------------------------- the header
@pytest.fixture(scope="module")
def lib():
    if build.is_stale():
        if shutil.which("hipcc") is None:
            pytest.skip("hipcc not available and library not prebuilt")
        build.build_library()
    return _abi.load()


def test_abi_version_is_unchanged(lib):
    assert lib.epg_version() == 2


def test_draws_argument_checks_without_gpu(lib):
    f = lib.epg_null_dist_draws_parts
    ok = dict(nparts=0, S=18, NA=379, NB=342, ga=379, gb=342, K=3)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["nparts"], None, None, None, None, None, a["S"], a["NA"], a["NB"], a["ga"], a["gb"], None, None, None, a["K"], None, None)
    for bad in (dict(nparts=-1), dict(S=0), dict(S=128), dict(NA=0), dict(NB=0), dict(K=0), dict(ga=0), dict(gb=0), dict(ga=400, gb=400)):
        assert call(**bad) == -1, bad
    # unsupported shapes are refused before any pointer is looked at
    assert call(S=40) == -2 and b"31 states" in lib.epg_last_error()
    assert call(NA=3000, NB=3001, ga=3000, gb=3001) == -2 and b"bit-string" in lib.epg_last_error()
    assert call(NA=1000, NB=1000, ga=100, gb=100) == -2                      # two strings: at most 1536 columns
    assert call(S=31, NA=1500, NB=1500, ga=1500, gb=1500) == -2 and b"LDS" in lib.epg_last_error()   # 372 KB of tables
    assert call() == -1 and b"NULL" in lib.epg_last_error()                  # the flagship shape is taken: the seeds are missing


def test_exceed_argument_checks_without_gpu(lib):
    assert lib.epg_null_exceed_ws_bytes(-1) == -1
    assert lib.epg_null_exceed_ws_bytes(1 << 31) == -1
    assert lib.epg_null_exceed(None, -1, None, 5, None, None, 0, None) == -1
    assert lib.epg_null_exceed(None, 5, None, -1, None, None, 0, None) == -1
    assert lib.epg_null_exceed(None, 0, None, 5, None, None, 0, None) == 0   # nothing to count
    assert lib.epg_null_exceed(None, 5, None, 5, None, None, 0, None) == -1 and b"NULL" in lib.epg_last_error()


# ---------------------------------------------------------------------------------------------------------- STEP 4
def _results(rng, with_exceed=True):
    """Three chromosomes of hand-made arrays, as driver.run_paired_groups hands them to STEP 4."""
    res, M = {}, 4 * 290
    for name, R in (("chr1", 200), ("chr2", 61), ("chrX", 40)):
        loc = np.array([[name, 1000 + 200 * i, 1200 + 200 * i] for i in range(R)], dtype=object)
        e = rng.integers(0, M + 1, size=R).astype(np.int64)
        e[:5] = 0                                                            # the smallest attainable p
        e[5] = M
        d = rng.normal(size=R).astype(np.float32) * 3
        entry = {"chrName": name, "locations": _io.Locations.from_object_array(loc), "nullDistances": rng.normal(size=R).astype(np.float32),
                 "quiescenceArr": rng.random(R) < 0.1, "distances": d, "maxDiff": rng.integers(1, 4, size=R).astype(np.int32)}
        if with_exceed:
            entry.update(nullExceed=e, nullPool=M)
        res["matrix_" + name] = entry
    return res, M


def _state_info(tmp):
    p = tmp / "metadata.tsv"
    p.write_text("zero_index\tshort_name\n" + "".join("{}\tstate{}\n".format(i, i + 1) for i in range(3)))
    return p


def test_step4_uses_the_exceedance_counts(tmp_path, monkeypatch):
    res, M = _results(np.random.default_rng(3))

    def no_fit(*a, **k):
        raise AssertionError("the gennorm fit must not run when the results carry exceedance counts")
    monkeypatch.setattr(rv, "_fitParams", no_fit)
    monkeypatch.setattr(rv, "fitOnSubSample", no_fit)
    monkeypatch.setattr(rv, "calculatePVals", no_fit)
    np.save(tmp_path / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
    rv.mainFromArrays(res, _state_info(tmp_path), tmp_path, "t", 1, True, 101, 100000, tmp_path / "exp_freq_t.npy", 10, False)
    assert not (tmp_path / "exp_freq_t.npy").exists()
    order = ["matrix_chr1", "matrix_chr2", "matrix_chrX"]
    e = np.concatenate([res[k]["nullExceed"] for k in order])
    d = np.concatenate([res[k]["distances"] for k in order])
    p = (1.0 + e.astype(np.float64)) / (1.0 + M)
    assert p.min() == 1.0 / (1 + M) and p.max() == 1.0
    assert np.array_equal(rv.empiricalPVals(e, M), p)
    bh = rv.benjaminiHochberg(p)
    with gzip.open(tmp_path / "pairwiseMetrics_t.txt.gz", "rt") as fh:
        rows = [l.split("\t") for l in fh.read().splitlines()]
    assert len(rows) == len(e) and all(len(r) == 8 for r in rows)            # chr, start, end, state, |d|, sign, p, BH p
    assert [r[6] for r in rows] == ["%.5e" % x for x in p]
    assert [r[7] for r in rows] == ["%.5e" % x for x in bh]
    assert [r[4] for r in rows] == ["%.5f" % abs(float(x)) for x in d]
    assert [r[0] for r in rows[:200]] == ["chr1"] * 200 and rows[-1][0] == "chrX"
    with gzip.open(tmp_path / "significantLoci_t.txt.gz", "rt") as fh:
        sig = [l.split("\t") for l in fh.read().splitlines()]
    assert len(sig) == int((bh <= 0.1).sum()) and all(len(r) == 9 for r in sig)
    roi = [l.split("\t") for l in (tmp_path / "regionsOfInterest_t.txt").read_text().splitlines()]
    assert all(len(r) == 9 for r in roi)


def test_step4_without_counts_still_fits(tmp_path, monkeypatch):
    res, _M = _results(np.random.default_rng(4), with_exceed=False)
    called = []
    monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: called.append(1) or (1.5, 0.0, 2.0))
    np.save(tmp_path / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
    rv.mainFromArrays(res, _state_info(tmp_path), tmp_path, "t", 1, True, 3, 100000, tmp_path / "exp_freq_t.npy", 10, False)
    assert called == [1]
    with gzip.open(tmp_path / "pairwiseMetrics_t.txt.gz", "rt") as fh:
        assert all(len(l.split("\t")) == 8 for l in fh.read().splitlines())


def test_main_reads_the_side_car(tmp_path, monkeypatch):
    """main() on the files a run with keep_temps leaves: temp_nullExceed_* next to temp_pairMetrics_* -> the same p-values, no fit;
    the side-cars are removed with the other temporaries."""
    from tests.fake_backend import OracleBackend
    res, M = _results(np.random.default_rng(5))
    monkeypatch.setattr(rv, "_fitParams", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fit")))
    for stem, v in res.items():
        R = len(v["distances"])
        _io.write_scores(tmp_path / "pairwiseDelta_t_{}.txt.gz".format(stem), v["locations"], np.zeros((R, 3), dtype=np.float32))
        starts, ends = v["locations"].start_end()
        np.savez_compressed(tmp_path / "temp_pairMetrics_t_{}.npz".format(stem), chrName=np.array([v["chrName"]]), distances=v["distances"],
                            maxDiff=v["maxDiff"], starts=starts, ends=ends)
        np.savez_compressed(tmp_path / "temp_nullDistances_t_{}.npz".format(stem), chrName=np.array([v["chrName"]]), nullDistances=v["nullDistances"])
        np.savez_compressed(tmp_path / "temp_quiescence_t_{}.npz".format(stem), chrName=np.array([v["chrName"]]), quiescenceArr=v["quiescenceArr"])
        np.savez_compressed(tmp_path / "temp_nullExceed_t_{}.npz".format(stem), chrName=np.array([v["chrName"]]), nullExceed=v["nullExceed"],
                            nullPool=np.array([M], dtype=np.int64))
    np.save(tmp_path / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
    rv.main("A", "B", _state_info(tmp_path), tmp_path, "t", 1, True, False, 3, 100000, tmp_path / "exp_freq_t.npy", 10, False,
            backend=OracleBackend())
    assert not list(tmp_path.glob("temp_*.npz"))
    e = np.concatenate([res[k]["nullExceed"] for k in ("matrix_chr1", "matrix_chr2", "matrix_chrX")])
    with gzip.open(tmp_path / "pairwiseMetrics_t.txt.gz", "rt") as fh:
        got = [l.split("\t")[6] for l in fh.read().splitlines()]
    assert got == ["%.5e" % x for x in (1.0 + e) / (1.0 + M)]
