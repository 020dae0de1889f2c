"""`epilogos --chromhmm DIR`, the host side (no GPU): the usage errors of the new options -- printed before a file is read or a
directory made, and silent for every command line without them -- the default tag and the run order of the built matrices
(natural key of `matrix_{chr}.epgm`, not the order of the chromsizes file), and driver.run_groupings(resident=...) over the stand-in
backend of tests/groupings_backend.py with numpy arrays as the "device" matrices: no reader starts, nothing is parsed or
"uploaded", and the outputs are those of the same call on .epgm files written from the same arrays."""
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import backend, driver, helpers, stateByLine as sbl
from tests.groupings_backend import GroupingsBackend
from tests.test_groupings_host import same_tree

S = 5
SIZES_ORDER = ["chr10", "chr2", "chr1", "chrX"]                  # the chromsizes file's order
RUN_ORDER = ["chr1", "chr2", "chr10", "chrX"]                    # the order `-i` runs matrix_{chr}.epgm in
ROWS = {"chr10": 9, "chr2": 23, "chr1": 1, "chrX": 14}
N = 6


def _invoke(args, **env):
    from click.testing import CliRunner
    from epilogos_amd import run
    return CliRunner().invoke(run.main, args, env=env or None)


@pytest.fixture()
def be():
    b = GroupingsBackend()
    backend.set_for_testing(b)
    yield b
    backend.set_for_testing(None)
    driver.finish_writes()


def _states_file(path):
    path.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    return path


# ---- the command line's refusals ---------------------------------------------------------------------------------------------

def test_usage_errors_before_anything_is_read_or_made(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                        # relative paths everywhere: nothing may appear here
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    log = tmp_path.parent / (tmp_path.name + "_io.log")
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    tail = ["-o", "o", "-j", "j"]
    full = ["--chromhmm", "d", "--metadata", "m", "--chromsizes", "c"]

    def refused(args, *words, **env):
        out = _invoke(args + tail, **env).output
        assert out.startswith("ERROR: [--chromhmm] ") and out.count("\n") == 1, out
        for w in words:
            assert w in out, out
    refused(full + ["-i", "x"], "[-i]")
    refused(full + ["-m", "paired", "-a", "x"], "[-a]")
    refused(full + ["-m", "paired", "-b", "x"], "[-b]")
    refused(["--chromhmm", "d", "--chromsizes", "c"], "requires [--metadata]")
    refused(["--chromhmm", "d", "--metadata", "m"], "requires [--chromsizes]")
    for opt in (["--metadata", "m"], ["--chromsizes", "c"], ["--segments"], ["--bin-width", "100"], ["--state-names", "n"],
                ["--keep-matrices", "k"]):
        refused(["-i", "x"] + opt, "is required with [%s]" % opt[0])
    refused(full + ["--bin-width", "100"], "[--bin-width] goes with [--segments]")
    refused(full + ["--state-names", "n"], "[--state-names] goes with [--segments]")
    refused(full + ["-m", "paired"], "[--columns-a] and [--columns-b]", "[--groupings]")
    refused(full + ["--cache-dir", "cache"], "[--cache-dir]", "no parsed text to cache")
    refused(full + ["--gpus", "2"], "one GPU", "several ranks", "[--gpus 1]")
    refused(full + ["--gpus", "0"], "one GPU")
    refused(full, "one GPU", "several ranks", WORLD_SIZE="2")
    assert not list(tmp_path.iterdir()) and not log.exists()


def test_command_lines_without_the_options_do_not_hear_of_them(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    assert _invoke(["-o", "o", "-j", "j"]).output == "ERROR: [-i, --input-directory] is required in single mode\n"
    assert _invoke(["-m", "paired", "-a", "y", "-o", "o", "-j", "j"]).output == \
        "ERROR: [-a, --directory-one] and [-b, --directory-two] are required in paired mode\n"
    assert _invoke(["-i", "x", "--null-draws", "0", "-o", "o", "-j", "j"]).output == "ERROR: [--null-draws] must be at least 1\n"
    # with the option and its usage in order: on to today's checks and messages
    full = ["--chromhmm", "d", "--metadata", "m", "--chromsizes", "c"]
    assert _invoke(full + ["-j", "j"]).output == "ERROR: [-o, --output-directory] is required\n"
    assert _invoke(full + ["-m", "paired", "--columns-a", "1", "-o", "o", "-j", "j"]).output == \
        "ERROR: [--columns-a] and [--columns-b] must be given together\n"
    assert not list(tmp_path.iterdir())


def test_help_lists_the_options():
    out = " ".join(_invoke(["--help"]).output.split())
    for opt in ("--chromhmm", "--metadata", "--chromsizes", "--segments", "--bin-width", "--state-names", "--keep-matrices"):
        assert opt in out


# ---- the command over a stand-in builder and backend: default tag, run order ---------------------------------------------------

@pytest.fixture()
def calls(tmp_path):
    """A directory of state-by-line calls named `roadmap`: N biosamples x the chromosomes of SIZES_ORDER, one more biosample in the
    metadata without files and one more chromosome in the sizes that no file holds.  -> (dir, metadata, sizes, {chr: int8 [R, N]})."""
    rng = np.random.default_rng(44)
    d = tmp_path / "roadmap"
    d.mkdir()
    mats = {}
    for c in SIZES_ORDER:
        v = rng.integers(1, S + 1, size=(ROWS[c], N))
        for k in range(N):
            (d / ("B%03d_5_%s_statebyline.txt" % (k, c))).write_bytes(
                b"B%03d\t%s\nMaxStateE\n" % (k, c.encode()) + "".join("%d\n" % s for s in v[:, k]).encode())
        mats[c] = (v - 1).astype(np.int8)
    meta = tmp_path / "meta.txt"
    meta.write_text("id\n" + "".join("B%03d\n" % k for k in range(N)) + "B999\n")
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join("%s\t%d\n" % (c, ROWS.get(c, 83) * 200) for c in SIZES_ORDER[:2] + ["chrM"] + SIZES_ORDER[2:]))
    return d, meta, sizes, mats


def _numpy_builder(monkeypatch):
    """stateByLine.build_matrix_device stood in for by numpy (the padded layout, a host array)."""
    from epilogos_amd import engine
    from tests.test_statebyline_host import numpy_matrix

    def build(files):
        x, chrom = numpy_matrix([Path(f).read_bytes() for f in files])
        X = np.full((x.shape[0], engine.padded_width(x.shape[1])), -1, dtype=np.int8)
        X[:, :x.shape[1]] = x
        return X, x.shape[1], chrom, (int(x.min()) + 1, int(x.max()) + 1)
    monkeypatch.setattr(engine, "require_gpu", lambda: None)
    monkeypatch.setattr(sbl, "build_matrix_device", build)


def _epgm_dir(d, mats):
    d.mkdir(parents=True)
    for c, x in mats.items():
        sbl.write_epgm(d / ("matrix_%s.epgm" % c), x, c, (int(x.min()) + 1, int(x.max()) + 1))
    return d


def test_default_tag_and_run_order_are_those_of_the_matrix_directory(tmp_path, calls, be, monkeypatch):
    """Paired mode: the null shuffle is keyed by the file's ordinal in the run, so the bytes are those of `-i` on a directory of the
    same name only if the matrices run in the natural-key order of their file names -- the sizes file lists them otherwise."""
    d, meta, sizes, mats = calls
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    log = tmp_path / "io.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    _numpy_builder(monkeypatch)
    seen = []
    groupings = driver.run_groupings
    monkeypatch.setattr(driver, "run_groupings", lambda files, *a, **k: seen.append(list(files)) or groupings(files, *a, **k))
    states = _states_file(tmp_path / "states.tsv")
    common = ["-m", "paired", "--columns-a", "1-3", "--columns-b", "4-6", "-j", str(states), "--null-seed", "7", "-w", "3"]
    res = _invoke(common + ["--chromhmm", str(d), "--metadata", str(meta), "--chromsizes", str(sizes), "-o", str(tmp_path / "one")])
    assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    assert not log.exists()                                      # no input file was read as a matrix
    progress = "".join("Processing %s: %s\n" % (c, "0 files found. Skipping." if c == "chrM" else "%d files found. Done." % N)
                       for c in SIZES_ORDER[:2] + ["chrM"] + SIZES_ORDER[2:])
    assert res.output.startswith(progress) and res.output.index("State Model") >= len(progress)
    assert seen == [[Path("matrix_%s.epgm" % c) for c in RUN_ORDER]]
    res = _invoke(common + ["-i", str(_epgm_dir(tmp_path / "two_commands" / "roadmap", mats)), "-o", str(tmp_path / "two")])
    assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    names = same_tree(tmp_path / "one", tmp_path / "two")
    assert "pairwiseMetrics_roadmap_A_roadmap_B_s1.txt.gz" in names
    assert sorted(n for n in names if n.startswith("pairwiseDelta_")) == sorted(
        "pairwiseDelta_roadmap_A_roadmap_B_s1_matrix_%s.txt.gz" % c for c in RUN_ORDER)

    # single mode: the plain run's default tag, and the whole matrix as the one group
    res = _invoke(["--chromhmm", str(d), "--metadata", str(meta), "--chromsizes", str(sizes), "-j", str(states), "-w", "3", "-o", str(tmp_path / "s1")])
    assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    res = _invoke(["-i", str(tmp_path / "two_commands" / "roadmap"), "-j", str(states), "-w", "3", "-o", str(tmp_path / "s2")])
    assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    assert "scores_roadmap_s1_matrix_chr10.txt.gz" in same_tree(tmp_path / "s1", tmp_path / "s2")


def test_a_directory_none_of_whose_files_is_selected_is_the_empty_directory_of_the_matrix_route(tmp_path, calls, monkeypatch):
    d, _meta, sizes, _mats = calls
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    nobody = tmp_path / "nobody.txt"
    nobody.write_text("id\nZ001\n")
    states = _states_file(tmp_path / "states.tsv")
    empty = tmp_path / "empty"
    empty.mkdir()
    res = _invoke(["-i", str(empty), "-j", str(states), "-o", str(tmp_path / "o")])
    assert isinstance(res.exception, OSError) and str(res.exception) == "Ensure that directory is not empty: %s" % empty
    res = _invoke(["--chromhmm", str(d), "--metadata", str(nobody), "--chromsizes", str(sizes), "-j", str(states), "-o", str(tmp_path / "o")])
    assert isinstance(res.exception, OSError) and str(res.exception) == "Ensure that directory is not empty: %s" % d
    assert not (tmp_path / "o").exists()


# ---- driver.run_groupings(resident=...) ------------------------------------------------------------------------------------------

def _resident(mats):
    files = [Path("matrix_%s.epgm" % c) for c in RUN_ORDER]
    return files, {f: (mats[c], N, sbl.synth_locations(c, 0, ROWS[c])) for f, c in zip(files, RUN_ORDER)}


def _no_readers(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a reader was started for a resident matrix")
    monkeypatch.setattr(driver, "_Readers", refuse)
    monkeypatch.setattr(driver, "_columns_of", refuse)


@pytest.mark.parametrize("paired", [False, True])
def test_resident_matrices_are_scored_where_they_are(tmp_path, calls, be, monkeypatch, paired):
    _d, _meta, _sizes, mats = calls
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    if paired:
        groupings = [("halves", helpers.parseColumns("1-3"), helpers.parseColumns("4-6")), ("small", helpers.parseColumns("2"), helpers.parseColumns("6,1"))]
    else:
        groupings = [("all", helpers.parseColumns("1-6")), ("one", helpers.parseColumns("5")), ("mixed", helpers.parseColumns("2-3,6,1"))]
    kw = dict(quiescentState=S - 1, nullSeed=11, keep_temps=False) if paired else dict(keep_temps=False)
    # the oracle first: the same call on files written from the same arrays (its readers run)
    epgm = _epgm_dir(tmp_path / "m", {c: mats[c] for c in RUN_ORDER})
    on_files = sorted(epgm.iterdir(), key=lambda p: RUN_ORDER.index(p.name[len("matrix_"):-len(".epgm")]))
    want = []
    for name, _q, _results, info in driver.run_groupings(on_files, groupings, S, 1, tmp_path / "files", "t", **kw):
        driver.finish_writes()
        want.append(info)
    assert want[0]["uploads"] == want[0]["parsed_files"] == len(RUN_ORDER)

    log = tmp_path / "io.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    monkeypatch.setenv("EPILOGOS_RESIDENT_BYTES", "0")           # does not apply: there is no file to fall back to
    _no_readers(monkeypatch)
    files, resident = _resident(mats)
    before = {f: resident[f][0].copy() for f in files}
    opened = be.opened
    got = []
    for name, q, results, info in driver.run_groupings(files, groupings, S, 1, tmp_path / "resident", "t", resident=resident, **kw):
        driver.finish_writes()
        assert q.shape == (S,) and list(results) == ["matrix_%s" % c for c in RUN_ORDER]
        got.append((name, info))
    assert [g[0] for g in got] == [g[0] for g in groupings]
    for _name, info in got:
        assert info["uploads"] == 0 and info["parsed_files"] == 0
        assert info["kept_files"] == len(RUN_ORDER) and info["refused_files"] == 0 and info["resident_bytes"] == sum(ROWS.values()) * N
    assert not log.exists()
    assert be.opened - opened == len(groupings) == be.closed_sessions - opened
    assert all(np.array_equal(resident[f][0], before[f]) for f in files)       # read, never written
    for g in groupings:
        same_tree(tmp_path / "resident" / g[0], tmp_path / "files" / g[0])


def test_one_grouping_without_a_subdirectory_and_the_whole_matrix_as_its_group(tmp_path, calls, be, monkeypatch):
    _d, _meta, _sizes, mats = calls
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    epgm = _epgm_dir(tmp_path / "m", {c: mats[c] for c in RUN_ORDER})
    on_files = sorted(epgm.iterdir(), key=lambda p: RUN_ORDER.index(p.name[len("matrix_"):-len(".epgm")]))
    driver.run_single_group(on_files, S, 1, _made(tmp_path / "files"), "t", keep_temp_scores=False)
    _no_readers(monkeypatch)
    files, resident = _resident(mats)
    runs = list(driver.run_groupings(files, [("", None)], S, 1, _made(tmp_path / "flat"), "t", keep_temps=False, resident=resident, flat=True))
    assert len(runs) == 1 and runs[0][3]["uploads"] == 0 and runs[0][3]["parsed_files"] == 0
    same_tree(tmp_path / "flat", tmp_path / "files")
    with pytest.raises(ValueError, match="one grouping"):
        next(driver.run_groupings(files, [("a", None), ("b", None)], S, 1, tmp_path / "no", "t", resident=resident, flat=True))
    assert not (tmp_path / "no").exists()


def _made(d):
    d.mkdir()
    return d
