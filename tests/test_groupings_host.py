"""`epilogos --groupings`, the host side (no GPU): the groupings file's grammar and refusals (helpers.parseGroupings), the command
line's usage errors -- printed before an input file is touched or a directory made -- and driver.run_groupings over a stand-in
backend (tests/groupings_backend.py): every file is parsed and "uploaded" once for the whole run, the partition is planned once,
a closed session per grouping, and the directories equal those of the separate --columns commands byte for byte."""
import filecmp
import gzip
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import backend, driver, helpers
from tests.conftest import free_port
from tests.groupings_backend import GroupingsBackend
from tests.test_host_logic import write_tsv

ROOT = Path(__file__).resolve().parents[1]
S = 5
ROWS, N = (23, 1, 9), 11
GROUPINGS = [("all", "1-11"), ("one", "5"), ("mixed", "2-4,11,6-7")]


def _invoke(args):
    from click.testing import CliRunner
    from epilogos_amd import run
    return CliRunner().invoke(run.main, args).output


def same_tree(a, b):
    """Same file set, same bytes; no part or temp file left."""
    names = sorted(p.name for p in Path(a).iterdir())
    assert names == sorted(p.name for p in Path(b).iterdir()) and names
    assert not [n for n in names if n.startswith(".part_") or n.startswith("temp_")]
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert (mismatch, errors) == ([], []) and sorted(match) == names
    return names


# ---- the groupings file ------------------------------------------------------------------------------------------------------

def test_grammar_single(tmp_path):
    spec = tmp_path / "female.txt"
    spec.write_text("# female\n1-3\n7\n")
    f = tmp_path / "g.tsv"
    f.write_text("# name\tbiosamples\n\n   \nall\t1-11\n  # indented comment\none.b_1-x\t 5 \nfile\t@%s\nmixed\t2-4,11,6-7\n" % spec)
    got = helpers.parseGroupings(f, "single")
    assert [g[0] for g in got] == ["all", "one.b_1-x", "file", "mixed"] and all(len(g) == 2 for g in got)
    assert got[0][1].tolist() == list(range(11)) and got[0][1].dtype == np.int64
    assert got[1][1].tolist() == [4] and got[2][1].tolist() == [0, 1, 2, 6] and got[3][1].tolist() == [1, 2, 3, 10, 5, 6]


def test_grammar_paired(tmp_path):
    spec = tmp_path / "b.txt"
    spec.write_text("8-9\n")
    f = tmp_path / "g.tsv"
    f.write_text("\n#c\nsex\t1-5\t6-11\r\nsmall\t3\t5,7\nfile\t1\t@%s\n" % spec)
    got = helpers.parseGroupings(f, "paired")
    assert [g[0] for g in got] == ["sex", "small", "file"] and all(len(g) == 3 for g in got)
    assert got[0][1].tolist() == [0, 1, 2, 3, 4] and got[0][2].tolist() == [5, 6, 7, 8, 9, 10]
    assert got[1][1].tolist() == [2] and got[1][2].tolist() == [4, 6] and got[2][2].tolist() == [7, 8]


@pytest.mark.parametrize("mode,text,words", [
    ("single", "a\t1\nb\t1\t2\n", ("line 2", "3 field(s)", "NAME<TAB>SPEC")),
    ("single", "a\n", ("line 1", "1 field(s)")),
    ("paired", "#x\n\na\t1\n", ("line 3", "2 field(s)", "NAME<TAB>SPEC_A<TAB>SPEC_B")),
    ("paired", "a\t1\t2\t3\n", ("line 1", "4 field(s)")),
    ("single", "a\t1\nb/c\t2\n", ("line 2", "'b/c'", "cannot name")),
    ("single", "..\t1\n", ("line 1", "'..'", "cannot name")),
    ("single", ".\t1\n", ("line 1", "cannot name")),
    ("single", "\t1\n", ("line 1", "cannot name")),
    ("single", "a b\t1\n", ("line 1", "cannot name")),
    ("single", "a\t1\n\nb\t2\na\t3\n", ("line 4", "'a'", "line 1")),
    ("single", "a\t1\nb\t3-1\n", ("line 2", "[SPEC]", "descends")),
    ("single", "a\t\n", ("line 1", "[SPEC]", "empty")),
    ("single", "a\t0\n", ("line 1", "start at 1")),
    ("single", "a\t1,1\n", ("line 1", "biosample 1 is listed twice")),
    ("single", "a\t@/nowhere/at/all.txt\n", ("line 1", "cannot read")),
    ("paired", "a\t1\t2\nb\t1-3\tx\n", ("line 2", "[SPEC_B]", "malformed")),
    ("paired", "a\t1,,2\t5\n", ("line 1", "[SPEC_A]", "malformed")),
    ("paired", "a\t1\t2\n#\nb\t1-4\t6,4\n", ("line 3", "biosample 4 is in both groups")),
    ("single", "# nothing\n\n", ("no groupings",)),
    ("paired", "", ("no groupings",)),
])
def test_refusals_name_the_line(tmp_path, mode, text, words):
    f = tmp_path / "g.tsv"
    f.write_text(text)
    with pytest.raises(ValueError) as e:
        helpers.parseGroupings(f, mode)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_unreadable_file(tmp_path):
    with pytest.raises(ValueError, match="cannot read the groupings file"):
        helpers.parseGroupings(tmp_path / "missing.tsv", "single")


# ---- the command line's refusals ---------------------------------------------------------------------------------------------

def test_usage_errors_before_any_file_is_touched(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                        # relative -i / -o: nothing may appear here
    log = tmp_path.parent / (tmp_path.name + "_io.log")
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    good1, good2 = tmp_path / "g1.tsv", tmp_path / "g2.tsv"
    good1.write_text("a\t1-3\n")
    good2.write_text("a\t1-3\t4-5\n")
    tail = ["-o", "o", "-j", "j"]
    for args, opt in ((["--columns", "1"], "--columns"), (["--columns-a", "1"], "--columns-a"), (["--columns-b", "1"], "--columns-b"),
                      (["-m", "paired", "--columns-a", "1", "--columns-b", "2"], "--columns-a"), (["-a", "y"], "-a"),
                      (["-m", "paired", "-b", "z"], "-b")):
        out = _invoke(["-i", "x", "--groupings", str(good2 if "paired" in args else good1)] + args + tail)
        assert out == "ERROR: [--groupings] names the biosamples of every grouping itself; it cannot be combined with [%s]\n" % opt
    assert _invoke(["--groupings", str(good1)] + tail) == "ERROR: [-i, --input-directory] is required with [--groupings]\n"
    assert _invoke(["-m", "paired", "--groupings", str(good2)] + tail) == "ERROR: [-i, --input-directory] is required with [--groupings]\n"

    def refused(text, mode="single"):
        f = tmp_path / "bad.tsv"
        f.write_text(text)
        out = _invoke(["-i", "x", "-m", mode, "--groupings", str(f)] + tail)
        assert out.startswith("ERROR: [--groupings] ") and out.count("\n") == 1, out
        return out
    assert "line 1: 3 field(s)" in refused("a\t1\t2\n")                         # a paired line in single mode
    assert "line 2: 2 field(s)" in refused("a\t1\t2\nb\t1\n", "paired")
    assert "line 1: 'a/b' cannot name" in refused("a/b\t1\n")
    assert "line 3: the name 'a' is used by line 1 already" in refused("a\t1\n\na\t2\n")
    assert "line 2: [SPEC] malformed biosample list" in refused("a\t1\nb\t1,x\n")
    assert "line 1: [SPEC_B] biosample 5 is listed twice" in refused("a\t1\t5,5\n", "paired")
    assert "line 1: biosample 3 is in both groups" in refused("a\t1-3\t3-6\n", "paired")
    assert "no groupings in" in refused("# none\n")
    assert _invoke(["-i", "x", "--groupings", str(tmp_path / "missing.tsv")] + tail).startswith("ERROR: [--groupings] cannot read the groupings file")
    # a good file: on to today's checks and messages
    assert _invoke(["-i", "x", "--groupings", str(good1), "-j", "j"]) == "ERROR: [-o, --output-directory] is required\n"
    assert _invoke(["-i", "x", "--groupings", str(good1), "--null-draws", "0"] + tail) == "ERROR: [--null-draws] must be at least 1\n"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.tsv", "g1.tsv", "g2.tsv"] and not log.exists()


def test_biosample_beyond_the_files_columns(tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(0)
    write_tsv(ind / "matrix_chr1.txt.gz", rng.integers(0, 3, size=(5, 8)))
    write_tsv(ind / "matrix_chr2.txt.gz", rng.integers(0, 3, size=(5, 6)))
    meta = tmp_path / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\ts%d\n" % (i, i + 1, i) for i in range(3)))
    g = tmp_path / "g.tsv"
    g.write_text("a\t1-3\nb\t2,7\nc\t4\n")
    out = _invoke(["-i", str(ind), "-o", str(tmp_path / "o"), "-j", str(meta), "--groupings", str(g)])
    assert out.startswith("ERROR: biosample 7 is not in ") and "matrix_chr2.txt.gz" in out and "6 biosample columns" in out
    g.write_text("a\t1-3\t4-5\nb\t1\t9,2\n")
    out = _invoke(["-m", "paired", "-i", str(ind), "-o", str(tmp_path / "o"), "-j", str(meta), "--groupings", str(g)])
    assert out.startswith("ERROR: biosample 9 is not in ") and "matrix_chr1.txt.gz" in out and "8 biosample columns" in out
    assert not (tmp_path / "o").exists()               # refused before the first directory is made


def test_help_lists_the_option():
    from click.testing import CliRunner
    from epilogos_amd import run
    out = " ".join(CliRunner().invoke(run.main, ["--help"], terminal_width=200).output.split())
    assert "--groupings" in out and "NAME<TAB>SPEC" in out
    assert out.count("accepted and unused with --null-draws") == 2          # (-t and -z: the new option's help adds none)


def test_command_lines_without_the_option_do_not_hear_of_it():
    tail = ["-o", "o", "-j", "j"]
    for args in (["-o", "o", "-j", "j"], ["-i", "x", "-j", "j"], ["-i", "x", "-o", "o"], ["-i", "x", "-a", "y"] + tail,
                 ["-m", "paired", "-a", "y"] + tail, ["-m", "paired", "-i", "x", "-a", "y", "-b", "z"] + tail,
                 ["-i", "x", "--columns", "1,x"] + tail, ["-i", "x", "--columns-a", "1"] + tail,
                 ["-m", "paired", "-i", "x", "--columns-a", "1"] + tail, ["-m", "paired", "-i", "x", "--columns-a", "1-3", "--columns-b", "3"] + tail,
                 ["-m", "paired", "--columns-a", "1", "--columns-b", "2"] + tail, ["-i", "x", "--null-draws", "3"] + tail,
                 ["-m", "paired", "-a", "y", "-b", "z", "--null-draws", "3"] + tail, ["-i", "x", "--null-draws", "0"] + tail):
        out = _invoke(args)
        assert out.startswith("ERROR: ") and out.count("\n") == 1 and "grouping" not in out.lower(), out


# ---- the run over a stand-in backend -----------------------------------------------------------------------------------------

@pytest.fixture()
def be():
    b = GroupingsBackend()
    backend.set_for_testing(b)
    yield b
    backend.set_for_testing(None)
    driver.finish_writes()


@pytest.fixture()
def inputs(tmp_path):
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(7)
    for k, r in enumerate(ROWS):
        write_tsv(ind / ("matrix_chr%d.txt" % (k + 1)), rng.integers(0, S, size=(r, N)), chrom="chr%d" % (k + 1))
    meta = tmp_path / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    return ind, meta, sorted(ind.glob("*"))


def _reads(log):
    """Input paths of an EPILOGOS_IO_LOG in the order of the passes, one entry per pass."""
    return [l.split("\t")[2] for l in Path(log).read_text().splitlines()] if Path(log).exists() else []


def _walk(files, out, log, groupings=GROUPINGS, **kw):
    """run_groupings to the end -> [(name, info, passes over input files during the grouping)]."""
    seen, got = 0, []
    for name, q, results, info in driver.run_groupings(files, [(n, helpers.parseColumns(s)) for n, s in groupings], S, 1, out, "t", **kw):
        driver.finish_writes()
        assert q.shape == (S,) and sorted(results) == ["matrix_chr1", "matrix_chr2", "matrix_chr3"]
        assert sorted(p.name for p in (out / name).iterdir()) == ["exp_freq_t.npy"] + ["scores_t_matrix_chr%d.txt.gz" % k for k in (1, 2, 3)]
        reads = _reads(log)
        got.append((name, info, sorted(reads[seen:])))
        seen = len(reads)
    return got


def test_files_are_parsed_and_uploaded_once_for_the_run(tmp_path, inputs, be, monkeypatch):
    _ind, _meta, files = inputs
    log = tmp_path / "io.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    plans = []
    plan = driver._plan
    monkeypatch.setattr(driver, "_plan", lambda *a, **k: plans.append(1) or plan(*a, **k))
    got = _walk(files, tmp_path / "out", log, keep_temps=False)
    assert [g[0] for g in got] == ["all", "one", "mixed"]
    assert [(g[1]["parsed_files"], g[1]["uploads"]) for g in got] == [(3, 3), (0, 0), (0, 0)]
    assert [len(g[2]) for g in got] == [3, 0, 0] and sorted(_reads(log)) == sorted(str(f) for f in files)      # each file once in total
    assert len({g[1]["resident_bytes"] for g in got}) == 1 and got[0][1]["resident_bytes"] == sum(ROWS) * N
    assert len(plans) == 1                             # the partition is planned once per run
    assert (be.opened, be.closed_sessions) == (3, 3)   # a session per grouping, closed before the next one opens

    # the same three groupings with nothing kept: three passes and three uploads per grouping, the same bytes
    monkeypatch.setenv("EPILOGOS_RESIDENT_BYTES", "0")
    log2 = tmp_path / "io2.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log2))
    again = _walk(files, tmp_path / "out0", log2, keep_temps=False)
    assert [(g[1]["parsed_files"], g[1]["uploads"], g[1]["resident_bytes"]) for g in again] == [(3, 3, 0)] * 3
    assert [g[2] for g in again] == [sorted(str(f) for f in files)] * 3
    for name, _spec in GROUPINGS:
        same_tree(tmp_path / "out" / name, tmp_path / "out0" / name)


def test_a_cap_keeps_a_prefix_of_the_jobs(tmp_path, inputs, be, monkeypatch, capsys):
    _ind, _meta, files = inputs
    log = tmp_path / "io.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    monkeypatch.setenv("EPILOGOS_RESIDENT_BYTES", str(ROWS[0] * N))          # the first file's matrix, whatever file is parsed first
    got = _walk(files, tmp_path / "out", log, keep_temps=False)
    assert [(g[1]["parsed_files"], g[1]["uploads"]) for g in got] == [(3, 3), (2, 2), (2, 2)]
    assert got[1][2] == got[2][2] == sorted(str(f) for f in files[1:])
    assert all(g[1]["resident_bytes"] == ROWS[0] * N for g in got)
    said = capsys.readouterr().out
    assert said.count("1 of 3 input matrices stay on the device") == 1 and "2 do not" in said


def test_a_side_car_of_the_first_pass_does_not_change_the_plan(tmp_path, inputs, be, monkeypatch):
    _ind, _meta, files = inputs
    monkeypatch.setenv("EPILOGOS_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    log = tmp_path / "io.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    plans = []
    plan = driver._plan
    monkeypatch.setattr(driver, "_plan", lambda *a, **k: plans.append(plan(*a, **k)) or plans[-1])
    stores = []
    parts = driver._ResidentStore.parts
    monkeypatch.setattr(driver._ResidentStore, "parts", lambda self, jobs, *a, **k: stores.append((self, list(jobs))) or parts(self, jobs, *a, **k))
    try:
        got = _walk(files, tmp_path / "out", log, groupings=GROUPINGS[:2], keep_temps=False)
    finally:
        helpers.flushCacheWrites()
    assert len(list((tmp_path / "cache").glob("*.states.npy"))) == 3         # the side-cars exist by the second grouping
    assert len(plans) == 1 and stores[0][0] is stores[1][0] and stores[0][0].plan is plans[0]
    assert stores[0][1] == stores[1][1] == [(f, 0, None) for f in files]     # the second grouping's jobs are the first one's
    assert [(g[1]["parsed_files"], g[1]["uploads"]) for g in got] == [(3, 3), (0, 0)]


def test_command_writes_what_the_separate_commands_write(tmp_path, inputs, be, monkeypatch):
    from click.testing import CliRunner
    from epilogos_amd.run import main
    ind, meta, _files = inputs
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    g = tmp_path / "g.tsv"
    g.write_text("# three groups\n" + "".join("%s\t%s\n" % ns for ns in GROUPINGS))
    common = ["-i", str(ind), "-j", str(meta), "-s", "1", "-w", "3"]
    res = CliRunner().invoke(main, common + ["-o", str(tmp_path / "out"), "--groupings", str(g)])
    assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    at = [res.output.index("Grouping %d of 3: %s" % (k + 1, n)) for k, (n, _s) in enumerate(GROUPINGS)]
    assert at == sorted(at)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(n for n, _s in GROUPINGS)
    for name, spec in GROUPINGS:
        res = CliRunner().invoke(main, common + ["-o", str(tmp_path / "sep" / name), "--columns", spec])
        assert res.exit_code == 0 and "ERROR" not in res.output, res.output
        names = same_tree(tmp_path / "out" / name, tmp_path / "sep" / name)
        assert "regionsOfInterest_in_s1.txt" in names and "exp_freq_in_s1.npy" not in names


def test_paired_command_writes_what_the_separate_commands_write(tmp_path, inputs, be, monkeypatch):
    from click.testing import CliRunner
    from epilogos_amd.run import main
    ind, meta, _files = inputs
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    lines = [("halves", "1-5", "6-11"), ("small", "3", "5,7")]
    g = tmp_path / "g.tsv"
    g.write_text("".join("%s\t%s\t%s\n" % l for l in lines))
    common = ["-m", "paired", "-i", str(ind), "-j", str(meta), "-s", "1", "-w", "3", "--null-seed", "7", "-f", "t"]
    res = CliRunner().invoke(main, common + ["-o", str(tmp_path / "out"), "--groupings", str(g)])
    assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    for name, a, b in lines:
        res = CliRunner().invoke(main, common + ["-o", str(tmp_path / "sep" / name), "--columns-a", a, "--columns-b", b])
        assert res.exit_code == 0 and "ERROR" not in res.output, res.output
        names = same_tree(tmp_path / "out" / name, tmp_path / "sep" / name)
        assert "pairwiseMetrics_t.txt.gz" in names


def test_a_later_grouping_that_raises_leaves_the_earlier_ones_complete(tmp_path, inputs, be, monkeypatch):
    _ind, _meta, files = inputs
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    runs = driver.run_groupings(files, [("ok", np.arange(4)), ("beyond", np.array([2, 11])), ("never", np.arange(2))], S, 1, tmp_path / "out", "t",
                                keep_temps=False)
    name, _q, results, _info = next(runs)
    assert name == "ok" and len(results) == 3
    with pytest.raises(ValueError, match="biosample 12 is not in"):
        next(runs)
    assert len(list((tmp_path / "out" / "ok").glob("scores_t_*.txt.gz"))) == 3 and not (tmp_path / "out" / "never").exists()
    assert be.opened == be.closed_sessions == 2


def test_two_ranks_keep_what_they_parsed(tmp_path, inputs):
    """Two ranks over gloo, text inputs, --cache-dir set: each file is parsed once, by one rank, which keeps it; the plan of the
    first grouping ("assigned": the side-cars do not exist yet) is the plan of the later ones although every side-car exists by
    then; the border pieces change hands per grouping and the outputs are the one-rank run's."""
    ind, _meta, files = inputs
    specs = [s for _n, s in GROUPINGS]
    outs = {}
    for world in (1, 2):
        out = outs[world] = tmp_path / ("out%d" % world)
        log = tmp_path / ("io%d.log" % world)
        port = str(free_port())
        env = dict(os.environ, PYTHONPATH=str(ROOT), MASTER_ADDR="127.0.0.1", MASTER_PORT=port, EPILOGOS_IO_LOG=str(log),
                   EPILOGOS_CACHE_DIR=str(tmp_path / ("cache%d" % world)))
        env.pop("EPILOGOS_RESIDENT_BYTES", None)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", port, str(ROOT / "tests" / "groupings_gloo_worker.py"), str(ind), str(out), str(S)] + specs
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        infos = [json.loads(l) for r in range(world) for l in (tmp_path / ("info_%d_rank%d.jsonl" % (world, r))).read_text().splitlines()]
        assert len(infos) == 3 * world and all(i["plans"] == 1 for i in infos)
        assert {i["layout"] for i in infos} == {"whole" if world == 1 else "assigned"}
        assert sorted(_reads(log)) == sorted(str(f) for f in files)                    # each file once in total, whatever the ranks
        first = [i for i in infos if i["name"] == "g0"]
        assert sum(i["parsed_files"] for i in first) == sum(i["uploads"] for i in first) == sum(i["kept_files"] for i in first) == 3
        assert all((i["parsed_files"], i["uploads"]) == (0, 0) for i in infos if i["name"] != "g0")
        assert len(list((tmp_path / ("cache%d" % world)).glob("*.states.npy"))) == 3
    for k in range(3):
        a, b = outs[1] / ("g%d" % k), outs[2] / ("g%d" % k)
        names = sorted(p.name for p in a.iterdir())
        assert names == sorted(p.name for p in b.iterdir()) == ["exp_freq_t.npy"] + ["scores_t_matrix_chr%d.txt.gz" % c for c in (1, 2, 3)]
        assert (a / names[0]).read_bytes() == (b / names[0]).read_bytes()
        for n in names[1:]:                            # (a file cut by the range border is two gzip members: compared decompressed)
            with gzip.open(a / n, "rb") as fa, gzip.open(b / n, "rb") as fb:
                assert fa.read() == fb.read(), n
