"""`similaritySearch_run --gpus N` without a GPU: the option taken out of the arguments by cli(), its refusals, the STEP 2
children's command lines and environments, the shard rule and its reassembly, stale per-job files, the failure path and the
device check.  STEP 2 itself is replaced by a host stand-in (fake_search) so that the build runs end to end on the host."""
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import run as epilogos_run
from epilogos_amd import similaritySearch_calc as calc
from epilogos_amd import similaritySearch_run as run
from epilogos_amd import similaritySearch_write as wr
from epilogos_amd.helpers import splitGpusOption, splitRows

ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests" / "golden" / "simsearch.npz")
OUTPUTS = ["reduced_genome.npy", "simsearch.bed.gz", "simsearch.bed.gz.tbi", "simsearch_cube.npz", "simsearch_indices.npy"]


def _scores(tmp_path, case="s200"):
    p = tmp_path / ("scores_%s.txt" % case)
    p.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    return p


@pytest.fixture
def captured(monkeypatch):
    """buildSimSearch replaced by a recorder of its arguments."""
    calls = []
    monkeypatch.setattr(run, "buildSimSearch", lambda *a, **k: calls.append((a, k)))
    return calls


@pytest.mark.parametrize("where", ["first", "middle", "last", "equals"])
def test_gpus_is_taken_anywhere(tmp_path, captured, where):
    base = ["-b", "-s", "scores.txt", "-o", str(tmp_path / "o"), "-c", "4"]
    argv = {"first": ["--gpus", "2"] + base, "middle": base[:3] + ["--gpus", "2"] + base[3:],
            "last": base + ["--gpus", "2"], "equals": base[:5] + ["--gpus=2"] + base[5:]}[where]
    with pytest.raises(SystemExit) as e:
        run.cli(argv)
    assert e.value.code == 0
    (a, k), = captured
    assert a[0] == "scores.txt" and a[4] == 4 and k["gpus"] == 2


def test_without_gpus_the_build_is_the_single_process_one(tmp_path, captured):
    with pytest.raises(SystemExit):
        run.cli(["-b", "-s", "x.txt", "-o", str(tmp_path), "-j", "3"])
    with pytest.raises(SystemExit):
        run.cli(["-b", "-s", "x.txt", "-o", str(tmp_path), "--gpus", "1"])
    assert [k["gpus"] for _a, k in captured] == [1, 1]


def test_main_options_stay_the_reference_ones():
    names = sorted(o for p in run.main.params for o in p.opts)
    assert names == list(GOLD["click_options"]) and "--gpus" not in names


def test_split_helper_is_the_epilogos_one():
    argv = ["--gpus", "4", "-i", "in", "--gpus=3", "-o", "out", "--gpus"]
    assert splitGpusOption(argv) == ("", ["-i", "in", "-o", "out"])
    assert splitGpusOption(["-i", "in", "--gpus=3"]) == ("3", ["-i", "in"])
    assert splitGpusOption(["-i", "in"]) == (None, ["-i", "in"])
    assert epilogos_run._strip_gpus(argv) == ["-i", "in", "-o", "out"]


@pytest.mark.parametrize("value, words", [("-1", "positive or zero"), ("x", "whole number"), ("1.5", "whole number"),
                                          (None, "whole number")])
def test_bad_gpus_values_are_refused(tmp_path, captured, capsys, value, words):
    argv = ["-b", "-s", "x.txt", "-o", str(tmp_path)] + (["--gpus", value] if value is not None else ["--gpus"])
    with pytest.raises(SystemExit) as e:
        run.cli(argv)
    assert e.value.code == 2 and words in capsys.readouterr().err and not captured


def test_gpus_with_query_is_refused(tmp_path, captured, capsys):
    with pytest.raises(SystemExit) as e:
        run.cli(["--gpus", "2", "-q", "chr1:1-2", "-m", "x.bed.gz", "-o", str(tmp_path)])
    assert e.value.code == 2 and "query mode" in capsys.readouterr().err and not captured


def test_gpus_zero_is_every_visible_gpu(tmp_path, captured, monkeypatch):
    monkeypatch.setattr(epilogos_run, "_visible_gpus", lambda: 5)
    with pytest.raises(SystemExit):
        run.cli(["-b", "-s", "x.txt", "-o", str(tmp_path), "--gpus", "0"])
    assert captured[0][1]["gpus"] == 5


def test_child_commands_and_environments(tmp_path, monkeypatch):
    from epilogos_amd import _io
    monkeypatch.setattr(_io, "node_cores", lambda: 16)
    monkeypatch.setenv("PYTHONPATH", "/elsewhere")
    jobs = run.childJobs(tmp_path, 125, 5, 8, 100, 3)
    assert len(jobs) == 3
    for i, (argv, env) in enumerate(jobs):
        assert argv[:3] == [sys.executable, "-m", "epilogos_amd.similaritySearch_calc"]
        assert argv[3:] == [str(tmp_path.resolve()), "125", "5", "2", "100", "3", str(i)]
        assert env["LOCAL_RANK"] == str(i) and env["OMP_NUM_THREADS"] == "2"
        assert env["PYTHONPATH"].split(":") == [str(ROOT), "/elsewhere"]
    assert [(a[6], e["OMP_NUM_THREADS"]) for a, e in run.childJobs(tmp_path, 125, 5, 0, 100, 3)] == [("5", "5")] * 3
    assert {e["OMP_NUM_THREADS"] for _a, e in run.childJobs(tmp_path, 125, 5, 1, 100, 4)} == {"1"}
    # -c beyond the node's cores is capped by them, as the `epilogos` command's host budget is
    assert {e["OMP_NUM_THREADS"] for _a, e in run.childJobs(tmp_path, 125, 5, 64, 100, 2)} == {"8"}


@pytest.mark.parametrize("R", [0, 1, 2, 7, 1000])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_shards_cover_every_roi_once_and_reassemble(tmp_path, R, N):
    shards = splitRows(R, N)
    assert len(shards) == N and shards[0][0] == 0 and shards[-1][1] == R
    assert np.array_equal(np.concatenate([np.arange(lo, hi) for lo, hi in shards]), np.arange(R))
    n = 5
    want = np.random.default_rng(R * 10 + N).integers(-1, 10 ** 6, size=(R, n)).astype(np.int32)
    for i, (lo, hi) in enumerate(shards):
        part = want[lo:hi] if hi > lo else np.zeros((0, n), dtype=np.int32)       # what an empty shard writes
        np.save(tmp_path / ("simsearch_indices_%d.npy" % i), part)
    got = wr.readSimsearchIndices(tmp_path, R, n, N)
    assert got.dtype == np.int32 and np.array_equal(got, want)


def fake_search(G, Q, selfStart, nDesiredMatches, **_kw):
    """Host stand-in of similaritySearch_calc.simsearch: indices that depend on each ROI (its own start and its scores)."""
    G, Q = np.asarray(G), np.asarray(Q)
    P = G.shape[0] - Q.shape[1] + 1
    key = np.asarray(selfStart, dtype=np.int64) * 31 + Q.sum(axis=(1, 2)) % 97
    idx = ((key[:, None] + 7 * np.arange(nDesiredMatches)) % P).astype(np.int32)
    idx[:, -3:] = -1
    return idx, np.zeros(len(Q), dtype=np.int64)


def run_jobs_in_process(jobs):
    """runChildren's stand-in: every child's argv interface called in this process (STEP 2 through fake_search)."""
    for argv, env in jobs:
        assert argv[1:3] == ["-m", "epilogos_amd.similaritySearch_calc"] and env["LOCAL_RANK"] == argv[-1]
        calc.main(Path(argv[3]), *[int(a) for a in argv[4:]])


@pytest.fixture
def host_step2(monkeypatch):
    monkeypatch.setattr(calc, "simsearch", fake_search)
    monkeypatch.setattr(run, "runChildren", run_jobs_in_process)
    monkeypatch.setenv("EPILOGOS_DIST_BACKEND", "gloo")


@pytest.mark.parametrize("case", ["s200", "s20"])
def test_sharded_build_is_byte_identical(tmp_path, host_step2, case):
    sp = _scores(tmp_path, case)
    w = int(GOLD[case + "_windowBP"])
    outs = {}
    for N in (1, 2, 3, 8, 20):
        out = tmp_path / ("g%d" % N)
        out.mkdir()
        run.buildSimSearch(sp, out, w, 10, 1, 100, -1, -1, gpus=N)
        assert sorted(p.name for p in out.iterdir()) == OUTPUTS
        outs[N] = {f: (out / f).read_bytes() for f in OUTPUTS}
    assert len(np.load(tmp_path / "g1" / "simsearch_indices.npy")) < 20           # more children than ROIs included
    for N in (2, 3, 8, 20):
        assert outs[N] == outs[1], N


def test_stale_index_files_are_removed_before_step2(tmp_path, host_step2, monkeypatch):
    sp = _scores(tmp_path)
    out = tmp_path / "o"
    out.mkdir()
    run.buildSimSearch(sp, out, 25000, 10, 1, 100, -1, -1, gpus=1)
    want = (out / "simsearch_indices.npy").read_bytes()
    for i in range(8):                                # a previous build's leftovers, with more jobs than this one
        np.save(out / ("simsearch_indices_%d.npy" % i), np.full((2, 100), 9, dtype=np.int32))
    seen = []

    def children(jobs):
        seen.append(sorted(p.name for p in out.glob("simsearch_indices_*.npy")))
        run_jobs_in_process(jobs)
    monkeypatch.setattr(run, "runChildren", children)
    run.buildSimSearch(sp, out, 25000, 10, 1, 100, -1, -1, gpus=3)
    assert seen == [[]]
    assert (out / "simsearch_indices.npy").read_bytes() == want and not list(out.glob("simsearch_indices_*.npy"))


def test_a_failed_child_ends_the_build(tmp_path, monkeypatch):
    """Child 1 exits with status 3 while child 0 sleeps: the build stops, names child 1 and its status, stops the sleeper and
    writes no bed file.  No GPU: the children are plain Python processes."""
    monkeypatch.setenv("EPILOGOS_DIST_BACKEND", "gloo")
    sleeper = [sys.executable, "-c", "import time; time.sleep(600)"]
    failer = [sys.executable, "-c", "import sys; sys.stderr.write('first\\nsomething broke\\n'); sys.exit(3)"]
    monkeypatch.setattr(run, "childJobs", lambda *a: [(sleeper, None), (failer, None)])
    started = []

    class Recorded(subprocess.Popen):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            started.append(self)
    monkeypatch.setattr(run.subprocess, "Popen", Recorded)
    out = tmp_path / "o"
    out.mkdir()
    with pytest.raises(SystemExit) as e:
        run.buildSimSearch(_scores(tmp_path), out, 25000, 10, 1, 100, -1, -1, gpus=2)
    msg = str(e.value.code)
    assert "child 1 of 2 exited with status 3" in msg and "something broke" in msg
    assert len(started) == 2 and all(p.poll() is not None for p in started)      # nobody is left running
    assert started[0].returncode < 0                                             # the sleeper was stopped
    assert not (out / "simsearch.bed.gz").exists() and not (out / "simsearch.bed.gz.tbi").exists()


def test_a_failed_build_leaves_no_per_job_files_for_the_next(tmp_path, host_step2, monkeypatch):
    """Child 1 of 3 fails after children 0 and 2 wrote their files: they are removed, so that a one-process build into the
    same directory afterwards merges only its own."""
    sp = _scores(tmp_path)
    out = tmp_path / "o"
    out.mkdir()

    def children(jobs):
        run_jobs_in_process([jobs[0], jobs[2]])
        assert len(list(out.glob("simsearch_indices_*.npy"))) == 2
        raise SystemExit("ERROR: similarity search STEP 2 child 1 of 3 exited with status 3")
    monkeypatch.setattr(run, "runChildren", children)
    with pytest.raises(SystemExit, match="child 1 of 3"):
        run.buildSimSearch(sp, out, 25000, 10, 1, 100, -1, -1, gpus=3)
    assert not list(out.glob("simsearch_indices_*.npy")) and not (out / "simsearch.bed.gz").exists()
    run.buildSimSearch(sp, out, 25000, 10, 1, 100, -1, -1, gpus=1)
    assert sorted(p.name for p in out.iterdir()) == OUTPUTS
    ref = tmp_path / "ref"
    ref.mkdir()
    run.buildSimSearch(sp, ref, 25000, 10, 1, 100, -1, -1, gpus=1)
    assert all((out / f).read_bytes() == (ref / f).read_bytes() for f in OUTPUTS)


def test_sigterm_to_the_build_stops_its_children(tmp_path):
    pidfile = tmp_path / "child.pid"
    sleeper = "import os, time; open(%r, 'w').write(str(os.getpid())); time.sleep(600)" % str(pidfile)
    script = ("import sys; sys.path.insert(0, %r); from epilogos_amd import similaritySearch_run as r; "
              "r.runChildren([([sys.executable, '-c', %r], None)])" % (str(ROOT), sleeper))
    parent = subprocess.Popen([sys.executable, "-c", script], stderr=subprocess.PIPE, text=True)
    try:
        for _ in range(600):
            if pidfile.exists() and pidfile.read_text():
                break
            assert parent.poll() is None
            time.sleep(0.05)
        child = int(pidfile.read_text())
        parent.terminate()
        _out, err = parent.communicate(timeout=60)
    finally:
        if parent.poll() is None:
            parent.kill()
            parent.wait()
    assert parent.returncode == 1 and "stopped by SIGTERM" in err
    with pytest.raises(ProcessLookupError):            # stopped and reaped by the build
        os.kill(child, 0)


def test_a_child_killed_by_a_signal_is_named(tmp_path):
    jobs = [([sys.executable, "-c", "import os, signal; os.kill(os.getpid(), signal.SIGKILL)"], None)]
    with pytest.raises(SystemExit, match="child 0 of 1 was killed by signal SIGKILL"):
        run.runChildren(jobs)


def test_more_children_than_gpus_needs_the_shared_gpu_switch(tmp_path, monkeypatch):
    monkeypatch.setattr(epilogos_run, "_visible_gpus", lambda: 2)
    monkeypatch.delenv("EPILOGOS_DIST_BACKEND", raising=False)
    run.checkDevices(2)
    with pytest.raises(SystemExit, match=r"rank 2 of this node has no GPU: 3 rank\(s\) were started for 2 usable device"):
        run.checkDevices(3)
    out = tmp_path / "o"
    out.mkdir()
    with pytest.raises(SystemExit, match="no GPU"):                          # refused before STEP 1
        run.buildSimSearch(_scores(tmp_path), out, 25000, 10, 1, 100, -1, -1, gpus=3)
    assert not list(out.iterdir())
    monkeypatch.setenv("EPILOGOS_DIST_BACKEND", "gloo")
    run.checkDevices(3)
