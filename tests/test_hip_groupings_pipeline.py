"""GPU: `epilogos --groupings FILE` writes into OUT/NAME/, for every line of FILE, the files and bytes that the separate command
with --columns (or --columns-a / --columns-b) and -o OUT/NAME writes -- what STEP 4 deletes included -- while every input file
is parsed and uploaded once for the whole run (driver.run_groupings' info), device memory does not grow from grouping to
grouping, and a matrix the admission rule refuses is read again with the same bytes coming out.

Inputs: three chromosome files of 700 (more than one 512-row tile), 1 and 130 rows, 37 biosample columns (no multiple of 16: the
row pitch is padded to 48), written like those of tests/test_hip_groups_pipeline.py; an 18-state model as .txt.gz and as .epgm,
a 40-state model (the wide path: device gather) as .txt.gz.  Every command is a child process with a time limit of its own; once
a child has failed or run out of time no further child is started.

How directories are compared (same_tree): the same file names, and the same bytes by filecmp -- with ONE exception that is no
property of the run: Python's gzip module, which writes significantLoci_*.txt.gz, stores the second the file was opened in
header bytes 4..7, so two runs of today's command differ there too; those four bytes are masked in every .gz file (the native
writer of the other .gz files leaves them zero).  Across rank counts the .gz text is compared decompressed: a file cut by a
range border is a concatenation of gzip members, one per owner, by design (driver._assemble_text)."""
import filecmp
import gzip
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import driver, helpers, stateByLine as sbl
from tests.test_hip_groups_pipeline import ROOT, _broken, run_cli
from tests.test_host_logic import write_tsv

pytestmark = pytest.mark.gpu

ROWS, N, PITCH = (700, 1, 130), 37, 48
SINGLE = [("all", "1-37"), ("one", "5"), ("mixed", "2-9,30,12-20")]
PAIRED = [("halves", "1-18", "19-37"), ("small", "3", "5,7")]
CHILD_LIMIT = 240                                      # seconds: a run takes a few, the start of a process included


def _matrices(S):
    rng = np.random.default_rng(S)
    out = []
    for r in ROWS:
        x = np.where(rng.random((r, N)) < 0.5, S - 1, rng.integers(0, S, size=(r, N)))
        quiet = rng.random(r) < 0.2                    # quiescent in the groups that leave out biosamples 18 and 19
        x[quiet] = S - 1
        x[quiet, 17:19] = 0
        out.append(x)
    return out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{"txt18" | "epgm18" | "txt40": directory}, {18 | 40: metadata file}."""
    base = tmp_path_factory.mktemp("groupings")
    dirs, metas = {}, {}
    for S in (18, 40):
        metas[S] = base / ("metadata%d.tsv" % S)
        metas[S].write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
        d = dirs["txt%d" % S] = base / ("txt%d" % S) / "whole"
        d.mkdir(parents=True)
        for k, x in enumerate(_matrices(S)):
            write_tsv(d / ("matrix_chr%d.txt.gz" % (k + 1)), x, chrom="chr%d" % (k + 1))
    d = dirs["epgm18"] = base / "epgm18" / "whole"
    d.mkdir(parents=True)
    for k, x in enumerate(_matrices(18)):
        sbl.write_epgm(d / ("matrix_chr%d.epgm" % (k + 1)), x.astype(np.int8), "chr%d" % (k + 1), (1, 18))
    return dirs, metas


def _groupings_file(path, lines):
    path.write_text("# name, then the biosamples\n\n" + "".join("\t".join(l) + "\n" for l in lines))
    return path


def _masked(path):
    b = bytearray(Path(path).read_bytes())
    b[4:8] = b"\0\0\0\0"                                # gzip MTIME (see the module's text)
    return bytes(b)


def same_tree(a, b, decompress=False):
    names = sorted(p.name for p in Path(a).iterdir())
    assert names == sorted(p.name for p in Path(b).iterdir()) and names
    assert not [n for n in names if n.startswith(".part_") or n.startswith("temp_")], names
    plain = [n for n in names if not n.endswith(".gz")]
    match, mismatch, errors = filecmp.cmpfiles(a, b, plain, shallow=False)
    assert (mismatch, errors) == ([], []) and sorted(match) == plain
    for n in names:
        if n.endswith(".gz") and decompress:
            with gzip.open(Path(a) / n, "rb") as fa, gzip.open(Path(b) / n, "rb") as fb:
                assert fa.read() == fb.read(), n
        elif n.endswith(".gz"):
            assert _masked(Path(a) / n) == _masked(Path(b) / n), n
    return names


def _compare_single(tmp_path, ind, meta, sal, lines):
    common = ["-i", str(ind), "-j", str(meta), "-s", str(sal)]
    out = run_cli(common + ["--groupings", str(_groupings_file(tmp_path / "g.tsv", lines))], tmp_path / "out")
    assert sorted(p.name for p in out.iterdir()) == sorted(l[0] for l in lines)
    for name, spec in lines:
        sep = run_cli(common + ["--columns", spec], tmp_path / "sep" / name)
        names = same_tree(out / name, sep)
        assert sum(n.startswith("scores_t_") for n in names) == 3 and "regionsOfInterest_t.txt" in names and "exp_freq_t.npy" not in names


def test_single_s1_three_groupings_equal_three_commands(tmp_path, inputs):
    dirs, metas = inputs
    _compare_single(tmp_path, dirs["txt18"], metas[18], 1, SINGLE)
    with gzip.open(tmp_path / "out" / "one" / "scores_t_matrix_chr1.txt.gz", "rt") as fh:
        rows = fh.read().splitlines()
    assert len(rows) == 700 and len(rows[0].split("\t")) == 3 + 18


@pytest.mark.parametrize("which,S,sal,line", [("epgm18", 18, 2, SINGLE[2]), ("txt18", 18, 3, SINGLE[2]), ("txt40", 40, 1, SINGLE[0])],
                         ids=["s2-epgm", "s3", "wide-40-states"])
def test_single_other_levels_and_the_wide_model(tmp_path, inputs, which, S, sal, line):
    dirs, metas = inputs
    _compare_single(tmp_path, dirs[which], metas[S], sal, [line])


@pytest.mark.parametrize("sal,extra,lines", [(1, ["-n", "-t", "3", "--null-seed", "7"], PAIRED),
                                             (1, ["-n", "--null-seed", "7", "--null-draws", "3"], PAIRED),
                                             (2, ["--null-seed", "7"], PAIRED[:1])], ids=["s1-fit", "s1-null-draws", "s2"])
def test_paired_groupings_equal_their_commands(tmp_path, inputs, sal, extra, lines):
    dirs, metas = inputs
    common = ["-m", "paired", "-i", str(dirs["txt18"]), "-j", str(metas[18]), "-s", str(sal)] + extra
    out = run_cli(common + ["--groupings", str(_groupings_file(tmp_path / "g.tsv", lines))], tmp_path / "out")
    assert sorted(p.name for p in out.iterdir()) == sorted(l[0] for l in lines)
    for name, a, b in lines:
        sep = run_cli(common + ["--columns-a", a, "--columns-b", b], tmp_path / "sep" / name)
        names = same_tree(out / name, sep)
        assert sum(n.startswith("pairwiseDelta_t_") for n in names) == 3 and "pairwiseMetrics_t.txt.gz" in names


# ---- in process: what a grouping uploads, what stays on the device ------------------------------------------------------------

def _walk(files, out, S=18, sal=1, lines=SINGLE, probe=None):
    infos = []
    for name, _q, results, info in driver.run_groupings(files, [(n, helpers.parseColumns(s)) for n, s in lines], S, sal, out, "t", keep_temps=False):
        assert sorted(results) == ["matrix_chr1", "matrix_chr2", "matrix_chr3"]
        infos.append(info)
        if probe is not None:
            probe(len(infos))
    return infos


def _files(d):
    return sorted(d.glob("*"))


def test_uploads_once_and_memory_does_not_grow(tmp_path, inputs, monkeypatch):
    import torch
    dirs, _metas = inputs
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    held = {}

    def probe(k):
        torch.cuda.synchronize()
        held[k] = torch.cuda.memory_allocated()
    infos = _walk(_files(dirs["txt18"]), tmp_path / "out", probe=probe)
    assert [(i["uploads"], i["parsed_files"]) for i in infos] == [(3, 3), (0, 0), (0, 0)]      # one part per file on one rank
    assert [i["resident_bytes"] for i in infos] == [sum(ROWS) * PITCH] * 3 and infos[0]["refused_files"] == 0
    # Between the groupings a session holds nothing: what may differ is below one grouping's results, float32 scores of every bin:
    # 831 bins x 18 states x 4 B = 59 832 B (what does remain per grouping is the engine's cached membership bytes of its column
    # group, N = 37 B in an allocation of 512 B).
    bound = sum(ROWS) * 18 * 4
    assert held[3] <= held[1] + bound, (held, bound)
    assert held[1] >= sum(ROWS) * PITCH                # (the matrices ARE there)


@pytest.mark.parametrize("cap,later", [(ROWS[0] * PITCH, 2), (0, 3)], ids=["first-file-only", "nothing-kept"])
def test_a_cap_on_the_kept_bytes_reads_again_and_writes_the_same(tmp_path, inputs, monkeypatch, cap, later):
    dirs, _metas = inputs
    files = _files(dirs["txt18"])
    monkeypatch.delenv("EPILOGOS_RESIDENT_BYTES", raising=False)
    _walk(files, tmp_path / "free")
    monkeypatch.setenv("EPILOGOS_RESIDENT_BYTES", str(cap))
    infos = _walk(files, tmp_path / "capped")
    assert [(i["uploads"], i["parsed_files"]) for i in infos] == [(3, 3)] + [(later, later)] * 2
    assert all(i["resident_bytes"] == cap and i["kept_files"] == 3 - later for i in infos)
    for name, _spec in SINGLE:
        names = same_tree(tmp_path / "capped" / name, tmp_path / "free" / name)
        assert names == ["exp_freq_t.npy"] + ["scores_t_matrix_chr%d.txt.gz" % k for k in (1, 2, 3)]


# ---- two ranks, --check-states ------------------------------------------------------------------------------------------------

def _child(args, out, env_extra=()):
    """A command that may fail -> the finished process."""
    if _broken:
        pytest.fail("not started: an earlier child process failed (%s)" % _broken[0])
    env = dict(os.environ, PYTHONPATH=str(ROOT), **dict(env_extra))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "epilogos_amd.run", "-l"] + args + ["-o", str(out), "-f", "t"]
    try:
        return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
        _broken.append(" ".join(cmd))
        raise


def test_two_ranks_sharing_the_gpu_equal_one_rank(tmp_path, inputs):
    """`--gpus 2` from a plain start, the two ranks on the one GPU over gloo (as tests/test_hip_pipeline.py starts them): text
    inputs take the parse-once route, each rank keeps the files it parsed, the border pieces' histograms change hands per grouping.
    The grouping that is compared is the SECOND line of its file: the one whose matrices come out of the two ranks' stores."""
    dirs, metas = inputs
    single = ["-i", str(dirs["txt18"]), "-j", str(metas[18]), "-s", "1"]
    paired = ["-m", "paired"] + single + ["--null-seed", "7"]
    for tag, common, lines in (("s", single, [SINGLE[1], SINGLE[2]]), ("p", paired, [PAIRED[1], PAIRED[0]])):
        res = _child(common + ["--groupings", str(_groupings_file(tmp_path / (tag + ".tsv"), lines)), "--gpus", "2"], tmp_path / (tag + "2"),
                     {"EPILOGOS_DIST_BACKEND": "gloo"})
        if res.returncode != 0 or "ERROR" in res.stdout:
            _broken.append("--groupings --gpus 2 (%s)" % tag)
            pytest.fail(res.stdout + res.stderr)
        assert "GPUs = 2" in res.stdout and "Grouping 2 of 2: %s" % lines[1][0] in res.stdout and "stay on the device" not in res.stdout
        cols = ["--columns", lines[1][1]] if tag == "s" else ["--columns-a", lines[1][1], "--columns-b", lines[1][2]]
        one = run_cli(common + cols, tmp_path / (tag + "1"))
        names = same_tree(tmp_path / (tag + "2") / lines[1][0], one, decompress=True)
        assert sorted(p.name for p in (tmp_path / (tag + "2") / lines[0][0]).iterdir()) == names


def test_check_states_stops_before_any_grouping_writes(tmp_path, inputs):
    dirs, metas = inputs
    bad = tmp_path / "bad"
    shutil.copytree(dirs["epgm18"], bad)
    with open(bad / "matrix_chr2.epgm", "r+b") as fh:              # the second file's only row, biosample 4: a byte that is no state
        fh.seek(sbl.HEADER_BYTES + 3)
        fh.write(bytes([33]))
    g = _groupings_file(tmp_path / "g.tsv", SINGLE)
    res = _child(["-i", str(bad), "-j", str(metas[18]), "--groupings", str(g), "--check-states"], tmp_path / "out")
    said = [l for l in (res.stdout + res.stderr).splitlines() if "[--check-states]" in l]
    assert res.returncode == 1, res.stdout + res.stderr
    assert said == [driver.state_check_message(str(bad / "matrix_chr2.epgm"), 0, 4, 33, 18)], res.stdout + res.stderr
    left = [str(p) for p in (tmp_path / "out").rglob("*") if p.is_file()] if (tmp_path / "out").exists() else []
    assert left == []
    # the clean set with the option: the run is the run without it
    ok = run_cli(["-i", str(dirs["epgm18"]), "-j", str(metas[18]), "--groupings", str(_groupings_file(tmp_path / "g1.tsv", SINGLE[1:2])),
                  "--check-states"], tmp_path / "checked")
    plain = run_cli(["-i", str(dirs["epgm18"]), "-j", str(metas[18]), "--columns", SINGLE[1][1]], tmp_path / "plain")
    same_tree(ok / "one", plain)
