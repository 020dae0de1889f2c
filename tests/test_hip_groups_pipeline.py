"""GPU: the commands with column groups write, byte for byte, what today's commands write from inputs with those columns cut
out beforehand -- same -f, same --null-seed: scores_* / pairwiseDelta_*.txt.gz (compared decompressed), regionsOfInterest_* and
the paired metrics files; every file a command leaves in its output directory is compared.  (exp_freq_*.npy is removed by STEP 4
like the reference does; the scores are computed from it, and tests/test_hip_groups_sessions.py compares it bit for bit.)

Inputs: three files of 64, 301 and 1 rows, 40 biosamples; an 18-state model, and a 3-state and a 40-state model for the smallest
core and for the wide path (device gather).  The cut files are written here with numpy.  Every run is a child process with a time
limit of its own; once a child has failed or run out of time no further child is started."""
import gzip
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.conftest import free_port
from tests.test_host_logic import write_tsv

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ROWS, N = (64, 301, 1), 40
SINGLE = "1-3,6-9,12,17-20,24,31-32,39,40"            # a scattered group with both ends of the row: 17 biosamples
SPEC_A, SPEC_B = "1-17", "20-40"
CHILD_LIMIT = 240                                      # seconds: a run takes a few, the start of a process included
_broken = []                                           # the first child that failed: nothing is started after it


def _parse(spec):
    from epilogos_amd.run import parseColumns
    return parseColumns(spec)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{S: (whole dir, {spec: cut dir}, metadata)} for the three models."""
    base = tmp_path_factory.mktemp("groups")
    made = {}
    for S in (3, 18, 40):
        rng = np.random.default_rng(S)
        d = base / ("s%d" % S)
        whole = d / "whole"
        whole.mkdir(parents=True)
        cuts = {spec: d / ("cut_" + tag) for spec, tag in ((SINGLE, "one"), (SPEC_A, "A"), (SPEC_B, "B"))}
        for c in cuts.values():
            c.mkdir()
        for k, r in enumerate(ROWS):
            x = np.where(rng.random((r, N)) < 0.5, S - 1, rng.integers(0, S, size=(r, N)))
            quiet = rng.random(r) < 0.2                # quiescent in both paired groups, not in biosamples 18 and 19
            x[quiet] = S - 1
            x[quiet, 17:19] = 0
            name = "matrix_chr%d.txt.gz" % (k + 1)
            write_tsv(whole / name, x, chrom="chr%d" % (k + 1))
            for spec, c in cuts.items():
                write_tsv(c / name, x[:, _parse(spec)], chrom="chr%d" % (k + 1))
        meta = d / "metadata.tsv"
        meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
        made[S] = (whole, cuts, meta)
    return made


def run_cli(args, out, world=1):
    """One command as a child process -> its output directory.  Two ranks: torch.distributed.run, gloo, both on the one GPU."""
    if _broken:
        pytest.fail("not started: an earlier child process failed (%s)" % _broken[0])
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "epilogos_amd.run", "-l"] + args + ["-o", str(out), "-f", "t"]
    if world > 1:
        port = str(free_port())
        env.update(EPILOGOS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", port] + cmd[1:]
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
        _broken.append(" ".join(cmd))
        raise
    if res.returncode != 0 or "ERROR" in res.stdout:
        _broken.append(" ".join(cmd))
        pytest.fail("%s\n%s%s" % (" ".join(cmd), res.stdout, res.stderr))
    return out


def same_outputs(a, b):
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    assert any(n.startswith("regionsOfInterest_") for n in names)
    for n in names:
        if n.endswith(".gz"):
            with gzip.open(a / n, "rb") as fa, gzip.open(b / n, "rb") as fb:
                assert fa.read() == fb.read(), n
        else:
            assert (a / n).read_bytes() == (b / n).read_bytes(), n
    return names


@pytest.mark.parametrize("S,sal", [(18, 1), (18, 2), (18, 3), (3, 1), (40, 1), (40, 2)])
def test_single_columns_equal_cut_files(tmp_path, inputs, S, sal):
    whole, cuts, meta = inputs[S]
    common = ["-j", str(meta), "-s", str(sal)]
    cut = run_cli(["-i", str(cuts[SINGLE])] + common, tmp_path / "cut")
    col = run_cli(["-i", str(whole), "--columns", SINGLE] + common, tmp_path / "col")
    names = same_outputs(col, cut)
    assert sum(n.startswith("scores_t_") for n in names) == 3
    with gzip.open(col / "scores_t_matrix_chr2.txt.gz", "rt") as fh:
        rows = fh.read().splitlines()
    assert len(rows) == 301 and len(rows[0].split("\t")) == 3 + S


@pytest.mark.parametrize("S,sal,g", [(18, 1, None), (18, 2, None), (18, 1, 10), (18, 2, 10), (3, 1, None), (40, 1, None), (40, 2, 10)])
def test_paired_columns_equal_cut_directories(tmp_path, inputs, S, sal, g):
    whole, cuts, meta = inputs[S]
    common = ["-m", "paired", "-j", str(meta), "-s", str(sal), "--null-seed", "77"] + (["-g", str(g)] if g else [])
    cut = run_cli(["-a", str(cuts[SPEC_A]), "-b", str(cuts[SPEC_B])] + common, tmp_path / "cut")
    col = run_cli(["-i", str(whole), "--columns-a", SPEC_A, "--columns-b", SPEC_B] + common, tmp_path / "col")
    names = same_outputs(col, cut)
    assert sum(n.startswith("pairwiseDelta_t_") for n in names) == 3 and any(n.startswith("pairwiseMetrics_") for n in names)


@pytest.mark.parametrize("paired", [False, True])
def test_two_ranks_sharing_the_gpu_equal_one_rank(tmp_path, inputs, paired):
    whole, _cuts, meta = inputs[18]
    args = ["-i", str(whole), "-j", str(meta), "-s", "1"]
    args += ["-m", "paired", "--columns-a", SPEC_A, "--columns-b", SPEC_B, "--null-seed", "77"] if paired else ["--columns", SINGLE]
    one = run_cli(args, tmp_path / "one")
    two = run_cli(args, tmp_path / "two", world=2)
    same_outputs(two, one)


def test_default_tag_of_paired_columns(tmp_path, inputs):
    whole, _cuts, meta = inputs[18]
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    if _broken:
        pytest.fail("not started: an earlier child process failed (%s)" % _broken[0])
    res = subprocess.run([sys.executable, "-m", "epilogos_amd.run", "-l", "-m", "paired", "-i", str(whole), "--columns-a", SPEC_A, "--columns-b",
                          SPEC_B, "-j", str(meta), "-o", str(tmp_path / "o"), "--null-seed", "1"], env=env, capture_output=True, text=True,
                         timeout=CHILD_LIMIT, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout + res.stderr
    assert (tmp_path / "o" / "pairwiseDelta_whole_A_whole_B_s1_matrix_chr2.txt.gz").exists()
