"""GPU: the census through the commands.  `epilogos-prep --census` on the golden state-by-line calls and on the golden segment
files writes the table of the .epgm files it writes (numpy's census of their bytes) and leaves those bytes alone;
`python -m epilogos_amd.census` gives the same lines from the .epgm files, from the same matrices as .txt.gz and with --names;
`epilogos --check-states` changes nothing on a clean set, and on a patched set it stops every rank together, after STEP 1, with
one message that names the first byte that is no state."""
import gzip
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from epilogos_amd import census, preprocess, stateByLine as sbl
from tests.conftest import free_port
from tests.test_hip_groups_pipeline import ROOT, run_cli, same_outputs
from tests.test_hip_segments_pipeline import _golden_tree
from tests.test_host_logic import write_tsv
from tests.test_statebyline_host import GOLD

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 180                                      # seconds: a run takes a few, the start of a process included
S = 18


def _states_file(path, short=True):
    path.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)) if short else
                    "zero_index\tone_index\n" + "".join("%d\t%d\n" % (i, i + 1) for i in range(S)))
    return path


def _epgm_bytes(path):
    h = sbl.read_epgm_header(path)
    body = np.fromfile(path, dtype=np.uint8, offset=sbl.HEADER_BYTES).reshape(h["R"], h["N"])
    return h, body


def numpy_entry(path, nstates, names=None):
    h, x = _epgm_bytes(path)
    c = np.stack([np.bincount(x[:, n], minlength=256)[:nstates] for n in range(h["N"])]) if h["N"] else np.zeros((0, nstates), dtype=np.int64)
    return h["chrom"], c.astype(np.int64), h["R"] - c.sum(axis=1), h["R"], names


def rows_of(text, nstates=S):
    """The table without its head and without the biosample names, the state columns padded with zeros to `nstates`."""
    out = []
    for l in text.splitlines()[1:]:
        f = l.split("\t")
        assert int(f[3]) == int(f[4]) + sum(int(v) for v in f[5:]), l
        out.append((f[0], int(f[1]), int(f[3]), int(f[4])) + tuple(int(v) for v in f[5:]) + (0,) * (nstates - len(f[5:])))
    return out


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    """The golden calls as state-by-line files and as segment files, each prepared with and without --census."""
    base = tmp_path_factory.mktemp("census_golden")
    d = base / "sbl" / "calls"
    d.mkdir(parents=True)
    for k, n in enumerate(GOLD["names"]):
        with gzip.open(d / str(n), "wb") as fh:
            fh.write(GOLD["text_%d" % k].tobytes())
    for sub in ("sbl", "seg"):
        (base / sub / "meta.txt").parent.mkdir(parents=True, exist_ok=True)
        (base / sub / "meta.txt").write_bytes(GOLD["metadata"].tobytes())
        (base / sub / "sizes.txt").write_bytes(GOLD["chromsizes"].tobytes())
    _golden_tree(base / "seg")
    made = {}
    for sub, seg in (("sbl", False), ("seg", True)):
        b = base / sub
        plain, with_census = io.StringIO(), io.StringIO()
        w0 = preprocess.run(b / "calls", b / "meta.txt", b / "sizes.txt", b / "plain", out=plain, segments=seg)
        w1 = preprocess.run(b / "calls", b / "meta.txt", b / "sizes.txt", b / "census", out=with_census, segments=seg, census=b / "census.tsv")
        made[sub] = (w0, w1, plain.getvalue(), with_census.getvalue(), b / "census.tsv", b / "meta.txt")
    return base, made


@pytest.mark.parametrize("route", ["sbl", "seg"])
def test_prep_census_is_the_numpy_census_of_the_files_written(golden, route):
    _base, made = golden
    w0, w1, out0, out1, table, meta = made[route]
    assert out0 == out1 and [p.name for p in w0] == [p.name for p in w1] and w1
    for a, b in zip(w0, w1):
        assert a.read_bytes() == b.read_bytes(), a.name                          # the option leaves the .epgm bytes alone
    names = census.read_names(meta)
    heads = table.read_text().splitlines()[0].split("\t")
    assert heads[:5] == census.HEAD and heads[5:] == [str(k) for k in range(1, len(heads) - 4)]
    nstates = len(heads) - 5
    assert nstates == max(sbl.read_epgm_header(p)["hi"] for p in w1)
    want = census.table_lines([numpy_entry(p, nstates, names) for p in w1], heads[5:])
    assert table.read_text() == "\n".join(want) + "\n"
    assert [l.split("\t")[2] for l in want[1:1 + len(names)]] == names and want[-1].startswith("all\t%d\t" % len(names))


def test_census_command_on_epgm_text_and_with_names(golden, tmp_path):
    _base, made = golden
    _w0, w1, _o0, _o1, table, meta = made["sbl"]
    want = rows_of(table.read_text())
    states = _states_file(tmp_path / "states.tsv")
    # the .epgm files, as a child process writing to stdout: the command line itself
    res = subprocess.run([sys.executable, "-m", "epilogos_amd.census", "-i", str(w1[0].parent), "-j", str(states)], capture_output=True, text=True,
                         timeout=CHILD_LIMIT, cwd=str(ROOT), env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert lines[0].split("\t") == census.HEAD + ["state%d" % k for k in range(1, S + 1)]
    assert rows_of(res.stdout) == want and {l.split("\t")[2] for l in lines[1:]} == {"."}
    # the same matrices as text, in process, into a file; then with --names
    txt = tmp_path / "txt"
    txt.mkdir()
    for p in w1:
        h, x = _epgm_bytes(p)
        write_tsv(txt / (p.name.split(".")[0] + ".txt.gz"), x.view(np.int8).astype(np.int64), chrom=h["chrom"])
    census.run([txt], _states_file(tmp_path / "plain.tsv", short=False), out=tmp_path / "t.tsv")
    got = (tmp_path / "t.tsv").read_text()
    assert got.splitlines()[0].split("\t")[5:] == [str(k) for k in range(1, S + 1)] and rows_of(got) == want
    census.run([str(p) for p in w1], states, out=tmp_path / "n.tsv", names=meta)
    named = (tmp_path / "n.tsv").read_text()
    assert rows_of(named) == want
    assert [l.split("\t")[2] for l in named.splitlines()[1:]] == [l.split("\t")[2] for l in table.read_text().splitlines()[1:]]


def test_census_counts_a_files_bytes_and_the_next_read_clamps_again(golden, tmp_path):
    """The census command reads a .epgm file's bytes as they are -- for its own reads only: an ordinary read of the same file in the
    same process afterwards stores what is no state as -1, as before (a byte 33 must never reach the count kernels as state 1)."""
    from epilogos_amd import helpers
    _base, made = golden
    src = made["sbl"][1][0]
    h, _x = _epgm_bytes(src)
    p = tmp_path / src.name
    shutil.copy(src, p)
    with open(p, "r+b") as fh:
        fh.seek(sbl.HEADER_BYTES + 5 * h["N"] + 2)
        fh.write(bytes([33]))
    warnings = io.StringIO()
    entries = census.run([p], _states_file(tmp_path / "states.tsv"), out=tmp_path / "t.tsv", err=warnings)
    want = numpy_entry(p, S)
    assert np.array_equal(entries[0][1], want[1]) and np.array_equal(entries[0][2], want[2]) and int(want[2].sum()) >= 1
    _h, xp = _epgm_bytes(p)
    first = int(np.flatnonzero(xp.reshape(-1) >= S)[0])
    assert "the first is byte %d at row %d (0-based), biosample %d" % (xp.reshape(-1)[first], first // h["N"], first % h["N"] + 1) \
        in warnings.getvalue()
    after = helpers.readTable(p)[0]
    assert after[5, 2] == -1 and ((after >= 0) | (after == -1)).all()
    assert helpers.readTable(p, raw=True)[0][5, 2] == 33


# ---- epilogos --check-states -------------------------------------------------------------------------------------------------

ROWS, NCOL = 300, 20


def _write_set(d, seed):
    d.mkdir(parents=True)
    rng = np.random.default_rng(seed)
    for k in (1, 2, 3):
        x = np.where(rng.random((ROWS, NCOL)) < 0.5, S - 1, rng.integers(0, S, size=(ROWS, NCOL))).astype(np.int8)
        sbl.write_epgm(d / ("matrix_chr%d.epgm" % k), x, "chr%d" % k, (1, S))
    return d


def _patch(path, row, col, byte):
    with open(path, "r+b") as fh:
        fh.seek(sbl.HEADER_BYTES + row * NCOL + col)
        fh.write(bytes([byte]))


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    base = tmp_path_factory.mktemp("check_states")
    clean = _write_set(base / "clean", 1)
    bad = base / "bad"
    shutil.copytree(clean, bad)
    _patch(bad / "matrix_chr2.epgm", 10, 3, 33)                   # an alias of state 1 ...
    _patch(bad / "matrix_chr1.epgm", 211, 7, 200)                 # ... then an earlier byte (in run order) of file 1
    other = _write_set(base / "otherA", 2)                        # paired: group A, with the patched set as group B; its own offender
    _patch(other / "matrix_chr1.epgm", 250, 0, 0xFF)              # lies in the same file at a LATER row, so group B's comes first
    return base, clean, bad, other, _states_file(base / "states.tsv")


def _run(args, out, world=1):
    """run_cli's command (tests/test_hip_groups_pipeline.py) for a run that is expected to fail: -> the finished process."""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "epilogos_amd.run", "-l"] + args + ["-o", str(out), "-f", "t"]
    if world > 1:
        port = str(free_port())
        env.update(EPILOGOS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", port] + cmd[1:]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=str(ROOT))


def _expected(bad):
    from epilogos_amd import driver
    return [driver.state_check_message(str(bad / "matrix_chr1.epgm"), 211, 8, 200, S)]


def _verdicts(res):
    return [l for l in (res.stdout + res.stderr).splitlines() if "[--check-states]" in l]


def _nothing_written(out):
    left = [p.name for p in out.iterdir()] if out.exists() else []
    assert not [n for n in left if n.startswith(("scores_", "exp_freq_", "regionsOfInterest_", "pairwise", "significantLoci", ".part_"))], left


def test_clean_set_is_unchanged_by_the_option(sets, tmp_path):
    _base, clean, _bad, _other, states = sets
    a = run_cli(["-i", str(clean), "-j", str(states)], tmp_path / "plain")
    b = run_cli(["-i", str(clean), "-j", str(states), "--check-states"], tmp_path / "checked")
    names = same_outputs(a, b)
    assert sum(n.startswith("scores_") for n in names) == 3


def test_patched_set_fails_and_names_the_first_byte(sets, tmp_path):
    _base, _clean, bad, _other, states = sets
    res = _run(["-i", str(bad), "-j", str(states), "--check-states"], tmp_path / "o")
    assert res.returncode != 0, res.stdout + res.stderr
    msg = _verdicts(res)
    assert msg == _expected(bad), res.stdout + res.stderr
    assert str(bad / "matrix_chr1.epgm") in msg[0] and "row 211 " in msg[0] and "biosample 8:" in msg[0] and "byte 200 " in msg[0] \
        and "%d-state" % S in msg[0] and "matrix_chr2" not in msg[0]
    _nothing_written(tmp_path / "o")
    # --columns: the check still covers every biosample column of the file
    res = _run(["-i", str(bad), "-j", str(states), "--check-states", "--columns", "1-5"], tmp_path / "c")
    assert res.returncode != 0 and _verdicts(res) == msg


def test_patched_set_without_the_option_runs_as_before(sets, tmp_path):
    """Without the option the run is what it was before the option existed: no census, no message of it.  The reader of .epgm files
    stores the two bytes as -1, the count pass counts them nowhere, and the count check behind STEP 1 stops the run with its own
    message (no position) -- so an aliasing byte of a .epgm file never reached the kernels, with or without the option."""
    _base, _clean, bad, _other, states = sets
    res = _run(["-i", str(bad), "-j", str(states)], tmp_path / "o")
    out = res.stdout + res.stderr
    assert not _verdicts(res), out
    assert "STEP 1-3" in res.stdout, out                                           # the run got as far as the count pass
    assert res.returncode != 0 and "input contains states outside 1..numStates" in out, out


def test_two_ranks_stop_together_with_the_one_message(sets, tmp_path):
    _base, _clean, bad, _other, states = sets
    res = _run(["-i", str(bad), "-j", str(states), "--check-states"], tmp_path / "two", world=2)     # (a rank left waiting: TimeoutExpired)
    assert res.returncode != 0, res.stdout + res.stderr
    assert _verdicts(res) == _expected(bad), res.stdout + res.stderr               # the one-rank run's message, once
    _nothing_written(tmp_path / "two")


def test_paired_mode_checks_both_groups(sets, tmp_path):
    _base, _clean, bad, other, states = sets
    res = _run(["-m", "paired", "-a", str(other), "-b", str(bad), "-j", str(states), "--check-states"], tmp_path / "p")
    assert res.returncode != 0, res.stdout + res.stderr
    assert _verdicts(res) == _expected(bad), res.stdout + res.stderr
    _nothing_written(tmp_path / "p")
