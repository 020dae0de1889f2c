"""GPU: the concordance through the commands.  `python -m epilogos_amd.concordance` on a .epgm, a .txt and a .txt.gz file writes
the restatement of all their rows, under --names and --columns, and warns about a duplicated column; `epilogos-prep
--concordance` on the golden state-by-line calls and on the golden segment files writes what the command then writes from the
.epgm files it left, and leaves those files and its progress lines alone."""
import io
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from epilogos_amd import census, concordance, preprocess, stateByLine as sbl
from epilogos_amd.run import parseColumns
from tests.test_concordance_host import restatement
from tests.test_hip_groups_pipeline import ROOT
from tests.test_hip_segments_pipeline import _golden_tree
from tests.test_host_logic import write_tsv
from tests.test_statebyline_host import GOLD

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 180                                      # seconds: a run takes a few, the start of a process included
S = 18
NCOL = 7


def _states_file(path):
    path.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    return path


def test_command_on_epgm_text_and_gzip(tmp_path):
    rng = np.random.default_rng(5)
    d = tmp_path / "in"
    d.mkdir()
    xs = []
    for k, rows in enumerate((300, 170, 233)):
        x = np.where(rng.random((rows, NCOL)) < 0.5, S - 1, rng.integers(0, S, size=(rows, NCOL))).astype(np.int8)
        x[:, 6] = x[:, 1]                                                        # a duplicated biosample
        xs.append(x)
    xs[1][5, 2] = -1                                                             # the second file: a cell that is no state
    sbl.write_epgm(d / "matrix_chr1.epgm", xs[0], "chr1", (1, S))
    write_tsv(d / "matrix_chr2.txt", xs[1], chrom="chr2")
    write_tsv(d / "matrix_chr3.txt.gz", xs[2], chrom="chr3")
    meta = tmp_path / "meta.txt"
    meta.write_text("biosample\ttissue\n" + "".join("BSS%02d\tx\n" % k for k in range(1, NCOL + 1)))
    states = _states_file(tmp_path / "states.tsv")
    res = subprocess.run([sys.executable, "-m", "epilogos_amd.concordance", "-i", str(d), "-j", str(states), "-o", str(tmp_path / "all"),
                          "--names", str(meta)], capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=str(ROOT),
                         env=dict(os.environ, PYTHONPATH=str(ROOT)))
    assert res.returncode == 0, res.stdout + res.stderr
    wa, wb = restatement(np.concatenate(xs), S)
    assert wb[2, 2] == sum(x.shape[0] for x in xs) - 1
    names = census.read_names(meta)
    assert (tmp_path / "all.agree.tsv").read_text() == "\n".join(concordance.table_lines(wa, names)) + "\n"
    assert (tmp_path / "all.both.tsv").read_text() == "\n".join(concordance.table_lines(wb, names)) + "\n"
    warned = [l for l in res.stderr.splitlines() if l.startswith("WARNING:")]
    assert warned == [concordance.duplicate_warning(wa, wb, names)] and "1 pair(s)" in warned[0] and "BSS02 (column 2) and BSS07 (column 7)" in warned[0]
    # in process, with --columns and without names; the warning is about the whole matrix
    err = io.StringIO()
    a, b = concordance.run([d], states, tmp_path / "some", columns="5,1-2", err=err)
    assert np.array_equal(a, wa) and np.array_equal(b, wb)
    cols = parseColumns("5,1-2")
    assert (tmp_path / "some.agree.tsv").read_text() == "\n".join(concordance.table_lines(wa, None, cols)) + "\n"
    assert (tmp_path / "some.both.tsv").read_text() == "\n".join(concordance.table_lines(wb, None, cols)) + "\n"
    assert (tmp_path / "some.agree.tsv").read_text().splitlines()[0] == "biosample\t5\t1\t2"
    assert err.getvalue() == concordance.duplicate_warning(wa, wb) + "\n"


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    """The golden calls as state-by-line files and as segment files, each prepared with and without --concordance."""
    base = tmp_path_factory.mktemp("concordance_golden")
    d = base / "sbl" / "calls"
    d.mkdir(parents=True)
    for k, n in enumerate(GOLD["names"]):
        with gzip.open(d / str(n), "wb") as fh:
            fh.write(GOLD["text_%d" % k].tobytes())
    (base / "sbl" / "meta.txt").write_bytes(GOLD["metadata"].tobytes())
    (base / "sbl" / "sizes.txt").write_bytes(GOLD["chromsizes"].tobytes())
    _golden_tree(base / "seg")
    made = {}
    for sub, seg in (("sbl", False), ("seg", True)):
        b = base / sub
        plain, with_option = io.StringIO(), io.StringIO()
        w0 = preprocess.run(b / "calls", b / "meta.txt", b / "sizes.txt", b / "plain", out=plain, segments=seg)
        w1 = preprocess.run(b / "calls", b / "meta.txt", b / "sizes.txt", b / "pairs", out=with_option, segments=seg, concordance=b / "prep")
        made[sub] = (w0, w1, plain.getvalue(), with_option.getvalue(), b / "prep", b / "meta.txt")
    return made


@pytest.mark.parametrize("route", ["sbl", "seg"])
def test_prep_writes_what_the_command_writes_from_its_files(golden, route, tmp_path):
    w0, w1, out0, out1, prefix, meta = golden[route]
    assert out0 == out1 and [p.name for p in w0] == [p.name for p in w1] and w1
    for a, b in zip(w0, w1):
        assert a.read_bytes() == b.read_bytes(), a.name                          # the option leaves the .epgm bytes alone
    concordance.run([str(p) for p in w1], _states_file(tmp_path / "states.tsv"), tmp_path / "cmd", names=meta, err=io.StringIO())
    bodies = []
    for p in w1:
        h = sbl.read_epgm_header(p)
        bodies.append(np.fromfile(p, dtype=np.uint8, offset=sbl.HEADER_BYTES).reshape(h["R"], h["N"]))
    wa, wb = restatement(np.concatenate(bodies), S)
    names = census.read_names(meta)
    for tag, want in (("agree", wa), ("both", wb)):
        text = (tmp_path / ("cmd.%s.tsv" % tag)).read_text()
        assert text == "\n".join(concordance.table_lines(want, names)) + "\n"
        assert (prefix.parent / (prefix.name + ".%s.tsv" % tag)).read_text() == text
    assert wa.shape[0] == len(names) and wb.diagonal().sum() > 0
