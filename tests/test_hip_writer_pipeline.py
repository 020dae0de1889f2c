"""GPU: `epilogos --writer gpu` end to end against `--writer host`, on two small chromosomes (650 and 300 bins, 12 biosample columns,
an 18-state model): the output directories hold the same file names, every .gz decompresses to identical bytes, every other file is
byte-identical, and the score files of the device run are BGZF that tests/bgzf_ref.walk accepts.  The commands run in this process
(click's CliRunner, as tests/test_hip_pipeline.py does); --gpus 2 is two ranks over gloo on the one GPU, a child process
(tests/test_hip_groups_pipeline.run_cli).  In the paired run no delta array comes down: the sessions count their downloads."""
import gzip

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import bgzf_ref
from tests.test_hip_groupings_pipeline import _groupings_file
from tests.test_hip_groups_pipeline import run_cli
from tests.test_host_logic import write_tsv

pytestmark = pytest.mark.gpu

ROWS, N, S = (650, 300), 12, 18
A, B = "1-6", "7-12"


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from epilogos_amd import engine
    engine.require_gpu()
    base = tmp_path_factory.mktemp("writer")
    d = base / "whole"
    d.mkdir()
    rng = np.random.default_rng(23)
    mats = []
    for k, r in enumerate(ROWS):
        x = np.where(rng.random((r, N)) < 0.5, S - 1, rng.integers(0, S, size=(r, N)))
        x[rng.random(r) < 0.15] = S - 1
        x[40:70] = x[40]                                                         # a run of equal rows: equal score rows, row matches
        write_tsv(d / ("matrix_chr%d.txt.gz" % (k + 1)), x, chrom="chr%d" % (k + 1), start0=99000)
        mats.append(x)
    meta = base / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    return base, d, meta, mats


def invoke(args, out):
    from click.testing import CliRunner

    from epilogos_amd import driver, run
    try:
        res = CliRunner().invoke(run.main, ["-l"] + args + ["-o", str(out), "-f", "t"])
    finally:
        driver.finish_writes()
    assert res.exit_code == 0 and "ERROR" not in res.output, "%s\n%s" % (res.output, res.exception)
    return res.output


def same_outputs(host, gpu, kind):
    """-> the names; the score files of `gpu` are BGZF with one end-of-file block."""
    names = sorted(p.name for p in host.iterdir())
    assert names == sorted(p.name for p in gpu.iterdir()) and not [n for n in names if n.startswith(".part_")]
    text = [n for n in names if n.startswith(kind + "_")]
    assert len(text) == len(ROWS)
    for n in names:
        if (host / n).is_dir():
            continue
        if n.endswith(".gz"):
            assert gzip.decompress((host / n).read_bytes()) == gzip.decompress((gpu / n).read_bytes()), n
        else:
            assert (host / n).read_bytes() == (gpu / n).read_bytes(), n
    for n in text:
        blob = (gpu / n).read_bytes()
        ms = bgzf_ref.walk(blob)
        assert blob.count(bgzf_ref.EOF) == 1 and all(m.bsize <= 65536 for m in ms)
        with pytest.raises(bgzf_ref.BgzfError):                                 # (the host's own file is not: the comparison is between two writers)
            bgzf_ref.walk((host / n).read_bytes())
    return names


def both(tmp_path, args, kind="scores"):
    out = invoke(args + ["--writer", "host"], tmp_path / "host")
    out_gpu = invoke(args + ["--writer", "gpu"], tmp_path / "gpu")
    assert "WARNING:" not in out_gpu and out.count("[Done]") == out_gpu.count("[Done]")
    return same_outputs(tmp_path / "host", tmp_path / "gpu", kind)


@pytest.mark.parametrize("sal", [1, 2, 3])
def test_single_mode(tmp_path, inputs, sal):
    _base, d, meta, _mats = inputs
    names = both(tmp_path, ["-i", str(d), "-j", str(meta), "-s", str(sal), "-w", "5"])
    assert any(n.startswith("regionsOfInterest_") for n in names)


def test_paired_with_null_and_no_delta_download(tmp_path, inputs):
    from epilogos_amd import backend
    _base, d, meta, _mats = inputs
    args = ["-m", "paired", "-i", str(d), "--columns-a", A, "--columns-b", B, "-j", str(meta), "-n", "--null-seed", "7", "-t", "5", "-z", "200",
            "--fit", "gpu", "-w", "5"]
    backend._HipSession.downloaded.clear()
    invoke(args + ["--writer", "host"], tmp_path / "host")
    assert backend._HipSession.downloaded["delta"] == len(ROWS)
    backend._HipSession.downloaded.clear()
    out = invoke(args + ["--writer", "gpu"], tmp_path / "gpu")
    assert backend._HipSession.downloaded["delta"] == 0 and "WARNING:" not in out
    names = same_outputs(tmp_path / "host", tmp_path / "gpu", "pairwiseDelta")
    assert any(n.startswith("pairwiseMetrics_") for n in names)


def test_eight_columns(tmp_path, inputs):
    _base, d, meta, _mats = inputs
    both(tmp_path, ["-i", str(d), "-j", str(meta), "--columns", "1-3,5,7-9,12", "-w", "5"])


def test_a_groupings_file_of_two_lines(tmp_path, inputs):
    base, d, meta, _mats = inputs
    g = _groupings_file(base / "g.tsv", [("first", A, B), ("second", "1-3", "4-12")])
    args = ["-m", "paired", "-i", str(d), "-j", str(meta), "--null-seed", "7", "--groupings", str(g), "-w", "5"]
    invoke(args + ["--writer", "host"], tmp_path / "host")
    invoke(args + ["--writer", "gpu"], tmp_path / "gpu")
    for name in ("first", "second"):
        same_outputs(tmp_path / "host" / name, tmp_path / "gpu" / name, "pairwiseDelta")


def test_chromhmm(tmp_path, inputs):
    _base, _d, meta, mats = inputs
    calls = tmp_path / "roadmap"
    calls.mkdir()
    for c, x in zip(("chr1", "chr2"), mats):
        for k in range(N):
            (calls / ("B%03d_18_%s_statebyline.txt" % (k, c))).write_bytes(
                b"B%03d\t%s\nMaxStateE\n" % (k, c.encode()) + "".join("%d\n" % (s + 1) for s in x[:, k]).encode())
    ids = tmp_path / "ids.txt"
    ids.write_text("id\n" + "".join("B%03d\n" % k for k in range(N)))
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join("%s\t%d\n" % (c, r * 200) for c, r in zip(("chr1", "chr2"), ROWS)))
    both(tmp_path, ["--chromhmm", str(calls), "--metadata", str(ids), "--chromsizes", str(sizes), "-j", str(meta), "-w", "5"])


def test_two_ranks_on_one_gpu(tmp_path, inputs):
    """Every rank compresses its own parts; a chromosome cut by the ranks' border is assembled from part files that carry no
    end-of-file block."""
    _base, d, meta, _mats = inputs
    args = ["-i", str(d), "-j", str(meta), "-w", "5"]
    one = run_cli(args + ["--writer", "host"], tmp_path / "host")
    two = run_cli(args + ["--writer", "gpu"], tmp_path / "gpu", world=2)
    same_outputs(one, two, "scores")


def test_a_nan_score_sends_that_file_through_the_host_writer_with_one_warning(tmp_path, inputs, monkeypatch, capsys):
    from epilogos_amd import backend, driver
    _base, d, _meta, _mats = inputs
    files = sorted(d.iterdir())
    begin = backend._HipSingleSession._begin

    def poisoned(self, pids):
        begin(self, pids)
        for t in self._early.values():
            if t.shape[0] == 300:
                t[5, 2] = float("nan")
    monkeypatch.setattr(backend._HipSingleSession, "_begin", poisoned)
    for w in ("host", "gpu"):
        (tmp_path / w).mkdir()
        capsys.readouterr()
        driver.run_single_group(files, S, 1, tmp_path / w, "t", keep_temp_scores=False, writer=w)
        lines = [l for l in capsys.readouterr().out.splitlines() if "WARNING:" in l]
        assert len(lines) == (1 if w == "gpu" else 0)
    assert "scores_t_matrix_chr2.txt.gz" in lines[0] and "host writer" in lines[0]
    for n in ("scores_t_matrix_chr1.txt.gz", "scores_t_matrix_chr2.txt.gz"):
        a, b = gzip.decompress((tmp_path / "host" / n).read_bytes()), gzip.decompress((tmp_path / "gpu" / n).read_bytes())
        assert a == b and (b"\tnan\t" in a) == (n.endswith("chr2.txt.gz"))
    assert bgzf_ref.walk((tmp_path / "gpu" / "scores_t_matrix_chr1.txt.gz").read_bytes())
    with pytest.raises(bgzf_ref.BgzfError):
        bgzf_ref.walk((tmp_path / "gpu" / "scores_t_matrix_chr2.txt.gz").read_bytes())
