"""GPU: `epilogos --roi gpu --metrics gpu` end to end, through run.py's entry point in this process: three .epgm files of 300, 150 and
200 bins, 12 biosample columns split 6 + 6, --null-seed 7, -w 10.  Four modes -- single, paired, paired -n, paired -n --null-draws 3 --
each as a --columns command, as a --groupings file of two lines, and with the other device stages on (--fit gpu --pvals gpu
--writer gpu, as far as the mode takes them).

With the two options every output file is byte-identical to the run without them (gzip's MTIME masked: significantLoci is written
by Python's gzip), except pairwiseMetrics_*.txt.gz, whose decompressed bytes are identical and which is valid BGZF with one
end-of-file block.  The null fits see every null distance (fewer than -z of them), so two host runs fit the same parameters."""
import gzip

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import roiAndVisualPairwise as rv
from tests import bgzf_ref
from tests.test_null_draws_host import _results, _state_info

pytestmark = pytest.mark.gpu

S, N, ROWS = 5, 12, (300, 150, 200)
A, B = "1-6", "7-12"
MODES = {"single": [], "paired": ["-m", "paired"], "paired-n": ["-m", "paired", "-n", "-t", "3"],
         "paired-n-draws": ["-m", "paired", "-n", "--null-draws", "3"]}
STAGES = {"single": ["--writer", "gpu"], "paired": ["--writer", "gpu"], "paired-n": ["--fit", "gpu", "--pvals", "gpu", "--writer", "gpu"],
          "paired-n-draws": ["--pvals", "gpu", "--writer", "gpu"]}


def invoke(args, out):
    from click.testing import CliRunner

    from epilogos_amd import run
    res = CliRunner().invoke(run.main, ["-l"] + args + ["-o", str(out), "-f", "t", "-w", "10"])
    assert res.exit_code == 0 and "ERROR" not in res.output and res.exception is None, res.output
    return res.output


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from epilogos_amd import engine, stateByLine as sbl
    engine.require_gpu()
    base = tmp_path_factory.mktemp("step4")
    d = base / "whole"
    d.mkdir()
    rng = np.random.default_rng(11)
    for k, r in enumerate(ROWS):
        x = np.where(rng.random((r, N)) < 0.5, S - 1, rng.integers(0, S, size=(r, N)))
        x[rng.random(r) < 0.15] = S - 1
        sbl.write_epgm(d / ("matrix_chr%d.epgm" % (k + 1)), x.astype(np.int8), "chr%d" % (k + 1), (1, S))
    meta = base / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    single = base / "single.tsv"
    single.write_text("first\t%s\nsecond\t1-3,9\n" % A)
    paired = base / "paired.tsv"
    paired.write_text("first\t%s\t%s\nsecond\t1-3\t4-12\n" % (A, B))
    return base, ["-i", str(d), "-j", str(meta)], {"single": single, "paired": paired}


def commands(inputs, mode, kind):
    _base, common, gfiles = inputs
    args = common + MODES[mode] + ([] if mode == "single" else ["--null-seed", "7"])
    if kind == "groupings":
        return args + ["--groupings", str(gfiles["single" if mode == "single" else "paired"])]
    args += ["--columns", A] if mode == "single" else ["--columns-a", A, "--columns-b", B]
    return args + (STAGES[mode] if kind == "stages" else [])


def new_options(mode):
    return ["--roi", "gpu"] + ([] if mode == "single" else ["--metrics", "gpu"])


def masked(path):
    b = bytearray(path.read_bytes())
    if path.name.endswith(".gz"):
        b[4:8] = b"\0\0\0\0"                                                    # gzip MTIME
    return bytes(b)


def same_but_metrics(host, gpu, mode):
    names = sorted(p.name for p in host.iterdir())
    assert names == sorted(p.name for p in gpu.iterdir()) and "regionsOfInterest_t.txt" in names
    assert not [n for n in names if n.startswith(".part_") or n.startswith("temp_")], names
    for n in names:
        if n.startswith("pairwiseMetrics_"):
            blob = (gpu / n).read_bytes()
            text = gzip.decompress(blob)
            assert text == gzip.decompress((host / n).read_bytes()) and text.count(b"\n") == sum(ROWS), n
            assert bgzf_ref.walk(blob) and blob.endswith(bgzf_ref.EOF) and blob.count(bgzf_ref.EOF) == 1
            assert len(text.split(b"\n")[0].split(b"\t")) == (8 if "-n" in MODES[mode] else 6)
        else:
            assert masked(host / n) == masked(gpu / n), n
    assert ("pairwiseMetrics_t.txt.gz" in names) == (mode != "single")
    return names


@pytest.mark.parametrize("kind", ["columns", "groupings", "stages"])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_file_is_the_host_run_s(inputs, mode, kind):
    base = inputs[0]
    args = commands(inputs, mode, kind)
    host, gpu = base / ("%s_%s_host" % (mode, kind)), base / ("%s_%s_gpu" % (mode, kind))
    invoke(args, host)
    out = invoke(args + new_options(mode), gpu)
    assert "WARNING" not in out, out
    if kind == "groupings":
        assert sorted(p.name for p in gpu.iterdir()) == ["first", "second"]
        for name in ("first", "second"):
            same_but_metrics(host / name, gpu / name, mode)
    else:
        names = same_but_metrics(host, gpu, mode)
        assert (mode == "paired-n" or mode == "paired-n-draws") == ("significantLoci_t.txt.gz" in names)
        assert (host / "regionsOfInterest_t.txt").stat().st_size > 0 or "-n" in MODES[mode]


@pytest.mark.parametrize("mode", ["single", "paired-n"])
def test_the_options_at_host_write_the_bytes_of_a_run_without_them(inputs, mode):
    base = inputs[0]
    args = commands(inputs, mode, "columns")
    plain = base / ("%s_columns_host" % mode)
    if not plain.exists():
        invoke(args, plain)
    named = base / ("%s_named_host" % mode)
    invoke(args + ["--roi", "host"] + ([] if mode == "single" else ["--metrics", "host"]), named)
    names = sorted(p.name for p in plain.iterdir())
    assert names == sorted(p.name for p in named.iterdir())
    assert all(masked(plain / n) == masked(named / n) for n in names)


def test_a_nan_p_value_takes_the_host_writer_with_one_warning(tmp_path, capsys):
    """In this process: a distance array with one NaN gives a NaN p-value; metrics="gpu" prints the one warning, the host writer writes
    the file, and the run is complete: the files of metrics="host"."""
    wrote = {}
    for where in ("host", "gpu"):
        res, _M = _results(np.random.default_rng(4), with_exceed=False)
        res["matrix_chr2"]["distances"][17] = np.nan
        out = tmp_path / where
        out.mkdir()
        np.save(out / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
        capsys.readouterr()
        rv.mainFromArrays(res, _state_info(tmp_path), out, "t", 1, True, 3, 200, out / "exp_freq_t.npy", 10, False, fit="gpu", seed=7,
                          **rv._metricsOptions(where))
        text = capsys.readouterr().out
        assert text.count("WARNING:") == text.count("WARNING: [--metrics gpu]") == (1 if where == "gpu" else 0), text
        wrote[where] = out
    names = sorted(p.name for p in wrote["host"].iterdir())
    assert names == sorted(p.name for p in wrote["gpu"].iterdir()) and {"pairwiseMetrics_t.txt.gz", "regionsOfInterest_t.txt", "significantLoci_t.txt.gz"} <= set(names)
    assert all(masked(wrote["host"] / n) == masked(wrote["gpu"] / n) for n in names)
    assert b"\tnan\t" in gzip.decompress((wrote["gpu"] / "pairwiseMetrics_t.txt.gz").read_bytes())
