"""GPU: `epilogos -m paired -n --pvals gpu` end to end, at the shapes of tests/test_hip_gennorm_pipeline.py (three files of 300, 150
and 200 bins, 12 biosample columns split 6 + 6, --null-seed 7).  Every command is a child process
(tests/test_hip_groups_pipeline.run_cli), started once per module.

  (i)   --null-draws 3: the p-values are the host's empirical ones and the device's Benjamini-Hochberg is bit-exact, so every file
        is byte-identical to the run without --pvals gpu;
  (ii)  --fit gpu (seeded, so that both runs fit the same parameters): pairwiseDelta_* byte-identical; pairwiseMetrics_* with the
        same fields 1-6 and p fields at most one unit of the last printed digit apart (the number of lines that differ at all is
        printed; at the bounds of tests/test_hip_pvals.py none is expected); significantLoci_* and regionsOfInterest_* with the same
        bins in the same order wherever the host's adjusted p is not within 1e-9 of the 0.1 threshold;
  (iii) the same pair of runs from one two-line --groupings file, both groupings;
  (iv)  in this process: a distance array with one NaN through mainFromArrays(pvals="gpu") prints the one warning and writes what
        pvals="host" writes."""
import gzip
from decimal import Decimal

import numpy as np
import pytest

from epilogos_amd import roiAndVisualPairwise as rv
from tests.test_hip_gennorm_pipeline import A, B, N, ROWS, S
from tests.test_hip_groupings_pipeline import _groupings_file, same_tree
from tests.test_hip_groups_pipeline import run_cli
from tests.test_host_logic import write_tsv
from tests.test_null_draws_host import _results, _state_info

pytestmark = pytest.mark.gpu

GROUPINGS = [("first", A, B), ("second", "1-3", "4-12")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("pvals")
    d = base / "whole"
    d.mkdir()
    rng = np.random.default_rng(11)
    for k, r in enumerate(ROWS):
        x = np.where(rng.random((r, N)) < 0.5, S - 1, rng.integers(0, S, size=(r, N)))
        x[rng.random(r) < 0.15] = S - 1
        write_tsv(d / ("matrix_chr%d.txt.gz" % (k + 1)), x, chrom="chr%d" % (k + 1))
    meta = base / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    common = ["-m", "paired", "-i", str(d), "-j", str(meta), "-n", "--null-seed", "7"]
    cols = ["--columns-a", A, "--columns-b", B]
    draws, fit = ["--null-draws", "3"], ["-t", "5", "-z", "200", "--fit", "gpu"]
    gfile = ["--groupings", str(_groupings_file(base / "g.tsv", GROUPINGS))]
    out = {}
    for name, args in (("draws", common + cols + draws), ("fit", common + cols + fit), ("groupings", common + fit + gfile)):
        out[name, "host"] = run_cli(args, base / (name + "_host"))
        out[name, "gpu"] = run_cli(args + ["--pvals", "gpu"], base / (name + "_gpu"))
    return out


def _lines(path):
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as fh:
        return [l.split("\t") for l in fh.read().splitlines()]


def _one_unit_apart(a, b):
    """Two %.5e strings: equal, or at most one unit of the last printed digit apart."""
    if a == b:
        return True
    da, db = Decimal(a), Decimal(b)
    return abs(da - db) <= Decimal(1).scaleb(max(da.adjusted(), db.adjusted()) - 5)


def compare_fitted(host, gpu):
    """(ii) on one output directory."""
    names = sorted(p.name for p in host.iterdir())
    assert names == sorted(p.name for p in gpu.iterdir())
    assert {"pairwiseMetrics_t.txt.gz", "significantLoci_t.txt.gz", "regionsOfInterest_t.txt"} <= set(names)
    for n in names:
        if n.startswith("pairwiseDelta_"):
            assert (host / n).read_bytes() == (gpu / n).read_bytes(), n
    h, g = _lines(host / "pairwiseMetrics_t.txt.gz"), _lines(gpu / "pairwiseMetrics_t.txt.gz")
    assert len(h) == len(g) == sum(ROWS) and [r[:6] for r in h] == [r[:6] for r in g] and all(len(r) == 8 for r in g)
    differ = sum(1 for a, b in zip(h, g) if a != b)
    print("%s: %d of %d pairwiseMetrics lines differ" % (gpu.name, differ, len(h)))
    for a, b in zip(h, g):
        assert _one_unit_apart(a[6], b[6]) and _one_unit_apart(a[7], b[7]), (a, b)
    # a printed adjusted p other than 1.00000e-01 is at least 5e-7 from the threshold
    near = {tuple(r[:3]) for r in h if r[7] == "1.00000e-01"}
    hl, gl = _lines(host / "significantLoci_t.txt.gz"), _lines(gpu / "significantLoci_t.txt.gz")
    keep = lambda rows: [r[:6] for r in rows if tuple(r[:3]) not in near]
    assert keep(hl) == keep(gl)
    hr, gr = _lines(host / "regionsOfInterest_t.txt"), _lines(gpu / "regionsOfInterest_t.txt")
    if not near:
        assert len(hl) == len(gl) and len(hr) == len(gr)
    k = min(len(hr), len(gr))
    assert [r[:6] for r in hr[:k]] == [r[:6] for r in gr[:k]]
    for a, b in zip(hl + hr[:k], gl + gr[:k]):
        if tuple(a[:3]) not in near:
            assert _one_unit_apart(a[6], b[6]) and _one_unit_apart(a[7], b[7]), (a, b)
    return differ


def test_empirical_p_values_every_file_is_byte_identical(runs):
    names = same_tree(runs["draws", "host"], runs["draws", "gpu"])
    assert {"pairwiseMetrics_t.txt.gz", "significantLoci_t.txt.gz", "regionsOfInterest_t.txt"} <= set(names)
    assert sum(n.startswith("pairwiseDelta_t_") for n in names) == 3
    assert all(len(r) == 8 for r in _lines(runs["draws", "gpu"] / "pairwiseMetrics_t.txt.gz"))


def test_fitted_p_values_agree_to_the_last_printed_digit(runs):
    compare_fitted(runs["fit", "host"], runs["fit", "gpu"])


def test_a_groupings_file_takes_the_option_for_every_grouping(runs):
    host, gpu = runs["groupings", "host"], runs["groupings", "gpu"]
    assert sorted(p.name for p in gpu.iterdir()) == sorted(p.name for p in host.iterdir()) == ["first", "second"]
    for name, _a, _b in GROUPINGS:
        compare_fitted(host / name, gpu / name)
    same_tree(gpu / "first", runs["fit", "gpu"])                            # its first line is the --columns-a/-b command


def test_a_nan_distance_falls_back_to_the_host_with_one_warning(tmp_path, capsys):
    from epilogos_amd import engine
    engine.require_gpu()
    wrote = {}
    for where in ("host", "gpu"):
        res, _M = _results(np.random.default_rng(4), with_exceed=False)
        res["matrix_chr2"]["distances"][17] = np.nan
        out = tmp_path / where
        out.mkdir()
        np.save(out / "exp_freq_t.npy", np.zeros(3, dtype=np.float32))
        capsys.readouterr()
        rv.mainFromArrays(res, _state_info(tmp_path), out, "t", 1, True, 3, 200, out / "exp_freq_t.npy", 10, False, fit="gpu", seed=7, pvals=where)
        text = capsys.readouterr().out
        assert text.count("WARNING:") == (1 if where == "gpu" else 0), text
        wrote[where] = out
    same_tree(wrote["host"], wrote["gpu"])
