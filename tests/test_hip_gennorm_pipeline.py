"""GPU: `epilogos -m paired -n --fit gpu` end to end.  Three files of 300, 150 and 200 bins, 12 biosample columns split 6 + 6,
-t 5 -z 200 --null-seed 7: more non-quiescent null distances than the sampling size, so the trials fit seeded sub-samples.

  * two runs write the same bytes in every file, p-values included (the host fit draws its sub-samples from OS entropy);
  * pairwiseDelta_* -- the files that hold no p-value -- and the first six columns of pairwiseMetrics are those of --fit host;
  * the p-value column is calculatePVals under the parameters _fitParams(fit="gpu", seed=7) returns for the same null distances;
  * a two-line --groupings file writes, for its first line, the same directory.

Every command is a child process (tests/test_hip_groups_pipeline.run_cli), started once per module."""
import gzip

import numpy as np
import pytest

from epilogos_amd import driver, helpers
from epilogos_amd import roiAndVisualPairwise as rv
from tests.test_hip_groupings_pipeline import _groupings_file, same_tree
from tests.test_hip_groups_pipeline import run_cli
from tests.test_host_logic import write_tsv

pytestmark = pytest.mark.gpu

ROWS, N, S = (300, 150, 200), 12, 18
A, B = "1-6", "7-12"
FIT = ["-n", "-t", "5", "-z", "200", "--null-seed", "7"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("gennorm")
    d = base / "whole"
    d.mkdir()
    rng = np.random.default_rng(11)
    for k, r in enumerate(ROWS):
        x = np.where(rng.random((r, N)) < 0.5, S - 1, rng.integers(0, S, size=(r, N)))
        x[rng.random(r) < 0.15] = S - 1                                     # quiescent bins: no null distance of theirs is fitted
        write_tsv(d / ("matrix_chr%d.txt.gz" % (k + 1)), x, chrom="chr%d" % (k + 1))
    meta = base / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    common = ["-m", "paired", "-i", str(d), "-j", str(meta)] + FIT
    cols = ["--columns-a", A, "--columns-b", B]
    out = {"gpu1": run_cli(common + cols + ["--fit", "gpu"], base / "gpu1"), "gpu2": run_cli(common + cols + ["--fit", "gpu"], base / "gpu2"),
           "host": run_cli(common + cols + ["--fit", "host"], base / "host"),
           "groupings": run_cli(common + ["--fit", "gpu", "--groupings", str(_groupings_file(base / "g.tsv", [("first", A, B), ("second", "1-3", "4-12")]))],
                                base / "groupings")}
    return d, meta, out


def _metrics(path):
    with gzip.open(path / "pairwiseMetrics_t.txt.gz", "rt") as fh:
        return [l.split("\t") for l in fh.read().splitlines()]


def test_two_runs_with_the_same_seed_write_the_same_bytes(runs):
    _d, _meta, out = runs
    names = same_tree(out["gpu1"], out["gpu2"])
    assert {"pairwiseMetrics_t.txt.gz", "significantLoci_t.txt.gz", "regionsOfInterest_t.txt"} <= set(names)
    assert sum(n.startswith("pairwiseDelta_t_") for n in names) == 3


def test_what_holds_no_p_value_is_the_host_runs(runs):
    _d, _meta, out = runs
    names = sorted(p.name for p in out["gpu1"].iterdir())
    assert names == sorted(p.name for p in out["host"].iterdir())
    for n in names:
        if n.startswith("pairwiseDelta_"):
            assert (out["gpu1"] / n).read_bytes() == (out["host"] / n).read_bytes(), n
    g, h = _metrics(out["gpu1"]), _metrics(out["host"])
    assert len(g) == len(h) == sum(ROWS) and [r[:6] for r in g] == [r[:6] for r in h] and all(len(r) == 8 for r in g)


def test_the_p_values_are_those_of_the_device_fits_parameters(runs, tmp_path):
    d, _meta, out = runs
    files = sorted(d.glob("*"))
    _exp, results = driver.run_paired_columns(files, helpers.parseColumns(A), helpers.parseColumns(B), S, 1, tmp_path, "t", S - 1, -1, 7, keep_temps=False)
    driver.finish_writes()
    order = ["matrix_chr1", "matrix_chr2", "matrix_chr3"]
    null = np.concatenate([results[k]["nullDistances"] for k in order])
    quies = np.concatenate([results[k]["quiescenceArr"] for k in order])
    dist = np.concatenate([results[k]["distances"] for k in order])
    assert int((~quies.astype(bool)).sum()) > 200                           # the trials fit sub-samples, not everything
    params = rv._fitParams(null, quies, 1, 5, 200, fit="gpu", seed=7)
    assert params == rv._fitParams(null, quies, 1, 5, 200, fit="gpu", seed=7) and params != rv._fitParams(null, quies, 1, 5, 200, fit="gpu", seed=8)
    assert all(np.isfinite(params)) and params[0] > 0 and params[2] > 0
    pvals = rv.calculatePVals(dist, params[0], params[-2], params[-1])
    rows = _metrics(out["gpu1"])
    assert [r[6] for r in rows] == ["%.5e" % p for p in pvals]
    assert [r[7] for r in rows] == ["%.5e" % p for p in rv.benjaminiHochberg(pvals)]


def test_a_groupings_file_fits_every_grouping_with_the_same_seed(runs):
    _d, _meta, out = runs
    assert sorted(p.name for p in out["groupings"].iterdir()) == ["first", "second"]
    same_tree(out["groupings"] / "first", out["gpu1"])
    assert len(_metrics(out["groupings"] / "second")) == sum(ROWS)
