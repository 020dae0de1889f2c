"""Similarity search on the GPU (epg_simsearch): distances, modes and indices equal to the numpy int64 restatement of
tests/simsearch_ref.py on edge shapes, the command line's -b / -q outputs equal to tests/golden/simsearch.npz, and one
whole-genome-size case."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import simsearch_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests" / "golden" / "simsearch.npz")


def _run(G, Q, rs, n, **kw):
    from epilogos_amd import similaritySearch_calc as calc
    return calc.simsearch(G, Q, rs, n, want_dist=True, **kw)


def _check(G, Q, rs, n, **kw):
    idx, mode, dist = _run(G, Q, rs, n, **kw)
    for r in range(len(Q)):
        D = ref.distances(G, Q[r])
        assert np.array_equal(dist[r], D), "distances of ROI %d" % r
        want, m = ref.pick(D, rs[r], Q.shape[1], n)
        assert mode[r] == m, "mode of ROI %d" % r
        assert np.array_equal(idx[r], want), "indices of ROI %d" % r
    return idx, mode


def _genome(rng, Pg, S, classes=6, planted=4, W=25, amp=200000, bg=0.9):
    """Rows of a few repeated classes, class 0 (the background) with probability bg, and noisy copies of one random window."""
    base = rng.integers(0, amp, size=(classes, S))
    G = base[np.where(rng.random(Pg) < bg, 0, rng.integers(0, classes, size=Pg))]
    src = rng.integers(0, amp, size=(W, S))
    for _ in range(planted):
        if Pg > W:
            a = int(rng.integers(0, Pg - W))
            G[a:a + W] = src + rng.integers(-50, 50, size=src.shape)
    return G.astype(np.int64), src


def _rois(rng, G, R, W):
    rs = rng.integers(0, G.shape[0] - W + 1, size=R)
    return np.stack([G[s:s + W] for s in rs]), rs


@pytest.mark.parametrize("S", [15, 18, 25, 100, 150])
def test_states(S):
    rng = np.random.default_rng(S)
    G, _ = _genome(rng, 700, S)
    Q, rs = _rois(rng, G, 6, 25)
    _check(G, Q, rs, 100)


@pytest.mark.parametrize("P", [1, 25, 127, 128, 129, 257])
def test_positions(P):
    rng = np.random.default_rng(P)
    G, _ = _genome(rng, P + 24, 18)
    Q, rs = _rois(rng, G, 5, 25)
    _check(G, Q, rs, 7)


def test_one_roi_and_batch_edges():
    rng = np.random.default_rng(7)
    G, _ = _genome(rng, 900, 18)
    Q, rs = _rois(rng, G, 9, 25)
    _check(G, Q[:1], rs[:1], 100)
    a = _check(G, Q, rs, 100, batch=4)          # batches of 4, 4, 1 (a batch size + 1 ROIs in the last two)
    b = _check(G, Q, rs, 100, batch=9)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_candidates_run_out_leave_zeros():
    # every window at the same distance: the mode is that distance and the first candidate outside the ROI stops the row (-1)
    G = np.zeros((80, 18), dtype=np.int64)
    idx, mode = _check(G, np.ones((1, 25, 18), dtype=np.int64), [0], 10)
    assert (idx == -1).all() and mode[0] == 25 * 18
    # every window equal to the ROI: mode 0, every non-overlapping window is a match; the picks run out, the rest stays 0
    G = np.full((120, 15), 7, dtype=np.int64)
    idx, mode = _check(G, np.full((1, 25, 15), 7, dtype=np.int64), [50], 100)
    assert mode[0] == 0 and list(idx[0, :4]) == [0, 25, 75, 0] and (idx[0, 3:] == 0).all()


def test_all_distances_distinct_no_matches():
    rng = np.random.default_rng(11)
    G = rng.integers(0, 10 ** 6, size=(400, 18)).astype(np.int64)
    Q = np.stack([G[100:125]])
    idx, mode = _check(G, Q, [100], 100)
    assert mode[0] == 0 and (idx == -1).all()          # the mode is the minimum: the ROI's own window


def test_many_identical_windows():
    G = np.tile(np.arange(18, dtype=np.int64) * 1000, (600, 1))
    G[300:325] += 5000
    Q = np.stack([G[300:325]])
    Q2 = np.stack([G[10:35]])
    _check(G, np.concatenate([Q, Q2]), [300, 10], 100)


@pytest.mark.parametrize("case", ["s200", "s20"])
def test_cli_build_and_query_match_golden(tmp_path, case):
    sp = tmp_path / "scores.txt"
    sp.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "epilogos_amd.similaritySearch_run", "-b", "-s", str(sp), "-o", str(out),
           "-w", str(int(GOLD[case + "_windowBP"])), "-j", "3", "--calc-mem", "1"]
    subprocess.run(cmd, cwd=ROOT, check=True, capture_output=True, text=True, timeout=600)
    assert sorted(p.name for p in out.iterdir()) == ["reduced_genome.npy", "simsearch.bed.gz", "simsearch.bed.gz.tbi",
                                                     "simsearch_cube.npz", "simsearch_indices.npy"]
    import gzip
    assert gzip.decompress((out / "simsearch.bed.gz").read_bytes()) == GOLD[case + "_bed_text"].tobytes()
    got = np.load(out / "simsearch_indices.npy")
    want = GOLD[case + "_indices"]
    keep = np.setdiff1d(np.arange(len(want)), GOLD[case + "_skip"])
    assert got.dtype == np.int32 and np.array_equal(got[keep], want[keep])
    assert np.array_equal(np.load(out / "reduced_genome.npy"), GOLD[case + "_reduced_genome"])
    c, s, e = GOLD[case + "_bed_text"].tobytes().decode().splitlines()[0].split("\t")[:3]
    q = tmp_path / "q"
    subprocess.run([sys.executable, "-m", "epilogos_amd.similaritySearch_run", "-q", "%s:%s-%s" % (c, s, e), "-m",
                    str(out / "simsearch.bed.gz"), "-o", str(q)], cwd=ROOT, check=True, capture_output=True, timeout=300)
    assert (q / ("similarity_search_region_%s_%s_%s_recs.bed" % (c, s, e))).exists()


def test_golden_indices_through_the_kernel():
    """STEP 2 alone on the golden cube: indices and modes as the reference (rows it lists as disagreeing excepted)."""
    for case in ("s200", "s20"):
        G = np.rint(GOLD[case + "_reduced_genome"] * 1e5).astype(np.int64)
        Q = np.rint(GOLD[case + "_cube_scores"] * 1e5).astype(np.int64)
        idx, mode, _ = _run(G, Q, GOLD[case + "_self_start"], 100)
        keep = np.setdiff1d(np.arange(len(Q)), GOLD[case + "_skip"])
        assert np.array_equal(idx[keep], GOLD[case + "_indices"][keep])
        assert np.array_equal(mode, GOLD[case + "_modes"])


def test_whole_genome_size():
    """3 M reduced positions, 8 ROIs against the restatement; every ROI run twice, byte-identical."""
    rng = np.random.default_rng(2026)
    Pg, S, W = 3_000_024, 18, 25
    G, src = _genome(rng, Pg, S, classes=40, planted=300, amp=100000, bg=0.97)
    Q = np.stack([src] + [G[s:s + W] for s in rng.integers(0, Pg - W, size=7)])
    rs = np.array([0] + list(rng.integers(0, Pg - W, size=7)))
    idx1, mode1 = _check(G, Q, rs, 100)
    from epilogos_amd import similaritySearch_calc as calc
    idx2, mode2 = calc.simsearch(G, Q, rs, 100, batch=3)
    assert idx1.tobytes() == idx2.tobytes() and mode1.tobytes() == mode2.tobytes()
    assert (idx1[0] > 0).sum() >= 50                 # the planted copies are found


def test_chr1_sampled_rows_through_the_kernel():
    """STEP 2 on the chr1 example's cube: the sampled rows equal the exact restatement (distances, modes, indices) and the
    reference's indices except on the rows the golden lists with their reason."""
    from epilogos_amd import similaritySearch_calc as calc
    from epilogos_amd import similaritySearch_max_mean as mm
    import tempfile
    sp_dir = Path(tempfile.mkdtemp())
    sp = ref.chr1_scores_file(sp_dir / "scores_chr1.txt.gz")
    mm.main(sp_dir, sp, 125, 5, 25000, -1, -1)
    G = mm.to_grid(np.load(sp_dir / "reduced_genome.npy"))
    cube = np.load(sp_dir / "simsearch_cube.npz", allow_pickle=True)
    rows = GOLD["chr1_rows"]
    Q = mm.to_grid(cube["scores"][rows])
    rs = GOLD["chr1_self_start"]
    idx, mode = _check(G, Q, rs, 100)
    assert np.array_equal(mode, GOLD["chr1_modes"])
    keep = np.setdiff1d(np.arange(len(rows)), GOLD["chr1_skip"])
    assert np.array_equal(idx[keep], GOLD["chr1_indices"][keep])
    assert not np.array_equal(idx, GOLD["chr1_indices"]) or len(GOLD["chr1_skip"]) == 0


def test_chr1_cli_build(tmp_path):
    """-b end to end on chr1: the output set, and the sampled rows' indices as the reference's (listed rows excepted)."""
    import hashlib
    sp = ref.chr1_scores_file(tmp_path / "scores_chr1.txt.gz")
    out = tmp_path / "out"
    subprocess.run([sys.executable, "-m", "epilogos_amd.similaritySearch_run", "-b", "-s", str(sp), "-o", str(out)], cwd=ROOT,
                   check=True, capture_output=True, text=True, timeout=1200)
    assert sorted(p.name for p in out.iterdir()) == ["reduced_genome.npy", "simsearch.bed.gz", "simsearch.bed.gz.tbi",
                                                     "simsearch_cube.npz", "simsearch_indices.npy"]
    cube = np.load(out / "simsearch_cube.npz", allow_pickle=True)
    assert hashlib.sha256(np.ascontiguousarray(cube["scores"])).digest() == GOLD["chr1_cube_sha256"].tobytes()
    got = np.load(out / "simsearch_indices.npy")[GOLD["chr1_rows"]]
    keep = np.setdiff1d(np.arange(len(got)), GOLD["chr1_skip"])
    assert np.array_equal(got[keep], GOLD["chr1_indices"][keep])
    import gzip
    lines = gzip.decompress((out / "simsearch.bed.gz").read_bytes()).decode().splitlines()
    assert len(lines) == int(GOLD["chr1_n_regions"])
