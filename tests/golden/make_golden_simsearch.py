#!/usr/bin/env python3
"""Golden vectors of the similarity search (tests/golden/simsearch.npz) from the REAL reference (similaritySearch_max_mean.py,
similaritySearch_calc.py, similaritySearch_write.py) run in-process on two synthetic scores files.  Runs only in the build
container, where the reference is mounted; the tests read the npz.

natsort / pyranges are stubbed as in make_golden.py; pysam.tabix_compress is stubbed to capture the bed text before compression
(pysam is not installed) and tabix_index to a no-op.  The generator checks that the exact-integer restatement of
tests/simsearch_ref.py reproduces the reference's indices on every stored row; rows where the reference's float rounding or
unstable tie order disagree are listed in `<case>_skip` with the reason (none on these inputs).

    python tests/golden/make_golden_simsearch.py

Cases (prefix of every key):
  s200  three chromosomes (chr1, chr2, chr10) of 200-bp bins, 18 states: background bins, random salient segments and noisy
        copies of one segment planted elsewhere; -w 25000 (125 bins, block size 5).
  s20   one chromosome of 20-bp bins, 15 states, -w 500 (25 bins, block size 1).
  chr1  the S1 scores of the chr1 example (rebuilt from chr1_full.npz, pinned by its text_sha256), -w 25000: STEP 1 pinned by
        the cube coordinates and SHA-256 digests of the cube and reduced genome, STEP 2 on 64 evenly spaced regions
        (run_chr1).
Keys per case: scores_txt (the input file's text, uint8), windowBP, cube_coords, cube_scores, reduced_genome, indices, modes,
self_start, bed_text (uint8), skip (int64 rows excluded from the index comparison) + skip_reason.  Global: click_options."""
import io
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

REF = "/root/reference"
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))


def import_reference():
    for m in ("natsort", "pyranges"):
        sys.modules[m] = types.ModuleType(m)
    captured = {}
    pysam = types.ModuleType("pysam")

    def tabix_compress(src, dst, force=False):
        captured["text"] = Path(src).read_bytes()
        Path(dst).write_bytes(b"stub")

    def tabix_index(fn, force=False, zerobased=False, preset=None):
        Path(str(fn) + ".tbi").write_bytes(b"stub")

    pysam.tabix_compress, pysam.tabix_index = tabix_compress, tabix_index
    sys.modules["pysam"] = pysam
    sys.path.insert(0, REF)
    import epilogos.similaritySearch_calc as calc
    import epilogos.similaritySearch_max_mean as mm
    import epilogos.similaritySearch_run as run
    import epilogos.similaritySearch_write as wr
    return mm, calc, wr, run, captured


def synth_scores(rng, chroms, binSize, S, n_salient, seg_len, n_copies):
    """Score text: background bins (one constant row: the windows of the background are one distance class, the mode), salient
    segments of larger random values, and noisy copies of segment 0 planted elsewhere (the matches)."""
    G = sum(n for _c, n in chroms)
    x = np.zeros((G, S))
    x[:, -1] = 0.01234
    segs = []
    for _ in range(n_salient):
        a = int(rng.integers(0, G - seg_len))
        x[a:a + seg_len] = np.round(rng.gamma(2.0, 0.4, size=(seg_len, S)) * (rng.random(S) < 0.4), 5)
        segs.append(a)
    src = x[segs[0]:segs[0] + seg_len].copy()
    for _ in range(n_copies):
        a = int(rng.integers(0, G - seg_len))
        x[a:a + seg_len] = np.round(np.maximum(src + rng.normal(0, 0.02, size=src.shape), 0), 5)
    lines, i = [], 0
    for c, n in chroms:
        for b in range(n):
            lines.append("%s\t%d\t%d\t%s\n" % (c, b * binSize, (b + 1) * binSize, "\t".join("%.5f" % v for v in x[i])))
            i += 1
    return "".join(lines)


def run_case(mods, text, windowBP, binSize, nDesiredMatches=100):
    mm, calc, wr, run, captured = mods
    from tests import simsearch_ref as ref
    blockSize = run.determineBlockSize200(windowBP) if binSize == 200 else run.determineBlockSize20(windowBP)
    windowBins = int(windowBP / binSize)
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        sp = d / "scores.txt"
        sp.write_text(text)
        mm.main(d, sp, windowBins, blockSize, windowBP, -1, -1)
        cube = np.load(d / "simsearch_cube.npz", allow_pickle=True)
        reduced = np.load(d / "reduced_genome.npy", allow_pickle=True)
        coords = np.load(d / "genome_stats.npz", allow_pickle=True)["coords"]
        calc.main(d, windowBins, blockSize, 1, nDesiredMatches, 1, 0)
        captured.clear()
        wr.main(d, windowBins, blockSize, 1, nDesiredMatches)
        indices = np.load(d / "simsearch_indices.npy", allow_pickle=True)
        assert not (d / "genome_stats.npz").exists()
    # the exact-integer restatement on every row
    G = np.rint(reduced * 1e5).astype(np.int64)
    Q = np.rint(cube["scores"] * 1e5).astype(np.int64)
    first = {}
    for i, (c, s) in enumerate(zip(coords[:, 0], coords[:, 1])):
        first.setdefault((c, int(s)), i)
    rs = np.array([first[(c, int(s))] // blockSize for c, s in cube["coords"][:, :2]], dtype=np.int64)
    mine, modes = ref.search(G, Q, rs, nDesiredMatches)
    skip = [r for r in range(len(Q)) if not np.array_equal(mine[r], indices[r])]
    print("windowBP %d: %d regions, %d reduced positions, %d rows differ from the restatement" % (
        windowBP, len(Q), len(G), len(skip)), flush=True)
    return dict(scores_txt=np.frombuffer(text.encode(), dtype=np.uint8), windowBP=np.int64(windowBP),
                cube_coords=cube["coords"].astype(str), cube_coord_ints=cube["coords"][:, 1:].astype(np.int64),
                cube_scores=cube["scores"], reduced_genome=reduced, indices=indices, modes=modes, self_start=rs,
                bed_text=np.frombuffer(captured["text"], dtype=np.uint8), skip=np.array(skip, dtype=np.int64),
                skip_reason=np.array(["float rounding or unstable tie order of the reference"] * len(skip), dtype=str))


def chr1_text(tmpdir):
    """The reference's S1 scores file of the chr1 example, rebuilt from chr1_full.npz (oracle + native writer) and pinned by its
    text_sha256, as tests/test_chr1_full.py does."""
    import gzip
    import hashlib
    from epilogos_amd import _io
    from oracle import oracle_np as onp
    g = np.load(HERE / "chr1_full.npz")
    x = g["x"]
    R = x.shape[0]
    s32 = onp.score_s1(x, onp.normalise(onp.expected_s1(x, 18)), 18).astype(np.float32)
    start = int(g["start0"]) + 200 * np.arange(R, dtype=np.int64)
    blob = "".join("chr1\t%d\t%d\n" % (s, s + 200) for s in start).encode()
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum([len(l) + 1 for l in blob.decode().split("\n")[:-1]], out=off[1:])
    path = Path(tmpdir) / "scores_chr1.txt.gz"
    _io.write_scores(path, _io.Locations(np.frombuffer(blob, dtype=np.uint8).copy(), off), s32)
    with gzip.open(path, "rb") as fh:
        text = fh.read()
    assert hashlib.sha256(text).digest() == g["text_sha256"].tobytes()
    return path


def run_chr1(mods, n_sample=64, nDesiredMatches=100):
    """chr1 S1 (1 246 253 bins, -w 25000): the reference's STEP 1 in full, its STEP 2 on a fixed sample of rows (every
    len // n_sample-th region of the cube).  Stored: cube coordinates (starts, ends), SHA-256 of the cube scores and of the
    reduced genome, the sampled rows' indices, modes (exact), self starts, and the rows where the restatement disagrees."""
    import hashlib
    import pandas as pd
    mm, calc, wr, run, captured = mods
    from tests import simsearch_ref as ref
    windowBP, windowBins, blockSize = 25000, 125, 5
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        sp = chr1_text(d)
        mm.main(d, sp, windowBins, blockSize, windowBP, -1, -1)
        cube = np.load(d / "simsearch_cube.npz", allow_pickle=True)
        reduced = np.load(d / "reduced_genome.npy", allow_pickle=True)
        coords = np.load(d / "genome_stats.npz", allow_pickle=True)["coords"]
    roiCube, roiCoords = cube["scores"], cube["coords"]
    rows = np.unique(np.linspace(0, len(roiCube) - 1, n_sample).astype(np.int64))
    genomeCoords = pd.DataFrame(coords, columns=["Chromosome", "Start", "End"])
    arr = np.zeros((len(rows), nDesiredMatches), dtype=np.int32)
    calc._initEuclideanDistance(genomeCoords, reduced, pd.DataFrame(roiCoords[rows], columns=["Chromosome", "Start", "End"]),
                                roiCube[rows], arr, windowBins, blockSize, nDesiredMatches)
    calc.runEuclideanDistance((0, len(rows)))
    G = np.rint(reduced * 1e5).astype(np.int64)
    Q = np.rint(roiCube[rows] * 1e5).astype(np.int64)
    rs = (roiCoords[rows, 1].astype(np.int64) - int(coords[0, 1])) // 200 // blockSize
    mine, modes = ref.search(G, Q, rs, nDesiredMatches)
    skip = [i for i in range(len(rows)) if not np.array_equal(mine[i], arr[i])]
    reasons = [_chr1_reason(reduced, roiCube[rows[i]], G, Q[i]) for i in skip]
    for i, why in zip(skip, reasons):
        print("  sampled row %d (cube row %d): %s" % (i, rows[i], why), flush=True)
    print("chr1: %d regions (%d sampled), %d reduced positions, %d sampled rows differ from the restatement; picks per row %s" % (
        len(roiCube), len(rows), len(G), len(skip), sorted(set((arr >= 0).sum(axis=1).tolist()))), flush=True)
    return dict(windowBP=np.int64(windowBP), n_regions=np.int64(len(roiCube)),
                cube_starts=roiCoords[:, 1].astype(np.int64), cube_ends=roiCoords[:, 2].astype(np.int64),
                cube_sha256=np.frombuffer(hashlib.sha256(np.ascontiguousarray(roiCube)).digest(), dtype=np.uint8),
                reduced_shape=np.array(reduced.shape, dtype=np.int64),
                reduced_sha256=np.frombuffer(hashlib.sha256(np.ascontiguousarray(reduced)).digest(), dtype=np.uint8),
                rows=rows, indices=arr, modes=modes, self_start=rs, skip=np.array(skip, dtype=np.int64),
                skip_reason=np.array(reasons, dtype=str))


def _chr1_reason(reduced, cube_row, G, q):
    """Why the reference's row differs from the exact one: its float distances (sklearn's dot-product identity, :88-91) put
    other windows in the modal class than the exact distances do, or order near-equal distances differently."""
    import scipy.stats as st
    from sklearn.metrics.pairwise import euclidean_distances
    from tests import simsearch_ref as ref
    W = len(cube_row)
    P = len(reduced) - W + 1
    d0 = np.add(*np.broadcast_arrays(np.arange(W), np.arange(P).reshape(P, 1)))
    d1 = np.broadcast_to(np.arange(W), (P, W))
    Df = np.sum(euclidean_distances(reduced, cube_row, squared=True)[d0, d1], axis=1)
    D = ref.distances(G, q)
    fm, m = st.mode(Df, keepdims=False)[0], ref.mode(D)
    if not np.array_equal(Df == fm, D == m):
        return ("float rounding of the reference's distances changes the modal class (%d windows at its float mode, %d at the "
                "exact mode): halfMode moves" % (int((Df == fm).sum()), int((D == m).sum())))
    return "float rounding of the reference's distances reorders near-equal distances"


def main():
    mods = import_reference()
    run = mods[3]
    out = {"click_options": np.array(sorted(o for p in run.main.params for o in p.opts), dtype=str)}
    rng = np.random.default_rng(20261015)
    t200 = synth_scores(rng, [("chr1", 2400), ("chr2", 1500), ("chr10", 900)], 200, 18, 10, 125, 6)
    for k, v in run_case(mods, t200, 25000, 200).items():
        out["s200_" + k] = v
    t20 = synth_scores(rng, [("chr3", 3000)], 20, 15, 8, 25, 8)
    for k, v in run_case(mods, t20, 500, 20).items():
        out["s20_" + k] = v
    for k, v in run_chr1(mods).items():
        out["chr1_" + k] = v
    buf = io.BytesIO()
    np.savez_compressed(buf, **out)
    (HERE / "simsearch.npz").write_bytes(buf.getvalue())
    print("wrote", HERE / "simsearch.npz", len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
