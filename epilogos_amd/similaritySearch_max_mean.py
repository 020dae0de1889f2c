"""Similarity search STEP 1 -- salient region selection and block reduction.  Same signature and output files as the reference's
epilogos/similaritySearch_max_mean.py (main :9-49, readScores :52-77, makeSlice :80-102, removeRegions :105-136, reduceGenome
:139-160): genome_stats.npz, simsearch_cube.npz and reduced_genome.npy.

Scores are kept as exact integers, the "%.5f" values of the scores file times 1e5 (readScores refuses values off that grid).
The row sums that pick the retained bin of a block are exact integer sums; ties go to the lower bin, in makeSlice (the
reference's idxmax does the same) and in reduceGenome (the reference's sort_values + drop_duplicates(keep='last') breaks them by
the platform's unstable quicksort: tied bins whose rows differ are the only place the two can disagree)."""
import sys
from pathlib import Path
from time import time

import numpy as np
import pandas as pd

from . import roiSingle

SCALE = 100000


def to_grid(values, what="scores"):
    """float64 values of a "%.5f" text -> int64 values x 1e5; refuses values that are not on the 1e-5 grid."""
    v = np.asarray(values, dtype=np.float64)
    k = np.rint(v * SCALE)
    bad = k / SCALE != v
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), v.shape)
        raise ValueError("%s: value %r at %s is not on the 1e-5 grid of a \"%%.5f\" scores file; similarity search works on "
                         "exact integers and refuses it" % (what, float(v[i]), tuple(int(x) for x in i)))
    if np.abs(k).max(initial=0) >= 2 ** 31:
        raise ValueError("%s: |value| of 21474.83648 or more does not fit the int32 grid" % what)
    return k.astype(np.int64)


def readScores(scoresPath):
    """(reference :52-77) -> (stateScores float64 [G, S], inputArr object [G, 4]: chromosome, start, end, row sum,
    scaled int64 [G, S])."""
    scores = pd.read_table(scoresPath, sep="\t", header=None)
    inputDF = scores.iloc[:, :3].copy()
    inputDF[3] = scores.iloc[:, 3:].sum(axis=1)           # the reference's float row sums: maxMean ranks by them
    inputDF.columns = ["Chromosome", "Start", "End", "Score"]
    stateScores = scores.iloc[:, 3:].to_numpy(dtype=np.float64)
    return stateScores, inputDF.to_numpy(), to_grid(stateScores, str(scoresPath))


def _window(idx, windowBins):
    return (idx - windowBins // 2, idx + windowBins // 2 + 1) if windowBins % 2 else (idx - windowBins // 2, idx + windowBins // 2)


def _block_argmax(rowsums, blockSize):
    """Index of the largest row sum of each block of blockSize rows (a partial last block included), the first on ties."""
    n = len(rowsums)
    nb = -(-n // blockSize)
    pad = np.full(nb * blockSize, np.iinfo(np.int64).min, dtype=np.int64)
    pad[:n] = rowsums
    return np.argmax(pad.reshape(nb, blockSize), axis=1) + np.arange(nb) * blockSize


def makeSlice(genome, idx, windowBins, blockSize):
    """(reference :80-102) The reduced window around centre bin idx: per block, the row with the largest sum.  genome: int64
    [G, S] (scaled scores)."""
    a, b = _window(int(idx), windowBins)
    a = max(a, 0)
    w = genome[a:b]
    return w[_block_argmax(w.sum(axis=1), blockSize)]


def removeRegions(roiCoords, roiCube, filterState, filterScore):
    """(reference :105-136) roiCoords: object [R, 3]; roiCube: int64 [R, 25, S] scaled.  filterScore is in score units."""
    dropped = list(np.where(roiCoords[:, 1].astype(np.int64) >= roiCoords[:, 2].astype(np.int64))[0])
    if filterState != 0:
        fs = roiCube.shape[2] - 1 if filterState == -1 else filterState - 1
        dropped += list(np.where(np.argmax(np.max(roiCube, axis=1), axis=1) == fs)[0])
    if filterScore != -1:
        dropped += list(np.where(np.max(roiCube, axis=(1, 2)) / SCALE < filterScore)[0])
    keep = np.setdiff1d(np.arange(len(roiCoords)), np.array(dropped, dtype=np.int64))
    return roiCoords[keep], roiCube[keep]


def reduceGenomeIndices(genome, blockSize):
    """Bins kept by the genome reduction (reference :139-160): the largest row sum of each block, the lower bin on ties."""
    return _block_argmax(genome.sum(axis=1), blockSize)


def reduceGenome(outputDir, genome, blockSize):
    """reduced_genome.npy: float64 [ceil(G / blockSize), S], as the reference stores it."""
    np.save(Path(outputDir) / "reduced_genome.npy", genome[reduceGenomeIndices(genome, blockSize)] / SCALE, allow_pickle=True)


def selectRegions(inputArr, genome, windowBins, blockSize, filterState, filterScore):
    """maxMean with maxRegions = G // windowBins, makeSlice and removeRegions -> (roiCoords object [R, 3], roiCube int64)."""
    maxRegions = int(genome.shape[0] // windowBins)
    chrom, start, end, _score, orig = roiSingle.maxMean(inputArr[:, 0], inputArr[:, 1], inputArr[:, 2],
                                                        inputArr[:, 3].astype(np.float64), windowBins, maxRegions)
    S = genome.shape[1]
    nblk = windowBins // blockSize
    roiCoords = np.empty((len(orig), 3), dtype=object)
    if len(orig):
        roiCoords[:, 0], roiCoords[:, 1], roiCoords[:, 2] = chrom, start, end
    roiCube = (np.stack([makeSlice(genome, i, windowBins, blockSize) for i in orig]) if len(orig)
               else np.zeros((0, nblk, S), dtype=np.int64))
    return removeRegions(roiCoords, roiCube, filterState, filterScore)


def main(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore):
    outputDir = Path(outputDir)
    print("Reading in data...", flush=True); t = time()
    stateScores, inputArr, genome = readScores(scoresPath)
    np.savez_compressed(outputDir / "genome_stats", scores=stateScores, coords=inputArr[:, :3])
    print("    Time:", format(time() - t, '.0f'), "seconds\n", flush=True)
    print("Finding regions of size {}kb...".format(windowBP // 1000), flush=True); t1 = time()
    roiCoords, roiCube = selectRegions(inputArr, genome, windowBins, blockSize, filterState, filterScore)
    np.savez_compressed(file=outputDir / "simsearch_cube", scores=roiCube / SCALE, coords=roiCoords)
    print("    Time:", format(time() - t1, '.0f'), "seconds\n", flush=True)
    print("Reducing genome scores by factor of {}...".format(blockSize), flush=True); t2 = time()
    reduceGenome(outputDir, genome, blockSize)
    print("    Time:", format(time() - t2, '.0f'), "seconds\n", flush=True)
    print("Total time:", format(time() - t, '.0f'), "seconds\n", flush=True)


if __name__ == "__main__":
    main(Path(sys.argv[1]), Path(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]),
         float(sys.argv[7]))
