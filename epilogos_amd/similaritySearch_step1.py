"""Similarity search STEP 1 on the GPU (`similaritySearch_run -b --step1 gpu`): the signature, progress lines and output files of
similaritySearch_max_mean.main -- genome_stats.npz, simsearch_cube.npz, reduced_genome.npy, the same arrays -- with the scores file
parsed on the device (scoresText.read_scores_device), the windows ranked and picked there (include/epilogos_simsearch_pick.h), their
slices cut there (epg_simsearch_slices) and the genome reduced there (epg_simsearch_reduce).

What stays on the host, and why:
  - the rolling MEAN: pandas' Series.rolling(W, center=True).mean() is an online compensated sum whose last bits depend on the whole
    history, and those bits break ties between windows that share their maximum (roiSingle.maxMean).  The score vector is downloaded,
    that one pandas call runs, the result is uploaded.
  - the final best-first order of the picked windows (a lexsort of a few thousand rows), removeRegions, and the three file writes;
    genome_stats.npz is written on a host thread while the device works.

The centre score of a bin is pandas' float64 row sum of the "%.5f" values; epg_simsearch_rowscore computes the same bits from the
int32 grid (correctly rounded k / 1e5, added left to right).  The keys must be these floats, not the exact integer sums: rows with
equal integer sums mostly have different float sums.

A file the strict reader refuses (scoresText.NotStrict) gets the warning line similaritySearch_query.readGrid prints and is built by
similaritySearch_max_mean.main.  Without a GPU or the library the module raises, as the engine does.

The device steps are module-level functions (readDevice, rowScores, rollingMax, rankWindows, pickWindows, slices, reduce, deviceOf): a host
test puts numpy restatements in their place, on CPU tensors.  `python -m epilogos_amd.similaritySearch_step1 outputDir scoresPath
windowBins blockSize windowBP filterState filterScore` is the child of a `--gpus N` build: one fresh process on LOCAL_RANK."""
import os
import sys
import threading
from pathlib import Path
from time import perf_counter, time

import numpy as np
import pandas as pd

from . import similaritySearch_max_mean as mm

SLICE_BATCH = 256


# ---- the device steps ----------------------------------------------------------------------------------------------------------

def readDevice(scoresPath, timings=None, inflate="host"):
    """-> (x int32 [G, S] device tensor, start int64 [G], end int64 [G] host arrays, runs [(chromosome, row0, row1)]); raises
    scoresText.NotStrict.  inflate "gpu" (--inflate gpu): a BGZF file is inflated on the device too."""
    from . import engine, scoresText
    engine.require_gpu()
    return scoresText.read_scores_device(scoresPath, timings=timings, **({"inflate": inflate} if inflate != "host" else {}))


def rowScores(x):
    """x int32 [G, S] -> float64 [G], pandas' row sums of the scores (epg_simsearch_rowscore)."""
    from . import engine
    return engine.simsearch_rowscore(x)


def rollingMax(v, W):
    """float64 [n] -> float64 [n], _io.rolling_max(v, W): NaN where the centred window is incomplete."""
    from . import engine
    return engine.simsearch_rolling_max(v.contiguous(), W)


def rankWindows(rmax, rmean, score):
    """-> int32 [n] (the bits of the library's uint32): the position of each window in np.lexsort((-score, -rmean, -rmax))."""
    from . import engine
    return engine.simsearch_rank(rmax.contiguous(), rmean.contiguous(), score.contiguous())


def pickWindows(rank, W, maxRegions):
    """-> (picked positions int64, ascending, host array; sweeps over the tiles)."""
    from . import engine
    picked, count, launches = engine.simsearch_pick(rank, W, maxRegions)
    return picked[:int(count.cpu()[0])].cpu().numpy(), launches


def slices(x, first, nblk, blockSize):
    """The block-reduced windows that start at rows `first`: int64 [B, nblk, S] host array (epg_simsearch_slices, SLICE_BATCH
    windows a call)."""
    from . import engine
    first = np.ascontiguousarray(first, dtype=np.int64)
    out = np.empty((len(first), int(nblk), x.shape[1]), dtype=np.int64)
    for b0 in range(0, len(first), SLICE_BATCH):
        f = first[b0:b0 + SLICE_BATCH]
        out[b0:b0 + len(f)] = engine.simsearch_slices(x, f, nblk, blockSize).cpu().numpy()
    return out


def reduce(x, blockSize):
    """The block-reduced genome: int64 [ceil(G / blockSize), S] host array (epg_simsearch_reduce)."""
    from . import engine
    return engine.simsearch_reduce(x, blockSize).cpu().numpy().astype(np.int64)


def deviceOf():
    """The device STEP 4's region search uploads its three vectors to (roiSingle.maxMeanDevice); raises without a GPU or the library."""
    import torch
    from . import engine
    engine.require_gpu()
    return torch.device("cuda", torch.cuda.current_device())


# ---- plumbing ------------------------------------------------------------------------------------------------------------------

def rollingMean(sc, W, timings=None):
    """pandas' centred rolling mean of a device vector, back on its device (see the module text: not reproducible in parallel)."""
    import torch
    t = perf_counter()
    host = sc.cpu().numpy()
    t1 = perf_counter()
    mean = pd.Series(host).rolling(int(W), center=True).mean().to_numpy()
    t2 = perf_counter()
    out = torch.from_numpy(mean).to(sc.device)
    _sync(sc)
    if timings is not None:
        timings.update(rolling_mean_download_s=t1 - t, rolling_mean_pandas_s=t2 - t1, rolling_mean_upload_s=perf_counter() - t2)
    return out


def _sync(t):
    if t.is_cuda:
        import torch
        torch.cuda.synchronize(t.device)


class _Clock:
    """timings[name + "_s"] = seconds since the last tick, the device's queued work included."""

    def __init__(self, timings, ref):
        self.timings, self.ref, self.t = timings, ref, perf_counter()

    def tick(self, name):
        if self.timings is not None:
            _sync(self.ref)
            now = perf_counter()
            self.timings[name + "_s"] = now - self.t
            self.t = now


def coordsOf(start, end, runs):
    """object [G, 3]: chromosome, start, end -- the values of mm.readScores' inputArr[:, :3]."""
    coords = np.empty((len(start), 3), dtype=object)
    for name, a, b in runs:
        coords[a:b, 0] = name
    coords[:, 1], coords[:, 2] = start, end
    return coords


def pickTop(sc, rmean, valid, W, maxRegions, clock=None, timings=None):
    """The device part of roiSingle.maxMean, shared by pickRegions and by STEP 4's `--roi gpu` (roiSingle.maxMeanDevice): sc and rmean
    float64 [m] (the centre scores and pandas' rolling means of the rows that have both shifted coordinates), valid bool [m] (False
    where a window spans two chromosomes), all on one device -> (at, rmax): the picked windows' indices into sc, best first, and their
    rolling maxima, as host arrays.  Rolling maximum, compaction of the kept windows, rank and greedy pick run through the
    module-level steps, the pick in the compacted index space as the host's does; the final best-first order of the few picked
    windows is the host's lexsort."""
    import torch
    tick = clock.tick if clock is not None else (lambda name: None)
    none = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float64)
    rmax = rollingMax(sc, W)
    tick("rolling_max")
    ok = ~torch.isnan(rmax)                                # incomplete edge windows
    ok &= valid                                            # windows spanning two chromosomes
    keep = torch.nonzero(ok).reshape(-1)
    sc_c, rmax_c, rmean_c = sc[keep], rmax[keep], rmean[keep]
    tick("compact")
    if not keep.numel():
        return none
    rank = rankWindows(rmax_c, rmean_c, sc_c)
    tick("rank")
    chosen, launches = pickWindows(rank, W, maxRegions)
    tick("pick")
    if timings is not None:
        timings.update(pick_launches=launches, windows=int(keep.numel()), picked=int(len(chosen)))
    if not len(chosen):
        return none
    ch = torch.from_numpy(chosen).to(sc.device)
    # best first, as maxMean's last sort: by (rolling max, rolling mean), windows that tie on both in genomic order
    top = rmax_c[ch].cpu().numpy()
    final = np.lexsort((-rmean_c[ch].cpu().numpy(), -top))
    at = keep[ch].cpu().numpy()[final]
    tick("final_order")
    return at, top[final]


def pickRegions(x, start, end, windowBins, timings=None):
    """roiSingle.maxMean with maxRegions = G // windowBins on the device grid -> the centre rows (int64, best first) and the
    window coordinates (start of the bin h to the left, end of the bin h / h - 1 to the right)."""
    import torch
    clock = _Clock(timings, x)
    G = x.shape[0]
    W, h = int(windowBins), int(windowBins) // 2
    maxRegions = G // W
    e_off = h if W % 2 else h - 1
    lo, hi = h, G - e_off                                  # rows that have both shifted coordinates
    none = np.zeros(0, dtype=np.int64)
    if hi <= lo:
        return none, none, none
    score = rowScores(x)
    clock.tick("rowscore")
    sc = score[lo:hi]
    rmean = rollingMean(sc, W, timings)
    clock.tick("rolling_mean")
    w_start, w_end = start[lo - h:hi - h], end[lo + e_off:hi + e_off]
    at, _top = pickTop(sc, rmean, torch.from_numpy(np.asarray(w_start < w_end)).to(x.device), W, maxRegions, clock, timings)
    if not len(at):
        return none, none, none
    return lo + at, np.asarray(w_start)[at], np.asarray(w_end)[at]                # (at: index into rows lo .. hi)


def selectRegions(x, start, end, runs, windowBins, blockSize, filterState, filterScore, timings=None):
    """mm.selectRegions on the device grid -> (roiCoords object [R, 3], roiCube int64 [R, windowBins // blockSize, S])."""
    orig, w_start, w_end = pickRegions(x, start, end, windowBins, timings)
    clock = _Clock(timings, x)
    nblk = int(windowBins) // int(blockSize)
    roiCoords = np.empty((len(orig), 3), dtype=object)
    if len(orig):
        row0 = np.array([r[1] for r in runs], dtype=np.int64)
        names = np.array([r[0] for r in runs], dtype=object)
        roiCoords[:, 0] = names[np.searchsorted(row0, orig, side="right") - 1]
        roiCoords[:, 1], roiCoords[:, 2] = w_start, w_end
        roiCube = slices(x, orig - int(windowBins) // 2, nblk, blockSize)
    else:
        roiCube = np.zeros((0, nblk, x.shape[1]), dtype=np.int64)
    clock.tick("slices")
    return mm.removeRegions(roiCoords, roiCube, filterState, filterScore)


class _Writer(threading.Thread):
    """genome_stats.npz on a host thread; join() raises what the thread raised."""

    def __init__(self, outputDir, grid, coords):
        super().__init__()
        self.args, self.error, self.seconds = (outputDir, grid, coords), None, None

    def run(self):
        try:
            t = perf_counter()
            outputDir, grid, coords = self.args
            np.savez_compressed(Path(outputDir) / "genome_stats", scores=grid / float(mm.SCALE), coords=coords)
            self.seconds = perf_counter() - t
        except BaseException as e:                         # noqa: B036 -- handed to the caller of finish()
            self.error = e

    def finish(self):
        self.join()
        if self.error is not None:
            raise self.error
        return self.seconds


def main(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore, timings=None, inflate="host"):
    from . import scoresText
    outputDir = Path(outputDir)
    t = time()
    try:
        x, start, end, runs = readDevice(scoresPath, timings, **({"inflate": inflate} if inflate != "host" else {}))
    except scoresText.NotStrict as e:
        print("            Warning: %s is not a plain \"%%.5f\" scores file (row %d: %s); reading it with pandas"
              % (scoresPath, e.row, e.reason), flush=True)
        return mm.main(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore)
    print("Reading in data...", flush=True)
    if timings is not None:
        timings["read_s"] = time() - t
    writer = _Writer(outputDir, x.cpu().numpy(), coordsOf(start, end, runs))
    writer.start()
    try:
        print("    Time:", format(time() - t, '.0f'), "seconds\n", flush=True)
        print("Finding regions of size {}kb...".format(windowBP // 1000), flush=True); t1 = time()
        roiCoords, roiCube = selectRegions(x, start, end, runs, windowBins, blockSize, filterState, filterScore, timings)
        np.savez_compressed(file=outputDir / "simsearch_cube", scores=roiCube / mm.SCALE, coords=roiCoords)
        print("    Time:", format(time() - t1, '.0f'), "seconds\n", flush=True)
        print("Reducing genome scores by factor of {}...".format(blockSize), flush=True); t2 = time()
        np.save(outputDir / "reduced_genome.npy", reduce(x, blockSize) / mm.SCALE, allow_pickle=True)
        if timings is not None:
            timings["reduce_s"] = time() - t2
        print("    Time:", format(time() - t2, '.0f'), "seconds\n", flush=True)
    finally:
        seconds = writer.finish()
    if timings is not None:
        timings["genome_stats_write_s"] = seconds
    print("Total time:", format(time() - t, '.0f'), "seconds\n", flush=True)


if __name__ == "__main__":
    if "LOCAL_RANK" in os.environ:              # the STEP 1 child of `similaritySearch_run --gpus N --step1 gpu`: its GPU
        import torch
        if torch.cuda.is_available():            # (without one, require_gpu says so)
            local = int(os.environ["LOCAL_RANK"])
            torch.cuda.set_device(local % torch.cuda.device_count() if os.environ.get("EPILOGOS_DIST_BACKEND") else local)
    extra = {"inflate": sys.argv[9]} if len(sys.argv) > 9 and sys.argv[8] == "--inflate" else {}      # (step1Job appends it for `gpu` alone)
    main(Path(sys.argv[1]), Path(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]),
         float(sys.argv[7]), **extra)
