"""A restatement of the pieces of roiSingle.maxMean that `simsearch -b --step1 gpu` moves to the device, to test against: the greedy
walk over a given order (roiSingle.greedyWalk's loop), the lexsort rank, pandas' rolling maximum and row sums; CPU-tensor stand-ins of
similaritySearch_step1's device steps built from them; the rank patterns of the pick tests; a synthetic scores file with a plateau.
A plain module, not a conftest: the tests that want it import it."""
import numpy as np
import pandas as pd


def walk(order, n, W, maxRegions):
    """greedyWalk's loop: the positions of `order` (best first) taken while none of the W positions of their window is hit; sorted."""
    h = int(W) // 2
    hits = np.zeros(n, dtype=bool)
    chosen = []
    for m in order:
        if len(chosen) >= maxRegions:
            break
        a = max(m - h, 0)
        b = min(m + h + 1 if W % 2 else m + h, n)
        if not hits[a:b].any():
            hits[a:b] = True
            chosen.append(int(m))
    return np.array(sorted(chosen), dtype=np.int64)


def pick(rank, W, maxRegions):
    """The walk over the order that `rank` (a permutation: rank[i] = position of i in the order) stands for."""
    rank = np.asarray(rank, dtype=np.int64)
    order = np.empty(len(rank), dtype=np.int64)
    order[rank] = np.arange(len(rank))
    return walk(order, len(rank), W, maxRegions)


def lexsort_rank(rmax, rmean, score):
    order = np.lexsort((-np.asarray(score), -np.asarray(rmean), -np.asarray(rmax)))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank


def rolling_max(v, W):
    return pd.Series(np.asarray(v, dtype=np.float64)).rolling(int(W), center=True).max().to_numpy()


def row_scores(x):
    """((x[:, 0] / 1e5 + x[:, 1] / 1e5) + x[:, 2] / 1e5) + ..., float64, left to right."""
    x = np.asarray(x)
    acc = np.zeros(x.shape[0], dtype=np.float64)
    for s in range(x.shape[1]):
        acc = acc + x[:, s].astype(np.float64) / 1e5
    return acc


# ---- rank patterns of the pick tests ---------------------------------------------------------------------------------------------

PATTERNS = ["random", "identity", "reversed", "saw_tile", "saw_window", "best_first_of_tile", "best_last_of_tile"]


def _rank_of_keys(keys):
    """Ranks of a key vector, smallest key best, ties in index order."""
    order = np.argsort(keys, kind="stable")
    rank = np.empty(len(keys), dtype=np.int64)
    rank[order] = np.arange(len(keys))
    return rank


def pattern(name, n, W, T, seed=0):
    """A permutation of 0 .. n - 1 as the ranks of n positions."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    if name == "random":
        return rng.permutation(n).astype(np.int64)
    if name == "identity":                         # an all-ties plateau: ranked by position
        return i.astype(np.int64)
    if name == "reversed":
        return i[::-1].astype(np.int64)
    if name == "saw_tile":
        return _rank_of_keys(i % T)
    if name == "saw_window":
        return _rank_of_keys(i % W)
    rank = rng.permutation(n).astype(np.int64)
    at = {"best_first_of_tile": (min(n - 1, T) // T) * T, "best_last_of_tile": min(n, T) - 1}[name]
    rank[np.nonzero(rank == 0)[0][0]], rank[at] = rank[at], 0
    return rank


# ---- CPU-tensor stand-ins of similaritySearch_step1's device steps -----------------------------------------------------------------

def install(monkeypatch, step1, mm):
    """numpy in place of every device step of `step1`; the reader returns what mm.readScores gives, as CPU tensors."""
    import torch
    from epilogos_amd.similaritySearch_query import chromosomeTable

    def readDevice(scoresPath, timings=None):
        _scores, inputArr, genome = mm.readScores(scoresPath)
        table = chromosomeTable(inputArr[:, 0], inputArr[:, 1], inputArr[:, 2])
        runs = sorted(((name, row0, row0 + len(st)) for name, (row0, st, _e) in table.items()), key=lambda r: r[1])
        return (torch.from_numpy(genome.astype(np.int32)), inputArr[:, 1].astype(np.int64), inputArr[:, 2].astype(np.int64), runs)

    def slices(x, first, nblk, blockSize):
        g = x.numpy().astype(np.int64)
        w = int(nblk) * int(blockSize)
        return np.stack([mm.makeSlice(g, int(f) + w // 2, w, blockSize) for f in first])

    def reduce(x, blockSize):
        g = x.numpy().astype(np.int64)
        return g[mm.reduceGenomeIndices(g, blockSize)]

    monkeypatch.setattr(step1, "readDevice", readDevice)
    monkeypatch.setattr(step1, "rowScores", lambda x: torch.from_numpy(row_scores(x.numpy())))
    monkeypatch.setattr(step1, "rollingMax", lambda v, W: torch.from_numpy(rolling_max(v.numpy(), W)))
    monkeypatch.setattr(step1, "rankWindows", lambda a, b, c: torch.from_numpy(lexsort_rank(a.numpy(), b.numpy(), c.numpy()).astype(np.int32)))
    monkeypatch.setattr(step1, "pickWindows", lambda rank, W, maxRegions: (pick(rank.numpy(), W, maxRegions), 0))
    monkeypatch.setattr(step1, "slices", slices)
    monkeypatch.setattr(step1, "reduce", reduce)


# ---- a synthetic scores file -------------------------------------------------------------------------------------------------------

def plateau_scores_text(bins=6000, S=15, first_chrom=2937, plateau=(3200, 4700), seed=7):
    """A 200-bp "%.5f" scores file of `bins` rows by S states as bytes: two chromosomes (the change, at row first_chrom, falls inside
    windows of 125 bins that start before it), and a stretch of identical rows (a plateau: windows tied on all three keys)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-30000, 250000, size=(bins, S))
    k[rng.random((bins, S)) < 0.5] = 0
    k[plateau[0]:plateau[1]] = k[plateau[0]]
    lines = []
    for r in range(bins):
        chrom, r0 = ("chr1", r) if r < first_chrom else ("chr2", r - first_chrom)
        lines.append("%s\t%d\t%d\t%s\n" % (chrom, r0 * 200, r0 * 200 + 200, "\t".join("%.5f" % (v / 1e5) for v in k[r])))
    return "".join(lines).encode()
