"""Similarity search STEP 2 -- the search itself, on the GPU.  Same signature and output as the reference's
epilogos/similaritySearch_calc.py (main :14-33, runEuclideanDistance :67-123): simsearch_indices_{processTag}.npy, int32
[rows, nDesiredMatches], indices into reduced_genome.npy.

For every region of interest (ROI) the distance to every window of the reduced genome, their mode, their stable order and the
greedy pick of non-overlapping windows closer than half the mode run in epg_simsearch (csrc/epg_simsearch.hip) on exact
integers, ROI batches sized from a workspace cap."""
import os
import sys
from pathlib import Path
from time import time

import numpy as np

from .helpers import splitRows
from .similaritySearch_max_mean import to_grid

WS_CAP_BYTES = 2 << 30          # device workspace per batch (keys, sorted keys and positions: about 20 bytes per ROI and window)
EXACT_LIMIT = 1 << 53


def state_ranges(X):
    """Per-state (min, max) of X [..., S] (int64)."""
    X = X.reshape(-1, X.shape[-1])
    return X.min(axis=0), X.max(axis=0)


def bound_from_ranges(g_range, q_range, W):
    """W * sum_s range_s^2, range_s the spread of state s over the genome's and the ROIs' (min, max).  A Python int."""
    lo = np.minimum(g_range[0], q_range[0]).astype(object)
    hi = np.maximum(g_range[1], q_range[1]).astype(object)
    return int(W) * int(sum((h - l) ** 2 for h, l in zip(hi, lo)))


def key_bound(G, Q, W, g_range=None):
    """An upper bound of every distance between a W-row window of G [Pg, S] and a ROI of Q [B, W, S] (int64): W * sum_s range_s^2,
    range_s the spread of state s over both.  g_range: G's state_ranges, when the caller has them.  A Python int."""
    return bound_from_ranges(g_range if g_range is not None else state_ranges(G), state_ranges(Q), W)


def check_exact(bound, S, W):
    if bound >= EXACT_LIMIT:
        raise ValueError("similarity search: distances up to %d (units of 1e-10) are not exact in fp64; the bound is 2^53 = %d, "
                         "i.e. %d * sum over the %d states of (max - min score)^2 < 2^53 (all scores within +-A: A < %.2f)"
                         % (bound, EXACT_LIMIT, W, S, (EXACT_LIMIT / (W * S)) ** 0.5 / 2e5))


def batch_rows(Pg, S, W, R, ws_cap=WS_CAP_BYTES):
    """ROIs per epg_simsearch call under the workspace cap (at least 1)."""
    from . import engine
    P = Pg - W + 1
    fixed = engine.simsearch_ws_bytes(Pg, S, W, 1) - 20 * P
    return int(max(1, min(R, (ws_cap - fixed) // (20 * P))))


def tensor_ranges(x):
    """state_ranges of a device tensor [..., S]."""
    x = x.reshape(-1, x.shape[-1])
    return x.amin(dim=0).cpu().numpy().astype(np.int64), x.amax(dim=0).cpu().numpy().astype(np.int64)


def search_on_device(g, g_range, R, W, nDesiredMatches, batch_of, ws_cap=WS_CAP_BYTES, batch=None, want_dist=False):
    """The search on tensors that are on the device already: g int32 [Pg, S] (the reduced genome, row-major), g_range its
    state_ranges; batch_of(r0, r1) -> (q int32 [r1 - r0, W, S], self starts int32 [r1 - r0]) of ROIs r0 .. r1, device tensors.
    ROI batches under the workspace cap, each with its own key_bound (check_exact refuses it beyond 2^53) -> (indices int32
    [R, n], mode int64 [R] and, with want_dist, the distances int64 [R, Pg - W + 1]), numpy arrays."""
    import torch
    from . import engine
    Pg, S = g.shape
    n = int(nDesiredMatches)
    if Pg < W:
        raise ValueError("similarity search: a reduced genome of %d positions is shorter than the %d-position window" % (Pg, W))
    P = Pg - W + 1
    idx = np.zeros((R, n), dtype=np.int32)
    mode = np.zeros(R, dtype=np.int64)
    dist = np.zeros((R, P), dtype=np.int64) if want_dist else None
    B = int(batch) if batch else batch_rows(Pg, S, W, R, ws_cap)
    ws = torch.empty(engine.simsearch_ws_bytes(Pg, S, W, min(B, R)), dtype=torch.uint8, device=g.device)
    for r0 in range(0, R, B):
        r1 = min(R, r0 + B)
        q, ss = batch_of(r0, r1)
        bound = bound_from_ranges(g_range, tensor_ranges(q), W)
        check_exact(bound, S, W)
        o_idx, o_mode, o_dist = engine.simsearch(g, W, q, ss, n, bound, ws=ws, want_dist=want_dist)
        idx[r0:r1] = o_idx.cpu().numpy()
        mode[r0:r1] = o_mode.cpu().numpy()
        if want_dist:
            dist[r0:r1] = o_dist.cpu().numpy()
    return (idx, mode, dist) if want_dist else (idx, mode)


def simsearch(G, Q, selfStart, nDesiredMatches, ws_cap=WS_CAP_BYTES, batch=None, want_dist=False):
    """G int64 [Pg, S], Q int64 [R, W, S] (scaled scores), selfStart int [R] -> (indices int32 [R, n], mode int64 [R]
    (units of 1e-10) and, with want_dist, the distances int64 [R, Pg - W + 1])."""
    import torch
    from . import engine
    engine.require_gpu()
    G = np.asarray(G, dtype=np.int64)
    Q = np.asarray(Q, dtype=np.int64)
    Pg, S = G.shape
    R, W = Q.shape[0], Q.shape[1]
    n = int(nDesiredMatches)
    if R == 0:
        idx, mode = np.zeros((0, n), dtype=np.int32), np.zeros(0, dtype=np.int64)
        return (idx, mode, np.zeros((0, max(Pg - W + 1, 0)), dtype=np.int64)) if want_dist else (idx, mode)
    if Pg < W:
        raise ValueError("similarity search: a reduced genome of %d positions is shorter than the %d-position window" % (Pg, W))
    g_range = state_ranges(G)                    # once: each batch's bound combines it with the batch's own ROIs
    check_exact(key_bound(G, Q, W, g_range), S, W)
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.int32)).to(dev)   # row-major (reduced_genome.npy may be F-ordered)
    selfStart = np.asarray(selfStart)

    def upload(r0, r1):
        return (torch.from_numpy(np.ascontiguousarray(Q[r0:r1], dtype=np.int32)).to(dev),
                torch.from_numpy(np.ascontiguousarray(selfStart[r0:r1], dtype=np.int32)).to(dev))
    return search_on_device(g, g_range, R, W, n, upload, ws_cap, batch, want_dist)


def selfStarts(genomeCoords, roiCoords, blockSize):
    """Reduced position of each ROI's own window: the index of the first genome bin with the ROI's chromosome and start,
    // blockSize (reference :96-98).  Looks up the ROIs only: one sorted (chromosome, start) key array of the genome."""
    chroms, cidx = np.unique(np.asarray(genomeCoords[:, 0]).astype(str), return_inverse=True)
    gstart = np.asarray(genomeCoords[:, 1]).astype(np.int64)
    order = np.lexsort((np.arange(len(gstart)), gstart, cidx))       # by chromosome, start, then bin: the first bin of a key first
    kc, ks = cidx[order], gstart[order]
    rc = np.searchsorted(chroms, np.asarray(roiCoords[:, 0]).astype(str))
    rst = np.asarray(roiCoords[:, 1]).astype(np.int64)
    out = np.empty(len(rst), dtype=np.int64)
    for i, (c, s) in enumerate(zip(rc, rst)):
        lo = np.searchsorted(kc, c, side="left")
        hi = np.searchsorted(kc, c, side="right")
        j = lo + np.searchsorted(ks[lo:hi], s, side="left")
        if c >= len(chroms) or j >= hi or ks[j] != s:
            raise ValueError("similarity search: region %s:%d has no bin in the genome" % (roiCoords[i, 0], s))
        out[i] = order[j] // blockSize
    return out


def main(outputDir, windowBins, blockSize, nCores, nDesiredMatches, nJobs, processTag):
    print("Calculating search results...", flush=True); t = time()
    outputDir = Path(outputDir)
    genomeCoords = np.load(outputDir / "genome_stats.npz", allow_pickle=True)["coords"]
    cube = np.load(outputDir / "simsearch_cube.npz", allow_pickle=True)
    roiCube, roiCoords = cube["scores"], cube["coords"]
    lo, hi = splitRows(roiCube.shape[0], nJobs)[processTag]
    G = to_grid(np.load(outputDir / "reduced_genome.npy", allow_pickle=True), "reduced_genome.npy")
    Q = to_grid(roiCube[lo:hi], "simsearch_cube.npz")
    rs = selfStarts(genomeCoords, roiCoords[lo:hi], blockSize)
    idx, _mode = simsearch(G, Q, rs, nDesiredMatches)
    np.save(outputDir / "simsearch_indices_{}.npy".format(processTag), idx, allow_pickle=True)
    print("    Time:", format(time() - t, '.0f'), "seconds\n", flush=True)


if __name__ == "__main__":
    if "LOCAL_RANK" in os.environ:              # a child of `similaritySearch_run --gpus N`: its own GPU (shared under
        import torch                             # EPILOGOS_DIST_BACKEND=gloo, as the `epilogos` command's ranks share it)
        if torch.cuda.is_available():            # (without one, simsearch's require_gpu says so)
            local = int(os.environ["LOCAL_RANK"])
            torch.cuda.set_device(local % torch.cuda.device_count() if os.environ.get("EPILOGOS_DIST_BACKEND") else local)
    main(Path(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]),
         int(sys.argv[7]))
