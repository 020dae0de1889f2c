#!/usr/bin/env python3
"""Similarity search STEP 2 on a whole-genome-size synthetic input: distance, sort and select times per region of interest.

    python tools/simsearch_bench.py [--positions 3000000] [--states 18] [--rois 512] [--batch 0] [--reps 2]

The reduced genome has --positions rows (a 200-bp genome with the default 25 kb window and block size 5 has about 3 M): a
background class (90 % of the rows) among 40 row classes, plus planted noisy copies of one window; the ROIs are windows of the
genome.  Timed: the bare epg_simsearch calls over all ROIs in batches (`ms_per_roi`), and the product's path,
similaritySearch_calc.simsearch (host bounds, uploads, downloads: what `similaritySearch_run -b` runs as STEP 2,
`simsearch_path_ms_per_roi`).  The split into distance, sort and select (`stages_ms_per_roi`) comes from a child run of this tool
under `rocprofv3 --kernel-trace --stats` (kernel device time: k_simsearch_dist, the rocPRIM sort kernels with their buffer fills,
k_simsearch_select); --no-stages skips it.  Prints one JSON line, with the path's time extrapolated to 20 000 and 120 000 ROIs.

    python tools/simsearch_bench.py --gpus N [--bins 1000000]

times the whole command instead, `python -m epilogos_amd.similaritySearch_run -b --gpus N`, on a synthetic 200-bp scores file of
--bins bins drawn the same way (default window: 25 kb, block size 5).  The JSON line has the wall time of the command and of its
STEP 1, STEP 2 and STEP 3 (from the moment each STEP line reaches this tool's pipe; `startup_s` is the time before STEP 1).  This
process never touches the GPU.  With more processes than GPUs, set EPILOGOS_DIST_BACKEND=gloo to let them share one: STEP 2's
GPU work is then the same as with --gpus 1 and the difference is the cost of the extra processes.

    python tools/simsearch_bench.py --query N [--bins 1000000] [--genome-bins 15000000]

times the live query (`similaritySearch_run -q ... -s ...`, similaritySearch_query.py) for N random regions on the same synthetic
scores file (multi-member gzip as the scoring path writes it, BGZF with --bgzf): seconds to read it (`read_s`: readGrid, the median
of --read-reps reads) with its parts (`read_split`: inflate_s = the host's inflate alone, count_s = chunk cutting and row counts, upload_parse_ms = staging,
upload and the parse kernels between two HIP events, coords_s = coordinates and chromosome names to the host, download_s = the
int32 grid back to the host as int64, which readGrid's host-array contract costs) next to pandas' read of the same file
(`pandas_read_s`, mm.readScores, the reads taken in turn), ms for the upload + epg_simsearch_reduce (`upload_reduce_ms`), for
epg_simsearch_slices of all N (`slices_ms`), per region for slices + search one region per call and at the workspace cap's batch
(`search_ms_per_region`), and for the coordinates and files (`write_ms`).  `genome` has the reduce kernel alone on --genome-bins
bins made on the device (best of --reps + 1), a device-to-device copy of the same bytes on the same device, the host's
reduceGenomeIndices + gather of the same array, and slices + search of the N regions on that genome.

    python tools/simsearch_bench.py --step1 [--bins 1000000] [--genome-bins 15000000]

times STEP 1 of the build both ways on the same synthetic scores file, one JSON line per path: the host's
(similaritySearch_max_mean: read, pick = roiSingle.maxMean, slices = makeSlice per region + removeRegions, reduce, the
genome_stats write) and the device's (similaritySearch_step1: read, rowscore, the pandas rolling mean with its download and
upload, rolling max, compaction, rank, pick with its sweeps, final order, slices, reduce, the genome_stats write on its thread), and
stops if the two paths' files differ.  A third line has the rank and the pick alone on --genome-bins windows whose three keys are
made in memory, with one plateau of 90 000 tied windows, against roiSingle.greedyWalk (maxMean's sort and walk) on the same
keys; it stops if the two picks differ."""
import argparse
import csv
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=3_000_000)
    ap.add_argument("--states", type=int, default=18)
    ap.add_argument("--rois", type=int, default=512)
    ap.add_argument("--batch", type=int, default=0, help="ROIs per call (0: from the 2 GiB workspace cap)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-stages", action="store_true", help="skip the profiled child run that splits the stages")
    ap.add_argument("--gpus", type=int, default=None, help="time the -b command with --gpus N end to end instead")
    ap.add_argument("--bins", type=int, default=1_000_000, help="bins of the synthetic scores file (with --gpus, --query)")
    ap.add_argument("--query", type=int, default=None, help="time the live query of N random regions instead")
    ap.add_argument("--genome-bins", type=int, default=15_000_000, help="bins of the reduce kernel's own measurement (--query)")
    ap.add_argument("--read-reps", type=int, default=5, help="reads of the scores file per reader; the medians are reported (--query)")
    ap.add_argument("--bgzf", action="store_true", help="write the synthetic scores file as BGZF: its blocks inflate in parallel (--query)")
    ap.add_argument("--step1", action="store_true", help="time STEP 1 of the build on the host and on the device instead")
    a = ap.parse_args()
    if a.step1:
        step1_bench(a)
        return
    if a.query is not None:
        query_bench(a)
        return
    if a.gpus is not None:
        build_bench(a)
        return
    import torch
    from epilogos_amd import _abi, engine
    from epilogos_amd import similaritySearch_calc as calc
    engine.require_gpu()
    W, S = 25, a.states
    Pg = a.positions + W - 1
    rng = np.random.default_rng(0)
    base = rng.integers(0, 100000, size=(40, S))
    G = base[np.where(rng.random(Pg) < 0.9, 0, rng.integers(0, 40, size=Pg))].astype(np.int64)
    src = rng.integers(0, 100000, size=(W, S))
    for s in rng.integers(0, Pg - W, size=500):
        G[s:s + W] = src + rng.integers(-50, 50, size=src.shape)
    starts = rng.integers(0, Pg - W, size=a.rois)
    Q = np.stack([G[s:s + W] for s in starts])
    B = a.batch or calc.batch_rows(Pg, S, W, a.rois)
    bound = calc.key_bound(G, Q, W)
    calc.check_exact(bound, S, W)
    dev = torch.device("cuda", 0)
    g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.int32)).to(dev)
    q = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.int32)).to(dev)
    ss = torch.from_numpy(starts.astype(np.int32)).to(dev)
    lib = _abi.load()
    wsb = lib.epg_simsearch_ws_bytes(Pg, S, W, B)
    _abi.check(wsb)
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
    idx = torch.empty((a.rois, 100), dtype=torch.int32, device=dev)
    mode = torch.empty(a.rois, dtype=torch.int64, device=dev)

    def run_all(kb):
        for r0 in range(0, a.rois, B):
            b = min(B, a.rois - r0)
            _abi.call("epg_simsearch", engine._ptr(g), Pg, S, W, C.c_void_p(q.data_ptr() + r0 * W * S * 4), b,
                      C.c_void_p(ss.data_ptr() + r0 * 4), 100, C.c_uint64(kb), engine._ptr(ws), int(wsb),
                      C.c_void_p(idx.data_ptr() + r0 * 400), C.c_void_p(mode.data_ptr() + r0 * 8), None, engine._stream())

    def timed(kb):
        best = None
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            run_all(kb)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return best

    run_all(bound)                            # warm-up (code objects, sort configuration)
    t_full = timed(bound)
    per_roi = t_full / a.rois * 1e3
    res = {"tool": "simsearch_bench", "positions": a.positions, "states": S, "rois": a.rois, "batch": B,
           "key_bits": int(bound).bit_length(), "ms_per_roi": round(per_roi, 4), "total_s": round(t_full, 3),
           "dist_gflop_per_roi": round(3 * a.positions * W * S / 1e9, 2)}
    if a.no_stages:
        print(json.dumps(res), flush=True)
        return
    torch.cuda.synchronize()
    t = time.perf_counter()
    calc.simsearch(G, Q, starts, 100, batch=B)
    path_ms = (time.perf_counter() - t) / a.rois * 1e3
    res["simsearch_path_ms_per_roi"] = round(path_ms, 4)
    res["extrapolated_s"] = {"20000": round(path_ms * 20000 / 1e3, 1), "120000": round(path_ms * 120000 / 1e3, 1)}
    res["stages_ms_per_roi"] = stages(a, B)
    print(json.dumps(res), flush=True)


def synthetic_scores(path, bins, S):
    """A 200-bp scores file (chr1) of 40 row classes, the first on 90 % of the bins, values on the 1e-5 grid in [0, 1)."""
    from epilogos_amd import _io
    rng = np.random.default_rng(0)
    base = rng.integers(0, 100000, size=(40, S))
    x = base[np.where(rng.random(bins) < 0.9, 0, rng.integers(0, 40, size=bins))] + rng.integers(0, 50, size=(bins, S))
    lines = ["chr1\t%d\t%d\n" % (200 * i, 200 * i + 200) for i in range(bins)]
    blob = "".join(lines).encode()
    off = np.zeros(bins + 1, dtype=np.int64)
    np.cumsum([len(line) for line in lines], out=off[1:])
    _io.write_scores(path, _io.Locations(np.frombuffer(blob, dtype=np.uint8).copy(), off), (x / 1e5).astype(np.float32))


def query_bench(a):
    """The live query's stages on a synthetic scores file, and the reduce kernel against a copy on a genome-size array."""
    import torch
    from epilogos_amd import _abi, engine
    from epilogos_amd import similaritySearch_max_mean as mm
    from epilogos_amd import similaritySearch_query as sq
    from epilogos_amd import similaritySearch_write as wr
    from epilogos_amd import scoresText
    engine.require_gpu()
    S, N, blockSize, nblk, windowBins = a.states, a.query, 5, 25, 125

    def timed(f, reps=1):
        best = None
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return best, out

    with tempfile.TemporaryDirectory() as d:
        sp = Path(d) / "scores.txt.gz"
        was = os.environ.get("EPILOGOS_BGZF")
        if a.bgzf:
            os.environ["EPILOGOS_BGZF"] = "1"         # for the writer of the synthetic file only
        else:
            os.environ.pop("EPILOGOS_BGZF", None)
        synthetic_scores(sp, a.bins, S)
        if was is None:
            os.environ.pop("EPILOGOS_BGZF", None)
        else:
            os.environ["EPILOGOS_BGZF"] = was
        torch.zeros(1, device="cuda")                 # the context is not part of the first stage
        med = lambda v: round(float(np.median(v)), 4)
        pandas_s, read_s, split = [], [], {"inflate_s": [], "count_s": [], "upload_parse_ms": [], "coords_s": [], "download_s": []}
        sq.readGrid(sp)                               # warm-up (code objects, the page-locked buffers' first allocation)
        for _ in range(a.read_reps):                  # the two readers in turn: other people's work shares the host
            t = time.perf_counter()
            _scores, inputArr, genome_pd = mm.readScores(sp)
            pandas_s.append(time.perf_counter() - t)
            t = time.perf_counter()
            coords, genome = sq.readGrid(sp)
            read_s.append(time.perf_counter() - t)
            tm = {}
            x, _start, _end, _runs = scoresText.read_scores_device(sp, timings=tm)
            torch.cuda.synchronize()
            t = time.perf_counter()
            x.cpu().numpy().astype(np.int64)          # what readGrid's host-array contract costs on top (the re-upload is
            tm["download_s"] = time.perf_counter() - t    # upload_reduce_ms below)
            del x
            for k in split:
                split[k].append(tm[k])
        same = bool(np.array_equal(genome, genome_pd) and (coords == inputArr[:, :3]).all())
        if not same:
            sys.exit("simsearch_bench: readGrid and mm.readScores disagree on %s: no timing of a wrong result" % sp)
        read_s, pandas_read_s, split = med(read_s), med(pandas_s), {k: med(v) for k, v in split.items()}
        del genome_pd, inputArr
        t_reduce, state = timed(lambda: sq.reduceGenome(genome, blockSize))
        first = np.random.default_rng(1).integers(0, a.bins - windowBins + 1, size=N)
        sq.slices(state, first[:1], nblk, blockSize)
        t_slices, _q = timed(lambda: sq.slices(state, first, nblk, blockSize), 1 + a.reps)
        sq.search(state, first[:1], nblk, blockSize, 100)                     # warm-up (code objects, sort configuration)
        n1 = min(N, 8)
        t_one, _ = timed(lambda: sq.search(state, first[:n1], nblk, blockSize, 100, batch=1), a.reps)
        t_cap, idx = timed(lambda: sq.search(state, first, nblk, blockSize, 100), a.reps)
        t = time.perf_counter()
        reducedCoords = wr.reduceGenomeCoords(coords, blockSize)
        for f, row in zip(first, idx):
            (Path(d) / ("region_%d_recs.bed" % f)).write_text(sq.recsText(row, reducedCoords, nblk))
        write_ms = (time.perf_counter() - t) * 1e3
        Pg = state[1].shape[0]
    res = {"tool": "simsearch_bench", "mode": "query", "bins": a.bins, "states": S, "regions": N, "positions": int(Pg),
           "batch_at_cap": calc_batch(Pg, S, nblk, N), "file": "bgzf" if a.bgzf else "gzip", "read_s": read_s, "read_split": split,
           "pandas_read_s": pandas_read_s, "read_reps": a.read_reps, "read_equal_to_pandas": same, "upload_reduce_ms": round(t_reduce * 1e3, 3),
           "slices_ms": round(t_slices * 1e3, 4),
           "search_ms_per_region": {"batch_1": round(t_one / n1 * 1e3, 4), "batch_at_cap": round(t_cap / N * 1e3, 4)},
           "write_ms": round(write_ms, 2)}
    del state

    # the reduce kernel alone at genome size, against a copy of the same bytes and the host code it replaces
    R = a.genome_bins
    g0 = torch.Generator(device="cuda").manual_seed(0)
    base = torch.randint(0, 100000, (40, S), dtype=torch.int32, device="cuda", generator=g0)
    cls = torch.randint(0, 40, (R,), device="cuda", generator=g0)
    cls[torch.rand(R, device="cuda", generator=g0) < 0.9] = 0
    x = base[cls].contiguous()
    del cls
    g = torch.empty((-(-R // blockSize), S), dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    reduce_call = lambda: _abi.call("epg_simsearch_reduce", engine._ptr(x), R, S, blockSize, engine._ptr(g), None, engine._stream())
    reduce_call()
    t_k, _ = timed(reduce_call, 1 + a.reps)
    y.copy_(x)
    t_c, _ = timed(lambda: y.copy_(x), 1 + a.reps)
    del y
    # slices + search at genome size (what a whole-genome -q -s run pays per region), one region per call and at the cap's batch
    state = (x, g, calc_ranges(g))
    Pg = g.shape[0]
    first = np.random.default_rng(2).integers(0, R - windowBins + 1, size=N)
    sq.search(state, first[:1], nblk, blockSize, 100)
    t_one, _ = timed(lambda: sq.search(state, first[:n1], nblk, blockSize, 100, batch=1), a.reps)
    t_cap, _ = timed(lambda: sq.search(state, first, nblk, blockSize, 100), a.reps)
    t_sl, _ = timed(lambda: sq.slices(state, first, nblk, blockSize), 1 + a.reps)
    del state
    xh = x.cpu().numpy().astype(np.int64)
    t = time.perf_counter()
    gh = xh[mm.reduceGenomeIndices(xh, blockSize)]
    host_s = time.perf_counter() - t
    same = bool(np.array_equal(g.cpu().numpy(), gh))
    nbytes = R * S * 4
    res["genome"] = {"bins": R, "bytes_read": nbytes, "reduce_kernel_ms": round(t_k * 1e3, 4),
                     "reduce_tb_per_s": round((nbytes + nbytes // blockSize) / t_k / 1e12, 3),
                     "copy_ms": round(t_c * 1e3, 4), "copy_tb_per_s": round(2 * nbytes / t_c / 1e12, 3),
                     "host_reduce_s": round(host_s, 2), "equal_to_host": same, "positions": int(Pg),
                     "batch_at_cap": calc_batch(Pg, S, nblk, N), "slices_ms": round(t_sl * 1e3, 4),
                     "search_ms_per_region": {"batch_1": round(t_one / n1 * 1e3, 4), "batch_at_cap": round(t_cap / N * 1e3, 4)}}
    print(json.dumps(res), flush=True)


def step1_bench(a):
    """STEP 1 of `-b` on the host and on the device (--step1 gpu): the stages of both, the files compared; then rank + pick at
    genome size against roiSingle.greedyWalk."""
    import torch
    from epilogos_amd import engine, roiSingle
    from epilogos_amd import similaritySearch_max_mean as mm
    from epilogos_amd import similaritySearch_step1 as step1
    engine.require_gpu()
    S, blockSize, windowBins, windowBP = a.states, 5, 125, 25000
    r3 = lambda d: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in d.items()}
    with tempfile.TemporaryDirectory() as d:
        sp = Path(d) / "scores.txt.gz"
        synthetic_scores(sp, a.bins, S)
        host, dev = Path(d) / "host", Path(d) / "dev"
        host.mkdir(), dev.mkdir()
        torch.zeros(1, device="cuda")                 # the context is not part of the first stage
        tm = {}
        t0 = t = time.perf_counter()
        stateScores, inputArr, genome = mm.readScores(sp)
        tm["read_s"] = time.perf_counter() - t; t = time.perf_counter()
        np.savez_compressed(host / "genome_stats", scores=stateScores, coords=inputArr[:, :3])
        tm["genome_stats_write_s"] = time.perf_counter() - t; t = time.perf_counter()
        chrom, start, end, _sc, orig = roiSingle.maxMean(inputArr[:, 0], inputArr[:, 1], inputArr[:, 2], inputArr[:, 3].astype(np.float64),
                                                         windowBins, genome.shape[0] // windowBins)
        tm["pick_s"] = time.perf_counter() - t; t = time.perf_counter()
        roiCoords = np.empty((len(orig), 3), dtype=object)
        roiCoords[:, 0], roiCoords[:, 1], roiCoords[:, 2] = chrom, start, end
        roiCube = np.stack([mm.makeSlice(genome, i, windowBins, blockSize) for i in orig])
        roiCoords, roiCube = mm.removeRegions(roiCoords, roiCube, -1, -1)
        np.savez_compressed(file=host / "simsearch_cube", scores=roiCube / mm.SCALE, coords=roiCoords)
        tm["slices_s"] = time.perf_counter() - t; t = time.perf_counter()
        mm.reduceGenome(host, genome, blockSize)
        tm["reduce_s"] = time.perf_counter() - t
        tm["total_s"] = time.perf_counter() - t0
        print(json.dumps(dict({"tool": "simsearch_bench", "mode": "step1", "path": "host", "bins": a.bins, "states": S,
                               "regions": int(len(roiCoords))}, **r3(tm))), flush=True)
        del stateScores, inputArr, genome, roiCube

        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            step1.main(dev, sp, windowBins, blockSize, windowBP, -1, -1)          # warm-up (code objects, sort configuration)
            tm = {}
            t0 = time.perf_counter()
            step1.main(dev, sp, windowBins, blockSize, windowBP, -1, -1, timings=tm)
            tm["total_s"] = time.perf_counter() - t0
        for f in ("genome_stats.npz", "simsearch_cube.npz"):
            x, y = np.load(host / f, allow_pickle=True), np.load(dev / f, allow_pickle=True)
            if not (x["scores"].tobytes() == y["scores"].tobytes() and x["coords"].shape == y["coords"].shape and (x["coords"] == y["coords"]).all()):
                sys.exit("simsearch_bench: the host's and the device's %s differ: no timing of a wrong result" % f)
        if (host / "reduced_genome.npy").read_bytes() != (dev / "reduced_genome.npy").read_bytes():
            sys.exit("simsearch_bench: the host's and the device's reduced_genome.npy differ: no timing of a wrong result")
        print(json.dumps(dict({"tool": "simsearch_bench", "mode": "step1", "path": "gpu", "bins": a.bins, "states": S,
                               "files_equal_to_host": True}, **r3(tm))), flush=True)

    # rank + pick alone at genome size: keys made in memory, one plateau of 90 000 windows tied on all three
    n, W, plateau = a.genome_bins, windowBins, 90000
    rng = np.random.default_rng(3)
    rmax = rng.integers(0, 40000, size=n) / 16.0                  # a few thousand equal maxima each: the means decide
    rmean, sc = rng.random(n), rng.random(n)
    p0 = n // 3
    rmax[p0:p0 + plateau], rmean[p0:p0 + plateau], sc[p0:p0 + plateau] = 2600.0, 0.5, 0.5      # the best windows of all
    maxRegions = n // W
    t = time.perf_counter()
    want = roiSingle.greedyWalk(sc, rmean, rmax, W, maxRegions)
    host_s = time.perf_counter() - t
    k = [torch.from_numpy(v).cuda() for v in (rmax, rmean, sc)]
    step1.pickWindows(step1.rankWindows(*[v[:100000] for v in k]), W, 100)        # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    rank = step1.rankWindows(*k)
    torch.cuda.synchronize()
    rank_s = time.perf_counter() - t; t = time.perf_counter()
    got, launches = step1.pickWindows(rank, W, maxRegions)
    pick_s = time.perf_counter() - t
    if not np.array_equal(got, want):
        sys.exit("simsearch_bench: the device's pick and roiSingle.greedyWalk differ at %d windows: no timing of a wrong result" % n)
    print(json.dumps({"tool": "simsearch_bench", "mode": "step1", "path": "rank_pick", "windows": n, "W": W, "plateau": plateau,
                      "maxRegions": maxRegions, "picked": int(len(got)), "host_sort_walk_s": round(host_s, 2), "gpu_rank_ms": round(rank_s * 1e3, 2),
                      "gpu_pick_ms": round(pick_s * 1e3, 2), "pick_launches": launches, "equal_to_host": True}), flush=True)


def calc_ranges(g):
    from epilogos_amd import similaritySearch_calc as calc
    return calc.tensor_ranges(g)


def calc_batch(Pg, S, W, R):
    from epilogos_amd import similaritySearch_calc as calc
    return calc.batch_rows(Pg, S, W, R, calc.WS_CAP_BYTES)


def build_bench(a):
    """`similaritySearch_run -b --gpus N` end to end: total and per-STEP wall times, as the command's STEP lines arrive."""
    root = Path(__file__).resolve().parents[1]
    with tempfile.TemporaryDirectory() as d:
        sp = Path(d) / "scores.txt.gz"
        synthetic_scores(sp, a.bins, a.states)
        out = Path(d) / "out"
        cmd = [sys.executable, "-m", "epilogos_amd.similaritySearch_run", "-b", "-s", str(sp), "-o", str(out),
               "--gpus", str(a.gpus)]
        env = dict(os.environ)
        env["PYTHONPATH"] = str(root) + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        marks = {}
        with tempfile.TemporaryFile() as err:
            t0 = time.perf_counter()
            p = subprocess.Popen(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=err, text=True)
            for line in p.stdout:
                for k in ("STEP 1:", "STEP 2:", "STEP 3:"):
                    if line.strip().startswith(k):
                        marks[k[:6]] = time.perf_counter() - t0
            rc = p.wait()
            total = time.perf_counter() - t0
            if rc != 0:
                err.seek(0)
                sys.exit("the build failed (%d):\n%s" % (rc, err.read().decode(errors="replace")[-3000:]))
        rois = len(np.load(out / "simsearch_indices.npy"))
        positions = len(np.load(out / "reduced_genome.npy"))
    s1, s2, s3 = marks["STEP 1"], marks["STEP 2"], marks["STEP 3"]
    res = {"tool": "simsearch_bench", "mode": "build", "gpus": a.gpus, "bins": a.bins, "states": a.states, "rois": rois,
           "positions": positions, "total_s": round(total, 2), "startup_s": round(s1, 2), "step1_s": round(s2 - s1, 2),
           "step2_s": round(s3 - s2, 2), "step3_s": round(total - s3, 2),
           "shared_gpu": bool(os.environ.get("EPILOGOS_DIST_BACKEND"))}
    print(json.dumps(res), flush=True)


def stages(a, B):
    """Kernel device time per ROI by stage, from a child run of this tool (--no-stages: warm-up + reps passes over the ROIs) under
    rocprofv3 --kernel-trace --stats."""
    if shutil.which("rocprofv3") is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__,
               "--positions", str(a.positions), "--states", str(a.states), "--rois", str(a.rois), "--batch", str(B),
               "--reps", str(a.reps), "--no-stages"]
        subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
        tot = {"distance": 0, "sort": 0, "select": 0, "other": 0}
        for f in Path(d).rglob("*kernel_stats.csv"):
            for r in csv.DictReader(open(f)):
                n, ns = r["Name"], int(float(r["TotalDurationNs"]))
                key = ("distance" if "k_simsearch_dist" in n else "select" if "k_simsearch_select" in n
                       else "sort" if ("rocprim" in n or "fillBuffer" in n) else "other")
                tot[key] += ns
    runs = a.rois * (1 + a.reps)
    return {k: round(v / runs / 1e6, 4) for k, v in tot.items()}


if __name__ == "__main__":
    main()
