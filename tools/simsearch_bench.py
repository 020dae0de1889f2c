#!/usr/bin/env python3
"""Similarity search STEP 2 on a whole-genome-size synthetic input: distance, sort and select times per region of interest.

    python tools/simsearch_bench.py [--positions 3000000] [--states 18] [--rois 512] [--batch 0] [--reps 2]

The reduced genome has --positions rows (a 200-bp genome with the default 25 kb window and block size 5 has about 3 M): a
background class (90 % of the rows) among 40 row classes, plus planted noisy copies of one window; the ROIs are windows of the
genome.  Timed: the bare epg_simsearch calls over all ROIs in batches (`ms_per_roi`), and the product's path,
similaritySearch_calc.simsearch (host bounds, uploads, downloads: what `similaritySearch_run -b` runs as STEP 2,
`simsearch_path_ms_per_roi`).  The split into distance, sort and select (`stages_ms_per_roi`) comes from a child run of this tool
under `rocprofv3 --kernel-trace --stats` (kernel device time: k_simsearch_dist, the rocPRIM sort kernels with their buffer fills,
k_simsearch_select); --no-stages skips it.  Prints one JSON line, with the path's time extrapolated to 20 000 and 120 000 ROIs."""
import argparse
import csv
import ctypes as C
import json
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
    a = ap.parse_args()
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
