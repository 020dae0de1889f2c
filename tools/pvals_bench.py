#!/usr/bin/env python3
"""The p-value stage of paired mode with -n, host against device (measurement aid, not the contract bench).  One JSON line.

Synthetic distances -- signed squares of normals times 0.02, float32 -- of M = 1 246 253 (one chromosome) and M = 15 000 000 (a
genome) values under the parameters DESIGN.md section 13's device fit picked.  Per size, in a child process of its own:
  host   roiAndVisualPairwise.calculatePVals on --cores threads (default 16) and benjaminiHochberg: wall seconds each
  gpu    after one warm-up pass, by device events: the upload of the distances and the parameters, epgf_gennorm_pvals, epgf_bh_adjust
         (sort, tile minima, carry and scatter together: the entry point is one call, its parts are not timed apart); by the host
         clock the download of p, the adjusted p and the flags; and the wall seconds of roiAndVisualPairwise._pvalsGpu, the whole
         device stage as STEP 4 runs it
  and    the largest difference of the device's p from the host's below loc (relative) and above loc (absolute), the number of
         %.5e strings that differ, and whether the device's adjusted p equal the host's benjaminiHochberg of the DEVICE's p bit for bit
Then, unless --no-groupings, tools/groupings_bench.py --only paired --fit gpu once without and once with --pvals gpu, at this
commit, and the two JSON lines it printed.  Every step that uses the GPU is a child under its own time limit; the tool stops at the
first that fails.
usage: pvals_bench.py [--sizes 1246253,15000000] [--cores 16] [--no-groupings]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

PARAMS = (0.34783607404786054, -6.108733046270553e-11, 0.0005049397097227771)

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=str, default="1246253,15000000")
ap.add_argument("--cores", type=int, default=16)
ap.add_argument("--no-groupings", action="store_true")
ap.add_argument("--size-limit", type=int, default=300, help="seconds the child of one size may take")
ap.add_argument("--groupings-limit", type=int, default=600, help="seconds a groupings_bench run may take")
ap.add_argument("--one", type=int, default=None, help="(the child of one size: prints its JSON row)")
a = ap.parse_args()


def note(text):
    print("[pvals_bench] " + text, file=sys.stderr, flush=True)


def one(M):
    import torch
    from epilogos_amd import engine
    from epilogos_amd import roiAndVisualPairwise as rv
    engine.require_gpu()
    z = np.random.default_rng(M).normal(size=M)
    x = (np.sign(z) * z * z * 0.02).astype(np.float32)
    del z
    beta, loc, scale = (np.float64(v) for v in PARAMS)
    row = {}
    t0 = time.perf_counter()
    p_host = rv.calculatePVals(x, beta, loc, scale, threads=a.cores)
    row["host_pvals_s"] = round(time.perf_counter() - t0, 4)
    t0 = time.perf_counter()
    adj_host = rv.benjaminiHochberg(p_host)
    row["host_bh_s"] = round(time.perf_counter() - t0, 4)
    note("M=%d host: p-values %.3f s, BH %.3f s" % (M, row["host_pvals_s"], row["host_bh_s"]))

    def device_pass():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        xd = torch.from_numpy(x).cuda()
        theta = torch.from_numpy(np.array(PARAMS, dtype=np.float64)).cuda()
        ev[1].record()
        p, pflags = engine.gennorm_pvals(xd, theta)
        ev[2].record()
        adj, bflags = engine.bh_adjust(p)
        ev[3].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = p.cpu().numpy(), adj.cpu().numpy(), torch.cat([pflags, bflags]).cpu().numpy()
        t_down = time.perf_counter() - t0
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(3)], t_down, out
    device_pass()                                                               # warm-up: code objects, the allocator
    ms, t_down, (p_dev, adj_dev, flags) = device_pass()
    row["gpu"] = {"upload_ms": round(ms[0], 3), "pvals_kernel_ms": round(ms[1], 3), "bh_ms": round(ms[2], 3), "download_s": round(t_down, 4),
                  "flags": [int(v) for v in flags]}
    t0 = time.perf_counter()
    got = rv._pvalsGpu(x, PARAMS, None)
    row["gpu_wall_s"] = round(time.perf_counter() - t0, 4)
    assert got is not None
    row["host_over_gpu"] = round((row["host_pvals_s"] + row["host_bh_s"]) / row["gpu_wall_s"], 2)
    xd = x.astype(np.float64)
    below, above = xd <= loc, xd > loc
    with np.errstate(all="ignore"):
        rel = np.abs(p_dev[below] - p_host[below]) / p_host[below]
    row["p_max_rel_diff_below_loc"] = float(np.nanmax(rel))
    row["p_max_abs_diff_above_loc"] = float(np.max(np.abs(p_dev[above] - p_host[above])))
    step = max(1, M // 2_000_000)                                               # (formatting 15 M strings twice takes a minute)
    row["p_strings_compared"] = len(range(0, M, step))
    row["p_strings_differ"] = int(sum(("%.5e" % u) != ("%.5e" % v) for u, v in zip(p_dev[::step], p_host[::step])))
    row["adj_equals_host_bh_of_device_p"] = bool(np.array_equal(adj_dev.view(np.uint64), rv.benjaminiHochberg(p_dev).view(np.uint64)))
    row["adj_max_abs_diff_from_host"] = float(np.max(np.abs(adj_dev - adj_host)))
    note("M=%d gpu: %s wall %.3f s" % (M, row["gpu"], row["gpu_wall_s"]))
    print(json.dumps(row))


def child(cmd, limit):
    """One GPU step under its own time limit -> the last line it printed; the tool ends here if it failed."""
    note(" ".join(cmd))
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
        raise SystemExit("ran longer than %d s: %s" % (limit, " ".join(cmd)))
    sys.stderr.write("".join(l + "\n" for l in res.stderr.splitlines() if l.startswith("[")))
    if res.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s%s" % (" ".join(cmd), res.returncode, res.stdout[-2000:], res.stderr[-2000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    if a.one is not None:
        return one(a.one)
    result = {"params": list(PARAMS), "cores": a.cores, "sizes": {}}
    for M in a.sizes.split(","):
        result["sizes"][M] = child([sys.executable, str(Path(__file__).resolve()), "--one", M, "--cores", str(a.cores)], a.size_limit)
    if not a.no_groupings:
        for pvals in ("host", "gpu"):
            cmd = [sys.executable, str(ROOT / "tools" / "groupings_bench.py"), "--only", "paired", "--fit", "gpu", "--pvals", pvals]
            result["groupings_paired_fit_gpu_pvals_" + pvals] = child(cmd, a.groupings_limit)["paired"]
    print(json.dumps(result))


main()
