#!/usr/bin/env python3
"""The null fit of paired mode with -n, host against device (measurement aid, not the contract bench).  One JSON line.

Synthetic null distances -- signed squares of normals times 0.02, float32, the shape real null distances have (beta about 0.34) --
of M = 1 246 253 (one chromosome) and M = 15 000 000 (a genome) values, T = 101 trials on sub-samples of n = 100 000.  Per size:
  host   roiAndVisualPairwise._fitParams(fit="host") with --cores processes (default 16): wall seconds
  gpu    _fitParams(fit="gpu", seed=1): wall seconds of the whole call after one warm-up call, and its parts: the draw of the
         sub-sample indices on the host (wall), then by device events the upload (values and indices), the fit kernel, the two
         nnlf kernels, and the read-back with the median pick (wall); evaluations per trial and the share of trials that stopped
         at the cap (flag 1); whether the two fits picked parameters whose nnlf over all values differ, and by how much
Then, unless --no-groupings, tools/groupings_bench.py --only paired once without and once with --fit gpu, at this commit, and the
two JSON lines it printed.
usage: fit_bench.py [--sizes 1246253,15000000] [--trials 101] [--sampling 100000] [--cores 16] [--no-host] [--no-groupings]"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=str, default="1246253,15000000")
ap.add_argument("--trials", type=int, default=101)
ap.add_argument("--sampling", type=int, default=100000)
ap.add_argument("--cores", type=int, default=16)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--no-groupings", action="store_true")
ap.add_argument("--groupings-limit", type=int, default=900, help="seconds a groupings_bench run may take")
a = ap.parse_args()


def note(text):
    print("[fit_bench] " + text, file=sys.stderr, flush=True)


def gpu_parts(rv, engine, torch, values, T, n, seed):
    """The steps of _fitParamsGpu, timed one by one."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t0 = time.perf_counter()
    idx = rv.fitIndices(values.size, T, n, seed)
    t_draw = time.perf_counter() - t0
    ev[0].record()
    x = torch.from_numpy(values).cuda()
    idxd = None if idx is None else torch.from_numpy(idx).cuda()
    ev[1].record()
    params, _fval, info = engine.gennorm_fit(x, idxd)
    ev[2].record()
    nnlf = engine.gennorm_nnlf(x, params)
    ev[3].record()
    torch.cuda.synchronize()                                                             # (the read-back's time without the kernels')
    t0 = time.perf_counter()
    info, params, nnlf = info.cpu().numpy(), params.cpu().numpy(), nnlf.cpu().numpy()
    pick = rv.medianTrial(nnlf) if idx is not None else 0
    t_pick = time.perf_counter() - t0
    torch.cuda.synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(3)]
    return {"draw_indices_s": round(t_draw, 4), "upload_ms": round(ms[0], 3), "fit_kernel_ms": round(ms[1], 3), "nnlf_kernels_ms": round(ms[2], 3),
            "readback_and_pick_s": round(t_pick, 4), "evaluations_per_trial": {"min": int(info[:, 0].min()), "mean": round(float(info[:, 0].mean()), 1),
                                                                                 "max": int(info[:, 0].max())},
            "share_flag_1": round(float((info[:, 1] == 1).mean()), 4), "share_flag_2": round(float((info[:, 1] == 2).mean()), 4),
            "picked": [float(v) for v in params[pick]], "picked_nnlf": float(nnlf[pick])}


def main():
    import torch
    from epilogos_amd import engine
    from epilogos_amd import roiAndVisualPairwise as rv
    engine.require_gpu()
    T, n = a.trials, a.sampling
    result = {"trials": T, "sampling": n, "cores": a.cores, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for M in (int(v) for v in a.sizes.split(",")):
        rng = np.random.default_rng(M)
        z = rng.normal(size=M)
        values = (np.sign(z) * z * z * 0.02).astype(np.float32)
        del z
        quies = np.zeros(M, dtype=bool)
        row = {}
        gpu_parts(rv, engine, torch, values, min(T, 2), n, 0)                                # warm-up: code objects, the allocator
        t0 = time.perf_counter()
        params_gpu = rv._fitParams(values, quies, a.cores, T, n, fit="gpu", seed=1)
        row["gpu_wall_s"] = round(time.perf_counter() - t0, 4)
        row["gpu"] = gpu_parts(rv, engine, torch, values, T, n, 1)
        note("M=%d gpu: %.3f s (%s)" % (M, row["gpu_wall_s"], row["gpu"]))
        if not a.no_host:
            t0 = time.perf_counter()
            params_host = rv._fitParams(values, quies, a.cores, T, n)
            row["host_wall_s"] = round(time.perf_counter() - t0, 3)
            row["host_picked"] = [float(v) for v in params_host]
            both = engine.gennorm_nnlf(torch.from_numpy(values).cuda(), torch.tensor([list(params_gpu), list(params_host)], dtype=torch.float64, device="cuda"))
            row["nnlf_gpu_pick_minus_host_pick"] = float(both[0] - both[1])
            row["host_over_gpu"] = round(row["host_wall_s"] / row["gpu_wall_s"], 2)
            note("M=%d host: %.2f s" % (M, row["host_wall_s"]))
        result["sizes"][str(M)] = row
    if not a.no_groupings:
        for fit in ("host", "gpu"):
            cmd = [sys.executable, str(ROOT / "tools" / "groupings_bench.py"), "--only", "paired", "--trials", str(T), "--fit", fit]
            note(" ".join(cmd))
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.groupings_limit, cwd=str(ROOT))
            if res.returncode != 0:
                raise SystemExit("groupings_bench failed:\n" + res.stdout[-2000:] + res.stderr[-2000:])
            result["groupings_paired_fit_" + fit] = json.loads(res.stdout.strip().splitlines()[-1])["paired"]
    print(json.dumps(result))


main()
