#!/usr/bin/env python3
"""Timing of the grouped count pass against what it replaces (measurement aid, not the contract bench).  One JSON line.

Three launches in one process, plain allocations, medians of event-timed launches after warm-up, interleaved round by round:
  groups   epg_bin_hist_groups over the whole matrix, two groups of 379 and 342 columns scattered over the row
  whole    epg_bin_hist over the same matrix (what the pass costs with no groups)
  cut      epg_bin_hist_parts over the two matrices cut to the groups' columns (pitch 384 and 352): the count pass without this
           entry point -- after a second parse, upload and resident copy, which are not timed here
usage: groups_bench.py [--bins 15000000] [--rounds 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402
from epilogos_amd import engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bins", type=int, default=15_000_000)
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()

engine.require_gpu()
N, S, R = 833, 18, a.bins
perm = np.random.default_rng(0).permutation(N)
groups = [np.sort(perm[:379]), np.sort(perm[379:379 + 342])]
X = engine.alloc_states(R, N)
bench.generate_shard(torch, X, N, S, 0)
cuts = [engine.select_columns(X, g) for g in groups]
widths = [len(g) for g in groups]
Hc = engine.hist_rows_alloc([R, R], S, X.device)
H1 = torch.empty((R, S), dtype=torch.int16, device="cuda")
c1 = torch.zeros(S, dtype=torch.int64, device="cuda")
c2 = torch.zeros(2 * S, dtype=torch.int64, device="cuda")
engine.group_members(X.device, N, groups)              # (built and cached before the first timed launch)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


runs = {"groups": lambda: engine.bin_hist_groups(X, N, S, groups, counts=c2),
        "whole": lambda: engine.bin_hist(X, N, S, counts=c1, H=H1),
        "cut": lambda: engine.bin_hist_parts(cuts, widths, S, counts=c1, Hs=Hc)}
ms = {k: [] for k in runs}
for rnd in range(a.warmup + a.rounds):
    for k, fn in runs.items():
        t = timed(fn)
        if rnd >= a.warmup:
            ms[k].append(t)
pitch = [c.stride(0) for c in cuts]
bytes_per_bin = {"groups": X.stride(0) + 2 * 2 * S, "whole": X.stride(0) + 2 * S, "cut": sum(pitch) + 2 * 2 * S}
med = {k: statistics.median(v) for k, v in ms.items()}
print(json.dumps({"bins": R, "N": N, "S": S, "group_widths": widths, "cut_pitch": pitch, "rounds": a.rounds,
                  "ms": {k: round(v, 4) for k, v in med.items()},
                  "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                  "bytes_per_bin": bytes_per_bin,
                  "GBps": {k: round(bytes_per_bin[k] * R / med[k] / 1e6, 1) for k in med}}))
