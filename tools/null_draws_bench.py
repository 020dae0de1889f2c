#!/usr/bin/env python3
"""Timing of K null draws per bin (--null-draws K; measurement aid, not the contract bench).  One JSON line.

Paired S1 on 379 + 342 biosamples, 18 states, one part; medians of event-timed runs after warm-up, interleaved round by round:
  fused   epg_null_dist_draws_parts: K draws of every bin in one launch, one float per bin and draw
  loop    K x (epg_null_hist_from_binhist_parts, epg_pair_scores_s1_parts): the same null distances by the calls a one-draw
          run makes -- what K draws cost without the kernel
  exceed  epg_null_exceed (keys, radix sort, count) over one chunk of draws as the session sizes it (buffers under 2 GiB)
usage: null_draws_bench.py [--bins 15000000] [--draws 16] [--rounds 10] [--warmup 2]"""
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
from epilogos_amd.helpers import null_draw_seeds  # noqa: E402
from epilogos_amd.scores import s1ScoreTable  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bins", type=int, default=15_000_000)
ap.add_argument("--draws", type=int, default=16)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()

engine.require_gpu()
NA, NB, S, R, K = 379, 342, 18, a.bins, a.draws
XA, XB = engine.alloc_states(R, NA), engine.alloc_states(R, NB)
bench.generate_shard(torch, XA, NA, S, 0)
bench.generate_shard(torch, XB, NB, S, 0, seed=4321)
counts = engine.zeros_counts(S)
(HA, HB), _ = engine.bin_hist_parts([XA, XB], [NA, NB], S, counts=counts)
del XA, XB
q = (counts.double() / counts.sum()).float().cpu().numpy()
TA, TB = (torch.from_numpy(s1ScoreTable(q, n)[1]).cuda() for n in (NA, NB))
seeds = null_draw_seeds(20240229, K)
out = torch.empty((K, R), dtype=torch.float32, device="cuda")
# a chunk of draws as the paired session sizes it
per = K
while per > 1 and 4 * per * R + engine.null_exceed_ws_bytes(per * R) > 2 << 30:
    per -= 1
ws = torch.empty(engine.null_exceed_ws_bytes(per * R), dtype=torch.uint8, device="cuda")
exceed = torch.zeros(R, dtype=torch.int64, device="cuda")
last = {}


def fused():
    engine.null_dist_draws_parts([HA], [HB], [0], S, NA, NB, NA, NB, TA, TB, seeds, outs=[out])


def loop():
    for s in seeds:
        OA, OB = engine.null_hist_from_binhist_parts([HA], [HB], NA + NB, S, NA, NB, int(s), [0])
        last["r"] = engine.pair_scores_s1_parts([(HA, HB, OA[0], OB[0])], S, NA, NB, NA, NB, TA, TB, TA, TB)[0]


def count():
    engine.null_exceed(out[:per].reshape(-1), last["r"]["rdist"], exceed, ws=ws)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


runs = {"loop": loop, "fused": fused, "exceed": count}
ms = {k: [] for k in runs}
for rnd in range(a.warmup + a.rounds):
    for k, fn in runs.items():
        t = timed(fn)
        if rnd >= a.warmup:
            ms[k].append(t)
same = bool(torch.equal(out[K - 1].view(torch.int32), last["r"]["null"].view(torch.int32)))     # the last seed's null, bit for bit
med = {k: statistics.median(v) for k, v in ms.items()}
print(json.dumps({"bins": R, "NA": NA, "NB": NB, "S": S, "draws": K, "rounds": a.rounds, "draws_per_chunk": per,
                  "ms": {k: round(v, 3) for k, v in med.items()},
                  "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                  "ms_per_draw": {"loop": round(med["loop"] / K, 4), "fused": round(med["fused"] / K, 4),
                                  "exceed": round(med["exceed"] / per, 4)},
                  "fused_over_loop": round(med["fused"] / med["loop"], 4), "fused_equals_loop": same}))
