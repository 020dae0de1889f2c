#!/usr/bin/env python3
"""The biosample concordance (epg_concordance) against the only other way to the same numbers: the trace over the state pairs
of hist_s3's [N, N, S, S] co-occurrence counts, on one resident matrix -- by default the synthetic chromosome of
tools/census_bench.py, 1 246 253 bins x 833 biosamples x 18 states drawn from the chr1 state frequencies.  Prints ONE JSON line:

  concordance_ms       median of --reps event-timed calls of epg_concordance (agree and both, workspace given) after the warm-up
  hist_s3_trace_ms     the same for epg_hist_s3 (matrix-core path, workspace given) plus the trace of its counts, same matrix
  ratio                hist_s3_trace_ms / concordance_ms
  pair_words_per_s     N (N + 1) / 2 pairs x ceil(bins / 32) words per second of the concordance median
  exact                agree equals the trace off the diagonal (one fresh call each), both triangles, and the diagonal of agree
                       and of both equals the valid bins of the columns
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tools.census_bench import timed  # noqa: E402
from tools.prep_bench import FREQS  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bins", type=int, default=1246253)
    ap.add_argument("--biosamples", type=int, default=833)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    from epilogos_amd import engine
    engine.require_gpu()
    R, N, S = a.bins, a.biosamples, len(FREQS)
    rng = np.random.default_rng(a.seed)
    lut = torch.from_numpy(rng.choice(S, size=1 << 16, p=FREQS / FREQS.sum()).astype(np.int8)).cuda()
    X = engine.alloc_states(R, N)
    X.fill_(-1)
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    for r0 in range(0, R, 1 << 16):                              # (in slices: the index tensor is eight bytes per cell)
        r1 = min(R, r0 + (1 << 16))
        X[r0:r1, :N] = lut[torch.randint(0, 1 << 16, (r1 - r0, N), device="cuda", generator=gen)]
    agree = torch.zeros((N, N), dtype=torch.int64, device="cuda")
    both = torch.zeros((N, N), dtype=torch.int64, device="cuda")
    ws = torch.empty(engine.concordance_ws_bytes(R, N, S), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(N * N * S * S, dtype=torch.int32, device="cuda")
    ws3 = torch.empty(engine.hist_s3_ws_bytes(R, N, S), dtype=torch.uint8, device="cuda")

    def trace():
        engine.hist_s3(X, N, S, counts=counts, ws=ws3)
        return torch.diagonal(counts.view(N, N, S, S), dim1=2, dim2=3).sum(-1, dtype=torch.int64)
    conc_ms = timed(torch, lambda: engine.concordance(X, N, S, agree=agree, both=both, ws=ws), a.reps, a.warmup)
    trace_ms = timed(torch, trace, a.reps, a.warmup)
    agree.zero_()
    both.zero_()
    counts.zero_()
    engine.concordance(X, N, S, agree=agree, both=both, ws=ws)
    t = trace()
    off = ~torch.eye(N, dtype=torch.bool, device="cuda")
    valid = (X[:, :N] >= 0).sum(0)
    exact = bool(torch.equal(agree[off], t[off])) and bool(torch.equal(agree, agree.T)) and bool(torch.equal(both, both.T)) \
        and bool(torch.equal(torch.diagonal(agree), valid)) and bool(torch.equal(torch.diagonal(both), valid))
    pair_words = N * (N + 1) // 2 * ((R + 31) // 32)
    print(json.dumps({"bins": R, "biosamples": N, "states": S, "matrix_bytes": X.numel(), "concordance_ms": round(conc_ms, 4),
                      "hist_s3_trace_ms": round(trace_ms, 3), "ratio": round(trace_ms / conc_ms, 2),
                      "pair_words_per_s": round(pair_words / conc_ms * 1e3), "workspace_bytes": ws.numel(), "reps": a.reps, "exact": exact}))


if __name__ == "__main__":
    main()
