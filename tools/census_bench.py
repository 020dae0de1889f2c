#!/usr/bin/env python3
"""The state census (epg_state_census) against the counts-only count pass on one resident matrix: by default the synthetic chromosome
of tools/prep_bench.py, 1 246 253 bins x 833 biosamples x 18 states drawn from the chr1 state frequencies.  Both kernels are one
streaming read of the matrix, so the counts-only pass (epg_bin_hist with H = NULL) is the yardstick.  Prints ONE JSON line:

  census_ms            median of --reps event-timed calls of epg_state_census (census, other and first_bad) after the warm-up
  bin_hist_counts_ms   the same for epg_bin_hist with H = NULL, in the same process on the same matrix
  torch_census_ms      the S masked sum(0) passes of torch that the kernel replaces (median of 3)
  ratio                census_ms / bin_hist_counts_ms
  census_bytes_per_s, bin_hist_bytes_per_s   matrix bytes (R x ldx) per second of the two medians
  exact                the census equals the torch passes, its column sums equal the count pass's counts
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tools.prep_bench import FREQS  # noqa: E402


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


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
    census = torch.zeros((N, S), dtype=torch.int64, device="cuda")
    other = torch.zeros(N, dtype=torch.int64, device="cuda")
    fb = torch.full((1,), engine.FIRST_BAD_NONE, dtype=torch.int64, device="cuda")
    counts = torch.zeros(S, dtype=torch.int64, device="cuda")
    census_ms = timed(torch, lambda: engine.state_census(X, N, S, census=census, other=other, first_bad=fb), a.reps, a.warmup)
    hist_ms = timed(torch, lambda: engine.bin_hist(X, N, S, want_hist=False, counts=counts), a.reps, a.warmup)
    Xv = X[:, :N]

    def torch_census():
        return torch.stack([(Xv == s).sum(0) for s in range(S)], dim=1)
    torch_ms = timed(torch, torch_census, 3, 1)
    calls = a.reps + a.warmup
    exact = bool(torch.equal(census, torch_census() * calls)) and bool(torch.equal(census.sum(0), counts)) and int(other.sum().item()) == 0 \
        and int(fb.item()) == engine.FIRST_BAD_NONE
    nbytes = X.numel()
    print(json.dumps({"bins": R, "biosamples": N, "states": S, "matrix_bytes": nbytes, "census_ms": round(census_ms, 4),
                      "bin_hist_counts_ms": round(hist_ms, 4), "torch_census_ms": round(torch_ms, 3), "ratio": round(census_ms / hist_ms, 3),
                      "census_bytes_per_s": round(nbytes / census_ms * 1e3), "bin_hist_bytes_per_s": round(nbytes / hist_ms * 1e3),
                      "reps": a.reps, "exact": exact}))


if __name__ == "__main__":
    main()
