#!/usr/bin/env python3
"""Per-stage times of the state-by-line preprocessing (epilogos_amd/stateByLine.py) on a synthetic chromosome: by default
1 246 253 bins x 833 biosamples (chr1 of the 833-biosample hg19 set), states drawn from the chr1 state frequencies.
Prints ONE JSON line:

  inflate_s          wall time the pipeline waited for the inflating threads and the staging copies
  upload_ms          HIP events around the host-to-device copies of the batches, summed
  parse_ms           ... around the epg_sbl_parse calls
  transpose_ms       ... around the epg_sbl_transpose calls
  build_s            wall time of build_matrix_device as a whole (the four above overlap inside it)
  download_write_s   the matrix to the host and into matrix_<chr>.epgm
  total_s            build_s + download_write_s

`--segments` writes the same chromosome as ChromHMM segment files (one line per run of equal states: runs of about 30 bins on
average, a fifth of them single bins, three runs of 100 000 bins) and times epilogos_amd/segments.py instead; the line then has
expand_ms (HIP events around the epg_seg_expand calls) and expand_col_bytes_per_s (column bytes written per second of it) as well.

`--distinct K` call files are written (gzip, K different columns) and the list of `--biosamples` files cycles through them: every
file is inflated, uploaded and parsed for itself, only the synthesis is shared.  The reference's shell script is not run here."""
import argparse
import gzip
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

FREQS = np.array([.00570, .00293, .00430, .00212, .03260, .10464, .00154, .00057, .01001, .00416, .01554, .00618,
                  .02498, .00262, .00140, .01412, .05563, .71097])


def write_segments(path, rng, bins):
    """One synthetic segment file of chr1: run lengths 1 with probability 0.2, else geometric, 30 bins on average; three runs of
    100 000 bins among them; states from FREQS, no two neighbours equal."""
    n = bins // 15
    lengths = np.where(rng.random(n) < 0.2, 1, rng.geometric(1.0 / 28.2, size=n))
    lengths[rng.choice(n, size=3, replace=False)] = 100000
    ends = np.cumsum(lengths)
    last = int(np.searchsorted(ends, bins))                      # the run that reaches the chromosome's last bin
    ends = ends[:last + 1]
    ends[-1] = bins
    states = rng.choice(len(FREQS), size=len(ends), p=FREQS / FREQS.sum())
    same = np.flatnonzero(states[1:] == states[:-1]) + 1
    states[same] = (states[same - 1] + 1 + rng.integers(0, len(FREQS) - 1, size=len(same))) % len(FREQS)
    starts = np.concatenate([[0], ends[:-1]])
    with gzip.open(path, "wb", compresslevel=1) as fh:
        fh.write("".join("chr1\t%d\t%d\tE%d\n" % (s * 200, e * 200, v + 1) for s, e, v in zip(starts.tolist(), ends.tolist(), states.tolist())).encode())
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bins", type=int, default=1246253)
    ap.add_argument("--biosamples", type=int, default=833)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--segments", action="store_true", help="segment files (epilogos_amd/segments.py) instead of state-by-line files")
    ap.add_argument("--repeat", type=int, default=2, help="runs; the last one is reported (the first pays allocations and page-locking)")
    args = ap.parse_args()
    import torch
    from epilogos_amd import _io, segments as seg, stateByLine as sbl
    rng = np.random.default_rng(0)
    table = np.array([b"%d\n" % (s + 1) for s in range(len(FREQS))], dtype=object)
    with tempfile.TemporaryDirectory(prefix="epg_prep_bench_") as tmp:
        tmp = Path(tmp)
        paths = []
        for k in range(min(args.distinct, args.biosamples)):
            if args.segments:
                paths.append(write_segments(tmp / ("B%03d_18_segments.bed.gz" % k), rng, args.bins))
                continue
            col = rng.choice(len(FREQS), size=args.bins, p=FREQS / FREQS.sum())
            p = tmp / ("B%03d_18_chr1_statebyline.txt.gz" % k)
            with gzip.open(p, "wb", compresslevel=1) as fh:
                fh.write(b"B%03d\tchr1\nMaxState E\n" % k + b"".join(table[col].tolist()))
            paths.append(p)
        files = [paths[k % len(paths)] for k in range(args.biosamples)]
        res = {}
        for _ in range(max(1, args.repeat)):
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if args.segments:
                (chrom, (X, state_range)), = seg.build_matrices_device(files, ["chr1"], timings=tm).items()
                N = len(files)
            else:
                X, N, chrom, state_range = sbl.build_matrix_device(files, timings=tm)
            t1 = time.perf_counter()
            sbl.write_epgm(tmp / "matrix_chr1.epgm", X[:, :N].contiguous(), chrom, state_range)
            t2 = time.perf_counter()
            res = {"tool": "prep_bench", "bins": args.bins, "biosamples": N, "host_threads": _io.host_budget(),
                   "call_file_bytes": int(paths[0].stat().st_size), "inflate_s": round(tm["inflate_s"], 4),
                   "upload_ms": round(tm["upload_ms"], 3), "parse_ms": round(tm["parse_ms"], 3), "transpose_ms": round(tm["transpose_ms"], 3),
                   "build_s": round(t1 - t0, 4), "download_write_s": round(t2 - t1, 4), "total_s": round(t2 - t0, 4),
                   "epgm_bytes": int((tmp / "matrix_chr1.epgm").stat().st_size), "device": torch.cuda.get_device_name(0)}
            if args.segments:
                res.update(tool="prep_bench --segments", expand_ms=round(tm["expand_ms"], 3),
                           expand_col_bytes_per_s=round(args.bins * N / (tm["expand_ms"] * 1e-3)) if tm["expand_ms"] else None)
            del X
    print(json.dumps(res))


if __name__ == "__main__":
    main()
