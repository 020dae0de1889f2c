#!/usr/bin/env python3
"""Wall time of one `epilogos --groupings` run against the G separate `--columns` commands it replaces (measurement aid, not the
contract bench).  One JSON line.

Input: one synthetic chromosome of 1 246 253 bins x 833 biosamples x 18 states (chr1 of hg19 at 200 bp), written once as .epgm,
and G = 8 groupings of random column subsets (single: one subset of 40 .. 400 biosamples; paired: two disjoint ones).  Timed, as
child processes one after another, on the same input at the same commit:
  separate   G commands `epilogos -i DIR --columns SPEC` (paired: `--columns-a / --columns-b -n --null-seed 1`)
  groupings  one command `epilogos -i DIR --groupings FILE` with the same G lines
For each: the wall time from the start of the first child to the exit of the last.  For the groupings run also
`before_first_count_s` and its share of the run's wall time: the time from the child's start to the line EPILOGOS_TIMING=1 prints
at the end of the first grouping's STEP 1 -- imports, device init, the read of the file, its upload and that grouping's count
pass (milliseconds) -- which is the fixed cost the later groupings do not pay again; and the [timing] lines of the run, summed
by phase, which say where the rest went.  Output directories and the input go to a scratch directory that is removed at the end.
usage: groupings_bench.py [--bins 1246253] [--columns 833] [--groupings 8] [--only single|paired] [--trials 101] [--fit host|gpu]
                          [--pvals host|gpu] [--workdir DIR]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from epilogos_amd import stateByLine as sbl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bins", type=int, default=1_246_253)
ap.add_argument("--columns", type=int, default=833)
ap.add_argument("--groupings", type=int, default=8)
ap.add_argument("--only", choices=["single", "paired"], default=None)
ap.add_argument("--trials", type=int, default=101, help="-t of the paired commands (the fits of -n)")
ap.add_argument("--fit", choices=["host", "gpu"], default=None, help="--fit of the paired commands (default: not passed, the host fit)")
ap.add_argument("--pvals", choices=["host", "gpu"], default=None, help="--pvals of the paired commands (default: not passed, the host stage)")
ap.add_argument("--workdir", type=str, default=None)
ap.add_argument("--child-limit", type=int, default=900, help="seconds a child process may take")
a = ap.parse_args()
R, N, S, G = a.bins, a.columns, 18, a.groupings


def note(text):
    print("[groupings_bench] " + text, file=sys.stderr, flush=True)


def spec(cols):
    """Sorted 0-based columns -> a SPEC of 1-based numbers and ranges."""
    out, k = [], 0
    while k < len(cols):
        j = k
        while j + 1 < len(cols) and cols[j + 1] == cols[j] + 1:
            j += 1
        out.append(str(cols[k] + 1) if j == k else "%d-%d" % (cols[k] + 1, cols[j] + 1))
        k = j + 1
    return ",".join(out)


def child(args, out, timing=False):
    """One command -> (wall seconds, [(seconds since its start, line)])."""
    env = dict(os.environ, PYTHONPATH=str(ROOT), PYTHONUNBUFFERED="1")
    if timing:
        env["EPILOGOS_TIMING"] = "1"
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "epilogos_amd.run", "-l"] + args + ["-o", str(out), "-f", "t"]
    t0 = time.perf_counter()
    lines = []
    with subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(ROOT)) as p:
        for line in p.stdout:
            lines.append((time.perf_counter() - t0, line.rstrip("\n")))
            if time.perf_counter() - t0 > a.child_limit:
                p.kill()
                raise SystemExit("a child ran longer than %d s: %s" % (a.child_limit, " ".join(cmd)))
        rc = p.wait()
    wall = time.perf_counter() - t0
    if rc != 0 or any(l.startswith("ERROR") for _t, l in lines):
        raise SystemExit("%s\n%s" % (" ".join(cmd), "\n".join(l for _t, l in lines[-30:])))
    return wall, lines


def phases(lines):
    """{label of a [timing] line: seconds summed over the run}."""
    out = {}
    for _t, l in lines:
        if l.startswith("    [timing] ") and l.rstrip().endswith(" s"):
            label, _, secs = l[len("    [timing] "):].rstrip()[:-2].rpartition(" ")
            try:
                out[label.strip()] = round(out.get(label.strip(), 0.0) + float(secs), 3)
            except ValueError:
                pass
    return out


work = Path(tempfile.mkdtemp(prefix="groupings_bench_", dir=a.workdir))
result = {"bins": R, "N": N, "S": S, "groupings": G, "input": ".epgm", "trials": a.trials, "fit": a.fit or "host"}
try:
    ind = work / "in"
    ind.mkdir()
    rng = np.random.default_rng(0)
    x = np.empty((R, N), dtype=np.int8)
    for lo in range(0, R, 1 << 17):                    # (in slabs: the uniform draw of a slab is 8 B per value for a moment)
        hi = min(R, lo + (1 << 17))
        x[lo:hi] = np.where(rng.random((hi - lo, N), dtype=np.float32) < 0.5, S - 1, rng.integers(0, S, size=(hi - lo, N), dtype=np.int8))
    sbl.write_epgm(ind / "matrix_chr1.epgm", x, "chr1", (1, S))
    del x
    meta = work / "states.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    note("input written: %.2f GB" % ((ind / "matrix_chr1.epgm").stat().st_size / 1e9))
    for mode in ([a.only] if a.only else ["single", "paired"]):
        lines = []
        for g in range(G):
            perm = rng.permutation(N)
            na, nb = (int(v) for v in rng.integers(min(40, N // 4), min(400, N // 2) + 1, size=2))
            groups = [np.sort(perm[:na])] + ([np.sort(perm[na:na + nb])] if mode == "paired" else [])
            lines.append(["g%02d" % g] + [spec(c.tolist()) for c in groups])
        gfile = work / (mode + ".tsv")
        gfile.write_text("".join("\t".join(l) + "\n" for l in lines))
        common = ["-i", str(ind), "-j", str(meta), "-s", "1"] + (["-m", "paired", "-n", "--null-seed", "1", "-t", str(a.trials)] + (["--fit", a.fit] if a.fit else []) + (["--pvals", a.pvals] if a.pvals else [])
                                                       if mode == "paired" else [])
        walls = []
        for l in lines:
            cols = ["--columns", l[1]] if mode == "single" else ["--columns-a", l[1], "--columns-b", l[2]]
            w, _ = child(common + cols, work / ("sep_" + mode) / l[0])
            walls.append(round(w, 3))
            note("%s: separate command %s took %.2f s" % (mode, l[0], w))
        wall_b, out_b = child(common + ["--groupings", str(gfile)], work / ("grp_" + mode), timing=True)
        first = next((t for t, l in out_b if "[timing] parse + upload + expected counts" in l), None)
        starts = [round(t, 3) for t, l in out_b if l.startswith("Grouping ")]
        note("%s: the groupings run took %.2f s" % (mode, wall_b))
        result[mode] = {"separate_wall_s": round(sum(walls), 3), "separate_each_s": walls, "groupings_wall_s": round(wall_b, 3),
                        "speedup": round(sum(walls) / wall_b, 3),
                        "before_first_count_s": None if first is None else round(first, 3),
                        "before_first_count_share": None if first is None else round(first / wall_b, 3),
                        "grouping_starts_s": starts, "groupings_phases_s": phases(out_b)}
finally:
    shutil.rmtree(work, ignore_errors=True)
print(json.dumps(result))
