#!/usr/bin/env python3
"""Wall time from ChromHMM output to scores, two ways, on the synthetic chromosome of tools/prep_bench.py (by default 1 246 253 bins
x 833 biosamples x 18 states; `--segments`: the same chromosome as segment files):

  two commands   `epilogos-prep DIR META SIZES -o M/`, then `epilogos -i M/ -s 1`: the matrix is written and read back
  one command    `epilogos --chromhmm DIR --metadata META --chromsizes SIZES -s 1`: the matrix is scored where it was built

and the same pair with an 8-line `--groupings` file.  Every command is a child process of its own, one after another, with
EPILOGOS_TIMING=1; the baseline is the two-command route of this very tree.  Prints ONE JSON line: for `plain` and `groupings`
the walls `two_commands_s` (with `prep_s` and `run_s`) and `one_command_s`, and the phase table of each command (its `[timing]`
lines in seconds; a phase that every grouping goes through is summed over the groupings).  `--distinct K` call files are written
and the 833 names of the directory are links to them, as prep_bench cycles through them: every file is inflated, uploaded and
parsed for itself.  No ratio is a pass criterion: the tool measures."""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from prep_bench import FREQS, write_segments  # noqa: E402


def write_inputs(tmp, bins, biosamples, distinct, segments):
    """-> (directory, metadata, chromsizes) as epilogos-prep takes them."""
    rng = np.random.default_rng(0)
    table = np.array([b"%d\n" % (s + 1) for s in range(len(FREQS))], dtype=object)
    src, d = tmp / "distinct", tmp / "calls"
    src.mkdir()
    d.mkdir()
    paths = []
    for k in range(min(distinct, biosamples)):
        if segments:
            paths.append(write_segments(src / ("D%03d.bed.gz" % k), rng, bins))
            continue
        col = rng.choice(len(FREQS), size=bins, p=FREQS / FREQS.sum())
        p = src / ("D%03d.txt.gz" % k)
        with gzip.open(p, "wb", compresslevel=1) as fh:
            fh.write(b"D%03d\tchr1\nMaxState E\n" % k + b"".join(table[col].tolist()))
        paths.append(p)
    for k in range(biosamples):
        name = "B%03d_18_segments.bed.gz" % k if segments else "B%03d_18_chr1_statebyline.txt.gz" % k
        os.link(paths[k % len(paths)], d / name)
    (tmp / "meta.txt").write_text("id\n" + "".join("B%03d\n" % k for k in range(biosamples)))
    (tmp / "sizes.txt").write_text("chr1\t%d\n" % (bins * 200))
    return d, tmp / "meta.txt", tmp / "sizes.txt"


def timed(cmd, env):
    """A child process to its end -> (wall seconds, {phase: seconds} of its [timing] lines)."""
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, "-m"] + [str(c) for c in cmd], env=env, capture_output=True, text=True, cwd=str(ROOT))
    wall = time.perf_counter() - t0
    print("%8.2f s  %s" % (wall, " ".join(str(c) for c in cmd[:2])), file=sys.stderr, flush=True)
    if res.returncode != 0 or "ERROR" in res.stdout:
        sys.exit("%s failed:\n%s%s" % (" ".join(str(c) for c in cmd), res.stdout, res.stderr))
    phases = {}
    for l in res.stdout.splitlines():                            # "    [timing] label   1.23 s"; a label of every grouping is summed
        f = l.split()
        if len(f) > 3 and f[0] == "[timing]" and f[-1] == "s":
            try:
                phases[" ".join(f[1:-2])] = round(phases.get(" ".join(f[1:-2]), 0.0) + float(f[-2]), 2)
            except ValueError:
                pass
    return round(wall, 3), phases


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bins", type=int, default=1246253)
    ap.add_argument("--biosamples", type=int, default=833)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--segments", action="store_true", help="segment files instead of state-by-line files")
    args = ap.parse_args()
    env = dict(os.environ, PYTHONPATH=str(ROOT), EPILOGOS_TIMING="1")
    with tempfile.TemporaryDirectory(prefix="epg_chromhmm_bench_") as tmp:
        tmp = Path(tmp)
        d, meta, sizes = write_inputs(tmp, args.bins, args.biosamples, args.distinct, args.segments)
        states = tmp / "states.tsv"
        states.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(len(FREQS))))
        groupings = tmp / "groupings.tsv"
        n, eighth = args.biosamples, max(args.biosamples // 8, 1)
        groupings.write_text("".join("g%d\t%d-%d\n" % (k, min(k * eighth + 1, n), n if k == 7 else min((k + 1) * eighth, n)) for k in range(8)))
        seg = ["--segments"] if args.segments else []
        res = {"tool": "chromhmm_run_bench" + (" --segments" if args.segments else ""), "bins": args.bins, "biosamples": n, "states": len(FREQS)}
        for what, extra in (("plain", []), ("groupings", ["--groupings", groupings])):
            run = ["-s", "1", "-j", states, "-f", "t"] + extra
            m = tmp / ("matrices_" + what)
            prep_s, prep_t = timed(["epilogos_amd.preprocess", d, meta, sizes, "-o", m] + seg, env)
            run_s, run_t = timed(["epilogos_amd.run", "-i", m, "-o", tmp / ("two_" + what)] + run, env)
            one_s, one_t = timed(["epilogos_amd.run", "--chromhmm", d, "--metadata", meta, "--chromsizes", sizes, "-o", tmp / ("one_" + what)]
                                 + seg + run, env)
            res[what] = {"two_commands_s": round(prep_s + run_s, 3), "prep_s": prep_s, "run_s": run_s, "one_command_s": one_s,
                         "phases_prep": prep_t, "phases_run": run_t, "phases_one_command": one_t}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
