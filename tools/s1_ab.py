#!/usr/bin/env python3
"""GPU box: bench.py's S1 headline (no extras) under a list of settings, one child process each, several times through the list:
usage: s1_ab.py [--turns 2] [--unplaced] "lib=<file under tools/_ab_libs>,KEY=VALUE,..." ...   ("-" = the in-tree library, no setting).
--unplaced keeps bench.py's jobs with a plain (unplaced) histogram cache, so that every child reports the step and K1 for both
allocations; after the last turn: median and min-max per setting of the step and of K1, genome (placed / plain) and shard."""
import json, os, statistics, subprocess, sys
R = os.environ.get("GRAFT_REPO_ROOT", "/root/repo")
args = sys.argv[1:]
turns, unplaced = 2, False
while args and args[0].startswith("--"):
    a = args.pop(0)
    if a == "--turns":
        turns = int(args.pop(0))
    elif a == "--unplaced":
        unplaced = True
    else:
        sys.exit(__doc__)
seen = {}
for spec in args * turns:
    env = dict(os.environ)
    if spec != "-":
        for kv in spec.split(","):
            k, v = kv.split("=", 1)
            if k == "lib":
                env["EPILOGOS_HIP_LIB"] = R + "/tools/_ab_libs/" + v
            else:
                env[k] = v
    r = subprocess.run([sys.executable, R + "/bench.py", "--full", "--no-cpu-baseline", "--configs", "none", "--dist-variants", "0", "--graph-leg", "0",
                        "--placement-experiment", "1" if unplaced else "0"], env=env, capture_output=True, text=True)
    try:
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        sh = d["s1_paths"]["shard_1875000_bins"]
        un = d["placement"].get("unplaced") or {}
        print("%-30s %.1f Mbins/s  step %.4f ms  K1 %.4f  rest %.4f | shard step %.4f K1 %.4f | placement %s | plain H: step %s K1 %s" % (
            spec, d["value"], d["ms_per_step"], d["kernels_ms"]["k_bin_hist"], d["kernels_ms"]["combine(normalise,table)+score_from_hist"],
            sh["session_ms_per_step"], sh["session_k_bin_hist_ms"], (d["placement"].get("report") or {}).get("whole_matrix_ms"),
            un.get("ms_per_step"), un.get("k_bin_hist_ms")), flush=True)
        row = {"step": d["ms_per_step"], "K1": d["kernels_ms"]["k_bin_hist"], "shard step": sh["session_ms_per_step"], "shard K1": sh["session_k_bin_hist_ms"]}
        if un.get("ms_per_step"):
            row.update({"plain-H step": un["ms_per_step"], "plain-H K1": un["k_bin_hist_ms"]})
        for k, v in row.items():
            seen.setdefault(spec, {}).setdefault(k, []).append(v)
    except Exception as e:
        print(spec, "failed", repr(e), r.stderr[-400:], flush=True)
for spec, rows in seen.items():
    print("%-30s %s" % (spec, "  ".join("%s %.4f (%.4f-%.4f)" % (k, statistics.median(v), min(v), max(v)) for k, v in rows.items())))
