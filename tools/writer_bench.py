#!/usr/bin/env python3
"""The score-text writer, host against device (measurement aid, not the contract bench).  One JSON line.

A synthetic chromosome of 1 246 253 bins x 18 states, four float32 arrays: `random` (N(0, 0.3) scores), `zeros` (the
same with 60 % of the values 0), `runs30` (runs of 30 equal rows) and `delta` (the difference of two `zeros`-like arrays, as paired
mode's deltas are).  Per array, in ONE child process:
  gpu    after one warm-up pass, by device events: epgw_format_scores, epgw_bgzf_compress, the device-to-host copy of the stream; the
         text's and the stream's bytes and their ratio; and the wall seconds of engine.scores_text_bgzf + the copy, the whole part
         call as STEP 3 runs it (locations upload and both synchronisations included)
  host   _io.write_scores on --cores threads (default 16) at gzip level 0 (the library's own compressor, the default) and with
         EPILOGOS_BGZF=1 (zlib level 1 in BGZF blocks): wall seconds and file bytes
  and    whether gzip.decompress of the device's stream equals the host file's text.
Then two commands, each with --writer host and --writer gpu at this commit, alternated host, gpu, host, gpu (--rounds 2), every run a
child process with EPILOGOS_TIMING=1: wall seconds of every run, their medians, and the phase table of each writer's last run:
  single  one chromosome (matrix_chr1.epgm, --bins x --columns), single mode, S1
  paired  the 8-line --groupings command of tools/pvals_bench.py (tools/groupings_bench.py --only paired --fit gpu --pvals gpu)
Every step that uses the GPU is a child under its own time limit; the tool stops at the first that fails.
usage: writer_bench.py [--bins 1246253] [--columns 833] [--cores 16] [--rounds 2] [--no-commands]"""
import argparse
import gzip
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

ap = argparse.ArgumentParser()
ap.add_argument("--bins", type=int, default=1_246_253)
ap.add_argument("--states", type=int, default=18)
ap.add_argument("--columns", type=int, default=833)
ap.add_argument("--groupings", type=int, default=8)
ap.add_argument("--cores", type=int, default=16)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--no-commands", action="store_true")
ap.add_argument("--kernels-limit", type=int, default=420, help="seconds the child of the kernel part may take")
ap.add_argument("--child-limit", type=int, default=300, help="seconds one command may take")
ap.add_argument("--workdir", type=str, default=None)
ap.add_argument("--kernels", action="store_true", help="(the child of the kernel part: prints its JSON row)")
a = ap.parse_args()


def note(text):
    print("[writer_bench] " + text, file=sys.stderr, flush=True)


def arrays(R, S):
    rng = np.random.default_rng(8)
    rnd = rng.normal(0.0, 0.3, size=(R, S)).astype(np.float32)
    zeros = rnd.copy()
    zeros[rng.random(size=zeros.shape) < 0.6] = 0.0
    other = rng.normal(0.0, 0.3, size=(R, S)).astype(np.float32)
    other[rng.random(size=other.shape) < 0.6] = 0.0
    return {"random": rnd, "zeros": zeros, "runs30": np.repeat(rnd[::30], 30, axis=0)[:R].copy(), "delta": zeros - other}


def kernels():
    import torch
    from epilogos_amd import _io, engine
    from epilogos_amd.stateByLine import synth_locations
    engine.require_gpu()
    R, S = a.bins, a.states
    loc = synth_locations("chr1", 0, R)
    blob, off = torch.from_numpy(np.ascontiguousarray(loc.blob)).cuda(), torch.from_numpy(np.ascontiguousarray(loc.offsets, dtype=np.int64)).cuda()
    work = Path(tempfile.mkdtemp(prefix="writer_bench_k_", dir=a.workdir))
    rows = {}
    try:
        for name, x in arrays(R, S).items():
            xd = torch.from_numpy(x).cuda()

            def device_pass():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                ev[0].record()
                text, row_off, flags = engine.format_scores(xd, blob, off)
                ev[1].record()
                n = int(row_off[R])                                             # (the one synchronisation between the two calls)
                ev[2].record()
                out, n_out, cflags = engine.bgzf_compress(text, n, row_off, eof=True)
                ev[3].record()
                n_bytes = int(n_out[0])
                ev[4].record()
                host = out[:n_bytes].cpu()
                ev[5].record()
                torch.cuda.synchronize()
                assert int(flags[0]) == 0 and int(cflags[0]) == 0
                return [ev[k].elapsed_time(ev[k + 1]) for k in (0, 2, 4)], n, host.numpy()
            device_pass()                                                       # warm-up: code objects, the allocator
            ms, n_text, stream = device_pass()
            t0 = time.perf_counter()
            got = engine.scores_text_bgzf(loc, xd)
            part = got[0][:got[1]].cpu().numpy()
            wall = time.perf_counter() - t0
            engine.release_text_buffers()
            row = {"format_ms": round(ms[0], 3), "compress_ms": round(ms[1], 3), "download_ms": round(ms[2], 3), "part_call_wall_s": round(wall, 4),
                   "text_bytes": n_text, "gpu_bytes": int(stream.size), "gpu_ratio": round(stream.size / n_text, 4), "part_call_bytes": int(part.size)}
            text = None
            for label, env in (("host_level0", {}), ("host_bgzf", {"EPILOGOS_BGZF": "1"})):
                for k in ("EPILOGOS_BGZF", "EPILOGOS_GZIP_LEVEL"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                p = work / (name + "_" + label + ".txt.gz")
                t0 = time.perf_counter()
                _io.write_scores(p, loc, x, threads=a.cores)
                row[label + "_s"] = round(time.perf_counter() - t0, 4)
                row[label + "_bytes"] = p.stat().st_size
                row[label + "_ratio"] = round(p.stat().st_size / n_text, 4)
                if text is None:
                    text = gzip.decompress(p.read_bytes())
                p.unlink()
            os.environ.pop("EPILOGOS_BGZF", None)
            row["same_text"] = bool(gzip.decompress(stream.tobytes()) == text and len(text) == n_text)
            row["gpu_over_host_level0_bytes"] = round(stream.size / row["host_level0_bytes"], 4)
            note("%s: %s" % (name, row))
            rows[name] = row
            del xd
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(rows))


def child(cmd, limit, env=None):
    """One GPU step under its own time limit -> (wall seconds, its stdout); the tool ends here if it failed."""
    note(" ".join(cmd))
    t0 = time.perf_counter()
    try:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=str(ROOT), env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit("ran longer than %d s: %s" % (limit, " ".join(cmd)))
    wall = time.perf_counter() - t0
    sys.stderr.write("".join(l + "\n" for l in res.stderr.splitlines() if l.startswith("[")))
    if res.returncode != 0 or "ERROR" in res.stdout:
        raise SystemExit("%s failed (%d):\n%s%s" % (" ".join(cmd), res.returncode, res.stdout[-2000:], res.stderr[-2000:]))
    return wall, res.stdout


def phases(out):
    """{label of a [timing] line: seconds summed over the run}."""
    table = {}
    for l in out.splitlines():
        if l.startswith("    [timing] ") and l.rstrip().endswith(" s"):
            label, _, secs = l[len("    [timing] "):].rstrip()[:-2].rpartition(" ")
            try:
                table[label.strip()] = round(table.get(label.strip(), 0.0) + float(secs), 3)
            except ValueError:
                pass
    return table


def spec(cols):
    return ",".join(str(c + 1) for c in cols)


def commands(result):
    from epilogos_amd import stateByLine as sbl
    R, N, S, G = a.bins, a.columns, a.states, a.groupings
    work = Path(tempfile.mkdtemp(prefix="writer_bench_", dir=a.workdir))
    try:
        ind = work / "in"
        ind.mkdir()
        rng = np.random.default_rng(0)
        x = np.empty((R, N), dtype=np.int8)
        for lo in range(0, R, 1 << 17):
            hi = min(R, lo + (1 << 17))
            x[lo:hi] = np.where(rng.random((hi - lo, N), dtype=np.float32) < 0.5, S - 1, rng.integers(0, S, size=(hi - lo, N), dtype=np.int8))
        sbl.write_epgm(ind / "matrix_chr1.epgm", x, "chr1", (1, S))
        del x
        meta = work / "states.tsv"
        meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
        lines = []
        for g in range(G):
            perm = rng.permutation(N)
            na, nb = (int(v) for v in rng.integers(min(40, N // 4), min(400, N // 2) + 1, size=2))
            lines.append("g%02d\t%s\t%s\n" % (g, spec(np.sort(perm[:na]).tolist()), spec(np.sort(perm[na:na + nb]).tolist())))
        gfile = work / "paired.tsv"
        gfile.write_text("".join(lines))
        base = [sys.executable, "-m", "epilogos_amd.run", "-l", "-i", str(ind), "-j", str(meta), "-s", "1", "-f", "t"]
        cases = {"single": [], "paired": ["-m", "paired", "-n", "--null-seed", "1", "-t", "101", "--fit", "gpu", "--pvals", "gpu", "--groupings", str(gfile)]}
        env = dict(os.environ, EPILOGOS_TIMING="1", PYTHONPATH=str(ROOT))
        for case, args in cases.items():
            row = {"host_wall_s": [], "gpu_wall_s": []}
            for rnd in range(a.rounds):
                for w in ("host", "gpu"):
                    out = work / ("out_%s_%s_%d" % (case, w, rnd))
                    wall, text = child(base + args + ["-o", str(out), "--writer", w], a.child_limit, env)
                    row[w + "_wall_s"].append(round(wall, 3))
                    row[w + "_phases_s"] = phases(text)
                    row[w + "_text_bytes"] = sum(p.stat().st_size for p in out.rglob("*.txt.gz") if p.name.startswith(("scores_", "pairwiseDelta_")))
                    shutil.rmtree(out, ignore_errors=True)
                    note("%s --writer %s: %.2f s" % (case, w, wall))
            for w in ("host", "gpu"):
                row[w + "_median_s"] = round(float(np.median(row[w + "_wall_s"])), 3)
            row["host_over_gpu"] = round(row["host_median_s"] / row["gpu_median_s"], 3)
            result[case] = row
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    if a.kernels:
        return kernels()
    result = {"bins": a.bins, "states": a.states, "columns": a.columns, "cores": a.cores, "rounds": a.rounds}
    _wall, out = child([sys.executable, str(Path(__file__).resolve()), "--kernels", "--bins", str(a.bins), "--states", str(a.states), "--cores", str(a.cores)]
                       + (["--workdir", a.workdir] if a.workdir else []), a.kernels_limit)
    result["arrays"] = json.loads(out.strip().splitlines()[-1])
    if not a.no_commands:
        commands(result)
    print(json.dumps(result))


main()
