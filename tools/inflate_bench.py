"""What `--inflate gpu` costs and saves on one GPU: the text of tools/writer_bench.py (1 246 253 bins x 18 states, 221 MB) as BGZF from
the three producers -- the host writer's own DEFLATE, zlib level 6, the device writer -- read by scoresText.read_scores_device with the
host's inflate (the parent commit's path) and with the device's.  Per producer:
    file_bytes, text_bytes, members
    host_inflate_s        _io.Text on --cores threads: the inflate of the host path alone, median of --rounds
    decode_ms, decode_gbps  epgz_bgzf_inflate alone on the resident file (HIP events, the best of --rounds), GB/s of text
    waves_per_cu          members a CU works on at a time: 160 KB of LDS over epgz_inflate_lds_bytes()
    index_s, upload_inflate_ms, newline_index_ms, inflate_s   the device path's timings (read_scores_device's `timings`)
    read_s_host, read_s_gpu   read_scores_device, the two alternated, median of --rounds
The outputs of the two reads are compared and the tool stops if they differ.  Prints one JSON line.
usage: inflate_bench.py [--bins 1246253] [--states 18] [--cores 16] [--rounds 5] [--workdir DIR]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ap = argparse.ArgumentParser()
ap.add_argument("--bins", type=int, default=1_246_253)
ap.add_argument("--states", type=int, default=18)
ap.add_argument("--cores", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--workdir", type=str, default=None)
a = ap.parse_args()


def note(text):
    print("[inflate_bench] " + text, file=sys.stderr, flush=True)


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def main():
    import torch
    from epilogos_amd import _abi, _io, bgzfIndex, engine, scoresText
    from epilogos_amd.stateByLine import synth_locations
    engine.require_gpu()
    os.environ["EPILOGOS_NUM_CORES"] = str(a.cores)
    R, S = a.bins, a.states
    rng = np.random.default_rng(8)
    x = rng.normal(0.0, 0.3, size=(R, S)).astype(np.float32)                   # writer_bench's "random" scores
    loc = synth_locations("chr1", 0, R)
    work = Path(tempfile.mkdtemp(prefix="inflate_bench_", dir=a.workdir))
    result = {"bins": R, "states": S, "cores": a.cores, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    try:
        paths = {}
        for name, env in (("host_own", {"EPILOGOS_BGZF": "1"}), ("zlib6", {"EPILOGOS_BGZF": "1", "EPILOGOS_GZIP_LEVEL": "6"})):
            for k in ("EPILOGOS_BGZF", "EPILOGOS_GZIP_LEVEL"):
                os.environ.pop(k, None)
            os.environ.update(env)
            paths[name] = work / (name + ".txt.gz")
            _io.write_scores(paths[name], loc, x, threads=a.cores)
        for k in ("EPILOGOS_BGZF", "EPILOGOS_GZIP_LEVEL"):
            os.environ.pop(k, None)
        got = engine.scores_text_bgzf(loc, torch.from_numpy(x).cuda(), eof=True)
        paths["device"] = work / "device.txt.gz"
        paths["device"].write_bytes(got[0][:got[1]].cpu().numpy().tobytes())
        engine.release_text_buffers()
        del got
        lds = int(_abi.call("epgz_inflate_lds_bytes"))
        for name, p in paths.items():
            table, total = bgzfIndex.members(p)
            row = {"file_bytes": p.stat().st_size, "text_bytes": int(total), "members": int(len(table)), "lds_bytes": lds, "waves_per_cu": (160 * 1024) // lds}
            t = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                with _io.Text(p, a.cores) as text:
                    n = len(text.data)
                t.append(time.perf_counter() - t0)
                assert n == total
            row["host_inflate_s"] = round(median(t), 4)
            comp = torch.from_numpy(np.fromfile(p, dtype=np.uint8)).cuda()
            dtable = torch.from_numpy(table).cuda()
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
            ms = []
            for _ in range(a.rounds + 1):
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                _o, status, flags = engine.bgzf_inflate(comp, dtable, out=out)
                ev1.record()
                torch.cuda.synchronize()
                assert int(flags[0]) == 0
                ms.append(ev0.elapsed_time(ev1))
            row["decode_ms"] = round(min(ms[1:]), 3)
            row["decode_gbps"] = round(total / (min(ms[1:]) * 1e-3) / 1e9, 3)
            del comp, dtable, out
            scoresText.read_scores_device(p, inflate="gpu")                    # warm-up: code objects, the page-locked buffers' first allocation
            scoresText.read_scores_device(p)
            host_s, gpu_s, tim = [], [], {}
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                h = scoresText.read_scores_device(p)
                torch.cuda.synchronize()
                host_s.append(time.perf_counter() - t0)
                tim = {}
                t0 = time.perf_counter()
                g = scoresText.read_scores_device(p, timings=tim, inflate="gpu")
                torch.cuda.synchronize()
                gpu_s.append(time.perf_counter() - t0)
                if not (torch.equal(h[0], g[0]) and np.array_equal(h[1], g[1]) and np.array_equal(h[2], g[2]) and h[3] == g[3]):
                    sys.exit("inflate_bench: the two reads of %s differ: no timing of a wrong result" % p)
                del h, g
            if "upload_inflate_ms" not in tim:
                sys.exit("inflate_bench: %s was not inflated on the device" % p)
            row["read_s_host"], row["read_s_gpu"] = round(median(host_s), 4), round(median(gpu_s), 4)
            for k in ("index_s", "upload_inflate_ms", "newline_index_ms", "inflate_s", "upload_parse_ms"):
                row[k] = round(float(tim[k]), 4)
            note("%s: %s" % (name, row))
            result[name] = row
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
