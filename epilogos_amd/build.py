"""Build libepilogos_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import shutil
import subprocess
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB_DIR = PKG / "_lib"
LIB_PATH = LIB_DIR / "libepilogos_hip.so"
SOURCES = ["epg_abi.hip", "epg_s1.hip", "epg_s2.hip", "epg_s3.hip", "epg_s3_transpose.hip", "epg_s3_gemm.hip", "epg_s3_lanes.hip", "epg_null.hip", "epg_wide.hip", "epg_simsearch.hip",
           "epg_simsearch_prep.hip", "epg_scores_text.hip", "epg_groups.hip", "epg_null_exceed.hip", "epg_statebyline.hip", "epg_segments.hip", "epg_simsearch_pick.hip", "epg_census.hip", "epg_concordance.hip", "epg_gennorm.hip", "epg_pvals.hip", "epg_textout.hip", "epg_bgzf_inflate.hip", "epg_metrics_text.hip"]
# the public headers under include/, each bound by the table of the same key in _abi.HEADERS
PUBLIC_HEADERS = {"core": "epilogos_amd.h", "scores_text": "epilogos_scores_text.h", "groups": "epilogos_groups.h", "nulldraws": "epilogos_nulldraws.h",
                  "statebyline": "epilogos_statebyline.h", "segments": "epilogos_segments.h", "simsearch_pick": "epilogos_simsearch_pick.h",
                  "census": "epilogos_census.h", "concordance": "epilogos_concordance.h", "gennorm": "epilogos_gennorm.h"}
# package-internal entry points: declared next to their kernels, bound by the table of the same key in _abi.INTERNAL (csrc/epg_pvals.h
# says why they are not under include/ yet)
INTERNAL_HEADERS = {"pvals": "epg_pvals.h"}
# the device text writer's entry points (epgw_): package-internal in the same way, bound by _abi.WRITER.  A registry of its own:
# tests/test_pvals_host.py pins INTERNAL_HEADERS to the p-value header alone
WRITER_HEADERS = {"textout": "epg_textout.h"}
# the device BGZF reader's entry points (epgz_): package-internal in the same way, bound by _abi.READER.  Again a registry of its own:
# tests/test_writer_host.py pins WRITER_HEADERS to the text writer's header alone
READER_HEADERS = {"bgzf_inflate": "epg_bgzf_inflate.h"}
# the device metrics writer's entry points (epgm_): package-internal in the same way, bound by _abi.METRICS.  Once more a registry of
# its own: tests/test_inflate_host.py pins READER_HEADERS to the reader's header alone, and the three registries above to their order
METRICS_HEADERS = {"metrics_text": "epg_metrics_text.h"}
HEADERS = [CSRC / "epg_common.h", CSRC / "epg_count.h", CSRC / "epg_paircount.h", CSRC / "epg_parts.h", CSRC / "epg_pairdist.h", CSRC / "epg_text_scan.h", CSRC / "epg_text_rows.h", CSRC / "epg_fmt_f5.h", CSRC / "epg_fmt_e5.h", CSRC / "epg_bgzf_block.h", CSRC / "epg_bgzf_inflate_block.h",
           *[ROOT / "include" / name for name in PUBLIC_HEADERS.values()], *[CSRC / name for name in INTERNAL_HEADERS.values()], *[CSRC / name for name in WRITER_HEADERS.values()], *[CSRC / name for name in READER_HEADERS.values()], *[CSRC / name for name in METRICS_HEADERS.values()]]
ARCH = "gfx950"


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libepilogos_hip.so")
    return exe


def is_stale():
    if not LIB_PATH.exists():
        return True
    t = LIB_PATH.stat().st_mtime
    deps = [CSRC / s for s in SOURCES] + HEADERS
    return any(d.stat().st_mtime > t for d in deps)


IO_LIB_PATH = LIB_DIR / "libepilogos_io.so"
IO_SOURCE = CSRC / "epg_io.cpp"
IO_HEADER = ROOT / "include" / "epilogos_io.h"


def io_is_stale():
    if not IO_LIB_PATH.exists():
        return True
    t = IO_LIB_PATH.stat().st_mtime
    return any(f.stat().st_mtime > t for f in (IO_SOURCE, IO_HEADER, CSRC / "epg_deflate.h", CSRC / "epg_inflate.h", CSRC / "epg_crc32.h"))


def build_io_library(force=False, verbose=False):
    """Host-side native TSV parser / score writer (g++, zlib, pthreads)."""
    if not force and not io_is_stale():
        return IO_LIB_PATH
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("g++ not found: cannot build libepilogos_io.so")
    tmp = LIB_DIR / (IO_LIB_PATH.name + ".tmp.%d" % os.getpid())
    cmd = [cxx, "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + str(ROOT / "include"), str(IO_SOURCE),
           "-lz", "-o", str(tmp)]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("g++ failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, IO_LIB_PATH)
    return IO_LIB_PATH


OBJ_DIR = LIB_DIR / "obj"


def _compile_one(src, obj, extra_flags, verbose):
    cmd = [_hipcc(), "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-c",
           "-I" + str(ROOT / "include"), "-I" + str(CSRC), *extra_flags, str(src), "-o", str(obj)]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s%s" % (src.name, res.stdout, res.stderr))


def build_library(force=False, verbose=False, extra_flags=()):
    """Compile every HIP source into one shared library (one object per source, the stale ones in parallel, then one
    link).  Returns the path.  EPILOGOS_BUILD_EXPERIMENTS=1 in the environment builds with -DEPILOGOS_BUILD_EXPERIMENTS: the
    measurement switches of the kernels (EPG_S3_DBG, EPG_S3_SCORE_DBG, EPG_S3_KC, EPG_S3_AHEAD, EPG_S3_MFMA, EPG_PAIR_WAVES) then
    read the environment; the default library never does."""
    if os.environ.get("EPILOGOS_BUILD_EXPERIMENTS") == "1":
        extra_flags = tuple(extra_flags) + ("-DEPILOGOS_BUILD_EXPERIMENTS",)
    if not force and not is_stale():
        return LIB_PATH
    from concurrent.futures import ThreadPoolExecutor
    OBJ_DIR.mkdir(parents=True, exist_ok=True)
    flag_tag = OBJ_DIR / "flags.txt"
    flags_now = " ".join(extra_flags)
    same_flags = flag_tag.exists() and flag_tag.read_text() == flags_now
    hdr_t = max(h.stat().st_mtime for h in HEADERS)
    todo, objs = [], []
    for s in SOURCES:
        src, obj = CSRC / s, OBJ_DIR / (s + ".o")
        objs.append(obj)
        if force or not same_flags or not obj.exists() or obj.stat().st_mtime < max(src.stat().st_mtime, hdr_t):
            todo.append((src, obj))
    jobs = max(1, min(len(todo), int(os.environ.get("EPILOGOS_BUILD_JOBS", os.cpu_count() or 4))))
    if todo:
        with ThreadPoolExecutor(max_workers=jobs) as pool:
            for f in [pool.submit(_compile_one, src, obj, extra_flags, verbose) for src, obj in todo]:
                f.result()
        flag_tag.write_text(flags_now)
    tmp = LIB_DIR / (LIB_PATH.name + ".tmp.%d" % os.getpid())
    cmd = [_hipcc(), "--offload-arch=" + ARCH, "-fPIC", "-shared", *[str(o) for o in objs], "-o", str(tmp)]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + res.stdout + res.stderr)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
    print(build_io_library(force=True, verbose=True))
