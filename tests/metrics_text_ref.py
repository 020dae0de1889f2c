"""What the tests of the device metrics writer (csrc/epg_metrics_text.h) share: synthetic rows of pairwiseMetrics, the host writer's text
of them (the judge: epgio_write_metrics through _io.write_metrics, decompressed), the "%.5e" edge values, and the walk through the
validation order of epgm_format_metrics, which needs the library but no GPU.  A plain module, not a conftest."""
import ctypes
import gzip

import numpy as np

from epilogos_amd import _io

CHROMS = ["1", "chr1", "chrUn_gl000220"]
STATES = ["".join(chr(ord("a") + (i + k) % 26) for i in range(k + 1)) for k in range(20)]        # names of 1 to 20 bytes
SIZES = [0, 1, 255, 256, 257, 4097, 70001]
UP = lambda v: float(np.nextafter(v, 2.0))
DOWN = lambda v: float(np.nextafter(v, -1.0))
_E5 = [0.0, 1.0, 0.5, 0.1, 5e-324, 2.2250738585072014e-308, 1e-99, 9.999996e-100, 1e-100, 9.999995e-5, 0.9999995]
# every edge value of the list, and the doubles just below and above it that are still p-values
E5_EDGES = [v for e in _E5 for v in (e, DOWN(e), UP(e)) if 0.0 <= v <= 1.0 and not (v == 0.0 and np.signbit(v))]
DIST_EDGES = [0.0, -0.0, 1e-7, -1e-7, 2.0 ** 31 - 128, -(2.0 ** 31 - 128)]
FLAG = dict(dist=1, pval=2, state=4, chrom=8, coord=16, cap=32)


def rows(R, seed, with_p=True):
    """-> dict of the row arrays of R rows: every chromosome and state name, coordinates from 0 to 2^40, distances with the edge values
    among them, p-values drawn uniformly, log-uniformly over the whole exponent range and from the edge values."""
    rng = np.random.default_rng(seed)
    ci = np.sort(rng.integers(0, len(CHROMS), size=R)).astype(np.int32)
    start = rng.integers(0, 1 << 28, size=R).astype(np.int64)
    kind = rng.integers(0, 8, size=R)
    start[kind == 0] = rng.integers(0, 1000, size=int((kind == 0).sum()))
    start[kind == 1] = rng.integers(1 << 39, (1 << 40) - 200, size=int((kind == 1).sum()))
    if R:
        start[0] = 0
        start[-1] = (1 << 40) - 200
    dist = (rng.normal(0.0, 3.0, size=R)).astype(np.float32)
    at = rng.permutation(R)[:len(DIST_EDGES)]
    dist[at] = np.array(DIST_EDGES, dtype=np.float32)[:len(at)]
    out = dict(chrom_idx=ci, start=start, end=start + 200, maxdiff=rng.integers(1, len(STATES) + 1, size=R).astype(np.int32), dist=dist,
               pvals=None, mh=None)
    if with_p:
        for key in ("pvals", "mh"):
            p = rng.random(R)
            logu = rng.random(R) < 0.4
            bits = (rng.integers(0, 1023, size=R).astype(np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, size=R).astype(np.uint64)
            p[logu] = bits.view(np.float64)[logu]
            edge = rng.permutation(R)[:len(E5_EDGES)]
            p[edge] = np.array(E5_EDGES)[:len(edge)]
            assert ((p >= 0) & (p <= 1)).all()
            out[key] = p
    return out


def host_text(tmp, r, name="ref.txt.gz"):
    """The decompressed bytes of the host writer's file of the rows r."""
    path = tmp / name
    _io.write_metrics(path, CHROMS, r["chrom_idx"], r["start"], r["end"], STATES, r["maxdiff"], r["dist"], r["pvals"], r["mh"])
    return gzip.decompress(path.read_bytes())


def check_validation_order(lib):
    """epgm_format_metrics refuses what its header lists, in the header's order: the shape, the unsupported size, the pointers in the
    order of the arguments, the alignments, the sizes -- before any HIP call (every pointer here is a made-up address: no call of this
    function gets as far as a launch)."""
    p = ctypes.c_void_p(1 << 20)
    msg, fn = lib.epg_last_error, lib.epgm_format_metrics
    good = [p, p, 3, 10, p, p, p, p, p, 20, 100, p, p, p, p, 5, p, 1000, p, p, p, 1 << 30]
    NAMES = {0: "chrom", 1: "chrom_off", 4: "chrom_idx", 5: "start", 6: "end", 7: "names", 8: "names_off", 11: "maxdiff", 12: "dist", 16: "text",
             17: None, 18: "row_off", 19: "flags", 20: "ws"}

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return fn(*a, None)
    assert lib.epgm_text_bytes_max(10, 14, 20, 1) == 10 * (14 + 20 + 87) and lib.epgm_text_bytes_max(10, 14, 20, 0) == 10 * (14 + 20 + 61)
    assert lib.epgm_text_bytes_max(-1, 1, 1, 0) == -1 and lib.epgm_text_bytes_max(1, 4097, 1, 0) == -1 and lib.epgm_text_bytes_max(1 << 31, 1, 1, 0) == -1
    assert lib.epgm_format_ws_bytes(1 << 31) == -1 and lib.epgm_format_ws_bytes(-1) == -1
    assert lib.epgm_format_ws_bytes(0) % 256 == 0 and lib.epgm_format_ws_bytes(257) >= 257 * 4 + 2 * 8 and lib.epgm_format_ws_bytes(257) % 256 == 0
    # the shape comes before everything
    for k in (2, 3, 9, 10, 15):
        assert call(**{"a%d" % k: -1, "a0": None, "a16": None}) == -1 and b"bad shape" in msg(), k
    # then the unsupported size, before any pointer
    assert call(a15=1 << 31, a0=None, a20=None) == -2 and b"2^31" in msg()
    # then the pointers, in the order of the arguments: with two of them NULL the first one is named
    order = [k for k in sorted(NAMES) if NAMES[k]]
    for i, k in enumerate(order):
        later = order[i + 1] if i + 1 < len(order) else None
        change = {"a%d" % k: None}
        if later is not None:
            change["a%d" % later] = None
        assert call(**change) == -1 and ("%s is NULL" % NAMES[k]).encode() in msg(), NAMES[k]
    # pvals with mh: both or neither, checked between dist and text
    assert call(a13=None) == -1 and b"go together" in msg() and call(a14=None, a16=None) == -1 and b"go together" in msg()
    assert call(a12=None, a13=None) == -1 and b"dist is NULL" in msg()
    assert call(a13=None, a14=None, a20=None) == -1 and b"ws is NULL" in msg()
    bad = ctypes.c_void_p(p.value + 64)
    # then the alignments (text before ws), before the sizes
    assert call(a16=bad, a20=bad, a17=-1) == -1 and b"text is not 256-byte aligned" in msg()
    assert call(a20=bad, a17=-1, a21=0) == -1 and b"ws is not 256-byte aligned" in msg()
    # then the sizes: text_cap before the workspace
    assert call(a17=-1, a21=0) == -1 and b"text_cap" in msg()
    assert call(a21=0) == -4 and b"workspace" in msg()
