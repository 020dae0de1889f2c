"""ChromHMM -printstatebyline calls -> the [bins, biosamples] state matrix, on the GPU (csrc/epg_statebyline.hip,
include/epilogos_statebyline.h), and the binary matrix file `matrix_<chr>.epgm` that `-i` reads directly (helpers.readTable).

What the reference does with `paste | awk` (bin/preprocess_data_ChromHMM.sh): one file per biosample and chromosome, two header
lines, then one state per 200 bp bin; the files of a chromosome side by side are its matrix.

find_calls           the script's selection rule (:34-45): which files make which chromosome's matrix, in which order
build_matrix_device  the files of one chromosome -> int8 [R, ldx] on the device
write_epgm / read_epgm_header / read_epgm   the file format (layout: include/epilogos_statebyline.h)

The parser on the device is strict.  A file it refuses is named in one warning line and parsed on the host in numpy the way
pandas would read it (blanks and '\\r' stripped); what that cannot read raises."""
import fnmatch
import os
import struct
from pathlib import Path

import numpy as np

from . import _abi, _io
from .textBatches import TextBatches, align, first_fields, mark, pointers, put_column, reread_on_host, set_timings

BIN_WIDTH = 200                                                  # the script's awk: (NR-3)*200, (NR-2)*200
MAGIC = b"EPGM1\0\0\0"
HEADER_BYTES = 128
_HEADER = struct.Struct("<8sqqqiiii80s")                         # magic, R, N, pitch, width, lo, hi, 0, chromosome
assert _HEADER.size == HEADER_BYTES
EXT = ".epgm"


# ---- which files ---------------------------------------------------------------------------------------------------------------

def iter_calls(datadir, metadata, chromsizes):
    """(chromosome, [files]) for EVERY chromosome of `chromsizes`, an empty list where the directory holds none of its files."""
    for chrom, files, _names in iter_calls_named(datadir, metadata, chromsizes):
        yield chrom, files


def iter_calls_named(datadir, metadata, chromsizes):
    """iter_calls with the biosample of every file: (chromosome, [files], [biosample names])."""
    datadir = Path(datadir)
    names = sorted(n for n in os.listdir(datadir) if not n.startswith("."))          # (a glob's order; `*` does not match a leading dot)
    biosamples = first_fields(metadata, skip=1)
    for chrom in first_fields(chromsizes):
        files, found = [], []
        for b in biosamples:
            hits = [n for n in names if fnmatch.fnmatchcase(n, "*{}*{}_*.txt*".format(b, chrom))]
            if len(hits) > 1:
                raise ValueError("biosample {} has more than one file for {}: {} and {}".format(
                    b, chrom, datadir / hits[0], datadir / hits[1]))
            if hits:
                files.append(datadir / hits[0])
                found.append(b)
        yield chrom, files, found


def find_calls(datadir, metadata, chromsizes):
    """[(chromosome, [files in metadata order])] of the chromosomes that have files: chromosomes are column 1 of `chromsizes`
    in file order, biosamples column 1 of `metadata` behind its header line, a biosample's file is the one that matches
    `*{biosample}*{chr}_*.txt*`; a biosample without one has no column in that chromosome's matrix; two matches raise."""
    return [(c, f) for c, f in iter_calls(datadir, metadata, chromsizes) if f]


# ---- one file on the host ------------------------------------------------------------------------------------------------------

def header_chromosome(a):
    """The second blank-separated field of the first line of the text (the script's `chr=$2` at NR==1); "" when there is none."""
    nl = np.flatnonzero(a[:65536] == 10)
    first = a[:int(nl[0]) if len(nl) else min(len(a), 65536)].tobytes().decode("latin-1")
    f = first.split()
    return f[1] if len(f) > 1 else ""


def count_rows_text(a):
    """Lines of the text behind the two headers (a last line without '\\n' counts)."""
    if len(a) == 0:
        return 0
    lines = _io.count_newlines(a, 1) + (1 if a[-1] != 10 else 0)
    return max(lines - 2, 0)


def parse_lenient(a, path="<text>"):
    """The column of a text the strict parser refuses, the way pandas would read it: '\\r' and blanks around a value are dropped,
    lines of nothing but blanks are skipped, "+3" and "3.0" are 3.  -> (int8 column of value - 1, lo, hi); raises ValueError."""
    lines = a.tobytes().decode("latin-1").split("\n")
    if len(lines) < 2 or (len(lines) == 2 and lines[1] == ""):
        raise ValueError("{}: fewer than two header lines".format(path))
    body = np.array([l.strip() for l in lines[2:]], dtype=str)
    body = body[body != ""]
    try:
        f = body.astype(np.float64)
    except ValueError as e:
        raise ValueError("{}: a line is not a state ({})".format(path, e)) from None
    v = f.astype(np.int64)
    if len(v) and not (np.array_equal(v, f) and v.min() >= 1 and v.max() <= 127):
        raise ValueError("{}: states must be whole numbers 1..127".format(path))
    return (v - 1).astype(np.int8), (int(v.min()) if len(v) else 0), (int(v.max()) if len(v) else 0)


# ---- the files of a chromosome on the device -----------------------------------------------------------------------------------

def build_matrix_device(files, timings=None, threads=None):
    """files: the state-by-line files of ONE chromosome, one per biosample, in column order.
    -> (X int8 [R, ldx] on the current device with ldx = N rounded up to 16 and -1 in columns >= N, N, chrName, (lo, hi)).
    The host inflates the files through the native reader, `_io.host_budget()` at a time; a batch of files is uploaded at once
    (textBatches.TextBatches), each is parsed into its column of the batch (epg_sbl_parse) and the batch is transposed into X
    (epg_sbl_transpose).  Batch k + 1 is inflated while batch k is on the device.  `timings` (a dict) receives inflate_s (waiting
    for the inflating threads and staging), upload_ms, parse_ms and transpose_ms (HIP events, summed over the batches)."""
    import torch
    from . import engine
    engine.require_gpu()
    files = [Path(f) for f in files]
    if not files:
        raise ValueError("no state-by-line files")
    N = len(files)
    threads = max(1, int(threads or _io.host_budget()))
    batch = int(_abi.call("epg_sbl_constant", 3))
    dev = torch.device("cuda", torch.cuda.current_device())
    ev = {k: [] for k in ("upload", "parse", "transpose")}

    def inspect(k, data):                                        # -> (chromosome of the header, rows: of the first file only)
        return header_chromosome(data), (count_rows_text(data) if k == 0 else None)

    infos = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    info_of = pointers(infos)
    chroms = []
    X = R = col_pitch = cols = col_of = None
    with TextBatches(files, batch, threads, dev, inspect) as batches:
        for b in batches:
            chroms.extend(c for c, _rows in b.facts)
            if R is None:
                R = b.facts[0][1]
                col_pitch = max(align(R, 16), 16)
                X = torch.full((R, align(N, 16)), -1, dtype=torch.int8, device=dev)
                cols = torch.empty((batch, col_pitch), dtype=torch.int8, device=dev)
                col_of = pointers(cols)
            wsb = max(int(_abi.call("epg_sbl_ws_bytes", n)) for n in b.sizes)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            e1 = mark()                                          # (behind the first batch's fill of X, which is not the parser's time)
            for j, text in enumerate(pointers(b.text, b.offsets[:-1])):
                _abi.call("epg_sbl_parse", text, b.sizes[j], col_of[j], R, info_of[b.k0 + j], engine.ptr(ws), wsb, engine.stream())
            e2 = mark()
            _abi.call("epg_sbl_transpose", engine.ptr(cols), b.nb, col_pitch, R, engine.ptr(X), X.shape[1], b.k0, engine.stream())
            e3 = mark()
            b.release()
            ev["upload"].append(b.upload), ev["parse"].append((e1, e2)), ev["transpose"].append((e2, e3))
        inflate_s = batches.inflate_s
    info = infos.cpu().numpy()                                   # the one synchronisation
    set_timings(timings, inflate_s, ev)
    lo, hi = 128, 0
    for k in range(N):
        rows, flo, fhi, bad = (int(v) for v in info[k])
        if bad >= 0:
            col, flo, fhi = reread_on_host(files[k], bad + 1, "a plain state 1..127", lambda a: parse_lenient(a, files[k]))
            rows = len(col)
            if rows == R and rows:
                put_column(X, k, col, col_pitch)
        if rows != R:
            raise ValueError("{} holds {} bins, {} holds {}: the files of a chromosome must have the same number of lines".format(
                files[0], R, files[k], rows))
        if chroms[k] != chroms[0]:
            raise ValueError("{} names chromosome {!r} in its header, {} names {!r}".format(files[0], chroms[0], files[k], chroms[k]))
        if rows:
            lo, hi = min(lo, flo), max(hi, fhi)
    torch.cuda.synchronize()
    return X, N, chroms[0], ((lo, hi) if R else (0, 0))


# ---- the binary matrix file ----------------------------------------------------------------------------------------------------

def write_epgm(path, states, chrom, state_range, width=BIN_WIDTH):
    """states: int8 [R, >= N] host array or tensor whose first N columns are the matrix (N = states.shape[1] unless the
    array is wider: pass states[:, :N]).  Written under a temporary name and renamed, so a reader never sees half a file."""
    a = states.cpu().numpy() if hasattr(states, "cpu") else np.asarray(states)
    if a.dtype != np.int8 or a.ndim != 2:
        raise ValueError("states must be int8 [R, N]")
    name = str(chrom).encode()
    if len(name) > 79 or b"\0" in name or not name:
        raise ValueError("chromosome name {!r} does not fit the header".format(chrom))
    R, N = a.shape
    path = Path(path)
    tmp = path.with_name(path.name + ".tmp%d" % os.getpid())
    with open(tmp, "wb") as fh:
        fh.write(_HEADER.pack(MAGIC, R, N, N, int(width), int(state_range[0]), int(state_range[1]), 0, name))
        np.ascontiguousarray(a).tofile(fh)
    os.replace(tmp, path)
    return path


def is_epgm(path):
    return str(path).endswith(EXT)


def read_epgm_header(path):
    """-> dict(R, N, pitch, width, lo, hi, chrom); EpilogosIOError (with the path) for a wrong magic, a truncated file or a size
    that is not the header's."""
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as fh:
            raw = fh.read(HEADER_BYTES)
    except OSError as e:
        raise _io.EpilogosIOError("{}: {}".format(path, e)) from None
    if len(raw) < HEADER_BYTES or raw[:8] != MAGIC:
        raise _io.EpilogosIOError("{}: not a binary state matrix (no EPGM1 header)".format(path))
    _m, R, N, pitch, width, lo, hi, _z, name = _HEADER.unpack(raw)
    if R < 0 or N < 0 or pitch != N or width <= 0 or N > 0x7fffffff:
        raise _io.EpilogosIOError("{}: bad header (R={} N={} pitch={} width={})".format(path, R, N, pitch, width))
    want = HEADER_BYTES + R * pitch
    if size < want:
        raise _io.EpilogosIOError("{}: truncated: {} bytes, the header promises {}".format(path, size, want))
    if size != want:
        raise _io.EpilogosIOError("{}: {} bytes, the header promises {}".format(path, size, want))
    return {"R": R, "N": N, "pitch": pitch, "width": width, "lo": lo, "hi": hi, "chrom": name.rstrip(b"\0").decode()}


def synth_locations(chrom, lo, hi, width=BIN_WIDTH):
    """The Locations of rows lo .. hi - 1: "chrom\\t{i*width}\\t{(i+1)*width}\\n", no Python work per row."""
    n = max(hi - lo, 0)
    if n == 0:
        return _io.Locations(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    start = np.arange(lo, hi, dtype=np.int64) * width
    name = np.frombuffer(chrom.encode(), dtype=np.uint8)
    digits = len(str(int(hi) * width))

    def field(v):                                                # decimal text, NUL behind it
        return np.ascontiguousarray(v.astype("S%d" % digits)).view(np.uint8).reshape(n, digits)
    tab, nl = np.full((n, 1), 9, dtype=np.uint8), np.full((n, 1), 10, dtype=np.uint8)
    mat = np.concatenate([np.broadcast_to(name, (n, len(name))), tab, field(start), tab, field(start + width), nl], axis=1)
    keep = mat != 0
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return _io.Locations(mat[keep], off)


def read_epgm(path, rows=None, alloc=None, with_range=False, raw=False):
    """helpers.readTable for a .epgm file: rows [lo, hi) out of the memory-mapped body into alloc(R, N) (pad columns -1), values
    above _io.state_limit() as -1, the rows' Locations synthesised.  raw=True hands the file's bytes on AS THEY ARE instead: what
    `epilogos --check-states` and the census command ask for, which report a byte that is no state by its value.  An argument of
    this one read, not a switch: every other read of the process stores what is no state as -1."""
    h = read_epgm_header(path)
    R, N = h["R"], h["N"]
    _io._log_io("read_epgm", path, *((0, -1) if rows is None else rows))
    lo, hi = (0, R) if rows is None else (max(rows[0], 0), min(rows[1], R))
    hi = max(hi, lo)
    n = hi - lo
    body = np.memmap(path, dtype=np.int8, mode="r", offset=HEADER_BYTES, shape=(R, N)) if R * N else np.zeros((R, N), dtype=np.int8)
    out = np.empty((n, N), dtype=np.int8) if alloc is None else alloc(n, N)
    dest = out[:, :N]
    dest[...] = body[lo:hi]
    if not raw:
        limit = _io.state_limit()
        dest[(dest >= limit) | (dest < 0)] = -1                  # (0-based: a value above the limit as written)
    if alloc is not None:
        out[:, N:] = -1
    loc = synth_locations(h["chrom"], lo, hi, h["width"])
    if with_range:
        return out, loc, (h["lo"], h["hi"])
    return out, loc
