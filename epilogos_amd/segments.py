"""ChromHMM segment files (`<cell>_<n>_segments.bed`: one file per biosample for the whole genome, one line
`chrom TAB start TAB end TAB label` per run of equal states) -> the [bins, biosamples] state matrix of every chromosome, on the GPU
(csrc/epg_segments.hip, include/epilogos_segments.h), for `python -m epilogos_amd.preprocess --segments`.

find_segments         which file is which biosample's (the rule of stateByLine.iter_calls, for one file per biosample)
read_chromsizes       the chromosome table: names in file order, sizes where the file gives them
parse_host            one file on the host, for what the strict device grammar refuses
check_files           the rules across files: the same chromosomes in every file, the same R_c, R_c within the chromosome
build_matrices_device the files -> {chromosome: (X int8 [R_c, ldx] on the device, (lo, hi))}

The parser on the device is strict (the grammar is written out in the header).  A file it refuses is named in one warning line
and parsed on the host, which also takes '\\r\\n', blanks around fields, track / browser / # lines, more than four fields and
labels that are names (--state-names); errors of content raise ValueError with file and line on either path."""
import fnmatch
import os
import re
from pathlib import Path

import numpy as np

from . import _abi, _io
from .stateByLine import BIN_WIDTH
from .textBatches import TextBatches, align, first_fields, mark, offsets_of, pointers, put_column, reread_on_host, set_timings

NAME_BYTES = 80
_LABEL = re.compile(r"^[A-Za-z]?([0-9]{1,3})(_.*)?$", re.S)
_PREFIX = re.compile(r"^[0-9]+_")


# ---- which files ---------------------------------------------------------------------------------------------------------------

def find_segments(datadir, metadata):
    """[files in metadata order]: biosamples are column 1 of `metadata` behind its header line, a biosample's file is the one
    name of `datadir` that matches `*{biosample}*segments.bed*` (no leading dot); a biosample without one has no column; two
    matches raise."""
    return find_segments_named(datadir, metadata)[0]


def find_segments_named(datadir, metadata):
    """find_segments with the biosample of every file: ([files], [biosample names])."""
    datadir = Path(datadir)
    names = sorted(n for n in os.listdir(datadir) if not n.startswith("."))
    files, found = [], []
    for b in first_fields(metadata, skip=1):
        hits = [n for n in names if fnmatch.fnmatchcase(n, "*{}*segments.bed*".format(b))]
        if len(hits) > 1:
            raise ValueError("biosample {} has more than one segment file: {} and {}".format(b, datadir / hits[0], datadir / hits[1]))
        if hits:
            files.append(datadir / hits[0])
            found.append(b)
    return files, found


def read_chromsizes(chromsizes):
    """-> (names in file order, {name: size in bp} for the lines that give one)."""
    names, sizes = [], {}
    with open(chromsizes, "r", newline="\n") as fh:
        for line in fh.read().split("\n"):
            f = line.split("\t")
            first = f[0].split()
            if not first:
                continue
            names.extend(first)
            if len(first) == 1 and len(f) > 1 and f[1].strip().isdigit():
                sizes[first[0]] = int(f[1])
    return names, sizes


def read_state_names(path):
    """--state-names: a state metadata TSV whose header has `one_index` and `short_name` -> {short_name: state 1..127}."""
    with open(path, "r") as fh:
        lines = [l.rstrip("\r\n").split("\t") for l in fh if l.strip()]
    if not lines or "one_index" not in lines[0] or "short_name" not in lines[0]:
        raise ValueError("{}: no header with one_index and short_name columns".format(path))
    i, k = lines[0].index("one_index"), lines[0].index("short_name")
    table = {}
    for n, f in enumerate(lines[1:], 2):
        if len(f) <= max(i, k) or not f[i].strip().isdigit():
            raise ValueError("{}:{}: not a state line".format(path, n))
        table[f[k].strip()] = int(f[i])
    return table


# ---- one file on the host ------------------------------------------------------------------------------------------------------

def _state_of(label, table, where):
    m = _LABEL.match(label)
    if m:
        v = int(m.group(1))
    else:
        v = None
        if table:
            v = table.get(label)
            if v is None:
                v = table.get(_PREFIX.sub("", label, count=1))
        if v is None:
            raise ValueError("{}: the label {!r} is neither a state number nor a name of --state-names".format(where, label))
    if not 1 <= v <= 127:
        raise ValueError("{}: state {} outside 1..127".format(where, v))
    return v


def parse_host(a, path, chroms, width=BIN_WIDTH, state_names=None):
    """The text `a` (uint8 array or bytes) of one segment file, leniently: '\\r' and blanks around fields dropped, empty lines and
    track / browser / # lines skipped, fields behind the fourth ignored, labels that are names looked up in `state_names` (whole,
    or behind a leading `<digits>_`).  -> {chromosome: (int8 column of state - 1, lo, hi)} for the chromosomes of `chroms` the file
    holds.  Errors of content raise ValueError naming `path` and the 1-based line; runs of other chromosomes are skipped."""
    text = bytes(a.tobytes() if hasattr(a, "tobytes") else a).decode("latin-1")
    want = set(chroms)
    out, done = {}, set()
    cur, keep, starts, ends, states, prev_end = None, False, [], [], [], 0

    def close():
        if cur is not None and keep:
            s, e, v = np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64), np.array(states, dtype=np.int64)
            out[cur] = (np.repeat((v - 1).astype(np.int8), e - s), int(v.min()), int(v.max()))

    for no, line in enumerate(text.split("\n"), 1):
        line = line.strip(" \r")
        if not line.strip() or line.startswith(("track", "browser", "#")):
            continue
        where = "{}:{}".format(path, no)
        f = [x.strip() for x in line.split("\t")]
        if len(f) < 4:
            raise ValueError("{}: {} fields, a segment line has chrom, start, end and label".format(where, len(f)))
        chrom = f[0]
        if chrom != cur:
            close()
            if cur is not None:
                done.add(cur)
            if chrom in done and chrom in want:
                raise ValueError("{}: chromosome {} comes in two runs of lines".format(where, chrom))
            cur, keep, starts, ends, states, prev_end = chrom, chrom in want, [], [], [], None
        if not keep:
            continue
        if not (f[1].isdigit() and f[2].isdigit() and f[1].isascii() and f[2].isascii()):
            raise ValueError("{}: start and end must be whole numbers".format(where))
        s, e = int(f[1]), int(f[2])
        if s % width or e % width:
            raise ValueError("{}: {}..{} is off the grid of {} bp bins".format(where, s, e, width))
        if e <= s:
            raise ValueError("{}: end {} is not behind start {}".format(where, e, s))
        if e // width >= 1 << 31:
            raise ValueError("{}: end {} is beyond 2^31 bins".format(where, e))
        if prev_end is None:
            if s != 0:
                raise ValueError("{}: the first segment of {} starts at {}, not at 0".format(where, chrom, s))
        elif s != prev_end:
            raise ValueError("{}: a {} of {} bp: the segment starts at {}, the one before it ends at {}".format(
                where, "gap" if s > prev_end else "overlap", abs(s - prev_end), s, prev_end))
        states.append(_state_of(f[3], state_names, where))
        starts.append(s // width), ends.append(e // width)
        prev_end = e
    close()
    return out


# ---- the rules across files ----------------------------------------------------------------------------------------------------

def check_files(files, chroms, rows, width=BIN_WIDTH, sizes=None):
    """rows[k] = {chromosome: R_c} of the table's chromosomes file k holds.  -> {chromosome: R_c} of the chromosomes the files hold,
    in table order.  Raises ValueError for a chromosome that some files hold and others do not (column k must be the same
    biosample in every matrix), for an R_c that differs between two files and for an R_c beyond ceil(size / width)."""
    out = {}
    for c in chroms:
        have = [k for k in range(len(files)) if c in rows[k]]
        if not have:
            continue
        if len(have) < len(files):
            lack = next(k for k in range(len(files)) if c not in rows[k])
            raise ValueError("chromosome {} is in {} but not in {}: every segment file must hold the same chromosomes".format(
                c, files[have[0]], files[lack]))
        R = rows[have[0]][c]
        for k in have[1:]:
            if rows[k][c] != R:
                raise ValueError("{} holds {} bins of {}, {} holds {}: the files must end a chromosome at the same place".format(
                    files[have[0]], R, c, files[k], rows[k][c]))
        if sizes and c in sizes and R > -(-sizes[c] // width):
            raise ValueError("{} holds {} bins of {}, which is {} bp long: {} bins of {} bp at most".format(
                files[have[0]], R, c, sizes[c], -(-sizes[c] // width), width))
        out[c] = R
    return out


def name_table(chroms):
    """The chromosome table epg_seg_parse takes: uint8 [nchrom, 80], NUL-padded."""
    t = np.zeros((len(chroms), NAME_BYTES), dtype=np.uint8)
    for i, c in enumerate(chroms):
        b = str(c).encode()
        if not b or len(b) >= NAME_BYTES or b"\0" in b:
            raise ValueError("chromosome name {!r} does not fit the table (1..79 bytes)".format(c))
        t[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return t


def count_lines(a):
    if len(a) == 0:
        return 0
    return _io.count_newlines(a, 1) + (1 if a[-1] != 10 else 0)


# ---- the files on the device ---------------------------------------------------------------------------------------------------

def build_matrices_device(files, chroms, width=BIN_WIDTH, sizes=None, state_names=None, timings=None, threads=None):
    """files: one segment file per biosample, in column order; chroms: the chromosome table.
    -> {chromosome: (X int8 [R_c, ldx] on the current device with ldx = N rounded up to 16 and -1 in columns >= N, (lo, hi))} for
    the chromosomes the files hold, in table order.  The host inflates the files `_io.host_budget()` at a time; a batch of up to
    64 texts is uploaded at once (textBatches.TextBatches), each text is parsed (epg_seg_parse), and for every chromosome the
    batch's columns are expanded (epg_seg_expand) and transposed into its resident matrix (epg_sbl_transpose).  R_c comes from
    the first file (one synchronisation); every matrix stays resident until the caller has written it.  `timings` (a dict)
    receives inflate_s, upload_ms, parse_ms, expand_ms and transpose_ms (HIP events, summed over the batches)."""
    import torch
    from . import engine
    engine.require_gpu()
    files = [Path(f) for f in files]
    chroms = list(chroms)
    if not files:
        raise ValueError("no segment files")
    if width <= 0:
        raise ValueError("the bin width must be positive")
    N, nchrom = len(files), len(chroms)
    if nchrom > int(_abi.call("epg_seg_constant", 3)):
        raise ValueError("{} chromosomes, the table holds {} at most".format(nchrom, int(_abi.call("epg_seg_constant", 3))))
    threads = max(1, int(threads or _io.host_budget()))
    batch = int(_abi.call("epg_sbl_constant", 3))
    dev = torch.device("cuda", torch.cuda.current_device())
    names = torch.from_numpy(name_table(chroms)).to(dev) if nchrom else torch.zeros(1, dtype=torch.uint8, device=dev)
    ev = {k: [] for k in ("upload", "parse", "expand", "transpose")}

    def host_file(k, line):
        return reread_on_host(files[k], line, "a strict segment line", lambda a: parse_host(a, files[k], chroms, width, state_names))

    infos = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    runs = torch.zeros((N, max(nchrom, 1), 3), dtype=torch.int64, device=dev)
    caps = []                                                    # the lines of every file, counted on the host
    host_cols = {}                                               # file -> what parse_host gave
    ref = X = cols = col_of = col_pitch = None                   # ref: {chromosome index: R_c} of the first file
    ldx = align(N, 16)
    with TextBatches(files, batch, threads, dev, lambda k, data: count_lines(data)) as batches:
        info_of, runs_of = pointers(infos), pointers(runs)
        for b in batches:
            k0, nb, stream = b.k0, b.nb, engine.stream()
            caps.extend(b.facts)
            loff = offsets_of([max(n, 1) for n in b.facts])       # where every file's lines start in `first` and `state`
            wsb = max(int(_abi.call("epg_seg_ws_bytes", n, nchrom)) for n in b.sizes)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            first = torch.empty(int(loff[-1]), dtype=torch.int32, device=dev)
            state = torch.empty(int(loff[-1]), dtype=torch.int8, device=dev)
            text_of, first_of, state_of = pointers(b.text, b.offsets[:-1]), pointers(first, loff[:-1]), pointers(state, loff[:-1])
            for j in range(nb):
                _abi.call("epg_seg_parse", text_of[j], b.sizes[j], engine.ptr(names), nchrom, int(width), first_of[j], state_of[j], caps[k0 + j],
                          runs_of[k0 + j], info_of[k0 + j], engine.ptr(ws), wsb, stream)
            e2 = mark()
            b.release()
            ev["upload"].append(b.upload), ev["parse"].append((b.upload[1], e2))
            if ref is None:                                      # R_c, to allocate: the one synchronisation before the last
                bad = int(infos[0, 3].item())
                if bad >= 0:
                    host_cols[0] = host_file(0, bad + 1)
                    ref = {i: len(host_cols[0][c][0]) for i, c in enumerate(chroms) if c in host_cols[0]}
                else:
                    r0 = runs[0].cpu().numpy()
                    ref = {i: int(r0[i, 2]) for i in range(nchrom) if r0[i, 1] > 0}
                col_pitch = max(align(max(ref.values(), default=0), 16), 16)
                need = sum(ref.values()) * ldx + batch * col_pitch
                free = torch.cuda.mem_get_info(dev)[0]
                if need > free:
                    raise RuntimeError("the matrices of {} chromosomes and {} biosamples take {:.2f} GB of device memory, {:.2f} GB are free".format(
                        len(ref), N, need / 1e9, free / 1e9))
                X = {i: torch.full((R, ldx), -1, dtype=torch.int8, device=dev) for i, R in ref.items()}
                cols = torch.empty((batch, col_pitch), dtype=torch.int8, device=dev)
                col_of = pointers(cols)
            for i, R in ref.items():
                e3 = mark()
                for j in range(nb):
                    _abi.call("epg_seg_expand", first_of[j], state_of[j], runs_of[k0 + j], i, col_of[j], R, stream)
                e4 = mark()
                _abi.call("epg_sbl_transpose", engine.ptr(cols), nb, col_pitch, R, engine.ptr(X[i]), ldx, k0, stream)
                e5 = mark()
                ev["expand"].append((e3, e4)), ev["transpose"].append((e4, e5))
        inflate_s = batches.inflate_s
    info = infos.cpu().numpy()                                   # the one synchronisation behind the batches
    run = runs.cpu().numpy()
    set_timings(timings, inflate_s, ev)
    rows = []
    for k in range(N):
        lines, _lo, _hi, bad = (int(v) for v in info[k])
        if bad >= 0 and k not in host_cols:
            host_cols[k] = host_file(k, bad + 1)
        if k in host_cols:
            rows.append({c: len(v[0]) for c, v in host_cols[k].items()})
        else:
            if lines != caps[k]:
                raise RuntimeError("{}: {} lines on the device, {} on the host".format(files[k], lines, caps[k]))
            rows.append({c: int(run[k, i, 2]) for i, c in enumerate(chroms) if run[k, i, 1] > 0})
    held = check_files(files, chroms, rows, width, sizes)
    out = {}
    for i, c in enumerate(chroms):
        if c not in held:
            continue
        for k, got in host_cols.items():
            put_column(X[i], k, got[c][0], col_pitch)
        lo, hi = torch.aminmax(X[i][:, :N])                      # every cell is a state of the grammar: the range as written is this + 1
        out[c] = (X[i], (int(lo) + 1, int(hi) + 1))
    torch.cuda.synchronize()
    return out
