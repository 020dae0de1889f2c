"""Genome-wide driver: replaces the reference's per-chromosome SLURM fan-out (run.py:190-279) with a contiguous
bin-range partition across the GPUs of one node and a single all-reduce of the state-count array.

The bins of all input files, concatenated in file order, are split with the reference's own splitRows rule
(helpers.py:116-118): rank g of G owns global bins [g*R//G, (g+1)*R//G).  Pass 1 counts locally, one
all-reduce(SUM) over torch.distributed (backend nccl = RCCL over xGMI on GPUs; gloo in the CPU tests) makes the
counts global, every rank normalises identically, pass 2 scores locally with no further communication.  Integer
sums make the result independent of G and of the reduction order.

Data flow of a rank (the pipeline bench.py times, plus the host ends):
  parser threads (files in parallel, native inflate + parse straight into pinned, row-padded staging buffers)
  -> ONE asynchronous H2D copy per part -> count pass (k_bin_hist ...) whose per-bin histograms (S1/S2) or state matrix
  (S3, paired) STAY in HBM -> all-reduce -> count check + normalise -> score pass from the resident data -> D2H of the
  float32 scores -> native "%.5f" + gzip writer threads.  Host memory holds the parts in flight, not the genome.
Outputs keep the reference's names.  A file that lies inside one rank's range is written by that rank under its final
name; a file cut by a range border is written as gzip members named from the partition plan (file index + first row)
and concatenated by rank 0 (a multi-member gzip file is a valid gzip file).  The arrays STEP 4 needs travel to rank 0
through torch.distributed send/recv, not through the file system."""
import os
import sys
import time
import shutil
from concurrent.futures import ThreadPoolExecutor
from contextlib import closing
from pathlib import Path

import numpy as np

from . import _io
from . import backend as _backend
from .helpers import fileStem, readStates, readTable, splitRows
from .scores import writeScores


def shuffle_key(file_index, row):
    """Philox counter base of a bin in the paired-mode null shuffle: (file ordinal, row in the file) packed as
    file << 40 | row.  The reference's shuffle is unseeded (helpers.py:183), so any key that does not depend on the partition
    will do; this one is known the moment a file has been parsed -- round 3 keyed by the GLOBAL bin index, which the one-rank
    command line only learns after the last file -- and the outputs stay identical for 1, 2, ... N GPUs."""
    return (int(file_index) << 40) + int(row)


def plan_partition(rows_per_file, world):
    """[(file_index, lo, hi)] per rank: rank ranges from splitRows on the concatenated bins, cut at file borders."""
    total = int(sum(rows_per_file))
    starts = np.concatenate([[0], np.cumsum(rows_per_file)]).astype(np.int64)
    plans = []
    for (g_lo, g_hi) in splitRows(total, world):
        parts = []
        for f, n in enumerate(rows_per_file):
            lo, hi = max(g_lo, starts[f]), min(g_hi, starts[f + 1])
            if lo < hi:
                parts.append((f, int(lo - starts[f]), int(hi - starts[f])))
        plans.append(parts)
    return plans


class _Timer:
    """EPILOGOS_TIMING=1 prints the wall time of the driver's phases on rank 0."""

    def __init__(self, rank):
        self.on = rank == 0 and bool(os.environ.get("EPILOGOS_TIMING"))
        self.time = time.perf_counter
        self.t = self.time()

    def lap(self, label):
        if self.on:
            now = self.time()
            print("    [timing] %-34s %7.2f s" % (label, now - self.t), flush=True)
            self.t = now

    def note(self, text):
        if self.on:
            print("    [timing] " + text, flush=True)


_DTYPES = [np.float32, np.uint8, np.int64, np.int32, np.bool_, np.int16, np.int8]


class _Dist:
    """Thin wrapper so that the single-process case needs no process group."""

    def __init__(self):
        import torch.distributed as dist
        self.dist = dist if dist.is_available() and dist.is_initialized() else None
        self.rank = self.dist.get_rank() if self.dist else 0
        self.world = self.dist.get_world_size() if self.dist else 1
        self.comm_device = None
        if self.dist and self.dist.get_backend() == "nccl":         # RCCL moves device tensors only
            import torch
            self.comm_device = torch.device("cuda", torch.cuda.current_device())

    def all_reduce_counts(self, counts, device=None):
        """SUM-all-reduce an integer numpy array (host-array backends; the product backend reduces its device tensor)."""
        if not self.dist:
            return counts
        import torch
        t = torch.from_numpy(np.ascontiguousarray(counts))
        dev = device if device is not None else self.comm_device
        if dev is not None:
            t = t.to(dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return t.cpu().numpy().reshape(counts.shape)

    def all_reduce_tensor(self, t):
        """SUM-all-reduce a tensor in place where it lives (device tensors go over RCCL/xGMI)."""
        if self.dist:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return t

    def barrier(self):
        if self.dist:
            self.dist.barrier()

    def max_ints(self, values):
        """Element-wise maximum of a short list of non-negative integers over the ranks (a rank without files learns the
        column counts this way instead of opening a file)."""
        if not self.dist:
            return [int(v) for v in values]
        import torch
        t = torch.tensor([int(v) for v in values], dtype=torch.int64)
        if self.comm_device is not None:
            t = t.to(self.comm_device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return [int(v) for v in t.cpu().tolist()]

    # point-to-point hand-over of arrays / tensors: a small header (dtype, shape), then the bytes.  Device tensors travel
    # device to device over RCCL; with a host-side backend (gloo) they are staged through the host.
    def send_tensors(self, tensors, dst):
        import torch
        for t in tensors:
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(np.ascontiguousarray(t))
            if t.dim() > 2:
                raise ValueError("send_tensors: at most two dimensions")
            t = t.contiguous()
            np_dtype = np.dtype(str(t.dtype).replace("torch.", "")).type
            shape = list(t.shape) + [1] * (2 - t.dim())
            head = torch.tensor([_DTYPES.index(np_dtype), t.dim()] + shape, dtype=torch.int64)
            self.dist.send(head.to(self.comm_device) if self.comm_device is not None else head, dst)
            if t.numel():
                flat = t.reshape(-1).view(torch.uint8)
                flat = flat.to(self.comm_device) if self.comm_device is not None else flat.cpu()
                self.dist.send(flat, dst)

    def recv_tensors(self, n, src):
        """-> n tensors, on the communicator's device (RCCL) or on the host (gloo)."""
        import torch
        out = []
        for _ in range(n):
            head = torch.zeros(4, dtype=torch.int64, device=self.comm_device)
            self.dist.recv(head, src)
            code, ndim, d0, d1 = (int(v) for v in head.cpu().tolist())
            dtype = getattr(torch, np.dtype(_DTYPES[code]).name)
            shape = (d0, d1)[:ndim]
            nbytes = int(np.prod(shape)) * np.dtype(_DTYPES[code]).itemsize
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.comm_device)
            if nbytes:
                self.dist.recv(buf, src)
            out.append(buf.view(dtype).reshape(shape))
        return out

    def send_arrays(self, arrays, dst):
        self.send_tensors([np.ascontiguousarray(a) for a in arrays], dst)

    def recv_arrays(self, n, src):
        return [t.cpu().numpy() for t in self.recv_tensors(n, src)]


# ---- input side
def _check_range(path, rng, numStates):
    """The reference indexes a numStates-long array with (file value - 1) and dies on anything outside the model
    (expected.py:113 IndexError); a state model smaller than the data must not run to completion here either."""
    lo, hi = rng
    if (lo, hi) != (0, 0) and (lo < 1 or hi > numStates):
        raise ValueError("{}: state values {}..{} are outside the {}-state model (1..{})".format(path, lo, hi, numStates, numStates))


class _Readers:
    """The parser threads of a rank.  jobs: [(path, lo, hi or None)].  Files are inflated and parsed in threads (inflate is
    serial per file, files run in parallel; the native reader releases the GIL); `parts()` yields (ticket = index in jobs, states
    [rows, width], N, Locations) AS THE PARTS COMPLETE.  Destinations come from the session (page-locked staging, the reader with
    the largest file first) -- which need not exist yet when the threads start: a reader asks for its destination only after
    its file's inflate and line count, so the command line starts them BEFORE it imports torch and initialises the GPU (about a
    second of a whole-genome run) and attaches the session later (`attach`).
    Scheduling: one worker per usable core, largest files first.  Round 2 measured the whole genome on 16 cores with 24
    workers and parts handed over in file order: every part waited behind chr1, whose inflate -- the longest job, started
    together with 23 others on 16 cores -- took 7 s instead of 3; the count pass does not care about the order."""

    def __init__(self, jobs, raw=False):
        import threading
        self.jobs = [(Path(p), lo, hi) for p, lo, hi in jobs]
        self.raw = bool(raw)                               # --check-states: .epgm bytes as they are (helpers.readTable raw=True)
        self.sess = None
        self.ready = threading.Event()
        self.failed = False
        self.trace = os.environ.get("EPILOGOS_TIMING") == "2"        # per-part timeline on stderr
        self.t_origin = time.perf_counter()
        # This rank's share of the host (eight ranks that each sized their pools from the whole node ran 120
        # native threads on a 16-core quota -- the cgroup then throttles every process for the rest of each 100 ms period).
        ncores = _io.host_budget()
        self.workers = max(1, min(int(os.environ.get("EPILOGOS_PARSE_WORKERS", ncores)), max(len(self.jobs), 1)))
        self.left = len(self.jobs)
        self.pool = ThreadPoolExecutor(max_workers=self.workers)
        _io.set_reader_plan(min(self.workers, self.left))      # files being read side by side: what the readers share the cores by
        order = sorted(range(len(self.jobs)), key=lambda t: (-self._weight(t), t))
        self.futs = [self.pool.submit(self._read, t) for t in order]

    def _weight(self, ticket):                         # bytes of input behind a job (a row range: unknown share, the whole file)
        try:
            return os.path.getsize(self.jobs[ticket][0])
        except OSError:
            return 0

    def attach(self, sess):
        """The session whose staging buffers the readers parse into (or any object with alloc(ticket) / skip(ticket))."""
        if hasattr(sess, "pool") and all(hi is None for _p, _lo, hi in self.jobs):
            # whole text files: their sizes tell the staging pool how large its buffers will have to become (PinnedPool.hint)
            sess.pool.hint({t: max(self._weight(t), 1) for t in range(len(self.jobs))})
        self.sess = sess
        self.ready.set()

    def abort(self):
        """Give up: wake every reader that waits for a session or a staging buffer, drop the jobs that have not started."""
        self.failed = True
        self.ready.set()
        if self.sess is not None and hasattr(self.sess, "pool"):
            self.sess.pool.abort()
        for f in self.futs:
            f.cancel()

    def _read(self, ticket):
        path, lo, hi = self.jobs[ticket]
        N = [None]
        t_begin = time.perf_counter() - self.t_origin

        def alloc(R, n):                               # called by the native reader once it knows the file's shape
            N[0] = n
            self.ready.wait()
            if self.failed:
                raise RuntimeError("readers aborted")
            a0 = self.sess.alloc(ticket)
            return a0(R, n) if a0 is not None else np.empty((R, n), dtype=np.int8)
        try:
            # native threads per file: 0 = "share" -- every parallel phase of a file takes this rank's budget divided by the
            # files being read at that moment (one thread each while sixteen files inflate side by side, more for the last,
            # largest files).  (With every reader fanning its short parse phases out to all cores next to fifteen inflating
            # threads, a cgroup CPU quota throttles the whole process for the rest of each 100 ms period: phases that take
            # 0.03 s alone took 1 s.)
            arr, loc, rng = readTable(path, None if hi is None else (lo, hi), alloc=alloc, with_range=True, threads=0, raw=self.raw)
        except BaseException:
            if self.sess is not None:
                self.sess.skip(ticket)
            raise
        if self.trace:                                     # (absolute CLOCK_MONOTONIC seconds too: they line up with [epgio])
            print("    [part %2d] %-28s reader %6.2f .. %6.2f s  (%.3f .. %.3f)" % (ticket, Path(path).name[:28], t_begin,
                  time.perf_counter() - self.t_origin, t_begin + self.t_origin, time.perf_counter()), file=sys.stderr, flush=True)
        return ticket, arr, N[0], loc, rng

    def parts(self, numStates):
        from concurrent.futures import as_completed
        try:
            for f in as_completed(self.futs):
                self.left -= 1
                _io.set_reader_plan(min(self.workers, self.left))
                t, arr, N, loc, rng = f.result()
                _check_range(self.jobs[t][0], rng, numStates)
                t_yield = time.perf_counter() - self.t_origin
                yield t, arr, N, loc
                if self.trace:
                    print("    [part %2d] consumed %6.2f .. %6.2f s" % (t, t_yield, time.perf_counter() - self.t_origin), file=sys.stderr, flush=True)
        except BaseException:
            self.abort()
            raise
        finally:
            _io.set_reader_plan(0)
            self.pool.shutdown(wait=True)


_early = None


def start_readers_early(jobs, raw=False):
    """Called by the command line before it imports torch: the rank's readers start on `jobs` now; the stage driver picks them
    up if it arrives at the same job list (`_stream_parts`), else they are aborted and fresh ones start."""
    global _early
    _early = _Readers(jobs, raw)
    return _early


def abort_early_readers():
    global _early
    if _early is not None:
        _early.abort()
        _early = None


def _stream_parts(jobs, sess, numStates, raw=False):
    """-> generator of (ticket, states, N, Locations) in order of completion (see _Readers)."""
    global _early
    jobs = [(Path(p), lo, hi) for p, lo, hi in jobs]
    readers, _early = _early, None
    if readers is not None and (readers.jobs != jobs or readers.raw != bool(raw)):
        readers.abort()
        readers.pool.shutdown(wait=True)
        readers = None
    if readers is None:
        readers = _Readers(jobs, raw)
    readers.attach(sess)
    return readers.parts(numStates)


def _columns_of(path):
    return readStates(file1Path=path, rowsToCalc=(0, 1), verbose=False).shape[1]


def _part_name(kind, fileTag, fi, lo):
    return ".part_{}_{}_f{:04d}_{:012d}.gz".format(kind, fileTag, fi, lo)


def _clean_parts(outputDir, kind, fileTag):
    """Part files of a crashed earlier run with the same tag must not be mistaken for this run's."""
    import re
    pat = re.compile(r"^\.part_{}_{}_f\d{{4}}_\d{{12}}\.gz$".format(re.escape(kind), re.escape(fileTag)))
    for p in outputDir.iterdir():
        if pat.match(p.name):
            p.unlink()


BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def write_bgzf(path, pieces, eof=True):
    """--writer gpu: the ONE place a device-written file is put together.  pieces: BGZF streams WITHOUT an end-of-file block, in row
    order -- byte blobs (what the device compressed) or paths of part files (removed once copied).  eof: the file is complete and
    gets its one end-of-file block; a part file of a range border (eof=False) gets none, because it will be a piece itself.  A file
    without rows is that block alone."""
    with open(path, "wb") as out:
        for piece in pieces:
            if isinstance(piece, (str, os.PathLike)):
                with open(piece, "rb") as src:
                    shutil.copyfileobj(src, out)
                os.unlink(piece)
            else:
                out.write(memoryview(piece))
        if eof:
            out.write(BGZF_EOF)


def _assemble_text(outputDir, kind, final_name, fileTag, fi, owners, rows_fi, writer="host"):
    """Rank 0: a file cut by range borders is the concatenation of its parts' gzip members, in row order, by the exact
    names the plan gives; a file with one owner was written under its final name already.  writer="gpu": the parts are BGZF
    without end-of-file blocks and write_bgzf completes the file."""
    if len(owners) == 1 and owners[0] == (0, rows_fi):
        return
    if writer == "gpu":
        write_bgzf(outputDir / final_name, [outputDir / _part_name(kind, fileTag, fi, lo) for lo, _hi in owners])
        return
    with open(outputDir / final_name, "wb") as out:
        for lo, _hi in owners:
            p = outputDir / _part_name(kind, fileTag, fi, lo)
            with open(p, "rb") as src:
                shutil.copyfileobj(src, out)
            p.unlink()


def _cat(arrs, empty):
    if len(arrs) == 1:
        return arrs[0]                                 # (a file that lies in one rank's range: no copy of its 70 B per bin)
    return np.concatenate(arrs) if arrs else empty


def _cat_locations(locs):
    if len(locs) == 1:
        return locs[0]
    blobs = [np.asarray(l.blob) for l in locs]
    offs, base = [np.zeros(1, dtype=np.int64)], 0
    for l in locs:
        offs.append(np.asarray(l.offsets[1:]) + base)
        base += int(l.offsets[-1])
    return _io.Locations(_cat(blobs, np.zeros(0, dtype=np.uint8)), np.concatenate(offs))


def _gather_parts(d, plans, my_payloads, n_arrays):
    """Rank 0 collects every part's arrays in plan order: {(file, lo): [arrays]}; the other ranks send theirs."""
    if d.rank != 0:
        for payload in my_payloads:
            d.send_arrays(payload, 0)
        return None
    got = {}
    for r, parts in enumerate(plans):
        for k, (fi, lo, hi) in enumerate(parts):
            got[(fi, lo)] = my_payloads[k] if r == 0 else d.recv_arrays(n_arrays, r)
    return got


def _cached_rows(path):
    """Rows of an input file if the --cache-dir side-car of an earlier run knows them (no pass over the file), else None.  A binary
    matrix file (stateByLine.py, .epgm) knows them from its header."""
    from .helpers import _cache_paths, countRows
    from .stateByLine import is_epgm
    if is_epgm(path):
        return countRows(path)
    cache = _cache_paths(path)
    if cache is None or not all(c.exists() for c in cache):
        return None
    return int(np.load(cache[2], mmap_mode="r").shape[0]) - 1


def _assign_files(files, world, sizes=None):
    """Parser rank of every file while the row counts are still unknown.  Inflating and parsing a file is one serial stream
    (plus the count pass over it, which for S3 is the bulk of the job), so what has to be even is the BYTES per rank: longest
    file first, each to the rank with the least so far (LPT) -- hg19's 24 files over 8 ranks: the fullest rank holds 1.04 x the
    mean.  (Round 3 gave every file to the rank whose bin range holds most of it, so that only border pieces changed hands:
    1.40 x the mean at 8 ranks; what changes hands is 36 B per bin for S1 / S2 / paired and one state row for S3 -- device to
    device, a fraction of a second for a genome -- while an unbalanced parse costs seconds.)  Ties go to the rank whose
    estimated bin range holds most of the file, which keeps the small cases -- a file or two per rank -- local."""
    if sizes is None:
        sizes = [max(os.path.getsize(f), 1) for f in files]
    local, share = [0] * len(files), [-1] * len(files)
    for g, parts in enumerate(plan_partition(sizes, world)):
        for fi, lo, hi in parts:
            if hi - lo > share[fi]:
                share[fi], local[fi] = hi - lo, g
    load, owner = [0] * world, [0] * len(files)
    for fi in sorted(range(len(files)), key=lambda k: (-sizes[k], k)):
        least = min(load)
        g = local[fi] if load[local[fi]] == least else load.index(least)
        owner[fi] = g
        load[g] += sizes[fi]
    return owner


def _plan(files, d, tm, files2=None):
    """-> (mode, rows per file or None, jobs [(file index, lo, hi or None)] of this rank, parser rank per file or None).
    "whole":    one rank; whole files, the row counts come out of the parse.
    "ranges":   several ranks and every row count is known from the --cache-dir side-cars: each rank reads exactly its own
                row ranges from the cache; nothing is inflated, nothing changes hands.
    "assigned": several ranks, text inputs.  Every file is inflated and parsed ONCE, by ONE rank (_assign_files), which
                also runs the count pass over it -- the counts are summed over the ranks anyway, whoever owns the bins.
                The row counts are then exchanged (one all-reduce of a vector with an entry per file), the exact bin-range
                partition follows, and what the score pass needs of the rows a rank parsed for another (per-bin histograms
                for S1 / S2 / paired, state rows for S3) is handed over device to device.  (Round 2 let EVERY rank gunzip
                EVERY file just to count its lines before the first byte was parsed: the reference's helpers.py:154
                re-read, one level up.)"""
    F = len(files)
    if d.world == 1:
        return "whole", None, [(fi, 0, None) for fi in range(F)], None
    rows = [_cached_rows(f) for f in files]
    cached = all(r is not None for r in rows) and all(_cached_rows(f) is not None for f in (files2 or []))
    # The two modes run different collective sequences, so the ranks must agree: "ranges" only if EVERY rank sees every
    # side-car (a cache being filled or cleaned by another run, per-rank file-system views) and the same row counts.
    mine = [int(r) for r in rows] if cached else [0] * F
    agree = d.max_ints([0 if cached else 1] + mine + [-r for r in mine])     # max and (negated) min of every row count
    if agree[0] == 0 and agree[1:1 + F] == mine and agree[1 + F:] == [-r for r in mine]:
        return "ranges", rows, plan_partition(rows, d.world)[d.rank], None
    owner = _assign_files(files, d.world)
    return "assigned", None, [(fi, 0, None) for fi in range(F) if owner[fi] == d.rank], owner


def _exchange_rows(d, jobs, locs, F):
    """Row count of every file from the ranks that parsed them: one all-reduce of an int64 vector."""
    vec = np.zeros(F, dtype=np.int64)
    for t, (fi, _lo, _hi) in enumerate(jobs):
        vec[fi] = len(locs[t])
    return [int(v) for v in d.all_reduce_counts(vec)]


def _redistribute(d, sess, plans, owner, mine, starts, widths):
    """"assigned" mode, after the exact plan is known.  mine: {file index: (session part id of the whole file, Locations)}
    of the files this rank parsed.  Walks every part of every rank's range in ONE global order (all ranks run the same
    loop, so each blocking send meets its receive): a part whose parser is its owner becomes a row slice of the resident
    data; otherwise the parser sends what the score pass needs plus the rows' coordinates, and the owner takes them in.
    Returns the session part ids and the Locations of this rank's parts, in plan order."""
    pid_of, loc_of = {}, {}
    for g, parts in enumerate(plans):
        for fi, lo, hi in parts:
            p = owner[fi]
            row0 = shuffle_key(fi, lo)
            if p == g:
                if d.rank == g:
                    pid, loc = mine[fi]
                    part = loc.slice(lo, hi)
                    pid_of[(fi, lo)] = sess.slice_part(pid, lo, hi, row0)
                    loc_of[(fi, lo)] = _io.Locations(np.ascontiguousarray(part.blob), np.ascontiguousarray(part.offsets))
            elif d.rank == p:
                pid, loc = mine[fi]
                part = loc.slice(lo, hi)
                d.send_tensors(list(sess.export_rows(pid, lo, hi)) + [np.ascontiguousarray(part.blob), np.ascontiguousarray(part.offsets)], g)
            elif d.rank == g:
                got = d.recv_tensors(sess.n_export + 2, p)
                pid_of[(fi, lo)] = sess.import_rows(got[:-2], widths, row0)
                loc_of[(fi, lo)] = _io.Locations(got[-2].cpu().numpy(), got[-1].cpu().numpy())
    for pid, _loc in mine.values():                    # the whole-file entries; the slices keep alive what they use
        sess.drop_part(pid)
    my = plans[d.rank]
    return [pid_of[(fi, lo)] for fi, lo, _hi in my], [loc_of[(fi, lo)] for fi, lo, _hi in my]


_deferred = []


def _wait_writes(writer, jobs):
    try:
        for j in jobs:
            j.result()
    finally:
        writer.shutdown(wait=True)


def finish_writes():
    """Wait for the text writers a run with defer_writes=True left running (and re-raise what one of them raised)."""
    while _deferred:
        writer, jobs, tm, label = _deferred.pop()
        _wait_writes(writer, jobs)
        tm.lap(label)


# ---- STEP 1-3, written once for both modes.  Every rank runs the same collectives (barrier, all-reduce, send / recv) in the
# same order, so the sequence lives in _run_groups alone; a mode object supplies only what differs between the modes: its
# inputs and session, how a parsed file becomes a session part, its per-part outputs and rank 0's per-file result.
class _DeviceText:
    """--writer gpu: what a part hands the writer pool -- blob, the file's BGZF bytes from the device (no end-of-file block), or
    None with `array`, the float32 scores downloaded for the host writer, when the device refused a value."""

    def __init__(self, blob, array):
        self.blob, self.array = blob, array


class _Single:
    """One group: a part is one file's rows; scores_* text; rank 0's result per file is (chrName, scores, Locations)."""
    kind, census, upload_note = "scores", "single", ""
    n_payload = 1                                      # arrays of a part that travel to rank 0, besides its Locations

    n_widths = 1                                       # widths the session works with: N
    check_states = False                               # --check-states (set by the run_* functions)

    def __init__(self, files, numStates, saliency, keep_temps, columns=None):
        self.groups, self.S, self.sal, self.keep_temps = (files,), numStates, saliency, keep_temps
        self.columns = None if columns is None else np.ascontiguousarray(columns, dtype=np.int64)   # 0-based: the group IS these columns

    def open(self, be):
        return be.open_single(self.S, self.sal)

    def see_width(self, widths, g, n):
        """A parsed job of file group g has n columns: what that says about the session's widths."""
        widths[0] = max(widths[0], n if self.columns is None or not n else len(self.columns))

    def default_widths(self):
        """The widths when this rank parsed nothing that has one."""
        return [_columns_of(self.groups[0][0]) if self.columns is None else len(self.columns)]

    def add(self, sess, t, arr, n, part):
        """A parsed job (its index t, its states) into the session -> the part's session id (None while it is incomplete)."""
        if self.columns is None:
            return sess.add_part(arr, n, t)
        _check_columns_fit(self.columns, n, self.groups[0][part[0]])
        return sess.add_part(arr, n, t, columns=self.columns)

    def add_resident(self, sess, X, n, part):
        """add() for a job whose matrix is on the device already (run_groupings: uploaded by this or an earlier grouping, or handed
        in by the caller).  No columns: the group is the whole matrix, as in add()."""
        if self.columns is None:
            return sess.add_device(X, n)
        _check_columns_fit(self.columns, n, self.groups[0][part[0]])
        return sess.add_device(X, n, columns=self.columns)

    def part_out(self, sess, pid, loc=None):
        """-> (the array written as text, [the arrays rank 0 collects]) of a part.  loc (the part's Locations; --writer gpu): the
        first is a _DeviceText."""
        if loc is None:
            sc = sess.scores(pid)
            return sc, [sc]
        sc, blob = sess.scores(pid, text=loc)
        return _DeviceText(blob, sc), [sc]

    def result(self, temp, chrName, loc, arrays):
        """Rank 0: a file's entry of the results from its parts' arrays (arrays[i] = array i of every part, in row order)."""
        scoreArr = _cat(arrays[0], np.zeros((0, self.S), dtype=np.float32))
        if self.keep_temps:
            np.savez_compressed(temp("scores"), chrName=np.array([chrName]), scoreArr=scoreArr, locationArr=loc.to_object_array())
        return chrName, scoreArr, loc


class _Paired:
    """Two groups: a part is the same rows of a file of each group; pairwiseDelta_* text; rank 0's result per file is a dict."""
    kind, census, upload_note = "pairwiseDelta", "paired", " x 2 groups"
    n_payload = 4
    n_widths = 2                                       # NA, NB
    check_states = False

    def __init__(self, files1, files2, numStates, saliency, quiescentState, groupSize, nullSeed, keep_temps, nullDraws=1):
        self.groups, self.S, self.sal, self.keep_temps = (files1, files2), numStates, saliency, keep_temps
        self.qstate, self.groupSize, self.seed = quiescentState, groupSize, nullSeed
        self.halves = {}                               # part index -> its group that arrived first
        # --null-draws K > 1: a part also carries its exceedance counts against the pooled null of K draws per bin, and the
        # session knows the pool's size (one rank: the counts are additive over ranks, which nothing adds up yet)
        self.draws, self.pool = int(nullDraws), None
        if self.draws > 1:
            self.n_payload = 5

    def open(self, be):
        if self.draws > 1:
            if _Dist().world > 1:
                raise ValueError("more than one null draw per bin is not available on several ranks")
            return be.open_paired(self.S, self.sal, self.qstate, self.groupSize, self.seed, draws=self.draws)
        return be.open_paired(self.S, self.sal, self.qstate, self.groupSize, self.seed)

    def see_width(self, widths, g, n):
        widths[g] = max(widths[g], n)

    def default_widths(self):
        return [_columns_of(group[0]) for group in self.groups]

    def add(self, sess, t, x, n, part):
        staged = (sess.stage(x, n, t), n, x.shape[0])
        other = self.halves.pop(t // 2, None)          # part k's two groups are jobs 2k and 2k + 1, in HBM as soon as parsed
        if other is None:
            self.halves[t // 2] = staged
            return None
        (XA, nA, rA), (XB, nB, rB) = (other, staged) if t % 2 else (staged, other)
        fi, lo, _hi = part
        if rA != rB:
            raise ValueError("paired inputs differ in length: {} vs {}".format(self.groups[0][fi], self.groups[1][fi]))
        # the key of the part's first row in the null shuffle: (file, row in the file) -- known here in every mode, so the
        # session draws the null groups right behind the count pass (on its second stream)
        return sess.add_staged(XA, nA, XB, nB, shuffle_key(fi, lo))

    def part_out(self, sess, pid, loc=None):
        res = sess.results(pid) if loc is None else sess.results(pid, text=loc)
        arrays = [np.asarray(res["null"], dtype=np.float32), np.asarray(res["quies"], dtype=np.bool_),
                  np.asarray(res["rdist"], dtype=np.float32), np.asarray(res["mdiff"], dtype=np.int32)]
        if self.draws > 1:
            arrays.append(np.asarray(res["exceed"], dtype=np.int64))
            self.pool = int(sess.null_pool)
        return (res["delta"] if loc is None else _DeviceText(res["delta_text"], res["delta"])), arrays

    def result(self, temp, chrName, loc, arrays):
        null, quies, dist, mdiff = (_cat(a, np.zeros(0, dtype=t)).astype(t) for a, t in zip(arrays, (np.float32, bool, np.float32, np.int32)))
        extra = {}
        if self.draws > 1:
            # the pool is the whole run's (every file's bins, K draws each): the same number in every file's entry
            extra = {"nullExceed": _cat(arrays[4], np.zeros(0, dtype=np.int64)).astype(np.int64), "nullPool": int(self.pool or 0)}
            if self.keep_temps:
                np.savez_compressed(temp("nullExceed"), chrName=np.array([chrName]), nullExceed=extra["nullExceed"],
                                    nullPool=np.array([extra["nullPool"]], dtype=np.int64))
        if self.keep_temps:
            np.savez_compressed(temp("nullDistances"), chrName=np.array([chrName]), nullDistances=null)
            np.savez_compressed(temp("quiescence"), chrName=np.array([chrName]), quiescenceArr=quies)
            # side-car for this engine's STEP 4 (roiAndVisualPairwise.readInData): the per-bin reduction the reference redoes
            # from the pairwiseDelta text, already computed on the GPU; removed with the other temps
            starts, ends = loc.start_end()
            np.savez_compressed(temp("pairMetrics"), chrName=np.array([chrName]), distances=dist, maxDiff=mdiff, starts=starts, ends=ends)
        return {"chrName": chrName, "locations": loc, "nullDistances": null, "quiescenceArr": quies, "distances": dist, "maxDiff": mdiff,
                **extra}


class _PairedColumns(_Paired):
    """Two groups that are column groups of ONE set of files: a part is one parsed file -- parsed and uploaded once -- that
    feeds both groups (session add_columns).  Outputs, payloads and rank 0's results are paired mode's."""
    upload_note = ""

    def __init__(self, files, colsA, colsB, numStates, saliency, quiescentState, groupSize, nullSeed, keep_temps, nullDraws=1):
        super().__init__(files, (), numStates, saliency, quiescentState, groupSize, nullSeed, keep_temps, nullDraws)
        self.groups = (files,)
        self.colsA, self.colsB = np.ascontiguousarray(colsA, dtype=np.int64), np.ascontiguousarray(colsB, dtype=np.int64)

    def see_width(self, widths, g, n):
        if n:
            widths[0], widths[1] = len(self.colsA), len(self.colsB)

    def default_widths(self):
        return [len(self.colsA), len(self.colsB)]

    def add(self, sess, t, x, n, part):
        fi, lo, _hi = part
        for cols in (self.colsA, self.colsB):
            _check_columns_fit(cols, n, self.groups[0][fi])
        return sess.add_columns(sess.stage(x, n, t), n, self.colsA, self.colsB, shuffle_key(fi, lo))

    def add_resident(self, sess, X, n, part):
        fi, lo, _hi = part
        for cols in (self.colsA, self.colsB):
            _check_columns_fit(cols, n, self.groups[0][fi])
        return sess.add_columns(X, n, self.colsA, self.colsB, shuffle_key(fi, lo))


def _check_columns_fit(cols, n, path):
    """A column group against a parsed file of n columns (an empty file has none and holds nothing to select from)."""
    if n and len(cols) and int(cols.max()) >= n:
        raise ValueError("biosample {} is not in {}: the file has {} biosample columns".format(int(cols.max()) + 1, path, n))


class StateCheckFailed(SystemExit):
    """--check-states found a byte that is no state: every rank leaves with this (exit status 1), rank 0 has printed the message."""


_KEY_NONE = (1 << 62)                                  # above every key of _verdict_key


def state_check_message(path, row, column, byte, S):
    return ("ERROR: [--check-states] {}: row {} (0-based), biosample {}: byte {} is not a state of the {}-state model "
            "(a state byte is 0..{})".format(path, row, column, byte, S, S - 1))


def _verdict_key(fi, row, col, g):
    """(file in run order, row, column, group) packed so that integer order is that order (paired mode: group A before B as the
    last tie-break); None when a field does not fit (14, 31, 16 bits and 1)."""
    if not (0 <= fi < 1 << 14 and 0 <= row < 1 << 31 and 0 <= col < 1 << 16 and 0 <= g < 2):
        return None
    return (((fi << 31 | row) << 16 | col) << 1) | g


def _verdict_fields(key):
    """-> (fi, row, col, g) of a key."""
    return key >> 48, (key >> 17) & 0x7fffffff, (key >> 1) & 0xffff, key & 1


def _state_verdict(d, sess, mode, jobs):
    """--check-states, after STEP 1: the smallest (file in run order, row, biosample) whose byte is no state, over every matrix
    any rank uploaded (paired mode: group A before group B at the same position).  jobs: this rank's (file index, first row, ...)
    per part, as parsed.  Every rank takes part in the same two all-reduces (the minimum of the packed position together with
    "a position did not fit the key", then the byte of the rank that holds the minimum), so all of them learn the one verdict and
    stop together -- no rank raises on its own; rank 0 prints the one message, the same for any number of ranks."""
    G = len(mode.groups)
    key, byte, unfit = _KEY_NONE, 0, 0
    for t, (row, col, b, _n) in sess.state_offenders().items():
        k, g = divmod(t, G)
        cand = _verdict_key(jobs[k][0], jobs[k][1] + row, col, g)
        if cand is None:                               # (beyond 16 384 files or 2^31 rows a file: every rank hears of it below)
            unfit = 1
        elif cand < key:
            key, byte = cand, b
    if d.world > 1:
        first, unfit = d.max_ints([-key, unfit])
        first = -first
    else:
        first = key
    if unfit:
        raise ValueError("--check-states: a byte that is no state lies beyond file 16384 or row 2^31 of a file: its position does not "
                         "fit the verdict's key")
    if first == _KEY_NONE:
        return
    if d.world > 1:
        byte = d.max_ints([byte if key == first else 0])[0]
    fi, row, col, g = _verdict_fields(first)
    if d.rank == 0:
        print(state_check_message(mode.groups[g][fi], row, col + 1, byte, mode.S), flush=True)
    d.barrier()                                        # the message is out before any rank's exit makes a launcher end the others
    raise StateCheckFailed(1)


def _run_groups(mode, outputDir, fileTag, backend, defer_writes, store=None, writer="host"):
    """STEP 1-3 of either mode over the bin-range partition -> (exp_freq, results of rank 0 by file stem, else None).
    store (a _ResidentStore, run_groupings): the partition is the store's -- planned by the run's first grouping -- and STEP 1
    takes its parts from the store's replayable source (_ResidentStore.parts), which keeps the uploaded matrices for the groupings
    to come; the session is closed on the way out.  Everything behind the count pass is the same code."""
    be = backend if backend is not None else _backend.get()
    _io.set_state_limit(mode.S)                        # above 31 states the parser keeps values up to 127 (wide kernels)
    d = _Dist()
    outputDir = Path(outputDir)
    tm = _Timer(d.rank)
    if d.rank == 0:
        _clean_parts(outputDir, mode.kind, fileTag)
    d.barrier()
    if store is None:
        plan = _plan(mode.groups[0], d, tm, *mode.groups[1:])
    else:
        if store.plan is None:                         # once per run: a side-car the first pass writes must not change the second's
            store.plan = _plan(mode.groups[0], d, tm)
        plan = store.plan
    sess = mode.open(be)
    try:
        return _run_session(mode, sess, d, tm, plan, outputDir, fileTag, defer_writes, store, writer)
    finally:
        if store is not None:
            store.uploads = int(getattr(sess, "n_uploads", 0))
            sess.close()                               # histograms, null groups and results go before the next grouping's session opens


def _run_session(mode, sess, d, tm, plan, outputDir, fileTag, defer_writes, store, text_writer="host"):
    """_run_groups, from the open session on.  text_writer="gpu": a part's text is formatted and compressed on the device, the
    writer pool's job is a plain file write (write_bgzf); a part whose scores the device refuses goes through the host writer."""
    if text_writer not in ("host", "gpu"):
        raise ValueError("writer must be 'host' or 'gpu'")
    files = mode.groups[0]
    layout, rows, my_parts, owner = plan
    if mode.check_states:
        sess.check_states = True                       # (--check-states: every uploaded matrix is censused, see _state_verdict)

    # STEP 1: every part of this rank is parsed, uploaded once and counted; what the score pass needs stays resident
    pids, locs, widths = [None] * len(my_parts), [None] * len(my_parts), [0] * mode.n_widths
    # paired: part k's two groups are jobs 2k and 2k + 1, the second group follows the first one's row ranges
    jobs = [(group[fi], lo, hi) for fi, lo, hi in my_parts for group in mode.groups]
    # a store (run_groupings; one file group) hands out matrices that are on the device: its own, or read and uploaded just now
    stream = (store.parts if store is not None else _stream_parts)(jobs, sess, mode.S, raw=mode.check_states)
    with closing(stream) as stream:
        for t, x, n, loc in stream:                    # in order of completion
            k, g = divmod(t, len(mode.groups))
            mode.see_width(widths, g, n)               # an empty file has no width: it must not be the one that is remembered
            if g == 0:
                locs[k] = loc
            pids[k] = mode.add(sess, t, x, n, my_parts[k]) if store is None else mode.add_resident(sess, x, n, my_parts[k])
    if mode.check_states:                              # before anything of this run is written
        _state_verdict(d, sess, mode, my_parts)
    if layout == "whole":                              # single rank: the row counts come from the parse
        rows = [len(l) for l in locs]
        my_parts = [(fi, 0, rows[fi]) for fi in range(len(files))]
    if d.world > 1:
        widths = d.max_ints(widths)                    # a rank without bins learns the widths from the others
    if layout == "assigned":
        rows = _exchange_rows(d, my_parts, locs, len(files))
        tm.lap("parse + upload + expected counts (each file once, on one rank)")
        plans = plan_partition(rows, d.world)
        starts = np.concatenate([[0], np.cumsum(rows)])
        mine = {fi: (pids[k], locs[k]) for k, (fi, _lo, _hi) in enumerate(my_parts)}
        session_widths = widths[0] if len(widths) == 1 else tuple(widths)          # N, or (NA, NB)
        pids, locs = _redistribute(d, sess, plans, owner, mine, starts, session_widths)
        my_parts = plans[d.rank]
        tm.lap("hand border pieces to their owners")
    else:
        plans = plan_partition(rows, d.world) if d.world > 1 else [my_parts]
        tm.lap("parse + upload + expected counts")
    if not widths[0]:
        widths = mode.default_widths()
    N = sum(widths)                                    # paired: the background counts are over the concatenation [A|B]
    sess.ensure_acc(N)
    sess.all_reduce(d)                                 # the one exchange step; a rank without bins contributes zeros
    # STEP 2 (identical normalisation on every rank) and STEP 3 of every part enqueued without a host synchronisation; then
    # the host side: count check, S1 table verification, exp_freq as a host array (bench.py times this very sequence)
    sess.launch(int(sum(rows)), N, pids)
    q = sess.finish(int(sum(rows)), N)
    if d.rank == 0:
        np.save(outputDir / "exp_freq_{}.npy".format(fileTag), q, allow_pickle=False)
    tm.lap("all-reduce + check + normalise")

    # STEP 3: results from the resident data; text is formatted and compressed by writer threads while the next part scores
    payloads, jobs = [], []
    nwriters = min(2, _io.host_budget())               # two files are written at a time: half of this rank's cores each
    wthreads = max(1, _io.host_budget() // nwriters)
    writer = ThreadPoolExecutor(max_workers=nwriters)
    try:
        for k, (fi, lo, hi) in enumerate(my_parts):
            text, arrays = mode.part_out(sess, pids[k]) if text_writer == "host" else mode.part_out(sess, pids[k], locs[k])
            whole = lo == 0 and hi == rows[fi]
            name = "{}_{}_{}.txt.gz".format(mode.kind, fileTag, fileStem(files[fi])) if whole else _part_name(mode.kind, fileTag, fi, lo)
            if isinstance(text, _DeviceText) and text.blob is not None:
                jobs.append(writer.submit(write_bgzf, outputDir / name, [text.blob], whole))
                payloads.append(arrays + [np.asarray(locs[k].blob), np.asarray(locs[k].offsets)])
                continue
            if isinstance(text, _DeviceText):
                print("WARNING: [--writer gpu] {} holds a value the device does not format (not finite, or 2^31 and above): this file is "
                      "written by the host writer".format(name), flush=True)
                text = text.array
            jobs.append(writer.submit(writeScores, text, outputDir / name, locs[k], None, wthreads))
            payloads.append(arrays + [np.asarray(locs[k].blob), np.asarray(locs[k].offsets)])
        if text_writer == "gpu":
            sess.release_text()
        tm.lap("scores (kernels + download)")
    except BaseException:
        writer.shutdown(wait=True)
        raise
    if defer_writes and d.world == 1:
        # one process: the text goes on being formatted and compressed in the writer threads while the caller runs STEP 4 on the
        # arrays (finish_writes() waits for them); several ranks need their part files complete before rank 0 assembles them
        _deferred.append((writer, jobs, tm, "write text (under STEP 4)"))
    else:
        _wait_writes(writer, jobs)
        tm.lap("write text (overlapped tail)")
    tm.note("H2D uploads: %d for %d part(s)" % (getattr(sess, "n_uploads", 0), len(my_parts)) + mode.upload_note)
    d.barrier()
    got = _gather_parts(d, plans, payloads, mode.n_payload + 2)
    results = {} if d.rank == 0 else None
    if d.rank == 0:
        for fi, f in enumerate(files):
            stem = fileStem(f)
            final = "{}_{}_{}.txt.gz".format(mode.kind, fileTag, stem)
            owners = sorted((lo, hi) for parts in plans for (pf, lo, hi) in parts if pf == fi)
            _assemble_text(outputDir, mode.kind, final, fileTag, fi, owners, rows[fi], text_writer)
            if not owners and text_writer == "gpu":
                write_bgzf(outputDir / final, [])
            elif not owners:                           # an empty input file still gets its (empty) output
                writeScores(np.zeros((0, mode.S), dtype=np.float32), outputDir / final,
                            _io.Locations(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)))
            parts = [got[(fi, lo)] for lo, _ in owners]
            loc = _cat_locations([_io.Locations(p[-2], p[-1]) for p in parts])
            chrName = loc.slice(0, 1).to_object_array()[0, 0] if len(loc) else ""
            results[stem] = mode.result(lambda what: outputDir / "temp_{}_{}_{}.npz".format(what, fileTag, stem), chrName, loc,
                                        [[p[i] for p in parts] for i in range(mode.n_payload)])
        tm.lap("assemble files" + (" + temp npz" if mode.keep_temps else ""))
    _io.log_thread_census("%s s%d rank %d of %d" % (mode.census, mode.sal, d.rank, d.world))
    d.barrier()
    return q, results


def _nbytes(X):
    return int(X.nbytes) if isinstance(X, np.ndarray) else int(X.numel() * X.element_size())


def _device_free(X):
    """Free bytes of the device X lives on, None when X is no device tensor (the host stand-ins of the tests)."""
    if isinstance(X, np.ndarray) or not X.is_cuda:
        return None
    import torch
    return int(torch.cuda.mem_get_info(X.device)[0])


class _ResidentStore:
    """The input matrices of a run_groupings run on this rank's device, between its groupings: job (path, lo, hi) -> (matrix,
    its width, its Locations), plus the run's partition plan.  `parts` is the replayable source STEP 1 reads from: a kept job comes
    from the store -- no parse, no staging buffer, no upload -- any other job goes through the ordinary readers and one upload,
    on every pass.

    Admission is per job, on the pass that first reads it.  A matrix is kept unless
      - the device's free memory at that moment is below FREE_FACTOR x its bytes + FREE_SLACK (a grouping's session needs
        histograms, null groups and results next to the matrices: up to 36 B per bin and group against N B per bin), or
      - the kept bytes would exceed EPILOGOS_RESIDENT_BYTES (per rank; 0 = keep nothing, unset = no cap).
    FREE_FACTOR and FREE_SLACK are a choice, not a measurement: twice the matrix plus 2 GiB is room that every session measured
    so far fits in many times over at 833 biosamples; nobody has looked for the smallest values that work.
    The cap is applied IN JOB ORDER, whatever order the readers finish in (a matrix that arrives early waits, on the device, for
    the verdicts of the jobs before it), so that what is kept does not depend on the timing of the parser threads.

    `seed` is the way in for matrices that never were files (run_groupings(resident=...)): they are kept from the start under the
    jobs of their virtual paths, so no pass reads, parses or uploads anything.  Whether they fit is the caller's question, asked
    once for all of them with the same rule (`fits`); EPILOGOS_RESIDENT_BYTES does not apply -- there is no file to fall back to."""
    FREE_FACTOR, FREE_SLACK = 2, 2 << 30

    def __init__(self):
        cap = os.environ.get("EPILOGOS_RESIDENT_BYTES", "")
        self.cap = int(cap) if cap.strip() else None
        self.plan = None
        self.kept, self.bytes, self.refused = {}, 0, []
        self._seen, self._wait, self._next = set(), {}, 0
        self.uploads = self.parsed = 0                 # of the grouping under way

    @classmethod
    def fits(cls, nbytes, free):
        """The admission rule: `free` bytes of device memory (None: not a device) leave room for a session next to nbytes of matrices."""
        return free is None or free >= cls.FREE_FACTOR * nbytes + cls.FREE_SLACK

    def seed(self, files, resident):
        """Matrices that are on the device already: resident[path] = (X, N, Locations) for every path of `files` (one rank, whole
        files: the plan is made from what is here, no header is read)."""
        resident = {Path(p): v for p, v in resident.items()}
        for f in files:
            X, n, loc = resident[Path(f)]
            self.kept[(Path(f), 0, None)] = (X, n, loc)
            self.bytes += _nbytes(X)
        self._seen.update(self.kept)
        self.plan = ("whole", None, [(fi, 0, None) for fi in range(len(files))], None)

    def _offer(self, t, job, X, n, loc):
        nbytes, free = _nbytes(X), _device_free(X)
        room = self.fits(nbytes, free)
        self._wait[t] = (job, X if room else None, n, loc, nbytes)
        while self._next in self._wait:
            job, X, n, loc, nbytes = self._wait.pop(self._next)
            self._next += 1
            if X is not None and (self.cap is None or self.bytes + nbytes <= self.cap):
                self.kept[job] = (X, n, loc)
                self.bytes += nbytes
            else:
                self.refused.append(job)

    def parts(self, jobs, sess, numStates, raw=False):
        """-> generator of (index in jobs, matrix on the device, N, Locations): the kept jobs first, then the others as their
        readers finish."""
        jobs = [(Path(p), lo, hi) for p, lo, hi in jobs]
        self.uploads = self.parsed = 0
        first = not self._seen                         # the pass that admits: every job is new to it
        todo = [t for t, job in enumerate(jobs) if job not in self.kept]
        if first:
            self._seen.update(jobs)
            self._wait, self._next = {}, 0
        for t, job in enumerate(jobs):
            if job in self.kept:
                X, n, loc = self.kept[job]
                if raw:                                # (--check-states, the first pass: only a seeded matrix is kept by then)
                    sess.check_resident(X, n, t)
                yield t, X, n, loc
        if not todo:
            return
        with closing(_stream_parts([jobs[t] for t in todo], sess, numStates, raw=raw)) as stream:
            for rt, arr, n, loc in stream:             # (rt: the reader's ticket, which is what the staging buffer is held under)
                X = sess.stage(arr, n, rt)
                self.parsed += 1
                if first:
                    self._offer(todo[rt], jobs[todo[rt]], X, n, loc)
                yield todo[rt], X, n, loc


def run_groupings(files, groupings, numStates, saliency, outputDir, fileTag, quiescentState=None, groupSize=-1, nullSeed=None,
                  verbose=False, backend=None, device=None, keep_temps=True, defer_writes=False, nullDraws=1, checkStates=False,
                  resident=None, flat=False, writer="host"):
    """Many groupings of the biosample columns of ONE set of files in one run: every file is parsed and uploaded once, its matrix
    stays on the device (_ResidentStore: unless the admission rule refuses it), and every grouping runs STEP 1-3 from the resident
    matrices with a session of its own.  groupings: [(name, cols)] -- each what run_single_group(columns=cols) computes -- or
    [(name, colsA, colsB)] -- run_paired_columns -- with 0-based column indices (helpers.parseGroupings); the outputs of a
    grouping go to outputDir/name, the files and bytes of that function called with that directory.  The remaining arguments are
    those functions'; nullSeed=None draws one seed for the whole run (one rank; several ranks must be given the same seed).
    A GENERATOR: yields (name, exp_freq, results, info) as each grouping is done -- results as the run_* function returns them
    (rank 0, else None) -- so a caller finishes a grouping (STEP 4, finish_writes()) before the next one begins.  info:
    uploads (H2D matrix copies this rank made for the grouping), parsed_files (passes over input files this rank made for it),
    resident_bytes (bytes of input matrices this rank holds on the device after it), kept_files / refused_files (this rank's jobs
    in and not in the store).  checkStates censuses every matrix on the first pass, which is the pass that uploads them all.
    A grouping that raises ends the run; the directories of the groupings before it are complete.
    resident ({path: (X, N, Locations)} for every path of `files`, one rank): the matrices are on the device already -- built there,
    never files -- and `files` only names them (output stems, messages, the run order that keys the null shuffle).  The store is
    seeded with them: no reader starts, nothing is parsed or uploaded, every grouping's info says uploads == parsed_files == 0, and
    checkStates censuses them where they are.  They are read, never written.
    flat (one grouping): its outputs go to outputDir itself -- a plain run, --columns or --columns-a/-b over resident matrices is
    a one-grouping run of this function; a single-mode grouping whose columns are None is the whole matrix.
    writer ("host" or "gpu", here and in the run_* functions below): where the score text of every part is formatted and compressed
    (write_bgzf; the command line's --writer)."""
    files = [Path(f) for f in files]
    groupings = [tuple(g) for g in groupings]
    if not groupings:
        raise ValueError("no groupings")
    paired = len(groupings[0]) == 3
    if any(len(g) != len(groupings[0]) or len(g) not in (2, 3) for g in groupings):
        raise ValueError("a grouping is (name, columns) or (name, columns A, columns B), the same kind for the whole run")
    d = _Dist()
    if paired and nullSeed is None:
        if d.world > 1:
            raise ValueError("several ranks must be given the same null seed")
        nullSeed = int(np.random.SeedSequence().generate_state(1)[0])
    if flat and len(groupings) != 1:
        raise ValueError("a run without subdirectories has one grouping")
    store = _ResidentStore()
    if resident is not None:
        if d.world > 1:
            raise ValueError("resident matrices are one rank's: sharing them out over several ranks is not available")
        store.seed(files, resident)
    try:
        for k, g in enumerate(groupings):
            out = Path(outputDir) if flat else Path(outputDir) / g[0]
            out.mkdir(parents=True, exist_ok=True)
            if paired:
                mode = _PairedColumns(files, g[1], g[2], numStates, saliency, quiescentState, groupSize, nullSeed, keep_temps, nullDraws)
            else:
                mode = _Single(files, numStates, saliency, keep_temps, g[1])
            mode.check_states = bool(checkStates) and k == 0
            q, results = _run_groups(mode, out, fileTag, backend, defer_writes, store, writer)
            if k == 0 and len(groupings) > 1:
                # what did not fit is said once, by rank 0, for all ranks (a collective: every rank is here after its first grouping)
                kept, refused = (int(v) for v in d.all_reduce_counts(np.array([len(store.kept), len(store.refused)], dtype=np.int64)))
                if refused and d.rank == 0:
                    print("epilogos_amd: {} of {} input matrices stay on the device between the groupings; {} do not (free device "
                          "memory or EPILOGOS_RESIDENT_BYTES) and are read, parsed and uploaded again by every grouping"
                          .format(kept, kept + refused, refused), flush=True)
            yield g[0], q, results, {"uploads": store.uploads, "parsed_files": store.parsed, "resident_bytes": store.bytes,
                                     "kept_files": len(store.kept), "refused_files": len(store.refused)}
    finally:
        abort_early_readers()
        store.kept = {}


def run_single_group(files, numStates, saliency, outputDir, fileTag, verbose=False, backend=None, device=None,
                     keep_temp_scores=True, defer_writes=False, columns=None, checkStates=False, writer="host"):
    """STEP 1-3 for a single group over `files` (one per chromosome).  Returns (exp_freq float32, results) where results
    (rank 0 only, else None) maps file stem -> (chrName, float32 scores [R, S], _io.Locations) for an in-process STEP 4.
    keep_temp_scores writes the reference's temp_scores_{tag}_{stem}.npz (scores.py:166-169) for a STEP 4 run
    elsewhere; the command line skips them because its STEP 4 would delete them a moment later.  columns (0-based indices of
    biosample columns): the group is these columns of the files; the outputs are those of files cut to them beforehand."""
    mode = _Single([Path(f) for f in files], numStates, saliency, keep_temp_scores, columns)
    mode.check_states = bool(checkStates)
    return _run_groups(mode, outputDir, fileTag, backend, defer_writes, writer=writer)


def run_paired_groups(files1, files2, numStates, saliency, outputDir, fileTag, quiescentState, groupSize, nullSeed,
                      verbose=False, backend=None, device=None, keep_temps=True, defer_writes=False, nullDraws=1, checkStates=False,
                      writer="host"):
    """STEP 1-3 of paired mode (reference run.py:205-221,258-279 + scores.py:172-256) over the bin-range partition.
    Background counts are taken over the column concatenation [A|B] (helpers.py:173) -- from the two groups' own
    histograms, each group is uploaded once -- all-reduced once; each rank then scores A, B and the two shuffled null
    groups of its bins from the resident data.  The null shuffle is keyed by (seed, file ordinal, row in the file)
    (shuffle_key), so the outputs do not depend on the number of GPUs.  Returns (exp_freq, results); results (rank 0) maps file stem ->
    dict(chrName, locations, nullDistances, quiescenceArr, distances, maxDiff) for an in-process STEP 4; keep_temps
    also writes temp_nullDistances / temp_quiescence (the reference's, scores.py:246-255) and temp_pairMetrics (the
    side-car of this engine's STEP 4).  nullDraws K > 1 (one rank): every bin's null groups are drawn K times (seeds
    helpers.null_draw_seeds(nullSeed, K): draw 0 is the run's own null, every other output is unchanged) and every file's entry
    also has nullExceed (int64 per bin: how many of the pooled null distances of the non-quiescent bins reach |distance|) and
    nullPool (their number), from which STEP 4 takes empirical p-values; keep_temps writes them as temp_nullExceed."""
    mode = _Paired([Path(f) for f in files1], [Path(f) for f in files2], numStates, saliency, quiescentState, groupSize, nullSeed,
                   keep_temps, nullDraws)
    mode.check_states = bool(checkStates)
    return _run_groups(mode, outputDir, fileTag, backend, defer_writes, writer=writer)


def run_paired_columns(files, colsA, colsB, numStates, saliency, outputDir, fileTag, quiescentState, groupSize, nullSeed,
                       verbose=False, backend=None, device=None, keep_temps=True, defer_writes=False, nullDraws=1, checkStates=False,
                      writer="host"):
    """run_paired_groups for two groups that are column groups (0-based indices) of ONE set of files: every file is parsed and
    uploaded once and feeds both groups.  The partition, the hand-over between ranks and the all-reduce are run_paired_groups':
    they move histograms and row ranges.  Outputs are those of run_paired_groups on files cut to the groups beforehand."""
    mode = _PairedColumns([Path(f) for f in files], colsA, colsB, numStates, saliency, quiescentState, groupSize, nullSeed, keep_temps,
                          nullDraws)
    mode.check_states = bool(checkStates)
    return _run_groups(mode, outputDir, fileTag, backend, defer_writes, writer=writer)
