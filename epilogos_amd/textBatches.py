"""Batches of inflated text files on the device: the pipeline stateByLine.build_matrix_device and segments.build_matrices_device
share.  Nothing here knows a file format.

TextBatches      inflate a batch of files on a thread pool while the batch before it is on the device, stage the texts 16-byte
                 aligned into one of two pinned slots, copy the slot to the device on the current stream
reread_on_host   the one warning line for a file the device refused, and the file's text for the host parser
put_column       a host column into column k of a resident matrix (a one-column epg_sbl_transpose)
align, first_fields, offsets_of, slot_capacity, pointers, mark, set_timings   the small things both readers use"""
from concurrent.futures import ThreadPoolExecutor
from time import perf_counter

import numpy as np

from . import _abi, _io

TEXT_ALIGN = 16                                                  # every text of a batch starts at a multiple of this
PAGE = 4096


def align(n, a):
    return (int(n) + a - 1) // a * a


def first_fields(path, skip=0):
    """`cut -f1 FILE | tail -n +(skip+1)` inside `$( )`: the first tab-separated field of every line, split at blanks."""
    out = []
    with open(path, "r", newline="\n") as fh:
        for line in fh.read().split("\n")[skip:]:
            out.extend(line.split("\t")[0].split())
    return out


def offsets_of(sizes, a=TEXT_ALIGN):
    """int64 [len(sizes) + 1]: where each of the texts starts when every one is aligned to `a` bytes; the last entry is the total."""
    offs = np.zeros(len(sizes) + 1, dtype=np.int64)
    for j, n in enumerate(sizes):
        offs[j + 1] = offs[j] + align(n, a)
    return offs


def slot_capacity(total, have=None):
    """The bytes a staging slot must hold for a batch of `total` bytes when it holds `have` (None: no buffer yet): what it has
    while that is enough, otherwise an eighth more than asked for, rounded up to a page."""
    if have is not None and have >= total:
        return have
    return align(total + total // 8, PAGE)


def pointers(t, starts=None):
    """The address (an int: the entry points take it as void*, 0 as NULL) of every row of the tensor t, or with `starts` of t[s:]
    for every s: one data_ptr() and integer arithmetic.  Neither a tensor view nor a ctypes object per file: objects the garbage
    collector tracks, kept by the thousand for a batch, bring its full collection (50 - 120 ms with torch loaded) into a build more
    often than before; views in front of each launch also slowed the launch-bound expand loop (9.4 against 7.2 - 8.3 ms a build)."""
    base, step = t.data_ptr(), t.element_size()
    if starts is None:
        starts, step = range(t.shape[0]), step * t.stride(0)
    return [base + step * int(s) for s in starts]


def mark():
    """A timing event recorded on the current stream."""
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record(torch.cuda.current_stream())
    return e


def set_timings(timings, inflate_s, events):
    """timings (a dict or None) receives inflate_s and, for every name of `events` ({name: [(start, end)]}), name_ms: the HIP
    event times summed over the batches.  Call it behind the synchronisation that follows the last batch."""
    if timings is None:
        return
    timings["inflate_s"] = inflate_s
    for k, pairs in events.items():
        timings[k + "_ms"] = float(sum(a.elapsed_time(b) for a, b in pairs))


class Batch:
    """Files k0 .. k0 + nb - 1 on the device: text j is bytes offsets[j] .. offsets[j] + sizes[j] of `text` (uint8, the slot's
    whole device buffer: pointers(text, offsets[:-1]) are the texts), facts[j] is what inspect() returned for it, upload =
    (event before, event after) the copy.  release() tells the pipeline that everything enqueued so far on the current stream is all that reads
    `text`: the slot is staged again only when that has run."""

    def __init__(self, slot, k0, nb, offsets, sizes, facts, upload):
        self._slot, self.k0, self.nb, self.offsets, self.sizes, self.facts, self.upload = slot, k0, nb, offsets, sizes, facts, upload
        self.text = slot["device"]

    def release(self):
        self._slot["free"] = mark()


class TextBatches:
    """with TextBatches(files, batch, threads, device, inspect) as batches: for b in batches: ... b.release()

    Inflates `batch` files at a time through the native reader on `threads` threads; batch k + 1 is submitted before batch k is
    handed out, so it inflates while the consumer enqueues batch k's kernels.  inspect(k, data) runs on the inflated text of file
    k while it is open.  Two slots of pinned and device memory alternate; a slot is staged again after the event of its last
    batch's release(), and grows (slot_capacity) when a batch does not fit.  Every text is closed before its batch is handed out;
    leaving the `with` block, by an exception too, waits for the files still inflating and gives their buffers back.
    inflate_s: the time spent waiting for the inflating threads and staging, so far."""

    def __init__(self, files, batch, threads, device, inspect):
        self.files, self.batch, self.threads, self.device, self.inspect = list(files), int(batch), int(threads), device, inspect
        self.inflate_s = 0.0
        self._pool, self._next = None, []

    def _submit(self, k0):
        return [self._pool.submit(_io.Text, self.files[k], 1) for k in range(k0, min(k0 + self.batch, len(self.files)))]

    def __enter__(self):
        self._pool = ThreadPoolExecutor(max_workers=self.threads)
        self._next = self._submit(0)
        return self

    def __exit__(self, *exc):
        for f in self._next:                                     # an error on the way: give the inflated buffers back
            try:
                f.result().close()
            except Exception:
                pass
        self._next = []
        self._pool.shutdown(wait=True)
        return False

    def __iter__(self):
        import torch
        N, pool = len(self.files), self._pool
        slots = [{"pinned": None, "device": None, "free": None} for _ in range(2)]      # free: None = never used, False = handed out
        for bi, k0 in enumerate(range(0, N, self.batch)):
            nb = min(self.batch, N - k0)
            slot = slots[bi % 2]
            t0 = perf_counter()
            futs, self._next = self._next, []
            texts = []
            try:
                for f in futs:                                   # (one that fails leaves the rest to the finally below)
                    texts.append(f.result())
                sizes = [len(tx.data) for tx in texts]
                facts = [self.inspect(k0 + j, tx.data) for j, tx in enumerate(texts)]
                offs = offsets_of(sizes)
                total = int(offs[-1])
                if slot["free"] is False:
                    raise RuntimeError("TextBatches: the batch before the last was not released")
                if slot["free"] is not None:
                    slot["free"].synchronize()
                cap = slot_capacity(total, None if slot["pinned"] is None else slot["pinned"].numel())
                if slot["pinned"] is None or cap != slot["pinned"].numel():
                    slot["pinned"] = torch.empty(cap, dtype=torch.uint8).pin_memory()
                    slot["device"] = torch.empty(cap, dtype=torch.uint8, device=self.device)
                host = slot["pinned"].numpy()

                def stage(j):
                    host[offs[j]:offs[j] + sizes[j]] = texts[j].data
                list(pool.map(stage, range(nb)))
                if k0 + nb < N:                                  # the next batch inflates while this one is on the device
                    self._next = self._submit(k0 + nb)
            finally:
                for tx in texts:
                    tx.close()
                for f in futs[len(texts):]:
                    try:
                        f.result().close()
                    except Exception:
                        pass
            self.inflate_s += perf_counter() - t0
            e0 = mark()
            slot["device"][:total].copy_(slot["pinned"][:total], non_blocking=True)
            e1 = mark()
            slot["free"] = False
            yield Batch(slot, k0, nb, offs, sizes, facts, (e0, e1))


def reread_on_host(path, line, what, parse):
    """A file the device refused at 1-based `line`: one warning line that says what the line is not, then parse(text) of the
    file's inflated text."""
    print("epilogos_amd: {}: line {} is not {} -- reading this file on the host (slow)".format(path, line, what), flush=True)
    with _io.Text(path, 1) as tx:
        return parse(tx.data)


def put_column(X, k, col, pitch):
    """col: int8 host column of X.shape[0] states -> column k of the resident matrix X [R, ldx], on the current stream."""
    import torch
    from . import engine
    R = X.shape[0]
    c = torch.empty(pitch, dtype=torch.int8, device=X.device)
    c[:R].copy_(torch.from_numpy(col))
    _abi.call("epg_sbl_transpose", engine.ptr(c), 1, pitch, R, engine.ptr(X), X.shape[1], k, engine.stream())
