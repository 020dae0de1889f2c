"""The scores file of a live similarity search query, read on the GPU (csrc/epg_scores_text.hip, include/epilogos_scores_text.h).

read_scores_device(path) inflates the file with the native library (BGZF blocks in parallel, other gzip on one core), cuts the
text into chunks of whole rows, stages each chunk in one of two page-locked buffers, uploads it on a copy stream and parses it
on the current stream: chunk k + 1 is staged and uploaded while chunk k parses.  Nothing is synchronised before the last chunk:
the rows of a chunk are counted on the host (its newlines), so every chunk knows its row offset in the final tensors, and the
status word is shared by all chunks.  The parser is strict: a file that is not of its grammar raises NotStrict with the first
offending row and the caller reads it with pandas instead (similaritySearch_query.readGrid), as helpers.readTable does for
state matrices.  Python does no per-row work: chromosome names are read from the text at the rows where they change."""
import ctypes as C

import numpy as np

from . import _abi, _io

CHUNK_BYTES = 32 << 20
CLEAN = 2 ** 63 - 1
REASONS = {1: "a field count that differs from the first row's", 2: "an empty field", 3: "a blank, a control character or a byte outside ASCII",
           4: "a chromosome that does not start with a letter or _", 5: "start or end is not a plain integer",
           6: "a score that is not [-]digits[.1-5 digits]", 7: "a score beyond the int32 grid", 8: "more rows than counted"}
# chromosome names pandas would not keep as the text they are (its NA spellings, booleans, infinities)
NOT_TEXT = {"#n/a", "#n/a n/a", "#na", "-nan", "-inf", "inf", "infinity", "-infinity", "<na>", "n/a", "na", "null", "nan", "none",
            "true", "false"}


class NotStrict(Exception):
    """The file is outside the strict grammar: `reason` (text) at `row` (0-based row of the file)."""

    def __init__(self, reason, row, code=0):
        super().__init__("row %d: %s" % (row, reason))
        self.reason, self.row, self.code = reason, int(row), int(code)      # code: the EPGT_REASON_* of the device, 0 = the host's


def cut_chunks(text, chunk_bytes):
    """[(first byte, end)] of the chunks of `text` (bytes or uint8 array): each ends behind the last newline within chunk_bytes of
    its start, behind the first one after that when a row is longer than chunk_bytes, at the end of the text when there is none."""
    a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else text
    n, chunk_bytes, out, lo = len(a), max(1, int(chunk_bytes)), [], 0
    while lo < n:
        hi = min(n, lo + chunk_bytes)
        if hi < n:
            end, step = -1, 4096
            top = hi
            while end < 0 and top > lo:                          # the last newline of a[lo:hi], a block at a time from the back
                bot = max(lo, top - step)
                nl = np.flatnonzero(a[bot:top] == 10)
                if len(nl):
                    end = bot + int(nl[-1]) + 1
                top, step = bot, step * 4
            while end < 0 and hi < n:                            # a row longer than the chunk: on to its newline
                nl = np.flatnonzero(a[hi:hi + step] == 10)
                end = hi + int(nl[0]) + 1 if len(nl) else -1
                hi = min(n, hi + step)
            hi = end if end > 0 else n
        out.append((lo, hi))
        lo = hi
    return out


def first_row_fields(a):
    """Number of tab-separated fields of the first row of the text."""
    step, lo = 1 << 16, 0
    tabs = 0
    while lo < len(a):
        blk = a[lo:lo + step]
        nl = np.flatnonzero(blk == 10)
        if len(nl):
            return tabs + int(np.count_nonzero(blk[:nl[0]] == 9)) + 1
        tabs += int(np.count_nonzero(blk == 9))
        lo += step
    return tabs + 1


def _name_at(a, pos):
    """The chromosome field that starts at byte `pos`."""
    step = 64
    while True:
        blk = a[pos:pos + step]
        tab = np.flatnonzero(blk == 9)
        if len(tab) or pos + step >= len(a):
            return blk[:tab[0] if len(tab) else len(blk)].tobytes().decode("ascii")
        step *= 8


def read_scores_device(path, chunk_bytes=CHUNK_BYTES, timings=None):
    """-> (x int32 [R, S] device tensor, start int64 [R], end int64 [R] host arrays, runs [(chromosome, row0, row1)]); raises
    NotStrict.  `timings` (a dict) receives inflate_s (the file to text), count_s (chunk cutting and row counts), upload_parse_ms (HIP events
    around all chunks) and coords_s."""
    import torch
    from time import perf_counter
    from . import engine
    engine.require_gpu()
    chunk_bytes = min(int(chunk_bytes), 0x7fff0000 // 2)
    threads = _io.host_budget()
    t0 = perf_counter()
    with _io.Text(path, threads) as text:
        a = text.data
        if len(a) == 0:
            raise NotStrict("an empty file", 0)
        if timings is not None:
            timings["inflate_s"] = perf_counter() - t0
        t0 = perf_counter()
        F = first_row_fields(a)
        if F < 4:
            raise NotStrict(REASONS[1], 0, 1)
        chunks = cut_chunks(a, chunk_bytes)
        rows = [_io.count_newlines(a[lo:hi], threads) for lo, hi in chunks]
        if a[-1] != 10:
            rows[-1] += 1
        row0 = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
        R, S = int(row0[-1]), F - 3
        if timings is not None:
            timings["count_s"] = perf_counter() - t0
        dev = torch.device("cuda", torch.cuda.current_device())
        cap = max(hi - lo for lo, hi in chunks)
        x = torch.empty((R, S), dtype=torch.int32, device=dev)
        start = torch.empty(R, dtype=torch.int64, device=dev)
        end = torch.empty(R, dtype=torch.int64, device=dev)
        chrom_at = torch.empty(R, dtype=torch.int32, device=dev)
        status = torch.tensor([CLEAN, 0], dtype=torch.int64, device=dev)
        wsb = _abi.call("epgt_scores_ws_bytes", cap)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(min(2, len(chunks)))]
        dtext = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in pinned]
        copied = [torch.cuda.Event() for _ in pinned]
        parsed = [torch.cuda.Event() for _ in pinned]
        main, copy = torch.cuda.current_stream(), torch.cuda.Stream()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(main)
        for k, (lo, hi) in enumerate(chunks):
            s, n = k % 2, hi - lo
            if k >= 2:
                copied[s].synchronize()                          # the pinned buffer's last upload has left it
            pinned[s].numpy()[:n] = a[lo:hi]
            with torch.cuda.stream(copy):
                if k >= 2:
                    copy.wait_event(parsed[s])                   # the device buffer's last parse is done
                dtext[s][:n].copy_(pinned[s][:n], non_blocking=True)
                copied[s].record(copy)
            main.wait_event(copied[s])
            _abi.call("epgt_scores_parse", engine._ptr(dtext[s]), n, F, int(rows[k]), int(row0[k]), engine._ptr(x), engine._ptr(start),
                      engine._ptr(end), engine._ptr(chrom_at), engine._ptr(ws), wsb, engine._ptr(status), engine._stream())
            parsed[s].record(main)
        ev1.record(main)
        word, _found = status.cpu().tolist()                     # the one synchronisation
        if timings is not None:
            timings["upload_parse_ms"] = ev0.elapsed_time(ev1)
        if word != CLEAN:
            raise NotStrict(REASONS.get(word & 15, "reason %d" % (word & 15)), word >> 4, word & 15)
        t0 = perf_counter()
        at = torch.nonzero(chrom_at >= 0).reshape(-1)
        pos = chrom_at[at].cpu().numpy().astype(np.int64)
        at = at.cpu().numpy()
        pos += np.asarray([c[0] for c in chunks], dtype=np.int64)[np.searchsorted(row0, at, side="right") - 1]
        runs = []
        for r, p in zip(at.tolist(), pos.tolist()):              # one turn per change of chromosome (and per chunk)
            name = _name_at(a, p)
            if runs and runs[-1][0] == name:                     # a chunk's first row carries on the chromosome before it
                continue
            if name.lower() in NOT_TEXT:
                raise NotStrict("a chromosome name pandas does not keep as text (%s)" % name, r)
            if runs:
                runs[-1][2] = r
            runs.append([name, r, R])
        start, end = start.cpu().numpy(), end.cpu().numpy()
        if timings is not None:
            timings["coords_s"] = perf_counter() - t0
    return x, start, end, [tuple(r) for r in runs]
