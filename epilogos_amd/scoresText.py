"""The scores file of a live similarity search query, read on the GPU (csrc/epg_scores_text.hip, include/epilogos_scores_text.h).

read_scores_device(path) inflates the file with the native library (BGZF blocks in parallel, other gzip on one core), cuts the
text into chunks of whole rows, stages each chunk in one of two page-locked buffers, uploads it on a copy stream and parses it
on the current stream: chunk k + 1 is staged and uploaded while chunk k parses.  Nothing is synchronised before the last chunk:
the rows of a chunk are counted on the host (its newlines), so every chunk knows its row offset in the final tensors, and the
status word is shared by all chunks.  The parser is strict: a file that is not of its grammar raises NotStrict with the first
offending row and the caller reads it with pandas instead (similaritySearch_query.readGrid), as helpers.readTable does for
state matrices.  Python does no per-row work: chromosome names are read from the text at the rows where they change.

read_scores_device(path, inflate="gpu") (`simsearch --inflate gpu`) inflates a BGZF file on the device instead
(csrc/epg_bgzf_inflate.h): bgzfIndex.members gives the member table, the COMPRESSED bytes are uploaded through the two page-locked
buffers in groups of whole members and inflated into one device text buffer, the newline index of the text (engine.newline_index)
lets the host cut the chunks and count their rows without the text, and the parser runs on slices of the device text."""
import numpy as np

from . import _io

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


class _DeviceText:
    """The device text as _name_at reads it: a slice is a small download."""

    def __init__(self, text, n):
        self.text, self.n = text, n

    def __len__(self):
        return self.n

    def __getitem__(self, s):
        return self.text[s.start:min(s.stop, self.n)].cpu().numpy()


def cut_chunks_indexed(n, chunk_bytes, seg_bytes, count, last):
    """cut_chunks without the text, from its newline index (engine.newline_index: per segment of seg_bytes bytes the number of
    newlines and the offset of the last one, -1 for none) -> ([(first byte, end)], rows of every chunk).  The rule is cut_chunks':
    a chunk ends behind a newline within chunk_bytes of its start -- the last one of the whole segments that end there, so up to a
    segment earlier than cut_chunks would --, a row longer than that runs on to a newline (the last one of the first segment that
    has one), the text's end closes the last chunk and counts as a row when no newline stands there."""
    n, chunk_bytes, seg_bytes = int(n), max(1, int(chunk_bytes)), int(seg_bytes)
    count, last = np.asarray(count, dtype=np.int64), np.asarray(last, dtype=np.int64)
    newest = np.maximum.accumulate(last) if len(last) else last                # the last newline at or before each segment's end
    before = np.concatenate(([0], np.cumsum(count))).astype(np.int64)
    total = int(before[-1]) + (1 if n and (not len(newest) or int(newest[-1]) != n - 1) else 0)
    chunks, rows, lo, done = [], [], 0, 0
    while lo < n:
        lim = lo + chunk_bytes
        if lim >= n:
            hi = n
        else:
            s = lim // seg_bytes - 1                                          # the last whole segment that ends at or before lim
            e = int(newest[s]) if s >= 0 else -1
            if e < lo:                                                         # a row longer than the chunk
                s = int(np.searchsorted(newest, lo, side="left"))
                e = int(newest[s]) if s < len(newest) else n - 1
            hi = e + 1
        r = total - done if hi == n else int(before[(hi - 1) // seg_bytes + 1]) - done
        chunks.append((lo, hi))
        rows.append(r)
        lo, done = hi, done + r
    return chunks, rows


def _parse_chunks(dev, chunks, rows, row0, F, texts, timings):
    """What both readers do with their chunks: the outputs for all row0[-1] rows, the status word the chunks share, and one
    epgt_scores_parse per chunk -- texts(parse) brings chunk after chunk to the device its own way and calls parse(k, device text)
    for each, on the current stream.  -> (x int32 [R, S], start, end int64 [R], chrom_at int32 [R]), device tensors; raises NotStrict.
    Synchronises once, to read the status word; timings receives upload_parse_ms (HIP events around all chunks)."""
    import torch
    from . import engine
    R, S = int(row0[-1]), F - 3
    x = torch.empty((R, S), dtype=torch.int32, device=dev)
    start = torch.empty(R, dtype=torch.int64, device=dev)
    end = torch.empty(R, dtype=torch.int64, device=dev)
    chrom_at = torch.empty(R, dtype=torch.int32, device=dev)
    status = torch.tensor([CLEAN, 0], dtype=torch.int64, device=dev)
    ws = torch.empty(engine.scores_ws_bytes(max(hi - lo for lo, hi in chunks)), dtype=torch.uint8, device=dev)
    main = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(main)
    texts(lambda k, t: engine.scores_parse(t, chunks[k][1] - chunks[k][0], F, int(rows[k]), int(row0[k]), x, start, end, chrom_at, ws, status))
    ev1.record(main)
    word, _found = status.cpu().tolist()
    if timings is not None:
        timings["upload_parse_ms"] = ev0.elapsed_time(ev1)
    if word != CLEAN:
        raise NotStrict(REASONS.get(word & 15, "reason %d" % (word & 15)), word >> 4, word & 15)
    return x, start, end, chrom_at


GROUP_BYTES = 32 << 20
INFLATE_CHOICES = ("host", "gpu")


def _read_scores_inflated(path, chunk_bytes, timings):
    """read_scores_device's result with the file inflated on the device (csrc/epg_bgzf_inflate.h), None when the host has to do it:
    the file is not BGZF all the way (plain gzip, text: nothing is said), or the device gave up a member (one warning line)."""
    import mmap
    import torch
    from time import perf_counter
    from . import bgzfIndex, engine
    t_all = perf_counter()
    got = bgzfIndex.members(path)
    if got is None or got[1] == 0:
        return None
    table, total = got
    M = len(table)
    if timings is not None:
        timings["index_s"] = perf_counter() - t_all
    chunk_bytes = min(int(chunk_bytes), 0x7fff0000 // 2)
    seg_bytes = max(16, min(4096, chunk_bytes // 4 // 16 * 16))
    dev = torch.device("cuda", torch.cuda.current_device())
    ends = table[:, 0] + table[:, 1] + bgzfIndex.TRAILER                       # the file offset behind every member
    groups, m0 = [], 0
    while m0 < M:                                                              # whole members, about GROUP_BYTES of the file each
        b0 = int(table[m0, 0]) - bgzfIndex.HEADER
        m1 = max(m0 + 1, int(np.searchsorted(ends, b0 + GROUP_BYTES, side="right")))
        groups.append((m0, m1, b0, int(ends[m1 - 1])))
        m0 = m1
    with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        a = np.frombuffer(mm, dtype=np.uint8)
        try:
            comp_bytes = len(a)
            cap = max(b1 - b0 for _m0, _m1, b0, b1 in groups)
            dcomp = torch.empty(comp_bytes, dtype=torch.uint8, device=dev)
            dtable = torch.from_numpy(table).to(dev)
            text = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
            mstatus = torch.empty(M, dtype=torch.int32, device=dev)
            flags = torch.zeros(len(groups), dtype=torch.int32, device=dev)
            pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(min(2, len(groups)))]
            copied = [torch.cuda.Event() for _ in pinned]
            main, copy = torch.cuda.current_stream(), torch.cuda.Stream()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            copy.wait_stream(main)
            ev[0].record(main)
            for k, (m0, m1, b0, b1) in enumerate(groups):
                s, nb = k % 2, b1 - b0
                if k >= 2:
                    copied[s].synchronize()                      # the pinned buffer's last upload has left it
                pinned[s].numpy()[:nb] = a[b0:b1]
                with torch.cuda.stream(copy):
                    dcomp[b0:b1].copy_(pinned[s][:nb], non_blocking=True)
                    copied[s].record(copy)
                main.wait_event(copied[s])
                engine.bgzf_inflate(dcomp, dtable[m0:m1], out=text, status=mstatus[m0:m1], flags=flags[k:k + 1])
            ev[1].record(main)
            count, last = engine.newline_index(text, seg_bytes, total)
            ev[2].record(main)
            count, last, bad = count.cpu().numpy(), last.cpu().numpy(), int(flags.sum().cpu())      # the one synchronisation
        finally:
            del a
    if timings is not None:
        timings["inflate_s"] = perf_counter() - t_all
        timings["upload_inflate_ms"] = ev[0].elapsed_time(ev[1])
        timings["newline_index_ms"] = ev[1].elapsed_time(ev[2])
    if bad:
        st = mstatus.cpu().numpy()
        k = int(np.flatnonzero(st)[0])
        print("WARNING: [--inflate gpu] %s: member %d (%s); inflating on the host instead"
              % (path, k, MEMBER_REASONS.get(int(st[k]), "reason %d" % int(st[k]))), flush=True)
        return None
    t0 = perf_counter()
    has = np.flatnonzero(last >= 0)
    head = text[:int(last[has[0]]) + 1 if len(has) else total].cpu().numpy()  # the first row (and what follows it in its segment)
    F = first_row_fields(head)
    if F < 4:
        raise NotStrict(REASONS[1], 0, 1)
    chunks, rows = cut_chunks_indexed(total, chunk_bytes, seg_bytes, count, last)
    row0 = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
    R = int(row0[-1])
    if timings is not None:
        timings["count_s"] = perf_counter() - t0

    def texts(parse):                                                          # slices of the device text: no second upload
        for k, (lo, hi) in enumerate(chunks):
            parse(k, text[lo:hi])
    x, start, end, chrom_at = _parse_chunks(dev, chunks, rows, row0, F, texts, timings)
    t0 = perf_counter()
    runs = _runs_of(_DeviceText(text, total), chrom_at, chunks, row0, R)
    start, end = start.cpu().numpy(), end.cpu().numpy()
    if timings is not None:
        timings["coords_s"] = perf_counter() - t0
    return x, start, end, [tuple(r) for r in runs]


# enum Reason of csrc/epg_bgzf_inflate_block.h
MEMBER_REASONS = {1: "its table row is refused", 2: "block type 3", 3: "a stored block's LEN and NLEN disagree", 4: "an over-subscribed code",
                  5: "an incomplete code", 6: "a repeat with no length before it", 7: "a run of code lengths past their number",
                  8: "literal/length symbol 286 or 287", 9: "distance symbol 30 or 31", 10: "a distance before the member's first byte",
                  11: "output beyond ISIZE", 12: "bits past the payload", 13: "CRC-32 mismatch", 14: "fewer bytes than ISIZE",
                  15: "bits that are no code", 16: "a bad dynamic block header", 17: "the stream ends before the payload"}


def _runs_of(a, chrom_at, chunks, row0, R):
    """[[chromosome, row0, row1]] from the rows where the parser saw the name change: the names are read from the text `a` there."""
    import torch
    at = torch.nonzero(chrom_at >= 0).reshape(-1)
    pos = chrom_at[at].cpu().numpy().astype(np.int64)
    at = at.cpu().numpy()
    pos += np.asarray([c[0] for c in chunks], dtype=np.int64)[np.searchsorted(row0, at, side="right") - 1]
    runs = []
    for r, p in zip(at.tolist(), pos.tolist()):                  # one turn per change of chromosome (and per chunk)
        name = _name_at(a, p)
        if runs and runs[-1][0] == name:                         # a chunk's first row carries on the chromosome before it
            continue
        if name.lower() in NOT_TEXT:
            raise NotStrict("a chromosome name pandas does not keep as text (%s)" % name, r)
        if runs:
            runs[-1][2] = r
        runs.append([name, r, R])
    return runs


def read_scores_device(path, chunk_bytes=CHUNK_BYTES, timings=None, inflate="host"):
    """-> (x int32 [R, S] device tensor, start int64 [R], end int64 [R] host arrays, runs [(chromosome, row0, row1)]); raises
    NotStrict.  `timings` (a dict) receives inflate_s (the file to text), count_s (chunk cutting and row counts), upload_parse_ms (HIP events
    around all chunks) and coords_s.
    inflate "gpu": a BGZF file is inflated on the device (_read_scores_inflated: the compressed bytes are uploaded, the text never
    exists on the host); timings then also receives index_s, upload_inflate_ms and newline_index_ms, and inflate_s is the device
    path's wall time up to its synchronisation.  Any other file, and a file of which the device gives up a member, is read as
    with "host"."""
    import torch
    from time import perf_counter
    from . import engine
    engine.require_gpu()
    if inflate not in INFLATE_CHOICES:
        raise ValueError("inflate must be one of %s, not %r" % (", ".join(INFLATE_CHOICES), inflate))
    if inflate == "gpu":
        got = _read_scores_inflated(path, chunk_bytes, timings)
        if got is not None:
            return got
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
        R = int(row0[-1])
        if timings is not None:
            timings["count_s"] = perf_counter() - t0
        dev = torch.device("cuda", torch.cuda.current_device())
        cap = max(hi - lo for lo, hi in chunks)
        pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(min(2, len(chunks)))]
        dtext = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in pinned]
        copied = [torch.cuda.Event() for _ in pinned]
        parsed = [torch.cuda.Event() for _ in pinned]
        main, copy = torch.cuda.current_stream(), torch.cuda.Stream()

        def texts(parse):                                        # chunk k + 1 is staged and uploaded while chunk k parses
            for k, (lo, hi) in enumerate(chunks):
                s, n = k % 2, hi - lo
                if k >= 2:
                    copied[s].synchronize()                      # the pinned buffer's last upload has left it
                pinned[s].numpy()[:n] = a[lo:hi]
                with torch.cuda.stream(copy):
                    if k >= 2:
                        copy.wait_event(parsed[s])               # the device buffer's last parse is done
                    dtext[s][:n].copy_(pinned[s][:n], non_blocking=True)
                    copied[s].record(copy)
                main.wait_event(copied[s])
                parse(k, dtext[s])
                parsed[s].record(main)
        x, start, end, chrom_at = _parse_chunks(dev, chunks, rows, row0, F, texts, timings)      # (ends with the one synchronisation)
        t0 = perf_counter()
        runs = _runs_of(a, chrom_at, chunks, row0, R)
        start, end = start.cpu().numpy(), end.cpu().numpy()
        if timings is not None:
            timings["coords_s"] = perf_counter() - t0
    return x, start, end, [tuple(r) for r in runs]
