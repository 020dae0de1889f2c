"""The member chain of a BGZF file, for the device inflater (csrc/epg_bgzf_inflate.h): members(path) walks the gzip members' headers and
trailers through a memory map and returns the table epgz_bgzf_inflate takes -- a row per member: where its raw DEFLATE payload lies in
the file, its bytes, where its text goes, ISIZE and CRC-32.  Nothing is inflated and no field is trusted before it was checked: the
file is BGZF "all the way" by the format's own description (SAM specification, section 4.1), or the answer is None and the caller
inflates on the host.  Accepted is what the project's own writers produce (EPILOGOS_BGZF=1, --writer gpu, simsearch.bed.gz) and
what bgzip writes: every member starts with the gzip magic, the deflate method and FEXTRA alone, its extra field is exactly the one
'BC' subfield of length 2, BSIZE stays inside the file and leaves room for header and trailer, ISIZE is at most 65 280, and no byte
follows the last member.  An end-of-file block (an empty member) may stand anywhere, or be missing."""
import mmap
import struct

import numpy as np

MAX_MEMBER = 65536
MAX_TEXT = 65280
HEADER = 18
TRAILER = 8
COLS = 5                    # payload offset, payload bytes, text offset, ISIZE, CRC-32
_FIXED = struct.Struct("<HBBIBBH2sHH")


def walk(buf):
    """members() of a bytes-like object: (int64 [M, 5] table, total text bytes) or None."""
    n = len(buf)
    rows, at, text = [], 0, 0
    while at < n:
        if n - at < HEADER + 2 + TRAILER:
            return None
        magic, method, flg, _mtime, _xfl, _os, xlen, si, slen, bsize = _FIXED.unpack_from(buf, at)
        if magic != 0x8b1f or method != 8 or flg != 4 or xlen != 6 or si != b"BC" or slen != 2:
            return None
        bsize += 1
        if bsize < HEADER + 2 + TRAILER or at + bsize > n:
            return None
        crc, isize = struct.unpack_from("<II", buf, at + bsize - TRAILER)
        if isize > MAX_TEXT:
            return None
        rows.append((at + HEADER, bsize - HEADER - TRAILER, text, isize, crc))
        text += isize
        at += bsize
    return np.asarray(rows, dtype=np.int64).reshape(-1, COLS), text


def members(path_or_buffer):
    """(table int64 [M, 5], total text bytes) of a BGZF file (a path) or buffer (bytes, bytearray, memoryview, uint8 array), None
    when it is not BGZF from its first byte to its last: plain gzip, text, an empty file, a damaged chain."""
    if isinstance(path_or_buffer, (bytes, bytearray, memoryview)):
        return walk(path_or_buffer)
    if isinstance(path_or_buffer, np.ndarray):
        return walk(memoryview(np.ascontiguousarray(path_or_buffer, dtype=np.uint8)).cast("B"))
    with open(path_or_buffer, "rb") as f:
        head = f.read(4)
        if not head:
            return walk(b"")
        if head != b"\x1f\x8b\x08\x04":                          # (before a map is made of a file that is something else)
            return None
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
            return walk(m)
