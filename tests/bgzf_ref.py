"""A strict walker of BGZF streams for the writer tests: structure only, by the format's own description (SAM specification, section
4.1).  It inflates nothing and trusts no field it has not checked; the payload it returns goes to gzip / zlib / the library's own
inflaters in the tests."""
import collections
import struct

Member = collections.namedtuple("Member", "bsize isize crc payload")

EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MAX_MEMBER = 65536
MAX_TEXT = 65280


class BgzfError(ValueError):
    pass


def members(data):
    """The members of `data` as Member(BSIZE, ISIZE, CRC-32, raw DEFLATE payload), whatever the stream ends with.  Raises BgzfError
    on: a member that does not start with the gzip magic, deflate method and FEXTRA alone; an extra field that is not exactly the
    one 'BC' subfield of length 2; a BSIZE that reaches beyond the data, or leaves no room for header and trailer; an ISIZE above
    65 280; bytes behind the last member."""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 28:
            raise BgzfError("%d stray bytes at offset %d" % (len(data) - at, at))
        magic, method, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<HBBIBBH", data, at)
        if magic != 0x8b1f or method != 8 or flg != 4:
            raise BgzfError("offset %d: not a BGZF member header" % at)
        if xlen != 6 or data[at + 12:at + 14] != b"BC" or struct.unpack_from("<H", data, at + 14)[0] != 2:
            raise BgzfError("offset %d: the extra field is not the one BC subfield" % at)
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        if bsize < 18 + 2 + 8 or bsize > MAX_MEMBER:
            raise BgzfError("offset %d: BSIZE %d is impossible" % (at, bsize))
        if at + bsize > len(data):
            raise BgzfError("offset %d: BSIZE %d reaches beyond the data" % (at, bsize))
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        if isize > MAX_TEXT:
            raise BgzfError("offset %d: ISIZE %d above %d" % (at, isize, MAX_TEXT))
        out.append(Member(bsize, isize, crc, data[at + 18:at + bsize - 8]))
        at += bsize
    return out


def walk(data, eof=True):
    """members(data) of a finished file: additionally raises unless the stream ends in exactly one end-of-file block (the empty
    28-byte member) and holds no other empty member.  eof=False: a part that is to be concatenated -- no empty member at all."""
    ms = members(data)
    empty = [k for k, m in enumerate(ms) if m.isize == 0]
    if eof:
        if not ms or bytes(data)[-28:] != EOF:
            raise BgzfError("the end-of-file block is missing")
        if empty != [len(ms) - 1]:
            raise BgzfError("%d empty members, wanted the one at the end" % len(empty))
    elif empty:
        raise BgzfError("an empty member in a stream that is to be concatenated")
    return ms
