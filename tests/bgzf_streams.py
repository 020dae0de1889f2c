"""DEFLATE streams and BGZF members for the inflater's tests, made with zlib and by hand: the streams of tests/bgzf_inflate_check.cpp,
restated in Python so that the GPU tests run the device on what the host program has passed.  A Member is (payload, isize, crc): the
raw DEFLATE bytes and the trailer's two fields."""
import collections
import struct
import zlib

import numpy as np

Member = collections.namedtuple("Member", "payload isize crc")

# enum Reason of csrc/epg_bgzf_inflate_block.h
(OK, E_ROW, E_BTYPE, E_STORED_LEN, E_OVERSUBSCRIBED, E_INCOMPLETE, E_REPEAT_FIRST, E_REPEAT_RUN, E_LITLEN_SYM, E_DIST_SYM, E_DIST_FAR, E_OUTPUT,
 E_BITS, E_CRC, E_ISIZE, E_CODE, E_HEADER, E_TRAILING) = range(18)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def member_of(payload, text):
    return Member(bytes(payload), len(text), zlib.crc32(text))


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out = c.compress(text[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) if flush_at else b""
    return member_of(out + c.compress(text[flush_at:]) + c.flush(), text)


def wrap(m):
    """A Member as the bytes of a BGZF member."""
    bsize = 18 + len(m.payload) + 8
    return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", bsize - 1) + m.payload
            + struct.pack("<II", m.crc, m.isize))


def score_text(rows, seed=1, states=18):
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((rows, states)) < 0.4, 0.0, rng.normal(0, 1.5, (rows, states)))
    return "".join("chr%d\t%d\t%d\t%s\n" % (1 + r // 5000, 9800 + 200 * r, 10000 + 200 * r, "\t".join("%.5f" % v for v in x[r])) for r in range(rows)).encode()


def fibonacci_text(symbols=22, seed=2):
    a, b, parts = 1, 1, []
    for s in range(symbols):
        parts.append(bytes([65 + s]) * a)
        a, b = b, a + b
    t = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    np.random.default_rng(seed).shuffle(t)
    return t.tobytes()


class BitW:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, c, n):                                                      # a Huffman code: most significant bit first
        self.bits += [(c >> i) & 1 for i in range(n - 1, -1, -1)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return np.packbits(np.asarray(b, dtype=np.uint8), bitorder="little").tobytes() if b else b""


def canon(lens):
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, c = [0] * 16, 0
    for l in range(1, 16):
        c = (c + cnt[l - 1]) << 1
        nxt[l] = c
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return codes


class Hand:
    """A dynamic block by hand.  The code-length code of every header: symbols 0 .. 12 in four bits, 13 .. 18 in five (complete)."""

    def __init__(self, llen, dlen=None, hlit=257, hdist=1):
        self.w = BitW()
        self.llen = [0] * 288
        self.dlen = [0] * 32
        for k, v in llen.items():
            self.llen[k] = v
        for k, v in (dlen or {}).items():
            self.dlen[k] = v
        self.hlit, self.hdist = hlit, hdist
        self.cllen = [4 if i < 13 else 5 for i in range(19)]
        self.clcode = canon(self.cllen)
        self.lcode, self.dcode = canon(self.llen), canon(self.dlen)

    def cl(self, s):
        self.w.code(self.clcode[s], self.cllen[s])

    def header(self, bfinal, first16=False, hdist_field=None, lengths=True):
        w = self.w
        w.put(bfinal, 1)
        w.put(2, 2)
        w.put(self.hlit - 257, 5)
        w.put((self.hdist if hdist_field is None else hdist_field) - 1, 5)
        w.put(15, 4)
        for k in range(19):
            w.put(self.cllen[CL_ORDER[k]], 3)
        if first16:
            self.cl(16)
            w.put(0, 2)
        for i in range(self.hlit):
            self.cl(self.llen[i])
        if lengths:
            for i in range(self.hdist):
                self.cl(self.dlen[i])
        return self

    def lit(self, s):
        self.w.code(self.lcode[s], self.llen[s])
        return self

    def dist(self, s):
        self.w.code(self.dcode[s], self.dlen[s])
        return self


def fixed_lit(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed(symbols):
    """One final fixed block of ("l", literal/length symbol) and ("d", distance symbol) items."""
    w = BitW()
    w.put(1, 1)
    w.put(1, 2)
    for kind, s in symbols:
        if kind == "l":
            fixed_lit(w, s)
        else:
            w.code(s, 5)
    return w.bytes()


def good_members(text):
    """name -> (Member, its text): every kind of valid stream of the host program.  `text` is at most 65 280 bytes of score text."""
    A = ord("a")
    out = {}
    for level in (1, 6, 9):
        out["level %d" % level] = (deflate(text, level), text)
    out["Z_FIXED"] = (deflate(text, 6, zlib.Z_FIXED), text)
    out["Z_HUFFMAN_ONLY"] = (deflate(text, 6, zlib.Z_HUFFMAN_ONLY), text)
    out["stored"] = (deflate(text, 0), text)
    out["full flush"] = (deflate(text, 6, flush_at=len(text) // 2 + 1), text)
    t = b"x" * 65536
    out["65536 equal bytes"] = (deflate(t), t)
    half = np.random.default_rng(3).integers(0, 256, 32000, dtype=np.uint8).tobytes()
    out["period 32000"] = (deflate(half + half, 9), half + half)              # (zlib itself never reaches back more than 32 506 bytes)
    half = np.random.default_rng(3).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    t = half + (half + half)[:127 * 258]                                       # by hand: a stored block, then 127 matches of 258 bytes at distance 32 768
    w = BitW()
    w.put(1, 1)
    w.put(1, 2)
    for _ in range(127):
        fixed_lit(w, 285)
        w.code(29, 5)
        w.put(8191, 13)
    fixed_lit(w, 256)
    out["distance 32768"] = (member_of(b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + half + w.bytes(), t), t)
    t = fibonacci_text()
    out["fibonacci"] = (deflate(t, 6, zlib.Z_HUFFMAN_ONLY), t)
    t = np.random.default_rng(4).integers(0, 256, 3000, dtype=np.uint8).tobytes()
    out["literals only"] = (deflate(t), t)
    out["one byte"] = (deflate(b"q"), b"q")
    out["zero bytes"] = (deflate(b""), b"")
    out["end-of-file block"] = (Member(b"\x03\x00", 0, 0), b"")
    t = (score_text(700, seed=5) * 2)[:65536]
    out["65536 bytes"] = (deflate(t), t)
    t = text[:65280].ljust(65280, b"\n")
    out["65280 bytes"] = (deflate(t), t)
    aaaa = b"a" * 121
    h = Hand({A: 1, 256: 2, 257: 2}, {0: 1}, hlit=258).header(1).lit(A)
    for _ in range(40):
        h.lit(257).dist(0)
    out["single distance code"] = (member_of(h.lit(256).w.bytes(), aaaa), aaaa)
    h = Hand({A: 1, 256: 1}).header(0)
    for _ in range(60):
        h.lit(A)
    h.lit(256).header(1)
    for _ in range(61):
        h.lit(A)
    out["no distance code"] = (member_of(h.lit(256).w.bytes(), aaaa), aaaa)
    out["end-of-block code alone"] = (member_of(Hand({256: 1}).header(1).lit(256).w.bytes(), b""), b"")
    return out


def bad_members(text):
    """name -> (Member, the reason the inflater must give): every corruption of the host program, each by a known edit."""
    A = ord("a")
    out = {}
    w = BitW()
    w.put(1, 1)
    w.put(3, 2)
    out["block type 3"] = (member_of(w.bytes(), b""), E_BTYPE)
    m = deflate(text, 0)
    out["LEN / NLEN"] = (m._replace(payload=m.payload[:3] + bytes([m.payload[3] ^ 1]) + m.payload[4:]), E_STORED_LEN)
    out["over-subscribed"] = (member_of(Hand({A: 1, A + 1: 1, 256: 1}).header(1).w.bytes(), b""), E_OVERSUBSCRIBED)
    out["incomplete"] = (member_of(Hand({A: 2, 256: 2}).header(1).lit(256).w.bytes(), b""), E_INCOMPLETE)
    out["incomplete distances"] = (member_of(Hand({A: 1, 256: 1}, {0: 2, 1: 2}, hdist=2).header(1).lit(256).w.bytes(), b""), E_INCOMPLETE)
    out["repeat first"] = (member_of(Hand({A: 1, 256: 1}).header(1, first16=True).w.bytes(), b""), E_REPEAT_FIRST)
    h = Hand({A: 1, 256: 1}).header(1, hdist_field=30, lengths=False)          # 287 lengths promised, 257 given, then 138 zeros
    h.cl(18)
    h.w.put(127, 7)
    out["run past the lengths"] = (member_of(h.w.bytes(), b""), E_REPEAT_RUN)
    for s in (286, 287):
        out["symbol %d" % s] = (member_of(fixed([("l", A), ("l", s), ("d", 0), ("l", 256)]), b"a"), E_LITLEN_SYM)
    for s in (30, 31):
        out["distance symbol %d" % s] = (member_of(fixed([("l", A), ("l", 257), ("d", s), ("l", 256)]), b"aaaa"), E_DIST_SYM)
    out["distance too far"] = (member_of(fixed([("l", A), ("l", 257), ("d", 1), ("l", 256)]), b"aaaa"), E_DIST_FAR)
    m = deflate(text, 6)
    out["output beyond ISIZE"] = (Member(m.payload, m.isize - 1, zlib.crc32(text[:-1])), E_OUTPUT)
    out["fewer bytes than ISIZE"] = (m._replace(isize=m.isize + 1), E_ISIZE)
    out["CRC-32"] = (m._replace(crc=m.crc ^ 0x10000), E_CRC)
    out["bits past the payload"] = (m._replace(payload=m.payload[:-1]), E_BITS)
    out["half the payload"] = (m._replace(payload=m.payload[:len(m.payload) // 2]), E_BITS)
    out["a byte behind the stream"] = (m._replace(payload=m.payload + b"\0"), E_TRAILING)
    h = Hand({A: 1, 256: 2, 257: 2}, {0: 1}, hlit=258).header(1).lit(A).lit(257)
    h.w.put(1, 1)
    h.lit(256).w.put(0, 16)
    out["no such distance code"] = (member_of(h.w.bytes(), b"aaaa"), E_CODE)
    return out


def write_members(path, members):
    """[(Member, reason wanted)] as the file `bgzf_inflate_check --members` reads."""
    with open(path, "wb") as f:
        for m, want in members:
            f.write(struct.pack("<IIII", len(m.payload), m.isize, m.crc, want) + m.payload)
