"""An independent judge of DEFLATE payloads for the compressor's tests: a decoder written from RFC 1951 alone, which returns not only
the bytes but what the encoder chose -- every block's type, HLIT / HDIST / HCLEN, the three code-length arrays and the token list.
It imports none of the project's inflaters or tables; tests/test_bgzf_hostile_host.py holds it against zlib.

    text, blocks = decode(payload)          # payload: one raw DEFLATE stream, such as bgzf_ref.Member.payload

A literal token is an int, a match the tuple (length, distance).  DeflateError on: a reserved block type, LEN / NLEN that disagree,
an over-subscribed code, an incomplete code (other than RFC 1951's one distance code of one bit, which zlib also takes for the
literal/length code, and no distance code at all), a repeat with nothing before it or past HLIT + HDIST, a missing end-of-block
code, a bit pattern or symbol (286, 287, 30, 31) that is no code, a distance before the start, length 258 written as symbol 284 + 31, bits beyond the payload, bytes left
over behind the final block."""
import collections

Block = collections.namedtuple("Block", "btype hlit hdist hclen cllen llen dlen tokens")

STORED, FIXED, DYNAMIC = 0, 1, 2
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951, 3.2.5: symbol 257 + i has LEN_BASE[i] and LEN_EXTRA[i] extra bits, distance symbol i DIST_BASE[i] and DIST_EXTRA[i]
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
PAD = 8


class DeflateError(ValueError):
    pass


def length_symbol(L):
    """(symbol, extra bits) of a match length 3 .. 258: the last symbol whose base is not above L (258 is symbol 285 alone)."""
    if not 3 <= L <= 258:
        raise ValueError("no match length: %d" % L)
    i = max(k for k in range(29) if LEN_BASE[k] <= L)
    assert L - LEN_BASE[i] < (1 << LEN_EXTRA[i])
    return 257 + i, LEN_EXTRA[i]


def distance_symbol(d):
    if not 1 <= d <= 32768:
        raise ValueError("no distance: %d" % d)
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    assert d - DIST_BASE[i] < (1 << DIST_EXTRA[i])
    return i, DIST_EXTRA[i]


def kraft(lens):
    """Sum of 2^-len over the used symbols, as (numerator over 2^15)."""
    return sum(1 << (15 - l) for l in lens if l)


def _table(lens, what, none_ok=False):
    """(table, bits): table[the next `bits` bits of the stream] = symbol * 16 + code length, -1 where no code begins so."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    used = len(lens) - count[0]
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise DeflateError("%s code: over-subscribed" % what)
    if left > 0 and not ((used == 0 and none_ok) or (used == 1 and count[1] == 1)):
        raise DeflateError("%s code: incomplete" % what)
    bits = max(max(lens), 1) if lens else 1
    table = [-1] * (1 << bits)
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1] * (l > 1)) << 1
        nxt[l] = code
    for s, l in enumerate(lens):
        if not l:
            continue
        c, nxt[l] = nxt[l], nxt[l] + 1
        r = int(format(c, "0%db" % l)[::-1], 2)                                # Huffman codes are packed most significant bit first
        for k in range(r, 1 << bits, 1 << l):
            table[k] = s * 16 + l
    return table, bits


_FIXED_L = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32


def decode(payload):
    """-> (bytes, [Block]).  Stored blocks have no codes and the single token list of their bytes as literals."""
    n = len(payload)
    d = bytes(payload) + bytes(PAD)
    try:
        return _decode(d, n)
    except IndexError:
        raise DeflateError("bits beyond the payload") from None


def _decode(d, n):
    out, blocks = bytearray(), []
    acc = nb = at = 0

    final = 0
    while not final:
        while nb < 3:
            acc |= d[at] << nb
            at += 1
            nb += 8
        final, btype = acc & 1, (acc >> 1) & 3
        acc >>= 3
        nb -= 3
        if btype == 3:
            raise DeflateError("block type 3")
        if btype == STORED:
            at -= nb // 8                                                      # back to the byte boundary
            acc = nb = 0
            if at + 4 > n:
                raise DeflateError("bits beyond the payload")
            ln, nln = d[at] | d[at + 1] << 8, d[at + 2] | d[at + 3] << 8
            if ln ^ nln != 0xFFFF:
                raise DeflateError("stored block: LEN and NLEN disagree")
            at += 4
            if at + ln > n:
                raise DeflateError("bits beyond the payload")
            out += d[at:at + ln]
            blocks.append(Block(STORED, None, None, None, None, None, None, list(d[at:at + ln])))
            at += ln
            continue
        if btype == FIXED:
            hlit = hdist = hclen = cllen = None
            llen, dlen = list(_FIXED_L), list(_FIXED_D)
        else:
            while nb < 14:
                acc |= d[at] << nb
                at += 1
                nb += 8
            hlit, hdist, hclen = 257 + (acc & 31), 1 + ((acc >> 5) & 31), 4 + ((acc >> 10) & 15)
            acc >>= 14
            nb -= 14
            if hlit > 286 or hdist > 30:
                raise DeflateError("HLIT %d / HDIST %d" % (hlit, hdist))
            cllen = [0] * 19
            for k in range(hclen):
                while nb < 3:
                    acc |= d[at] << nb
                    at += 1
                    nb += 8
                cllen[CL_ORDER[k]] = acc & 7
                acc >>= 3
                nb -= 3
            ctab, cbits = _table(cllen, "code-length")
            lens = []
            while len(lens) < hlit + hdist:
                while nb < 14:
                    acc |= d[at] << nb
                    at += 1
                    nb += 8
                e = ctab[acc & ((1 << cbits) - 1)]
                if e < 0:
                    raise DeflateError("no such code-length code")
                acc >>= e & 15
                nb -= e & 15
                s = e >> 4
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise DeflateError("repeat with no length before it")
                    v, rep, eb = lens[-1], 3 + (acc & 3), 2
                elif s == 17:
                    v, rep, eb = 0, 3 + (acc & 7), 3
                else:
                    v, rep, eb = 0, 11 + (acc & 127), 7
                acc >>= eb
                nb -= eb
                if len(lens) + rep > hlit + hdist:
                    raise DeflateError("a run past HLIT + HDIST lengths")
                lens += [v] * rep
            llen, dlen = lens[:hlit], lens[hlit:]
            if llen[256] == 0:
                raise DeflateError("no end-of-block code")
        ltab, lbits = _table(llen, "literal/length")
        dtab, dbits = _table(dlen, "distance", none_ok=True)
        lmask, dmask = (1 << lbits) - 1, (1 << dbits) - 1
        tokens = []
        while True:
            while nb < 20:                                                     # a code of 15 bits and the length's 5 extra bits
                acc |= d[at] << nb
                at += 1
                nb += 8
            e = ltab[acc & lmask]
            if e < 0:
                raise DeflateError("no such literal/length code")
            acc >>= e & 15
            nb -= e & 15
            s = e >> 4
            if s < 256:
                tokens.append(s)
                out.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise DeflateError("literal/length symbol %d" % s)
            eb = LEN_EXTRA[s - 257]
            L = LEN_BASE[s - 257] + (acc & ((1 << eb) - 1))
            if s == 284 and L == 258:
                raise DeflateError("length 258 as symbol 284: RFC 1951 gives it 227 .. 257, 258 is symbol 285")
            acc >>= eb
            nb -= eb
            while nb < 28:                                                     # 15 bits and 13 extra
                acc |= d[at] << nb
                at += 1
                nb += 8
            e = dtab[acc & dmask]
            if e < 0:
                raise DeflateError("no such distance code")
            acc >>= e & 15
            nb -= e & 15
            s = e >> 4
            if s > 29:
                raise DeflateError("distance symbol %d" % s)
            eb = DIST_EXTRA[s]
            dist = DIST_BASE[s] + (acc & ((1 << eb) - 1))
            acc >>= eb
            nb -= eb
            if dist > len(out):
                raise DeflateError("distance %d before the start (%d bytes so far)" % (dist, len(out)))
            tokens.append((L, dist))
            if dist >= L:
                out += out[len(out) - dist:len(out) - dist + L]
            else:
                for _ in range(L):
                    out.append(out[-dist])
        if (8 * at - nb) > 8 * n:
            raise DeflateError("bits beyond the payload")
        blocks.append(Block(btype, hlit, hdist, hclen, cllen, llen, dlen, tokens))
    if (8 * at - nb) > 8 * n:
        raise DeflateError("bits beyond the payload")
    if ((8 * at - nb) + 7) // 8 != n:
        raise DeflateError("%d bytes left over behind the final block" % (n - ((8 * at - nb) + 7) // 8))
    return bytes(out), blocks


def expand(blocks):
    """The bytes that the token lists alone stand for."""
    out = bytearray()
    for b in blocks:
        for t in b.tokens:
            if isinstance(t, tuple):
                L, dist = t
                if dist > len(out):
                    raise DeflateError("distance %d before the start" % dist)
                for _ in range(L):
                    out.append(out[-dist])
            else:
                out.append(t)
    return bytes(out)
