"""Hostile text for the device BGZF compressor (csrc/epg_bgzf_block.h), and what it must make of it.

expected_tokens restates the matching rule from the comment at the top of that header (not from its `walk`): at a position p of row r
the candidate is p - d, d = the length of row r - 1; a match is tried only for 1 <= d <= 32768 and p - d >= the block's start; it is
at most 258 bytes and never passes the row's end or the block's; 6 bytes or more are a match, anything else one literal.  Row offsets
are clamped into [0, n], row 0 at 0 and row R at n.  Nothing here knows how rows are dealt to threads: that the tokens do not depend
on it is part of what the tests hold the device to.

The builders are deterministic; each returns (bytes, int64 row offsets or None)."""
import numpy as np

BLOCK = 65280
MINM = 6
ALPHABET = np.frombuffer(b"0123456789.-\tchr", dtype=np.uint8)


def clamp_offsets(row_off, n):
    off = np.clip(np.asarray(row_off, dtype=np.int64), 0, n)
    off[0], off[-1] = 0, n
    return off


def expected_tokens(text, row_off, B0, B1):
    """The token list of the block text[B0:B1]: ints (literals) and (length, distance) tuples.  row_off None: literals alone."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(t)
    assert 0 <= B0 <= B1 <= n
    if row_off is None or B0 == B1:
        return t[B0:B1].tolist()
    off = clamp_offsets(row_off, n)
    if (np.diff(off) < 0).any():
        raise ValueError("row offsets out of order: the block is stored, there are no tokens to expect")
    p = np.arange(B0, B1, dtype=np.int64)
    r = np.searchsorted(off, p, side="right") - 1                               # the row that holds p (empty rows hold nothing)
    above = np.concatenate([[0], np.diff(off)])[r]                             # d: the length of row r - 1; row 0 has none
    row_end = np.minimum(off[r + 1], B1)
    tried = (above >= 1) & (above <= 32768) & (p - above >= B0)
    equal = np.zeros(len(p), dtype=bool)
    equal[tried] = t[p[tried]] == t[p[tried] - above[tried]]
    # run[i]: how many bytes from p[i] on are equal to their candidates, within the row
    stop = np.where(equal, B1, p)                                               # the first position at or behind p[i] that is not equal
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    run = (np.minimum(stop, row_end) - p).tolist()
    lit, dist = t[B0:B1].tolist(), above.tolist()
    out, i, m = [], 0, len(p)
    while i < m:
        L = run[i]
        if L >= MINM:
            L = min(L, 258)
            out.append((L, dist[i]))
            i += L
        else:
            out.append(lit[i])
            i += 1
    return out


def block_ranges(n):
    return [(B0, min(B0 + BLOCK, n)) for B0 in range(0, n, BLOCK)]


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def _other(rng, byte):
    """A letter of the alphabet that is not `byte`."""
    k = int(np.flatnonzero(ALPHABET == byte)[0]) if byte in ALPHABET else 0
    return int(ALPHABET[(k + 1 + int(rng.integers(0, 15))) % 16])


# lengths whose row the first block's border cuts (row 217: 222 bytes wanted, 180 left) or leaves without a source (row 218): the
# ladder ends with a second row for each, so that every length 6 .. 258 is emitted whole
LADDER_AGAIN = (222, 223)


def ladder_lengths(seed=21):
    """A row of 300 random letters, then a row of 300 for every L in 6 .. 258: its first L bytes copy the row above, every later byte
    differs from the byte 300 before it.  One match of exactly L per row."""
    rng = np.random.default_rng(seed)
    rows = [ALPHABET[rng.integers(0, 16, 300)].copy()]
    for L in list(range(6, 259)) + list(LADDER_AGAIN):
        up = rows[-1]
        row = up.copy()
        for k in range(L, 300):
            row[k] = _other(rng, up[k])
        rows.append(row)
    return np.concatenate(rows).tobytes(), _offsets([300] * len(rows))


def ladder_distance_list():
    """Both ends of every distance symbol's range, then two distances DEFLATE cannot code."""
    ds = [1, 2, 3, 4]
    for sym in range(4, 30):
        nb = sym // 2 - 1
        lo = 1 + ((2 + (sym & 1)) << nb)
        ds += [lo, lo + (1 << nb) - 1]
    return ds + [32769, 40000]


def ladder_distances(seed=22):
    """For every d of ladder_distance_list: a row of d bytes with no match (every byte differs from the one 40 before it), then a row
    of 40 bytes that is one 40-byte match against it -- for d < 40 the source repeats with period d, so the match overlaps itself."""
    rng = np.random.default_rng(seed)
    ds = ladder_distance_list()
    total = sum(ds) + 40 * len(ds)
    t = ALPHABET[rng.integers(0, 16, total)].copy()
    shift = rng.integers(1, 16, total)
    index = np.full(256, 0, dtype=np.int64)
    index[ALPHABET] = np.arange(16)
    lengths, at = [], 0
    for d in ds:
        if at:                                                                  # the row above is 40 bytes: differ from the byte 40 before
            for p in range(at, at + d, 40):                                     # (40 at a time: their sources are written already)
                q = min(p + 40, at + d)
                t[p:q] = ALPHABET[(index[t[p - 40:q - 40]] + shift[p:q]) % 16]
        at += d
        for p in range(at, at + 40):
            t[p] = t[p - d]
        at += 40
        lengths += [d, 40]
    assert at == total
    return t.tobytes(), _offsets(lengths)


def chain(seed=23):
    """Byte k = 0 .. 20 occurs F(k + 2) times (1, 2, 3, 5, 8, ...), shuffled: with the end-of-block symbol the weights are the Fibonacci
    numbers 1, 1, 2, 3, 5, ..., whose Huffman tree is a chain 21 deep."""
    a, b, parts = 1, 2, []
    for k in range(21):
        parts.append(np.full(a, k, dtype=np.uint8))
        a, b = b, a + b
    t = np.concatenate(parts)
    assert len(t) == 46366
    np.random.default_rng(seed).shuffle(t)
    return t.tobytes(), None


DYADIC = {4: 6, 5: 12, 6: 5, 7: 16, 8: 5, 9: 7, 10: 1, 11: 16, 13: 1, 14: 1, 15: 153}


def dyadic(seed=24):
    """223 byte values, each 2^(15 - L) times for the code length L it must get (DYADIC: how many values per L; the end-of-block symbol
    takes the last slot of 15 bits): the literal code is exactly 15 deep with nothing to cut, and the histogram of its lengths
    ([0,2,0,0,6,12,5,16,5,7,1,16,0,1,1,154,0,0,1] with the distance code's two and the run of zeros) needs a code-length code 8 deep."""
    parts, v = [], 0
    for L, count in DYADIC.items():
        for _ in range(count):
            parts.append(np.full(1 << (15 - L), v, dtype=np.uint8))
            v += 1
    t = np.concatenate(parts)
    assert v == 223 and len(t) == 32767
    np.random.default_rng(seed).shuffle(t)
    return t.tobytes(), None


def one_byte_rows(seed=25, rows=70000):
    """Rows of one byte, two in three equal to the row above: 65 280 rows in a block, and nothing to match (a row ends after 1 byte)."""
    rng = np.random.default_rng(seed)
    t = ALPHABET[rng.integers(0, 16, rows)].copy()
    same = rng.random(rows) < 2 / 3
    for r in range(1, rows):
        if same[r]:
            t[r] = t[r - 1]
    return t.tobytes(), np.arange(rows + 1, dtype=np.int64)


def long_rows(seed=26):
    """Three equal rows of 50 000 bytes (no distance fits), five equal rows of 32 768 (d = 32768: a match wherever p - d is not before
    the block's start).  Every block has one to three rows: most threads idle."""
    rng = np.random.default_rng(seed)
    a, b = ALPHABET[rng.integers(0, 16, 50000)], ALPHABET[rng.integers(0, 16, 32768)]
    return np.concatenate([a] * 3 + [b] * 5).tobytes(), _offsets([50000] * 3 + [32768] * 5)


def empty_rows(seed=27, rows=3000):
    """Rows in fours: 57 random letters, the same 57 again (a match), an empty row, 57 random letters whose d is 0."""
    rng = np.random.default_rng(seed)
    parts = []
    for r in range(rows):
        if r % 4 == 1:
            parts.append(parts[-1])
        elif r % 4 == 2:
            parts.append(np.zeros(0, dtype=np.uint8))
        else:
            parts.append(ALPHABET[rng.integers(0, 16, 57)])
    return np.concatenate(parts).tobytes(), _offsets([len(x) for x in parts])


def border(pad=0, seed=28, rows=652):
    """Equal rows of 300 bytes over three blocks (65 280 is no multiple of 300), behind a leading row of `pad` bytes.  pad = 180: a
    row starts exactly at the second block's start, so the row behind it matches from its first byte; pad = 179: that source
    starts one byte before the block, and the first byte of the row behind it is a literal."""
    rng = np.random.default_rng(seed)
    row = ALPHABET[rng.integers(0, 16, 300)]
    lead = [ALPHABET[rng.integers(0, 16, pad)]] if pad else []
    return np.concatenate(lead + [row] * rows).tobytes(), _offsets([pad] * bool(pad) + [300] * rows)


def hostile_offsets(text, row_off, seed=29):
    """Every seventh offset replaced by a value from [-50, n + 50]: the first by -50, the second by n + 50, the others at random."""
    rng = np.random.default_rng(seed)
    off = np.array(row_off, dtype=np.int64)
    for k, i in enumerate(range(1, len(off) - 1, 7)):
        off[i] = (-50, len(text) + 50)[k] if k < 2 else int(rng.integers(0, len(text) + 101)) - 50
    return off


# ---- what a code must cost -------------------------------------------------------------------------------------------------------------
def huffman_depths(freq):
    """{symbol: depth} of a Huffman tree over the symbols with freq != 0 (heapq; a leaf before an internal node of equal weight, then
    the lower symbol / the older node).  The depths depend on that tie rule, their cost sum(freq * depth) does not."""
    import heapq
    heap = [(f, 0, s, (s,)) for s, f in enumerate(freq) if f]
    if len(heap) < 2:
        return {h[2]: 1 for h in heap}
    heapq.heapify(heap)
    depth = {h[2]: 0 for h in heap}
    made = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            depth[s] += 1
        made += 1
        heapq.heappush(heap, (a[0] + b[0], 1, made, a[3] + b[3]))
    return depth


def optimal_cost(freq):
    return sum(freq[s] * d for s, d in huffman_depths(freq).items())


def token_histograms(tokens, length_symbol, distance_symbol):
    """(literal/length histogram [286] with the end-of-block symbol counted, distance histogram [30], extra bits) of a token list."""
    ll, dd, extra = [0] * 286, [0] * 30, 0
    for t in tokens:
        if isinstance(t, tuple):
            s, e = length_symbol(t[0])
            ll[s] += 1
            extra += e
            s, e = distance_symbol(t[1])
            dd[s] += 1
            extra += e
        else:
            ll[t] += 1
    ll[256] += 1
    return ll, dd, extra


def code_length_histogram(llen, dlen):
    """How often each of the 19 code-length symbols occurs when llen + dlen is written with runs of zeros as 17 (3 .. 10) and 18
    (11 .. 138) and every other length as itself: the header comment's "code-length code over the lengths with runs of zeros coded
    as 17 / 18"."""
    seq, hist, i = list(llen) + list(dlen), [0] * 19, 0
    while i < len(seq):
        run = 1
        if seq[i] == 0:
            while i + run < len(seq) and run < 138 and seq[i + run] == 0:
                run += 1
            if run >= 11:
                hist[18] += 1
            elif run >= 3:
                hist[17] += 1
            else:
                hist[0] += run
        else:
            hist[seq[i]] += 1
        i += run
    return hist
