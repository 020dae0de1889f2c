"""CPU: the judge and the inputs of tests/test_hip_bgzf_hostile.py, held to references before the device sees them.
tests/deflate_tokens.py against zlib (bytes, and token lists that expand to the same bytes) and against the corrupt members of
tests/bgzf_streams.py; the builders of tests/bgzf_hostile.py against the properties they are there for, computed with a heapq
Huffman and expected_tokens alone.  The compressor's own phases run on the same families in tests/bgzf_block_check.cpp
(tests/test_writer_host.py builds and runs it under the sanitizers)."""
import zlib

import numpy as np
import pytest

from tests import bgzf_hostile as bh
from tests import bgzf_streams as bs
from tests import deflate_tokens as dt

TEXTS = {"score text": bs.score_text(300), "fibonacci": bs.fibonacci_text(), "random bytes": np.random.default_rng(31).integers(0, 256, 5000, dtype=np.uint8).tobytes()}
SETTINGS = {"level 0": (0, zlib.Z_DEFAULT_STRATEGY), "level 1": (1, zlib.Z_DEFAULT_STRATEGY), "level 6": (6, zlib.Z_DEFAULT_STRATEGY),
            "level 9": (9, zlib.Z_DEFAULT_STRATEGY), "Z_FIXED": (6, zlib.Z_FIXED), "Z_HUFFMAN_ONLY": (6, zlib.Z_HUFFMAN_ONLY)}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(TEXTS))
def test_the_decoder_reproduces_zlib(name, setting):
    text = TEXTS[name]
    level, strategy = SETTINGS[setting]
    payload = bs.deflate(text, level, strategy).payload
    assert zlib.decompressobj(-15).decompress(payload) == text
    got, blocks = dt.decode(payload)
    assert got == text and dt.expand(blocks) == text
    kinds = {b.btype for b in blocks}
    if setting == "level 0":
        assert kinds == {dt.STORED}
    if setting == "Z_FIXED":
        assert kinds == ({dt.STORED} if name == "random bytes" else {dt.FIXED})    # (zlib stores what a fixed code would inflate)
    if setting == "Z_HUFFMAN_ONLY":
        assert all(not isinstance(t, tuple) for b in blocks for t in b.tokens)
    if setting in ("level 6", "level 9") and name == "score text":
        assert kinds == {dt.DYNAMIC} and any(isinstance(t, tuple) for b in blocks for t in b.tokens)
    for b in blocks:
        if b.btype == dt.DYNAMIC:
            assert len(b.llen) == b.hlit and len(b.dlen) == b.hdist and len(b.cllen) == 19 and dt.kraft(b.llen) == 1 << 15


def test_the_decoder_reads_every_valid_member_of_the_inflater_s_tests():
    for name, (m, want) in bs.good_members(bs.score_text(600)[:65280]).items():
        got, blocks = dt.decode(m.payload)
        assert got == want and dt.expand(blocks) == want, name


# the corruptions of bgzf_streams.bad_members that lie in the payload; CRC-32 and ISIZE are the member's, not the stream's
REFUSED = ["block type 3", "LEN / NLEN", "over-subscribed", "incomplete", "incomplete distances", "repeat first", "run past the lengths", "symbol 286",
           "symbol 287", "distance symbol 30", "distance symbol 31", "distance too far", "bits past the payload", "half the payload",
           "a byte behind the stream", "no such distance code"]


@pytest.mark.parametrize("name", REFUSED)
def test_the_decoder_refuses(name):
    bad = bs.bad_members(bs.score_text(600)[:65280])
    assert set(REFUSED) <= set(bad)
    with pytest.raises(dt.DeflateError):
        dt.decode(bad[name][0].payload)


def test_symbol_tables_against_every_length_and_distance():
    """Each length 3 .. 258 and distance 1 .. 32768 lies in exactly one symbol's range, and the ranges tile without a gap."""
    at = 3
    for i in range(28):
        assert dt.LEN_BASE[i] == at
        at += 1 << dt.LEN_EXTRA[i]
    assert at == 259 and dt.length_symbol(258) == (285, 0) and dt.length_symbol(257) == (284, 5) and dt.length_symbol(3) == (257, 0)
    at = 1
    for i in range(30):
        assert dt.DIST_BASE[i] == at
        at += 1 << dt.DIST_EXTRA[i]
    assert at == 32769 and dt.distance_symbol(32768) == (29, 13) and dt.distance_symbol(1) == (0, 0)


# ---- the builders ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    out = {"ladder_lengths": bh.ladder_lengths(), "ladder_distances": bh.ladder_distances(), "one_byte_rows": bh.one_byte_rows(), "long_rows": bh.long_rows(),
           "empty_rows": bh.empty_rows(), "border": bh.border(0), "border 180": bh.border(180), "border 179": bh.border(179)}
    return {k: (t, off, [bh.expected_tokens(t, off, B0, B1) for B0, B1 in bh.block_ranges(len(t))]) for k, (t, off) in out.items()}


def test_expected_tokens_stand_for_the_text(built):
    """Block by block: no match reaches before its block, so each block's tokens expand on their own."""
    for name, (text, off, blocks) in built.items():
        assert len(off) >= 2 and off[0] == 0 and off[-1] == len(text) and (np.diff(off) >= 0).all(), name
        for (B0, B1), tokens in zip(bh.block_ranges(len(text)), blocks):
            block = dt.Block(dt.DYNAMIC, None, None, None, None, None, None, tokens)
            assert dt.expand([block]) == text[B0:B1], name
            assert all(bh.MINM <= t[0] <= 258 and 1 <= t[1] <= 32768 for t in tokens if isinstance(t, tuple)), name
        assert bh.expected_tokens(text, None, 0, min(len(text), bh.BLOCK)) == list(text[:bh.BLOCK]), name


def test_the_ladders_reach_every_length_and_every_distance_symbol(built):
    matches = [t for name in ("ladder_lengths", "ladder_distances") for tokens in built[name][2] for t in tokens if isinstance(t, tuple)]
    assert {L for L, _d in matches} >= set(range(6, 259))
    assert {dt.distance_symbol(d)[0] for _L, d in matches} == set(range(30))
    assert {dt.length_symbol(L)[0] for L, _d in matches} == set(range(260, 286))            # every length symbol a match of 6 or more can use
    text, off, blocks = built["ladder_lengths"]
    assert len(text) == 300 * 256 and [t for t in blocks[0] if isinstance(t, tuple)][:3] == [(6, 300), (7, 300), (8, 300)]
    assert (180, 300) in blocks[0] and blocks[0][-1] == (180, 300)                           # the row the block's border cuts
    assert not isinstance(blocks[1][0], tuple) and {(222, 300), (223, 300)} <= set(blocks[1])
    text, off, blocks = built["ladder_distances"]
    ds = bh.ladder_distance_list()
    assert len(ds) == 58 and ds[:12] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16] and ds[-6:] == [16385, 24576, 24577, 32768, 32769, 40000]
    found = {d for tokens in blocks for L, d in (t for t in tokens if isinstance(t, tuple))}
    assert found <= set(ds) and 32769 not in found and 40000 not in found and {1, 2, 3, 39, 32768} & found >= {1, 2, 3}
    assert all(L <= 40 for tokens in blocks for L, _d in (t for t in tokens if isinstance(t, tuple)))
    assert any(t == (40, 1) for t in blocks[0]) and any(t == (40, 33) for t in blocks[0])   # overlapping (d < L) and not


def test_row_geometry_builders(built):
    text, off, blocks = built["one_byte_rows"]
    assert len(text) == 70000 and len(off) == 70001 and all(not isinstance(t, tuple) for tokens in blocks for t in tokens)
    same = np.frombuffer(text, dtype=np.uint8)
    assert 0.6 < float((same[1:] == same[:-1]).mean()) < 0.75
    text, off, blocks = built["long_rows"]
    assert len(blocks) == 5 and all(d == 32768 for tokens in blocks for _L, d in (t for t in tokens if isinstance(t, tuple)))
    assert all(not isinstance(t, tuple) for t in blocks[0] + blocks[1])                      # the rows of 50 000 bytes: no distance fits
    # rows of 32 768 from 150 000 on, blocks from 130 560, 195 840, 261 120: p - d is inside p's block for 13 072, 19 696, 12 816 and
    # 19 952 bytes of the second to fifth row, 51 + 77 + 50 + 78 matches of at most 258
    assert sum(isinstance(t, tuple) for tokens in blocks for t in tokens) == 256
    text, off, blocks = built["empty_rows"]
    assert int((np.diff(off) == 0).sum()) == 750 and sum(t == (57, 57) for tokens in blocks for t in tokens) >= 748
    text, off, blocks = built["border"]
    assert len(blocks) == 3 and len(text) % bh.BLOCK and bh.BLOCK % 300
    text, off, blocks = built["border 180"]
    assert off[218] == bh.BLOCK and blocks[1][299:302] == [text[bh.BLOCK + 299], (258, 300), (42, 300)]
    text, off, blocks = built["border 179"]
    assert off[218] == bh.BLOCK - 1 and blocks[1][298:302] == [text[bh.BLOCK + 298], text[bh.BLOCK + 299], (258, 300), (41, 300)]


def test_hostile_offsets_are_out_of_order_in_every_block(built):
    text, off, _blocks = built["ladder_lengths"]
    bad = bh.hostile_offsets(text, off)
    assert bad[0] == 0 and bad[-1] == len(text) and int((bad != off).sum()) >= 30 and bad.min() == -50 and bad.max() == len(text) + 50
    c = bh.clamp_offsets(bad, len(text))
    assert (np.diff(c) < 0).sum() >= 30
    with pytest.raises(ValueError):
        bh.expected_tokens(text, bad, 0, bh.BLOCK)


def test_chain_is_deeper_than_fifteen_bits():
    text, off = bh.chain()
    assert off is None and len(text) == 46366
    ll, _dd, extra = bh.token_histograms(list(text), dt.length_symbol, dt.distance_symbol)
    assert sorted(f for f in ll if f)[:6] == [1, 1, 2, 3, 5, 8] and extra == 0
    depth = max(bh.huffman_depths(ll).values())
    print("chain: unlimited Huffman depth", depth)
    assert depth >= 16


def test_dyadic_is_fifteen_deep_and_its_header_needs_eight():
    text, off = bh.dyadic()
    assert off is None and len(text) == 32767
    ll, dd, _extra = bh.token_histograms(bh.expected_tokens(text, off, 0, len(text)), dt.length_symbol, dt.distance_symbol)
    depths = bh.huffman_depths(ll)
    assert max(depths.values()) == 15 and depths[256] == 15 and not any(dd)
    counts = np.bincount(list(depths.values()), minlength=16)
    assert {L: int(c) for L, c in enumerate(counts) if c} == {**bh.DYADIC, 15: bh.DYADIC[15] + 1}
    assert sum(1 << (15 - d) for d in depths.values()) == 1 << 15                            # complete with nothing cut: these ARE the lengths
    llen = [depths.get(s, 0) for s in range(257)]
    hist = bh.code_length_histogram(llen, [1, 1])                                            # no distance used: two codes of one bit
    assert hist == [0, 2, 0, 0, 6, 12, 5, 16, 5, 7, 1, 16, 0, 1, 1, 154, 0, 0, 1]
    depth = max(bh.huffman_depths(hist).values())
    print("dyadic: unlimited depth of the code-length code", depth)
    assert depth >= 8
