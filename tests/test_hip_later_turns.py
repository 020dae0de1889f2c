"""GPU: the text kernels' SECOND AND LATER loop turns.

Four one-workgroup scans of the text writers and readers walk their field in turns, and none of the sizes of the modules' own tests
gives any of them a second one:
  * k_text_tile_offsets (both row writers) and k_bgzf_offsets: st_scan_chunks, ceil(n / 1024) consecutive tiles or blocks per thread --
    more than one beyond 1024 tiles of 256 rows, 1024 blocks of 65 280 bytes;
  * k_sbl_scan and k_seg_scan: st_scan_segments, turns of 1024 segments of 4096 bytes of text with a carry; k_seg_runs, turns of 1024
    blocks of 256 lines with a carried maximum.
The sizes here are the last one-turn shape, the first two-turn shape and a three-turn shape with a ragged last thread or turn.  Every
case states its arithmetic from constants restated beside it, and is judged as in the kernel's own module: the row writers byte for
byte against the host writers' text, the compressor by gzip and tests/bgzf_ref, the readers against the arrays the text was made from.
The host references are computed once per module."""
import gzip

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import _abi
from tests import bgzf_ref
from tests import metrics_text_ref as mref
from tests import test_hip_metrics_text as metrics
from tests import test_hip_segments as segs
from tests import test_hip_statebyline as sbl
from tests import test_hip_textout as textout
from tests.grid_cap import cdiv

pytestmark = pytest.mark.gpu

SCAN_THREADS = 1024                                # k_text_tile_offsets<1024>, BG_SCAN_THREADS, SBL_SCAN_THREADS, SEG_SCAN_THREADS
TEXT_ROWS = 256                                    # epg_text_rows.h: rows per tile of the row writers
BLOCK = 65280                                      # epg_bgzf_block.h: text bytes per BGZF block
SEGMENT = 4096                                     # epg_statebyline.hip, epg_segments.hip: bytes of text per segment (held against the library below)
LINE_BLOCK = 256                                   # epg_segments.hip: lines per workgroup of the line kernels, an entry of k_seg_runs
SEG_MIN_LINE = 8                                   # epg_segments.hip: the per-line arrays hold nbytes / 8 + 2 lines


def chunks_of(n):
    """st_scan_chunks over n values: (values per thread, threads that own one, values of the last of them)."""
    chunk = cdiv(n, SCAN_THREADS)
    owners = cdiv(n, chunk)
    return chunk, owners, n - (owners - 1) * chunk


def turns_of(n):
    """st_scan_segments over n values: (turns, values of the last turn)."""
    return cdiv(n, SCAN_THREADS), n - (cdiv(n, SCAN_THREADS) - 1) * SCAN_THREADS


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    yield engine
    engine.release_text_buffers()


# ---- the row writers: k_text_tile_offsets with two and three tiles per thread -----------------------------------------------------------
ROW_SIZES = (262144, 262145, 524801)


def test_the_arithmetic_of_the_row_cases():
    assert chunks_of(cdiv(70001, TEXT_ROWS)) == (1, 274, 1)                     # the largest size of the writers' own modules
    assert [cdiv(R, TEXT_ROWS) for R in ROW_SIZES] == [1024, 1025, 2051]
    assert chunks_of(1024) == (1, 1024, 1)                                      # the last shape of one tile per thread
    assert chunks_of(1025) == (2, 513, 1)                                       # threads 513 .. 1023 own nothing, thread 512 one tile of ONE row
    assert chunks_of(2051) == (3, 684, 2) and 524801 % TEXT_ROWS == 1           # thread 683 is ragged, and so is the last tile


def newline_offsets(want, R):
    off = np.zeros(R + 1, dtype=np.int64)
    off[1:] = np.flatnonzero(np.frombuffer(want, dtype=np.uint8) == 10) + 1
    return off


@pytest.mark.parametrize("R", ROW_SIZES)
def test_score_rows_with_chunks_of_tiles(eng, tmp_path, R):
    assert chunks_of(cdiv(R, TEXT_ROWS))[0] == {262144: 1, 262145: 2, 524801: 3}[R]
    loc, x = textout.locations(R, "chr1"), textout.scores_of("edges", R, 1, R)
    edges = np.flatnonzero(np.isin(x.reshape(-1), textout.edge_values()[[1, 3, 5, 7]]))
    assert edges.size >= 4 and edges.max() // TEXT_ROWS >= cdiv(R, TEXT_ROWS) // 2       # edge values in the late tiles too
    want = textout.host_text(tmp_path, loc, x)
    assert want.count(b"\n") == R
    text, row_off, flag = textout.device_text(eng, loc, x)
    assert flag == 0
    assert np.array_equal(row_off.cpu().numpy(), newline_offsets(want, R))
    assert text[:len(want)].cpu().numpy().tobytes() == want


@pytest.mark.parametrize("with_p", [True, False], ids=["p", "nop"])
@pytest.mark.parametrize("R", ROW_SIZES)
def test_metrics_rows_with_chunks_of_tiles(eng, tmp_path, R, with_p):
    assert chunks_of(cdiv(R, TEXT_ROWS))[0] == {262144: 1, 262145: 2, 524801: 3}[R]
    r = mref.rows(R, 1000 + R, with_p)
    edges = np.flatnonzero(np.isin(r["dist"], np.array(mref.DIST_EDGES, dtype=np.float32)))
    assert edges.size >= len(mref.DIST_EDGES) and edges.max() // TEXT_ROWS >= cdiv(R, TEXT_ROWS) // 2   # edge values in the late tiles too
    want = mref.host_text(tmp_path, r)
    assert want.count(b"\n") == R
    text, off, flag = metrics.device_text(eng, r)
    assert flag == 0 and len(off) == R + 1
    assert np.array_equal(off, newline_offsets(want, R))
    assert text[:len(want)].cpu().numpy().tobytes() == want


# ---- the compressor: k_bgzf_offsets with two blocks per thread -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_text(tmp_path_factory):
    """(text, row offsets): the 70001 x 18 score text of tests/test_hip_textout.py, tiled to a little more than 1025 blocks.  The rows'
    lengths differ, so a block's text is never the block before it shifted by a whole number of rows: the blocks' sizes differ."""
    R, S = 70001, 18
    loc, x = textout.locations(R, "chr1"), textout.scores_of("edges", R, S, 105)
    one = textout.host_text(tmp_path_factory.mktemp("later"), loc, x)
    copies = cdiv(1025 * BLOCK + 1, len(one))
    text = one * copies
    off1 = newline_offsets(one, R)
    off = np.concatenate([off1[:-1] + k * len(one) for k in range(copies)] + [np.array([len(text)], dtype=np.int64)])
    assert len(text) >= 1025 * BLOCK + 1 and len(off) == copies * R + 1 and off[-1] == len(text)
    return text, off


def hold_stream(blob, want, eof):
    """The judges of tests/test_hip_textout.check_stream that are not the library's own: gzip (every member's CRC-32 and ISIZE), the
    structure walk, the members' ISIZEs, exactly one end-of-file block when one was asked for."""
    assert gzip.decompress(blob) == want
    ms = bgzf_ref.walk(blob, eof=eof)
    blocks = cdiv(len(want), BLOCK)
    assert len(ms) == blocks + (1 if eof else 0)
    assert [m.isize for m in ms[:blocks]] == [BLOCK] * (blocks - 1) + [len(want) - (blocks - 1) * BLOCK]
    assert (blob[-28:] == bgzf_ref.EOF) == bool(eof) and blob.count(bgzf_ref.EOF) == (1 if eof else 0)
    return ms


@pytest.mark.parametrize("rows", [False, True], ids=["literals", "rows"])
def test_bgzf_offsets_with_two_blocks_per_thread(eng, long_text, rows):
    text, off = long_text
    blocks = cdiv(len(text), BLOCK)
    assert blocks >= 1025 and chunks_of(blocks)[0] == 2 and chunks_of(blocks)[1] < SCAN_THREADS      # two blocks per thread, the last threads none
    assert chunks_of(cdiv(70001 * 18 * 9, BLOCK))[0] == 1                                  # (the writers' own largest text: under 200 blocks)
    row_off = torch.from_numpy(off).cuda() if rows else None
    blob = textout.compressed(eng, text, row_off, True)
    ms = hold_stream(blob, text, True)
    assert len({m.bsize for m in ms[:-1]}) > 100                                             # the scan adds sizes that differ
    # the same text cut to 1024 blocks is the one-block-per-thread side: its members are the long stream's first 1024
    cut = 1024 * BLOCK
    assert chunks_of(cdiv(cut, BLOCK)) == (1, 1024, 1)
    if rows:
        last = int(np.searchsorted(off, cut, side="left"))                                   # the rows that begin inside the cut text
        row_off = torch.from_numpy(np.append(off[:last], cut)).cuda()
    short = textout.compressed(eng, text[:cut], row_off, False)
    hold_stream(short, text[:cut], False)
    assert short == blob[:len(short)] and len(short) == sum(m.bsize for m in ms[:1024])


# ---- state-by-line: k_sbl_scan's second and third turn ---------------------------------------------------------------------------------------
SBL_SIZES = (4194303, 4194304, 4194305, 2 * 4194304 + 4097)


def sbl_segments(nbytes):
    return nbytes // SEGMENT + 1                                                            # sbl_seg_words / seg_ws: nseg


def test_the_arithmetic_of_the_reader_cases():
    assert sbl.BB() == SEGMENT == segs.BB() and 4194304 == SCAN_THREADS * SEGMENT
    assert [turns_of(sbl_segments(n)) for n in SBL_SIZES] == [(1, 1024), (2, 1), (2, 1), (3, 2)]
    # the second turn of the 4 194 304-byte text is one segment that holds no byte of it: only the virtual newline can fall there


def sbl_text(nbytes, final_newline, seed):
    """-> (a state-by-line text of exactly nbytes bytes, the values of its lines): built from the array, the header padded."""
    rng = np.random.default_rng([seed, nbytes])
    v = sbl.mixed_values(rng, nbytes // 2)
    size = 2 + (v >= 10) + (v >= 100)                                                       # a line with its newline
    end = np.cumsum(size)
    room = nbytes + (0 if final_newline else 1) - len(sbl.HEAD) - 40                        # (a dropped last newline makes room for one byte more)
    R = int(np.searchsorted(end, room, side="right"))
    v, size, end = v[:R], size[:R], end[:R]
    body = np.full(int(end[-1]), 10, dtype=np.uint8)
    body[end - 2] = 48 + v % 10
    body[(end - 3)[v >= 10]] = 48 + (v // 10 % 10)[v >= 10]
    body[(end - 4)[v >= 100]] = 48 + (v // 100)[v >= 100]
    pad = room + 40 - int(end[-1])
    text = sbl.HEAD[:-1] + b"x" * pad + b"\n" + body.tobytes()
    text = text if final_newline else text[:-1]
    assert len(text) == nbytes and text.endswith(b"\n") == final_newline
    return text, v


@pytest.mark.parametrize("final_newline", [True, False], ids=["newline", "no-newline"])
@pytest.mark.parametrize("nbytes", SBL_SIZES)
def test_statebyline_texts_of_more_than_1024_segments(nbytes, final_newline):
    assert turns_of(sbl_segments(nbytes))[0] == {4194303: 1, 4194304: 2, 4194305: 2, 2 * 4194304 + 4097: 3}[nbytes]
    text, v = sbl_text(nbytes, final_newline, 3)
    assert text[-20:].count(b"\n") >= 4 and sbl.ref_rows(text) == len(v)                    # lines up to the text's end, in the last segment
    col, _before, info = sbl.parse_call(text, cap=len(v), text_mis=5, col_mis=3)
    assert info.tolist() == [len(v), int(v.min()), int(v.max()), -1]
    assert np.array_equal(col, (v - 1).astype(np.int8))


# ---- segments: k_seg_scan's (and k_seg_runs') second and third turn ------------------------------------------------------------------------
SEG_POOL_LINES = 140000


@pytest.fixture(scope="module")
def seg_pool():
    """Per chromosome of the table: (run lengths, states, the lines as bytes, their cumulative size), made once."""
    rng = np.random.default_rng(12)
    pool = []
    for name in segs.TABLE:
        n = SEG_POOL_LINES
        lengths = np.where(rng.random(n) < 0.2, 1, rng.geometric(1.0 / 6.0, size=n)).astype(np.int64)
        states = rng.integers(1, 128, size=n)
        lines = [b"\t".join(l) + b"\n" for l in segs.make_lines([(name, lengths, states)])]
        pool.append((name, lengths, states, lines, np.cumsum([len(l) for l in lines])))
    return pool


def seg_text(pool, nbytes, final_newline):
    """-> (a segment text of exactly nbytes bytes, its chromosomes for the module's restatement): a third of the bytes per chromosome,
    a line of a chromosome outside the table in front whose label is padded to the size."""
    budget = (nbytes - 64) // len(pool)
    chroms, body = [], []
    for name, lengths, states, lines, size in pool:
        k = int(np.searchsorted(size, budget, side="right"))
        assert 0 < k < len(lines), "the pool is too small for %d bytes" % nbytes
        chroms.append((name, lengths[:k], states[:k]))
        body.append(b"".join(lines[:k]))
    body = b"".join(body)
    body = body if final_newline else body[:-1]
    head = b"chrPad\t0\t200\t1_"
    text = head + b"p" * (nbytes - len(body) - len(head) - 1) + b"\n" + body
    assert len(text) == nbytes
    return text, segs._behind_pad(chroms)


@pytest.mark.parametrize("final_newline", [True, False], ids=["newline", "no-newline"])
@pytest.mark.parametrize("nbytes", SBL_SIZES)
def test_segment_texts_of_more_than_1024_segments(seg_pool, nbytes, final_newline):
    assert turns_of(sbl_segments(nbytes))[0] == {4194303: 1, 4194304: 2, 4194305: 2, 2 * 4194304 + 4097: 3}[nbytes]
    text, chroms = seg_text(seg_pool, nbytes, final_newline)
    lines = sum(len(c[1]) for c in chroms)
    line_blocks = cdiv(nbytes // SEG_MIN_LINE + 2, LINE_BLOCK)                              # k_seg_runs scans as many entries
    assert turns_of(line_blocks)[0] == {4194303: 3, 4194304: 3, 4194305: 3, 2 * 4194304 + 4097: 5}[nbytes]
    if nbytes > 2 * 4194304:
        assert lines > SCAN_THREADS * LINE_BLOCK                                            # ... and lines of the text lie in its second turn
    segs.check_good(chroms, text=text, text_mis=7)
