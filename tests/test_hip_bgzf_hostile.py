"""GPU: the device BGZF compressor (csrc/epg_bgzf_block.h, k_bgzf_plan / k_bgzf_offsets / k_bgzf_emit) on the hostile text of
tests/bgzf_hostile.py, judged token by token.  Every stream goes through tests/test_hip_textout.check_stream (gzip, the library's
inflaters, the BGZF walker), then tests/deflate_tokens.py -- a decoder that shares nothing with the project -- opens every member:
the tokens must be exactly bgzf_hostile.expected_tokens, the codes complete and, where no length limit cuts them, of the one optimal
cost (heapq Huffman over the decoded tokens' histogram).  tests/test_bgzf_hostile_host.py has held the judge against zlib and the
inputs against what they are there for; tests/bgzf_block_check.cpp runs the same families through the phases on the host.

Ratios (stream / text, no end-of-file block; nothing is asserted but stream < text).  The host program's at the parent commit:
chain 0.3285, dyadic 0.6487; the device's are printed by test_chain and test_dyadic and recorded in DESIGN.md section 15."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import bgzfIndex
from tests import bgzf_hostile as bh
from tests import bgzf_ref
from tests import deflate_tokens as dt
from tests.test_hip_abi_contract import I64, U8, run_case
from tests.test_hip_abi_streams import stream_case
from tests.test_hip_textout import check_stream, compressed, s_compress

pytestmark = pytest.mark.gpu

BUILDERS = {"ladder_lengths": bh.ladder_lengths, "ladder_distances": bh.ladder_distances, "one_byte_rows": bh.one_byte_rows, "long_rows": bh.long_rows,
            "empty_rows": bh.empty_rows, "border": lambda: bh.border(0), "border 180": lambda: bh.border(180), "border 179": lambda: bh.border(179),
            "chain": bh.chain, "dyadic": bh.dyadic}
TOKEN_CASES = [n for n in BUILDERS if n not in ("chain", "dyadic")]
HOST_RATIO = {"chain": 0.3285, "dyadic": 0.6487}


@pytest.fixture(scope="module")
def eng():
    from epilogos_amd import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


_built, _done = {}, {}


def built(name):
    if name not in _built:
        _built[name] = BUILDERS[name]() if name in BUILDERS else hostile_ladder()
    return _built[name]


def hostile_ladder():
    text, off = built("ladder_lengths")
    return text, bh.hostile_offsets(text, off)


def device(eng, name, rows=True):
    """(text, row offsets or None, the stream without the end-of-file block, [(Member, decoded bytes, [Block])]): compressed with
    `eof` both ways, every inflater and the walker passed, every member opened by deflate_tokens.  Once per input."""
    key = (name, rows)
    if key not in _done:
        text, off = built(name)
        off = off if rows else None
        row_off = None if off is None else torch.from_numpy(off).cuda()
        with_eof, without = compressed(eng, text, row_off, True), compressed(eng, text, row_off, False)
        assert with_eof == without + bgzf_ref.EOF
        check_stream(with_eof, text, True)
        ms = check_stream(without, text, False)
        opened = []
        for m, (B0, B1) in zip(ms, bh.block_ranges(len(text))):
            got, blocks = dt.decode(m.payload)
            assert got == text[B0:B1] and dt.expand(blocks) == got
            opened.append((m, got, blocks))
        _done[key] = (text, off, without, opened)
    return _done[key]


def one_dynamic_block(blocks):
    assert len(blocks) == 1 and blocks[0].btype == dt.DYNAMIC
    return blocks[0]


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "no offsets"])
@pytest.mark.parametrize("name", TOKEN_CASES)
def test_the_tokens_are_exactly_the_expected(eng, name, rows):
    text, off, _stream, opened = device(eng, name, rows)
    assert len(opened) == len(bh.block_ranges(len(text)))
    for (_m, _got, blocks), (B0, B1) in zip(opened, bh.block_ranges(len(text))):
        b = one_dynamic_block(blocks)
        want = bh.expected_tokens(text, off, B0, B1)
        if b.tokens != want:
            k = next((i for i, (x, y) in enumerate(zip(b.tokens, want)) if x != y), min(len(want), len(b.tokens)))
            raise AssertionError("%s, block at %d: %d tokens for %d, the first difference at token %d: %r for %r"
                                 % (name, B0, len(b.tokens), len(want), k, b.tokens[k:k + 3], want[k:k + 3]))
        if not rows:
            assert all(not isinstance(t, tuple) for t in b.tokens)


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "no offsets"])
@pytest.mark.parametrize("name", TOKEN_CASES)
def test_the_codes_are_complete_and_cost_what_huffman_s_cost(eng, name, rows):
    """No code of these inputs is 15 bits deep (asserted on the reference tree), so the builder's lengths must reach the optimal
    cost, which is unique; the member's size must be exactly header + tokens + extra bits + end-of-block."""
    _text, _off, _stream, opened = device(eng, name, rows)
    for m, _got, blocks in opened:
        b = one_dynamic_block(blocks)
        ll, dd, _extra = bh.token_histograms(b.tokens, dt.length_symbol, dt.distance_symbol)
        assert max(bh.huffman_depths(ll).values()) < 15 and max(bh.huffman_depths(dd).values(), default=0) < 15
        assert dt.kraft(b.llen) == 1 << 15 and dt.kraft(b.dlen) == 1 << 15
        assert all(b.llen[s] for s, f in enumerate(ll) if f) and all(b.dlen[s] for s, f in enumerate(dd) if f)
        cost = sum(f * b.llen[s] for s, f in enumerate(ll) if f)
        assert cost == bh.optimal_cost(ll), (name, cost, bh.optimal_cost(ll))
        if sum(1 for f in dd if f) >= 2:
            cost = sum(f * b.dlen[s] for s, f in enumerate(dd) if f)
            assert cost == bh.optimal_cost(dd), (name, cost, bh.optimal_cost(dd))
        assert b.hlit == max(257, 1 + max(s for s, f in enumerate(ll) if f)) and len(m.payload) < m.isize + 5


def deep(eng, name):
    text, off, stream, opened = device(eng, name, True)
    assert off is None and len(opened) == 1
    m, got, blocks = opened[0]
    b = one_dynamic_block(blocks)                                               # dynamic Huffman: not stored
    assert m.payload[0] & 7 == 5 and len(m.payload) < len(text) + 5 and b.tokens == list(text)
    assert dt.kraft(b.llen) == 1 << 15 and max(b.llen) == 15
    assert all(b.llen[c] for c in set(text)) and b.llen[256]
    print("%s: text %d, device stream %d, ratio %.4f (the host program's: %.4f)" % (name, len(text), len(stream), len(stream) / len(text), HOST_RATIO[name]))
    assert len(stream) < len(text)
    return b


def test_chain_is_cut_to_fifteen_bits(eng):
    b = deep(eng, "chain")
    ll, _dd, _extra = bh.token_histograms(b.tokens, dt.length_symbol, dt.distance_symbol)
    assert max(bh.huffman_depths(ll).values()) > 15                             # the cut applied: the cost is above the unlimited optimum
    assert sum(f * b.llen[s] for s, f in enumerate(ll) if f) > bh.optimal_cost(ll)
    assert sorted(l for l in b.llen if l)[-2:] == [15, 15]


def test_dyadic_fifteen_bits_and_a_code_length_code_cut_to_seven(eng):
    b = deep(eng, "dyadic")
    ll, _dd, _extra = bh.token_histograms(b.tokens, dt.length_symbol, dt.distance_symbol)
    depths = bh.huffman_depths(ll)
    assert [b.llen[s] for s in range(257)] == [depths.get(s, 0) for s in range(257)]          # dyadic weights: the lengths are forced
    assert max(b.cllen) == 7 and sum(1 << (7 - l) for l in b.cllen if l) == 1 << 7
    hist = bh.code_length_histogram(b.llen, b.dlen)
    assert max(bh.huffman_depths(hist).values()) >= 8 and all(b.cllen[s] for s, f in enumerate(hist) if f)


def inflate_on_the_device(eng, stream, text):
    table, total = bgzfIndex.members(stream)
    assert total == len(text) and len(table) == len(bh.block_ranges(len(text)))
    out = torch.full((total + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    o, status, flags = eng.bgzf_inflate(torch.from_numpy(np.frombuffer(stream, dtype=U8).copy()).cuda(), torch.from_numpy(table).cuda(), out=out[:total])
    torch.cuda.synchronize()
    assert int(flags[0]) == 0 and not bool(status.any())
    assert o[:total].cpu().numpy().tobytes() == text and bool((out[total:] == 0xAB).all())


@pytest.mark.parametrize("name", list(BUILDERS))
def test_the_device_inflater_reads_every_stream(eng, name):
    text, _off, stream, _opened = device(eng, name, True)
    inflate_on_the_device(eng, stream, text)


def hostile_stream(eng):
    if "hostile" not in _done:
        text, bad = built("hostile")
        row_off = torch.from_numpy(bad).cuda()
        with_eof, without = compressed(eng, text, row_off, True), compressed(eng, text, row_off, False)
        assert with_eof == without + bgzf_ref.EOF
        check_stream(with_eof, text, True)
        _done["hostile"] = (text, bad, without, check_stream(without, text, False))
    return _done["hostile"]


def test_hostile_row_offsets_round_trip_and_are_stored(eng):
    """Every seventh offset is anywhere in [-50, n + 50].  A member whose rows -- those that lie strictly inside its block by the
    offsets that were left alone -- hold a pair out of order cannot be tokenised: it must be a stored block."""
    text, bad, stream, ms = hostile_stream(eng)
    _text, good = built("ladder_lengths")
    c = bh.clamp_offsets(bad, len(text))
    saw = 0
    for m, (B0, B1) in zip(ms, bh.block_ranges(len(text))):
        inside = [r for r in range(1, len(good) - 1) if B0 < good[r] and good[r + 1] < B1 and bad[r] == good[r] and bad[r + 1] != good[r + 1]]
        if any(c[r + 1] < c[r] or c[r + 2] < c[r + 1] for r in inside):
            saw += 1
            assert m.payload[0] == 1 and len(m.payload) == 5 + m.isize and m.payload[5:] == text[B0:B1]
        got, _blocks = dt.decode(m.payload)
        assert got == text[B0:B1]
    assert saw == len(ms) == 2
    inflate_on_the_device(eng, stream, text)


@pytest.mark.parametrize("name,eof", [("hostile", True), ("dyadic", False)])
def test_contract_and_streams_on_hostile_input(eng, abi, name, eof):
    """The guarded arena (out exactly the stream's size, dirty workspace) and the stream cases (side stream, capture, two replays)."""
    if name == "hostile":
        text, off, stream, _ms = hostile_stream(eng)
        off = np.ascontiguousarray(off, dtype=I64)
    else:
        text, off, stream, _opened = device(eng, name, True)
    n_out = len(stream) + (28 if eof else 0)
    run_case(s_compress(abi, text, off, eof, n_out), abi)
    stream_case(s_compress(abi, text, off, eof, n_out), abi)
