"""GPU: the device text writer (csrc/epg_textout.h).  The judge is never the code under test: the text is held against the
decompressed bytes of the host writer (_io.write_scores), the BGZF stream against gzip.decompress (which checks every member's
CRC-32 and ISIZE), the library's two inflaters and tests/bgzf_ref.walk.

Size conditions (conditions, not measurements):
  * random scores under the chromosome name "1" hold at most 16 distinct byte values, and an optimal prefix code is never worse than
    4 bits a symbol: the stream is at most 0.5 x text + 128 bytes per block (header, code description, trailer);
  * the runs-of-30-equal-rows input comes out BELOW its zeroth-order entropy n * H0 / 8, which no coder of literals alone can reach:
    the row matches exist.
The arena and stream cases follow tests/test_hip_pvals_streams.py: exact-size buffers between guards, dirty outputs and workspace,
side stream, capture and two replays."""
import gzip
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import _io
from tests import bgzf_ref
from tests.test_hip_abi_contract import F32, I32, I64, U8, Spec, run_case
from tests.test_hip_abi_streams import stream_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 127), (64, 18), (65, 15), (4097, 25), (70001, 18)]
CHROMS = ["1", "chr1", "chrUn_gl000220"]
BLOCK = 65280


def edge_values():
    base = [0.0, 1e-6, 2.0 ** -6, 3 * 2.0 ** -6, 9.999995, 99999.99, float(np.float32(1e-45)), 2147483520.0]
    v = np.array(base + [-x for x in base], dtype=np.float32)
    assert np.signbit(v[len(base)]) and v[len(base)] == 0 and v[6] > 0 and v[7] == np.float32(2.0 ** 31 - 128)
    return v


def locations(R, chrom, start0=99400):
    """Rows of 200 bp from start0: the coordinates pass 100 000 a few rows in, so their digit count changes within the file."""
    rows = [("%s\t%d\t%d\n" % (chrom, start0 + 200 * r, start0 + 200 * (r + 1))).encode() for r in range(R)]
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    return _io.Locations(np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), off)


def scores_of(kind, R, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.3, size=(R, S)).astype(np.float32)
    if kind == "edges":
        e = edge_values()
        flat = x.reshape(-1)
        at = rng.permutation(flat.size)[:e.size] if flat.size >= 4 * e.size else np.arange(min(e.size, flat.size))
        flat[at] = e[:at.size]                                                # ((1, 1) holds one of them: test_every_edge_value_alone)
    elif kind == "zeros":
        x[rng.random(size=x.shape) < 0.6] = 0.0
    elif kind == "runs30":
        x = np.repeat(x[::30], 30, axis=0)[:R].copy()
    elif kind == "equal":
        x[:] = x[0]
    return x


def host_text(tmp, loc, x):
    p = tmp / "ref.txt.gz"
    _io.write_scores(p, loc, x)
    return gzip.decompress(p.read_bytes())


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


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (Locations, float32 [R, S] scores, the host writer's text), computed once."""
    tmp = tmp_path_factory.mktemp("textout")
    out = {}
    for k, (R, S) in enumerate(SHAPES):
        loc, x = locations(R, CHROMS[k % 3]), scores_of("edges", R, S, 100 + k)
        out["%dx%d" % (R, S)] = (loc, x, host_text(tmp, loc, x))
    for kind, R, S, chrom in (("empty", 0, 18, "chr1"), ("equal", 300, 127, "chr1"), ("runs30", 20001, 18, "chr1"), ("zeros", 20001, 18, "chr1"),
                              ("random1", 20001, 18, "1")):
        loc, x = locations(R, chrom), scores_of(kind, R, S, 7)
        out[kind] = (loc, x, host_text(tmp, loc, x))
    return out


def device_text(eng, loc, x, pad=0):
    R, S = x.shape
    full = torch.full((R, S + pad), float("nan"), dtype=torch.float32, device="cuda")
    full[:, :S] = torch.from_numpy(x)
    blob = torch.from_numpy(np.ascontiguousarray(loc.blob)).cuda() if R else torch.zeros(1, dtype=torch.uint8, device="cuda")
    text, row_off, flags = eng.format_scores(full[:, :S], blob, torch.from_numpy(loc.offsets).cuda())
    torch.cuda.synchronize()
    return text, row_off, int(flags[0])


# ---- format ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["%dx%d" % s for s in SHAPES] + ["empty", "equal"])
@pytest.mark.parametrize("pad", [0, 5])
def test_the_text_is_the_host_writer_s(eng, inputs, name, pad):
    loc, x, want = inputs[name]
    text, row_off, flag = device_text(eng, loc, x, pad)
    off = row_off.cpu().numpy()
    assert flag == 0 and off[0] == 0 and off[-1] == len(want)
    assert text[:len(want)].cpu().numpy().tobytes() == want
    ends = np.frombuffer(want, dtype=np.uint8)[off[1:] - 1] if len(want) else np.zeros(0, dtype=np.uint8)
    assert (ends == 10).all() and want.count(b"\n") == x.shape[0]


def test_a_row_that_crosses_two_window_boundaries(eng, tmp_path):
    """Three rows, S = 2; the middle row's location is 70 000 bytes long, so the row begins in one 32 KB window of the text, fills the
    next completely and ends in a third: the only way a single row's bytes are split between windows."""
    rows = [b"chr1\t0\t200\n", b"c" + b"A" * 70000 + b"\t200\t400\n", b"chr1\t400\t600\n"]
    off = np.zeros(4, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    loc = _io.Locations(np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), off)
    x = np.array([[0.25, -1.5], [3.125, -0.00001], [12345.678, 0.0]], dtype=np.float32)
    want = host_text(tmp_path, loc, x)
    assert want.count(b"\n") == 3 and want.startswith(b"chr1\t0\t200\t0.25000\t-1.50000\nc" + b"A" * 70000 + b"\t200\t400\t3.12500\t")
    text, row_off, flag = device_text(eng, loc, x)
    o = row_off.cpu().numpy()
    assert flag == 0 and o[0] == 0 and o[-1] == len(want)
    assert o[1] < 32768 and o[2] > 65536 + 16                   # the middle row: from inside the first window into the third
    assert text[:len(want)].cpu().numpy().tobytes() == want
    assert (np.frombuffer(want, dtype=np.uint8)[o[1:] - 1] == 10).all()


def test_every_edge_value_alone(eng, tmp_path):
    """(R, S) = (1, 1) holds one value: each edge value in turn, and as a column, so that every one of them is formatted."""
    e = edge_values()
    loc = locations(e.size, "chr1")
    x = e.reshape(-1, 1)
    want = host_text(tmp_path, loc, x)
    assert b"\t0.01562\n" in want and b"\t-0.01562\n" in want and b"\t0.04688\n" in want and b"\t-0.00000\n" in want and b"\t2147483520.00000\n" in want
    text, _off, flag = device_text(eng, loc, x)
    assert flag == 0 and text[:len(want)].cpu().numpy().tobytes() == want
    for v in e:
        one = locations(1, "1")
        w = host_text(tmp_path, one, np.array([[v]], dtype=np.float32))
        text, _off, flag = device_text(eng, one, np.array([[v]], dtype=np.float32))
        assert flag == 0 and text[:len(w)].cpu().numpy().tobytes() == w, v


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 2.0 ** 31, -2.0 ** 31, 3e38])
def test_a_value_the_device_does_not_format_sets_the_flag(eng, inputs, bad):
    loc, x, _want = inputs["65x15"]
    y = x.copy()
    y[40, 7] = bad
    _text, _off, flag = device_text(eng, loc, y)
    assert flag & 1
    assert device_text(eng, loc, x)[2] == 0


def s_format(abi, loc, x, want, ld):
    R, S = x.shape
    full = np.full((R, ld), np.nan, dtype=F32)
    full[:, :S] = x
    off = np.zeros(R + 1, dtype=I64)
    text = np.frombuffer(want, dtype=U8)
    off[1:] = np.flatnonzero(text == 10) + 1
    sp = Spec(18)
    sp.inp("scores", full, mis=4)
    sp.inp("loc", np.ascontiguousarray(loc.blob), mis=1)
    sp.inp("loc_off", np.ascontiguousarray(loc.offsets, dtype=I64), mis=8)
    sp.out("text", U8, len(want))                                               # exactly the text: a byte beyond it lands in the guard
    sp.out("row_off", I64, R + 1, mis=8)
    sp.out("flags", I32, 1, mis=4)
    sp.ws("ws", abi.call("epgw_format_ws_bytes", R))
    sp.call = lambda abi, P, st: abi.call("epgw_format_scores", P["scores"], R, S, ld, P["loc"], P["loc_off"], P["text"], len(want), P["row_off"],
                                          P["flags"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert list(o["flags"]) == [0] and np.array_equal(o["row_off"], off) and o["text"].tobytes() == want
    sp.verify = verify
    return sp


@pytest.mark.parametrize("name,ld", [("65x15", 15), ("4097x25", 29)])
def test_format_contract_and_streams(abi, inputs, name, ld):
    loc, x, want = inputs[name]
    run_case(s_format(abi, loc, x, want, ld), abi)
    stream_case(s_format(abi, loc, x, want, ld), abi)


def test_a_text_that_does_not_fit_is_flagged_and_not_written(eng, abi, inputs):
    loc, x, want = inputs["64x18"]
    blob, off = torch.from_numpy(np.ascontiguousarray(loc.blob)).cuda(), torch.from_numpy(loc.offsets).cuda()
    text = torch.full((len(want) + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    _t, _o, flags = eng.format_scores(torch.from_numpy(x).cuda(), blob, off, text=text[:len(want) - 1])
    torch.cuda.synchronize()
    assert int(flags[0]) == 2 and bool((text == 0xAB).all())


# ---- compress ----------------------------------------------------------------------------------------------------------------------
def compressed(eng, want, row_off, eof):
    text = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda() if want else torch.zeros(1, dtype=torch.uint8, device="cuda")
    out, n_out, flags = eng.bgzf_compress(text, len(want), row_off, eof=eof)
    torch.cuda.synchronize()
    assert int(flags[0]) == 0
    n = int(n_out[0])
    assert n <= eng._abi.call("epgw_bgzf_bytes_max", len(want), int(eof))
    return out[:n].cpu().numpy().tobytes()


def check_stream(blob, want, eof):
    assert gzip.decompress(blob) == want
    if blob:
        cap = len(want) + 4096
        assert _io.inflate_mem(blob, own=True, cap=cap) == want and _io.inflate_mem(blob, own=False, cap=cap) == want
        if eof:
            assert _io.inflate_mem(blob, own=2, cap=cap) == want
    ms = bgzf_ref.walk(blob, eof=eof)
    blocks = -(-len(want) // BLOCK)
    assert len(ms) == blocks + (1 if eof else 0)
    assert all(m.bsize <= 65536 and m.isize <= BLOCK for m in ms)
    assert [m.isize for m in ms[:blocks]] == [min(BLOCK, len(want) - k * BLOCK) for k in range(blocks)]
    assert (blob[-28:] == bgzf_ref.EOF) == bool(eof) and blob.count(bgzf_ref.EOF) == (1 if eof else 0)
    return ms


@pytest.fixture(scope="module")
def streams(eng, inputs):
    """name -> (text, stream with the end-of-file block, stream without), the row offsets from the device's own format call."""
    out = {}
    for name, (loc, x, want) in inputs.items():
        _text, row_off, flag = device_text(eng, loc, x)
        assert flag == 0
        out[name] = (want, compressed(eng, want, row_off, True), compressed(eng, want, row_off, False))
    return out


@pytest.mark.parametrize("name", ["%dx%d" % s for s in SHAPES] + ["empty", "equal", "runs30", "zeros", "random1"])
def test_every_inflater_reads_the_stream(streams, name):
    want, with_eof, without = streams[name]
    check_stream(with_eof, want, True)
    check_stream(without, want, False)
    assert with_eof == without + bgzf_ref.EOF
    if name == "empty":
        assert with_eof == bgzf_ref.EOF and without == b""
    if name == "equal":
        assert want.index(b"\n") > 258                                          # a row is longer than one match


@pytest.mark.parametrize("n", [70001, 65281])
def test_arbitrary_bytes_round_trip_stored(eng, n):
    data = np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8).tobytes()
    for eof in (True, False):
        blob = compressed(eng, data, None, eof)
        ms = check_stream(blob, data, eof)
        assert len(ms) == 2 + int(eof)
        for k, m in enumerate(ms[:2]):                                          # random bytes do not compress: both members are stored blocks
            assert m.payload[0] == 1 and len(m.payload) == 5 + m.isize and m.payload[5:] == data[k * BLOCK:(k + 1) * BLOCK]


def test_text_without_row_offsets_still_round_trips(eng, inputs):
    want = inputs["4097x25"][2]
    check_stream(compressed(eng, want, None, True), want, True)


def test_size_conditions(streams):
    want, blob, _ = streams["random1"]
    assert len(set(want)) <= 16
    blocks = -(-len(want) // BLOCK)
    print("random scores, chromosome 1: text %d, stream %d (%.4f), bound %.0f" % (len(want), len(blob), len(blob) / len(want), 0.5 * len(want) + 128 * blocks))
    assert len(blob) - 28 <= 0.5 * len(want) + 128 * blocks
    want, blob, _ = streams["runs30"]
    counts = np.bincount(np.frombuffer(want, dtype=np.uint8), minlength=256).astype(np.float64)
    p = counts[counts > 0] / len(want)
    h0 = -float((p * np.log2(p)).sum())
    print("runs of 30 equal rows: text %d, stream %d (%.4f), n H0 / 8 = %.0f (%.4f)" % (len(want), len(blob), len(blob) / len(want), len(want) * h0 / 8, h0 / 8))
    assert len(blob) < len(want) * h0 / 8 and math.isfinite(h0)


def s_compress(abi, want, off, eof, n_out):
    sp = Spec(18)
    R = 0 if off is None else len(off) - 1                                      # (None: no row offsets, the pointer is NULL)
    sp.inp("text", np.frombuffer(want, dtype=U8), mis=3)
    if off is not None:
        sp.inp("row_off", off, mis=8)
    sp.out("out", U8, n_out)                                                    # exactly the stream: a byte beyond it lands in the guard
    sp.out("n_out", I64, 1, mis=8)
    sp.out("flags", I32, 1, mis=4)
    sp.ws("ws", abi.call("epgw_bgzf_ws_bytes", len(want)))
    sp.call = lambda abi, P, st: abi.call("epgw_bgzf_compress", P["text"], len(want), P.get("row_off"), R, int(eof), P["out"], n_out, P["n_out"], P["flags"],
                                          P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert list(o["flags"]) == [0] and list(o["n_out"]) == [n_out]
        check_stream(o["out"].tobytes(), want, eof)
    sp.verify = verify
    return sp


@pytest.mark.parametrize("name,eof", [("65x15", True), ("4097x25", False)])
def test_compress_contract_and_streams(abi, inputs, streams, name, eof):
    want = inputs[name][2]
    off = np.zeros(inputs[name][1].shape[0] + 1, dtype=I64)
    off[1:] = np.flatnonzero(np.frombuffer(want, dtype=U8) == 10) + 1
    n_out = len(streams[name][1 if eof else 2])
    run_case(s_compress(abi, want, off, eof, n_out), abi)
    stream_case(s_compress(abi, want, off, eof, n_out), abi)


def test_a_stream_that_does_not_fit_is_flagged(eng, inputs, streams):
    want = inputs["4097x25"][2]
    text = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()
    n = len(streams["4097x25"][1])
    out = torch.full((n + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    _o, n_out, flags = eng.bgzf_compress(text, len(want), None, eof=True, out=out[:n - 1])
    torch.cuda.synchronize()
    assert int(flags[0]) == 1 and bool((out[n - 28:] == 0xAB).all())


def test_the_engine_s_part_call(eng, inputs):
    """scores_text_bgzf: the file's bytes without the end-of-file block, None on a flag, buffers reused between parts."""
    for name in ("4097x25", "65x15", "empty"):
        loc, x, want = inputs[name]
        got = eng.scores_text_bgzf(loc, torch.from_numpy(x).cuda())
        blob = got[0][:got[1]].cpu().numpy().tobytes()
        check_stream(blob, want, False)
    held = {k: int(t.numel()) for k, t in eng._text_bufs.items()}
    assert len(held) == 3, held
    loc, x, _want = inputs["65x15"]
    y = x.copy()
    y[3, 3] = np.nan
    assert eng.scores_text_bgzf(loc, torch.from_numpy(y).cuda()) is None
    eng.release_text_buffers()
    assert not eng._text_bufs
