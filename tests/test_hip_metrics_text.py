"""GPU: the device metrics writer (csrc/epg_metrics_text.h).  The judge is never the code under test: the text is held against the
decompressed bytes of the host writer (epgio_write_metrics through _io.write_metrics), the compressed file against zlib and
tests/bgzf_ref.  The arena and stream cases follow tests/test_hip_textout.py: exact-size buffers between guards, dirty outputs and
workspace, side stream, capture and two replays."""
import gzip

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import _io, driver
from tests import bgzf_ref
from tests import metrics_text_ref as ref
from tests.test_hip_abi_contract import I32, I64, U8, Spec, run_case
from tests.test_hip_abi_streams import stream_case

pytestmark = pytest.mark.gpu


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
    """(R, with_p) -> (the rows, the host writer's text), computed once."""
    tmp = tmp_path_factory.mktemp("metrics")
    out = {}
    for R in ref.SIZES:
        for with_p in (True, False):
            r = ref.rows(R, 1000 + R, with_p)
            out[R, with_p] = (r, ref.host_text(tmp, r))
    return out


def tables():
    blobs = []
    for names in (ref.CHROMS, ref.STATES):
        blob, off = _io._string_table(names)
        blobs += [torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda(), int(off[-1])]
    return blobs


def device_text(eng, r, text=None, **change):
    """-> (text tensor, row offsets as a host array, the flag word) of the rows r, `change` replacing row arrays."""
    c, co, cb, n, no, nb = tables()
    a = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in {**r, **change}.items()}
    text, row_off, flags = eng.format_metrics(c, co, cb, a["chrom_idx"], a["start"], a["end"], n, no, nb, a["maxdiff"], a["dist"], a["pvals"], a["mh"],
                                              text=text, chrom_max=14, name_max=20)
    torch.cuda.synchronize()
    return text, row_off.cpu().numpy(), int(flags[0])


@pytest.mark.parametrize("with_p", [True, False], ids=["p", "nop"])
@pytest.mark.parametrize("R", ref.SIZES)
def test_the_text_is_the_host_writer_s(eng, inputs, R, with_p):
    r, want = inputs[R, with_p]
    text, off, flag = device_text(eng, r)
    assert flag == 0 and off[0] == 0 and off[-1] == len(want) and len(off) == R + 1
    assert text[:len(want)].cpu().numpy().tobytes() == want
    assert np.array_equal(off[1:], np.flatnonzero(np.frombuffer(want, dtype=np.uint8) == 10) + 1)
    if R >= 4097:                                                               # the inputs do hold what the cases are about
        lines = want.split(b"\n")
        assert any(l.startswith(b"chrUn_gl000220\t") for l in lines) and any(l.startswith(b"1\t") for l in lines)
        assert b"\t1099511627576\t" in want and b"\t0\t200\t" in want and b"\t2147483520.00000\t-" in want and b"\t0.00000\t+" in want
        assert all(b"\t" + s.encode() + b"\t" in want for s in ref.STATES)
        assert not with_p or (b"e-308" in want and b"e-100\t" in want and b"\t1.00000e+00" in want and b"\t0.00000e+00" in want)


def test_every_e5_edge_value_alone_in_a_row(eng, tmp_path):
    assert len(ref.E5_EDGES) >= 28
    for k, v in enumerate(ref.E5_EDGES):
        r = ref.rows(1, k)
        r["pvals"], r["mh"] = np.array([v]), np.array([ref.E5_EDGES[-1 - k]])
        want = ref.host_text(tmp_path, r)
        text, off, flag = device_text(eng, r)
        assert flag == 0 and text[:off[-1]].cpu().numpy().tobytes() == want, (v, want)
    r = ref.rows(len(ref.DIST_EDGES), 5)
    r["dist"] = np.array(ref.DIST_EDGES, dtype=np.float32)
    want = ref.host_text(tmp_path, r)
    assert want.count(b"\t0.00000\t+") == 3 and want.count(b"\t0.00000\t-") == 1   # 0.0, -0.0 and 1e-7 are "+", -1e-7 prints 0.00000 and "-"
    text, off, flag = device_text(eng, r)
    assert flag == 0 and text[:off[-1]].cpu().numpy().tobytes() == want


@pytest.mark.parametrize("field,value,bit", [
    ("dist", float("nan"), "dist"), ("dist", float("inf"), "dist"), ("dist", -2.0 ** 31, "dist"),
    ("pvals", -0.0, "pval"), ("pvals", -1e-5, "pval"), ("pvals", float(np.nextafter(1.0, 2.0)), "pval"), ("mh", float("nan"), "pval"), ("mh", float("inf"), "pval"),
    ("maxdiff", 0, "state"), ("maxdiff", len(ref.STATES) + 1, "state"), ("chrom_idx", -1, "chrom"), ("chrom_idx", len(ref.CHROMS), "chrom"),
    ("start", -1, "coord"), ("end", -200, "coord")])
def test_each_flagged_input_sets_its_flag(eng, inputs, field, value, bit):
    r, want = inputs[257, True]
    a = r[field].copy()
    a[200] = value
    _text, off, flag = device_text(eng, r, **{field: a})
    assert flag == ref.FLAG[bit]
    assert abs(int(off[-1]) - len(want)) < 64                                   # the row is still a row: offsets stay in bounds
    assert device_text(eng, r)[2] == 0


def test_a_text_cap_one_byte_short_writes_nothing(eng, inputs):
    r, want = inputs[257, True]
    text = torch.full((len(want) + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    _t, off, flag = device_text(eng, r, text=text[:len(want) - 1])
    assert flag == ref.FLAG["cap"] and bool((text == 0xAB).all()) and off[-1] == len(want)
    _t, _off, flag = device_text(eng, r, text=text[:len(want)])
    assert flag == 0 and text[:len(want)].cpu().numpy().tobytes() == want and bool((text[len(want):] == 0xAB).all())


def test_the_validation_order_of_the_contract(abi):
    ref.check_validation_order(abi.load())


def s_metrics(abi, r, want):
    R = len(r["dist"])
    off = np.zeros(R + 1, dtype=I64)
    off[1:] = np.flatnonzero(np.frombuffer(want, dtype=U8) == 10) + 1
    cblob, coff = _io._string_table(ref.CHROMS)
    nblob, noff = _io._string_table(ref.STATES)
    with_p = r["pvals"] is not None
    sp = Spec(len(ref.STATES))
    sp.inp("chrom", cblob[:-1].copy(), mis=1)                                   # exactly the names: a byte beyond them lands in the guard
    sp.inp("chrom_off", coff, mis=8)
    sp.inp("chrom_idx", r["chrom_idx"], mis=4)
    sp.inp("start", r["start"], mis=8)
    sp.inp("end", r["end"], mis=8)
    sp.inp("names", nblob[:-1].copy(), mis=1)
    sp.inp("names_off", noff, mis=8)
    sp.inp("maxdiff", r["maxdiff"], mis=4)
    sp.inp("dist", r["dist"], mis=4)
    if with_p:
        sp.inp("pvals", r["pvals"], mis=8)
        sp.inp("mh", r["mh"], mis=8)
    sp.out("text", U8, len(want))                                               # exactly the text
    sp.out("row_off", I64, R + 1, mis=8)
    sp.out("flags", I32, 1, mis=4)
    sp.ws("ws", abi.call("epgm_format_ws_bytes", R))
    sp.call = lambda abi, P, st: abi.call("epgm_format_metrics", P["chrom"], P["chrom_off"], len(ref.CHROMS), int(coff[-1]), P["chrom_idx"], P["start"],
                                          P["end"], P["names"], P["names_off"], len(ref.STATES), int(noff[-1]), P["maxdiff"], P["dist"],
                                          P["pvals"] if with_p else None, P["mh"] if with_p else None, R, P["text"], len(want), P["row_off"],
                                          P["flags"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert list(o["flags"]) == [0] and np.array_equal(o["row_off"], off) and o["text"].tobytes() == want
    sp.verify = verify
    return sp


@pytest.mark.parametrize("R,with_p", [(257, True), (4097, False)])
def test_format_contract_and_streams(abi, inputs, R, with_p):
    r, want = inputs[R, with_p]
    run_case(s_metrics(abi, r, want), abi)
    stream_case(s_metrics(abi, r, want), abi)


@pytest.mark.parametrize("with_p", [True, False], ids=["p", "nop"])
def test_the_compressed_file_of_70001_rows(eng, inputs, tmp_path, monkeypatch, with_p):
    """engine.metrics_text_bgzf -> driver.write_bgzf: zlib and tests/bgzf_ref read the file, it ends in exactly one end-of-file block;
    with a small chunk rule the file is several chunks' streams back to back and still that text."""
    r, want = inputs[70001, with_p]
    for chunk in (eng.METRICS_CHUNK_TEXT_BYTES, 1 << 20):
        monkeypatch.setattr(eng, "METRICS_CHUNK_TEXT_BYTES", chunk)
        pieces = eng.metrics_text_bgzf(ref.CHROMS, r["chrom_idx"], r["start"], r["end"], ref.STATES, r["maxdiff"], r["dist"], r["pvals"], r["mh"])
        assert pieces is not None and (len(pieces) == 1) == (chunk > (1 << 20))
        path = tmp_path / "pairwiseMetrics_t.txt.gz"
        driver.write_bgzf(path, pieces)
        blob = path.read_bytes()
        assert gzip.decompress(blob) == want
        ms = bgzf_ref.members(blob)
        assert bgzf_ref.walk(blob) and blob.endswith(bgzf_ref.EOF) and blob.count(bgzf_ref.EOF) == 1
        assert len(ms) >= -(-len(want) // 65280) + 1 and len(blob) < len(want)
    p = torch.from_numpy(r["pvals"]).cuda() if with_p else None                 # p-values that are on the device already
    mh = torch.from_numpy(r["mh"]).cuda() if with_p else None
    again = eng.metrics_text_bgzf(ref.CHROMS, r["chrom_idx"], r["start"], r["end"], ref.STATES, r["maxdiff"], r["dist"], p, mh)
    assert b"".join(a.tobytes() for a in again) == b"".join(a.tobytes() for a in pieces)
    bad = r["dist"].copy()
    bad[69000] = np.inf
    assert eng.metrics_text_bgzf(ref.CHROMS, r["chrom_idx"], r["start"], r["end"], ref.STATES, r["maxdiff"], bad, r["pvals"], r["mh"]) is None
    assert eng.metrics_text_bgzf(ref.CHROMS, r["chrom_idx"][:0], r["start"][:0], r["end"][:0], ref.STATES, r["maxdiff"][:0], r["dist"][:0]) == []
    eng.release_text_buffers()
