"""ChromHMM state-by-line preprocessing, the host side (no GPU): the header's constants (tests/test_abi_symbols.py holds it
against its binding), the entry points' argument checks, the script's file selection rule (stateByLine.find_calls), and the binary matrix file
(.epgm) read by helpers.readTable exactly as the equivalent text matrix is -- pinned to the reference's own matrix_chr1.txt
(tests/golden/statebyline.npz) through a pure-numpy builder."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import _abi, _io, helpers, stateByLine as sbl

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "statebyline.npz")


# ---- the header's constants and the entry points' checks (tests/test_abi_symbols.py holds the header against its binding) ---

def test_constants_and_argument_validation_without_gpu():
    lib = _abi.load()
    hdr = _abi.HEADERS["statebyline"].path.read_text()
    which = {n: int(v) for n, v in re.findall(r"#define EPG_SBL_(THREAD_BYTES|BLOCK_BYTES|TILE_BINS|MAX_BATCH) (\d+)", hdr)}
    assert sorted(which.values()) == [0, 1, 2, 3]
    tb, bb = lib.epg_sbl_constant(which["THREAD_BYTES"]), lib.epg_sbl_constant(which["BLOCK_BYTES"])
    assert tb >= 4 and bb > tb and bb % tb == 0
    assert lib.epg_sbl_constant(which["TILE_BINS"]) % 16 == 0 and lib.epg_sbl_constant(which["MAX_BATCH"]) >= 1
    assert lib.epg_sbl_constant(4) == -1 and lib.epg_sbl_constant(-1) == -1
    assert lib.epg_sbl_ws_bytes(-1) == -1 and lib.epg_sbl_ws_bytes(0x7fff0001) == -1
    assert lib.epg_sbl_ws_bytes(0) > 0 and lib.epg_sbl_ws_bytes(1 << 24) >= 4 * ((1 << 24) // bb + 1)
    x = ctypes.c_void_p(4096)
    ok = dict(text=x, n=1000, col=x, cap=10, info=x, ws=x, wsb=1 << 20)

    def parse(**kw):
        a = dict(ok, **kw)
        return lib.epg_sbl_parse(a["text"], a["n"], a["col"], a["cap"], a["info"], a["ws"], a["wsb"], None)
    assert parse(n=-1) == -1 and parse(n=0x7fff0001) == -1 and parse(cap=-1) == -1
    for name in ("text", "col", "info", "ws"):
        assert parse(**{name: None}) == -1 and b"NULL" in lib.epg_last_error(), name
    assert parse(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.epg_last_error()
    assert parse(info=ctypes.c_void_p(4100)) == -1
    assert parse(wsb=lib.epg_sbl_ws_bytes(1000) - 1) == -4

    def tr(cols=x, nb=4, pitch=64, R=50, X=x, ldx=16, col0=0):
        return lib.epg_sbl_transpose(cols, nb, pitch, R, X, ldx, col0, None)
    assert tr(nb=-1) == -1 and tr(R=-1) == -1 and tr(col0=-1) == -1
    assert tr(nb=lib.epg_sbl_constant(which["MAX_BATCH"]) + 1) == -2
    assert tr(pitch=48) == -1 and tr(pitch=72) == -1 and b"pitch" in lib.epg_last_error()
    assert tr(col0=13) == -1                                     # columns 13 .. 16 in rows of 16
    assert tr(cols=None) == -1 and tr(X=None) == -1
    assert tr(cols=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.epg_last_error()
    assert tr(nb=0, cols=None, X=None) == 0 and tr(R=0, cols=None, X=None) == 0     # nothing to do, whatever the pointers are


# ---- which files ----------------------------------------------------------------------------------------------------------

def _tree(tmp_path, names, biosamples, chroms):
    d = tmp_path / "calls"
    d.mkdir()
    for n in names:
        (d / n).write_text("x\tchr\nh\n1\n")
    meta = tmp_path / "meta.txt"
    meta.write_text("id\tother\n" + "".join("%s\tz\n" % b for b in biosamples))
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("".join("%s\t1000\n" % c for c in chroms))
    return d, meta, sizes


def test_find_calls_follows_the_metadata_and_chromsizes_order(tmp_path):
    names = ["A_18_chr1_statebyline.txt.gz", "B_18_chr1_statebyline.txt", "C_18_chr1_statebyline.txt.gz",
             "A_18_chr2_statebyline.txt.gz", "C_18_chr2_statebyline.txt.gz", "A_18_chr10_statebyline.txt.gz", "notes_chr1.md"]
    d, meta, sizes = _tree(tmp_path, names, ["C", "A", "B"], ["chr2", "chr1", "chrX", "chr10"])
    got = sbl.find_calls(d, meta, sizes)
    assert [c for c, _f in got] == ["chr2", "chr1", "chr10"]                          # chromsizes order; chrX has no file: skipped
    by = {c: [f.name for f in fs] for c, fs in got}
    assert by["chr1"] == [names[2], names[0], names[1]]                              # metadata order beats directory order
    assert by["chr2"] == [names[4], names[3]]                                        # B is missing for chr2 only
    assert by["chr10"] == [names[5]]                                                 # `chr1_` does not match chr10
    assert all(f.parent == d for _c, fs in got for f in fs)
    every = list(sbl.iter_calls(d, meta, sizes))
    assert [c for c, _f in every] == ["chr2", "chr1", "chrX", "chr10"] and every[2][1] == []


def test_find_calls_refuses_two_files_for_one_biosample(tmp_path):
    names = ["A_18_chr1_statebyline.txt.gz", "A_15_chr1_statebyline.txt.gz"]
    d, meta, sizes = _tree(tmp_path, names, ["A"], ["chr1"])
    with pytest.raises(ValueError) as e:
        sbl.find_calls(d, meta, sizes)
    assert names[0] in str(e.value) and names[1] in str(e.value)


def test_header_chromosome_row_count_and_lenient_parse():
    a = np.frombuffer(b"BSS1\tchr7\nMaxState E\n3\n12\n", dtype=np.uint8)
    assert sbl.header_chromosome(a) == "chr7" and sbl.count_rows_text(a) == 2
    assert sbl.count_rows_text(a[:-1]) == 2 and sbl.count_rows_text(a[:10]) == 0 and sbl.count_rows_text(a[:0]) == 0
    col, lo, hi = sbl.parse_lenient(np.frombuffer(b"h\th\r\nh\r\n3\r\n 12 \r\n+7\n\n", dtype=np.uint8))
    assert col.dtype == np.int8 and col.tolist() == [2, 11, 6] and (lo, hi) == (3, 12)
    for bad in (b"h\nh\nx\n", b"h\nh\n0\n", b"h\nh\n128\n", b"h\nh\n1.5\n", b"h\n"):
        with pytest.raises(ValueError):
            sbl.parse_lenient(np.frombuffer(bad, dtype=np.uint8), "f")


# ---- the binary matrix file -----------------------------------------------------------------------------------------------

def _text_matrix(path, x0, chrom="chr1"):
    path.write_text("".join("%s\t%d\t%d\t%s\n" % (chrom, 200 * r, 200 * r + 200, "\t".join(str(int(v) + 1) for v in x0[r])) for r in range(len(x0))))
    return path


def _padded(R, N):
    return np.full((R, (N + 15) // 16 * 16), 77, dtype=np.int8)


def _same_read(a, b, whole=True):
    """The range is the header's pair, the whole file's; the text reader's is that of the lines it parsed, so the two are
    compared where the whole file is read."""
    assert a[0].dtype == np.int8 and a[0].shape == b[0].shape and np.array_equal(a[0], b[0])
    assert a[1].blob.dtype == b[1].blob.dtype and np.array_equal(a[1].blob, b[1].blob)
    assert a[1].offsets.dtype == b[1].offsets.dtype and np.array_equal(a[1].offsets, b[1].offsets)
    assert len(a) == len(b)
    if len(a) == 3 and whole:
        assert tuple(a[2]) == tuple(b[2])


@pytest.fixture()
def pair(tmp_path):
    """A small matrix as text and as .epgm: 700 rows (coordinates of 1 .. 6 digits), 10 biosamples, states 2 .. 17 as written."""
    rng = np.random.default_rng(5)
    x0 = rng.integers(1, 17, size=(700, 10)).astype(np.int8)
    txt = _text_matrix(tmp_path / "matrix_chr1.txt", x0)
    epgm = sbl.write_epgm(tmp_path / "matrix_chr1.epgm", x0, "chr1", (int(x0.min()) + 1, int(x0.max()) + 1))
    return x0, txt, epgm


@pytest.mark.parametrize("rows", [None, (0, 700), (0, 1), (3, 58), (499, 501), (650, 900), (700, 700), (5, 5)])
def test_epgm_reads_like_the_text_matrix(pair, rows):
    _x0, txt, epgm = pair
    _same_read(helpers.readTable(epgm, rows), helpers.readTable(txt, rows))
    whole = rows in (None, (0, 700))
    _same_read(helpers.readTable(epgm, rows, with_range=True), helpers.readTable(txt, rows, with_range=True), whole)
    _same_read(helpers.readTable(epgm, rows, alloc=_padded, with_range=True), helpers.readTable(txt, rows, alloc=_padded, with_range=True), whole)
    assert helpers.readTable(epgm, rows, with_range=True)[2] == (2, 17)              # the header's pair, whatever the rows
    got = helpers.readTable(epgm, rows, alloc=_padded)[0]
    assert got.shape[1] == 16 and (got[:, 10:] == -1).all()


def test_epgm_row_count_comes_from_the_header(pair, tmp_path, monkeypatch):
    _x0, txt, epgm = pair
    log = tmp_path / "io.log"
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    assert helpers.countRows(epgm) == helpers.countRows(txt) == 700
    assert [l.split("\t")[1] for l in log.read_text().splitlines()] == ["count"]    # the text file was counted; the binary one was not read
    from epilogos_amd import driver
    assert driver._cached_rows(epgm) == 700 and driver._cached_rows(txt) is None
    assert helpers.fileStem(epgm) == helpers.fileStem(txt) == "matrix_chr1"


def test_epgm_is_not_cached(pair, tmp_path, monkeypatch):
    _x0, _txt, epgm = pair
    cache = tmp_path / "cache"
    monkeypatch.setenv("EPILOGOS_CACHE_DIR", str(cache))
    helpers.readTable(epgm, (0, 10))
    helpers.flushCacheWrites()
    assert not cache.exists() or not list(cache.iterdir())


def test_epgm_values_above_the_state_limit_read_as_no_state(tmp_path):
    x0 = np.array([[0, 30, 31, 126], [17, 18, 99, 5]], dtype=np.int8)
    txt = _text_matrix(tmp_path / "m.txt", x0)
    epgm = sbl.write_epgm(tmp_path / "m.epgm", x0, "chr1", (1, 127))
    try:
        for states in (18, 40):
            _io.set_state_limit(states)
            a, b = helpers.readTable(epgm, with_range=True), helpers.readTable(txt, with_range=True)
            _same_read(a, b)
            assert a[0][0].tolist() == ([0, 30, -1, -1] if states == 18 else [0, 30, 31, 126])
    finally:
        _io.set_state_limit(18)


def test_epgm_header_layout_and_refusals(pair, tmp_path):
    x0, _txt, epgm = pair
    raw = epgm.read_bytes()
    assert len(raw) == 128 + 700 * 10 and raw[:8] == b"EPGM1\0\0\0"
    assert np.frombuffer(raw[8:32], dtype="<i8").tolist() == [700, 10, 10]
    assert np.frombuffer(raw[32:48], dtype="<i4").tolist() == [200, int(x0.min()) + 1, int(x0.max()) + 1, 0]
    assert raw[48:128] == b"chr1" + b"\0" * 76
    assert np.array_equal(np.frombuffer(raw[128:], dtype=np.int8).reshape(700, 10), x0)
    h = sbl.read_epgm_header(epgm)
    assert (h["R"], h["N"], h["width"], h["chrom"]) == (700, 10, 200, "chr1")
    cases = {"magic.epgm": b"EPGM2" + raw[5:], "short.epgm": raw[:-1], "head.epgm": raw[:100], "long.epgm": raw + b"\0",
             "rows.epgm": raw[:8] + np.array([701], dtype="<i8").tobytes() + raw[16:], "empty.epgm": b""}
    for name, blob in cases.items():
        p = tmp_path / name
        p.write_bytes(blob)
        for fn in (helpers.readTable, helpers.countRows):
            with pytest.raises(_io.EpilogosIOError) as e:
                fn(p)
            assert name in str(e.value), name
    with pytest.raises(_io.EpilogosIOError):
        helpers.countRows(tmp_path / "missing.epgm")
    empty = sbl.write_epgm(tmp_path / "none.epgm", np.zeros((0, 10), dtype=np.int8), "chrM", (0, 0))
    st, loc, rng = helpers.readTable(empty, with_range=True)
    assert st.shape == (0, 10) and len(loc) == 0 and rng == (0, 0) and helpers.countRows(empty) == 0


def test_synth_locations_at_large_coordinates():
    loc = sbl.synth_locations("chrUn_gl000220", 1246250, 1246253)
    assert loc.blob.tobytes() == (b"chrUn_gl000220\t249250000\t249250200\nchrUn_gl000220\t249250200\t249250400\n"
                                  b"chrUn_gl000220\t249250400\t249250600\n")
    assert loc.offsets.tolist() == [0, 35, 70, 105]
    s, e = loc.start_end()
    assert s.tolist() == [249250000, 249250200, 249250400] and e.tolist() == [249250200, 249250400, 249250600]


# ---- the reference's own matrix -------------------------------------------------------------------------------------------

def numpy_matrix(texts):
    """The matrix of state-by-line texts in plain numpy: split lines, int - 1, stack columns.  -> (int8 [R, N], chromosome)."""
    cols, chrom = [], None
    for t in texts:
        lines = bytes(t).decode().split("\n")
        if lines[-1] == "":
            lines.pop()
        chrom = chrom or lines[0].split()[1]
        cols.append(np.array([int(l) - 1 for l in lines[2:]], dtype=np.int8))
    return np.stack(cols, axis=1), chrom


def test_golden_matrix_equals_the_numpy_builders_epgm(tmp_path, golden_real):
    x, chrom = numpy_matrix([GOLD["text_%d" % k] for k in range(10)])
    assert x.shape == (2048, 10) and chrom == "chr1"
    # the same slice as the real-slice fixture, whose columns follow the reference's own metadata file
    assert sorted(c.tobytes() for c in x.T) == sorted(c.tobytes() for c in golden_real["x"].T)
    txt = tmp_path / "matrix_chr1.txt"
    txt.write_bytes(GOLD["matrix"].tobytes())
    epgm = sbl.write_epgm(tmp_path / "matrix_chr1.epgm", x, chrom, (int(x.min()) + 1, int(x.max()) + 1))
    for rows in (None, (1000, 1100)):
        _same_read(helpers.readTable(epgm, rows, alloc=_padded, with_range=True), helpers.readTable(txt, rows, alloc=_padded, with_range=True), rows is None)


def test_golden_names_follow_the_selection_rule(tmp_path):
    d = tmp_path / "calls"
    d.mkdir()
    for k, n in enumerate(GOLD["names"]):
        (d / str(n)).write_bytes(GOLD["text_%d" % k].tobytes())
    (tmp_path / "meta.txt").write_bytes(GOLD["metadata"].tobytes())
    (tmp_path / "sizes.txt").write_bytes(GOLD["chromsizes"].tobytes())
    got = sbl.find_calls(d, tmp_path / "meta.txt", tmp_path / "sizes.txt")
    assert [c for c, _f in got] == ["chr1"] and [f.name for f in got[0][1]] == [str(n) for n in GOLD["names"]]


def test_preprocess_command_needs_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from epilogos_amd import preprocess
    with pytest.raises(_abi.EpilogosHipError):
        preprocess.run(tmp_path, tmp_path / "m", tmp_path / "c", tmp_path / "out")


def test_console_script_of_the_packaging_resolves():
    import importlib

    import tomli
    root = Path(__file__).resolve().parents[1]
    target = tomli.loads((root / "pyproject.toml").read_text())["project"]["scripts"]["epilogos-prep"]
    mod, fn = target.split(":")
    assert callable(getattr(importlib.import_module(mod), fn))
    assert "epilogos-prep = %s" % target in (root / "setup.py").read_text()
