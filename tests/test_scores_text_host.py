"""The GPU scores-text reader, the host side (no GPU): the header's status constants (tests/test_abi_symbols.py holds it against
its binding), the entry points' argument checks, chunk cutting, and similaritySearch_query.readGrid -- without a GPU, with the device step refusing
the file, and with the device step's results put together into mm.readScores' arrays."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import _abi, _io, scoresText
from epilogos_amd import similaritySearch_max_mean as mm
from epilogos_amd import similaritySearch_query as sq

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "simsearch.npz")


# ---- the header ---------------------------------------------------------------------------------------------------------------

def test_the_headers_status_constants_are_the_host_fronts():
    """(tests/test_abi_symbols.py holds the header against its binding and the library's exports.)"""
    hdr = _abi.HEADERS["scores_text"].path.read_text()
    for code, _text in scoresText.REASONS.items():
        assert re.search(r"#define EPGT_REASON_[A-Z]+ %d\b" % code, hdr)
    assert len(re.findall(r"#define EPGT_REASON_", hdr)) == len(scoresText.REASONS)
    assert "#define EPGT_CLEAN INT64_MAX" in hdr and scoresText.CLEAN == 2 ** 63 - 1


def test_argument_validation_without_gpu():
    lib = _abi.load()
    assert lib.epg_version() == 2
    assert lib.epgt_scores_ws_bytes(-1) == -1
    assert lib.epgt_scores_ws_bytes(0x7fff0001) == -1
    assert lib.epgt_scores_ws_bytes(0) > 0
    assert lib.epgt_scores_ws_bytes(1 << 20) >= 4 * ((1 << 20) + 1) + 4 * ((1 << 20) // 4096 + 2)
    x = ctypes.c_void_p(4096)
    ok = dict(text=x, n=1000, F=21, rows=5, row0=0, X=x, start=x, end=x, chrom=x, ws=x, wsb=1 << 20, status=x)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.epgt_scores_parse(a["text"], a["n"], a["F"], a["rows"], a["row0"], a["X"], a["start"], a["end"], a["chrom"], a["ws"],
                                     a["wsb"], a["status"], None)
    assert call(n=-1) == -1
    assert call(n=0x7fff0001) == -1
    assert call(F=3) == -1 and b"fields per row" in lib.epg_last_error()
    assert call(rows=-1) == -1
    assert call(rows=1001) == -1
    assert call(row0=-1) == -1
    for name in ("text", "X", "start", "end", "chrom", "ws", "status"):
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.epg_last_error()
    assert call(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.epg_last_error()
    assert call(wsb=lib.epgt_scores_ws_bytes(1000) - 1) == -4
    # a chunk of no bytes is valid and does nothing, whatever the pointers are
    assert call(n=0, rows=0, text=None, X=None, ws=None, status=None) == 0
    assert call(n=0, rows=1) == -1


# ---- chunk cutting --------------------------------------------------------------------------------------------------------

def _rows(n, S=3, seed=0):
    rng = np.random.default_rng(seed)
    return ["chr%d\t%d\t%d\t%s\n" % (1 + i // 7, 200 * i, 200 * i + 200, "\t".join("%.5f" % v for v in rng.normal(size=S) * 10 ** rng.integers(0, 4)))
            for i in range(n)]


@pytest.mark.parametrize("final_newline", [True, False])
def test_chunks_are_whole_rows(final_newline):
    rows = _rows(50)
    text = "".join(rows).encode()
    if not final_newline:
        text = text[:-1]
    longest = max(len(r) for r in rows)
    for chunk in [1, 5, len(rows[0]) - 1, len(rows[0]), len(rows[0]) + 1, longest, 3 * longest + 1, 1000, len(text) - 1, len(text), 10 * len(text)]:
        cuts = scoresText.cut_chunks(text, chunk)
        assert cuts[0][0] == 0 and cuts[-1][1] == len(text)
        assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and all(hi > lo for lo, hi in cuts)
        for lo, hi in cuts[:-1]:
            assert text[hi - 1:hi] == b"\n"
        pieces = [text[lo:hi] for lo, hi in cuts]
        assert b"".join(pieces) == text
        for (lo, hi), piece in zip(cuts, pieces):
            # as many rows as fit: one row more would pass the chunk size (unless the chunk is a single row longer than it)
            nxt = text.find(b"\n", hi)
            nxt = len(text) if nxt < 0 else nxt + 1
            assert hi - lo <= chunk or piece.rstrip(b"\n").count(b"\n") == 0
            assert hi == len(text) or nxt - lo > chunk
    assert scoresText.cut_chunks(b"", 10) == []
    assert scoresText.cut_chunks(np.frombuffer(text, dtype=np.uint8), len(rows[0])) == scoresText.cut_chunks(text, len(rows[0]))


def test_chunk_of_exactly_one_row():
    rows = ["a\t1\t2\t0.5\n"] * 4
    text = "".join(rows).encode()
    assert scoresText.cut_chunks(text, len(rows[0])) == [(i * len(rows[0]), (i + 1) * len(rows[0])) for i in range(4)]
    assert scoresText.cut_chunks(text[:-1], len(rows[0])) == [(0, 10), (10, 20), (20, 30), (30, 39)]
    assert scoresText.first_row_fields(np.frombuffer(text, dtype=np.uint8)) == 4
    assert scoresText.first_row_fields(np.frombuffer(b"a\tb", dtype=np.uint8)) == 2


def test_native_text_and_newline_count(tmp_path):
    import gzip
    text = "".join(_rows(3000, S=18)).encode()
    (tmp_path / "plain.txt").write_bytes(text)
    (tmp_path / "one.txt.gz").write_bytes(gzip.compress(text))
    (tmp_path / "multi.txt.gz").write_bytes(gzip.compress(text[:70000]) + gzip.compress(text[70000:]))
    (tmp_path / "empty.txt").write_bytes(b"")
    for name in ("plain.txt", "one.txt.gz", "multi.txt.gz"):
        with _io.Text(tmp_path / name) as t:
            assert t.data.tobytes() == text
            assert _io.count_newlines(t.data) == 3000 and _io.count_newlines(t.data[5:-1]) == 2999
    with _io.Text(tmp_path / "empty.txt") as t:
        assert len(t.data) == 0
    assert _io.count_newlines(np.zeros(0, dtype=np.uint8)) == 0
    big = np.full(40 << 20, 10, dtype=np.uint8)                  # enough for several counting threads
    big[::3] = 65
    assert _io.count_newlines(big, 4) == int((big == 10).sum())
    with pytest.raises(_io.EpilogosIOError):
        _io.Text(tmp_path / "missing.txt")


# ---- readGrid -------------------------------------------------------------------------------------------------------------

def _scores(tmp_path, case="s200"):
    p = tmp_path / ("scores_%s.txt" % case)
    p.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    return p


def _same(got, want):
    coords, genome = got
    _s, inputArr, grid = want
    assert genome.dtype == grid.dtype and np.array_equal(genome, grid)
    assert coords.dtype == object and coords.shape == (len(grid), 3)
    assert (coords == inputArr[:, :3]).all()
    assert [type(v) for v in coords[0]] == [type(v) for v in inputArr[0, :3]]


def test_read_grid_without_gpu_is_read_scores(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(scoresText, "read_scores_device", lambda *a, **k: pytest.fail("no GPU: the device reader must not run"))
    sp = _scores(tmp_path)
    _same(sq.readGrid(sp), mm.readScores(sp))


def test_not_strict_falls_back_and_names_the_row(tmp_path, monkeypatch, capsys):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)

    def refuse(path, *a, **k):
        raise scoresText.NotStrict(scoresText.REASONS[6], 1234)
    monkeypatch.setattr(scoresText, "read_scores_device", refuse)
    sp = _scores(tmp_path)
    _same(sq.readGrid(sp), mm.readScores(sp))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "row 1234" in out and scoresText.REASONS[6] in out and "pandas" in out
    # a file that to_grid refuses still raises to_grid's error
    bad = tmp_path / "offgrid.txt"
    bad.write_text("chr1\t0\t200\t0.123456\t1.00000\n")
    with pytest.raises(ValueError, match="not on the 1e-5 grid"):
        sq.readGrid(bad)


def test_device_results_become_read_scores_arrays(tmp_path, monkeypatch):
    """readGrid's assembly: the device reader's tensors and runs (here made from the pandas read) give mm.readScores' arrays, types
    of the elements included."""
    import torch
    sp = _scores(tmp_path, "s20")
    want = mm.readScores(sp)
    inputArr, grid = want[1], want[2]
    table = sq.chromosomeTable(inputArr[:, 0], inputArr[:, 1], inputArr[:, 2])
    runs = [(name, row0, row0 + len(starts)) for name, (row0, starts, _e) in table.items()]

    def device(path, *a, **k):
        return (torch.from_numpy(grid.astype(np.int32)), inputArr[:, 1].astype(np.int64), inputArr[:, 2].astype(np.int64), runs)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(scoresText, "read_scores_device", device)
    _same(sq.readGrid(sp), want)
