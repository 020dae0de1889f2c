"""ChromHMM segment files, the host side (no GPU): which file is which biosample's, the rules across files, the lenient host
parser on every form it takes and every error of content it raises (file:line), the header's constants, the entry points'
argument checks, and the command line.  Expected columns are np.repeat over the runs."""
import ctypes
import re

import numpy as np
import pytest
from click.testing import CliRunner

from epilogos_amd import _abi, preprocess, segments as seg, stateByLine as sbl


# ---- which files ----------------------------------------------------------------------------------------------------------

def _tree(tmp_path, names, biosamples, chromsizes="chr1\t1000\nchr2\t600\n"):
    d = tmp_path / "calls"
    d.mkdir()
    for n in names:
        (d / n).write_text("chr1\t0\t200\tE1\n")
    meta = tmp_path / "meta.txt"
    meta.write_text("id\tother\n" + "".join("%s\tz\n" % b for b in biosamples))
    sizes = tmp_path / "sizes.txt"
    sizes.write_text(chromsizes)
    return d, meta, sizes


def test_find_segments_one_none_and_two_matches(tmp_path):
    names = ["A_18_segments.bed.gz", "B_18_segments.bed", "C_18_dense.bed", ".D_18_segments.bed", "E_18_segments.bed", "E2_18_segments.bed"]
    d, meta, _sizes = _tree(tmp_path, names, ["B", "C", "A", "D"])
    assert [f.name for f in seg.find_segments(d, meta)] == [names[1], names[0]]      # metadata order; C and D have no column
    assert all(f.parent == d for f in seg.find_segments(d, meta))
    meta.write_text("id\nE\n")
    with pytest.raises(ValueError) as e:
        seg.find_segments(d, meta)
    assert names[4] in str(e.value) and names[5] in str(e.value)
    meta.write_text("id\nE_\n")
    assert [f.name for f in seg.find_segments(d, meta)] == [names[4]]


def test_read_chromsizes_keeps_the_file_order(tmp_path):
    p = tmp_path / "sizes.txt"
    p.write_text("chr2\t600\nchr10\t1000\nchrM\n\nchr1\t249250621\textra\n")
    assert seg.read_chromsizes(p) == (["chr2", "chr10", "chrM", "chr1"], {"chr2": 600, "chr10": 1000, "chr1": 249250621})


def test_check_files_wants_the_same_chromosomes_and_rows_everywhere():
    files, chroms = ["f0", "f1", "f2"], ["chr1", "chr2", "chrX"]
    same = [{"chr2": 3, "chr1": 5}] * 3
    assert seg.check_files(files, chroms, same, 200, {"chr1": 1000, "chr2": 401}) == {"chr1": 5, "chr2": 3}
    assert list(seg.check_files(files, chroms, same)) == ["chr1", "chr2"]             # table order; chrX in no file: skipped
    with pytest.raises(ValueError) as e:
        seg.check_files(files, chroms, [{"chr1": 5, "chr2": 3}, {"chr1": 5}, {"chr1": 5, "chr2": 3}])
    assert "chr2" in str(e.value) and "f0" in str(e.value) and "f1" in str(e.value)
    with pytest.raises(ValueError) as e:
        seg.check_files(files, chroms, [{"chr1": 5}, {"chr1": 5}, {"chr1": 4}])
    assert "chr1" in str(e.value) and "f0" in str(e.value) and "f2" in str(e.value) and "5" in str(e.value) and "4" in str(e.value)
    with pytest.raises(ValueError) as e:                                              # R_c against CHROMSIZES: ceil(999 / 200) = 5
        seg.check_files(files, chroms, [{"chr1": 6}] * 3, 200, {"chr1": 999})
    assert "chr1" in str(e.value) and "999" in str(e.value)
    assert seg.check_files(files, chroms, [{"chr1": 5}] * 3, 200, {"chr1": 999}) == {"chr1": 5}
    assert seg.check_files(files, chroms, [{"chr1": 6}] * 3, 200, {"chr2": 1}) == {"chr1": 6}      # no size known: no bound


def test_a_chromosome_missing_from_some_files_raises_and_unknown_ones_are_ignored(tmp_path):
    texts = [b"chr1\t0\t400\tE1\nchrUn\t0\t200\tE2\nchr2\t0\t200\tE3\n", b"chrUn\t200\t400\tE9\nchr1\t0\t400\tE2\n"]
    chroms = ["chr1", "chr2"]
    got = [seg.parse_host(t, "f%d" % k, chroms) for k, t in enumerate(texts)]
    assert [sorted(g) for g in got] == [["chr1", "chr2"], ["chr1"]]                   # chrUn, even off the rules: ignored as a whole run
    rows = [{c: len(v[0]) for c, v in g.items()} for g in got]
    with pytest.raises(ValueError) as e:
        seg.check_files(["f0", "f1"], chroms, rows)
    assert "chr2" in str(e.value) and "f0" in str(e.value) and "f1" in str(e.value)


# ---- the host parser ------------------------------------------------------------------------------------------------------

RUNS = [("chr1", 0, 3, 7), ("chr1", 3, 4, 12), ("chr1", 4, 20, 1), ("chr2", 0, 1, 127), ("chr2", 1, 6, 3)]


def _want(runs, chrom):
    r = [x for x in runs if x[0] == chrom]
    v = np.array([x[3] for x in r])
    return np.repeat((v - 1).astype(np.int8), [x[2] - x[1] for x in r]), int(v.min()), int(v.max())


def _same(got, runs, chroms):
    assert sorted(got) == sorted(chroms)
    for c in chroms:
        col, lo, hi = _want(runs, c)
        assert got[c][0].dtype == np.int8 and np.array_equal(got[c][0], col) and got[c][1:] == (lo, hi), c


def _lines(runs, w=200, label="E%d"):
    return ["%s\t%d\t%d\t%s" % (c, a * w, b * w, label % s) for c, a, b, s in runs]


def test_host_parser_reads_the_strict_form_and_every_lenient_one(tmp_path):
    chroms = ["chr2", "chr1"]
    plain = "\n".join(_lines(RUNS)) + "\n"
    _same(seg.parse_host(plain.encode(), "f", chroms), RUNS, chroms)
    _same(seg.parse_host(np.frombuffer(plain[:-1].encode(), dtype=np.uint8), "f", chroms), RUNS, chroms)
    _same(seg.parse_host(plain.replace("\n", "\r\n").encode(), "f", chroms), RUNS, chroms)                  # CRLF
    _same(seg.parse_host(plain.replace("\t", " \t ").encode(), "f", chroms), RUNS, chroms)                  # blanks around fields
    _same(seg.parse_host("\n".join(_lines(RUNS, 20, "%d")).encode(), "f", chroms, width=20), RUNS, chroms)
    _same(seg.parse_host(plain.encode(), "f", ["chr1"]), RUNS, ["chr1"])
    dense = 'track name="x" description="y" visibility=1 itemRgb="On"\nbrowser position chr1\n# note\n\n' + "".join(
        "%s\t%d\t%d\t%d\t0\t.\t%d\t%d\t255,0,0\n" % (c, a * 200, b * 200, s, a * 200, b * 200) for c, a, b, s in RUNS)
    _same(seg.parse_host(dense.encode(), "x_dense.bed", chroms), RUNS, chroms)                              # 9 fields, a track line
    numbered = "\n".join(_lines(RUNS, label="%d_TssFlnkU")) + "\n"
    _same(seg.parse_host(numbered.encode(), "f", chroms), RUNS, chroms)                                     # matched by number, no table


def test_host_parser_resolves_names_through_the_state_metadata(tmp_path):
    meta = tmp_path / "states.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\tlong_name\n0\t1\tTssA\tActive TSS\n1\t2\tTssFlnk\tFlanking TSS\n2\t3\tQuies\tQuiescent\n")
    table = seg.read_state_names(meta)
    assert table == {"TssA": 1, "TssFlnk": 2, "Quies": 3}
    text = b"chr1\t0\t200\tTssFlnk\nchr1\t200\t600\tQuies\nchr1\t600\t800\tTssA\nchr1\t800\t1000\t3_TssFlnkU\n"
    got = seg.parse_host(text, "f", ["chr1"], state_names=table)
    assert got["chr1"][0].tolist() == [1, 2, 2, 0, 2] and got["chr1"][1:] == (1, 3)
    with pytest.raises(ValueError) as e:
        seg.parse_host(text, "named.bed", ["chr1"])
    assert "named.bed:1" in str(e.value) and "TssFlnk" in str(e.value)
    with pytest.raises(ValueError) as e:
        seg.parse_host(text.replace(b"Quies", b"Het"), "named.bed", ["chr1"], state_names=table)
    assert "named.bed:2:" in str(e.value)
    table["ZNF/Rpts"] = 4
    assert seg.parse_host(b"chr1\t0\t200\t1234_ZNF/Rpts\nchr1\t200\t400\t12_ZNF/Rpts\n", "f", ["chr1"], state_names=table)["chr1"][0].tolist() == [3, 11]
    (tmp_path / "bad.tsv").write_text("a\tb\n1\t2\n")
    with pytest.raises(ValueError):
        seg.read_state_names(tmp_path / "bad.tsv")


CONTENT_ERRORS = {
    "a gap": (["chr1\t0\t400\tE1", "chr1\t600\t800\tE2"], 2),
    "an overlap": (["chr1\t0\t400\tE1", "chr1\t200\t800\tE2"], 2),
    "end == start": (["chr1\t0\t400\tE1", "chr1\t400\t800\tE1", "chr1\t800\t800\tE2"], 3),
    "end < start": (["chr1\t0\t400\tE1", "chr1\t400\t200\tE2"], 2),
    "a start off the grid": (["chr1\t0\t400\tE1", "chr1\t400\t500\tE1", "chr1\t500\t600\tE2"], 2),
    "state 0": (["chr1\t0\t400\tE0"], 1),
    "state 128": (["chr2\t0\t400\tE1", "chr1\t0\t400\tE128"], 2),
    "a chromosome in two runs": (["chr1\t0\t400\tE1", "chr2\t0\t400\tE1", "chrUn\t0\t200\tE1", "chr1\t400\t600\tE2"], 4),
    "a first start other than 0": (["chr2\t0\t400\tE1", "chr1\t200\t400\tE1"], 2),
    "a name that cannot be resolved": (["chr1\t0\t400\tE1", "chr1\t400\t600\tEnh"], 2),
    "three fields": (["chr1\t0\t400\tE1", "chr1\t400\t600"], 2),
    "a signed coordinate": (["chr1\t0\t400\tE1", "chr1\t+400\t600\tE1"], 2),
}


@pytest.mark.parametrize("what", sorted(CONTENT_ERRORS))
def test_host_parser_raises_on_errors_of_content_with_file_and_line(what):
    lines, at = CONTENT_ERRORS[what]
    for head, shift in (("", 0), ("track name=x\n\n", 2)):       # skipped lines count: the number is the file's
        for eol in ("\n", "\r\n"):
            text = (head + eol.join(lines) + eol).encode()
            with pytest.raises(ValueError) as e:
                seg.parse_host(text, "dir/some_segments.bed", ["chr1", "chr2"])
            assert "dir/some_segments.bed:%d:" % (at + shift) in str(e.value), (what, str(e.value))


# ---- the header's constants and the entry points' checks (tests/test_abi_symbols.py holds the header against its binding) ---

def test_constants_and_argument_validation_without_gpu():
    lib = _abi.load()
    hdr = _abi.HEADERS["segments"].path.read_text()
    which = {n: int(v) for n, v in re.findall(r"#define EPG_SEG_(THREAD_BYTES|BLOCK_BYTES|EXPAND_TILE_BINS|MAX_CHROMS) (\d+)", hdr)}
    assert sorted(which.values()) == [0, 1, 2, 3]
    tb, bb = lib.epg_seg_constant(which["THREAD_BYTES"]), lib.epg_seg_constant(which["BLOCK_BYTES"])
    assert tb >= 4 and bb > tb and bb % tb == 0
    maxc = lib.epg_seg_constant(which["MAX_CHROMS"])
    assert lib.epg_seg_constant(which["EXPAND_TILE_BINS"]) % 16 == 0 and maxc >= 1024
    assert lib.epg_seg_constant(4) == -1 and lib.epg_seg_constant(-1) == -1
    assert int(re.search(r"#define EPG_SEG_NAME_BYTES (\d+)", hdr).group(1)) == seg.NAME_BYTES == 80
    assert lib.epg_seg_ws_bytes(-1, 1) == -1 and lib.epg_seg_ws_bytes(0x7fff0001, 1) == -1
    assert lib.epg_seg_ws_bytes(10, -1) == -1 and lib.epg_seg_ws_bytes(10, maxc + 1) == -1
    assert lib.epg_seg_ws_bytes(0, 0) > 0 and lib.epg_seg_ws_bytes(1 << 24, maxc) > lib.epg_seg_ws_bytes(1 << 20, 24)
    x = ctypes.c_void_p(4096)
    ok = dict(text=x, n=1000, names=x, nchrom=3, width=200, first=x, state=x, cap=10, runs=x, info=x, ws=x, wsb=1 << 20)

    def parse(**kw):
        a = dict(ok, **kw)
        return lib.epg_seg_parse(a["text"], a["n"], a["names"], a["nchrom"], a["width"], a["first"], a["state"], a["cap"], a["runs"],
                                 a["info"], a["ws"], a["wsb"], None)
    assert parse(n=-1) == -1 and parse(n=0x7fff0001) == -1 and parse(cap=-1) == -1
    assert parse(width=0) == -1 and b"width" in lib.epg_last_error() and parse(width=-200) == -1
    assert parse(nchrom=-1) == -1 and parse(nchrom=maxc + 1) == -1 and b"chromosomes" in lib.epg_last_error()
    for name in ("text", "names", "first", "state", "runs", "info", "ws"):
        assert parse(**{name: None}) == -1 and b"NULL" in lib.epg_last_error(), name
    assert parse(ws=ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.epg_last_error()
    assert parse(info=ctypes.c_void_p(4100)) == -1 and parse(runs=ctypes.c_void_p(4100)) == -1 and parse(first=ctypes.c_void_p(4098)) == -1
    assert parse(wsb=lib.epg_seg_ws_bytes(1000, 3) - 1) == -4

    def expand(first=x, state=x, runs=x, c=0, col=x, R=100):
        return lib.epg_seg_expand(first, state, runs, c, col, R, None)
    assert expand(c=-1) == -1 and expand(c=maxc) == -1 and expand(R=-1) == -1 and expand(R=1 << 31) == -1
    for name in ("first", "state", "runs", "col"):
        assert expand(**{name: None}) == -1 and b"NULL" in lib.epg_last_error(), name
    assert expand(col=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.epg_last_error()
    assert expand(first=ctypes.c_void_p(4098)) == -1 and expand(runs=ctypes.c_void_p(4100)) == -1
    assert expand(R=0, first=None, state=None, runs=None, col=None) == 0              # nothing to do, whatever the pointers are


def test_name_table_is_nul_padded_and_bounded():
    t = seg.name_table(["chr1", "c" * 79])
    assert t.shape == (2, 80) and t.dtype == np.uint8 and t[0].tobytes() == b"chr1" + b"\0" * 76 and t[1].tobytes() == b"c" * 79 + b"\0"
    for bad in ("", "c" * 80):
        with pytest.raises(ValueError):
            seg.name_table([bad])


# ---- the command line -----------------------------------------------------------------------------------------------------

def test_command_without_segments_still_selects_state_by_line_files(tmp_path, monkeypatch):
    d, meta, sizes = _tree(tmp_path, ["A_18_segments.bed", "A_18_chr1_statebyline.txt"], ["A"])
    calls = []
    monkeypatch.setattr(preprocess, "run", lambda *a, **kw: calls.append((a, kw)))
    args = [str(d), str(meta), str(sizes), "-o", str(tmp_path / "out")]
    assert CliRunner().invoke(preprocess.main, args).exit_code == 0
    assert calls[-1][1] == dict(segments=False, width=200, state_names=None)
    assert [(c, [f.name for f in fs]) for c, fs in sbl.iter_calls(d, meta, sizes)] == [("chr1", ["A_18_chr1_statebyline.txt"]), ("chr2", [])]
    assert CliRunner().invoke(preprocess.main, args + ["--segments", "--bin-width", "20"]).exit_code == 0
    assert calls[-1][1] == dict(segments=True, width=20, state_names=None)
    n = len(calls)
    for extra in (["--segments", "--bin-width", "0"], ["--bin-width", "0"], ["--segments", "--bin-width", "-200"], ["--bin-width", "20"]):
        res = CliRunner().invoke(preprocess.main, args + extra)
        assert res.exit_code == 2 and "Usage" in res.output, extra               # a usage error: nothing was run
    assert len(calls) == n
