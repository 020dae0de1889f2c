"""The state census, the host side (no GPU; tests/test_abi_symbols.py holds include/epilogos_census.h against its binding): the entry
point's argument checks (made before the first HIP call), the table's text from given arrays, and the command lines."""
import ctypes

import numpy as np

from epilogos_amd import _abi, census


def test_argument_validation_without_gpu():
    lib = _abi.load()
    assert lib.epg_version() == 2
    x = ctypes.c_void_p(4096)
    ok = dict(X=x, R=10, N=20, ldx=32, S=18, census=x, other=x, first_bad=x)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.epg_state_census(a["X"], a["R"], a["N"], a["ldx"], a["S"], a["census"], a["other"], a["first_bad"], None)
    assert call(R=-1) == -1 and b"bad shape" in lib.epg_last_error()
    assert call(S=0) == -1 and b"S=0" in lib.epg_last_error()
    assert call(S=128) == -2 and b"S=128" in lib.epg_last_error()
    assert call(N=65536, ldx=65536) == -2 and b"65535" in lib.epg_last_error()
    assert call(ldx=19) == -1 and b"bad shape" in lib.epg_last_error()
    assert call(N=-1) == -1
    assert call(N=0, ldx=0) == -1                              # ldx >= max(N, 1)
    assert call(census=None) == -1 and b"census is NULL" in lib.epg_last_error()
    assert call(X=None) == -1 and b"X is NULL" in lib.epg_last_error()
    # the unsupported sizes are named before a NULL pointer is
    assert call(S=200, census=None) == -2
    # nothing to do: valid, no HIP call, X is not looked at
    assert call(R=0) == 0 and call(R=0, X=None) == 0
    assert call(N=0, ldx=1) == 0 and call(N=0, ldx=16, other=None, first_bad=None) == 0


# ---- the table ---------------------------------------------------------------------------------------------------------------

def _state_file(tmp_path, S, short=True):
    p = tmp_path / ("states_%d_%d.tsv" % (S, short))
    if short:
        p.write_text("zero_index\tone_index\tshort_name\tlong_name\n" + "".join("%d\t%d\tSt%d\tstate %d\n" % (i, i + 1, i + 1, i + 1) for i in range(S)))
    else:
        p.write_text("zero_index\tone_index\tlong_name\n" + "".join("%d\t%d\tstate %d\n" % (i, i + 1, i + 1) for i in range(S)))
    return p


def test_state_headers(tmp_path):
    assert census.state_headers(_state_file(tmp_path, 3), 3) == ["St1", "St2", "St3"]
    assert census.state_headers(_state_file(tmp_path, 3, short=False), 3) == ["1", "2", "3"]
    assert census.state_headers(None, 2) == ["1", "2"]


def test_table_from_given_arrays(tmp_path):
    c1 = np.array([[5, 0, 2], [1, 1, 1]])
    c2 = np.array([[0, 0, 4], [2, 2, 0]])
    entries = [("chr1", c1, np.array([0, 4]), 7, ["BSS1", "BSS2"]), ("chr2", c2, np.array([0, 0]), 4, ["BSS1"])]
    lines = census.table_lines(entries, census.state_headers(_state_file(tmp_path, 3), 3))
    assert lines == ["chrom\tcolumn\tbiosample\tbins\tnot_a_state\tSt1\tSt2\tSt3",
                     "chr1\t1\tBSS1\t7\t0\t5\t0\t2", "chr1\t2\tBSS2\t7\t4\t1\t1\t1",
                     "chr2\t1\tBSS1\t4\t0\t0\t0\t4", "chr2\t2\t.\t4\t0\t2\t2\t0",
                     "all\t1\tBSS1\t11\t0\t5\t0\t6", "all\t2\t.\t11\t4\t3\t3\t1"]
    for l in lines[1:]:
        f = l.split("\t")
        assert int(f[3]) == int(f[4]) + sum(int(v) for v in f[5:])
    # no names: `.`; files of different widths: no genome-wide lines
    entries = [("chr1", c1, np.array([0, 4]), 7, None), ("chrX", np.array([[3, 0, 0]]), np.array([0]), 3, None)]
    lines = census.table_lines(entries, census.state_headers(_state_file(tmp_path, 3, short=False), 3))
    assert lines == ["chrom\tcolumn\tbiosample\tbins\tnot_a_state\t1\t2\t3", "chr1\t1\t.\t7\t0\t5\t0\t2", "chr1\t2\t.\t7\t4\t1\t1\t1",
                     "chrX\t1\t.\t3\t0\t3\t0\t0"]
    out = tmp_path / "t.tsv"
    census.write_table(out, entries, ["1", "2", "3"])
    assert out.read_text() == "\n".join(lines) + "\n"


def test_names(tmp_path):
    meta = tmp_path / "meta.txt"
    meta.write_text("biosample\ttissue\nBSS01\tliver\nBSS02\theart\nBSS03\tlung\n")
    names = census.read_names(meta)
    assert names == ["BSS01", "BSS02", "BSS03"]
    from epilogos_amd import segments, stateByLine
    d = tmp_path / "data"
    d.mkdir()
    for n in ("x_BSS01_18_segments.bed.gz", "x_BSS03_18_segments.bed.gz", "BSS01_18_chr1_statebyline.txt", "BSS02_18_chr1_statebyline.txt",
              "BSS02_18_chr2_statebyline.txt"):
        (d / n).write_bytes(b"")
    files, found = segments.find_segments_named(d, meta)                         # a biosample without a file has no column, and no name
    assert [f.name for f in files] == ["x_BSS01_18_segments.bed.gz", "x_BSS03_18_segments.bed.gz"] and found == ["BSS01", "BSS03"]
    assert segments.find_segments(d, meta) == files
    sizes = tmp_path / "sizes.txt"
    sizes.write_text("chr1\t1000\nchr2\t1000\n")
    named = list(stateByLine.iter_calls_named(d, meta, sizes))
    assert [(c, [f.name for f in fs], ns) for c, fs, ns in named] == [
        ("chr1", ["BSS01_18_chr1_statebyline.txt", "BSS02_18_chr1_statebyline.txt"], ["BSS01", "BSS02"]),
        ("chr2", ["BSS02_18_chr2_statebyline.txt"], ["BSS02"])]
    assert list(stateByLine.iter_calls(d, meta, sizes)) == [(c, fs) for c, fs, _ns in named]
    assert census.offender_warning("f.epgm", 18, np.array([0, 2, 1]), 7 * 3 + 1, 3, 200) == \
        "WARNING: f.epgm: 3 byte(s) are not a state of the 18-state model; the first is byte 200 at row 7 (0-based), biosample 2"


def test_input_files_in_run_order(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    for n in ("matrix_chr10.epgm", "matrix_chr2.epgm", "matrix_chr1.epgm"):
        (d / n).write_bytes(b"")
    one = tmp_path / "single.txt.gz"
    one.write_bytes(b"")
    assert [p.name for p in census.input_files([d, one])] == ["matrix_chr1.epgm", "matrix_chr2.epgm", "matrix_chr10.epgm", "single.txt.gz"]


# ---- the command lines -------------------------------------------------------------------------------------------------------

def test_command_lines_parse(tmp_path):
    from click.testing import CliRunner
    from epilogos_amd import preprocess, run
    out = CliRunner().invoke(census.main, ["--help"]).output
    for opt in ("-i", "-j", "-o", "--names"):
        assert opt in out
    assert CliRunner().invoke(census.main, ["-i", str(tmp_path)]).exit_code == 2           # -j is required
    assert CliRunner().invoke(census.main, ["-j", str(_state_file(tmp_path, 3))]).exit_code == 2
    assert "--census" in CliRunner().invoke(preprocess.main, ["--help"]).output
    assert "--check-states" in CliRunner().invoke(run.main, ["--help"]).output
    # the option parses and today's checks follow it
    assert CliRunner().invoke(run.main, ["-i", "x", "-j", "j", "--check-states"]).output == "ERROR: [-o, --output-directory] is required\n"


def test_raw_is_an_argument_of_one_read(tmp_path):
    """read_epgm / readTable hand a .epgm file's bytes on unchanged only for the read that asks; the next read clamps again."""
    from epilogos_amd import _io, helpers, stateByLine
    _io.set_state_limit(18)
    p = tmp_path / "m.epgm"
    stateByLine.write_epgm(p, np.array([[0, 17, 33, -56]], dtype=np.int8), "chr1", (1, 18))
    assert helpers.readTable(p)[0].tolist() == [[0, 17, -1, -1]]
    assert helpers.readTable(p, raw=True)[0].tolist() == [[0, 17, 33, -56]]
    assert stateByLine.read_epgm(p, raw=True)[0].view(np.uint8).tolist() == [[0, 17, 33, 200]]
    assert helpers.readTable(p)[0].tolist() == [[0, 17, -1, -1]] and stateByLine.read_epgm(p)[0].tolist() == [[0, 17, -1, -1]]
    assert not hasattr(stateByLine, "keep_raw_bytes")                               # no process-wide switch


def test_verdict_key_orders_by_file_row_column():
    from epilogos_amd import driver
    key = driver._verdict_key
    assert key(0, 5, 3, 1) < key(0, 6, 0, 0) < key(1, 0, 0, 0)                      # file, then row ...
    assert key(2, 0, 9, 1) < key(2, 299, 0, 0)                                      # ... whatever the group (paired mode)
    assert key(2, 7, 3, 0) < key(2, 7, 3, 1) < key(2, 7, 4, 0)                      # the group only breaks a tie
    assert driver._verdict_fields(key(16383, 2 ** 31 - 1, 65535, 1)) == (16383, 2 ** 31 - 1, 65535, 1)
    assert key(16383, 2 ** 31 - 1, 65535, 1) < driver._KEY_NONE
    assert key(16384, 0, 0, 0) is None and key(0, 2 ** 31, 0, 0) is None and key(0, 0, 65536, 0) is None


def test_verdict_message_and_key():
    from epilogos_amd import driver
    msg = driver.state_check_message("/d/matrix_chr1.epgm", 120, 7, 200, 18)
    assert "/d/matrix_chr1.epgm" in msg and "row 120 " in msg and "biosample 7:" in msg and "byte 200 " in msg and "18-state" in msg
    assert msg.startswith("ERROR: [--check-states] ")
