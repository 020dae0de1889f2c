"""The biosample concordance, the host side (no GPU; tests/test_abi_symbols.py holds include/epilogos_concordance.h against its
binding): the entry points' argument checks (made before the first HIP call), the two tables and the duplicate warning from
handmade matrices, the command lines, and `epilogos-prep --concordance` with the device stood in for by numpy."""
import ctypes
import io
import re

import click
import numpy as np
import pytest

from epilogos_amd import _abi, concordance
from tests.test_statebyline_host import GOLD, numpy_matrix


def restatement(x, S):
    """x: uint8 [R, N] -> (agree, both) int64 [N, N], the issue's definition."""
    x = np.asarray(x).view(np.uint8) if np.asarray(x).dtype == np.int8 else np.asarray(x, dtype=np.uint8)
    N = x.shape[1]
    valid = x < S
    agree, both = np.zeros((N, N), dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    for i in range(N):
        agree[i] = ((x[:, i:i + 1] == x) & valid[:, i:i + 1]).sum(axis=0)
        both[i] = (valid[:, i:i + 1] & valid).sum(axis=0)
    return agree, both


def test_argument_validation_without_gpu():
    lib = _abi.load()
    assert lib.epg_version() == 2
    x = ctypes.c_void_p(4096)
    ok = dict(X=x, R=100, N=20, ldx=32, S=18, agree=x, both=x, ws=x, ws_bytes=1 << 30)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.epg_concordance(a["X"], a["R"], a["N"], a["ldx"], a["S"], a["agree"], a["both"], a["ws"], a["ws_bytes"], None)
    assert call(R=-1) == -1 and b"bad shape" in lib.epg_last_error()
    assert call(N=0, ldx=0) == -1 and b"bad shape" in lib.epg_last_error()
    assert call(ldx=19) == -1 and b"bad shape" in lib.epg_last_error()
    assert call(S=0) == -1 and b"S=0" in lib.epg_last_error()
    assert call(S=128) == -2 and b"S=128" in lib.epg_last_error()
    assert call(N=65536, ldx=65536) == -2 and b"65535" in lib.epg_last_error()
    assert call(X=None) == -1 and b"X is NULL" in lib.epg_last_error()
    assert call(agree=None) == -1 and b"agree is NULL" in lib.epg_last_error()
    assert call(ws=None) == -1 and b"ws is NULL" in lib.epg_last_error()
    assert call(ws=ctypes.c_void_p(4096 + 64)) == -1 and b"aligned" in lib.epg_last_error()
    assert call(ws_bytes=255) == -4 and b"workspace" in lib.epg_last_error()
    # the unsupported sizes are named before a NULL pointer is, the shape before both
    assert call(S=200, agree=None) == -2 and call(S=200, R=-1) == -1
    # nothing to do: valid, no HIP call, no pointer is looked at
    assert call(R=0) == 0 and call(R=0, X=None, agree=None, both=None, ws=None, ws_bytes=0) == 0


def test_workspace_size():
    lib = _abi.load()
    size = lib.epg_concordance_ws_bytes
    assert size(-1, 20, 18) == -1 and size(10, 0, 18) == -1 and size(10, 20, 0) == -1 and size(10, 20, 128) == -1 and size(10, 65536, 18) == -1
    for R, N, S in ((0, 1, 1), (1, 1, 1), (1, 65535, 127), (31, 65535, 127), (32, 65535, 127), (33, 40000, 100), (2049, 33, 18), (70001, 9, 18),
                    (1246253, 833, 18), (1246253, 833, 127), (1 << 40, 65535, 127)):
        n = size(R, N, S)
        assert 256 <= n <= R * N + (1 << 20) and n % 256 == 0, (R, N, S, n)
    # the genome-sized call fits in one chunk: 24 bytes per 32 bins and column
    assert size(1246253, 833, 18) == -(-((1246253 + 31) // 32 * 896 * 24) // 256) * 256


# ---- the tables --------------------------------------------------------------------------------------------------------------

AGREE = np.array([[7, 1, 2], [1, 5, 0], [2, 0, 9]])
BOTH = np.array([[7, 4, 6], [4, 5, 5], [6, 5, 9]])


def test_table_header_rows_and_names():
    assert concordance.table_lines(AGREE, ["BSS1", "BSS2", "BSS3"]) == ["biosample\tBSS1\tBSS2\tBSS3", "BSS1\t7\t1\t2", "BSS2\t1\t5\t0", "BSS3\t2\t0\t9"]
    # no names: the 1-based column numbers; a list that is too short names what it can
    assert concordance.table_lines(AGREE) == ["biosample\t1\t2\t3", "1\t7\t1\t2", "2\t1\t5\t0", "3\t2\t0\t9"]
    assert concordance.table_lines(AGREE, ["BSS1"])[0] == "biosample\tBSS1\t2\t3"
    assert [l.split("\t")[0] for l in concordance.table_lines(AGREE, ["BSS1"])] == ["biosample", "BSS1", "2", "3"]
    for l in concordance.table_lines(BOTH, ["a", "b", "c"])[1:]:
        assert all(re.fullmatch(r"\d+", v) for v in l.split("\t")[1:])


def test_columns_select_and_order_rows_and_columns(tmp_path):
    from epilogos_amd.run import parseColumns
    names = ["BSS1", "BSS2", "BSS3"]
    assert concordance.table_lines(AGREE, names, parseColumns("3,1")) == ["biosample\tBSS3\tBSS1", "BSS3\t9\t2", "BSS1\t2\t7"]
    assert concordance.table_lines(AGREE, None, parseColumns("2-3")) == ["biosample\t2\t3", "2\t5\t0", "3\t0\t9"]
    a, b = concordance.write_tables(tmp_path / "out", AGREE, BOTH, names, parseColumns("3,1-2"))
    assert a.name.endswith(".agree.tsv") and b.name.endswith(".both.tsv")
    assert a.read_text() == "biosample\tBSS3\tBSS1\tBSS2\nBSS3\t9\t2\t0\nBSS1\t2\t7\t1\nBSS2\t0\t1\t5\n"
    assert b.read_text() == "biosample\tBSS3\tBSS1\tBSS2\nBSS3\t9\t6\t5\nBSS1\t6\t7\t4\nBSS2\t5\t4\t5\n"
    with pytest.raises(click.UsageError):
        concordance.check_columns(parseColumns("1,4"), 3)
    concordance.check_columns(parseColumns("1,3"), 3)
    concordance.check_columns(None, 3)


def test_duplicate_warning():
    S = 4
    x = np.array([[0, 1, 2, 3], [1, 1, 0, 3], [2, 0, 2, 0], [3, 3, 3, 1]], dtype=np.uint8)            # no two columns equal
    assert concordance.duplicate_warning(*restatement(x, S)) is None
    one = x.copy()
    one[:, 2] = one[:, 0]
    a, b = restatement(one, S)
    assert concordance.duplicate_pairs(a, b) == [(0, 2)]
    assert concordance.duplicate_warning(a, b, ["A", "B", "C", "D"]) == \
        ("WARNING: 1 pair(s) of biosamples hold a state in the same bins and the same state in every one of them; the first is A (column 1) "
         "and C (column 3)")
    three = x.copy()
    three[:, 1] = three[:, 3]
    three[:, 2] = three[:, 3]
    a, b = restatement(three, S)
    assert concordance.duplicate_pairs(a, b) == [(1, 2), (1, 3), (2, 3)]
    assert concordance.duplicate_warning(a, b).startswith("WARNING: 3 pair(s) ") and concordance.duplicate_warning(a, b).endswith("2 (column 2) and 3 (column 3)")
    # the same states where both hold one, but not in the same bins: no duplicate; two columns without any state: none either
    holes = one.copy()
    holes[1, 2] = 0xFF
    assert concordance.duplicate_warning(*restatement(holes, S)) is None
    empty = x.copy()
    empty[:, 1] = 0xFF
    empty[:, 3] = 200
    a, b = restatement(empty, S)
    assert a[1, 3] == b[1, 1] == b[3, 3] == 0 and concordance.duplicate_warning(a, b) is None


# ---- the command lines -------------------------------------------------------------------------------------------------------

def test_command_lines_parse(tmp_path):
    from click.testing import CliRunner
    from epilogos_amd import preprocess
    out = CliRunner().invoke(concordance.main, ["--help"]).output
    for opt in ("-i", "-j", "-o", "--names", "--columns"):
        assert opt in out
    assert "--gpus" not in out
    assert CliRunner().invoke(concordance.main, ["-i", str(tmp_path)]).exit_code == 2                 # -j and -o are required
    assert "--concordance" in CliRunner().invoke(preprocess.main, ["--help"]).output


def test_command_needs_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    states = tmp_path / "states.tsv"
    states.write_text("zero_index\tone_index\n0\t1\n1\t2\n")
    with pytest.raises(_abi.EpilogosHipError):
        concordance.run([tmp_path], states, tmp_path / "p")


class _NumpyEngine:
    """engine.concordance on host tensors: the restatement, added to what is given."""

    def __init__(self):
        self.calls = []

    def __call__(self, X, N, S, agree=None, both=None):
        import torch
        a, b = restatement(X[:, :N].numpy(), S)
        self.calls.append((X.shape[0], N, S))
        a, b = torch.from_numpy(a), torch.from_numpy(b)
        return (a if agree is None else agree + a), (b if both is None else both + b)


def test_files_of_different_widths_are_a_usage_error(monkeypatch):
    import torch
    from epilogos_amd import engine
    monkeypatch.setattr(engine, "concordance", _NumpyEngine())
    t = concordance.Tally()
    t.add(torch.zeros((5, 16), dtype=torch.int8), 7, 3, "in/matrix_chr1.epgm")
    with pytest.raises(click.UsageError) as e:
        t.add(torch.zeros((5, 16), dtype=torch.int8), 6, 3, "in/matrix_chr2.epgm")
    assert "in/matrix_chr1.epgm" in e.value.message and "in/matrix_chr2.epgm" in e.value.message and "7" in e.value.message and "6" in e.value.message


def test_prep_progress_lines_are_unchanged_and_the_option_writes_the_tables(tmp_path, monkeypatch):
    """epilogos-prep on the golden state-by-line calls with the device stood in for: build_matrix_device is the numpy builder and
    engine.concordance the restatement.  Without the option the progress lines and the .epgm bytes are what they were; with it
    they are the same, and the two tables are the restatement of the matrix under the metadata names."""
    import torch
    from epilogos_amd import engine, preprocess, stateByLine as sbl
    d = tmp_path / "calls"
    d.mkdir()
    for k, n in enumerate(GOLD["names"]):
        (d / str(n)).write_bytes(GOLD["text_%d" % k].tobytes())
    (tmp_path / "meta.txt").write_bytes(GOLD["metadata"].tobytes())
    (tmp_path / "sizes.txt").write_bytes(GOLD["chromsizes"].tobytes())
    x, chrom = numpy_matrix([GOLD["text_%d" % k] for k in range(len(GOLD["names"]))])
    rng = (int(x.min()) + 1, int(x.max()) + 1)

    def build(files):
        assert [f.name for f in files] == [str(n) for n in GOLD["names"]]
        X = np.full((x.shape[0], engine.padded_width(x.shape[1])), -1, dtype=np.int8)
        X[:, :x.shape[1]] = x
        return torch.from_numpy(X), x.shape[1], chrom, rng
    fake = _NumpyEngine()
    monkeypatch.setattr(engine, "require_gpu", lambda: None)
    monkeypatch.setattr(sbl, "build_matrix_device", build)
    monkeypatch.setattr(engine, "concordance", fake)
    plain, with_option = io.StringIO(), io.StringIO()
    w0 = preprocess.run(d, tmp_path / "meta.txt", tmp_path / "sizes.txt", tmp_path / "plain", out=plain)
    assert not fake.calls
    w1 = preprocess.run(d, tmp_path / "meta.txt", tmp_path / "sizes.txt", tmp_path / "opt", out=with_option, concordance=tmp_path / "pairs")
    assert plain.getvalue() == "Processing chr1: %d files found. Done.\n" % len(GOLD["names"])
    assert with_option.getvalue() == plain.getvalue()
    assert [p.name for p in w0] == [p.name for p in w1] == ["matrix_chr1.epgm"] and w0[0].read_bytes() == w1[0].read_bytes()
    assert fake.calls == [(x.shape[0], x.shape[1], rng[1])]
    from epilogos_amd import census
    names = census.read_names(tmp_path / "meta.txt")
    a, b = restatement(x, rng[1])
    assert (tmp_path / "pairs.agree.tsv").read_text() == "\n".join(concordance.table_lines(a, names)) + "\n"
    assert (tmp_path / "pairs.both.tsv").read_text() == "\n".join(concordance.table_lines(b, names)) + "\n"
    assert (tmp_path / "pairs.agree.tsv").read_text().splitlines()[0].split("\t")[1:] == names[:x.shape[1]]
