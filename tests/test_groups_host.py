"""Column groups, the host side (no GPU; tests/test_abi_symbols.py holds include/epilogos_groups.h against its binding): the entry
point's argument checks (made before the first HIP call), and the membership bytes the engine builds for the kernel."""
import ctypes
import re

import numpy as np
import pytest

from epilogos_amd import _abi, engine


def test_the_headers_group_limit_is_the_engines():
    assert re.search(r"#define EPG_GROUPS_MAX %d\b" % engine.GROUPS_MAX, _abi.HEADERS["groups"].path.read_text())


def test_argument_validation_without_gpu():
    lib = _abi.load()
    assert lib.epg_version() == 2
    x = ctypes.c_void_p(4096)
    harr = (ctypes.c_void_p * 4)(4096, 8192, 12288, 16384)
    ok = dict(X=x, R=10, N=20, ldx=32, S=18, G=2, member=x, H=harr, counts=x)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.epg_bin_hist_groups(a["X"], a["R"], a["N"], a["ldx"], a["S"], a["G"], a["member"], a["H"], a["counts"], None)
    # EPG_ERR_UNSUPPORTED: what the kernel does not serve
    assert call(S=32) == -2 and b"S=32" in lib.epg_last_error()
    assert call(G=5) == -2 and b"G=5" in lib.epg_last_error()
    assert call(N=65536, ldx=65536) == -2 and b"65535" in lib.epg_last_error()
    # EPG_ERR_INVALID_ARG
    assert call(G=0) == -1 and b"bad shape" in lib.epg_last_error()
    assert call(G=-1) == -1
    assert call(N=0) == -1
    assert call(S=0) == -1
    assert call(R=-1) == -1
    assert call(ldx=19) == -1
    assert call(X=None) == -1 and b"NULL" in lib.epg_last_error()
    assert call(member=None) == -1 and b"NULL" in lib.epg_last_error()
    assert call(H=None, counts=None) == -1 and b"both NULL" in lib.epg_last_error()
    assert call(H=(ctypes.c_void_p * 4)(None, None, None, None), counts=None) == -1
    assert call(H=(ctypes.c_void_p * 4)(4096, 8200, 0, 0)) == -1 and b"aligned" in lib.epg_last_error()
    # the unsupported shapes are named before a NULL pointer is
    assert call(S=40, X=None) == -2
    # no rows: valid, nothing to do, no HIP call
    assert call(R=0) == 0
    assert call(R=0, H=None) == 0
    assert call(R=0, counts=None, H=(ctypes.c_void_p * 4)(None, 4096, None, None)) == 0


def test_membership_bytes(monkeypatch):
    import torch
    engine._members.clear()
    m = engine.group_members("cpu", 10, [np.array([0, 2, 9]), np.array([2, 3]), np.array([], dtype=np.int64)])
    assert m.dtype == torch.uint8 and m.tolist() == [1, 0, 3, 2, 0, 0, 0, 0, 0, 1]
    assert engine.group_members("cpu", 10, [[0, 2, 9], [2, 3], []]) is m                    # cached per (device, N, groups)
    assert engine.group_members("cpu", 11, [[0, 2, 9], [2, 3], []]) is not m
    assert engine.group_members("cpu", 10, [[0, 9, 2], [2, 3], []]) is not m                # (the order is part of the key)
    for bad in ([[-1]], [[10]], [[1, 1]]):
        with pytest.raises(ValueError):
            engine.group_members("cpu", 10, bad)
    engine._members.clear()


def test_select_columns_layout():
    import torch
    X = torch.arange(3 * 32, dtype=torch.int8).reshape(3, 32)
    Y = engine.select_columns(X, np.array([5, 0, 17]))
    assert Y.shape == (3, 16) and Y.dtype == torch.int8
    assert Y[:, :3].tolist() == [[5, 0, 17], [37, 32, 49], [69, 64, 81]]
    assert bool((Y[:, 3:] == -1).all())                                                     # padding bytes 0xFF
    assert engine.select_columns(X, np.arange(17)).shape == (3, 32)
    with pytest.raises(ValueError):
        engine.select_columns(X, np.array([1, 1]))


# ---- the SPEC parser ---------------------------------------------------------------------------------------------------------

def test_spec_numbers_and_ranges(tmp_path):
    from epilogos_amd.run import parseColumns
    assert parseColumns("1").tolist() == [0]
    assert parseColumns("1-3,7,9-10").tolist() == [0, 1, 2, 6, 8, 9]
    assert parseColumns(" 5 , 2 - 3 ").tolist() == [4, 1, 2]                                  # the order given is kept
    assert parseColumns("4-4").tolist() == [3]
    got = parseColumns("1-379,401,500-620")
    assert got.dtype == np.int64 and got.size == 379 + 1 + 121 and got[379] == 400 and got[-1] == 619
    f = tmp_path / "group.txt"
    f.write_text("# female biosamples\n1-3\n\n  7   # one more\n9-10\n#12\n")
    assert parseColumns("@" + str(f)).tolist() == [0, 1, 2, 6, 8, 9]


@pytest.mark.parametrize("spec,word", [("", "empty"), ("   ", "empty"), ("1,,2", "malformed"), ("1,", "malformed"), ("a", "malformed"),
                                       ("1-2-3", "malformed"), ("-3", "malformed"), ("1.5", "malformed"), ("3-1", "descends"),
                                       ("0", "start at 1"), ("0-4", "start at 1"), ("1,2,1", "listed twice"), ("1-5,3", "listed twice")])
def test_spec_errors(spec, word):
    from epilogos_amd.run import parseColumns
    with pytest.raises(ValueError, match=word):
        parseColumns(spec)


def test_spec_file_errors(tmp_path):
    from epilogos_amd.run import parseColumns
    with pytest.raises(ValueError, match="cannot read"):
        parseColumns("@" + str(tmp_path / "missing.txt"))
    (tmp_path / "empty.txt").write_text("# nothing\n\n")
    with pytest.raises(ValueError, match="empty"):
        parseColumns("@" + str(tmp_path / "empty.txt"))
    (tmp_path / "bad.txt").write_text("1-3\n4,5\n")                                          # one number or range per line
    with pytest.raises(ValueError, match="malformed"):
        parseColumns("@" + str(tmp_path / "bad.txt"))
    (tmp_path / "dup.txt").write_text("1-3\n2\n")
    with pytest.raises(ValueError, match="biosample 2 is listed twice"):
        parseColumns("@" + str(tmp_path / "dup.txt"))


# ---- run.py's flag combinations ----------------------------------------------------------------------------------------------

def _invoke(args):
    from click.testing import CliRunner
    from epilogos_amd import run
    res = CliRunner().invoke(run.main, args)
    return res.output


def test_todays_messages_for_todays_combinations():
    assert _invoke(["-o", "o", "-j", "j"]) == "ERROR: [-i, --input-directory] is required in single mode\n"
    assert _invoke(["-i", "x", "-a", "y", "-o", "o", "-j", "j"]) == "ERROR: [-a] and [-b] are only valid in paired mode\n"
    assert _invoke(["-m", "paired", "-a", "y", "-o", "o", "-j", "j"]) == \
        "ERROR: [-a, --directory-one] and [-b, --directory-two] are required in paired mode\n"
    assert _invoke(["-m", "paired", "-o", "o", "-j", "j"]) == \
        "ERROR: [-a, --directory-one] and [-b, --directory-two] are required in paired mode\n"
    assert _invoke(["-m", "paired", "-i", "x", "-a", "y", "-b", "z", "-o", "o", "-j", "j"]) == "ERROR: [-i] is only valid in single mode\n"
    assert _invoke(["-m", "paired", "-i", "x", "-o", "o", "-j", "j"]) == \
        "ERROR: [-a, --directory-one] and [-b, --directory-two] are required in paired mode\n"
    assert _invoke(["-i", "x", "-j", "j"]) == "ERROR: [-o, --output-directory] is required\n"
    assert _invoke(["-i", "x", "-o", "o"]) == "ERROR: [-j, --state-info] is required\n"


def test_column_flag_combinations():
    tail = ["-o", "o", "-j", "j"]
    assert "only valid in paired mode" in _invoke(["-i", "x", "--columns-a", "1"] + tail)
    assert "only valid in paired mode" in _invoke(["-i", "x", "--columns-b", "1", "--columns", "2"] + tail)
    assert "[--columns] is only valid in single mode" in _invoke(["-m", "paired", "-a", "y", "-b", "z", "--columns", "1"] + tail)
    assert "must be given together" in _invoke(["-m", "paired", "-i", "x", "--columns-a", "1"] + tail)
    assert "must be given together" in _invoke(["-m", "paired", "-i", "x", "--columns-b", "1"] + tail)
    assert "cannot be combined with [-a] and [-b]" in _invoke(["-m", "paired", "-a", "y", "-b", "z", "--columns-a", "1", "--columns-b", "2"] + tail)
    assert "cannot be combined with [-a] and [-b]" in _invoke(["-m", "paired", "-i", "x", "-a", "y", "--columns-a", "1", "--columns-b", "2"] + tail)
    assert "[-i, --input-directory] is required with" in _invoke(["-m", "paired", "--columns-a", "1", "--columns-b", "2"] + tail)
    # the SPEC's own errors, with the option named
    assert _invoke(["-i", "x", "--columns", ""] + tail) == "ERROR: [--columns] empty biosample list\n"
    assert _invoke(["-i", "x", "--columns", "1,x"] + tail).startswith("ERROR: [--columns] malformed")
    assert _invoke(["-i", "x", "--columns", "0"] + tail).startswith("ERROR: [--columns] biosample numbers start at 1")
    assert _invoke(["-i", "x", "--columns", "2,2"] + tail) == "ERROR: [--columns] biosample 2 is listed twice\n"
    assert _invoke(["-m", "paired", "-i", "x", "--columns-a", "1-3", "--columns-b", "5,5"] + tail) == \
        "ERROR: [--columns-b] biosample 5 is listed twice\n"
    assert _invoke(["-m", "paired", "-i", "x", "--columns-a", "1-3", "--columns-b", "3-6"] + tail) == \
        "ERROR: biosample 3 is in both [--columns-a] and [--columns-b]\n"
    for out in (_invoke(["-i", "x", "--columns", "1"]), _invoke(["-m", "paired", "-i", "x", "--columns-a", "1", "--columns-b", "2"])):
        assert out == "ERROR: [-o, --output-directory] is required\n"           # a good SPEC: on to today's checks


def test_biosample_above_a_files_column_count_names_the_file(tmp_path):
    from tests.test_host_logic import write_tsv
    ind = tmp_path / "in"
    ind.mkdir()
    rng = np.random.default_rng(0)
    write_tsv(ind / "matrix_chr1.txt.gz", rng.integers(0, 3, size=(5, 8)))
    write_tsv(ind / "matrix_chr2.txt.gz", rng.integers(0, 3, size=(5, 6)))
    meta = tmp_path / "metadata.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\ts%d\n" % (i, i + 1, i) for i in range(3)))
    tail = ["-i", str(ind), "-o", str(tmp_path / "o"), "-j", str(meta)]
    out = _invoke(["--columns", "1-7"] + tail)
    assert out.startswith("ERROR: biosample 7 is not in ") and "matrix_chr2.txt.gz" in out and "6 biosample columns" in out
    out = _invoke(["-m", "paired", "--columns-a", "1-3", "--columns-b", "4-9"] + tail)
    assert out.startswith("ERROR: biosample 9 is not in ") and "matrix_chr1.txt.gz" in out and "8 biosample columns" in out
