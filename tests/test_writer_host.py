"""`epilogos --writer [host|gpu]`, the host side (no GPU): tests/bgzf_ref.walk proven on the HOST writer's BGZF and on damaged copies
of it; driver.write_bgzf, the one helper that completes a device-written file; the option on the command line and its way down to
the drivers and STEP 3 (nothing is added for `host`); csrc/epg_textout.h against its binding table, type for type, and the library's
exports; the two stand-alone programs that hold the device's "%.5f" arithmetic against fmt_f5 and run the compressor's phases on
the host, built with the address and undefined-behaviour sanitizers."""
import ctypes
import gzip
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from epilogos_amd import _abi, _io, backend, build, driver
from tests import bgzf_ref
from tests.abi_headers import ctypes_of
from tests.groupings_backend import GroupingsBackend
from tests.host_programs import build_program as _build_program

NAMES = ["epgw_bgzf_bytes_max", "epgw_bgzf_compress", "epgw_bgzf_ws_bytes", "epgw_format_scores", "epgw_format_ws_bytes", "epgw_text_bytes_max"]
ROOT = build.ROOT


def _locations(R, chrom="chr1"):
    rows = [("%s\t%d\t%d\n" % (chrom, 99400 + 200 * r, 99600 + 200 * r)).encode() for r in range(R)]
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    return _io.Locations(np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), off)


def _host_bgzf(tmp_path, monkeypatch, R, name="host.txt.gz", seed=3):
    """-> (the file's bytes, its text): R rows x 18 scores through the host writer with EPILOGOS_BGZF=1."""
    monkeypatch.setenv("EPILOGOS_BGZF", "1")
    x = np.random.default_rng(seed).normal(0, 0.3, size=(R, 18)).astype(np.float32)
    _io.write_scores(tmp_path / name, _locations(R), x)
    blob = (tmp_path / name).read_bytes()
    return blob, gzip.decompress(blob)


# ---- (a) the walker ------------------------------------------------------------------------------------------------------------------
def test_the_walker_accepts_the_host_writer_s_file(tmp_path, monkeypatch):
    blob, text = _host_bgzf(tmp_path, monkeypatch, 3000)
    ms = bgzf_ref.walk(blob)
    assert len(ms) == -(-len(text) // 65280) + 1 and sum(m.bsize for m in ms) == len(blob) and ms[-1].isize == 0
    at = 0
    for m in ms:                                                               # the fields it returns are the members' own
        piece = zlib.decompressobj(-15).decompress(m.payload)
        assert len(piece) == m.isize and zlib.crc32(piece) == m.crc and piece == text[at:at + m.isize]
        at += m.isize
    assert at == len(text)
    empty, _ = _host_bgzf(tmp_path, monkeypatch, 0, "empty.txt.gz")
    assert empty == bgzf_ref.EOF and len(bgzf_ref.walk(empty)) == 1


def test_the_walker_refuses_damaged_copies(tmp_path, monkeypatch):
    blob, _text = _host_bgzf(tmp_path, monkeypatch, 3000)
    first = struct.unpack_from("<H", blob, 16)[0]
    for wrong in (first - 1, first + 1, 5, 0xFFFF):
        bad = blob[:16] + struct.pack("<H", wrong) + blob[18:]
        with pytest.raises(bgzf_ref.BgzfError):
            bgzf_ref.walk(bad)
    with pytest.raises(bgzf_ref.BgzfError, match="missing"):
        bgzf_ref.walk(blob[:-28])
    with pytest.raises(bgzf_ref.BgzfError, match="empty members"):
        bgzf_ref.walk(blob + bgzf_ref.EOF)
    with pytest.raises(bgzf_ref.BgzfError, match="empty members"):
        bgzf_ref.walk(bgzf_ref.EOF + blob)
    with pytest.raises(bgzf_ref.BgzfError):
        bgzf_ref.walk(blob + b"\0")
    with pytest.raises(bgzf_ref.BgzfError):
        bgzf_ref.walk(blob[:12] + b"XY" + blob[14:])
    with pytest.raises(bgzf_ref.BgzfError, match="concatenated"):
        bgzf_ref.walk(blob, eof=False)
    assert len(bgzf_ref.walk(blob[:-28], eof=False)) == len(bgzf_ref.walk(blob)) - 1
    plain = gzip.compress(b"no BC subfield")
    with pytest.raises(bgzf_ref.BgzfError):
        bgzf_ref.walk(plain)


# ---- (b) the assembly helper ---------------------------------------------------------------------------------------------------------
def test_parts_without_end_blocks_give_one_file_with_exactly_one(tmp_path, monkeypatch):
    assert driver.BGZF_EOF == bgzf_ref.EOF
    a, ta = _host_bgzf(tmp_path, monkeypatch, 700, "a.gz", seed=1)
    b, tb = _host_bgzf(tmp_path, monkeypatch, 300, "b.gz", seed=2)
    a, b = a[:-28], b[:-28]                                                     # what the device hands over: no end-of-file block
    driver.write_bgzf(tmp_path / "whole.gz", [np.frombuffer(a, dtype=np.uint8)])
    got = (tmp_path / "whole.gz").read_bytes()
    assert got == a + bgzf_ref.EOF and gzip.decompress(got) == ta and bgzf_ref.walk(got)
    # several ranks: part files carry no end-of-file block, the assembled file exactly one
    kind, tag = "scores", "t_s1"
    parts = [tmp_path / driver._part_name(kind, tag, 0, lo) for lo in (0, 700)]
    driver.write_bgzf(parts[0], [a], eof=False)
    driver.write_bgzf(parts[1], [memoryview(b)], eof=False)
    assert parts[0].read_bytes() == a and bgzf_ref.walk(parts[1].read_bytes(), eof=False)
    driver._assemble_text(tmp_path, kind, "final.txt.gz", tag, 0, [(0, 700), (700, 1000)], 1000, "gpu")
    got = (tmp_path / "final.txt.gz").read_bytes()
    assert got == a + b + bgzf_ref.EOF and got.count(bgzf_ref.EOF) == 1 and gzip.decompress(got) == ta + tb
    assert len(bgzf_ref.walk(got)) == len(bgzf_ref.walk(a, eof=False)) + len(bgzf_ref.walk(b, eof=False)) + 1
    assert not parts[0].exists() and not parts[1].exists()
    # one owner of the whole file: it was written under its final name, with its block, and is left alone
    driver._assemble_text(tmp_path, kind, "whole.gz", tag, 0, [(0, 700)], 700, "gpu")
    assert (tmp_path / "whole.gz").read_bytes() == a + bgzf_ref.EOF


def test_an_empty_file_is_the_end_block_alone(tmp_path):
    driver.write_bgzf(tmp_path / "none.gz", [])
    driver.write_bgzf(tmp_path / "zero.gz", [np.zeros(0, dtype=np.uint8)])
    for name in ("none.gz", "zero.gz"):
        got = (tmp_path / name).read_bytes()
        assert got == bgzf_ref.EOF and len(got) == 28 and gzip.decompress(got) == b"" and len(bgzf_ref.walk(got)) == 1


# ---- (c) the command line ------------------------------------------------------------------------------------------------------------
def _invoke(args):
    from click.testing import CliRunner

    from epilogos_amd import run
    return CliRunner().invoke(run.main, args)


def test_the_option_and_its_usage_error(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    log = tmp_path.parent / (tmp_path.name + "_io.log")
    monkeypatch.setenv("EPILOGOS_IO_LOG", str(log))
    from click.testing import CliRunner

    from epilogos_amd import run
    out = " ".join(CliRunner().invoke(run.main, ["-h"], terminal_width=200).output.split())
    assert "--writer [host|gpu]" in out and "BGZF" in out
    res = _invoke(["-i", "x", "-o", "o", "-j", "j", "--writer", "cpu"])
    assert res.exit_code == 2 and "--writer" in res.output
    assert not list(tmp_path.iterdir()) and not log.exists()                    # before any file is read or any directory made
    for args in (["-i", "x"], ["-m", "paired", "-a", "x", "-b", "y", "-n"], ["-i", "x", "-s", "3", "--cache-dir", "c"]):
        for w in ("host", "gpu"):
            res = _invoke(args + ["-o", "o", "-j", "j", "--writer", w])
            assert res.exit_code != 2 and "--writer" not in res.output, res.output


@pytest.fixture()
def be():
    b = GroupingsBackend()
    backend.set_for_testing(b)
    yield b
    backend.set_for_testing(None)
    driver.finish_writes()


class _Stop(Exception):
    pass


def _matrix_dir(tmp_path, S=5, N=6):
    from epilogos_amd import stateByLine as sbl
    d = tmp_path / "roadmap"
    d.mkdir()
    rng = np.random.default_rng(5)
    for c, R in (("chr1", 41), ("chr2", 17)):
        x = rng.integers(0, S, size=(R, N)).astype(np.int8)
        sbl.write_epgm(d / ("matrix_%s.epgm" % c), x, c, (1, S))
    states = tmp_path / "states.tsv"
    states.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(S)))
    return d, states


@pytest.mark.parametrize("mode", ["single", "paired", "groupings"])
def test_writer_host_adds_nothing_to_the_calls(tmp_path, be, monkeypatch, mode):
    """Default and --writer host: the drivers get the keyword arguments they always got and STEP 3 asks a part for its outputs with
    (session, part) alone; --writer gpu adds writer="gpu" to the driver call and nothing else."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    d, states = _matrix_dir(tmp_path)
    entry = {"single": "run_single_group", "paired": "run_paired_columns", "groupings": "run_groupings"}[mode]
    args = {"single": [], "paired": ["-m", "paired", "--columns-a", "1-3", "--columns-b", "4-6", "--null-seed", "7"], "groupings": []}[mode]
    if mode == "groupings":
        g = tmp_path / "g.tsv"
        g.write_text("left\t1-3\nright\t4-6\n")
        args = ["--groupings", str(g)]
    args = ["-i", str(d), "-j", str(states), "-w", "3"] + args
    seen, part_calls = [], []
    real = getattr(driver, entry)
    monkeypatch.setattr(driver, entry, lambda *a, **k: seen.append(sorted(k)) or real(*a, **k))
    for cls in (driver._Single, driver._Paired):
        orig = cls.part_out
        monkeypatch.setattr(cls, "part_out", (lambda orig: lambda self, *a, **k: part_calls.append((len(a), tuple(sorted(k)))) or orig(self, *a, **k))(orig))
    for k, extra in enumerate(([], ["--writer", "host"])):
        res = _invoke(args + ["-o", str(tmp_path / ("o%d" % k))] + extra)
        assert res.exit_code == 0 and "ERROR" not in res.output, res.output
    assert len(seen) == 2 and seen[0] == seen[1] and "writer" not in seen[0]
    assert part_calls and set(part_calls) == {(2, ())}
    for sub in ([""] if mode != "groupings" else ["left", "right"]):            # the same files and bytes
        a, b = tmp_path / "o0" / sub, tmp_path / "o1" / sub
        assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir())
        assert all((b / p.name).read_bytes() == p.read_bytes() for p in a.iterdir() if p.is_file())

    def stop(*a, **k):
        seen.append(sorted(k))
        raise _Stop()
    monkeypatch.setattr(driver, entry, stop)
    res = _invoke(args + ["-o", str(tmp_path / "o2"), "--writer", "gpu"])
    assert isinstance(res.exception, _Stop) and seen[2] == sorted(seen[0] + ["writer"])


def test_the_drivers_refuse_an_unknown_writer(tmp_path, be):
    d, _states = _matrix_dir(tmp_path)
    with pytest.raises(ValueError, match="writer"):
        driver.run_single_group(sorted(d.iterdir()), 5, 1, tmp_path, "t", writer="cpu")


def test_step3_writes_what_the_session_hands_over_and_falls_back_with_one_warning(tmp_path, be, monkeypatch, capsys):
    """--writer gpu over a session stood in for on the host: scores(pid, text=) hands out the host writer's BGZF of the part without
    its end-of-file block, and None for chr2, which the "device" refuses."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    d, _states = _matrix_dir(tmp_path)
    files = sorted(d.iterdir())
    (tmp_path / "host").mkdir()
    (tmp_path / "gpu").mkdir()
    driver.run_single_group(files, 5, 1, tmp_path / "host", "t", keep_temp_scores=False)
    sess_cls = type(be.open_single(5, 1))
    _plain = sess_cls.scores
    released = []

    def scores(self, pid, text=None):
        sc = _plain(self, pid)
        if text is None:
            return sc
        if sc.shape[0] == 17:                                                  # chr2: the device "refuses" it
            return sc, None
        monkeypatch.setenv("EPILOGOS_BGZF", "1")
        _io.write_scores(tmp_path / "tmp.gz", text, sc)
        monkeypatch.delenv("EPILOGOS_BGZF")
        return sc, np.frombuffer((tmp_path / "tmp.gz").read_bytes()[:-28], dtype=np.uint8)
    monkeypatch.setattr(sess_cls, "scores", scores)
    monkeypatch.setattr(sess_cls, "release_text", lambda self: released.append(1), raising=False)
    capsys.readouterr()
    driver.run_single_group(files, 5, 1, tmp_path / "gpu", "t", keep_temp_scores=False, writer="gpu")
    out = capsys.readouterr().out
    warnings = [l for l in out.splitlines() if "WARNING:" in l]
    assert len(warnings) == 1 and "scores_t_matrix_chr2.txt.gz" in warnings[0] and "host writer" in warnings[0] and released == [1]
    names = sorted(p.name for p in (tmp_path / "host").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "gpu").iterdir())
    for n in names:
        a, b = (tmp_path / "host" / n).read_bytes(), (tmp_path / "gpu" / n).read_bytes()
        assert (gzip.decompress(a) == gzip.decompress(b)) if n.endswith(".gz") else a == b, n
    assert bgzf_ref.walk((tmp_path / "gpu" / "scores_t_matrix_chr1.txt.gz").read_bytes())
    with pytest.raises(bgzf_ref.BgzfError):                                     # the refused file is the host writer's plain gzip
        bgzf_ref.walk((tmp_path / "gpu" / "scores_t_matrix_chr2.txt.gz").read_bytes())


# ---- (d) the header and its binding --------------------------------------------------------------------------------------------------
def header_prototypes(path):
    """name -> (return type, [parameter declarations]) of every epgw_ prototype of a header (the parser of tests/abi_headers.py, on a
    path and for this prefix)."""
    txt = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    txt = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", txt, flags=re.M)
    protos = {}
    for stmt in txt.split(";"):
        m = re.match(r"\s*(.*?)\b(epgw_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            args = " ".join(m.group(3).split())
            protos[m.group(2)] = (" ".join(m.group(1).split()), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return protos


@pytest.fixture(scope="module")
def lib():
    if build.is_stale():
        if shutil.which("hipcc") is None:
            pytest.skip("hipcc not available and library not prebuilt")
        build.build_library()
    return _abi.load()


def test_the_writer_s_table_is_apart_from_the_public_registry():
    assert list(_abi.WRITER) == list(build.WRITER_HEADERS) == ["textout"] and "textout" in _abi._INTERNAL_TABLES
    assert "textout" not in _abi.HEADERS and "textout" not in build.PUBLIC_HEADERS
    header = _abi.WRITER["textout"]
    assert header.path == build.CSRC / "epg_textout.h" and header.path in build.HEADERS and "epg_textout.hip" in build.SOURCES
    assert not list((build.ROOT / "include").glob("*textout*"))
    for other in [*_abi.HEADERS.values(), *_abi.INTERNAL.values()]:
        assert not set(other.prototypes) & set(header.prototypes)
    text = header.path.read_text()
    assert "PACKAGE-INTERNAL" in text and "include/epilogos_textout.h" in text and "tests/test_abi_symbols.py" in text
    assert "synchronisation" in text                                            # the one between the two calls, the caller's


def test_header_and_binding_agree():
    header = _abi.WRITER["textout"]
    protos = header_prototypes(header.path)
    assert sorted(protos) == sorted(header.prototypes) == NAMES
    for name, (res, args) in header.prototypes.items():
        ret, params = protos[name]
        assert res is ctypes_of(ret, returned=True), name
        assert len(args) == len(params), name
        for i, (a, p) in enumerate(zip(args, params)):
            assert "float " not in p.replace("float*", "") and a is ctypes_of(p), "%s: parameter %d is `%s` in the header, %s in the binding" % (name, i, p, a.__name__)
    assert protos["epgw_format_scores"][1][-1] == "void* stream" and protos["epgw_bgzf_compress"][1][-1] == "void* stream"


def test_library_exports_every_name(lib):
    fresh = ctypes.CDLL(str(_abi.lib_path()))
    for name in NAMES:
        fn = getattr(lib, name)
        assert hasattr(fresh, name) and fn.argtypes == _abi.WRITER["textout"].prototypes[name][1]
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(_abi.lib_path())], capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(NAMES) <= exported


def test_argument_validation_and_size_queries_without_gpu(lib):
    p = ctypes.c_void_p(1 << 20)
    msg = lib.epg_last_error
    fmt, cmp_ = lib.epgw_format_scores, lib.epgw_bgzf_compress
    assert lib.epgw_text_bytes_max(10, 18, 200) == 200 + 10 * 18 * 18 and lib.epgw_text_bytes_max(-1, 18, 0) == -1 and lib.epgw_text_bytes_max(1, 0, 0) == -1
    assert lib.epgw_bgzf_bytes_max(0, 1) == 28 and lib.epgw_bgzf_bytes_max(0, 0) == 0 and lib.epgw_bgzf_bytes_max(65281, 1) == 65281 + 2 * 31 + 28
    assert lib.epgw_bgzf_bytes_max(-1, 0) == -1 and lib.epgw_bgzf_ws_bytes(1 << 40) == -1 and lib.epgw_format_ws_bytes(1 << 31) == -1
    assert lib.epgw_bgzf_ws_bytes(65281) % 256 == 0 and lib.epgw_bgzf_ws_bytes(65281) > lib.epgw_bgzf_ws_bytes(65280) > 0
    assert fmt(p, 5, 0, 18, p, p, p, 100, p, p, p, 1 << 30, None) == -1 and b"bad shape" in msg()
    assert fmt(p, 5, 18, 17, p, p, p, 100, p, p, p, 1 << 30, None) == -1 and b"bad shape" in msg()
    assert fmt(p, 1 << 31, 18, 18, p, p, p, 100, p, p, p, 1 << 30, None) == -2 and b"2^31" in msg()
    for k, name in ((0, "scores"), (4, "loc"), (5, "loc_off"), (6, "text"), (8, "row_off"), (9, "flags"), (10, "ws")):
        a = [p, 5, 18, 18, p, p, p, 100, p, p, p, 1 << 30]
        a[k] = None
        assert fmt(*a, None) == -1 and (name + " is NULL").encode() in msg(), name
    assert fmt(p, 5, 18, 18, p, p, ctypes.c_void_p((1 << 20) + 64), 100, p, p, p, 1 << 30, None) == -1 and b"aligned" in msg()
    assert fmt(p, 5, 18, 18, p, p, p, 100, p, p, p, 0, None) == -4
    assert cmp_(p, -1, None, 0, 1, p, 100, p, p, p, 1 << 30, None) == -1 and b"bad shape" in msg()
    assert cmp_(p, 1 << 40, None, 0, 1, p, 100, p, p, p, 1 << 30, None) == -2
    for k, name in ((0, "text"), (2, "row_off"), (5, "out"), (7, "n_out"), (8, "flags"), (9, "ws")):
        a = [p, 100, p, 3, 1, p, 1000, p, p, p, 1 << 30]
        a[k] = None
        assert cmp_(*a, None) == -1 and (name + " is NULL").encode() in msg(), name
    assert cmp_(p, 100, None, 0, 1, ctypes.c_void_p((1 << 20) + 8), 1000, p, p, p, 1 << 30, None) == -1 and b"aligned" in msg()
    assert cmp_(p, 100, None, 0, 1, p, 1000, p, p, p, 16, None) == -4


# ---- (e) the stand-alone programs ------------------------------------------------------------------------------------------------------


def test_the_format_arithmetic_is_fmt_f5_s_under_the_sanitizers(tmp_path):
    exe = _build_program(tmp_path, "fmt_f5_check", [ROOT / "tests" / "fmt_f5_check.cpp", build.IO_SOURCE], ["-lz"])
    res = subprocess.run([str(exe), "1000000"], capture_output=True, text=True)
    assert res.returncode == 0 and "1000000 patterns" in res.stdout and " 0 differ" in res.stdout, res.stdout + res.stderr


def test_the_compressor_s_phases_round_trip_on_the_host_under_the_sanitizers(tmp_path):
    exe = _build_program(tmp_path, "bgzf_block_check", [ROOT / "tests" / "bgzf_block_check.cpp"], ["-lz"])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "bgzf_block_check: ok" in res.stdout, res.stdout + res.stderr
