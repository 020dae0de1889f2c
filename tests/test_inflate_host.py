"""`simsearch --inflate [host|gpu]`, the host side (no GPU): the stand-alone program that runs the device inflater's phases on the host
under the address and undefined-behaviour sanitizers, on its own streams and on those of tests/bgzf_streams.py (what the GPU tests
use); bgzfIndex.members against tests/bgzf_ref.members; csrc/epg_bgzf_inflate.h against its binding table, type for type, and the
library's exports; the argument checks made before the first HIP call; the option's usage errors; nothing is added for `host`."""
import ctypes
import gzip
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from epilogos_amd import _abi, _io, bgzfIndex, build, scoresText
from epilogos_amd import similaritySearch_run as run
from epilogos_amd import similaritySearch_write as ssw
from tests import bgzf_ref
from tests import bgzf_streams as bs
from tests.abi_headers import ctypes_of
from tests.host_programs import build_program as _build_program

NAMES = ["epgz_bgzf_inflate", "epgz_inflate_lds_bytes", "epgz_newline_index", "epgz_newline_segments"]
ROOT = build.ROOT


# ---- (a) the stand-alone program -----------------------------------------------------------------------------------------------------


def test_the_inflater_s_phases_agree_with_zlib_on_the_host_under_the_sanitizers(tmp_path):
    exe = _build_program(tmp_path, "bgzf_inflate_check", [ROOT / "tests" / "bgzf_inflate_check.cpp"], ["-lz"])
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "bgzf_inflate_check: ok" in res.stdout and " 0 wrong" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    assert int(re.search(r"(\d+) of them mutations", res.stdout).group(1)) >= 10000
    # the streams the GPU tests run, made in Python: the good ones good, every bad one with its reason
    text = bs.score_text(600)[:65280]
    good, bad = bs.good_members(text), bs.bad_members(text)
    for name, (m, want) in good.items():
        assert zlib.decompressobj(-15).decompress(m.payload) == want and zlib.crc32(want) == m.crc, name
    assert {why for _m, why in bad.values()} >= set(range(2, 16)) | {bs.E_TRAILING}
    bs.write_members(tmp_path / "members.bin", [(m, 0) for m, _t in good.values()] + list(bad.values()))
    res = subprocess.run([str(exe), "--members", str(tmp_path / "members.bin")], capture_output=True, text=True)
    assert res.returncode == 0 and "bgzf_inflate_check: ok" in res.stdout and "%d members" % (len(good) + len(bad)) in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_the_reason_codes_are_named_in_the_abi_header():
    block = (build.CSRC / "epg_bgzf_inflate_block.h").read_text()
    enum = re.search(r"enum Reason \{(.*?)\};", block, flags=re.S).group(1)
    codes = dict((n, int(v)) for n, v in re.findall(r"\b(BI_E_[A-Z_]+) = (\d+)", enum))
    assert sorted(codes.values()) == list(range(1, 18))
    header = _abi.READER["bgzf_inflate"].path.read_text()
    for name, v in codes.items():
        assert re.search(r"\b%d %s\b" % (v, name), header), name
    assert sorted(scoresText.MEMBER_REASONS) == sorted(codes.values())
    assert [getattr(bs, n[3:]) for n in sorted(codes, key=codes.get)] == list(range(1, 18))


# ---- (b) the member table ------------------------------------------------------------------------------------------------------------
def _locations(R, chrom="chr1"):
    rows = [("%s\t%d\t%d\n" % (chrom, 99400 + 200 * r, 99600 + 200 * r)).encode() for r in range(R)]
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    return _io.Locations(np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), off)


def _host_bgzf(tmp_path, monkeypatch, R, name="host.txt.gz", seed=3):
    monkeypatch.setenv("EPILOGOS_BGZF", "1")
    x = np.random.default_rng(seed).normal(0, 0.3, size=(R, 18)).astype(np.float32)
    _io.write_scores(tmp_path / name, _locations(R), x)
    blob = (tmp_path / name).read_bytes()
    return blob, gzip.decompress(blob)


def _agrees(blob, tmp_path):
    """bgzfIndex.members of the bytes, and of a file of them, against the walker: the same members, or None where it raises."""
    (tmp_path / "probe.gz").write_bytes(blob)
    got = [bgzfIndex.members(blob), bgzfIndex.members(tmp_path / "probe.gz"), bgzfIndex.members(np.frombuffer(blob, dtype=np.uint8)),
           bgzfIndex.members(memoryview(blob))]
    try:
        ms = bgzf_ref.members(blob)
    except bgzf_ref.BgzfError:
        assert got == [None] * 4
        return None
    at, text = 0, 0
    for table, total in got:
        assert table.dtype == np.int64 and table.shape == (len(ms), 5) and total == sum(m.isize for m in ms)
    for row, m in zip(got[0][0], ms):
        assert list(row) == [at + 18, len(m.payload), text, m.isize, m.crc] and blob[row[0]:row[0] + row[1]] == m.payload
        at, text = at + m.bsize, text + m.isize
    assert all(np.array_equal(g[0], got[0][0]) for g in got)
    return got[0]


def test_members_against_the_walker(tmp_path, monkeypatch):
    blob, text = _host_bgzf(tmp_path, monkeypatch, 3000)
    table, total = _agrees(blob, tmp_path)
    assert total == len(text) and table[-1, 3] == 0 and len(table) == -(-len(text) // 65280) + 1
    own = ssw.bgzf_compress(text)[0]                                           # python's zlib in BGZF members
    assert _agrees(own, tmp_path)[1] == len(text)
    mid = blob[:-28]
    assert _agrees(mid + bgzf_ref.EOF + mid + bgzf_ref.EOF, tmp_path)[1] == 2 * len(text)       # an end-of-file block in the middle
    assert _agrees(mid, tmp_path)[1] == len(text)                              # and none at all
    assert _agrees(bgzf_ref.EOF, tmp_path)[1] == 0
    # the damaged copies of tests/test_writer_host.py
    first = struct.unpack_from("<H", blob, 16)[0]
    for wrong in (first - 1, first + 1, 5, 0xFFFF):
        assert _agrees(blob[:16] + struct.pack("<H", wrong) + blob[18:], tmp_path) is None
    assert _agrees(blob + b"\0", tmp_path) is None
    assert _agrees(blob[:12] + b"XY" + blob[14:], tmp_path) is None
    assert _agrees(blob[:-3], tmp_path) is None
    assert _agrees(gzip.compress(b"no BC subfield"), tmp_path) is None         # plain gzip
    assert _agrees(gzip.compress(text), tmp_path) is None
    (tmp_path / "raw.txt").write_bytes(text)
    assert bgzfIndex.members(tmp_path / "raw.txt") is None
    big = bs.wrap(bs.deflate(b"x" * 65281))                                    # ISIZE above BGZF's limit: the walker's rule, restated
    assert _agrees(big, tmp_path) is None


# ---- (c) the header and its binding --------------------------------------------------------------------------------------------------
def header_prototypes(path):
    txt = re.sub(r"/\*.*?\*/", "", path.read_text(), flags=re.S)
    txt = re.sub(r'^\s*(#.*|extern "C" \{|\})\s*$', "", txt, flags=re.M)
    protos = {}
    for stmt in txt.split(";"):
        m = re.match(r"\s*(.*?)\b(epgz_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
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


def test_the_reader_s_table_is_apart_from_the_other_registries():
    assert list(_abi.READER) == list(build.READER_HEADERS) == ["bgzf_inflate"] and "bgzf_inflate" in _abi._INTERNAL_TABLES
    assert list(_abi._INTERNAL_TABLES) == [*build.INTERNAL_HEADERS, *build.WRITER_HEADERS, *build.READER_HEADERS]
    for reg in (_abi.HEADERS, _abi.INTERNAL, _abi.WRITER, build.PUBLIC_HEADERS, build.INTERNAL_HEADERS, build.WRITER_HEADERS):
        assert "bgzf_inflate" not in reg
    header = _abi.READER["bgzf_inflate"]
    assert header.path == build.CSRC / "epg_bgzf_inflate.h" and header.path in build.HEADERS and "epg_bgzf_inflate.hip" in build.SOURCES
    assert build.CSRC / "epg_bgzf_inflate_block.h" in build.HEADERS
    assert not list((build.ROOT / "include").glob("*inflate*"))
    for other in [*_abi.HEADERS.values(), *_abi.INTERNAL.values(), *_abi.WRITER.values()]:
        assert not set(other.prototypes) & set(header.prototypes)
    text = header.path.read_text()
    assert "PACKAGE-INTERNAL" in text and "include/epilogos_bgzf_inflate.h" in text and "tests/test_abi_symbols.py" in text


def test_header_and_binding_agree():
    header = _abi.READER["bgzf_inflate"]
    protos = header_prototypes(header.path)
    assert sorted(protos) == sorted(header.prototypes) == NAMES
    for name, (res, args) in header.prototypes.items():
        ret, params = protos[name]
        assert res is ctypes_of(ret, returned=True), name
        assert len(args) == len(params), name
        for i, (a, p) in enumerate(zip(args, params)):
            assert a is ctypes_of(p), "%s: parameter %d is `%s` in the header, %s in the binding" % (name, i, p, a.__name__)
    assert protos["epgz_bgzf_inflate"][1][-1] == "void* stream" and protos["epgz_newline_index"][1][-1] == "void* stream"
    assert int(re.search(r"#define EPGZ_TABLE_COLS (\d+)", header.path.read_text()).group(1)) == bgzfIndex.COLS == 5


def test_library_exports_every_name(lib):
    fresh = ctypes.CDLL(str(_abi.lib_path()))
    for name in NAMES:
        fn = getattr(lib, name)
        assert hasattr(fresh, name) and fn.argtypes == _abi.READER["bgzf_inflate"].prototypes[name][1]
    nm = shutil.which("nm")
    if nm is not None:
        out = subprocess.run([nm, "-D", "--defined-only", str(_abi.lib_path())], capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        assert set(NAMES) <= exported


def test_argument_validation_and_its_order_without_gpu(lib):
    p = ctypes.c_void_p(1 << 20)
    msg = lib.epg_last_error
    inf, idx, seg = lib.epgz_bgzf_inflate, lib.epgz_newline_index, lib.epgz_newline_segments
    for a in ((p, -1, p, 1, p, 10, p, p), (p, 10, p, -1, p, 10, p, p), (p, 10, p, 1, p, -1, p, p), (None, -1, None, 1, None, 10, None, None)):
        assert inf(*a, None) == -1 and b"bad shape" in msg()                   # the sizes come before the pointers
    assert inf(None, 10, None, 1 << 31, None, 10, None, None, None) == -2 and b"2^31" in msg()
    assert inf(None, 1 << 40, None, 1, None, 10, None, None, None) == -2 and b"2^40" in msg()
    assert inf(p, 10, p, 1, p, 1 << 40, p, p, None) == -2
    for k, name in ((0, "comp"), (2, "table"), (4, "out"), (6, "status"), (7, "flags")):
        a = [p, 10, p, 1, p, 10, p, p]
        for j in range(k, 8):                                                  # the first NULL in the header's order is the one named
            if j in (0, 2, 4, 6, 7):
                a[j] = None
        assert inf(*a, None) == -1 and (name + " is NULL").encode() in msg(), name
    assert inf(p, 10, ctypes.c_void_p((1 << 20) + 4), 1, p, 10, p, p, None) == -1 and b"aligned" in msg()
    assert inf(p, 10, ctypes.c_void_p((1 << 20) + 4), 1, p, 10, p, None, None) == -1 and b"flags is NULL" in msg()      # pointers before alignment
    assert 65536 + 4096 < lib.epgz_inflate_lds_bytes() <= 80 * 1024             # the window, the ring and the tables: two workgroups in a CU's 160 KB
    assert seg(0, 16) == 0 and seg(1, 16) == 1 and seg(4097, 4096) == 2 and seg(1 << 20, 1 << 20) == 1
    for bad in ((-1, 16), (10, 0), (10, 8), (10, 24), (10, (1 << 30) + 16), (1 << 40, 16)):
        assert seg(*bad) == -1 and b"bad shape" in msg()
    assert idx(p, -1, 16, p, p, None) == -1 and b"bad shape" in msg()
    assert idx(None, 10, 24, None, None, None) == -1 and b"bad shape" in msg()
    assert idx(None, 1 << 40, 16, None, None, None) == -2 and b"2^40" in msg()
    for k, name in ((0, "text"), (3, "count"), (4, "last")):
        a = [p, 10, 16, p, p]
        for j in (0, 3, 4):
            if j >= k:
                a[j] = None
        assert idx(*a, None) == -1 and (name + " is NULL").encode() in msg(), name
    assert idx(ctypes.c_void_p((1 << 20) + 8), 10, 16, p, p, None) == -1 and b"aligned" in msg()
    assert idx(None, 0, 16, None, None, None) == 0                             # n = 0: nothing to do, no launch


# ---- (d) the command line ------------------------------------------------------------------------------------------------------------
def _usage(argv, capsys):
    with pytest.raises(SystemExit) as e:
        run.cli(argv)
    return e.value.code, capsys.readouterr().err


def test_the_option_and_its_usage_errors(tmp_path, monkeypatch, capsys):
    from click.testing import CliRunner
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "o"
    read = []
    monkeypatch.setattr(run, "windowParameters", lambda *a, **k: read.append(a) or (_ for _ in ()).throw(AssertionError("a file was read")))
    for argv in (["-b", "-s", "x.txt.gz", "-o", str(out), "--inflate", "cpu", "--step1", "gpu"],
                 ["-b", "-s", "x.txt.gz", "-o", str(out), "--inflate"],
                 ["-q", "chr1:1-2", "-m", "x.bed.gz", "-o", str(out), "--inflate", "gpu"],           # -q -m without -s
                 ["-q", "chr1:1-2", "-m", "x.bed.gz", "-o", str(out), "--inflate=host"],
                 ["-b", "-s", "x.txt.gz", "-o", str(out), "--inflate", "gpu"],                        # -b with the host's STEP 1
                 ["-b", "-s", "x.txt.gz", "-o", str(out), "--inflate", "gpu", "--step1", "host"]):
        code, err = _usage(argv, capsys)
        assert code == 2 and "--inflate" in err, (argv, err)
    assert not read and not out.exists() and not list(tmp_path.iterdir())      # before any file is read or any directory made
    # through click's runner: the values reach main through ctx.obj, as cli() hands them over
    res = CliRunner().invoke(run.main, ["-q", "chr1:1-2", "-m", "x.bed.gz", "-o", str(out)], obj={"inflate": "gpu"})
    assert res.exit_code == 2 and "--inflate" in res.output
    res = CliRunner().invoke(run.main, ["-b", "-s", "x.txt.gz", "-o", str(out)], obj={"inflate": "gpu", "step1": "host"})
    assert res.exit_code == 2 and "--inflate" in res.output and not out.exists()
    assert run.splitInflateOption(["-b", "--inflate", "gpu", "-s", "x", "--inflate=host"]) == ("host", ["-b", "-s", "x"])
    assert run.splitInflateOption(["-b", "--step1", "gpu"]) == (None, ["-b", "--step1", "gpu"])


class _Stop(Exception):
    pass


@pytest.mark.parametrize("mode", ["query", "build", "build2"])
def test_inflate_host_adds_nothing_to_the_calls(tmp_path, monkeypatch, mode):
    """Default and --inflate host: liveQuery, STEP 1's main and the STEP 1 child get the arguments they always got; --inflate gpu adds
    inflate="gpu" (the child: two words to its command line) and nothing else."""
    from epilogos_amd import similaritySearch_query as sq
    from epilogos_amd import similaritySearch_step1 as s1
    seen = []

    def stop(*a, **k):
        seen.append((len(a), dict(k)))
        raise _Stop()
    monkeypatch.setattr(run, "windowParameters", lambda sp, w: (25000, 125, 5))
    monkeypatch.setattr(run, "checkDevices", lambda gpus: None)
    monkeypatch.setattr(run, "resolveGpus", lambda v: int(v))
    monkeypatch.setattr(sq, "liveQuery", stop)
    monkeypatch.setattr(s1, "main", stop)
    monkeypatch.setattr(run, "runChildren", lambda jobs, **k: stop(*jobs[0][0]))
    args = {"query": ["-q", "chr1:1-2", "-s", "x.txt.gz"], "build": ["-b", "-s", "x.txt.gz", "--step1", "gpu"],
            "build2": ["-b", "-s", "x.txt.gz", "--step1", "gpu", "--gpus", "2"]}[mode] + ["-o", str(tmp_path / "o")]
    for extra in ([], ["--inflate", "host"], ["--inflate", "gpu"]):
        with pytest.raises(_Stop):
            run.cli(args + extra)
    assert len(seen) == 3 and seen[0] == seen[1] and "inflate" not in seen[0][1]
    if mode == "build2":                                                       # the child's command line: `--inflate gpu` behind the seven arguments
        assert seen[2][0] == seen[0][0] + 2
        argv = run.step1Job(tmp_path, "x.txt.gz", 125, 5, 25000, -1, -1.0, 1, inflate="gpu")[0]
        assert argv[-2:] == ["--inflate", "gpu"] and argv[:-2] == run.step1Job(tmp_path, "x.txt.gz", 125, 5, 25000, -1, -1.0, 1)[0]
    else:
        assert seen[2] == (seen[0][0], dict(seen[0][1], inflate="gpu"))
    # one level down: the readers call scoresText.read_scores_device as they always did
    calls = []
    monkeypatch.setattr(scoresText, "read_scores_device", lambda *a, **k: calls.append((len(a), dict(k))) or (_ for _ in ()).throw(_Stop()))
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    from epilogos_amd import engine
    monkeypatch.setattr(engine, "require_gpu", lambda: None)
    for fn, k in ((sq.readGrid, {}), (sq.readGrid, {"inflate": "host"}), (sq.readGrid, {"inflate": "gpu"}),
                  (s1.readDevice, {}), (s1.readDevice, {"inflate": "host"}), (s1.readDevice, {"inflate": "gpu"})):
        with pytest.raises(_Stop):
            fn("x.txt.gz", **k)
    assert calls[0] == calls[1] and calls[3] == calls[4] and "inflate" not in calls[0][1] and "inflate" not in calls[3][1]
    assert calls[2] == (calls[0][0], dict(calls[0][1], inflate="gpu")) and calls[5] == (calls[3][0], dict(calls[3][1], inflate="gpu"))


def test_the_chunk_cutter_without_the_text():
    """cut_chunks_indexed on a host-made index: chunks of whole rows that tile the text, with their row counts, for texts with and
    without a final newline and a row longer than the chunk."""
    rng = np.random.default_rng(4)
    rows = [bytes(rng.integers(97, 123, int(n)).astype(np.uint8)) for n in rng.integers(0, 90, 400)]
    rows[100] = b"y" * 3000
    for tail in (b"\n", b""):
        text = b"\n".join(rows) + tail
        a = np.frombuffer(text, dtype=np.uint8)
        for chunk, seg in ((256, 64), (1000, 16), (4096, 1024), (17, 16), (1 << 20, 4096)):
            nseg = -(-len(a) // seg)
            count = np.array([np.count_nonzero(a[s * seg:(s + 1) * seg] == 10) for s in range(nseg)], dtype=np.int64)
            last = np.array([max([s * seg + int(i) for i in np.flatnonzero(a[s * seg:(s + 1) * seg] == 10)] or [-1]) for s in range(nseg)], dtype=np.int64)
            chunks, nrows = scoresText.cut_chunks_indexed(len(a), chunk, seg, count, last)
            assert chunks[0][0] == 0 and chunks[-1][1] == len(a) and all(x[1] == y[0] for x, y in zip(chunks, chunks[1:]))
            assert sum(nrows) == len(rows)
            for k, ((lo, hi), r) in enumerate(zip(chunks, nrows)):
                virtual = 1 if (k == len(chunks) - 1 and not tail) else 0
                assert hi > lo and (a[hi - 1] == 10 or hi == len(a)) and r == int(np.count_nonzero(a[lo:hi] == 10)) + virtual
                assert hi - lo <= chunk or hi - lo <= 3001 + seg                # only the long row's chunk may be longer
    assert scoresText.cut_chunks_indexed(0, 100, 16, [], []) == ([], [])
