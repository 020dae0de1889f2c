"""GPU: `--inflate gpu` end to end.  scoresText.read_scores_device(inflate="gpu") against inflate="host" -- the parent's path -- on one
scores file (3 chromosomes x 2 000 rows x 5 states) written as BGZF by each of the three producers, with chunk sizes that make chunk
cuts and member borders interleave; the files it hands to the host (plain gzip: silently; a damaged member: one warning line); the
strict grammar's refusals; and the two commands, whose output files must not change by a byte."""
import gzip
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import _io, bgzfIndex, scoresText
from epilogos_amd import similaritySearch_write as ssw

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CHROMS = [("chr1", 2000), ("chr2", 2003), ("chrX", 1999)]
S = 5


def _table():
    rng = np.random.default_rng(21)
    R = sum(n for _c, n in CHROMS)
    x = np.where(rng.random((R, S)) < 0.3, 0.0, rng.normal(0, 0.8, (R, S))).astype(np.float32)
    rows = [("%s\t%d\t%d\n" % (c, 200 * r, 200 * (r + 1))).encode() for c, n in CHROMS for r in range(n)]
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return _io.Locations(np.frombuffer(b"".join(rows), dtype=np.uint8).copy(), off), x


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path of the same text as BGZF from the three producers, and the text."""
    from epilogos_amd import engine
    engine.require_gpu()
    d = tmp_path_factory.mktemp("inflate")
    loc, x = _table()
    old = os.environ.get("EPILOGOS_BGZF")
    os.environ["EPILOGOS_BGZF"] = "1"
    try:
        _io.write_scores(d / "host.txt.gz", loc, x)
    finally:
        if old is None:
            del os.environ["EPILOGOS_BGZF"]
        else:
            os.environ["EPILOGOS_BGZF"] = old
    text = gzip.decompress((d / "host.txt.gz").read_bytes())
    got = engine.scores_text_bgzf(loc, torch.from_numpy(x).cuda(), eof=True)
    (d / "device.txt.gz").write_bytes(got[0][:got[1]].cpu().numpy().tobytes())
    engine.release_text_buffers()
    (d / "zlib.txt.gz").write_bytes(ssw.bgzf_compress(text)[0])
    paths = {n: d / (n + ".txt.gz") for n in ("host", "device", "zlib")}
    for p in paths.values():
        assert gzip.decompress(p.read_bytes()) == text and bgzfIndex.members(p) is not None
    assert len(bgzfIndex.members(paths["host"])[0]) >= 4                       # several members: rows span their borders
    return paths, text, d


def _outcome(fn):
    try:
        x, start, end, runs = fn()
        return "ok", x.cpu().numpy(), start, end, runs
    except scoresText.NotStrict as e:
        return "NotStrict", e.row, e.code, str(e)
    except Exception as e:                                                     # noqa: BLE001 -- whatever the host path raises is the outcome
        return type(e).__name__, str(e)


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0], a[-1], b[-1])
    if a[0] == "ok":
        assert a[1].dtype == b[1].dtype and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    else:
        assert a[1:] == b[1:]


@pytest.fixture(scope="module")
def want(files):
    return _outcome(lambda: scoresText.read_scores_device(files[0]["host"]))


@pytest.mark.parametrize("chunk", [4096, 65537])
@pytest.mark.parametrize("producer", ["host", "device", "zlib"])
def test_gpu_inflate_reads_what_the_host_inflate_reads(files, want, producer, chunk, capsys):
    p = files[0][producer]
    timings = {}
    got = _outcome(lambda: scoresText.read_scores_device(p, chunk, timings=timings, inflate="gpu"))
    assert want[0] == "ok" and want[1].shape == (sum(n for _c, n in CHROMS), S) and [r[0] for r in want[4]] == [c for c, _n in CHROMS]
    _same(got, want)
    _same(_outcome(lambda: scoresText.read_scores_device(p, chunk, inflate="host")), want)
    assert {"index_s", "upload_inflate_ms", "newline_index_ms", "inflate_s", "upload_parse_ms", "coords_s"} <= set(timings)    # the device path ran
    assert "WARNING" not in capsys.readouterr().out


def test_chunk_cuts_from_the_index_are_row_ends(files):
    from epilogos_amd import engine
    text = files[1]
    a = np.frombuffer(text, dtype=np.uint8)
    for chunk, seg in ((4096, 1024), (65537, 4096), (100, 16), (17, 16)):
        count, last = engine.newline_index(torch.from_numpy(a.copy()).cuda(), seg)
        chunks, rows = scoresText.cut_chunks_indexed(len(a), chunk, seg, count.cpu().numpy(), last.cpu().numpy())
        assert chunks[0][0] == 0 and chunks[-1][1] == len(a) and all(x[1] == y[0] for x, y in zip(chunks, chunks[1:]))
        longest = max(len(r) for r in text.split(b"\n")) + 1
        for (lo, hi), r in zip(chunks, rows):
            assert hi > lo and a[hi - 1] == 10 and r == int(np.count_nonzero(a[lo:hi] == 10)) and hi - lo <= max(chunk, longest + seg)


def test_no_final_newline_and_no_end_of_file_block(files, capsys):
    paths, text, d = files
    cut = d / "cut.txt.gz"
    cut.write_bytes(ssw.bgzf_compress(text[:-1])[0])                           # the last row ends with the file
    noeof = d / "noeof.txt.gz"
    noeof.write_bytes(paths["host"].read_bytes()[:-28])
    for p in (cut, noeof):
        for chunk in (4096, scoresText.CHUNK_BYTES):
            timings = {}
            got = _outcome(lambda: scoresText.read_scores_device(p, chunk, timings=timings, inflate="gpu"))
            _same(got, _outcome(lambda: scoresText.read_scores_device(p, chunk)))
            assert got[0] == "ok" and "index_s" in timings
    assert "WARNING" not in capsys.readouterr().out


def test_plain_gzip_goes_to_the_host_silently(files, want, capsys):
    paths, text, d = files
    plain = d / "plain.txt.gz"
    plain.write_bytes(gzip.compress(text))
    raw = d / "raw.txt"
    raw.write_bytes(text)
    for p in (plain, raw):
        timings = {}
        _same(_outcome(lambda: scoresText.read_scores_device(p, timings=timings, inflate="gpu")), want)
        assert "index_s" not in timings and "upload_inflate_ms" not in timings
    assert capsys.readouterr().out == ""


def test_a_flipped_payload_bit_warns_once_and_the_host_decides(files, capsys):
    paths, _text, d = files
    blob = bytearray(paths["zlib"].read_bytes())
    table, _total = bgzfIndex.members(bytes(blob))
    k = 2
    blob[int(table[k, 0]) + int(table[k, 1]) // 2] ^= 0x10
    bad = d / "flipped.txt.gz"
    bad.write_bytes(bytes(blob))
    host = _outcome(lambda: scoresText.read_scores_device(bad))
    capsys.readouterr()
    got = _outcome(lambda: scoresText.read_scores_device(bad, inflate="gpu"))
    lines = [l for l in capsys.readouterr().out.splitlines() if "WARNING" in l]
    assert len(lines) == 1 and lines[0].startswith("WARNING: [--inflate gpu] %s: member %d (" % (bad, k)) and lines[0].endswith("inflating on the host instead")
    _same(got, host)


def test_a_file_outside_the_grammar_raises_the_same(files):
    paths, text, d = files
    rows = text.split(b"\n")
    rows[4321] = rows[4321].replace(b"\t0.", b"\t0,", 1) if b"\t0." in rows[4321] else rows[4321] + b"x"
    p = d / "odd.txt.gz"
    p.write_bytes(ssw.bgzf_compress(b"\n".join(rows))[0])
    host = _outcome(lambda: scoresText.read_scores_device(p, 4096))
    assert host[0] == "NotStrict" and host[1] == 4321
    _same(_outcome(lambda: scoresText.read_scores_device(p, 4096, inflate="gpu")), host)
    with pytest.raises(ValueError, match="inflate"):
        scoresText.read_scores_device(p, inflate="cpu")


# ---- the commands --------------------------------------------------------------------------------------------------------------------
def _run(args, timeout=600):
    cmd = [sys.executable, "-m", "epilogos_amd.similaritySearch_run"] + [str(a) for a in args]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    return res.stdout


def test_the_live_query_writes_the_same_files(tmp_path):
    """The golden regions of tests/test_hip_simsearch_query.py against their scores file as BGZF."""
    from tests.test_hip_simsearch_step1 import GOLD
    sp = tmp_path / "scores_s200.txt.gz"
    sp.write_bytes(ssw.bgzf_compress(GOLD["s200_scores_txt"].tobytes())[0])
    qf = tmp_path / "regions.bed"
    qf.write_text("".join("\t".join(line.split("\t")[:3]) + "\n" for line in GOLD["s200_bed_text"].tobytes().decode().splitlines()))
    a, b = tmp_path / "a", tmp_path / "b"
    w = ["-q", qf, "-s", sp, "-w", int(GOLD["s200_windowBP"])]
    _run(w + ["-o", a])
    out = _run(w + ["-o", b, "--inflate", "gpu"])
    assert "WARNING" not in out and "Warning" not in out
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and len(names) == len(GOLD["s200_cube_coords"]) and all(n.endswith("_recs.bed") for n in names)
    assert all((a / n).read_bytes() == (b / n).read_bytes() for n in names) and any((a / n).stat().st_size > 0 for n in names)


def test_the_build_writes_the_same_files(tmp_path):
    from tests.test_hip_simsearch_step1 import GOLD, OUTPUTS
    sp = tmp_path / "scores_s200.txt.gz"
    sp.write_bytes(ssw.bgzf_compress(GOLD["s200_scores_txt"].tobytes())[0])
    w = ["-b", "-s", sp, "-w", int(GOLD["s200_windowBP"]), "--step1", "gpu"]
    _run(w + ["-o", tmp_path / "host"])
    out = _run(w + ["-o", tmp_path / "gpu", "--inflate", "gpu"])
    assert "WARNING" not in out and "Warning" not in out
    for f in OUTPUTS:
        if f == "simsearch_cube.npz":
            x, y = np.load(tmp_path / "host" / f, allow_pickle=True), np.load(tmp_path / "gpu" / f, allow_pickle=True)
            assert x["scores"].tobytes() == y["scores"].tobytes() and (x["coords"] == y["coords"]).all()
        else:
            assert (tmp_path / "host" / f).read_bytes() == (tmp_path / "gpu" / f).read_bytes(), f
