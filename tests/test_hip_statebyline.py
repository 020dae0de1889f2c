"""GPU: ChromHMM state-by-line calls -> state matrix (csrc/epg_statebyline.hip, epilogos_amd/stateByLine.py, the
`epilogos_amd.preprocess` command), bit for bit against a numpy restatement written here (split lines, int - 1, stack columns) and
against the reference's own matrix_chr1.txt (tests/golden/statebyline.npz).  Integers only: no tolerance anywhere.

Every kernel call runs in a guarded arena (tests/abi_arena.py): buffers sized exactly, guards checked after each call.  The text
boundaries the parser's cases aim at come from the library (epg_sbl_constant), not from a copy of its constants."""
import gzip
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import _abi, helpers, stateByLine as sbl
from tests.abi_arena import Arena
from tests.conftest import free_port
from tests.test_statebyline_host import GOLD, numpy_matrix

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEAD = b"BSS00001\tchr1\nMaxStateE\n"
CHILD_LIMIT = 240
_broken = []


def const(which):
    return int(_abi.load().epg_sbl_constant(which))


def TB():
    return const(0)


def BB():
    return const(1)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------

def make_text(values, head=HEAD, final_newline=True):
    body = "".join("%d\n" % v for v in values).encode()
    text = head + body
    return text if final_newline or not len(text) else text[:-1]


def ref_column(text):
    """-> (int8 column, rows, lo, hi) of a text of the grammar: split lines, int - 1."""
    lines = text.decode("latin-1").split("\n")
    if lines[-1] == "":
        lines.pop()
    v = np.array([int(l) for l in lines[2:]], dtype=np.int64)
    return (v - 1).astype(np.int8), len(v), (int(v.min()) if len(v) else 0), (int(v.max()) if len(v) else 0)


def mixed_values(rng, R, top=100):
    """1-, 2- and 3-digit values side by side, so that line starts drift against every power-of-two block of text."""
    v = np.where(rng.random(R) < 0.4, rng.integers(1, 10, size=R), rng.integers(10, top + 1, size=R))
    if R > 2:
        v[rng.integers(0, R, size=max(1, R // 7))] = top
    return v


def parse_call(text, cap=None, prefill="random", text_mis=0, col_mis=0, seed=0):
    """One epg_sbl_parse in a guarded arena.  -> (col [cap] as left by the call, what it held before, info [4])."""
    import torch
    lib = _abi.load()
    rng = np.random.default_rng(seed)
    n = len(text)
    if cap is None:
        cap = ref_rows(text)
    wsb = lib.epg_sbl_ws_bytes(n)
    ar = Arena("cuda", guard_byte=1)
    ar.add("text", n, role="in", misalign=text_mis)
    ar.add("col", cap, role="out", align=16, misalign=col_mis)
    ar.add("info", 32, role="out", align=8)
    ar.add("ws", wsb, role="ws", align=16)
    ar.build()
    ar.write("text", np.frombuffer(text, dtype=np.uint8))
    for name in ("col", "info", "ws"):
        ar.fill(name, prefill, rng)
    before = ar.read("col", np.int8)
    ar.snapshot()
    _abi.call("epg_sbl_parse", ar.ptr("text"), n, ar.ptr("col") if cap else None, cap, ar.ptr("info"), ar.ptr("ws"), wsb, None)
    torch.cuda.synchronize()
    ar.check()                                                   # guards intact, the text unchanged
    return ar.read("col", np.int8), before, ar.read("info", np.int64)


def ref_rows(text):
    if not text:
        return 0
    return max(text.count(b"\n") + (0 if text.endswith(b"\n") else 1) - 2, 0)


def check_good(text, **kw):
    want, rows, lo, hi = ref_column(text)
    col, _before, info = parse_call(text, **kw)
    assert info.tolist() == [rows, lo, hi, -1], (info.tolist(), [rows, lo, hi, -1])
    assert np.array_equal(col, want)


# ---- the parser -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("R", [0, 1, 63, 64, 65, 4097])
def test_parse_sizes(R, final_newline):
    rng = np.random.default_rng(R)
    text = make_text(mixed_values(rng, R), final_newline=final_newline)
    for k, prefill in enumerate((0x00, 0xFF, "random")):
        check_good(text, prefill=prefill, text_mis=(5 * k + 3) % 16, col_mis=(7 * k) % 16, seed=k)


def _text_with_line_at(start, values_before=5, rows_after=300, seed=0, final_newline=True):
    """A text whose line number `values_before` (a 2-digit value, 3 bytes with its newline) starts at byte `start`: the header
    is padded so that `values_before` 2-digit lines lie before it; mixed lines follow."""
    rng = np.random.default_rng(seed)
    pad = start - 3 * values_before - len(HEAD)
    assert pad >= 0
    head = HEAD[:-1] + b"x" * pad + b"\n"
    vals = np.concatenate([rng.integers(10, 100, size=values_before + 1), mixed_values(rng, rows_after)])
    text = make_text(vals, head=head, final_newline=final_newline)
    assert text[start:start + 3] == b"%d\n" % vals[values_before]
    return text


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("boundary", ["thread", "block", "block2"])
def test_parse_lines_across_the_kernels_text_boundaries(boundary, phase):
    """A 2-digit line "NN\\n" placed so that the boundary between two threads' (two workgroups') bytes of text falls before it
    (phase 0), between its digits (1), between the digits and the newline (2) and right behind the newline (3)."""
    b = {"thread": 3 * TB(), "block": BB(), "block2": 2 * BB()}[boundary]
    text = _text_with_line_at(b - phase, seed=phase)
    check_good(text, text_mis=phase, col_mis=11)
    check_good(text[:-1], text_mis=0, col_mis=0)


@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("boundary", ["thread", "block"])
def test_parse_text_that_ends_on_a_boundary(boundary, final_newline):
    """The last line's (real or virtual) newline is the last byte before, or the first byte behind, a boundary: the virtual one of
    a text of exactly one workgroup's bytes belongs to a workgroup that holds no byte of the text."""
    b = {"thread": 5 * TB(), "block": BB()}[boundary]
    for last in (7, 42, 100):
        digits = len(str(last))
        start = b - digits - (1 if final_newline else 0)         # the last line ends the text at byte b
        text = _text_with_line_at(start - 3, values_before=5, rows_after=0)     # six 2-digit lines end at byte `start`
        text = text[:start] + b"%d\n" % last
        text = text if final_newline else text[:-1]
        assert len(text) == b and ref_rows(text) == 7
        check_good(text, col_mis=3)


def test_parse_header_longer_than_a_block():
    rng = np.random.default_rng(3)
    noise = bytes(rng.choice(np.frombuffer(b"0123456789\r\t xyz\xff", dtype=np.uint8), size=BB() + 1000))
    for head in (b"n\tchr1\n" + noise + b"\n", noise + b"\n" + noise + noise + b"\n", b"\n\n"):
        text = make_text(mixed_values(rng, 500), head=head)
        check_good(text)


def test_parse_cap_below_the_rows_and_texts_without_headers():
    rng = np.random.default_rng(4)
    text = make_text(mixed_values(rng, 3000))
    want, rows, lo, hi = ref_column(text)
    for cap in (0, 1, 1499, 2999):
        col, before, info = parse_call(text, cap=cap, col_mis=9)
        assert info[0] == rows == 3000 and info[3] == -1
        assert np.array_equal(col, want[:cap])                   # (the arena's guard behind col[cap - 1] is intact: parse_call)
    col, before, info = parse_call(text, cap=3100, col_mis=2)    # a column longer than the text: the rest keeps what it held
    assert info.tolist() == [3000, lo, hi, -1] and np.array_equal(col[:3000], want) and np.array_equal(col[3000:], before[3000:])
    for text, bad in ((b"", 0), (b"one line", 1), (b"one line\n", 1)):
        col, before, info = parse_call(text, cap=16)
        assert info.tolist() == [0, 0, 0, bad] and np.array_equal(col, before)
    for text in (b"a\nb", b"a\nb\n"):                            # headers only
        col, before, info = parse_call(text, cap=16)
        assert info.tolist() == [0, 0, 0, -1] and np.array_equal(col, before)


BAD_LINES = {"carriage return": b"7\r", "empty line": b"", "zero": b"0", "128": b"128", "four digits": b"1234", "a letter": b"x",
             "a blank": b" 7", "a sign": b"+7", "a leading zero": b"07", "999": b"999"}


@pytest.mark.parametrize("what", sorted(BAD_LINES))
def test_parse_reports_the_first_line_outside_the_grammar(what):
    rng = np.random.default_rng(len(what))
    vals = mixed_values(rng, 3000)
    lines = [b"%d" % v for v in vals]
    for at in ([5], [1500, 2500], [2999], [0, 1, 2]):
        bad = list(lines)
        for r in at:
            bad[r] = BAD_LINES[what]
        text = HEAD + b"\n".join(bad) + b"\n"
        good = np.ones(3000, dtype=bool)
        good[at] = False
        for t in (text, text[:-1]) if what != "empty line" or at != [2999] else (text,):
            col, before, info = parse_call(t, cap=3010, col_mis=1)
            assert info[0] == 3000 and info[3] == 2 + at[0], (what, at, info.tolist())
            assert info[1] == vals[good].min() and info[2] == vals[good].max()
            assert np.array_equal(col[:3000][good], (vals[good] - 1).astype(np.int8))
            assert (col[:3000][~good] == -1).all()
            assert np.array_equal(col[3000:], before[3000:])
    text = HEAD + b"x\n" * 40                                    # no line of the grammar at all
    col, _before, info = parse_call(text, cap=40)
    assert info.tolist() == [40, 128, 0, 2] and (col == -1).all()


# ---- the transpose --------------------------------------------------------------------------------------------------------

def transpose_call(cols, R, pitch, ldx, col0, canary_seed=0, x_mis=0):
    """One epg_sbl_transpose in a guarded arena: cols [nb, pitch] (the bytes behind R random), X [R, ldx] prefilled with a
    canary pattern.  -> (X after, X before)."""
    import torch
    nb = cols.shape[0]
    rng = np.random.default_rng(canary_seed)
    ar = Arena("cuda", guard_byte=1)
    ar.add("cols", nb * pitch, role="in", align=16)
    ar.add("X", R * ldx, role="out", align=16, misalign=x_mis)
    ar.build()
    ar.write("cols", cols)
    ar.fill("X", "random", rng)
    before = ar.read("X", np.int8).reshape(R, ldx)
    ar.snapshot()
    _abi.call("epg_sbl_transpose", ar.ptr("cols"), nb, pitch, R, ar.ptr("X"), ldx, col0, None)
    torch.cuda.synchronize()
    ar.check()
    return ar.read("X", np.int8).reshape(R, ldx), before


# (N, ldx, [(col0, nb)]): the batches of one matrix; 65 columns go as two batches
LAYOUTS = [(10, 16, [(3, 7)]), (10, 16, [(9, 1)]), (10, 16, [(0, 10)]), (16, 16, [(0, 16)]), (16, 16, [(4, 7)]), (16, 16, [(15, 1)]),
           (833, 848, [(64, 64)]), (833, 848, [(769, 64)]), (833, 848, [(100, 64), (164, 1)]), (833, 848, [(832, 1)]), (833, 848, [(6, 7)]),
           (70, 70, [(3, 64)]), (68, 68, [(4, 64)])]


@pytest.mark.parametrize("R", [1, 63, 65, 4097])
def test_transpose(R):
    rng = np.random.default_rng(R)
    for N, ldx, batches in LAYOUTS:
        if max(nb for _c, nb in batches) > const(3):
            continue
        for extra, x_mis in ((0, 0), (48, 0), (0, 2)):           # (a matrix off the 4-byte boundary goes out by bytes)
            pitch = (R + 15) // 16 * 16 + extra
            for col0, nb in batches:
                cols = rng.integers(-128, 128, size=(nb, pitch)).astype(np.int8)
                X, before = transpose_call(cols, R, pitch, ldx, col0, canary_seed=N + col0, x_mis=x_mis)
                want = before.copy()
                want[:, col0:col0 + nb] = cols[:, :R].T
                assert np.array_equal(X, want), (N, ldx, col0, nb, R, pitch)


def test_transpose_of_the_largest_batch_plus_one_is_refused():
    with pytest.raises(_abi.EpilogosHipError) as e:
        transpose_call(np.zeros((const(3) + 1, 16), dtype=np.int8), 5, 16, 848, 0)
    assert e.value.code == -2


# ---- build_matrix_device --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_dir(tmp_path_factory):
    """The golden inputs as a data directory, metadata and chromsizes; the reference's matrix_chr1.txt next to them."""
    base = tmp_path_factory.mktemp("sbl")
    d = base / "calls"
    d.mkdir()
    for k, n in enumerate(GOLD["names"]):
        with gzip.open(d / str(n), "wb") as fh:
            fh.write(GOLD["text_%d" % k].tobytes())
    (base / "meta.txt").write_bytes(GOLD["metadata"].tobytes())
    (base / "sizes.txt").write_bytes(GOLD["chromsizes"].tobytes())
    ref = base / "ref" / "in"
    ref.mkdir(parents=True)
    (ref / "matrix_chr1.txt").write_bytes(GOLD["matrix"].tobytes())
    return base


def test_build_matrix_device_equals_the_golden_matrix(golden_dir):
    (chrom, files), = sbl.find_calls(golden_dir / "calls", golden_dir / "meta.txt", golden_dir / "sizes.txt")
    X, N, name, rng = sbl.build_matrix_device(files)
    want, _loc, want_rng = helpers.readTable(golden_dir / "ref" / "in" / "matrix_chr1.txt", with_range=True)
    assert (chrom, name, N) == ("chr1", "chr1", 10) and tuple(X.shape) == (2048, 16) and rng == want_rng
    x = X.cpu().numpy()
    assert np.array_equal(x[:, :10], want) and (x[:, 10:] == -1).all()
    assert np.array_equal(want, numpy_matrix([GOLD["text_%d" % k] for k in range(10)])[0])


def _write_calls(d, texts, chrom="chr1"):
    d.mkdir(parents=True, exist_ok=True)
    files = []
    for k, t in enumerate(texts):
        p = d / ("B%03d_18_chr1_statebyline.txt" % k)
        p.write_bytes(t)
        files.append(p)
    return files


def test_build_matrix_device_many_files_and_the_host_fallback(tmp_path, capsys):
    """More files than one batch holds, uncompressed and gzip side by side; one of them with \\r\\n line ends: warned about once,
    read on the host, the column right."""
    rng = np.random.default_rng(8)
    n = const(3) + 3
    vals = [mixed_values(rng, 777) for _ in range(n)]
    texts = [make_text(v, final_newline=k % 3 != 0) for k, v in enumerate(vals)]
    texts[5] = texts[5].replace(b"\n", b"\r\n")
    files = _write_calls(tmp_path / "calls", texts)
    with gzip.open(str(files[2]) + ".gz", "wb") as fh:
        fh.write(texts[2])
    files[2].unlink()
    files[2] = Path(str(files[2]) + ".gz")
    X, N, name, (lo, hi) = sbl.build_matrix_device(files)
    out = capsys.readouterr().out
    assert out.count(str(files[5])) == 1 and "line 3" in out and sum(str(f) in out for f in files) == 1
    want = np.stack(vals, axis=1)
    assert N == n and name == "chr1" and (lo, hi) == (want.min(), want.max())
    x = X.cpu().numpy()
    assert x.shape == (777, (n + 15) // 16 * 16) and np.array_equal(x[:, :n], (want - 1).astype(np.int8)) and (x[:, n:] == -1).all()


def test_build_matrix_device_third_batch_reuses_a_slot_that_has_to_grow(tmp_path, capsys):
    """Two full batches and one file more: the third batch is the first to reuse a staging slot.  Its one file is larger than the
    whole first batch plus an eighth (a padded second header line), so slot 0 waits for its event and grows; it has \\r\\n line
    ends as well, so its column is the host's.  R = 33 is no multiple of 16: the column pitch is 48."""
    rng = np.random.default_rng(129)
    batch, R = const(3), 33
    n = 2 * batch + 1
    vals = [mixed_values(rng, R) for _ in range(n)]
    texts = [make_text(v, final_newline=k % 3 != 0) for k, v in enumerate(vals)]
    first_batch = sum((len(t) + 15) // 16 * 16 for t in texts[:batch])
    pad = first_batch + first_batch // 8 + 4096                  # beyond what slot 0 was given for the first batch
    texts[n - 1] = make_text(vals[n - 1], head=HEAD[:-1] + b"x" * pad + b"\n").replace(b"\n", b"\r\n")
    files = _write_calls(tmp_path / "calls", texts)
    zipped = batch + 6                                           # a file of the second batch
    with gzip.open(str(files[zipped]) + ".gz", "wb") as fh:
        fh.write(texts[zipped])
    files[zipped].unlink()
    files[zipped] = Path(str(files[zipped]) + ".gz")
    X, N, name, (lo, hi) = sbl.build_matrix_device(files)
    out = capsys.readouterr().out
    assert out.count(str(files[n - 1])) == 1 and sum(str(f) in out for f in files) == 1
    want = np.stack(vals, axis=1)
    assert N == n == 129 and name == "chr1" and (lo, hi) == (want.min(), want.max())
    x = X.cpu().numpy()
    assert x.shape == (R, (n + 15) // 16 * 16) and np.array_equal(x[:, :n], (want - 1).astype(np.int8)) and (x[:, n:] == -1).all()


def test_build_matrix_device_refusals(tmp_path, capsys):
    rng = np.random.default_rng(9)
    texts = [make_text(mixed_values(rng, 100)) for _ in range(3)]
    files = _write_calls(tmp_path / "rows", texts[:2] + [make_text(mixed_values(rng, 99))])
    with pytest.raises(ValueError) as e:
        sbl.build_matrix_device(files)
    assert str(files[0]) in str(e.value) and str(files[2]) in str(e.value) and "100" in str(e.value) and "99" in str(e.value)
    files = _write_calls(tmp_path / "chrom", texts[:2] + [texts[2].replace(b"\tchr1\n", b"\tchr2\n", 1)])
    with pytest.raises(ValueError) as e:
        sbl.build_matrix_device(files)
    assert str(files[0]) in str(e.value) and str(files[2]) in str(e.value) and "chr2" in str(e.value)
    files = _write_calls(tmp_path / "junk", texts[:2] + [texts[2].replace(b"\n", b"\nx", 5)])
    with pytest.raises(ValueError) as e:
        sbl.build_matrix_device(files)
    assert str(files[2]) in str(e.value) and capsys.readouterr().out.count(str(files[2])) == 1


# ---- the command, end to end ----------------------------------------------------------------------------------------------

def _child(cmd, env):
    if _broken:
        pytest.fail("not started: an earlier child process failed (%s)" % _broken[0])
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
        _broken.append(" ".join(cmd))
        raise
    if res.returncode != 0 or "ERROR" in res.stdout:
        _broken.append(" ".join(cmd))
        pytest.fail("%s\n%s%s" % (" ".join(cmd), res.stdout, res.stderr))
    return res.stdout


def run_epilogos(args, out, world=1):
    """`epilogos -l` as a child process -> its output directory.  Two ranks: torch.distributed.run, gloo, both on the one GPU."""
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "epilogos_amd.run", "-l"] + args + ["-o", str(out), "-f", "t"]
    if world > 1:
        port = str(free_port())
        env.update(EPILOGOS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", port] + cmd[1:]
    _child(cmd, env)
    return out


def same_outputs(a, b, prefixes):
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir())
    for pre in prefixes:
        assert any(n.startswith(pre) for n in names), (pre, names)
    for n in names:
        if n.endswith(".gz"):
            with gzip.open(a / n, "rb") as fa, gzip.open(b / n, "rb") as fb:
                assert fa.read() == fb.read(), n
        else:
            assert (a / n).read_bytes() == (b / n).read_bytes(), n


@pytest.fixture(scope="module")
def prepared(golden_dir):
    """The command on the golden inputs -> (directory of the .epgm, directory of the reference's text matrix, state metadata)."""
    out = golden_dir / "epgm" / "in"
    (golden_dir / "sizes2.txt").write_text("chrM\t16571\nchr1\t249250621\n")
    stdout = _child([sys.executable, "-m", "epilogos_amd.preprocess", str(golden_dir / "calls"), str(golden_dir / "meta.txt"),
                     str(golden_dir / "sizes2.txt"), "-o", str(out), "-c", "4"], dict(os.environ, PYTHONPATH=str(ROOT)))
    assert stdout == "Processing chrM: 0 files found. Skipping.\nProcessing chr1: 10 files found. Done.\n"
    assert [p.name for p in out.iterdir()] == ["matrix_chr1.epgm"]
    meta = golden_dir / "states.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(18)))
    return out, golden_dir / "ref" / "in", meta


def test_command_writes_the_golden_matrix(prepared):
    epgm, ref, _meta = prepared
    a = helpers.readTable(epgm / "matrix_chr1.epgm", with_range=True)
    b = helpers.readTable(ref / "matrix_chr1.txt", with_range=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].blob, b[1].blob) and np.array_equal(a[1].offsets, b[1].offsets) and a[2] == b[2]
    assert sbl.read_epgm_header(epgm / "matrix_chr1.epgm")["chrom"] == "chr1"


def test_single_mode_from_the_binary_matrix_equals_the_text_matrix(tmp_path, prepared):
    epgm, ref, meta = prepared
    args = ["-j", str(meta), "-s", "1"]
    a = run_epilogos(["-i", str(epgm)] + args, tmp_path / "a")
    b = run_epilogos(["-i", str(ref)] + args, tmp_path / "b")
    same_outputs(a, b, ["scores_t_matrix_chr1", "regionsOfInterest_"])
    two = run_epilogos(["-i", str(epgm)] + args, tmp_path / "two", world=2)
    same_outputs(two, a, ["scores_t_matrix_chr1", "regionsOfInterest_"])


def test_paired_columns_from_the_binary_matrix_equal_the_text_matrix(tmp_path, prepared):
    epgm, ref, meta = prepared
    args = ["-m", "paired", "--columns-a", "1-5", "--columns-b", "6-10", "-j", str(meta), "-s", "1", "--null-seed", "77"]
    a = run_epilogos(["-i", str(epgm)] + args, tmp_path / "a")
    b = run_epilogos(["-i", str(ref)] + args, tmp_path / "b")
    same_outputs(a, b, ["pairwiseDelta_t_matrix_chr1", "pairwiseMetrics_"])
