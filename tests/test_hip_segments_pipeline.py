"""GPU: `python -m epilogos_amd.preprocess --segments` end to end (epilogos_amd/segments.py): the same calls written as
state-by-line files and as segment files give byte-identical .epgm files, the golden calls of tests/golden/statebyline.npz,
run-length encoded here, give the golden matrix, a file the device refuses goes through the host parser, errors of content and
a chromosome missing from one file raise, --bin-width reaches the header, and `epilogos -i` scores both directories alike."""
import io

import numpy as np
import pytest

from epilogos_amd import helpers, preprocess, stateByLine as sbl
from tests.test_hip_statebyline import run_epilogos, same_outputs
from tests.test_statebyline_host import GOLD

pytestmark = pytest.mark.gpu

CHROMS = [("chrA", 1), ("chrB", 300), ("chrC", 5000)]
N = 70                                                           # one batch of 64 columns and a second of 6


def rle(col):
    """A column of states -> (start bin, end bin, state) per run of equal states."""
    col = np.asarray(col)
    cut = np.flatnonzero(np.diff(col)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(col)]])
    return starts, ends, col[starts]


def segment_text(calls, width=200, label="E%d", eol="\n"):
    """calls: [(chromosome, column of states 1..127)] -> the text of a segment file."""
    out = []
    for chrom, col in calls:
        for s, e, v in zip(*rle(col)):
            out.append("%s\t%d\t%d\t%s%s" % (chrom, s * width, e * width, label % v, eol))
    return "".join(out).encode()


def random_calls(rng, R):
    """A column with runs: about a third of the bins start a new one."""
    v = rng.integers(1, 19, size=R)
    keep = rng.random(R) < 0.65
    keep[0] = False
    idx = np.maximum.accumulate(np.where(keep, 0, np.arange(R)))
    return v[idx]


@pytest.fixture(scope="module")
def calls():
    rng = np.random.default_rng(70)
    return [[(c, random_calls(rng, R)) for c, R in CHROMS] for _ in range(N)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory, calls):
    """The calls as a directory of state-by-line files and as one of segment files, with the metadata and chromsizes."""
    base = tmp_path_factory.mktemp("seg")
    (base / "sbl").mkdir()
    (base / "seg").mkdir()
    for k, per_chrom in enumerate(calls):
        for c, col in per_chrom:
            (base / "sbl" / ("B%03d_18_%s_statebyline.txt" % (k, c))).write_bytes(
                b"B%03d\t%s\nMaxStateE\n" % (k, c.encode()) + "".join("%d\n" % v for v in col).encode())
        (base / "seg" / ("B%03d_18_segments.bed" % k)).write_bytes(
            segment_text([("chrUn", [3, 3, 4])] + per_chrom[::-1] + [("chrM", [1])]))      # the file's own order, and other chromosomes
    (base / "meta.txt").write_text("id\n" + "".join("B%03d\n" % k for k in range(N)))
    (base / "sizes.txt").write_text("chrA\t200\nchrB\t60000\nchrZ\t5\nchrC\t999801\n")
    return base


def _run(base, src, dest, **kw):
    out = io.StringIO()
    written = preprocess.run(base / src, base / "meta.txt", base / kw.pop("sizes", "sizes.txt"), base / dest, out=out, **kw)
    return written, out.getvalue()


@pytest.fixture(scope="module")
def built(tree):
    a, out_a = _run(tree, "sbl", "out_sbl")
    b, out_b = _run(tree, "seg", "out_seg", segments=True)
    return a, out_a, b, out_b


def test_segments_and_state_by_line_write_the_same_bytes(built, calls):
    a, out_a, b, out_b = built
    assert out_a == out_b == ("Processing chrA: 70 files found. Done.\nProcessing chrB: 70 files found. Done.\n"
                              "Processing chrZ: 0 files found. Skipping.\nProcessing chrC: 70 files found. Done.\n")
    assert [p.name for p in a] == [p.name for p in b] == ["matrix_chrA.epgm", "matrix_chrB.epgm", "matrix_chrC.epgm"]
    for pa, pb, (c, R) in zip(a, b, CHROMS):
        raw = pb.read_bytes()
        assert raw == pa.read_bytes(), c                         # the header included
        want = np.stack([dict(per)[c] for per in calls], axis=1)
        assert np.array_equal(np.frombuffer(raw[128:], dtype=np.int8).reshape(R, N), (want - 1).astype(np.int8))
        h = sbl.read_epgm_header(pb)
        assert (h["R"], h["N"], h["width"], h["lo"], h["hi"], h["chrom"]) == (R, N, 200, want.min(), want.max(), c)


def _golden_columns():
    return [np.array([int(l) for l in GOLD["text_%d" % k].tobytes().decode().split("\n")[2:] if l]) for k in range(10)]


def _golden_tree(base, eol_of=lambda k: "\n", label="E%d"):
    d = base / "calls"
    d.mkdir(parents=True)
    biosamples = [l.split("\t")[0] for l in GOLD["metadata"].tobytes().decode().split("\n")[1:] if l]
    order = [next(k for k, n in enumerate(GOLD["names"]) if b in str(n)) for b in biosamples]
    assert sorted(order) == list(range(10))
    for k in order:
        (d / ("%s_18_segments.bed" % biosamples[order.index(k)])).write_bytes(segment_text([("chr1", _golden_columns()[k])], label=label, eol=eol_of(k)))
    (base / "meta.txt").write_bytes(GOLD["metadata"].tobytes())
    (base / "sizes.txt").write_bytes(GOLD["chromsizes"].tobytes())
    return d


@pytest.fixture(scope="module")
def golden_built(tmp_path_factory):
    base = tmp_path_factory.mktemp("seg_golden")
    _golden_tree(base)
    written, out = _run(base, "calls", "epgm", segments=True)
    ref = base / "ref"
    ref.mkdir()
    (ref / "matrix_chr1.txt").write_bytes(GOLD["matrix"].tobytes())
    return base, written, out


def test_golden_calls_as_segments_give_the_golden_matrix(golden_built):
    base, written, out = golden_built
    assert [p.name for p in written] == ["matrix_chr1.epgm"] and "Processing chr1: 10 files found. Done.\n" in out
    a = helpers.readTable(written[0], with_range=True)
    b = helpers.readTable(base / "ref" / "matrix_chr1.txt", with_range=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].blob, b[1].blob) and np.array_equal(a[1].offsets, b[1].offsets) and a[2] == b[2]
    assert sbl.read_epgm_header(written[0])["chrom"] == "chr1"


def test_a_refused_file_takes_the_host_path(tmp_path, golden_built, capsys):
    base, written, _out = golden_built
    d = _golden_tree(tmp_path, eol_of=lambda k: "\r\n" if k == 4 else "\n")
    capsys.readouterr()
    again, _ = _run(tmp_path, "calls", "epgm", segments=True)
    warned = capsys.readouterr().out
    crlf = [p for p in d.iterdir() if b"\r" in p.read_bytes()]
    assert len(crlf) == 1 and warned.count(str(crlf[0])) == 1 and warned.count("on the host") == 1 and "line 1 " in warned
    assert again[0].read_bytes() == written[0].read_bytes()
    # the first file refused (six fields): R_c comes from the host parser
    names = tmp_path / "names"
    d = _golden_tree(names, label="%d_S")
    first = sorted(d.iterdir(), key=lambda p: GOLD["metadata"].tobytes().decode().index(p.name.split("_18_")[0]))[0]
    first.write_bytes(first.read_bytes().replace(b"_S\n", b"_S\tx\ty\n"))
    third, _ = _run(names, "calls", "epgm", segments=True)
    assert capsys.readouterr().out.count(str(first)) == 1
    assert third[0].read_bytes() == written[0].read_bytes()


def test_errors_of_content_and_a_missing_chromosome_raise(tmp_path, tree, capsys):
    d = tmp_path / "seg"
    d.mkdir()
    for p in sorted((tree / "seg").iterdir())[:3]:
        (d / p.name).write_bytes(p.read_bytes())
    (tmp_path / "meta.txt").write_text("id\nB000\nB001\nB002\n")
    (tmp_path / "sizes.txt").write_text("chrA\t200\nchrB\t60000\nchrC\t999801\n")
    victim = d / "B001_18_segments.bed"
    good = victim.read_bytes()
    lines = good.split(b"\n")
    k = next(i for i, l in enumerate(lines) if l.startswith(b"chrB\t")) + 5
    gap = lines[:k] + lines[k + 1:]                              # a segment taken out: the one behind it starts late
    victim.write_bytes(b"\n".join(gap))
    with pytest.raises(ValueError) as e:
        _run(tmp_path, "seg", "out", segments=True)
    assert "%s:%d:" % (victim, k + 1) in str(e.value) and "gap" in str(e.value)
    assert capsys.readouterr().out.count(str(victim)) == 1       # refused on the device first, then read on the host
    victim.write_bytes(b"\n".join(l for l in lines if not l.startswith(b"chrB\t")))
    with pytest.raises(ValueError) as e:
        _run(tmp_path, "seg", "out", segments=True)
    assert "chrB" in str(e.value) and str(victim) in str(e.value) and str(d / "B000_18_segments.bed") in str(e.value)
    victim.write_bytes(good)
    with pytest.raises(ValueError) as e:                         # R_c against CHROMSIZES
        (tmp_path / "short.txt").write_text("chrA\t200\nchrB\t59800\nchrC\t999801\n")
        _run(tmp_path, "seg", "out", segments=True, sizes="short.txt")
    assert "chrB" in str(e.value) and "59800" in str(e.value)
    assert not (tmp_path / "out").exists() or not list((tmp_path / "out").iterdir())


def test_bin_width_reaches_the_header_and_the_coordinates(tmp_path, calls):
    d = tmp_path / "seg"
    d.mkdir()
    for k in range(3):
        (d / ("B%03d_18_segments.bed" % k)).write_bytes(segment_text(calls[k][:2], width=20, label="%d"))
    (tmp_path / "meta.txt").write_text("id\nB000\nB001\nB002\n")
    (tmp_path / "sizes.txt").write_text("chrA\t20\nchrB\t6000\n")
    written, out = _run(tmp_path, "seg", "out", segments=True, width=20)
    assert [p.name for p in written] == ["matrix_chrA.epgm", "matrix_chrB.epgm"]
    assert sbl.read_epgm_header(written[1])["width"] == 20
    states, loc = helpers.readTable(written[1])
    assert np.array_equal(states, np.stack([calls[k][1][1] for k in range(3)], axis=1) - 1)
    assert loc.blob.tobytes().startswith(b"chrB\t0\t20\nchrB\t20\t40\n") and loc.blob.tobytes().endswith(b"chrB\t5980\t6000\n")
    with pytest.raises(ValueError):                              # the same files are off the grid of 200 bp bins
        _run(tmp_path, "seg", "out200", segments=True)


def test_epilogos_scores_both_directories_alike(tmp_path, tree, golden_built):
    base, written, _out = golden_built
    d = base / "sbl_calls"
    d.mkdir()
    for k, n in enumerate(GOLD["names"]):
        (d / str(n).replace(".gz", "")).write_bytes(GOLD["text_%d" % k].tobytes())
    by_lines, _ = _run(base, "sbl_calls", "epgm_sbl")
    assert by_lines[0].read_bytes() == written[0].read_bytes()
    meta = tmp_path / "states.tsv"
    meta.write_text("zero_index\tone_index\tshort_name\n" + "".join("%d\t%d\tstate%d\n" % (i, i + 1, i + 1) for i in range(18)))
    args = ["-j", str(meta), "-s", "1"]
    a = run_epilogos(["-i", str(written[0].parent)] + args, tmp_path / "a")
    b = run_epilogos(["-i", str(by_lines[0].parent)] + args, tmp_path / "b")
    same_outputs(a, b, ["scores_t_matrix_chr1", "regionsOfInterest_"])


def test_third_batch_reuses_a_slot_that_has_to_grow(tmp_path, capsys):
    """build_matrices_device on two full batches and one file more: the third batch is the first to reuse a staging slot, and its
    one file is larger than the whole first batch plus an eighth (runs of a chromosome outside the table, which the device grammar
    skips), so slot 0 waits for its event and grows.  A file of the second batch has \\r\\n line ends and goes the host way."""
    from epilogos_amd import _abi, segments as seg
    batch = int(_abi.load().epg_sbl_constant(3))
    n = 2 * batch + 1
    table = [("chrP", 33), ("chrQ", 7)]
    rng = np.random.default_rng(129)
    per_file = [[(c, random_calls(rng, R)) for c, R in table] for _ in range(n)]
    crlf = batch + 6                                             # a file of the second batch
    texts = [segment_text(per, eol="\r\n" if k == crlf else "\n") for k, per in enumerate(per_file)]
    first_batch = sum((len(t) + 15) // 16 * 16 for t in texts[:batch])
    other = segment_text([("chrUn", np.arange(first_batch // 8) % 2 + 1)])        # one line of at least 17 bytes per bin
    assert len(other) > first_batch + first_batch // 8 + 4096    # beyond what slot 0 was given for the first batch
    texts[n - 1] = segment_text(per_file[n - 1][:1]) + other + segment_text(per_file[n - 1][1:])
    files = []
    for k, t in enumerate(texts):
        files.append(tmp_path / ("B%03d_18_segments.bed" % k))
        files[-1].write_bytes(t)
    got = seg.build_matrices_device(files, [c for c, _R in table])
    out = capsys.readouterr().out
    assert out.count("on the host") == 1 and out.count(str(files[crlf])) == 1 and sum(str(f) in out for f in files) == 1
    assert n == 129 and list(got) == [c for c, _R in table]
    for i, (c, R) in enumerate(table):
        want = np.stack([np.repeat(v, e - s) for s, e, v in (rle(per[i][1]) for per in per_file)], axis=1)
        X, (lo, hi) = got[c]
        x = X.cpu().numpy()
        assert x.shape == (R, (n + 15) // 16 * 16) and np.array_equal(x[:, :n], (want - 1).astype(np.int8)) and (x[:, n:] == -1).all(), c
        assert (lo, hi) == (want.min(), want.max()), c
