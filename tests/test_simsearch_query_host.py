"""The live similarity search query (`similaritySearch_run -q REGION -s scores`), the host side (no GPU): the window rule, the
command line's three spellings of -q, the whole path with the three device steps replaced by their numpy restatements against
tests/golden/simsearch.npz (the reference's own records for every golden region), and the argument checks of the two new entry
points."""
from pathlib import Path

import numpy as np
import pytest
from click.testing import CliRunner

from epilogos_amd import similaritySearch_max_mean as mm
from epilogos_amd import similaritySearch_query as sq
from epilogos_amd import similaritySearch_run as run
from epilogos_amd import similaritySearch_write as wr
from tests import simsearch_ref as ref

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "simsearch.npz")
CASES = ["s200", "s20"]


# ---- the window rule ------------------------------------------------------------------------------------------------------

def _table():
    """chrA: 40 bins of 200 bp from 1000 (rows 0..39), chrB: 5 bins from 0 (rows 40..44), chrC: 10 bins from 600 (rows 45..54)."""
    chroms = ["chrA"] * 40 + ["chrB"] * 5 + ["chrC"] * 10
    starts = [1000 + 200 * i for i in range(40)] + [200 * i for i in range(5)] + [600 + 200 * i for i in range(10)]
    return sq.chromosomeTable(chroms, starts, [s + 200 for s in starts])


W_BP, W_BINS = 2000, 10


def _first(chrom, start, end):
    return sq.windowFirstBin(_table(), chrom, start, end, W_BP, W_BINS)


def test_window_of_exact_length_is_taken_as_given():
    assert _first("chrA", 1000, 3000) == 0
    assert _first("chrA", 3400, 5400) == 12
    assert _first("chrC", 600, 2600) == 45                 # a chromosome of exactly the window


def test_window_of_a_longer_region_is_its_central_window():
    assert _first("chrA", 2000, 4400) == 6                 # surplus 400 (even): anchor 2200
    assert _first("chrA", 2000, 4600) == 6                 # surplus 600: anchor 2300, inside the bin at 2200
    assert _first("chrA", 2000, 4601) == 6                 # surplus 601 (odd): anchor 2000 + 300 = 2300
    assert _first("chrA", 2000, 4801) == 7                 # surplus 801 (odd): anchor 2400
    assert _first("chrA", 1000, 9000) == 15                # the whole chromosome: anchor 1000 + 3000 = 4000


def test_window_of_a_shorter_region_grows_around_its_centre():
    assert _first("chrA", 4000, 4200) == 10                # anchor 4000 - 900 = 3100, the bin at 3000
    assert _first("chrA", 4000, 4001) == 10                # anchor 4000 + (1 - 2000) // 2 = 3000
    assert _first("chrA", 4199, 4200) == 10                # anchor 4199 - 1000 = 3199: still inside the bin at 3000


def test_anchor_inside_a_bin_takes_that_bin():
    assert _first("chrA", 1399, 3399) == 1
    assert _first("chrA", 1400, 3400) == 2


def test_window_is_shifted_inside_the_chromosome():
    assert _first("chrA", 0, 2000) == 0                    # anchor before the chromosome's first bin
    assert _first("chrA", 1100, 1200) == 0                 # grown over the start
    assert _first("chrA", 8000, 10000) == 30               # sticks out at the end: the last 10 bins
    assert _first("chrA", 8900, 9000) == 30
    assert _first("chrA", 50000, 52000) == 30              # past the end altogether
    assert _first("chrC", 10000, 12000) == 45


def test_unsearchable_regions_are_refused():
    with pytest.raises(ValueError, match="fewer than the 10 of the window"):
        _first("chrB", 0, 1000)
    with pytest.raises(ValueError, match="chrZ is not in the scores file"):
        _first("chrZ", 0, 2000)
    with pytest.raises(ValueError, match="not contiguous"):
        sq.chromosomeTable(["chr1", "chr2", "chr1"], [0, 0, 200], [200, 200, 400])


# ---- the command line -----------------------------------------------------------------------------------------------------

def _scores(tmp_path, case):
    p = tmp_path / ("scores_%s.txt" % case)
    p.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    return p


def _bed_gz(tmp_path, case):
    gz, _blocks = wr.bgzf_compress(GOLD[case + "_bed_text"].tobytes())
    p = tmp_path / ("simsearch_%s.bed.gz" % case)
    p.write_bytes(gz)
    return p


def _bed_rows(case):
    """[(chr, start, end, [(chr, start, end) of each match])] of the golden simsearch.bed."""
    rows = []
    for line in GOLD[case + "_bed_text"].tobytes().decode().splitlines():
        c, s, e, m = line.split("\t")
        rows.append((c, int(s), int(e), [tuple(x.split(":")) for x in m[2:-2].split('", "')[1:]]))
    return rows


def _files(d):
    return {p.name: p.read_bytes() for p in Path(d).iterdir()}


def test_query_without_index_or_scores_is_a_usage_error(tmp_path):
    import click
    r = CliRunner().invoke(run.main, ["-q", "chr1:80000-105000", "-o", str(tmp_path / "o")], standalone_mode=False)
    assert isinstance(r.exception, click.UsageError)
    assert "-m simsearch.bed.gz" in r.exception.message and "-s scores.txt.gz" in r.exception.message
    assert not (tmp_path / "o").exists()


@pytest.mark.parametrize("with_scores", [False, True])
def test_query_with_index_is_the_lookup(tmp_path, with_scores, monkeypatch):
    from epilogos_amd import similaritySearch_query
    monkeypatch.setattr(similaritySearch_query, "liveQuery", lambda *a, **k: pytest.fail("-m must take the lookup"))
    bed = _bed_gz(tmp_path, "s200")
    c, s, e, _m = _bed_rows("s200")[4]
    q = "%s:%d-%d" % (c, s - 10, e + 10)
    want = tmp_path / "want"
    want.mkdir()
    run.querySimSearch(q, bed, want)
    args = ["-q", q, "-m", str(bed), "-o", str(tmp_path / "got")]
    if with_scores:
        args += ["-s", str(_scores(tmp_path, "s200"))]
    r = CliRunner().invoke(run.main, args, standalone_mode=False)
    assert r.exception is None, r.output
    assert len(_files(want)) == 1 and _files(tmp_path / "got") == _files(want)


# ---- the whole live path, the device steps restated in numpy --------------------------------------------------------------

@pytest.fixture
def numpy_device(monkeypatch):
    """reduceGenome, slices and search of similaritySearch_query as numpy: reduceGenomeIndices + gather, makeSlice anchored at the
    window's first bin, tests/simsearch_ref.search."""
    def reduce_genome(genome, blockSize):
        return genome, genome[mm.reduceGenomeIndices(genome, blockSize)], None

    def slices(state, first, nblk, blockSize):
        windowBins = nblk * blockSize
        return np.stack([mm.makeSlice(state[0], f + windowBins // 2, windowBins, blockSize) for f in first])

    def search(state, first, nblk, blockSize, n, ws_cap=None, batch=None):
        idx, _modes = ref.search(state[1], sq.slices(state, first, nblk, blockSize), np.asarray(first) // blockSize, n)
        return idx
    monkeypatch.setattr(sq, "reduceGenome", reduce_genome)
    monkeypatch.setattr(sq, "slices", slices)
    monkeypatch.setattr(sq, "search", search)


def _recs_file(rows_entry):
    return "".join("%s\t%s\t%s\n" % r for r in rows_entry[3])


@pytest.mark.parametrize("case", CASES)
def test_live_query_at_every_golden_region_writes_the_lookups_file(tmp_path, case, numpy_device):
    sp = _scores(tmp_path, case)
    rows = _bed_rows(case)
    assert len(rows) == len(GOLD[case + "_cube_coords"]) and len(GOLD[case + "_skip"]) == 0
    qf = tmp_path / "regions.bed"
    qf.write_text("".join("%s\t%d\t%d\n" % r[:3] for r in rows))
    out = tmp_path / "out"
    r = CliRunner().invoke(run.main, ["-q", str(qf), "-s", str(sp), "-o", str(out), "-w", str(int(GOLD[case + "_windowBP"]))],
                           standalone_mode=False)
    assert r.exception is None, r.output
    got = _files(out)
    assert len(got) == len(rows)
    for row in rows:
        name = "similarity_search_region_%s_%d_%d_recs.bed" % row[:3]
        assert got[name].decode() == _recs_file(row), name
    # and the lookup from the golden index writes the same set, byte for byte
    want = tmp_path / "want"
    want.mkdir()
    run.querySimSearch(str(qf), _bed_gz(tmp_path, case), want)
    assert _files(want) == got


def test_live_query_slices_and_self_starts_are_the_references(tmp_path):
    """The window rule at the golden regions' coordinates: the first bin's slice is the reference's cube row and its reduced
    position the reference's self start."""
    for case in CASES:
        sp = _scores(tmp_path, case)
        windowBP, windowBins, blockSize = run.windowParameters(sp, int(GOLD[case + "_windowBP"]))
        _s, inputArr, genome = mm.readScores(sp)
        table = sq.chromosomeTable(inputArr[:, 0], inputArr[:, 1], inputArr[:, 2])
        cube = np.rint(GOLD[case + "_cube_scores"] * 1e5).astype(np.int64)
        for i, (c, s, e) in enumerate(GOLD[case + "_cube_coords"]):
            f = sq.windowFirstBin(table, str(c), int(s), int(e), windowBP, windowBins)
            assert f // blockSize == GOLD[case + "_self_start"][i]
            assert np.array_equal(mm.makeSlice(genome, f + windowBins // 2, windowBins, blockSize), cube[i])


def test_bad_region_in_the_middle_of_a_bed_file(tmp_path, numpy_device):
    sp = _scores(tmp_path, "s200")
    rows = _bed_rows("s200")
    qf = tmp_path / "regions.bed"
    qf.write_text("%s\t%d\t%d\nchrZ\t0\t25000\n%s\t%d\t%d\n" % (rows[0][:3] + rows[3][:3]))
    out = tmp_path / "out"
    r = CliRunner().invoke(run.main, ["-q", str(qf), "-s", str(sp), "-o", str(out)], standalone_mode=False)
    assert r.exception is None, r.output
    assert "Could not find region in given query range: chrZ:0-25000" in r.output
    got = _files(out)
    assert sorted(got) == sorted("similarity_search_region_%s_%d_%d_recs.bed" % rows[i][:3] for i in (0, 3))
    for i in (0, 3):
        assert got["similarity_search_region_%s_%d_%d_recs.bed" % rows[i][:3]].decode() == _recs_file(rows[i])


def test_off_grid_region_is_named_by_the_window_searched(tmp_path, numpy_device):
    sp = _scores(tmp_path, "s200")
    out = tmp_path / "out"
    r = CliRunner().invoke(run.main, ["-q", "chr1:100050-100150", "-s", str(sp), "-o", str(out), "-n", "7"], standalone_mode=False)
    assert r.exception is None, r.output
    # anchor 100050 + (100 - 25000) // 2 = 87600: the bin at 87600, 125 bins on
    (name,) = _files(out)
    assert name == "similarity_search_region_chr1_87600_112600_recs.bed"
    lines = (out / name).read_text().splitlines()
    assert len(lines) <= 7 and all(int(x.split("\t")[2]) - int(x.split("\t")[1]) == 25000 for x in lines)


# ---- the entry points' argument checks ------------------------------------------------------------------------------------

def test_abi_validates_prep_arguments_without_gpu():
    import ctypes
    from epilogos_amd import _abi
    lib = _abi.load()
    assert lib.epg_simsearch_reduce(None, 0, 18, 5, None, None, None) == -1
    assert lib.epg_simsearch_reduce(None, 100, 0, 5, None, None, None) == -1
    assert lib.epg_simsearch_reduce(None, 100, 18, 0, None, None, None) == -1
    assert lib.epg_simsearch_reduce(None, 100, 18, 513, None, None, None) == -1
    assert lib.epg_simsearch_reduce(None, 100, 18, 5, None, None, None) == -1
    assert b"NULL" in lib.epg_last_error()
    first = (ctypes.c_int64 * 2)(0, 76)
    fp = ctypes.cast(first, ctypes.c_void_p)
    assert lib.epg_simsearch_slices(None, 200, 18, 5, 0, fp, 2, None, None) == -1
    assert lib.epg_simsearch_slices(None, 200, 18, 5, 65, fp, 2, None, None) == -1
    assert b"blocks outside 1..64" in lib.epg_last_error()
    assert lib.epg_simsearch_slices(None, 200, 18, 5, 25, fp, 0, None, None) == -1
    assert lib.epg_simsearch_slices(None, 200, 0, 5, 25, fp, 2, None, None) == -1
    assert lib.epg_simsearch_slices(None, 200, 18, 5, 25, None, 2, None, None) == -1
    assert lib.epg_simsearch_slices(None, 200, 18, 5, 25, fp, 2, None, None) == -1
    # a window that ends past the genome (76 + 25 * 5 > 200) is refused whatever the pointers are
    x = ctypes.c_void_p(16)
    assert lib.epg_simsearch_slices(x, 200, 18, 5, 25, fp, 2, x, None) == -1
    assert b"outside the 200 rows" in lib.epg_last_error()
    first[1] = -1
    assert lib.epg_simsearch_slices(x, 200, 18, 5, 25, fp, 2, x, None) == -1
