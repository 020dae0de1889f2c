"""The live similarity search query on the GPU: epg_simsearch_reduce and epg_simsearch_slices against the host's
reduceGenomeIndices / makeSlice (exact integers, ties the rule) and against the reference's reduced genome and cube
(tests/golden/simsearch.npz); the command `similaritySearch_run -q ... -s ...` in child processes against the lookup from the
reference's simsearch.bed for every golden region and against the numpy restatement on a synthetic genome; one genome-size case."""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from epilogos_amd import similaritySearch_max_mean as mm
from epilogos_amd import similaritySearch_query as sq
from epilogos_amd import similaritySearch_write as wr
from tests import simsearch_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
GOLD = np.load(ROOT / "tests" / "golden" / "simsearch.npz")
CASES = ["s200", "s20"]
BLOCK_SIZES = [1, 2, 5, 10, 15, 20]
STATES = [1, 15, 18, 25, 100, 150]


def _tied_genome(rng, R, S, classes=4):
    """Rows drawn from a few row classes, two of them with equal sums: within a block ties are the rule."""
    base = rng.integers(-50000, 200000, size=(classes, S)).astype(np.int64)
    base[1] = np.roll(base[0], 1)                    # another row, the same sum (the same row when S == 1)
    return base[rng.integers(0, classes, size=R)]


def _upload(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _reduce(X, blockSize):
    """(G_out, kept) of epg_simsearch_reduce as numpy arrays; the outputs sit between guard rows that must stay untouched."""
    import torch
    from epilogos_amd import _abi, engine
    R, S = X.shape
    nb = -(-R // blockSize)
    x = _upload(X)
    g = torch.full((nb + 2, S), -7, dtype=torch.int32, device="cuda")
    kept = torch.full((nb + 2,), -7, dtype=torch.int64, device="cuda")
    _abi.call("epg_simsearch_reduce", engine._ptr(x), R, S, blockSize, ctypes.c_void_p(g.data_ptr() + S * 4),
              ctypes.c_void_p(kept.data_ptr() + 8), engine._stream())
    torch.cuda.synchronize()
    g, kept = g.cpu().numpy(), kept.cpu().numpy()
    assert (g[0] == -7).all() and (g[-1] == -7).all() and kept[0] == -7 and kept[-1] == -7, "wrote outside its outputs"
    return g[1:-1].astype(np.int64), kept[1:-1]


def _slices(X, first, nblk, blockSize, x=None):
    import torch
    from epilogos_amd import _abi, engine
    R, S = X.shape
    x = _upload(X) if x is None else x
    first = np.ascontiguousarray(first, dtype=np.int64)
    q = torch.full((len(first) * nblk + 2, S), -7, dtype=torch.int32, device="cuda")
    _abi.call("epg_simsearch_slices", engine._ptr(x), R, S, blockSize, nblk, first.ctypes.data_as(ctypes.c_void_p), len(first),
              ctypes.c_void_p(q.data_ptr() + S * 4), engine._stream())
    torch.cuda.synchronize()
    q = q.cpu().numpy()
    assert (q[0] == -7).all() and (q[-1] == -7).all(), "wrote outside its output"
    return q[1:-1].reshape(len(first), nblk, S).astype(np.int64)


def _host_slice(X, f, nblk, blockSize):
    windowBins = nblk * blockSize
    return mm.makeSlice(X, f + windowBins // 2, windowBins, blockSize)


@pytest.mark.parametrize("S", STATES)
@pytest.mark.parametrize("blockSize", BLOCK_SIZES)
def test_reduce_matches_host(blockSize, S):
    rng = np.random.default_rng(1000 * blockSize + S)
    for R in sorted({1, blockSize - 1, blockSize, 7 * blockSize + 3, 100003} - {0}):
        X = _tied_genome(rng, R, S)
        want = mm.reduceGenomeIndices(X, blockSize)
        g, kept = _reduce(X, blockSize)
        assert np.array_equal(kept, want), "kept rows, R=%d" % R
        assert np.array_equal(g, X[want]), "reduced genome, R=%d" % R


def test_reduce_ties_take_the_lowest_row_and_sums_are_exact():
    # equal rows sums far beyond int32: 2^31 - 1 in every state, and a row that differs in the last unit only
    S = 18
    X = np.full((40, S), 2 ** 31 - 1, dtype=np.int64)
    X[7, 3] -= 1
    X[10:20] = -(2 ** 31)
    X[15, 0] += 1
    want = mm.reduceGenomeIndices(X, 10)
    assert list(want) == [0, 15, 20, 30]
    g, kept = _reduce(X, 10)
    assert np.array_equal(kept, want) and np.array_equal(g, X[want])


@pytest.mark.parametrize("S,blockSize", [(1000, 20), (3501, 5)])
def test_reduce_rows_too_long_for_lds(S, blockSize):
    """A block of rows beyond the LDS tile takes the unstaged form: same results."""
    rng = np.random.default_rng(S)
    X = _tied_genome(rng, 6 * blockSize + 2, S)
    want = mm.reduceGenomeIndices(X, blockSize)
    g, kept = _reduce(X, blockSize)
    assert np.array_equal(kept, want) and np.array_equal(g, X[want])
    first = np.array([0, 3, blockSize + 1, X.shape[0] - 4 * blockSize])
    q = _slices(X, first, 4, blockSize)
    for i, f in enumerate(first):
        assert np.array_equal(q[i], _host_slice(X, int(f), 4, blockSize))


@pytest.mark.parametrize("case", CASES)
def test_reduce_and_slices_match_reference(tmp_path, case):
    from epilogos_amd import similaritySearch_run as run
    sp = tmp_path / "scores.txt"
    sp.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    windowBP, windowBins, blockSize = run.windowParameters(sp, int(GOLD[case + "_windowBP"]))
    _s, inputArr, X = mm.readScores(sp)
    g, _kept = _reduce(X, blockSize)
    assert np.array_equal(g, np.rint(GOLD[case + "_reduced_genome"] * 1e5).astype(np.int64))
    table = sq.chromosomeTable(inputArr[:, 0], inputArr[:, 1], inputArr[:, 2])
    first = [sq.windowFirstBin(table, str(c), int(s), int(e), windowBP, windowBins) for c, s, e in GOLD[case + "_cube_coords"]]
    q = _slices(X, first, windowBins // blockSize, blockSize)
    assert np.array_equal(q, np.rint(GOLD[case + "_cube_scores"] * 1e5).astype(np.int64))


@pytest.mark.parametrize("S", STATES)
@pytest.mark.parametrize("blockSize", BLOCK_SIZES)
def test_slices_match_host(blockSize, S):
    rng = np.random.default_rng(77 * blockSize + S)
    for nblk in (1, 25, 64):
        span = nblk * blockSize
        R = span + 37
        X = _tied_genome(rng, R, S)
        first = np.concatenate(([0, R - span], rng.integers(0, R - span + 1, size=5)))
        q = _slices(X, first, nblk, blockSize)
        for i, f in enumerate(first):
            assert np.array_equal(q[i], _host_slice(X, int(f), nblk, blockSize)), "window at row %d, %d blocks" % (f, nblk)


def test_slices_more_windows_than_one_launch_takes():
    rng = np.random.default_rng(5)
    X = _tied_genome(rng, 5000, 18)
    first = rng.integers(0, 5000 - 125 + 1, size=600)
    q = _slices(X, first, 25, 5)
    for i in (0, 255, 256, 257, 511, 512, 599):
        assert np.array_equal(q[i], _host_slice(X, int(first[i]), 25, 5))


# ---- the command ----------------------------------------------------------------------------------------------------------

def _cli(args, timeout=600, prelude=""):
    code = prelude + "from epilogos_amd import similaritySearch_run as r; r.cli(%r)" % [str(a) for a in args]
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, capture_output=True, text=True, timeout=timeout)


def _files(d):
    return {p.name: p.read_bytes() for p in Path(d).iterdir()}


@pytest.mark.parametrize("case", CASES)
def test_cli_live_query_equals_the_lookup_for_every_golden_region(tmp_path, case):
    from epilogos_amd import similaritySearch_run as run
    sp = tmp_path / "scores.txt"
    sp.write_bytes(GOLD[case + "_scores_txt"].tobytes())
    text = GOLD[case + "_bed_text"].tobytes()
    bed = tmp_path / "simsearch.bed.gz"
    bed.write_bytes(wr.bgzf_compress(text)[0])
    qf = tmp_path / "regions.bed"
    qf.write_text("".join("\t".join(line.split("\t")[:3]) + "\n" for line in text.decode().splitlines()))
    want = tmp_path / "want"
    want.mkdir()
    run.querySimSearch(str(qf), bed, want)
    assert len(_files(want)) == len(GOLD[case + "_cube_coords"])
    got = tmp_path / "got"
    _cli(["-q", qf, "-s", sp, "-o", got, "-w", int(GOLD[case + "_windowBP"])])
    assert _files(got) == _files(want)


def _synthetic_scores(path, rng, S=18):
    """Two chromosomes of 200-bp bins (12 000 and 8 003), a background class on most rows, 30 planted noisy copies of one window
    of 125 bins on the grid of blocks of 5; returns (coords object [R, 3], genome int64 [R, S], the copies' first rows)."""
    sizes = {"chr1": 12000, "chr2": 8003}
    R = sum(sizes.values())
    base = rng.integers(0, 100000, size=(12, S))
    X = base[np.where(rng.random(R) < 0.97, 0, rng.integers(0, 12, size=R))]
    src = rng.integers(0, 100000, size=(125, S))
    plants = 5 * rng.integers(0, (R - 125) // 5, size=30)
    for a in plants:
        X[a:a + 125] = src + rng.integers(-40, 40, size=src.shape)
    X = X.astype(np.int64)
    coords = np.empty((R, 3), dtype=object)
    lines, r = [], 0
    for c, n in sizes.items():
        for i in range(n):
            coords[r] = (c, 1000 + 200 * i, 1200 + 200 * i)
            lines.append("%s\t%d\t%d\t%s\n" % (c, coords[r, 1], coords[r, 2], "\t".join("%.5f" % (v / 1e5) for v in X[r])))
            r += 1
    Path(path).write_text("".join(lines))
    return coords, X, plants


def test_cli_live_query_off_grid_regions_match_restatement(tmp_path):
    from epilogos_amd import _abi
    rng = np.random.default_rng(31)
    sp = tmp_path / "scores.txt"
    coords, X, plants = _synthetic_scores(sp, rng)
    windowBP, windowBins, blockSize, nblk, n = 25000, 125, 5, 25, 100
    table = sq.chromosomeTable(coords[:, 0], coords[:, 1], coords[:, 2])
    regions = []
    for _ in range(32):
        c = "chr1" if rng.random() < 0.6 else "chr2"
        start = int(rng.integers(0, 200 * len(table[c][1]) + 2000))
        regions.append((c, start, start + int(rng.integers(1, 60000))))
    for a in plants[-8:]:                            # and 8 inside the first bin of a planted copy, one window long
        if coords[a, 0] == coords[a + windowBins - 1, 0]:
            start = int(coords[a, 1]) + int(rng.integers(1, 200))
            regions.append((coords[a, 0], start, start + windowBP))
    qf = tmp_path / "regions.bed"
    qf.write_text("".join("%s\t%d\t%d\n" % r for r in regions))
    G = X[mm.reduceGenomeIndices(X, blockSize)]
    reducedCoords = wr.reduceGenomeCoords(coords, blockSize)
    want = {}
    for c, s, e in regions:
        f = sq.windowFirstBin(table, c, s, e, windowBP, windowBins)
        idx, _mode = ref.pick(ref.distances(G, _host_slice(X, f, nblk, blockSize)), f // blockSize, nblk, n)
        name = "similarity_search_region_%s_%d_%d_recs.bed" % (coords[f, 0], coords[f, 1], coords[f + windowBins - 1, 2])
        want[name] = sq.recsText(idx, reducedCoords, nblk).encode()
    assert len(regions) == 40 and sum(v.count(b"\n") >= 10 for v in want.values()) >= 3    # the planted copies find each other
    a, b, c3 = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    _cli(["-q", qf, "-s", sp, "-o", a])
    assert _files(a) == want
    _cli(["-q", qf, "-s", sp, "-o", b])
    assert _files(b) == _files(a)                                # the same run twice: byte-identical
    Pg, P = len(G), len(G) - nblk + 1
    fixed = _abi.load().epg_simsearch_ws_bytes(Pg, X.shape[1], nblk, 1) - 20 * P
    cap = fixed + 3 * 20 * P + 10 * P                            # batch_rows -> 3
    _cli(["-q", qf, "-s", sp, "-o", c3], prelude="from epilogos_amd import similaritySearch_calc as c; c.WS_CAP_BYTES = %d; "
         "assert c.batch_rows(%d, %d, %d, 40, c.WS_CAP_BYTES) == 3; " % (cap, Pg, X.shape[1], nblk))
    assert _files(c3) == _files(a)


def test_cli_gpus_is_still_refused_with_query(tmp_path):
    p = subprocess.run([sys.executable, "-m", "epilogos_amd.similaritySearch_run", "--gpus", "1", "-q", "chr1:0-25000", "-s", "x",
                        "-o", str(tmp_path / "o")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--gpus applies to -b only: query mode does not use a GPU" in p.stderr


# ---- genome size ----------------------------------------------------------------------------------------------------------

def test_whole_genome_size():
    """15 M bins x 18 states resident on the device: the reduce equals numpy's, 8 regions equal the restatement on the reduced
    genome, and a second run is byte-identical."""
    rng = np.random.default_rng(2027)
    R, S, blockSize, nblk, W = 15_000_003, 18, 5, 25, 125
    base = rng.integers(0, 100000, size=(40, S)).astype(np.int32)
    X = base[np.where(rng.random(R) < 0.97, 0, rng.integers(0, 40, size=R))]
    src = rng.integers(0, 100000, size=(W, S))
    plants = blockSize * rng.integers(0, (R - W) // blockSize, size=300)      # on the block grid: every copy reduces alike
    for a in plants:
        X[a:a + W] = src + rng.integers(-50, 50, size=src.shape)
    X = X.astype(np.int64)
    G = X[mm.reduceGenomeIndices(X, blockSize)]
    state = sq.reduceGenome(X, blockSize)
    assert np.array_equal(state[1].cpu().numpy(), G)
    first = np.concatenate(([plants[-1]], rng.integers(0, R - W + 1, size=6), [R - W]))   # the last copy planted is whole
    q = sq.slices(state, first, nblk, blockSize).cpu().numpy().astype(np.int64)
    idx = sq.search(state, first, nblk, blockSize, 100)
    for i, f in enumerate(first):
        want_q = _host_slice(X, int(f), nblk, blockSize)
        assert np.array_equal(q[i], want_q), "slice of region %d" % i
        want, _mode = ref.pick(ref.distances(G, want_q), int(f) // blockSize, nblk, 100)
        assert np.array_equal(idx[i], want), "indices of region %d" % i
    assert (idx[0] > 0).sum() >= 50                  # the planted copies are found
    assert sq.search(state, first, nblk, blockSize, 100, batch=3).tobytes() == idx.tobytes()
