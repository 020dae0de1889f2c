"""GPU: ChromHMM segment files -> lines, runs and columns (csrc/epg_segments.hip), bit for bit against a numpy restatement written
here: the first bins are a cumulative sum of the run lengths, a column is np.repeat over its runs.  Integers only: no tolerance
anywhere.

Every kernel call runs in a guarded arena (tests/abi_arena.py): buffers sized exactly, guards checked after each call, texts at
misaligned addresses.  The byte and bin boundaries the cases aim at come from the library (epg_seg_constant), not from a copy of
its constants.  A text holds three chromosomes of the table wherever the shape allows it."""
import numpy as np
import pytest

from epilogos_amd import _abi, segments as seg
from tests.abi_arena import Arena

pytestmark = pytest.mark.gpu

TABLE = ["chr1", "chr2", "chrX"]
LABELS = ("%d", "E%d", "U%d", "%d_TssFlnk")


def const(which):
    return int(_abi.load().epg_seg_constant(which))


def TB():
    return const(0)


def BB():
    return const(1)


def TILE():
    return const(2)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------

def make_lines(chroms, W=200, labels=LABELS):
    """chroms: [(name, run lengths in bins, states 1..127)] -> the lines as [chrom, start, end, label] of byte strings."""
    out = []
    for name, lengths, states in chroms:
        ends = np.cumsum(np.asarray(lengths, dtype=np.int64))
        starts = ends - lengths
        for s, e, v in zip(starts.tolist(), ends.tolist(), np.asarray(states).tolist()):
            out.append([name.encode(), b"%d" % (s * W), b"%d" % (e * W), (labels[len(out) % len(labels)] % v).encode()])
    return out


def join(lines, final_newline=True):
    text = b"".join(b"\t".join(l) + b"\n" for l in lines)
    return text if final_newline or not text else text[:-1]


def ref_parse(chroms, table=TABLE):
    """-> (first int32 [lines], state int8 [lines], runs int64 [len(table), 3], (lo, hi) over the table's chromosomes)."""
    first, state, runs, l, lo, hi = [], [], np.zeros((len(table), 3), dtype=np.int64), 0, 128, 0
    for name, lengths, states in chroms:
        lengths, states = np.asarray(lengths, dtype=np.int64), np.asarray(states, dtype=np.int64)
        first.append(np.cumsum(lengths) - lengths)
        state.append(states - 1)
        if name in table:
            runs[table.index(name)] = (l, len(lengths), lengths.sum())
            lo, hi = min(lo, int(states.min())), max(hi, int(states.max()))
        l += len(lengths)
    if not l:
        return np.zeros(0, np.int32), np.zeros(0, np.int8), runs, (0, 0)
    return np.concatenate(first).astype(np.int32), np.concatenate(state).astype(np.int8), runs, (lo, hi)


def ref_column(lengths, states):
    return np.repeat((np.asarray(states) - 1).astype(np.int8), np.asarray(lengths, dtype=np.int64))


def random_runs(rng, R, mean=6.0, top=127):
    """Run lengths that sum to R (a fifth of them single bins, the rest geometric) and a state 1..top for each."""
    lengths = []
    left = R
    while left > 0:
        n = 1 if rng.random() < 0.2 else int(rng.geometric(1.0 / mean))
        n = min(n, left)
        lengths.append(n)
        left -= n
    return np.array(lengths, dtype=np.int64), rng.integers(1, top + 1, size=len(lengths))


# ---- one call in a guarded arena ------------------------------------------------------------------------------------------

def parse_call(text, table=TABLE, W=200, cap=None, prefill="random", text_mis=0, seed=0):
    """One epg_seg_parse.  -> dict(first, state, runs, info as left by the call; first0, state0: what the outputs held before)."""
    import torch
    lib = _abi.load()
    rng = np.random.default_rng(seed)
    n = len(text)
    lines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    if cap is None:
        cap = lines
    wsb = lib.epg_seg_ws_bytes(n, len(table))
    ar = Arena("cuda", guard_byte=1)
    ar.add("text", n, role="in", misalign=text_mis)
    ar.add("names", 80 * len(table), role="in")
    ar.add("first", 4 * cap, role="out", align=16, misalign=4 * (seed % 4))
    ar.add("state", cap, role="out", align=16, misalign=(5 * seed + 3) % 16)
    ar.add("runs", 24 * len(table), role="out", align=8)
    ar.add("info", 32, role="out", align=8)
    ar.add("ws", wsb, role="ws", align=16)
    ar.build()
    ar.write("text", np.frombuffer(text, dtype=np.uint8))
    ar.write("names", seg.name_table(table))
    for name in ("first", "state", "runs", "info", "ws"):
        ar.fill(name, prefill, rng)
    before = {"first0": ar.read("first", np.int32), "state0": ar.read("state", np.int8)}
    ar.snapshot()
    _abi.call("epg_seg_parse", ar.ptr("text"), n, ar.ptr("names"), len(table), W, ar.ptr("first") if cap else None,
              ar.ptr("state") if cap else None, cap, ar.ptr("runs"), ar.ptr("info"), ar.ptr("ws"), wsb, None)
    torch.cuda.synchronize()
    ar.check()                                                   # guards intact, the text and the table unchanged
    return dict(before, first=ar.read("first", np.int32), state=ar.read("state", np.int8),
                runs=ar.read("runs", np.int64).reshape(len(table), 3), info=ar.read("info", np.int64))


def expand_call(first, state, runs, c, R, seed=0):
    """One epg_seg_expand into a column of exactly R bytes.  -> (col after, col before)."""
    import torch
    rng = np.random.default_rng(seed)
    ar = Arena("cuda", guard_byte=1)
    ar.add("first", 4 * len(first), role="in", align=4)
    ar.add("state", len(state), role="in", misalign=seed % 7)
    ar.add("runs", runs.size * 8, role="in", align=8)
    ar.add("col", R, role="out", align=16)
    ar.build()
    ar.write("first", first)
    ar.write("state", state)
    ar.write("runs", runs)
    ar.fill("col", "random", rng)
    before = ar.read("col", np.int8)
    ar.snapshot()
    _abi.call("epg_seg_expand", ar.ptr("first"), ar.ptr("state"), ar.ptr("runs"), c, ar.ptr("col"), R, None)
    torch.cuda.synchronize()
    ar.check()
    return ar.read("col", np.int8), before


def check_good(chroms, table=TABLE, W=200, labels=LABELS, final_newline=True, text=None, **kw):
    """Parse and expand every chromosome of the table against the restatement."""
    text = join(make_lines(chroms, W, labels), final_newline) if text is None else text
    first, state, runs, (lo, hi) = ref_parse(chroms, table)
    got = parse_call(text, table, W, **kw)
    assert got["info"].tolist() == [len(first), lo, hi, -1], (got["info"].tolist(), [len(first), lo, hi, -1])
    assert np.array_equal(got["first"], first) and np.array_equal(got["state"], state)
    assert np.array_equal(got["runs"], runs), (got["runs"].tolist(), runs.tolist())
    for name, lengths, states in chroms:
        if name in table:
            c, R = table.index(name), int(np.sum(lengths))
            col, _before = expand_call(got["first"], got["state"], got["runs"], c, R, seed=c)
            assert np.array_equal(col, ref_column(lengths, states)), (name, R)
    return got


def three(rng, sizes, **kw):
    return [(name,) + random_runs(rng, R, **kw) for name, R in zip(TABLE, sizes)]


# ---- sizes and run shapes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1, 15, 16), (17, 255, 256), (257, 4097, 1)])
def test_parse_and_expand_sizes(sizes):
    rng = np.random.default_rng(sum(sizes))
    chroms = three(rng, sizes)
    for k, prefill in enumerate((0x00, 0xFF, "random")):
        check_good(chroms, prefill=prefill, text_mis=(5 * k + 3) % 16, seed=k, final_newline=k != 1)


def test_every_run_one_bin_long_and_one_segment_per_chromosome():
    rng = np.random.default_rng(1)
    R = TILE() + 257                                             # the most lines a column can have: two tiles of them
    ones = [(name, np.ones(R - k, dtype=np.int64), rng.integers(1, 128, size=R - k)) for k, name in enumerate(TABLE)]
    check_good(ones, text_mis=1)
    single = [(name, np.array([R]), np.array([v])) for name, R, v in zip(TABLE, (1, 2 * TILE() + 17, 100000), (127, 100, 1))]
    check_good(single, text_mis=2)


def test_run_boundaries_around_the_threads_and_the_tiles_bins():
    T = TILE()
    rng = np.random.default_rng(2)
    chroms = []
    for k, name in enumerate(TABLE):                             # a run ends at 16 m - 1, 16 m and 16 m + 1, and at the tile's bins +- 1
        cuts = sorted({16 * m + d for m in (1, 2, 5, T // 16 - 1) for d in (-1, 0, 1)} | {T - 1 + k, T + k, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 40})
        lengths = np.diff([0] + cuts)
        chroms.append((name, lengths, rng.integers(100, 128, size=len(lengths))))             # states 100 .. 127
    check_good(chroms)
    one_cut = [(name, np.array([T - 1 + k, 3]), np.array([5, 9])) for k, name in enumerate(TABLE)]
    check_good(one_cut, text_mis=7)


def test_a_run_of_100000_bins_next_to_runs_of_one():
    rng = np.random.default_rng(3)
    chroms = []
    for k, name in enumerate(TABLE):
        lengths = np.concatenate([np.ones(40 + k, dtype=np.int64), [100000], np.ones(23, dtype=np.int64), [100000 + k], [1]])
        chroms.append((name, lengths, rng.integers(1, 128, size=len(lengths))))
    check_good(chroms, text_mis=9)


def test_labels_and_states():
    rng = np.random.default_rng(4)
    for labels in (("%d",), ("E%d",), ("U%d",), ("%d_TssFlnk",), ("z%d_a b/c_9",), LABELS):
        chroms = [(name, np.ones(28, dtype=np.int64) * (k + 1), np.arange(100, 128)) for k, name in enumerate(TABLE)]
        check_good(chroms, labels=labels)
    got = check_good([("chr2", [3, 4], [1, 9]), ("chr1", [1], [7])])
    assert got["runs"].tolist() == [[2, 1, 1], [0, 2, 7], [0, 0, 0]]                  # chrX absent; the table's order, not the text's
    check_good(three(rng, (50, 60, 70), top=18))


@pytest.mark.parametrize("W", [200, 20, 100000000])
def test_bin_widths_and_nine_and_ten_digit_coordinates(W):
    rng = np.random.default_rng(W)
    sizes = (60, 99, 98) if W == 100000000 else (5000000 if W == 200 else 700, 300, 45)       # up to 9 900 000 000 and 1 000 000 000
    chroms = three(rng, sizes, mean=2.0 if W == 100000000 else 40000.0 if W == 200 else 6.0)
    text = join(make_lines(chroms, W))
    if W != 20:
        assert max(len(l.split(b"\t")[2]) for l in text.split(b"\n")[:-1]) == 10
        assert any(len(l.split(b"\t")[1]) == 9 for l in text.split(b"\n")[:-1])
    check_good(chroms, W=W, text_mis=3)


def test_chromosomes_outside_the_table_and_a_name_of_79_bytes():
    rng = np.random.default_rng(5)
    long_name = "chrUn_" + "k" * 73
    table = ["chr1", long_name, "chrX"]
    assert len(long_name) == 79
    other = lambda name, R: (name,) + random_runs(rng, R)
    chroms = [("chrM", np.array([2, 3, 4, 5]), np.array([1, 2, 3, 4])), other("chrUn_1", 400), ("chr1",) + random_runs(rng, 600), other("chr10", 7),
              (long_name,) + random_runs(rng, 300), other(long_name[:-1], 9), other("chr", 2), ("chrX",) + random_runs(rng, 17), other("chrY", 900)]
    got = check_good(chroms, table=table, text_mis=5)
    assert (got["runs"][:, 1] > 0).all()
    # lines of the others are held to the per-line grammar only: chrM may start anywhere and leave gaps
    lines = make_lines(chroms)
    lines[0][1], lines[2][1] = b"200", b"1200"
    first, state, runs, (lo, hi) = ref_parse(chroms, table)
    got = parse_call(join(lines), table)
    assert got["info"].tolist() == [len(first), lo, hi, -1] and np.array_equal(got["runs"], runs)
    lines[2][3] = b"E0"                                          # ... but to that
    assert parse_call(join(lines), table)["info"][3] == 2


# ---- line starts against the parser's byte boundaries ---------------------------------------------------------------------

def _text_with_line_at(start, chroms, final_newline=True):
    """The lines of `chroms` behind one line of a chromosome outside the table whose label is padded so that the second line
    starts at byte `start`."""
    head = b"chrPad\t0\t200\t1_"
    assert start > len(head)
    text = head + b"p" * (start - len(head) - 1) + b"\n" + join(make_lines(chroms), final_newline)
    assert text[start - 1:start] == b"\n" and text[start:start + 4] == b"chr1"
    return text


def _behind_pad(chroms):
    return [("chrPad", [1], [1])] + chroms


@pytest.mark.parametrize("boundary", ["thread", "block", "block2"])
def test_line_starts_on_the_parsers_byte_boundaries(boundary):
    rng = np.random.default_rng(6)
    b = {"thread": 5 * TB(), "block": BB(), "block2": 2 * BB()}[boundary]
    chroms = three(rng, (300, 40, 500))
    for phase in (-1, 0, 1):
        text = _text_with_line_at(b + phase, chroms)
        check_good(_behind_pad(chroms), text=text, text_mis=phase % 16)
        check_good(_behind_pad(chroms), text=text[:-1])


@pytest.mark.parametrize("final_newline", [True, False])
@pytest.mark.parametrize("boundary", ["thread", "block"])
def test_text_that_ends_on_a_boundary(boundary, final_newline):
    """The last line's (real or virtual) newline is the last byte before, or the first byte behind, a boundary."""
    rng = np.random.default_rng(7)
    b = {"thread": 40 * TB(), "block": BB()}[boundary]
    chroms = three(rng, (20, 3, 9))
    body = len(join(make_lines(chroms), final_newline))
    for phase in (-1, 0, 1):
        text = _text_with_line_at(b + phase - body, chroms, final_newline)
        assert len(text) == b + phase
        check_good(_behind_pad(chroms), text=text, text_mis=11)


def test_a_line_longer_than_the_staged_text():
    rng = np.random.default_rng(8)
    chroms = three(rng, (300, 40, 500))
    text = _text_with_line_at(5 * BB() + 3, chroms)              # 20 KB in one label: the workgroup reads global memory
    check_good(_behind_pad(chroms), text=text)
    assert parse_call(text.replace(b"ppp\n", b"p\tp\n", 1))["info"][3] == 0          # ... and finds the tab at its far end


# ---- cap, R, empty --------------------------------------------------------------------------------------------------------

def test_cap_below_the_lines_and_R_below_the_rows():
    rng = np.random.default_rng(9)
    chroms = three(rng, (900, 5000, 700))
    first, state, runs, (lo, hi) = ref_parse(chroms)
    text = join(make_lines(chroms))
    L = len(first)
    ends = (runs[:, 0] + runs[:, 1]).tolist()
    for cap in (0, 1, ends[0] - 1, ends[0], ends[1], L - 1, L + 50):
        got = parse_call(text, cap=cap, seed=cap)
        n = min(cap, L)
        assert got["info"].tolist() == [L, lo, hi, -1]
        assert np.array_equal(got["first"][:n], first[:n]) and np.array_equal(got["state"][:n], state[:n])
        assert np.array_equal(got["first"][n:], got["first0"][n:]) and np.array_equal(got["state"][n:], got["state0"][n:])
        want = runs.copy()
        want[np.array(ends) > cap] = 0                           # a run that does not end below cap is reported as absent
        assert np.array_equal(got["runs"], want), cap
    lengths, states = chroms[1][1], chroms[1][2]
    want = ref_column(lengths, states)
    for R in (1, 15, 16, 17, TILE() - 1, TILE(), TILE() + 1, 4999, 5000, 5001, 5016, 5000 + TILE()):
        col, before = expand_call(first, state, runs, 1, R, seed=R)
        n = min(R, 5000)
        assert np.array_equal(col[:n], want[:n]) and np.array_equal(col[n:], before[n:]), R   # bytes >= R_c are not written
    absent = np.zeros_like(runs)
    col, before = expand_call(first, state, absent, 1, 100)
    assert np.array_equal(col, before)


def test_texts_without_lines_or_without_the_tables_chromosomes():
    for text in (b"", b"chrM\t0\t200\tE1\n", b"chrM\t0\t200\tE1"):
        got = parse_call(text, cap=4)
        lines = 1 if text else 0
        assert got["info"].tolist() == [lines, 128 if lines else 0, 0, -1] and not got["runs"].any()
        assert np.array_equal(got["first"][lines:], got["first0"][lines:]) and got["first"][:lines].tolist() == [0] * lines
    got = parse_call(b"\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n\n", cap=16)                    # more lines than a text of the grammar can hold
    assert got["info"][0] == 16 and got["info"][3] == 0 and not got["runs"].any()


# ---- the first line outside the grammar -----------------------------------------------------------------------------------

def _shift(lines, name, k_from, bins, W=200):
    for l in lines[k_from:]:
        if l[0] == name:
            l[1], l[2] = b"%d" % (int(l[1]) + bins * W), b"%d" % (int(l[2]) + bins * W)


def _three_fields(lines, k):
    lines[k] = lines[k][:3]


def _five_fields(lines, k):
    lines[k] = lines[k] + [b"x"]


def _empty(lines, k):
    lines[k] = [b""]


def _label(label):
    def f(lines, k):
        lines[k][3] = label
    return f


def _cr(lines, k):
    lines[k][3] += b"\r"


def _gap(lines, k):
    _shift(lines, lines[k][0], k, 1)


def _overlap(lines, k):
    _shift(lines, lines[k][0], k, -1)


def _end_is_start(lines, k):
    lines[k][2] = lines[k][1]


def _off_grid(lines, k):
    lines[k][1] = b"%d" % (int(lines[k][1]) + 100)


OFFENCES = {"3 fields": _three_fields, "5 fields": _five_fields, "an empty line": _empty, "a carriage return": _cr, "E0": _label(b"E0"),
            "E128": _label(b"E128"), "07": _label(b"07"), "a gap": _gap, "an overlap": _overlap, "end == start": _end_is_start,
            "a start off the grid": _off_grid}


def _offence_lines(rng):
    """About 900 lines (four workgroups of the line kernels): chrM, chr1, chr2, chrX; every line two bins or longer."""
    chroms = [("chrM", np.full(20, 2), rng.integers(1, 19, size=20))] + [
        (name, 2 + rng.integers(0, 9, size=n), rng.integers(1, 19, size=n)) for name, n in zip(TABLE, (350, 300, 250))]
    return make_lines(chroms), chroms


@pytest.mark.parametrize("what", sorted(OFFENCES))
def test_info_names_the_first_line_outside_the_grammar(what):
    rng = np.random.default_rng(len(what))
    for k in (25, 255, 256, 700):                                # inside a run (not its first line), a second offence behind it
        lines, _chroms = _offence_lines(rng)
        total = len(lines)
        OFFENCES[what](lines, k)
        lines[k + 100][3] = b"E0"
        for final_newline in (True, False):
            got = parse_call(join(lines, final_newline), seed=k)
            assert got["info"][0] == total and got["info"][3] == k, (what, k, got["info"].tolist())
    lines, _chroms = _offence_lines(rng)                         # ... and as the text's last line
    k = len(lines) - 1
    if what != "an empty line":                                  # (an empty last line without its newline is no line)
        OFFENCES[what](lines, k)
        for final_newline in (True, False):
            assert parse_call(join(lines, final_newline))["info"][3] == k, what


def test_a_first_start_of_200_and_a_chromosome_in_two_runs():
    rng = np.random.default_rng(11)
    lines, chroms = _offence_lines(rng)
    starts = {l[0]: k for k, l in reversed(list(enumerate(lines)))}
    for name in (b"chr1", b"chrX"):                              # the run's first line starts at 200: that line, and no other
        bad = [list(l) for l in lines]
        _shift(bad, name, 0, 1)
        assert bad[starts[name]][1] == b"200"
        bad[starts[name] + 100][3] = b"E0"
        assert parse_call(join(bad))["info"][3] == starts[name]
    # chr1 in two runs: its last 50 lines moved behind chr2's: the line that starts the second run
    a, b, c = starts[b"chr1"], starts[b"chr2"], starts[b"chrX"]
    moved = [list(l) for l in lines[:b - 50] + lines[b:c] + lines[b - 50:b] + lines[c:]]
    moved[c + 100][3] = b"E0"
    got = parse_call(join(moved))
    assert got["info"][3] == c - 50, got["info"].tolist()
    # ... also when the second run is one that could stand alone (it starts at 0)
    again = lines + make_lines([("chr2", [4, 4], [1, 2])])
    assert parse_call(join(again))["info"][3] == len(lines)
    # a chromosome outside the table may come twice
    twice = lines + make_lines([("chrM", [4, 4], [1, 2])])
    assert parse_call(join(twice))["info"].tolist()[0::3] == [len(lines) + 2, -1]
