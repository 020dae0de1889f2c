"""GPU: every entry point enqueues its work on the caller's stream and nowhere else, waits for nothing and keeps no pointer to a
host array -- the stream clauses of include/epilogos_amd.h ("enqueues its kernels on `stream`", "retains no pointer after the
call returns", "calls on different devices/streams are independent") and of the eight headers that repeat them.

On the null stream, which every other test hands over, a launch that goes to stream 0 instead of `st`, a read-back that waits for
the device, or a node that reads a host array after the call returned changes nothing.  Here every case of
tests/test_hip_abi_contract.py, and one or two cases of each entry point of the other headers (OTHERS), runs through five steps on
the buffers of the guarded arena (tests/abi_arena.py), held against the case's own oracle and against the bits of its null-stream run:

  (a) baseline       the call on the null stream, outputs against the oracle;
  (b) side stream    the same call on a fresh stream: bit-identical (it also loads code objects and sets kernel attributes before
                     anything is captured);
  (c) capture        workspace and outputs refilled with random bytes, accumulators with random starts, EVERY output and workspace
                     frozen; the call is recorded into a graph on the side stream (torch.cuda.graph, global error mode: a
                     synchronisation, a blocking copy, a default-stream operation or an allocation fails the capture).  Recorded work
                     does not execute: a byte that has changed after the capture went through another stream or ran eagerly;
  (d) first replay   the outputs pass the oracle and equal (a) bit for bit, accumulators = start + what one call adds;
  (e) second replay  every host array the call was given (pointer tables, rows, keys, seeds: Spec.keep) is overwritten with 0xFF
                     first, outputs and workspace get other dirt and new starts: the bits of (d).

One graph, one instantiation, two replays per case, on ONE stream: the graphs are chains.  A case whose header promises an error
code runs once on the side stream and must touch nothing.  EXEMPT names the entry points that document a host synchronisation and
so cannot be captured: they get (a) and (b).  test_two_streams_at_once enqueues pairs of cases that share no buffer on two
streams, alternating, without waiting in between.  The last tests drive the runner with stand-in "entry points" written in torch
that break one promise each, and want every one reported at its step.

tests/test_abi_streams_coverage.py (no GPU) checks that every prototype of the nine headers that takes a stream has a case here.

What it found: the reduced contraction of epg_hist_s3 cleared its count array and its "not a state" flag with one hipMemsetAsync of
1.0 to 1.3 MB in three cases.  Recorded into a graph, that memset replayed with a stale 32-bit fill pattern from the second launch
on (the byte count of an earlier copy, not 0), the gated kernels saw a flag that was neither 0 nor 1 and step (e) found nothing
added to `counts`.  csrc/epg_s3_gemm.hip now clears the range with a kernel of its own.  Memsets of up to 258 KB, all the others
these cases reach, replay correctly."""
import ctypes as C
import tempfile
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_hip_abi_contract import CASES, F32, F64, I32, I64, U8, U16, Run, Spec, same, spec_of

pytestmark = pytest.mark.gpu

U32 = np.uint32

# entry points that take a stream and are not captured, by name, with the reason: the header comment of each says that the call
# synchronises (tests/test_abi_streams_coverage.py holds the reason to that)
EXEMPT = {"epg_simsearch_pick": "reads its sweep counters on the host: one stream synchronisation per four sweeps "
                                "(\"Launches and synchronisations\" in epilogos_simsearch_pick.h)"}


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


# ------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------
def handle(stream):
    return C.c_void_p(stream.cuda_stream)


def scribble(host):
    """0xFF over every registered host array: a node that reads one at replay time sees no pointer, row count or seed of the call."""
    for a in host:
        if isinstance(a, torch.Tensor):
            a.view(torch.uint8).fill_(0xFF)
        elif isinstance(a, np.ndarray):
            a.view(U8)[...] = 0xFF
        else:
            C.memset(C.addressof(a), 0xFF, C.sizeof(a))


def _starts(spec, seed):
    rng = np.random.default_rng(seed)
    return {b.name: rng.integers(1, 1 << 20, size=b.payload[1].size).astype(b.payload[0]) for b in spec.bufs if b.kind == "acc"}


def _check_accs(what, spec, got, start, calls=1):
    for b in spec.bufs:
        if b.kind == "acc":
            dt, inc = b.payload
            assert np.array_equal(got[b.name], start[b.name] + calls * inc.astype(dt)), \
                "%s: %r is not start + %d x what the oracle says one call adds" % (what, b.name, calls)


def _less_start(outs, start):
    """The outputs as a call on zeroed accumulators leaves them: what spec.verify holds against the oracle."""
    return {k: v - start[k] if k in start else v for k, v in outs.items()}


def _plain(spec, outs):
    return {k: v for k, v in outs.items() if k not in [b.name for b in spec.bufs if b.kind == "acc"]}


def _forced(spec, abi):
    if spec.force:
        abi.call("epg_test_force", *spec.force)


def _unforced(spec, abi):
    if spec.force:
        abi.call("epg_test_force", spec.force[0], 0)


def stream_case(spec, abi, capture=True, run=None):
    """Steps (a) to (e) of one case; capture=False stops after (b)."""
    run = run or Run(spec, abi)
    pad = "clean" if spec.clean_pad else "const"
    side = torch.cuda.Stream()
    st = handle(side)
    _forced(spec, abi)
    try:
        if spec.error is not None:                                         # the promised code, on the side stream; nothing is touched
            run("refused on a side stream", pad="random", prefill="random", seed=1, stream=st)
            return
        base = run("baseline", pad=pad)                                                                                      # (a)
        spec.verify(base)
        same("side stream", run("side stream", pad=pad, stream=st), base)                                                    # (b)
        if not capture:
            return
        start = _starts(spec, 5)                                                                                             # (c)
        P = run.prepare(pad=pad, prefill="random", acc_start=start, seed=6, freeze=True)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, stream=side):
                code = run.call(P, st)
        except RuntimeError as e:
            raise AssertionError("capture: the call used something a stream capture does not allow: %s %s" % (e, run.message)) from None
        torch.cuda.synchronize()
        assert code == 0, "capture: the call returned %d %s" % (code, run.message)
        run.collect("capture (the graph has not been launched, every output and workspace is frozen)")
        host = list(spec.host)                                             # (alive until they are overwritten)
        run.freeze()
        graph.replay()                                                                                                       # (d)
        torch.cuda.synchronize()
        first = run.collect("first replay")
        try:
            spec.verify(_less_start(first, start))
        except AssertionError as e:
            raise AssertionError("first replay: %s" % e) from None
        same("first replay", _plain(spec, first), base)
        _check_accs("first replay", spec, first, start)
        scribble(host)                                                                                                       # (e)
        start = _starts(spec, 7)
        run.prepare(pad=pad, prefill="random", acc_start=start, seed=8)
        graph.replay()
        torch.cuda.synchronize()
        second = run.collect("second replay")
        same("second replay", _plain(spec, second), _plain(spec, first))
        _check_accs("second replay", spec, second, start)
    finally:
        _unforced(spec, abi)


@pytest.mark.parametrize("entry,builder,args,kw", CASES)
def test_stream_contract(abi, entry, builder, args, kw):
    stream_case(spec_of(abi, entry, builder, args, kw), abi)


# ------------------------------------------------------------------------------------------------------------------------
# the other headers: one or two cases per entry point, on the inputs and the references of each one's own contract test
# ------------------------------------------------------------------------------------------------------------------------
def _ptrs(sp, P, names):
    return sp.keep((C.c_void_p * len(names))(*[P[n] and P[n].value for n in names]))


def o_groups(abi, rng, S, N, R):
    """epg_bin_hist_groups: three groups, one of them empty (tests/test_hip_groups.py: its states, memberships and check)."""
    from oracle import oracle_np as onp
    from tests.test_hip_groups import make_states, menu
    sp = Spec(S)
    groups = [menu(N)[k] for k in ("every_other", "high_two_thirds", "empty")]
    G, ldx = len(groups), (N + 15) // 16 * 16
    x = make_states(rng, R, N, S)
    member = np.zeros(N, dtype=U8)
    for g, cols in enumerate(groups):
        member[cols] |= 1 << g
    member |= 0xF0 & rng.integers(0, 256, size=N).astype(U8)                # bits G .. 7 are ignored
    refs = [onp.bin_hist(x[:, cols], S) if len(cols) else np.zeros((R, S), dtype=I64) for cols in groups]
    sp.mat("X", x, ldx, mis=3)
    sp.inp("member", member, mis=1)
    for g in range(G):
        sp.out("H%d" % g, U16, R * S, align=16)
    sp.acc("counts", I64, np.stack([r.sum(axis=0) for r in refs]).astype(I64))
    sp.call = lambda abi, P, st: abi.call("epg_bin_hist_groups", P["X"], R, N, ldx, S, G, P["member"], _ptrs(sp, P, ["H%d" % g for g in range(G)]),
                                           P["counts"], st)

    def verify(o):
        for g in range(G):
            assert np.array_equal(o["H%d" % g].reshape(R, S).astype(I64), refs[g]), "H of group %d" % g
    sp.verify = verify
    return sp


def o_draws(abi, rng, NA, NB, S, rows):
    """epg_null_dist_draws_parts with K = 3 seeds; the reference is the two-call form of test_draws_equal_the_two_calls."""
    from epilogos_amd import engine
    from tests import test_hip_null_draws_many as dm
    from tests.test_hip_null_draws import KEYS, _hist, _states
    sp = Spec(S)
    n, K, keys = len(rows), len(dm.SEEDS), KEYS[:len(rows)]
    T = dm._tables(S, (NA, NB), S)
    xs = [(_states(rng, r, NA, S), _states(rng, r, NB, S)) for r in rows]
    hs = [(_hist(a, S), _hist(b, S)) for a, b in xs]
    for p, r in enumerate(rows):
        sp.inp("HA%d" % p, hs[p][0], align=16)
        sp.inp("HB%d" % p, hs[p][1], align=16)
        sp.out("out%d" % p, F32, K * r, mis=4)
    sp.inp("TnA", T[NA].cpu().numpy(), mis=4)
    sp.inp("TnB", T[NB].cpu().numpy(), mis=4)

    def call(abi, P, st):
        seeds = sp.keep(np.ascontiguousarray(dm.SEEDS, dtype=np.uint64).copy())
        i64s = lambda v: sp.keep((C.c_int64 * n)(*v))
        abi.call("epg_null_dist_draws_parts", n, _ptrs(sp, P, ["HA%d" % p for p in range(n)]), _ptrs(sp, P, ["HB%d" % p for p in range(n)]), i64s(rows),
                 i64s(keys), None, S, NA, NB, NA, NB, P["TnA"], P["TnB"], seeds.ctypes.data_as(C.c_void_p), K, _ptrs(sp, P, ["out%d" % p for p in range(n)]), st)
    sp.call = call
    want = []

    def verify(o):
        if not want:                                                       # once: the library's two other calls, seed by seed
            HAs, HBs = [dm._dev_hist(a, S) for a, _b in xs], [dm._dev_hist(b, S) for _a, b in xs]
            for seed in dm.SEEDS:
                want.append([dm._bits(w) for w in dm._two_calls(engine, HAs, HBs, S, NA, NB, NA, NB, T, seed, keys)])
        for p, r in enumerate(rows):
            for k in range(K):
                assert np.array_equal(o["out%d" % p].view(U32).reshape(K, r)[k], want[k][p]), "null distances of part %d, seed %d" % (p, k)
    sp.verify = verify
    return sp


def o_exceed(abi, rng, n, R):
    from tests.null_sampler_ref import exceed_inputs, exceed_np
    sp = Spec(18)
    x, d = exceed_inputs(1, n, R=R)
    d = np.where(np.isnan(d), np.float32(0.5), d)
    sp.inp("null", x, mis=4)
    sp.inp("d", d, mis=4)
    sp.acc("exceed", I64, exceed_np(x, d), mis=8)
    sp.ws("ws", abi.call("epg_null_exceed_ws_bytes", n))
    sp.call = lambda abi, P, st: abi.call("epg_null_exceed", P["null"], n, P["d"], R, P["exceed"], P["ws"], sp.nbytes("ws"), st)
    sp.verify = lambda o: None                                             # (the accumulator check is the oracle's)
    return sp


def o_scores_text(abi, rng, rows, S):
    """epgt_scores_parse on a text of `rows` lines, against the general reader (tests/test_hip_scores_text.py, test_memory_contract)."""
    from epilogos_amd import scoresText, similaritySearch_max_mean as mm
    from tests.test_hip_scores_text import _rows
    sp = Spec(18)
    lines = _rows(rng, rows, S, "many")
    text = "".join(lines).encode()[:-1]                                    # no final newline
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "s.txt").write_bytes(text)
        _s, arr, grid = mm.readScores(Path(d) / "s.txt")
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in lines])))[:-1]
    new = np.concatenate(([True], arr[1:, 0] != arr[:-1, 0]))
    sp.inp("text", np.frombuffer(text, dtype=U8), mis=5)
    sp.out("X", I32, rows * S, align=4)
    sp.out("start", I64, rows, align=8)
    sp.out("end", I64, rows, align=8)
    sp.out("chrom_at", I32, rows, align=4)
    sp.ws("ws", abi.call("epgt_scores_ws_bytes", len(text)))
    sp.inout("status", np.array([scoresText.CLEAN, 0x0101010101010101], dtype=I64))
    sp.call = lambda abi, P, st: abi.call("epgt_scores_parse", P["text"], len(text), S + 3, rows, 0, P["X"], P["start"], P["end"], P["chrom_at"], P["ws"],
                                           sp.nbytes("ws"), P["status"], st)

    def verify(o):
        assert o["status"].tolist() == [scoresText.CLEAN, rows]
        assert np.array_equal(o["X"].reshape(rows, S), grid) and np.array_equal(o["start"], arr[:, 1].astype(I64)) and np.array_equal(o["end"], arr[:, 2].astype(I64))
        assert np.array_equal(o["chrom_at"], np.where(new, offsets, -1))
    sp.verify = verify
    return sp


def o_sbl_parse(abi, rng, bins):
    from tests.test_hip_statebyline import make_text, mixed_values, ref_column
    sp = Spec(18)
    text = make_text(mixed_values(rng, bins), final_newline=False)
    want, rows, lo, hi = ref_column(text)
    sp.inp("text", np.frombuffer(text, dtype=U8), mis=7)
    sp.out("col", np.int8, rows, align=16, mis=13)                          # cap == rows: every byte is written
    sp.out("info", I64, 4, align=8)
    sp.ws("ws", abi.call("epg_sbl_ws_bytes", len(text)))
    sp.call = lambda abi, P, st: abi.call("epg_sbl_parse", P["text"], len(text), P["col"], rows, P["info"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert o["info"].tolist() == [rows, lo, hi, -1] and np.array_equal(o["col"], want)
    sp.verify = verify
    return sp


def o_sbl_transpose(abi, rng, R, nb):
    sp = Spec(18)
    pitch, ldx, col0 = (R + 15) // 16 * 16, 16, 5
    cols = rng.integers(0, 18, size=(nb, pitch)).astype(np.int8)
    before = rng.integers(-128, 128, size=(R, ldx)).astype(np.int8)         # the canary: only the named columns may change
    want = before.copy()
    want[:, col0:col0 + nb] = cols[:, :R].T
    sp.inp("cols", cols, align=16)
    sp.inout("X", before, mis=3)
    sp.call = lambda abi, P, st: abi.call("epg_sbl_transpose", P["cols"], nb, pitch, R, P["X"], ldx, col0, st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["X"].reshape(R, ldx), want)
    return sp


def _segments(rng):
    """Two chromosomes of the table, about 50 segments (tests/test_hip_segments.py: its lines and its restatement)."""
    from tests.test_hip_segments import random_runs
    return [("chr1",) + random_runs(rng, 130), ("chr2",) + random_runs(rng, 90)]


def o_seg_parse(abi, rng):
    from epilogos_amd import segments as seg
    from tests.test_hip_segments import TABLE, join, make_lines, ref_parse
    sp = Spec(18)
    chroms = _segments(rng)
    text = join(make_lines(chroms), final_newline=False)
    first, state, runs, (lo, hi) = ref_parse(chroms)
    L = len(first)
    sp.inp("text", np.frombuffer(text, dtype=U8), mis=7)
    sp.inp("names", seg.name_table(TABLE))
    sp.out("first", I32, L, align=16, mis=4)                                # cap == lines: every entry is written
    sp.out("state", np.int8, L, align=16, mis=3)
    sp.out("runs", I64, 3 * len(TABLE), align=8)
    sp.out("info", I64, 4, align=8)
    sp.ws("ws", abi.call("epg_seg_ws_bytes", len(text), len(TABLE)))
    sp.call = lambda abi, P, st: abi.call("epg_seg_parse", P["text"], len(text), P["names"], len(TABLE), 200, P["first"], P["state"], L, P["runs"],
                                           P["info"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert o["info"].tolist() == [L, lo, hi, -1] and np.array_equal(o["runs"].reshape(-1, 3), runs)
        assert np.array_equal(o["first"], first) and np.array_equal(o["state"], state)
    sp.verify = verify
    return sp


def o_seg_expand(abi, rng, c):
    from tests.test_hip_segments import ref_column, ref_parse
    sp = Spec(18)
    chroms = _segments(rng)
    first, state, runs, _range = ref_parse(chroms)
    want = ref_column(*chroms[c][1:])
    sp.inp("first", first, align=4)
    sp.inp("state", state, mis=3)
    sp.inp("runs", runs, align=8)
    sp.out("col", np.int8, len(want), align=16)                             # R == R_c: every byte is written
    sp.call = lambda abi, P, st: abi.call("epg_seg_expand", P["first"], P["state"], P["runs"], c, P["col"], len(want), st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["col"], want)
    return sp


def o_rowscore(abi, rng, R, S):
    from tests import simsearch_pick_ref as ref
    sp = Spec(18)
    x = rng.integers(-300000, 900000, size=(R, S)).astype(I32)
    x[rng.random((R, S)) < 0.3] = 0
    x[0, 0], x[-1, -1] = 2 ** 31 - 1, -2 ** 31
    want = ref.row_scores(x)
    sp.inp("X", x, mis=4)
    sp.out("score", F64, R, mis=8)
    sp.call = lambda abi, P, st: abi.call("epg_simsearch_rowscore", P["X"], R, S, P["score"], st)

    def verify(o):
        assert o["score"].tobytes() == want.tobytes()
    sp.verify = verify
    return sp


def o_rolling_max(abi, rng, n, W):
    from tests import simsearch_pick_ref as ref
    sp = Spec(18)
    v = np.round(rng.normal(size=n), 1)                                    # rounded: equal maxima inside a window are the rule
    v[n // 3:n // 3 + 2 * W] = -1.5
    want = ref.rolling_max(v, W)
    sp.inp("v", v, mis=8)
    sp.out("out", F64, n, mis=8)
    sp.call = lambda abi, P, st: abi.call("epg_simsearch_rolling_max", P["v"], n, W, P["out"], st)

    def verify(o):
        assert np.array_equal(np.isnan(o["out"]), np.isnan(want)) and np.array_equal(o["out"], want, equal_nan=True)
    sp.verify = verify
    return sp


def o_rank(abi, rng, n):
    from tests import simsearch_pick_ref as ref
    sp = Spec(18)
    rmax, rmean, sc = np.round(rng.normal(size=n), 1), rng.integers(-2, 3, size=n) / 8.0, rng.normal(size=n)      # ties in two keys
    want = ref.lexsort_rank(rmax, rmean, sc)
    for name, a in (("rmax", rmax), ("rmean", rmean), ("sc", sc)):
        sp.inp(name, a, mis=8)
    sp.out("rank", U32, n, mis=4)
    sp.ws("ws", abi.call("epg_simsearch_rank_ws_bytes", n))
    sp.call = lambda abi, P, st: abi.call("epg_simsearch_rank", P["rmax"], P["rmean"], P["sc"], n, P["rank"], P["ws"], sp.nbytes("ws"), st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["rank"], want)
    return sp


def o_pick(abi, rng, n, W):
    """epg_simsearch_pick (EXEMPT: steps (a) and (b)).  The entries of `picked` behind n_picked keep what the runner left there,
    the same bytes in both runs."""
    from tests import simsearch_pick_ref as ref
    sp = Spec(18)
    rank = ref.lexsort_rank(np.round(rng.normal(size=n), 1), rng.normal(size=n), rng.normal(size=n))
    want = ref.pick(rank, W, n)
    launches = C.c_int32(0)
    sp.inp("rank", rank.astype(U32), mis=4)
    sp.out("picked", I64, -(-n // W), mis=8)
    sp.out("n_picked", I64, 1, mis=8)
    sp.ws("ws", abi.call("epg_simsearch_pick_ws_bytes", n, W))
    sp.call = lambda abi, P, st: abi.call("epg_simsearch_pick", P["rank"], n, W, n, P["picked"], P["n_picked"], C.byref(launches), P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        k = int(o["n_picked"][0])
        assert k == len(want) and np.array_equal(o["picked"][:k], want) and launches.value >= 1
    sp.verify = verify
    return sp


def o_census(abi, rng, R, N, S):
    from tests.test_hip_census import NONE, make_bytes, reference
    sp = Spec(S)
    x = make_bytes(rng, R, N, N, S)
    census, other, first_bad = reference(x, S)
    sp.mat("X", x.view(np.int8), (N + 15) // 16 * 16)
    sp.acc("census", I64, census)
    sp.acc("other", I64, other)
    sp.inout("first_bad", np.array([NONE], dtype=I64))
    sp.call = lambda abi, P, st: abi.call("epg_state_census", P["X"], R, N, (N + 15) // 16 * 16, S, P["census"], P["other"], P["first_bad"], st)

    def verify(o):
        assert int(o["first_bad"][0]) == first_bad
    sp.verify = verify
    return sp


def o_concordance(abi, rng, R, N, S, ldx, mis=0):
    """epg_concordance: (333, 70, 18) takes the plane kernels, (20, 33, 18) the byte kernel (tests/test_hip_concordance.py)."""
    from tests.test_concordance_host import restatement
    from tests.test_hip_concordance import make_states
    sp = Spec(S)
    x = make_states(R, N, S, seed=R + N)
    wa, wb = restatement(x, S)
    sp.mat("X", x.view(np.int8), ldx, mis)
    sp.acc("agree", I64, wa)
    sp.acc("both", I64, wb)
    sp.ws("ws", abi.call("epg_concordance_ws_bytes", R, N, S))
    sp.call = lambda abi, P, st: abi.call("epg_concordance", P["X"], R, N, ldx, S, P["agree"], P["both"], P["ws"], sp.nbytes("ws"), st)
    sp.verify = lambda o: None                                             # (both outputs accumulate: the accumulator check is the oracle's)
    return sp


OTHERS = []


def other(entry, builder, *args, **kw):
    ident = "%s-%s" % (entry.split("_", 1)[1], "-".join([str(a).replace(" ", "") for a in args] + ["%s=%s" % (k, v) for k, v in kw.items()]))
    OTHERS.append(pytest.param(entry, builder, args, kw, id=ident.rstrip("-")))


other("epg_bin_hist_groups", o_groups, 18, 70, 333)
other("epg_null_dist_draws_parts", o_draws, 17, 16, 18, (130, 71))          # DRAW_CASES[0], two parts, three seeds
other("epg_null_exceed", o_exceed, 1000, 333)
other("epgt_scores_parse", o_scores_text, 300, 18)
other("epg_sbl_parse", o_sbl_parse, 2000)
other("epg_sbl_transpose", o_sbl_transpose, 2000, 3)
other("epg_seg_parse", o_seg_parse)
other("epg_seg_expand", o_seg_expand, 1)
other("epg_simsearch_rowscore", o_rowscore, 1003, 18)
other("epg_simsearch_rolling_max", o_rolling_max, 1003, 25)
other("epg_simsearch_rank", o_rank, 1003)
other("epg_state_census", o_census, 333, 70, 18)
other("epg_concordance", o_concordance, 333, 70, 18, 80)
other("epg_concordance", o_concordance, 20, 33, 18, 33, mis=1)
other("epg_simsearch_pick", o_pick, 4173, 25)


def captured_entry_points():
    """The entry points with a case that goes through the capture (a case without a promised error code)."""
    return {c.values[0] for c in CASES if "error" not in c.values[3]} | {c.values[0] for c in OTHERS if c.values[0] not in EXEMPT}


@pytest.mark.parametrize("entry,builder,args,kw", OTHERS)
def test_stream_contract_of_the_other_headers(abi, entry, builder, args, kw):
    rng = np.random.default_rng([len(entry)] + [a for a in args if isinstance(a, int)])
    stream_case(builder(abi, rng, *args, **kw), abi, capture=entry not in EXEMPT)


# ------------------------------------------------------------------------------------------------------------------------
# two streams at once
# ------------------------------------------------------------------------------------------------------------------------
def _case_of(abi, entry, args, kw):
    for c in CASES:
        if c.values[0] == entry and c.values[2] == args and c.values[3] == kw:
            return spec_of(abi, *c.values)
    raise KeyError("no case %s %r %r in tests/test_hip_abi_contract.py" % (entry, args, kw))


# pairs of cases that share no buffer, chosen for state two calls could share inside the library
PAIRS = [
    # a dynamic-LDS attribute and a memset  |  the count kernels' persistent grid
    (("epg_hist_s3", (18, 5, 700), dict(pitch="pad", mis=0, force=None)), ("epg_bin_hist", ("epg_bin_hist", 18, 833, 2049), dict(pitch="pad"))),
    # the radix sort's temporary storage inside the caller's workspace  |  a memset and three launches
    (("epg_simsearch", (18, 25, 300, 4, 1024), {}), ("epg_score_s3", (18, 5, 100), dict(pitch="pad", mis=0, force=None))),
    # the null draw and the paired score pass: the two the backend overlaps
    (("epg_null_hist_from_binhist", (18, 70, 53, [257]), dict(force=None)),
     ("epg_pair_scores_s1_parts", (18, 70, 53, 70, 53, [130, 0, 71]), dict(parts=True, qstate=3, alias=True))),
]
ROUNDS = 8


@pytest.mark.parametrize("a,b", PAIRS, ids=["%s+%s" % (a[0][4:], b[0][4:]) for a, b in PAIRS])
def test_two_streams_at_once(abi, a, b):
    """A on one side stream, B on another, alternating, ROUNDS times, the host never waiting in between: both end with the bits of
    their solo runs and ROUNDS increments in their accumulators.  Whether the device overlaps them is not asserted: either
    schedule must give these bits."""
    specs = [_case_of(abi, *a), _case_of(abi, *b)]
    assert all(sp.force is None and sp.error is None for sp in specs)
    runs = [Run(sp, abi) for sp in specs]
    pads = ["clean" if sp.clean_pad else "const" for sp in specs]
    solo = []
    for sp, run, pad in zip(specs, runs, pads):
        solo.append(run("solo", pad=pad))
        sp.verify(solo[-1])
    starts = [_starts(sp, 21 + i) for i, sp in enumerate(specs)]
    Ps = [run.prepare(pad=pad, prefill="random", acc_start=start, seed=22 + i) for i, (run, pad, start) in enumerate(zip(runs, pads, starts))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()                                               # the buffers are filled; from here on nobody waits
    codes = []
    for _round in range(ROUNDS):
        for run, P, s in zip(runs, Ps, streams):
            codes.append(run.call(P, handle(s)))
    torch.cuda.synchronize()
    assert not any(codes), "a call returned an error: %r" % codes
    for sp, run, base, start, name in zip(specs, runs, solo, starts, "AB"):
        got = run.collect("two streams, call %s" % name)
        same("two streams, call %s" % name, _plain(sp, got), _plain(sp, base))
        _check_accs("two streams, call %s" % name, sp, got, start, calls=ROUNDS)


# ------------------------------------------------------------------------------------------------------------------------
# the runner can fail: stand-in "entry points" in torch that break one promise each
# ------------------------------------------------------------------------------------------------------------------------
def _torch_stream(st):
    return torch.cuda.ExternalStream(st.value) if st.value else torch.cuda.default_stream()


def standin(fault):
    """A Spec whose "entry point" is torch code on the arena's own views: o = a + 1 (uint8) and a workspace that is filled, all on
    the handed stream -- unless `fault` says otherwise:
      "other stream"   the output is filled through a stream of the stand-in's own;
      "nothing"        under a capture the output's kernel is not enqueued at all;
      "host pointer"   the output is copied from a pinned host array that the call registered: a copy node that reads it again
                       at every replay."""
    n = 1000
    sp = Spec(18)
    a = np.random.default_rng(3).integers(0, 250, size=n).astype(U8)
    sp.inp("a", a, mis=3)
    sp.out("o", U8, n, mis=1)
    sp.ws("w", 64)
    run = Run(sp, _NoLibrary)
    own = torch.cuda.Stream()
    pinned = torch.empty(n, dtype=torch.uint8).pin_memory()
    src, dst, ws = run.arena.bytes("a"), run.arena.bytes("o"), run.arena.bytes("w")

    def call(_abi, P, st):
        assert P["a"].value == run.arena.addr("a") and P["o"].value == run.arena.addr("o")
        with torch.cuda.stream(_torch_stream(st)):
            ws.fill_(3)
            if fault == "host pointer":
                pinned.copy_(torch.from_numpy(a + 1))
                dst.copy_(sp.keep(pinned), non_blocking=True)
            elif fault is None or (fault == "nothing" and not torch.cuda.is_current_stream_capturing()):
                torch.add(src, 1, out=dst)
        if fault == "other stream":
            with torch.cuda.stream(own):
                torch.add(src, 1, out=dst)
    sp.call = call
    sp.verify = lambda o: np.testing.assert_array_equal(o["o"], a + 1)
    return sp, run


class _NoLibrary:
    """What the runner asks of the binding, for a Spec without a library call and without a switch."""
    class EpilogosHipError(Exception):
        code = -3


def _run_standin(fault):
    sp, run = standin(fault)
    stream_case(sp, _NoLibrary, run=run)


def test_a_stand_in_that_keeps_every_promise_passes():
    _run_standin(None)


def test_a_launch_on_another_stream_is_reported_at_the_capture():
    with pytest.raises(AssertionError, match=r"^capture .*buffer 'o' was written although the call was told not to produce it"):
        _run_standin("other stream")


def test_a_call_that_enqueues_nothing_is_reported_at_the_first_replay():
    with pytest.raises(AssertionError, match=r"^first replay: "):
        _run_standin("nothing")


def test_a_retained_host_pointer_is_reported_at_the_second_replay():
    with pytest.raises(AssertionError, match=r"^second replay: output 'o' differs"):
        _run_standin("host pointer")
