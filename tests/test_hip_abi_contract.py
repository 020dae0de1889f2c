"""GPU: every kernel reads and writes only what include/epilogos_amd.h names.

Each case of CASES is one call of an entry point, straight through ctypes, on buffers carved out of ONE guarded allocation
(tests/abi_arena.py): every buffer sized exactly, 64 KiB of guard before and behind it, state matrices at the pitches and base
misalignments the header accepts.  The call is repeated under the variations of the header's promises:

  baseline      outputs against the oracle (oracle/oracle_np.py, tests/simsearch_ref.py), with the comparison of the entry
                point's own parity test: integers, float32 tables and text-exact scores bit for bit, float64 KL scores at the
                tolerance that test asserts;
  hostile       row padding (the bytes of a row beyond N) and the guards around a state matrix hold VALID states drawn at
                random, guards of float inputs hold NaN, guards of integer inputs valid states -- twice, drawn differently:
                outputs bit-identical to the baseline.  (Production pads with whatever the allocator hands out.)
  dirty         workspace and every non-accumulating output prefilled with 0x00, 0xFF and random bytes: bit-identical;
  accumulate    `counts` outputs start from random non-zero integers: result = start + oracle, exactly;
  optional      every combination of NULL outputs the header allows: the others bit-identical, the buffer that was NOT handed
                over untouched;
  and in EVERY run: all guard bytes intact, all inputs bit-identical (arena.check()).

The null-draw entry points have no oracle for WHICH groups a seed gives: their reference is the library's own result on the
clean layout (-1 padding, zeroed outputs) plus the properties that do not depend on the stream, and the recorded draws of
tests/golden/null_draws.json where a case is one of them.

Out of reach of guard bands: a READ outside a buffer that changes no result (the clamped 16-byte load of a packed last row's
last chunk, say) -- that needs an address sanitizer.  Streams are tests/test_hip_abi_streams.py's: the same cases on a side stream,
captured into a graph and replayed, and pairs of them on two streams at once.

CAPPED is a second, short list: the same builders on the one-CU grid of epg_test_force(5, 1) (tests/grid_cap.py), with row counts
that give every wave three tiles and more and ragged multi-part layouts.  There a wave carries state from tile to tile -- tiles
fetched one iteration ahead, staged tiles in re-used LDS -- and hostile padding and dirty memory are what shows a prefetch that
reads a neighbour's rows or pad bytes as states, or a store of a stale staged tile.

tests/test_abi_arena.py (no GPU) checks that every entry point of the header with a pointer parameter has a case here."""
import collections
import ctypes as C
import hashlib
import json
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle_np as onp
from tests import simsearch_ref as ssr
from tests.abi_arena import Arena
from tests.grid_cap import FORCE_CUS, count_grid, pair_count_null_waves, pair_fused_waves, tile_rows

pytestmark = pytest.mark.gpu

# entry points without a case, by name, with the reason (anything else without one fails tests/test_abi_arena.py)
EXEMPT = {"epg_last_error": "returns the library's own thread-local message; takes no data pointer",
          "epg_test_force": "a test switch without a data pointer; the cases below use it"}

I16, U16, I32, I64, U64, F32, F64, U8 = np.int16, np.uint16, np.int32, np.int64, np.uint64, np.float32, np.float64, np.uint8
NAN32 = np.array([np.nan], dtype=F32).view(U8)
NAN64 = np.array([np.nan], dtype=F64).view(U8)


# ------------------------------------------------------------------------------------------------------------------------
# a case's buffers
# ------------------------------------------------------------------------------------------------------------------------
# one buffer of a case: kind is "mat" (state matrix; payload = (x, ldx)), "in" / "fin" (integer / float input; payload = the array),
# "inout", "out" (payload = dtype), "acc" (payload = (dtype, what one call adds)) or "ws"
Buf = collections.namedtuple("Buf", "name kind nbytes align mis payload")


class Spec:
    """What one call needs: buffers (state matrices, other inputs, outputs, accumulators, workspaces), the call itself and the
    check of the baseline's outputs."""

    def __init__(self, S):
        self.S = S
        self.bufs = []               # Buf records, in arena order
        self.optional = []           # tuples of output names that may be NULL together
        self.force = None            # (switch, value) of epg_test_force
        self.clean_pad = False       # null draws: the baseline is the clean layout (-1 padding, zeroed outputs)
        self.error = None            # the EPG_ERR_* code the header promises for this shape
        self.call = self.verify = None
        self.host = []               # the HOST arrays the last call handed over (pointer tables, rows, keys ...), see keep()

    def mat(self, name, x, ldx, mis=0):
        """int8 state matrix [R, ldx], exactly R * ldx bytes, base `mis` bytes off a 256-byte boundary."""
        assert ldx >= x.shape[1]
        self.bufs.append(Buf(name, "mat", x.shape[0] * ldx, 256, mis, (np.ascontiguousarray(x, dtype=np.int8), ldx)))

    def inp(self, name, a, mis=0, align=256):
        self.bufs.append(Buf(name, "fin" if a.dtype.kind == "f" else "in", a.nbytes, align, mis, np.ascontiguousarray(a)))

    def inout(self, name, a, mis=0):
        """Read AND written by the call (epg_combine_score_s1's counts): initialised before every run, read back after it."""
        self.bufs.append(Buf(name, "inout", a.nbytes, 256, mis, np.ascontiguousarray(a)))

    def out(self, name, dtype, n, mis=0, align=256):
        self.bufs.append(Buf(name, "out", int(n) * np.dtype(dtype).itemsize, align, mis, np.dtype(dtype)))

    def acc(self, name, dtype, inc, mis=0):
        """An accumulating output; inc = what one call adds, by the oracle."""
        self.bufs.append(Buf(name, "acc", inc.size * np.dtype(dtype).itemsize, 256, mis, (np.dtype(dtype), inc.reshape(-1))))

    def ws(self, name, nbytes, mis=0):
        """A workspace of exactly `nbytes` bytes."""
        self.bufs.append(Buf(name, "ws", int(nbytes), 256, mis, None))

    def nbytes(self, name):
        return [b.nbytes for b in self.bufs if b.name == name][0]

    def keep(self, array):
        """Register a host array that `call` hands to the entry point: it stays alive behind the call, and the stream tests
        overwrite it to show that the library kept no pointer to it.  -> the array."""
        self.host.append(array)
        return array


def ptr_array(P, prefix, n):
    """Host array of the n device pointers P[prefix + "0"] .. (NULL where a part has no such buffer or it is not handed over)."""
    return (C.c_void_p * n)(*[P.get("%s%d" % (prefix, k)) and P["%s%d" % (prefix, k)].value for k in range(n)])


def pitch_of(N, kind):
    """Row pitches of the header's "any ldx >= N is accepted": kind 0 = packed, 1 .. 15 = N + kind, "pad" = the next multiple
    of 16 (engine.alloc_states), "wide" = much wider than the row."""
    return N + kind if isinstance(kind, int) else (N + 15) // 16 * 16 if kind == "pad" else N + 300 + (N & 7)


def states(rng, R, N, S, junk=False, top=None):
    """[R, N] int8 states of an S-state model (top: only states < top occur, so that q has zero cells); junk: a few bytes
    that are not states inside the rows."""
    x = rng.integers(0, top or S, size=(R, N)).astype(np.int8)
    if junk and R * N > 4:
        k = max(1, R * N // 50)
        x.reshape(-1)[rng.integers(0, R * N, size=k)] = -1
        if S < 31:
            x.reshape(-1)[rng.integers(0, R * N, size=k)] = rng.integers(S, 32, size=k).astype(np.int8)
    return x


def hist(x, S):
    return onp.bin_hist(x, S).astype(U16)


def pair_counts(h):
    h = h.astype(I64)
    return h.T @ h - np.diag(h.sum(axis=0))


# ------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Run:
    def __init__(self, spec, abi):
        self.spec, self.abi = spec, abi
        self.arena = Arena("cuda", guard_byte=1)
        for b in spec.bufs:
            self.arena.add(b.name, b.nbytes, role="in" if b.kind in ("mat", "in", "fin") else "ws" if b.kind == "ws" else "out", align=b.align, misalign=b.mis)
        self.arena.build()
        self.message = ""            # of the last call that returned an error code

    def prepare(self, pad="const", prefill=None, acc_start=None, nulls=(), seed=0, freeze=False):
        """Fill every buffer for one call and take the snapshot.  pad: "const" (the guard byte, a valid state), "clean" (-1),
        "random" (valid states, hostile guards too); prefill: byte or "random" for workspaces and plain outputs (None: the guard
        byte); acc_start: name -> start values; nulls: outputs not handed over; freeze: every output and workspace must stay as
        it is (a call that may not execute yet: tests/test_hip_abi_streams.py).  -> name -> pointer, what spec.call takes."""
        spec, ar, S = self.spec, self.arena, self.spec.S
        rng = np.random.default_rng([seed, 12345])
        ar.reset()
        for name, kind, _n, _a, _m, payload in spec.bufs:
            if kind == "mat":
                x, ldx = payload
                full = np.empty((x.shape[0], ldx), dtype=np.int8)
                full[:, :x.shape[1]] = x
                rest = full[:, x.shape[1]:]
                if pad == "random":
                    rest[...] = rng.integers(0, S, size=rest.shape)
                    ar.poison_guards(name, rng.integers(0, S, size=4099).astype(U8))
                else:
                    rest[...] = 1 if pad == "const" else -1                     # "clean": the reference layout of the null draws
                ar.write(name, full)
            elif kind in ("in", "fin", "inout"):
                ar.write(name, payload)
                if pad == "random" and kind != "inout":
                    ar.poison_guards(name, (NAN64 if payload.dtype == F64 else NAN32) if kind == "fin" else rng.integers(0, S, size=4099).astype(U8))
            elif kind == "acc":
                dt, inc = payload
                ar.write(name, np.zeros(inc.size, dtype=dt) if acc_start is None else acc_start[name])
            elif prefill is not None:
                ar.fill(name, prefill, rng)
            elif spec.clean_pad and kind == "out":
                ar.fill(name, 0)
        self.freeze(nulls if spec.error is None and not freeze else [b.name for b in spec.bufs])
        return {b.name: None if b.name in nulls or b.nbytes == 0 else ar.ptr(b.name) for b in spec.bufs}

    def freeze(self, frozen=()):
        """(Re)take the snapshot: arena.check() then wants the guards, the inputs and the buffers of `frozen` unchanged."""
        self.arena.snapshot(frozen=frozen)

    def call(self, P, stream=None):
        """Enqueue the call on `stream` (a handle; None: torch's current stream), without waiting for it.  -> the code it returned."""
        self.spec.host = []                                                   # the host arrays of THIS call (Spec.keep)
        try:
            self.spec.call(self.abi, P, _stream() if stream is None else stream)
            return 0
        except self.abi.EpilogosHipError as e:
            self.message = str(e)
            return e.code

    def collect(self, what, nulls=()):
        """After the work is done: name -> host array of every output that was handed over; guards and inputs checked."""
        ar, outs = self.arena, {}
        for name, kind, _n, _a, _m, payload in self.spec.bufs:
            if name in nulls or kind not in ("out", "acc", "inout"):
                continue
            outs[name] = ar.read(name, payload if kind == "out" else payload[0] if kind == "acc" else payload.dtype)
        try:
            ar.check()
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e)) from None
        return outs

    def __call__(self, what, pad="const", prefill=None, acc_start=None, nulls=(), seed=0, stream=None):
        """One call, waited for and checked (the arguments of prepare()).  -> the outputs, as collect()."""
        P = self.prepare(pad, prefill, acc_start, nulls, seed)
        code = self.call(P, stream)
        torch.cuda.synchronize()
        assert code == (self.spec.error or 0), "%s: the call returned %d" % (what, code)
        return self.collect(what, nulls)


def same(what, got, want):
    for name in got:
        assert np.array_equal(got[name].view(U8), want[name].view(U8)), "%s: output %r differs from the baseline (%d of %d bytes)" % (
            what, name, int((got[name].view(U8) != want[name].view(U8)).sum()), got[name].nbytes)


def run_case(spec, abi):
    run = Run(spec, abi)
    if spec.force:
        abi.call("epg_test_force", *spec.force)
    try:
        if spec.force and spec.force[0] == FORCE_CUS:
            assert abi.call("epg_device_cus") == spec.force[1], "the grid cap is not live"
        if spec.error is not None:                                         # the header promises an error code: nothing is touched
            run("refused", pad="random", prefill="random", seed=1)
            return
        base = run("baseline", pad="clean" if spec.clean_pad else "const")
        spec.verify(base)
        for seed in (1, 2):
            same("hostile padding %d" % seed, run("hostile padding %d" % seed, pad="random", seed=seed, prefill=0 if spec.clean_pad else None), base)
        for fill in (0x00, 0xFF, "random"):
            same("dirty memory %s" % fill, run("dirty memory %s" % fill, prefill=fill, seed=3), base)
        accs = {b.name: b.payload for b in spec.bufs if b.kind == "acc"}
        if accs:
            rng = np.random.default_rng(99)
            start = {n: rng.integers(1, 1 << 20, size=inc.size).astype(dt) for n, (dt, inc) in accs.items()}
            got = run("accumulation", acc_start=start, seed=4)
            for n, (dt, inc) in accs.items():
                assert np.array_equal(got[n], start[n] + inc.astype(dt)), "accumulation: %r is not start + what the oracle says one call adds" % n
            same("accumulation", {k: v for k, v in got.items() if k not in accs}, base)
        for nulls in spec.optional:
            got = run("optional outputs, without %s" % ", ".join(nulls), nulls=nulls, prefill="random", seed=5)
            same("optional outputs, without %s" % ", ".join(nulls), got, base)
    finally:
        if spec.force:
            abi.call("epg_test_force", spec.force[0], 0)


# ------------------------------------------------------------------------------------------------------------------------
# the builders: case parameters -> Spec
# ------------------------------------------------------------------------------------------------------------------------
def b_count(abi, rng, entry, S, N, R, pitch="pad", mis=0, junk=True):
    """epg_bin_hist / epg_hist_s1 / epg_bin_hist_s2 / epg_hist_s2 on one matrix."""
    sp = Spec(S)
    x = states(rng, R, N, S, junk)
    ldx = pitch_of(N, pitch)
    h = hist(x, S)
    sp.mat("X", x, ldx, mis)
    if entry in ("epg_bin_hist", "epg_bin_hist_s2"):
        sp.out("H", U16, R * S, align=16)
    if entry != "epg_hist_s2":
        sp.acc("counts", I64, h.sum(axis=0, dtype=I64), mis=8)
    if entry in ("epg_bin_hist_s2", "epg_hist_s2"):
        sp.acc("counts2", I64, pair_counts(h))
    if entry == "epg_hist_s2":
        sp.ws("ws", abi.call("epg_ws_bytes", 2, R, N, S))
    if entry == "epg_bin_hist":
        sp.optional = [("H",), ("counts",)]
        sp.call = lambda abi, P, st: abi.call(entry, P["X"], R, N, ldx, S, P["H"], P["counts"], st)
    elif entry == "epg_hist_s1":
        sp.call = lambda abi, P, st: abi.call(entry, P["X"], R, N, ldx, S, P["counts"], st)
    elif entry == "epg_bin_hist_s2":
        sp.optional = [("counts",)]
        sp.call = lambda abi, P, st: abi.call(entry, P["X"], R, N, ldx, S, P["H"], P["counts"], P["counts2"], st)
    else:
        sp.call = lambda abi, P, st: abi.call(entry, P["X"], R, N, ldx, S, P["counts2"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        if "H" in o:
            assert np.array_equal(o["H"].reshape(R, S), h), "H differs from the oracle"
        if "counts" in o:
            assert np.array_equal(o["counts"], h.sum(axis=0, dtype=I64)), "state counts differ from the oracle"
        if "counts2" in o:
            assert np.array_equal(o["counts2"].reshape(S, S), onp.expected_s2(x, S)), "pair counts differ from the oracle"
    sp.verify = verify
    return sp


def b_parts(abi, rng, S, shapes):
    """epg_bin_hist_parts: shapes = [(R, N, pitch kind, base misalignment)]."""
    sp = Spec(S)
    n = len(shapes)
    xs = [states(rng, r, nn, S, junk=True) for r, nn, _p, _m in shapes]
    hs = [hist(x, S) for x in xs]
    for k, (x, (r, nn, p, m)) in enumerate(zip(xs, shapes)):
        if r:
            sp.mat("X%d" % k, x, pitch_of(nn, p), m)
            sp.out("H%d" % k, U16, r * S, align=16)
    sp.acc("counts", I64, sum(h.sum(axis=0, dtype=I64) for h in hs))
    live = [k for k in range(n) if shapes[k][0]]
    sp.optional = [("H%d" % live[0],), tuple("H%d" % k for k in live)] + ([("H%d" % live[-1], "H%d" % live[1])] if len(live) > 2 else [])

    def call(abi, P, st):
        arr = lambda pre: sp.keep(ptr_array(P, pre, n))
        Hs = arr("H") if any(P.get("H%d" % k) for k in range(n)) else None                 # (every entry NULL: the array itself is)
        abi.call("epg_bin_hist_parts", n, arr("X"), sp.keep((C.c_int64 * n)(*[s[0] for s in shapes])), sp.keep((C.c_int32 * n)(*[s[1] for s in shapes])),
                 sp.keep((C.c_int64 * n)(*[pitch_of(s[1], s[2]) for s in shapes])), S, Hs, P["counts"], st)
    sp.call = call

    def verify(o):
        for k in live:
            assert np.array_equal(o["H%d" % k].reshape(hs[k].shape), hs[k]), "H of part %d differs from the oracle" % k
        assert np.array_equal(o["counts"], sum(h.sum(axis=0, dtype=I64) for h in hs))
    sp.verify = verify
    return sp


def b_s2_from_hist(abi, rng, S, R, hi, pair=False):
    sp = Spec(S)
    ha = rng.integers(0, hi, size=(R, S)).astype(U16)
    hb = rng.integers(0, hi, size=(R, S)).astype(U16) if pair else np.zeros((R, S), dtype=U16)
    if hi > 4096:
        ha[: R // 2] %= 4096
    want = pair_counts(ha.astype(I64) + hb)
    sp.inp("HA", ha, align=16)
    if pair:
        sp.inp("HB", hb, align=16)
    sp.acc("counts", I64, want, mis=8)
    if pair:
        sp.call = lambda abi, P, st: abi.call("epg_hist_s2_from_binhist_pair", P["HA"], P["HB"], R, S, P["counts"], st)
    else:
        sp.call = lambda abi, P, st: abi.call("epg_hist_s2_from_binhist", P["HA"], R, S, P["counts"], st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["counts"].reshape(S, S), want)
    return sp


def b_hist_s3(abi, rng, S, N, R, pitch="pad", mis=0, use_ws=True, force=None, junk=True):
    sp = Spec(S)
    x = states(rng, R, N, S, junk)
    ldx = pitch_of(N, pitch)
    want = onp.expected_s3(x, S).reshape(-1)
    sp.mat("X", x, ldx, mis)
    sp.acc("counts", I32, want)
    if use_ws:
        sp.ws("ws", abi.call("epg_ws_bytes", 3, R, N, S))                   # (16-byte aligned, as the header asks)
    sp.force = force
    sp.call = lambda abi, P, st: abi.call("epg_hist_s3", P["X"], R, N, ldx, S, P["counts"], P.get("ws"), sp.nbytes("ws") if use_ws else 0, st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["counts"], want)
    return sp


def b_normalise(abi, rng, entry, n, mis=0):
    """The workspace: normalise_impl (csrc/epg_s1.hip) asks for ws_bytes >= 8 -- one int64 total, used above 4096 entries --
    and nothing quotes it; the case hands over exactly 8 bytes."""
    sp = Spec(18)
    dt = I64 if entry.endswith("i64") else I32
    c = rng.integers(0, 1 << 20, size=n).astype(dt)
    c[0] = 7
    sp.inp("C", c, mis=mis)
    sp.out("q", F32, n, mis=4)
    sp.ws("ws", 8, mis=8)
    sp.call = lambda abi, P, st: abi.call(entry, P["C"], n, P["q"], P["ws"], 8, st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["q"], onp.normalise(c))
    return sp


def _score_outs(sp, R, S):
    sp.out("out64", F64, R * S, align=16)
    sp.out("out32", F32, R * S, align=16)
    sp.optional = [("out64",), ("out32",)]


def _close(o, ref, rtol64, atol64, rtol32, atol32):
    if "out64" in o:
        np.testing.assert_allclose(o["out64"].reshape(ref.shape), ref, rtol=rtol64, atol=atol64)
    if "out32" in o:
        np.testing.assert_allclose(o["out32"].reshape(ref.shape), ref.astype(F32), rtol=rtol32, atol=atol32)


def b_score_s1(abi, rng, S, N, R, pitch="pad", mis=0, top=None, from_hist=False):
    """epg_score_s1 / epg_score_s1_from_binhist; tolerances of tests/test_hip_parity.py (_s1_check)."""
    sp = Spec(S)
    x = states(rng, R, N, S, top=top)
    q = onp.normalise(onp.expected_s1(x, S))
    ref = onp.score_s1(x, q, S)
    if from_hist:
        sp.inp("H", hist(x, S), align=16, mis=8)
        sp.ws("ws", abi.call("epg_ws_bytes", 1, 0, N, S))
    else:
        ldx = pitch_of(N, pitch)
        sp.mat("X", x, ldx, mis)
        sp.ws("ws", abi.call("epg_ws_bytes", 1, R, N, S))
    sp.inp("q", q, mis=4)
    _score_outs(sp, R, S)
    if from_hist:
        sp.call = lambda abi, P, st: abi.call("epg_score_s1_from_binhist", P["H"], R, N, S, P["q"], P["out64"], P["out32"], P["ws"], sp.nbytes("ws"), st)
    else:
        sp.call = lambda abi, P, st: abi.call("epg_score_s1", P["X"], R, N, ldx, S, P["q"], P["out64"], P["out32"], P["ws"], sp.nbytes("ws"), st)
    sp.verify = lambda o: _close(o, ref, 1e-11, 1e-15, 2e-7, 0)
    return sp


def b_combine(abi, rng, S, N, R, rezero):
    """epg_combine_score_s1; tolerances of test_combine_score_s1_and_pair_hist_direct."""
    sp = Spec(S)
    x = states(rng, max(R, 40), N, S)
    counts = onp.expected_s1(x, S)
    q = onp.normalise(counts)
    x = x[:R]
    if rezero:
        sp.inout("counts", counts, mis=8)
    else:
        sp.inp("counts", counts, mis=8)
    if R:
        sp.inp("H", hist(x, S), align=16, mis=8)
        _score_outs(sp, R, S)
    sp.out("q", F32, S, mis=4)
    sp.ws("ws", abi.call("epg_ws_bytes", 1, 0, N, S))
    sp.call = lambda abi, P, st: abi.call("epg_combine_score_s1", P["counts"], rezero, P.get("H"), R, N, S, P["q"], P.get("out64"), P.get("out32"),
                                           P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert np.array_equal(o["q"], q)
        if rezero:
            assert not o["counts"].any(), "rezero: the counts are not zero"
        if R:
            _close(o, onp.score_s1(x, q, S), 1e-11, 0, 2e-7, 0)
    sp.verify = verify
    return sp


def b_s1_table(abi, rng, S, N, R):
    from epilogos_amd.scores import s1ScoreTable
    sp = Spec(S)
    x = states(rng, R, N, S)
    q = onp.normalise(onp.expected_s1(x, S))
    t64, t32 = s1ScoreTable(q, N)
    ref = onp.score_s1(x, q, S)
    sp.inp("H", hist(x, S), align=16, mis=8)
    sp.inp("T64", t64, mis=8)
    sp.inp("T32", t32, mis=4)
    _score_outs(sp, R, S)
    sp.optional = [("T64", "out64"), ("T32", "out32")]
    sp.call = lambda abi, P, st: abi.call("epg_score_s1_from_binhist_table", P["H"], R, N, S, P["T64"], P["T32"], P["out64"], P["out32"], st)

    def verify(o):                                                           # the caller's table: the oracle's bits
        assert np.array_equal(o["out64"].reshape(R, S), ref) and np.array_equal(o["out32"].reshape(R, S), ref.astype(F32))
    sp.verify = verify
    return sp


def b_score_s2(abi, rng, S, N, R, pitch="pad", mis=0, top=None, from_hist=False):
    """epg_score_s2 / epg_score_s2_from_binhist; tolerances of tests/test_hip_parity.py (_s2_check)."""
    sp = Spec(S)
    x = states(rng, R, N, S, top=top)
    q = onp.normalise(onp.expected_s2(x, S))
    perms = N * (N - 1)
    ref = onp.score_s2(x, q, S)
    if from_hist:
        sp.inp("H", hist(x, S), align=16)
        sp.ws("ws", abi.call("epg_ws_bytes", 2, 0, N, S))
    else:
        ldx = pitch_of(N, pitch)
        sp.mat("X", x, ldx, mis)
        sp.ws("ws", abi.call("epg_ws_bytes", 2, R, N, S))
    sp.inp("q", q.reshape(-1), mis=4)
    _score_outs(sp, R, S)
    if from_hist:
        sp.call = lambda abi, P, st: abi.call("epg_score_s2_from_binhist", P["H"], R, N, S, perms, P["q"], P["out64"], P["out32"], P["ws"], sp.nbytes("ws"), st)
    else:
        sp.call = lambda abi, P, st: abi.call("epg_score_s2", P["X"], R, N, ldx, S, perms, P["q"], P["out64"], P["out32"], P["ws"], sp.nbytes("ws"), st)
    sp.verify = lambda o: _close(o, ref, 1e-6, 1e-12, 3e-7, 1e-12)
    return sp


def b_score_s3(abi, rng, S, N, R, pitch="pad", mis=0, force=None):
    """epg_score_s3; tolerances of tests/test_hip_s3_null.py."""
    sp = Spec(S)
    x = states(rng, R, N, S)
    q = onp.normalise(onp.expected_s3(x, S))
    ref = onp.score_s3_f64(x, q, S)
    ldx = pitch_of(N, pitch)
    sp.mat("X", x, ldx, mis)
    sp.inp("q", q.reshape(-1), mis=4)
    _score_outs(sp, R, S)
    sp.ws("ws", abi.call("epg_ws_bytes", 3, R, N, S))
    sp.force = force
    sp.call = lambda abi, P, st: abi.call("epg_score_s3", P["X"], R, N, ldx, S, P["q"], P["out64"], P["out32"], P["ws"], sp.nbytes("ws"), st)
    sp.verify = lambda o: _close(o, ref, 1e-6, 1e-9, 1e-6, 1e-9)
    return sp


def _gather(T, h):
    return T[h.astype(I64), np.arange(h.shape[1])[None, :]]


def b_pair_scores(abi, rng, S, NA, NB, ga, gb, rows, parts=False, qstate=None, alias=False, error=None):
    """epg_pair_scores_s1_from_binhist (rows = [R]) / epg_pair_scores_s1_parts; bit for bit against numpy gathers from the
    caller's tables, onp.pair_finish and onp.pair_metrics (test_paired_s1_in_one_pass_equals_the_separate_passes)."""
    from epilogos_amd.scores import s1ScoreTable
    sp = Spec(S)
    n = len(rows)
    q = onp.normalise(rng.integers(1, 1000, size=S))
    tabs = {w: s1ScoreTable(q, w)[1] for w in {NA, NB, ga, gb}}
    sp.inp("TA", tabs[NA], mis=4)
    sp.inp("TB", tabs[NB], mis=4)
    if not alias:
        sp.inp("TnA", tabs[ga], mis=4)
        sp.inp("TnB", tabs[gb], mis=4)
    want = []
    for k, R in enumerate(rows):
        if not R:
            want.append(None)
            continue
        xa, xb = states(rng, R, NA, S), states(rng, R, NB, S)
        if qstate is not None and qstate >= 0:
            xa[::7], xb[::7] = qstate, qstate
            xb[::21] = 0
        hs = [hist(xa, S), hist(xb, S), hist(states(rng, R, ga, S), S), hist(states(rng, R, gb, S), S)]
        for nm, h in zip(("HA", "HB", "HnA", "HnB"), hs):
            sp.inp("%s%d" % (nm, k), h, align=16)
        sp.out("delta%d" % k, F32, R * S, align=16)
        sp.out("null%d" % k, F32, R, mis=4)
        sp.out("dist%d" % k, F32, R, mis=4)
        sp.out("maxdiff%d" % k, I32, R, mis=4)
        if qstate is not None:
            sp.out("mask%d" % k, U8, R, mis=1)
        delta, _ = onp.pair_finish(_gather(tabs[NA], hs[0]), _gather(tabs[NB], hs[1]))
        _, nd = onp.pair_finish(_gather(tabs[ga], hs[2]), _gather(tabs[gb], hs[3]))
        dist, md = onp.pair_metrics(delta, True)
        want.append((delta, nd, dist, md, onp.quiescent_mask(xa, xb, -1 if qstate is None else qstate)))
    live = [k for k in range(n) if rows[k]]
    if qstate is not None:
        sp.optional = [("mask%d" % live[0],), tuple("mask%d" % k for k in live)]
    sp.error = error

    def call(abi, P, st):
        tn = (P["TA"], P["TB"]) if alias else (P["TnA"], P["TnB"])
        if not parts:
            return abi.call("epg_pair_scores_s1_from_binhist", P["HA0"], P["HB0"], P["HnA0"], P["HnB0"], rows[0], S, NA, NB, ga, gb, P["TA"], P["TB"],
                            *tn, P["delta0"], P["null0"], P["dist0"], P["maxdiff0"], st)
        arr = lambda pre: sp.keep(ptr_array(P, pre, n))
        mask = arr("mask") if qstate is not None and any(P.get("mask%d" % k) for k in range(n)) else None
        abi.call("epg_pair_scores_s1_parts", n, arr("HA"), arr("HB"), arr("HnA"), arr("HnB"), sp.keep((C.c_int64 * n)(*rows)), S, NA, NB, ga, gb, P["TA"], P["TB"],
                 *tn, arr("delta"), arr("null"), arr("dist"), arr("maxdiff"), mask, -1 if qstate is None else qstate, st)
    sp.call = call

    def verify(o):
        for k in live:
            delta, nd, dist, md, qm = want[k]
            assert np.array_equal(o["delta%d" % k].reshape(delta.shape), delta), "delta of part %d" % k
            assert np.array_equal(o["null%d" % k], nd), "null distance of part %d" % k
            assert np.array_equal(o["dist%d" % k], dist) and np.array_equal(o["maxdiff%d" % k], md), "STEP 4 inputs of part %d" % k
            if qstate is not None:
                assert np.array_equal(o["mask%d" % k].astype(bool), qm), "quiescence mask of part %d" % k
    sp.verify = verify
    return sp


def b_pair_finish(abi, rng, S, R):
    sp = Spec(S)
    a, b = rng.standard_normal((R, S)).astype(F32), rng.standard_normal((R, S)).astype(F32)
    a[::5] = b[::5]
    sp.inp("a", a, align=16)
    sp.inp("b", b, align=16)
    sp.out("delta", F32, R * S, align=16)
    sp.out("sqdist", F32, R, mis=4)
    sp.optional = [("sqdist",)]
    sp.call = lambda abi, P, st: abi.call("epg_pair_finish", P["a"], P["b"], R, S, P["delta"], P["sqdist"], st)
    d, dist = onp.pair_finish(a, b)

    def verify(o):
        assert np.array_equal(o["delta"].reshape(R, S), d) and np.array_equal(o["sqdist"], dist)
    sp.verify = verify
    return sp


def b_pair_metrics(abi, rng, S, R, roundtrip):
    sp = Spec(S)
    d = (rng.standard_normal((R, S)) * 3).astype(F32)
    d[::4, 1] = d[::4, S - 1]                                                # ties go to the higher state
    if not roundtrip:
        d = onp.text_roundtrip_f5(d)
    sp.inp("delta", d, align=16)
    sp.out("dist", F32, R, mis=4)
    sp.out("maxdiff", I32, R, mis=4)
    sp.call = lambda abi, P, st: abi.call("epg_pair_metrics", P["delta"], R, S, roundtrip, P["dist"], P["maxdiff"], st)
    dist, md = onp.pair_metrics(d, bool(roundtrip))

    def verify(o):
        assert np.array_equal(o["dist"], dist) and np.array_equal(o["maxdiff"], md)
    sp.verify = verify
    return sp


def b_quiescent(abi, rng, S, NA, NB, R, qstate, pa="pad", pb="pad", mis=0, from_hist=False):
    sp = Spec(S)
    xa, xb = states(rng, R, NA, S), states(rng, R, NB, S)
    if qstate >= 0:
        xa[::3], xb[::3] = qstate, qstate
        xa[::9, NA - 1] = (qstate + 1) % S                                   # all but the row's last column
        xb[3::9, 0] = (qstate + 1) % S
    want = onp.quiescent_mask(xa, xb, qstate)
    la, lb = pitch_of(NA, pa), pitch_of(NB, pb)
    if from_hist:
        sp.inp("HA", hist(xa, S), align=16)
        sp.inp("HB", hist(xb, S), align=16)
        sp.call = lambda abi, P, st: abi.call("epg_quiescent_from_binhist", P["HA"], P["HB"], R, S, NA, NB, qstate, P["mask"], st)
    else:
        sp.mat("XA", xa, la, mis)
        sp.mat("XB", xb, lb, (mis * 7) % 16)
        sp.call = lambda abi, P, st: abi.call("epg_quiescent", P["XA"], NA, la, P["XB"], NB, lb, R, qstate, P["mask"], st)
    sp.out("mask", U8, R, mis=1)
    sp.verify = lambda o: np.testing.assert_array_equal(o["mask"].astype(bool), want)
    return sp


def _null_props(what, oa, ob, ha, hb, ga, gb, full):
    """What every null draw satisfies whatever the stream: the two null groups are taken from the row's columns."""
    oa, ob, tot = oa.astype(I64), ob.astype(I64), ha.astype(I64) + hb.astype(I64)
    assert (oa + ob <= tot).all(), "%s: OA + OB exceeds HA + HB in some state" % what
    if full:                                                                # every column holds a state
        assert (oa.sum(axis=1) == ga).all() and (ob.sum(axis=1) == gb).all(), "%s: row sums are not ga / gb" % what


def b_null_hist(abi, rng, S, NA, NB, R, ga, gb, pa="pad", pb="pad", mis=0, error=None):
    """epg_null_hist (the matrix-scanning sampler)."""
    sp = Spec(S)
    xa, xb = states(rng, R, NA, min(S, 31)), states(rng, R, NB, min(S, 31))
    la, lb = pitch_of(NA, pa), pitch_of(NB, pb)
    sp.mat("XA", xa, la, mis)
    sp.mat("XB", xb, lb, (mis * 5) % 16)
    sp.out("HA", U16, R * S)
    sp.out("HB", U16, R * S)
    sp.clean_pad, sp.error = True, error
    sp.call = lambda abi, P, st: abi.call("epg_null_hist", P["XA"], NA, la, P["XB"], NB, lb, R, S, ga, gb, 4242, 1000, P["HA"], P["HB"], st)
    sp.verify = lambda o: _null_props("null_hist", o["HA"].reshape(R, S), o["HB"].reshape(R, S), hist(xa, S), hist(xb, S), ga, gb, True)
    return sp


def _golden_null(key):
    from tests.test_hip_null_draws import FIXTURE
    return json.loads(FIXTURE.read_text())["digests"][key]


def b_null_from_hist(abi, rng, S, NA, NB, rows, ga=None, gb=None, parts=False, force=None, golden=False):
    """epg_null_hist_from_binhist (rows = [R]) / _parts.  golden: the case is one of tests/golden/null_draws.json (inputs by
    tests/test_hip_null_draws.py's generator): its SHA-256 is asserted on top of the properties."""
    from tests import test_hip_null_draws as nd
    sp = Spec(S)
    n = len(rows)
    ga, gb = ga or NA, gb or NB
    seed = nd.SEEDS[0]
    if golden:
        xs = nd._parts(NA, NB, S, tuple(rows))
        keys = nd._keys(rows)
    else:
        xs = [(states(rng, r, NA, S, junk=True), states(rng, r, NB, S)) for r in rows]
        keys = [(k << 40) + 1000 * k for k in range(n)]
    hs = [(hist(a, S), hist(b, S)) for a, b in xs]
    for k, r in enumerate(rows):
        if r:
            sp.inp("HA%d" % k, hs[k][0], align=16)
            sp.inp("HB%d" % k, hs[k][1], align=16)
            sp.out("OA%d" % k, U16, r * S, align=16)
            sp.out("OB%d" % k, U16, r * S, align=16)
    sp.clean_pad, sp.force = True, force

    def call(abi, P, st):
        if not parts:
            return abi.call("epg_null_hist_from_binhist", P["HA0"], P["HB0"], rows[0], S, NA + NB, ga, gb, seed, keys[0], P["OA0"], P["OB0"], st)
        arr = lambda pre: sp.keep(ptr_array(P, pre, n))
        abi.call("epg_null_hist_from_binhist_parts", n, arr("HA"), arr("HB"), sp.keep((C.c_int64 * n)(*rows)), S, NA + NB, ga, gb, seed,
                 sp.keep((C.c_int64 * n)(*keys)), arr("OA"), arr("OB"), st)
    sp.call = call

    def verify(o):
        for k, r in enumerate(rows):
            if r:
                full = bool((hs[k][0].sum(axis=1) == NA).all()) and (ga, gb) == (NA, NB)
                _null_props("part %d" % k, o["OA%d" % k].reshape(r, S), o["OB%d" % k].reshape(r, S), hs[k][0], hs[k][1], ga, gb, full)
                if (ga, gb) == (NA, NB):
                    assert np.array_equal(o["OA%d" % k].astype(I64) + o["OB%d" % k], (hs[k][0].astype(I64) + hs[k][1]).reshape(-1))
        if golden:
            h = hashlib.sha256()
            for pre in ("OA", "OB"):
                for k, r in enumerate(rows):
                    if r:
                        h.update(o["%s%d" % (pre, k)].tobytes())
            assert h.hexdigest() == _golden_null("hist NA=%d NB=%d S=%d rows=%s ga=%d gb=%d force_seq=%d seed=%d" % (
                NA, NB, S, nd._rows_label(rows), ga, gb, 1 if force else 0, seed)), "the draws are not the recorded ones"
    sp.verify = verify
    return sp


def b_pair_count_null(abi, rng, S, NA, NB, rows, pa="pad", pb="pad", mis=0, golden=False, error=None):
    """epg_pair_count_null_parts: histograms and state counts against the oracle, draws as b_null_from_hist."""
    from tests import test_hip_null_draws as nd
    sp = Spec(S)
    n = len(rows)
    seed = nd.SEEDS[0]
    xs = nd._parts(NA, NB, S, tuple(rows)) if golden else [(states(rng, r, NA, S, junk=True), states(rng, r, NB, S)) for r in rows]
    keys = nd._keys(rows) if golden else [(k << 40) + 17 * k for k in range(n)]
    hs = [(hist(a, S), hist(b, S)) for a, b in xs]
    la, lb = pitch_of(NA, pa), pitch_of(NB, pb)
    for k, r in enumerate(rows):
        if r:
            sp.mat("XA%d" % k, xs[k][0], la, mis)
            sp.mat("XB%d" % k, xs[k][1], lb, (mis * 3) % 16)
            for nm in ("HA", "HB", "OA", "OB"):
                sp.out("%s%d" % (nm, k), U16, r * S, align=16)
    total = sum(a.sum(axis=0, dtype=I64) + b.sum(axis=0, dtype=I64) for a, b in hs)
    sp.acc("counts", I64, total, mis=8)
    sp.optional = [("counts",)]
    sp.clean_pad, sp.error = True, error

    def call(abi, P, st):
        arr = lambda pre: sp.keep(ptr_array(P, pre, n))
        i64s = lambda v: sp.keep((C.c_int64 * n)(*v))
        abi.call("epg_pair_count_null_parts", n, arr("XA"), arr("XB"), i64s(rows), NA, NB, i64s([la] * n), i64s([lb] * n),
                 S, arr("HA"), arr("HB"), P["counts"], seed, i64s(keys), arr("OA"), arr("OB"), st)
    sp.call = call

    def verify(o):
        for k, r in enumerate(rows):
            if r:
                assert np.array_equal(o["HA%d" % k].reshape(r, S), hs[k][0]) and np.array_equal(o["HB%d" % k].reshape(r, S), hs[k][1]), "histograms of part %d" % k
                full = bool((hs[k][0].sum(axis=1) == NA).all() and (hs[k][1].sum(axis=1) == NB).all())
                _null_props("part %d" % k, o["OA%d" % k].reshape(r, S), o["OB%d" % k].reshape(r, S), hs[k][0], hs[k][1], NA, NB, full)
                assert np.array_equal(o["OA%d" % k].astype(I64) + o["OB%d" % k], (hs[k][0].astype(I64) + hs[k][1]).reshape(-1))
        assert np.array_equal(o["counts"], total)
        if golden:
            h = hashlib.sha256()
            for pre in ("HA", "HB", "counts", "OA", "OB"):
                for k, r in enumerate(rows if pre != "counts" else [1]):
                    if r:
                        h.update(o[pre if pre == "counts" else "%s%d" % (pre, k)].tobytes())
            assert h.hexdigest() == _golden_null("fused NA=%d NB=%d S=%d rows=%s seed=%d" % (NA, NB, S, nd._rows_label(rows), seed)), \
                "the draws are not the recorded ones"
    sp.verify = verify
    return sp


def b_simsearch(abi, rng, S, W, P_, B, n):
    """epg_simsearch against tests/simsearch_ref.py (exact)."""
    sp = Spec(18)
    Pg = P_ + W - 1
    G = (rng.integers(0, 6, size=(Pg, S)) * 1000).astype(I32)
    starts = rng.integers(0, P_, size=B).astype(I32)
    Q = np.stack([G[s:s + W] for s in starts]).astype(I32)
    Q[B // 2] += (rng.integers(0, 2, size=(W, S)) * 1000).astype(I32)
    bound = int(W * S * 6000 ** 2)
    idx, modes = ssr.search(G.astype(I64), Q.astype(I64), starts, n)
    D = np.stack([ssr.distances(G.astype(I64), Q[r].astype(I64)) for r in range(B)])
    sp.inp("G", G)
    sp.inp("Q", Q)
    sp.inp("self_start", starts, mis=4)
    sp.ws("ws", abi.call("epg_simsearch_ws_bytes", Pg, S, W, B))
    sp.out("idx", I32, B * n, mis=4)
    sp.out("mode", U64, B, mis=8)
    sp.out("dist", U64, B * P_, mis=8)
    sp.optional = [("dist",)]
    sp.call = lambda abi, P, st: abi.call("epg_simsearch", P["G"], Pg, S, W, P["Q"], B, P["self_start"], n, bound, P["ws"], sp.nbytes("ws"), P["idx"],
                                           P["mode"], P["dist"], st)

    def verify(o):
        assert np.array_equal(o["dist"].reshape(B, P_).astype(I64), D), "distances"
        assert np.array_equal(o["mode"].astype(I64), modes), "modes"
        assert np.array_equal(o["idx"].reshape(B, n), idx), "picks"
    sp.verify = verify
    return sp


def _best_rows(X, first, bs, nblk):
    """Per block of bs rows from row `first`: the row with the largest int64 sum, the lowest on ties (a partial last block too)."""
    out = []
    for b in range(nblk):
        lo = first + b * bs
        blk = X[lo:min(lo + bs, len(X))].astype(I64)
        out.append(lo + int(np.argmax(blk.sum(axis=1))))
    return np.array(out, dtype=I64)


def b_reduce(abi, rng, S, R, bs):
    sp = Spec(18)
    X = rng.integers(-3, 4, size=(R, S)).astype(I32) * 1000
    nb = (R + bs - 1) // bs
    kept = _best_rows(X, 0, bs, nb)
    sp.inp("X", X)
    sp.out("G", I32, nb * S, mis=4)
    sp.out("kept", I64, nb, mis=8)
    sp.optional = [("kept",)]
    sp.call = lambda abi, P, st: abi.call("epg_simsearch_reduce", P["X"], R, S, bs, P["G"], P["kept"], st)

    def verify(o):
        assert np.array_equal(o["kept"], kept) and np.array_equal(o["G"].reshape(nb, S), X[kept])
    sp.verify = verify
    return sp


def b_slices(abi, rng, S, R, bs, nblk, B):
    sp = Spec(18)
    X = rng.integers(-3, 4, size=(R, S)).astype(I32) * 1000
    first = rng.integers(0, R - nblk * bs + 1, size=B).astype(I64)
    first[0], first[-1] = R - nblk * bs, 0
    want = np.stack([X[_best_rows(X, int(f), bs, nblk)] for f in first])
    sp.inp("X", X)
    sp.out("Q", I32, B * nblk * S, mis=4)
    sp.call = lambda abi, P, st: abi.call("epg_simsearch_slices", P["X"], R, S, bs, nblk, sp.keep((C.c_int64 * B)(*first.tolist())), B, P["Q"], st)
    sp.verify = lambda o: np.testing.assert_array_equal(o["Q"].reshape(B, nblk, S), want)
    return sp


# ------------------------------------------------------------------------------------------------------------------------
# the table: (id, entry point, builder, arguments).  The shapes sit on either side of the branches the host functions take.
# ------------------------------------------------------------------------------------------------------------------------
CASES = []


def case(entry, builder, *args, **kw):
    ident = "%s-%s" % (entry[4:], "-".join([str(a).replace(" ", "") for a in args] + ["%s=%s" % (k, str(v).replace(" ", "")) for k, v in kw.items()]))
    CASES.append(pytest.param(entry, builder, args, kw, id=ident[:120]))


# -- the count pass: N around the 16-byte chunk, the 128-byte group, the eight-group schedules and the any-width loop; S on the
#    three tuned cores, between them and wide; R around the 32-row super-tile and the 64-bin block; every pitch N .. N + 15,
#    the padded width and a much wider one; bases off the 16-byte boundary (fast_rows(): a pitch under the padded width sends
#    the last rows to the byte-granular kernel)
_NS = (1, 15, 16, 17, 127, 128, 129, 379, 833, 1024, 1025, 4100)
_SS = (15, 18, 25, 7, 20, 31, 40, 100)
_RS = (1, 63, 64, 65, 33, 200, 31)
_PITCH = (0,) + tuple(range(1, 16)) + ("pad", "wide")
# (the three tuned cores meet EVERY N of the list -- all load schedules, 1 .. 8 groups per row and the any-width loop, which N = 1025
#  and 4100 take; the other models take the next larger core's any-width instantiation, or the wide kernel, at every N once or twice)
for _i, (_s, _n) in enumerate([(_s, _n) for _s in (15, 18, 25) for _n in _NS] + [((7, 20, 31, 40, 100)[_k % 5], _NS[_k % 12]) for _k in range(24)]):
    case("epg_bin_hist", b_count, "epg_bin_hist", _s, _n, _RS[_i % 7], pitch=_PITCH[(5 * _i) % 18], mis=(3 * _i) % 16)
for _i in range(24):                                                                       # every N twice more, on the other two entry points
    case("epg_hist_s1", b_count, "epg_hist_s1", _SS[(3 * _i + _i // 12) % 8], _NS[_i % 12], _RS[(_i + 2) % 7], pitch=_PITCH[(7 * _i + 1) % 18], mis=(5 * _i) % 16)
    case("epg_bin_hist_s2", b_count, "epg_bin_hist_s2", (15, 18, 25)[(_i + _i // 12) % 3], _NS[_i % 12], _RS[(_i + 4) % 7], pitch=_PITCH[(11 * _i + 16) % 18],
         mis=(7 * _i) % 16)
case("epg_bin_hist", b_count, "epg_bin_hist", 15, 833, 33, pitch="pad")                    # odd R x odd S: the two-byte last store
case("epg_bin_hist", b_count, "epg_bin_hist", 18, 833, 2049, pitch="pad")                  # several blocks, a partial super-tile
case("epg_bin_hist", b_count, "epg_bin_hist", 25, 379, 4001, pitch=9, mis=2)
case("epg_bin_hist", b_count, "epg_bin_hist", 25, 129, 65, pitch=0, mis=5)                 # packed odd rows, unaligned base
for _i, (_s, _n, _r, _p) in enumerate([(18, 379, 65, "pad"), (15, 17, 1, 3), (25, 1025, 64, 0), (20, 128, 63, "wide"), (40, 129, 33, 7)]):
    case("epg_hist_s1", b_count, "epg_hist_s1", _s, _n, _r, pitch=_p, mis=(7 * _i) % 16)
# (epg_bin_hist_s2: one launch for 15 / 18 / 25 states, N <= 1024, every row on the fast kernel; else two passes)
for _s, _n, _r, _p, _m in [(18, 379, 65, "pad", 0), (15, 1024, 33, "pad", 0), (25, 127, 1, "wide", 9), (18, 1025, 64, "pad", 0), (20, 129, 63, "pad", 0),
                           (18, 129, 95, 0, 3), (15, 17, 31, 3, 0), (18, 833, 700, "pad", 0)]:
    case("epg_bin_hist_s2", b_count, "epg_bin_hist_s2", _s, _n, _r, pitch=_p, mis=_m)
for _s, _n, _r, _p in [(18, 41, 100, "pad"), (15, 129, 33, 0), (31, 16, 65, 5), (40, 20, 20, "pad")]:
    case("epg_hist_s2", b_count, "epg_hist_s2", _s, _n, _r, pitch=_p)
# (parts: widths in different schedule classes, an empty part, packed and unaligned parts, more parts than a launch holds (48))
_PARTS = [(0, 40, "pad", 0), (1, 40, "pad", 0), (95, 379, "pad", 0), (64, 342, 0, 0), (33, 379, 5, 3), (7, 1100, "pad", 0), (129, 833, "wide", 0), (31, 833, 0, 7)]
for _s in (18, 15, 20, 40):
    case("epg_bin_hist_parts", b_parts, _s, _PARTS)
case("epg_bin_hist_parts", b_parts, 18, [(1 + (5 * _k) % 23, 61, ("pad", 0, 2)[_k % 3], _k % 16) for _k in range(60)])
for _s, _r, _hi in [(18, 1000, 834), (5, 129, 4096), (31, 257, 4095), (25, 65, 65536), (40, 33, 70), (30, 1, 70)]:
    case("epg_hist_s2_from_binhist", b_s2_from_hist, _s, _r, _hi)
for _s, _r, _hi in [(18, 1000, 400), (15, 65, 30000), (40, 33, 70)]:
    case("epg_hist_s2_from_binhist_pair", b_s2_from_hist, _s, _r, _hi, pair=True)
# -- S3 counts.  The path each case takes (epg_hist_s3 / hist_s3_gemm; none of these calls has the 262 144 bins from which the
#    library picks the reduced contraction by itself):
#      no switch, workspace     the full matrix-core contraction over all S states
#      (2, 1)                   the same, forced
#      (2, 2), clean rows       the REDUCED contraction over S - 1 states + k_s3_reconstruct.  It needs room for its count array next to
#                               a chunk of the operand: epg_ws_bytes(3, ...) is at least s3_gemm_ws_bytes = fixed part + operand chunk +
#                               g_reduced_bytes for S >= 3, the chunk at least the 16 K bins (or the whole call) the condition asks for
#      (2, 2), junk in the rows both are enqueued; the "not a state" byte found by the transpose switches, on the device, to the full one
#      (3, 1), or no workspace, or S = 31: the LDS-counter kernel;  S = 40: the wide kernel
#    N not a multiple of 4 or 16, packed and unaligned rows, one bin, a partial 512-bin stage
for _s, _n, _r, _p, _m in [(18, 5, 700, "pad", 0), (15, 18, 33, 0, 3), (18, 33, 1, 7, 0)]:
    for _f in (None, (2, 1), (2, 2), (3, 1)):
        case("epg_hist_s3", b_hist_s3, _s, _n, _r, pitch=_p, mis=_m, force=_f)
    case("epg_hist_s3", b_hist_s3, _s, _n, _r, pitch=_p, mis=_m, use_ws=False)
for _s, _n, _r, _p, _m in [(18, 5, 700, "pad", 0), (15, 18, 33, 0, 3), (18, 33, 1, 7, 0), (25, 21, 1000, 3, 5), (3, 7, 513, 0, 1)]:
    for _f in ((2, 2), (2, 1)):                                                            # clean rows: the reduced contraction produces the counts
        case("epg_hist_s3", b_hist_s3, _s, _n, _r, pitch=_p, mis=_m, force=_f, junk=False)
case("epg_hist_s3", b_hist_s3, 31, 21, 100)
case("epg_hist_s3", b_hist_s3, 40, 6, 50, pitch=0, mis=1)
case("epg_hist_s3", b_hist_s3, 18, 16, 300, junk=False)
for _n, _m in [(1, 0), (257, 8), (324, 0), (4097, 8)]:
    case("epg_normalise_i64", b_normalise, "epg_normalise_i64", _n, mis=_m)
    case("epg_normalise_i32", b_normalise, "epg_normalise_i32", _n, mis=_m // 2)
# -- S1 scores: the fused kernel (18 states, every row on the fast kernel), the two-pass route; tables in LDS and in memory
for _s, _n, _r, _p, _m in [(18, 379, 65, "pad", 0), (18, 41, 100, 0, 5), (15, 129, 33, 5, 0), (18, 1100, 31, "wide", 0), (40, 50, 20, "pad", 0), (18, 16, 1, "pad", 0)]:
    case("epg_score_s1", b_score_s1, _s, _n, _r, pitch=_p, mis=_m, top=_s - 2 if _n == 41 else None)
for _s, _n, _r in [(18, 379, 1000), (18, 1100, 65), (15, 2500, 33), (25, 16, 1)]:
    case("epg_score_s1_from_binhist", b_score_s1, _s, _n, _r, from_hist=True, top=_s - 1 if _r == 65 else None)
for _s, _n, _r, _z in [(18, 379, 1001, 0), (18, 379, 65, 1), (15, 40, 0, 0), (25, 16, 33, 1), (15, 2500, 33, 1)]:
    case("epg_combine_score_s1", b_combine, _s, _n, _r, _z)
for _s, _n, _r in [(18, 379, 1001), (15, 16, 33), (25, 1100, 1)]:
    case("epg_score_s1_from_binhist_table", b_s1_table, _s, _n, _r)
# -- S2 scores: the bin kernel of 15 / 18 / 25 states and the generic one; the log table in LDS (N < 4096 and room next to the
#    staging area) or in memory; q with and without zero cells (the workspace cell LPQ[S * S] chooses the kernel on the device)
for _s, _n, _r, _p, _t in [(18, 41, 100, "pad", None), (15, 129, 33, 0, 13), (20, 30, 65, 3, None)]:
    case("epg_score_s2", b_score_s2, _s, _n, _r, pitch=_p, top=_t)
for _s, _n, _r, _t in [(18, 379, 200, None), (18, 379, 130, 16), (25, 2000, 65, None), (18, 5000, 33, None), (15, 16, 1, 3), (7, 50, 100, None), (40, 60, 20, None)]:
    case("epg_score_s2_from_binhist", b_score_s2, _s, _n, _r, top=_t, from_hist=True)
# -- S3 scores on both score kernels (switch 1), S above the biosample-lane kernel's 20 states, the wide model
for _s, _n, _r, _p, _m in [(18, 5, 100, "pad", 0), (15, 10, 33, 0, 3)]:
    for _f in (None, (1, 1)):
        case("epg_score_s3", b_score_s3, _s, _n, _r, pitch=_p, mis=_m, force=_f)
case("epg_score_s3", b_score_s3, 25, 7, 65, pitch=2)
case("epg_score_s3", b_score_s3, 40, 6, 20)
# -- paired S1
for _s, _na, _nb, _ga, _gb, _r, _al in [(18, 379, 342, 379, 342, 1001, True), (15, 40, 33, 20, 20, 65, False), (21, 7, 9, 9, 7, 33, False), (25, 12, 12, 12, 12, 1, True),
                                         (18, 40, 33, 40, 33, 127, False)]:
    case("epg_pair_scores_s1_from_binhist", b_pair_scores, _s, _na, _nb, _ga, _gb, [_r], alias=_al)
case("epg_pair_scores_s1_from_binhist", b_pair_scores, 18, 900, 880, 900, 880, [64], alias=True, error=-2)     # the tables do not fit a CU's LDS
case("epg_pair_scores_s1_parts", b_pair_scores, 18, 70, 53, 70, 53, [130, 0, 71], parts=True, qstate=3, alias=True)
case("epg_pair_scores_s1_parts", b_pair_scores, 21, 12, 9, 6, 6, [65, 1], parts=True, qstate=-1)
case("epg_pair_scores_s1_parts", b_pair_scores, 15, 40, 33, 20, 20, [9] * 30, parts=True, qstate=14)            # more parts than a launch holds (24)
case("epg_pair_scores_s1_parts", b_pair_scores, 25, 12, 12, 12, 12, [33, 64], parts=True)
for _s, _r in [(18, 1001), (5, 33), (40, 20), (15, 1)]:
    case("epg_pair_finish", b_pair_finish, _s, _r)
for _s, _r, _rt in [(18, 1001, 1), (18, 65, 0), (15, 33, 1), (40, 20, 1), (3, 1, 0)]:
    case("epg_pair_metrics", b_pair_metrics, _s, _r, _rt)
for _na, _nb, _r, _q, _pa, _pb, _m in [(5, 5, 300, 17, "pad", "pad", 0), (379, 342, 65, 3, 0, 5, 3), (1, 17, 33, 0, 0, 0, 1), (70, 53, 100, -1, "pad", "pad", 0),
                                       (1100, 16, 31, 5, "wide", "pad", 0)]:
    case("epg_quiescent", b_quiescent, 18, _na, _nb, _r, _q, pa=_pa, pb=_pb, mis=_m)
for _s, _r, _q in [(18, 1001, 17), (15, 33, 0), (40, 257, -1)]:
    case("epg_quiescent_from_binhist", b_quiescent, _s, 12, 9, _r, _q, from_hist=True)
# -- null draws
for _s, _na, _nb, _r, _ga, _gb, _pa, _pb, _m in [(18, 12, 9, 300, 6, 6, "pad", "pad", 0), (18, 70, 53, 257, 70, 53, 0, 3, 5), (15, 17, 16, 33, 17, 16, 0, 0, 1),
                                                 (25, 129, 130, 65, 100, 100, "wide", 7, 0)]:
    case("epg_null_hist", b_null_hist, _s, _na, _nb, _r, _ga, _gb, pa=_pa, pb=_pb, mis=_m)
case("epg_null_hist", b_null_hist, 40, 12, 9, 33, 12, 9, error=-2)                                            # stops at 31 states
for _f in (None, (0, 1)):                                                                                     # both sampler kernels
    case("epg_null_hist_from_binhist", b_null_from_hist, 18, 70, 53, [257], force=_f)
    case("epg_null_hist_from_binhist", b_null_from_hist, 15, 70, 53, [33], ga=20, gb=20, force=_f)
    case("epg_null_hist_from_binhist_parts", b_null_from_hist, 18, 17, 16, [130, 0, 71], parts=True, force=_f, golden=True)
case("epg_null_hist_from_binhist", b_null_from_hist, 40, 17, 16, [65])
case("epg_null_hist_from_binhist_parts", b_null_from_hist, 25, 70, 53, [1, 63, 64, 65, 0, 17], parts=True)
case("epg_null_hist_from_binhist_parts", b_null_from_hist, 18, 40, 33, [9] * 50, parts=True, ga=6, gb=6)
case("epg_pair_count_null_parts", b_pair_count_null, 15, 100, 120, [130, 0, 71], golden=True)
case("epg_pair_count_null_parts", b_pair_count_null, 18, 379, 342, [1, 63, 64, 65, 0, 129], pa="wide", mis=3)
case("epg_pair_count_null_parts", b_pair_count_null, 25, 300, 257, [33, 300])
case("epg_pair_count_null_parts", b_pair_count_null, 18, 70, 53, [9] * 40)                                     # more parts than a launch holds (32)
case("epg_pair_count_null_parts", b_pair_count_null, 20, 40, 40, [33], error=-2)                               # not a model of the fused kernel
case("epg_pair_count_null_parts", b_pair_count_null, 18, 100, 300, [33], error=-2)                             # one and three groups per row
case("epg_pair_count_null_parts", b_pair_count_null, 18, 70, 53, [33], pa=0, error=-2)                         # a pitch that is not padded to 16 bytes
# -- similarity search: P around the 128-position tile, B past the four regions of a thread, n at both ends; a genome tile that
#    only fits LDS 64 positions at a time; block reductions with a partial last block and rows too long to stage
for _s, _w, _p, _b, _n in [(4, 3, 1, 1, 1), (4, 3, 127, 5, 1024), (5, 2, 128, 1, 7), (4, 3, 129, 5, 1), (124, 3, 129, 2, 16), (18, 25, 300, 4, 1024)]:
    case("epg_simsearch", b_simsearch, _s, _w, _p, _b, _n)
for _s, _r, _bs in [(18, 1003, 25), (3, 7, 512), (150, 250, 100), (18, 64, 1)]:
    case("epg_simsearch_reduce", b_reduce, _s, _r, _bs)
for _s, _r, _bs, _nb, _b in [(18, 1003, 5, 25, 1), (18, 1003, 5, 25, 257), (150, 450, 100, 3, 2), (4, 64, 1, 64, 3)]:
    case("epg_simsearch_slices", b_slices, _s, _r, _bs, _nb, _b)


# -- the one-CU grid.  tiles = (tiles of the launch that matters, waves of its capped grid), the waves from the dispatch code as
#    tests/grid_cap.py restates it
CAPPED = []


def capped(entry, builder, *args, tiles, **kw):
    ntiles, waves = tiles
    assert ntiles // waves >= 3, "%s: %d tiles on %d waves" % (entry, ntiles, waves)
    ident = "%s-%s" % (entry[4:], "-".join([str(a).replace(" ", "") for a in args] + ["%s=%s" % (k, str(v).replace(" ", "")) for k, v in kw.items()]))
    CAPPED.append(pytest.param(entry, builder, args, kw, id=ident[:120]))


def _tiles(rows, tile):
    return sum((r + tile - 1) // tile for r in rows)


def _count_waves(rows):                      # the count kernels: grid_for_tiles workgroups of 4 waves, tiles of 32 rows
    return 4 * count_grid(32 * _tiles(rows, 32), 1)


_W8 = 1 * 8 * 4                                              # k_s2_hist_wave, k_null_hist_rows: num_cus() x 8 workgroups of 4 waves, tiles of 64 rows
assert tile_rows(2 * 2 * 18) == tile_rows(2 * 2 * 15) == 64


_RAGGED = [2 * 768 + 5, 1, 130, 768 + 63, 0, 64, 777]                                      # whole, ragged and one-row tiles; an empty part
capped("epg_bin_hist", b_count, "epg_bin_hist", 18, 833, 3 * 256 + 37, pitch="pad", tiles=(_tiles([805], 32), _count_waves([805])))
capped("epg_bin_hist", b_count, "epg_bin_hist", 15, 129, 4 * 256 + 1, pitch=0, mis=3, tiles=(_tiles([1025], 32), _count_waves([1025])))
capped("epg_bin_hist", b_count, "epg_bin_hist", 25, 4100, 3 * 256 + 5, pitch=5, tiles=(_tiles([773], 32), _count_waves([773])))
capped("epg_bin_hist_s2", b_count, "epg_bin_hist_s2", 18, 379, 3 * 256 + 33, pitch="pad", tiles=(_tiles([801], 32), _count_waves([801])))
capped("epg_bin_hist_s2", b_count, "epg_bin_hist_s2", 25, 1024, 3 * 256 + 1, pitch="wide", mis=9, tiles=(_tiles([769], 32), _count_waves([769])))
capped("epg_bin_hist_s2", b_count, "epg_bin_hist_s2", 15, 1025, 3 * 256 + 1, pitch="pad", tiles=(_tiles([769], 32), _count_waves([769])))   # two passes
# (parts: three groups per row -- 773 + 1 + 31 + 300 rows -- and seven -- 129 + 700 --, one launch each)
capped("epg_bin_hist_parts", b_parts, 18, [(3 * 256 + 5, 379, "pad", 0), (1, 342, 0, 0), (0, 40, "pad", 0), (31, 379, 5, 3), (300, 342, "wide", 0),
                                           (129, 833, "pad", 0), (700, 800, 0, 7)], tiles=(_tiles([129, 700], 32), _count_waves([129, 700])))
capped("epg_bin_hist_parts", b_parts, 15, [(700, 1100, 0, 7), (33, 4100, "pad", 0), (1, 1025, 3, 0), (3 * 256 + 5, 1200, "pad", 0)],
       tiles=(_tiles([700, 33, 1, 773], 32), _count_waves([700, 33, 1, 773])))                                          # the any-width loop
capped("epg_pair_scores_s1_parts", b_pair_scores, 18, 70, 53, 70, 53, _RAGGED, parts=True, qstate=3, alias=True, tiles=(_tiles(_RAGGED, 64), pair_fused_waves(18, 70, 53, 70, 53)))
capped("epg_pair_scores_s1_parts", b_pair_scores, 15, 40, 33, 20, 20, _RAGGED, parts=True, qstate=-1, tiles=(_tiles(_RAGGED, 64), pair_fused_waves(15, 40, 33, 20, 20)))
capped("epg_pair_scores_s1_parts", b_pair_scores, 21, 12, 9, 6, 6, _RAGGED, parts=True, tiles=(_tiles(_RAGGED, 64), pair_fused_waves(21, 12, 9, 6, 6)))
capped("epg_pair_count_null_parts", b_pair_count_null, 18, 379, 342, _RAGGED, pa="wide", mis=3, tiles=(_tiles(_RAGGED, 64), pair_count_null_waves(18, 379 + 342, 1)))
capped("epg_pair_count_null_parts", b_pair_count_null, 25, 300, 257, _RAGGED + _RAGGED, tiles=(_tiles(_RAGGED + _RAGGED, 64), pair_count_null_waves(25, 300 + 257, 1)))
capped("epg_null_hist_from_binhist_parts", b_null_from_hist, 18, 70, 53, [4100, 1, 0, 63, 2049], parts=True, tiles=(_tiles([4100, 1, 63, 2049], 64), _W8))
capped("epg_null_hist_from_binhist_parts", b_null_from_hist, 15, 70, 53, [4100, 1, 0, 63, 2049], parts=True, ga=20, gb=20,
       tiles=(_tiles([4100, 1, 63, 2049], 64), _W8))
capped("epg_hist_s2_from_binhist", b_s2_from_hist, 18, 3 * 2048 + 70, 65536, tiles=(_tiles([3 * 2048 + 70], 64), _W8))
capped("epg_hist_s2_from_binhist", b_s2_from_hist, 31, 3 * 2048 + 7, 4095, tiles=(_tiles([3 * 2048 + 7], 64), _W8))
capped("epg_hist_s2_from_binhist_pair", b_s2_from_hist, 15, 3 * 2048 + 70, 30000, pair=True, tiles=(_tiles([3 * 2048 + 70], 64), _W8))


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


_SPECS = {}


def spec_of(abi, entry, builder, args, kw):
    """The Spec of a case of CASES, built once per process: tests/test_hip_abi_streams.py runs the same cases, and the oracle's
    share of a case is most of its time.  No run changes a Spec."""
    key = repr((entry, args, sorted(kw.items())))
    if key not in _SPECS:
        _SPECS[key] = builder(abi, np.random.default_rng(zlib.crc32(key.encode())), *args, **kw)
    return _SPECS[key]


@pytest.mark.parametrize("entry,builder,args,kw", CASES)
def test_contract(abi, entry, builder, args, kw):
    run_case(spec_of(abi, entry, builder, args, kw), abi)


@pytest.mark.parametrize("entry,builder,args,kw", CAPPED)
def test_contract_on_the_one_cu_grid(abi, entry, builder, args, kw):
    rng = np.random.default_rng(zlib.crc32(repr(("one CU", entry, args, sorted(kw.items()))).encode()))
    spec = builder(abi, rng, *args, **kw)
    assert spec.force is None and spec.error is None
    spec.force = (FORCE_CUS, 1)
    real = abi.call("epg_device_cus")
    assert real > 1
    run_case(spec, abi)
    assert abi.call("epg_device_cus") == real


def test_a_store_into_a_guard_is_reported():
    """The arena on the device: a plain torch store inside the arena's OWN allocation, one byte behind a buffer."""
    ar = Arena("cuda", guard_byte=1)
    ar.add("X", 1000, role="in", misalign=3)
    ar.add("H", 36, role="out", align=16)
    ar.build()
    ar.snapshot()
    ar.bytes("H").fill_(7)                                                   # the output itself may change
    ar.check()
    ar.guards("H")[1][0] = 9
    with pytest.raises(AssertionError, match=r"guard behind buffer 'H' damaged: 1 byte\(s\), first at offset \+0, last at offset \+0"):
        ar.check()
