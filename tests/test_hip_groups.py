"""GPU: epg_bin_hist_groups (include/epilogos_groups.h) against the oracle on the column-sliced matrix,
onp.bin_hist(x[:, cols], S): integers, bit for bit.

Shapes are the smallest at which the kernel can go wrong: one row, rows that end a 16-row tile and a 32-row super-tile early,
three super-tiles (more than one wave); widths of one byte, one 16-byte chunk, one byte more, just past one and two 128-byte
groups, the flagship 833 and a row of more than eight groups (three turns of the four-in-flight load loop); every pitch
N .. N + 15 (the packed ones send the last rows through the row-safe kernel) from bases of every alignment; all four counting
cores and all four group counts.  Row padding holds VALID states, rows hold 0xFF and a byte in [S, 31] inside and outside the
selected columns.  The contract cases run on the guarded arena of tests/abi_arena.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import _abi, engine
from oracle import oracle_np as onp
from tests.abi_arena import Arena

pytestmark = pytest.mark.gpu

SS = (1, 15, 18, 25, 31)
RS = (1, 33, 95)
NS = (1, 16, 17, 130, 257, 833, 1100)


def menu(N):
    """The memberships of the issue, as column lists of a row of N."""
    allc = np.arange(N)
    return {"every_other": allc[::2], "only_first": allc[:1], "only_last": allc[-1:], "last_chunk": allc[16 * ((N - 1) // 16):],
            "empty": allc[:0], "low_two_thirds": allc[:max(1, 2 * N // 3)], "high_two_thirds": allc[N // 3:], "all": allc}


def make_states(rng, R, N, S):
    """[R, N] int8: states of the model, a few 0xFF and a few bytes that are no state of it (31: in [S, 31] for every S <= 31)."""
    x = rng.integers(0, S, size=(R, N)).astype(np.int8)
    k = max(1, R * N // 40)
    x.reshape(-1)[rng.integers(0, R * N, size=k)] = -1
    x.reshape(-1)[rng.integers(0, R * N, size=k)] = 31
    if S < 31:
        x.reshape(-1)[rng.integers(0, R * N, size=k)] = S
    return x


def device_matrix(rng, x, ldx, mis, S):
    """x at pitch ldx, `mis` bytes into an allocation that ends with the last row; padding and slack hold valid states."""
    R, N = x.shape
    host = rng.integers(0, S, size=mis + R * ldx).astype(np.int8)
    rows = host[mis:].reshape(R, ldx)
    rows[:, :N] = x
    buf = torch.from_numpy(host).cuda()
    return buf, buf.data_ptr() + mis


def run(xptr, R, N, ldx, S, groups, want=None, counts0=None):
    """One call.  want: per group whether H_g is handed over (default: all).  -> ([H_g or None], counts [G, S] - counts0)."""
    G = len(groups)
    want = [True] * G if want is None else want
    member = engine.group_members("cuda", N, groups)
    Hs = [torch.full((R, S), 0x5555, dtype=torch.int16, device="cuda") if w else None for w in want]
    harr = (C.c_void_p * G)(*[h.data_ptr() if h is not None else None for h in Hs])
    start = np.arange(1, G * S + 1, dtype=np.int64) * 1000003 if counts0 is None else counts0
    counts = torch.from_numpy(start.copy()).cuda()
    _abi.call("epg_bin_hist_groups", C.c_void_p(xptr), R, N, ldx, S, G, C.c_void_p(member.data_ptr()), harr, C.c_void_p(counts.data_ptr()),
              None)
    torch.cuda.synchronize()
    return [h.cpu().numpy().view(np.uint16) if h is not None else None for h in Hs], (counts.cpu().numpy() - start).reshape(G, S)


def check(x, S, groups, Hs, counts, what):
    for g, cols in enumerate(groups):
        ref = onp.bin_hist(x[:, cols], S) if len(cols) else np.zeros((x.shape[0], S), dtype=np.int64)
        if Hs[g] is not None:
            assert np.array_equal(Hs[g].astype(np.int64), ref), "%s: H of group %d" % (what, g)
        assert np.array_equal(counts[g], ref.sum(axis=0)), "%s: counts of group %d" % (what, g)


@pytest.mark.parametrize("N", NS)
def test_every_pitch_and_base(N):
    """R x pitch N .. N + 15; S, G, the base alignment and the memberships walk through their values on the way (5 models and 4
    group counts are coprime: the 48 calls of a width see every pair of them)."""
    rng = np.random.default_rng(1000 + N)
    kinds = menu(N)
    names = list(kinds)
    i = 0
    for R in RS:
        for k in range(16):
            S, G, mis = SS[i % 5], 1 + i % 4, (5 * i + 1) % 16
            groups = [kinds[names[(3 * i + 2 * g) % len(names)]] for g in range(G)]
            x = make_states(rng, R, N, S)
            buf, xptr = device_matrix(rng, x, N + k, mis, S)
            Hs, counts = run(xptr, R, N, N + k, S, groups)
            check(x, S, groups, Hs, counts, "R=%d N=%d ldx=%d S=%d G=%d base+%d" % (R, N, N + k, S, G, mis))
            i += 1


@pytest.mark.parametrize("G", (1, 2, 3, 4))
@pytest.mark.parametrize("S", SS)
def test_every_membership(S, G):
    """Every instantiation (counting core x group count) on every membership of the menu, G at a time, at a width with a tail chunk
    and at the flagship width; padded pitch (the tile kernel alone) and packed pitch (tile kernel + row-safe kernel)."""
    rng = np.random.default_rng(100 * S + G)
    for R, N, ldx in ((95, 257, 272), (33, 833, 833 + 3)):
        kinds = menu(N)
        names = list(kinds)
        x = make_states(rng, R, N, S)
        buf, xptr = device_matrix(rng, x, ldx, 7, S)
        for first in range(0, len(names), G):
            groups = [kinds[names[(first + g) % len(names)]] for g in range(G)]
            Hs, counts = run(xptr, R, N, ldx, S, groups)
            check(x, S, groups, Hs, counts, "S=%d G=%d N=%d from %s" % (S, G, N, names[first]))


@pytest.mark.parametrize("S", SS)
def test_all_columns_is_bin_hist(S):
    """One group of all columns = epg_bin_hist, H and counts, exactly; and the engine's wrapper returns the same."""
    rng = np.random.default_rng(7 + S)
    R, N = 95, 833
    x = make_states(rng, R, N, S)
    X = engine.states_to_device(x)
    H1, c1 = engine.bin_hist(X, N, S)
    Hs, cg = engine.bin_hist_groups(X, N, S, [np.arange(N)])
    assert cg.shape == (1, S) and torch.equal(cg[0], c1) and torch.equal(Hs[0], H1)
    assert np.array_equal(c1.cpu().numpy(), onp.expected_s1(x, S))
    # four groups through the wrapper: two launches' worth of results in one, counts added to the caller's
    groups = [np.arange(0, N, 2), np.arange(1, N, 2), np.arange(N)[100:700], np.zeros(0, dtype=np.int64)]
    acc = torch.ones(4 * S, dtype=torch.int64, device="cuda")
    Hs, cg = engine.bin_hist_groups(X, N, S, groups, counts=acc)
    check(x, S, groups, [h.cpu().numpy().view(np.uint16) for h in Hs], cg.cpu().numpy() - 1, "engine.bin_hist_groups")
    assert all(h.data_ptr() % 16 == 0 for h in Hs)
    _H, cg = engine.bin_hist_groups(X, N, S, groups[:2], want_hist=False)
    assert _H is None and torch.equal(cg[0] + cg[1], c1)                 # the halves of a partition add up to the whole


def test_select_columns_on_device():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 40, size=(33, 50)).astype(np.int8)
    X = engine.states_to_device(x)
    cols = np.array([49, 0, 7, 8, 30, 31, 32, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13])
    Y = engine.select_columns(X, cols)
    assert Y.shape == (33, 32) and Y.is_cuda
    assert np.array_equal(Y.cpu().numpy()[:, :17], x[:, cols]) and bool((Y[:, 17:] == -1).all())
    H, c = engine.bin_hist(Y, 17, 40)                                    # a wide model on the gathered matrix: the existing path
    assert np.array_equal(H.cpu().numpy().view(np.uint16).astype(np.int64), onp.bin_hist(x[:, cols], 40))


# ---- the ABI contract on the guarded arena ---------------------------------------------------------------------------------

CONTRACT = [dict(R=95, N=257, ldx=257 + 5, S=18, G=3, mis=3), dict(R=33, N=130, ldx=144, S=31, G=4, mis=0),
            dict(R=1, N=17, ldx=17, S=15, G=2, mis=9)]


def build_arena(case, rng):
    R, N, ldx, S, G = (case[k] for k in ("R", "N", "ldx", "S", "G"))
    kinds = menu(N)
    groups = [kinds[n] for n in ("every_other", "high_two_thirds", "last_chunk", "empty")[:G]]
    x = make_states(rng, R, N, S)
    a = Arena("cuda", guard_byte=1)
    a.add("X", R * ldx, role="in", misalign=case["mis"])
    a.add("member", N, role="in", misalign=1)
    for g in range(G):
        a.add("H%d" % g, R * S * 2, role="out", align=16)
    a.add("counts", G * S * 8, role="out")
    a.build()
    rows = rng.integers(0, S, size=(R, ldx)).astype(np.int8)             # valid states in the row padding
    rows[:, :N] = x
    a.write("X", rows)
    member = np.zeros(N, dtype=np.uint8)
    for g, cols in enumerate(groups):
        member[cols] |= 1 << g
    member |= 0xF0 & rng.integers(0, 256, size=N).astype(np.uint8)       # bits G .. 7 are ignored (bits 4 .. 7 here)
    a.write("member", member)
    return a, x, groups


def arena_call(a, case, H="all", counts=True, **over):
    k = dict(case, **over)
    G = case["G"]
    harr = None if H is None else (C.c_void_p * G)(*[a.addr("H%d" % g) if H == "all" or g in H else None for g in range(G)])
    rc = _abi.load().epg_bin_hist_groups(a.ptr("X"), k["R"], k["N"], k["ldx"], k["S"], k["G"], a.ptr("member"), harr,
                                         a.ptr("counts") if counts else None, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", CONTRACT, ids=lambda c: "R%(R)d-N%(N)d-ldx%(ldx)d-S%(S)d-G%(G)d" % c)
def test_contract(case):
    rng = np.random.default_rng(case["N"])
    a, x, groups = build_arena(case, rng)
    R, S, G = case["R"], case["S"], case["G"]
    refs = [onp.bin_hist(x[:, cols], S) if len(cols) else np.zeros((R, S), dtype=np.int64) for cols in groups]
    ref_counts = np.stack([r.sum(axis=0) for r in refs]).reshape(-1)
    start = rng.integers(1, 1 << 40, size=G * S).astype(np.int64)

    def prefill(byte):
        for g in range(G):
            a.fill("H%d" % g, byte)
        a.write("counts", start)

    # outputs prefilled 0x00 / 0xFF, counts starting non-zero; guards and inputs byte for byte
    for byte in (0x00, 0xFF):
        prefill(byte)
        a.snapshot()
        assert arena_call(a, case) == 0
        a.check()
        for g in range(G):
            assert np.array_equal(a.read("H%d" % g, np.uint16).reshape(R, S).astype(np.int64), refs[g]), "H%d over 0x%02x" % (g, byte)
        assert np.array_equal(a.read("counts", np.int64), start + ref_counts)
    # NULL H array: counts only; no H is touched
    prefill(0xFF)
    a.snapshot(frozen=["H%d" % g for g in range(G)])
    assert arena_call(a, case, H=None) == 0
    a.check()
    assert np.array_equal(a.read("counts", np.int64), start + ref_counts)
    # single NULL entries: the others are written, the one left out is untouched; NULL counts
    for keep in range(G):
        prefill(0xFF)
        a.snapshot(frozen=["H%d" % g for g in range(G) if g != keep] + ["counts"])
        assert arena_call(a, case, H=(keep,), counts=False) == 0
        a.check()
        assert np.array_equal(a.read("H%d" % keep, np.uint16).reshape(R, S).astype(np.int64), refs[keep])
    # the shapes the header refuses leave every buffer untouched
    prefill(0xFF)
    everything = ["H%d" % g for g in range(G)] + ["counts"]
    for code, over, kw in ((-2, dict(S=32), {}), (-2, dict(G=5), {}), (-2, dict(N=65536, ldx=65536), {}), (-1, dict(G=0), {}),
                           (-1, dict(N=0), {}), (-1, dict(ldx=case["N"] - 1), {}), (-1, {}, dict(H=None, counts=False))):
        a.snapshot(frozen=everything)
        if over.get("G", 0) > G:                     # (a pointer array of the case's own length: the call must not read it)
            assert _abi.load().epg_bin_hist_groups(a.ptr("X"), R, case["N"], case["ldx"], S, 5, a.ptr("member"), None, a.ptr("counts"), None) == code
        else:
            assert arena_call(a, case, **dict(over, **kw)) == code
        torch.cuda.synchronize()
        a.check()
