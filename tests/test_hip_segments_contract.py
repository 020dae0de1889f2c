"""GPU: the two entry points of include/epilogos_segments.h read and write only what the header names -- one call each in a
guarded arena (tests/abi_arena.py), the way tests/test_hip_statebyline_contract.py runs its header's: every buffer sized exactly
(the workspace exactly epg_seg_ws_bytes), outputs and workspace prefilled with 0x00, 0xFF and random bytes (the results
bit-identical), guards and inputs intact, nothing written behind min(lines, cap) or at or behind R_c, and a workspace one byte
short refused with EPG_ERR_WORKSPACE before anything is touched."""
import numpy as np
import pytest

from epilogos_amd import _abi, segments as seg
from tests.abi_arena import Arena
from tests.test_hip_segments import TABLE, TILE, expand_call, join, make_lines, parse_call, random_runs, ref_column, ref_parse

pytestmark = pytest.mark.gpu


def _chroms(seed):
    rng = np.random.default_rng(seed)
    return [("chrM",) + random_runs(rng, 90)] + [(name,) + random_runs(rng, R) for name, R in zip(TABLE, (3000, 2 * TILE() + 5, 777))]


def test_parse_contract():
    chroms = _chroms(1)
    text = join(make_lines(chroms), final_newline=False)
    first, state, runs, (lo, hi) = ref_parse(chroms)
    L = len(first)
    for cap in (L, L + 40, L - 7):
        n = min(L, cap)
        want_runs = runs.copy()
        want_runs[(runs[:, 0] + runs[:, 1]) > cap] = 0
        base = None
        for prefill in (0x00, 0xFF, "random"):
            got = parse_call(text, cap=cap, prefill=prefill, text_mis=7, seed=2)
            assert got["info"].tolist() == [L, lo, hi, -1] and np.array_equal(got["runs"], want_runs)
            assert np.array_equal(got["first"][:n], first[:n]) and np.array_equal(got["state"][:n], state[:n])
            assert np.array_equal(got["first"][n:], got["first0"][n:]) and np.array_equal(got["state"][n:], got["state0"][n:])
            res = (got["first"][:n].tobytes(), got["state"][:n].tobytes(), got["runs"].tobytes(), got["info"].tobytes())
            base = base or res
            assert res == base, prefill


def test_parse_of_a_refused_text_is_the_same_whatever_the_buffers_held():
    lines = make_lines(_chroms(2))
    lines[400][3] = b"E0"
    lines[900][1] = b"7"
    text = join(lines)
    base = None
    for prefill in (0x00, 0xFF, "random"):
        got = parse_call(text, prefill=prefill, text_mis=3, seed=5)
        assert got["info"][0] == len(lines) and got["info"][3] == 400
        res = (got["first"].tobytes(), got["state"].tobytes(), got["runs"].tobytes(), got["info"].tobytes())
        base = base or res
        assert res == base, prefill
        for c in range(len(TABLE)):                              # expanding what a refused text left stays inside the column
            expand_call(got["first"], got["state"], got["runs"], c, 5000, seed=c)


def test_parse_refuses_a_short_workspace_and_touches_nothing():
    import torch
    lib = _abi.load()
    text = join(make_lines(_chroms(3)))
    n, L = len(text), text.count(b"\n")
    wsb = lib.epg_seg_ws_bytes(n, len(TABLE))
    ar = Arena("cuda", guard_byte=1)
    ar.add("text", n, role="in")
    ar.add("names", 80 * len(TABLE), role="in")
    ar.add("first", 4 * L, role="out", align=16)
    ar.add("state", L, role="out", align=16)
    ar.add("runs", 24 * len(TABLE), role="out", align=8)
    ar.add("info", 32, role="out", align=8)
    ar.add("ws", wsb - 1, role="ws", align=16)
    ar.build()
    ar.write("text", np.frombuffer(text, dtype=np.uint8))
    ar.write("names", seg.name_table(TABLE))
    ar.snapshot(frozen=("first", "state", "runs", "info", "ws"))
    with pytest.raises(_abi.EpilogosHipError) as e:
        _abi.call("epg_seg_parse", ar.ptr("text"), n, ar.ptr("names"), len(TABLE), 200, ar.ptr("first"), ar.ptr("state"), L, ar.ptr("runs"),
                  ar.ptr("info"), ar.ptr("ws"), wsb - 1, None)
    assert e.value.code == -4
    torch.cuda.synchronize()
    ar.check()


def test_expand_contract():
    chroms = _chroms(4)
    first, state, runs, _range = ref_parse(chroms)
    for c, (_name, lengths, states) in enumerate(chroms[1:]):
        want = ref_column(lengths, states)
        Rc = len(want)
        for R in (Rc, Rc + 33, Rc - 1):
            n = min(R, Rc)
            base = None
            for seed in (0, 1, 2):                               # three canary patterns in the column
                col, before = expand_call(first, state, runs, c, R, seed=seed)
                assert np.array_equal(col[:n], want[:n]) and np.array_equal(col[n:], before[n:])
                base = base or col[:n].tobytes()
                assert col[:n].tobytes() == base
