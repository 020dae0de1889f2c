"""GPU: the two entry points of include/epilogos_statebyline.h read and write only what the header names -- one call each in a
guarded arena (tests/abi_arena.py), the way tests/test_hip_abi_contract.py runs the entry points of epilogos_amd.h: every buffer
sized exactly (the workspace exactly epg_sbl_ws_bytes), outputs and workspace prefilled with 0x00, 0xFF and random bytes (the
results bit-identical), guards and inputs intact, and a workspace one byte short refused with EPG_ERR_WORKSPACE before anything
is touched."""
import numpy as np
import pytest

from epilogos_amd import _abi
from tests.abi_arena import Arena
from tests.test_hip_statebyline import make_text, mixed_values, parse_call, ref_column, transpose_call

pytestmark = pytest.mark.gpu


def test_parse_contract():
    rng = np.random.default_rng(1)
    text = make_text(mixed_values(rng, 5000), final_newline=False)
    want, rows, lo, hi = ref_column(text)
    base = None
    for prefill in (0x00, 0xFF, "random"):
        col, before, info = parse_call(text, cap=rows + 40, prefill=prefill, text_mis=7, col_mis=13, seed=2)
        assert info.tolist() == [rows, lo, hi, -1] and np.array_equal(col[:rows], want)
        assert np.array_equal(col[rows:], before[rows:])         # nothing behind the rows is written
        got = (col[:rows].tobytes(), info.tobytes())
        base = base or got
        assert got == base, prefill


def test_parse_refuses_a_short_workspace_and_touches_nothing():
    import torch
    lib = _abi.load()
    text = make_text(mixed_values(np.random.default_rng(2), 9000))
    n, wsb = len(text), lib.epg_sbl_ws_bytes(len(text))
    ar = Arena("cuda", guard_byte=1)
    ar.add("text", n, role="in")
    ar.add("col", 9000, role="out", align=16)
    ar.add("info", 32, role="out", align=8)
    ar.add("ws", wsb - 1, role="ws", align=16)
    ar.build()
    ar.write("text", np.frombuffer(text, dtype=np.uint8))
    ar.snapshot(frozen=("col", "info", "ws"))
    with pytest.raises(_abi.EpilogosHipError) as e:
        _abi.call("epg_sbl_parse", ar.ptr("text"), n, ar.ptr("col"), 9000, ar.ptr("info"), ar.ptr("ws"), wsb - 1, None)
    assert e.value.code == -4
    torch.cuda.synchronize()
    ar.check()


def test_transpose_contract():
    rng = np.random.default_rng(3)
    R, pitch = 1000, 1008
    cols = rng.integers(0, 18, size=(37, pitch)).astype(np.int8)
    base = None
    for seed in (0, 1, 2):                                       # three canary patterns in X: the named columns identical, the rest kept
        X, before = transpose_call(cols, R, pitch, 848, 401, canary_seed=seed)
        want = before.copy()
        want[:, 401:438] = cols[:, :R].T
        assert np.array_equal(X, want)
        got = X[:, 401:438].tobytes()
        base = base or got
        assert got == base
