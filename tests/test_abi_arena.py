"""No GPU: the guarded arena of tests/abi_arena.py finds what it is meant to find (on CPU tensors, which it treats like device
ones), and every entry point of include/epilogos_amd.h that takes a pointer has a contract case in
tests/test_hip_abi_contract.py -- a new entry point without one fails here, before it reaches a GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.abi_arena import GUARD, Arena


def _arena():
    ar = Arena("cpu", guard_byte=1)
    ar.add("X", 1000, role="in", misalign=3)
    ar.add("H", 36, role="out", align=16)
    ar.add("ws", 300, role="ws")
    ar.add("q", 72, role="in", misalign=4)
    ar.build()
    ar.write("X", np.arange(1000, dtype=np.uint8))
    ar.write("q", np.linspace(0, 1, 18, dtype=np.float32))
    ar.snapshot()
    return ar


def test_layout_is_exact_and_guarded():
    ar = _arena()
    assert ar.addr("X") % 256 == 3 and ar.addr("H") % 16 == 0 and ar.addr("q") % 256 == 4
    spans = sorted((ar.at[n][0], ar.at[n][1]) for n in ar.at)
    assert spans[0][0] >= GUARD and spans[-1][1] + GUARD <= ar.mem.numel()
    assert all(b[0] - a[1] >= 2 * GUARD for a, b in zip(spans, spans[1:]))           # a guard of its own on either side
    assert [ar.nbytes(n) for n in ("X", "H", "ws", "q")] == [1000, 36, 300, 72]
    before, behind = ar.guards("H")
    assert before.numel() == behind.numel() == GUARD and bool((before == 1).all()) and bool((behind == 1).all())
    with pytest.raises(ValueError):
        Arena("cpu", guard_byte=0xFF)
    with pytest.raises(ValueError):
        Arena("cpu", guard=1024)
    with pytest.raises(ValueError):
        ar.write("H", np.zeros(37, dtype=np.uint8))                                 # sizes are exact


def test_untouched_arena_and_written_outputs_pass():
    ar = _arena()
    ar.check()
    ar.bytes("H").fill_(0)
    ar.fill("ws", "random", np.random.default_rng(0))
    ar.check()


@pytest.mark.parametrize("name", ["X", "H", "ws", "q"])
def test_one_byte_next_to_a_buffer_is_reported_by_name(name):
    ar = _arena()
    a, b, _ = ar.at[name]
    ar.mem[a - 1] = 7                                                             # just before
    with pytest.raises(AssertionError, match=r"guard before buffer '%s' damaged: 1 byte\(s\), first at offset -1, last at offset -1" % name):
        ar.check()
    ar = _arena()
    ar.mem[ar.at[name][1]] = 7                                                    # just behind
    with pytest.raises(AssertionError, match=r"guard behind buffer '%s' damaged: 1 byte\(s\), first at offset \+0, last at offset \+0" % name):
        ar.check()
    ar = _arena()
    ar.guards(name)[1][GUARD - 1] = 7                                             # the far edge of the guard behind
    ar.guards(name)[0][0] = 7                                                     # and of the one before
    with pytest.raises(AssertionError) as e:
        ar.check()
    assert "guard behind buffer '%s' damaged: 1 byte(s), first at offset +%d" % (name, GUARD - 1) in str(e.value)
    assert "guard before buffer '%s' damaged: 1 byte(s), first at offset -%d" % (name, GUARD) in str(e.value)


def test_a_run_of_damage_reports_first_and_last_offset():
    ar = _arena()
    ar.guards("H")[1][16:52] = 0
    with pytest.raises(AssertionError, match=r"guard behind buffer 'H' damaged: 36 byte\(s\), first at offset \+16, last at offset \+51"):
        ar.check()


def test_changed_input_and_frozen_output_are_reported():
    ar = _arena()
    ar.bytes("q")[5] = 0x55
    with pytest.raises(AssertionError, match=r"input buffer 'q' changed: 1 byte\(s\), first at offset \+5, last at offset \+5"):
        ar.check()
    ar = _arena()
    ar.snapshot(frozen=["H"])
    ar.bytes("ws").fill_(0)
    ar.check()
    ar.bytes("H")[35] = 0
    with pytest.raises(AssertionError, match="buffer 'H' was written although the call was told not to produce it"):
        ar.check()


def test_poisoned_guards_are_in_phase_with_the_buffer():
    ar = _arena()
    nan = np.array([np.nan], dtype=np.float32).view(np.uint8)
    ar.poison_guards("q", nan)
    before, behind = ar.guards("q")
    assert np.isnan(before.numpy().view(np.float32)).all() and np.isnan(behind.numpy().view(np.float32)).all()
    assert np.array_equal(ar.read("q", np.float32), np.linspace(0, 1, 18, dtype=np.float32))


def test_every_entry_point_with_a_pointer_has_a_contract_case():
    from tests.abi_headers import header_prototypes
    from tests.test_hip_abi_contract import CASES, EXEMPT
    protos = header_prototypes("core")
    assert len(protos) >= 36
    covered = {c.values[0] for c in CASES}
    assert covered <= set(protos), "cases of entry points the header does not declare: %s" % sorted(covered - set(protos))
    assert sorted(EXEMPT) == ["epg_last_error", "epg_test_force"] and all(EXEMPT.values())
    need = [name for name, (ret, params) in protos.items() if any("*" in p for p in params) and name not in EXEMPT]
    assert len(need) >= 30
    missing = sorted(set(need) - covered)
    assert not missing, "entry points without a contract case in tests/test_hip_abi_contract.py: %s" % missing
