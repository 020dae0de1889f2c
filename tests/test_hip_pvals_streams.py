"""GPU: epgf_gennorm_pvals and epgf_bh_adjust touch only what csrc/epg_pvals.h names, enqueue only on the caller's stream, wait for
nothing and can be captured -- the procedures of tests/test_hip_abi_contract.py (run_case: exact-size buffers between guards,
misaligned inputs, hostile guards, dirty outputs and workspace, inputs unchanged) and tests/test_hip_abi_streams.py (stream_case:
baseline, side stream, capture with every output and workspace frozen, two replays).  The entry points are package-internal and
carry the prefix epgf_, so they are not in those files' tables; this file is their case list.  The oracles are those of
tests/test_hip_pvals.py: scipy within the recorded bounds, benjaminiHochberg bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from epilogos_amd import roiAndVisualPairwise as rv
from tests import pvals_ref as ref
from tests.test_hip_abi_contract import F64, I32, Spec, run_case
from tests.test_hip_abi_streams import stream_case
from tests.test_hip_pvals import bh_input
from tests.test_pvals_host import host_pvals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


def s_pvals(abi, M, params):
    x = ref.values(M, params)
    want = host_pvals(x, params)
    sp = Spec(18)
    sp.inp("x", x, mis=4)                                                   # a float's alignment, no more
    sp.inp("params", np.array(params, dtype=F64), mis=8)
    sp.out("p", F64, M, mis=8)
    sp.out("flags", I32, 2, mis=4)
    sp.call = lambda abi, P, st: abi.call("epgf_gennorm_pvals", P["x"], M, P["params"], P["p"], P["flags"], st)

    def verify(o):
        assert list(o["flags"]) == [0, 0]
        rel, ab = ref.differences(o["p"], want, x, params[1])
        assert rel <= ref.FACTOR * ref.REL_BELOW and ab <= ref.FACTOR * ref.ABS_ABOVE
    sp.verify = verify
    return sp


def s_bh(abi, M, kind):
    p = bh_input(kind, M)
    want = rv.benjaminiHochberg(p)
    sp = Spec(18)
    sp.inp("p", p, mis=8)                                                   # a double's alignment, no more
    sp.out("adj", F64, M, mis=8)
    sp.out("flags", I32, 1, mis=4)
    sp.ws("ws", abi.call("epgf_bh_ws_bytes", M))
    sp.call = lambda abi, P, st: abi.call("epgf_bh_adjust", P["p"], M, P["adj"], P["flags"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        assert list(o["flags"]) == [0] and np.array_equal(o["adj"].view(np.uint64), want.view(np.uint64))
    sp.verify = verify
    return sp


@pytest.mark.parametrize("k", [0, 4], ids=["beta0.3478", "beta8"])
def test_pvals_contract_and_streams(abi, k):
    run_case(s_pvals(abi, 1025, ref.PARAMS[k]), abi)
    stream_case(s_pvals(abi, 1025, ref.PARAMS[k]), abi)


@pytest.mark.parametrize("M,kind", [(1025, "rounded"), (70001, "uniform")])
def test_bh_contract_and_streams(abi, M, kind):
    run_case(s_bh(abi, M, kind), abi)
    stream_case(s_bh(abi, M, kind), abi)
