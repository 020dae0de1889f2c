"""GPU: epgf_gennorm_fit and epgf_gennorm_nnlf enqueue only on the caller's stream, wait for nothing and keep no host pointer -- the
procedure of tests/test_hip_abi_streams.py (stream_case: baseline, side stream, capture with every output and workspace frozen, two
replays with the call's host arrays overwritten in between) on the guarded arena of tests/test_hip_abi_contract.py (Spec / Run:
exact-size buffers between guards, misaligned inputs, inputs unchanged).  The entry points carry the prefix epgf_ and so are not in
that file's table (include/epilogos_gennorm.h says why); this file is their case list.  The oracle of every step is scipy: the
fit-quality condition of tests/test_gennorm_host.py and scipy's nnlf within tests/gennorm_ref.nnlf_bound."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gennorm_ref as ref
from tests.test_gennorm_host import no_worse_than_scipy, scipy_nnlf
from tests.test_hip_abi_contract import F64, I32, Spec
from tests.test_hip_abi_streams import stream_case
from tests.test_hip_gennorm import FIT_CASES, INVALID, case_inputs, nnlf_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from epilogos_amd import _abi, engine
    engine.require_gpu()
    return _abi


def s_fit(abi, k):
    family, n, T, with_idx, flag, seed = FIT_CASES[k]
    x, idx = case_inputs(family, n, T, with_idx, seed)
    M = x.size
    sp = Spec(18)
    sp.inp("x", x, mis=4)                                                   # a float's alignment, no more
    if with_idx:
        sp.inp("idx", idx, mis=4)
    sp.out("params", F64, 3 * T, mis=8)
    sp.out("fval", F64, T, mis=8)
    sp.out("info", I32, 2 * T, mis=4)
    sp.ws("ws", abi.call("epgf_gennorm_ws_bytes", M, T, n))

    def call(abi, P, st):
        if with_idx:
            sp.keep(idx.copy())                                             # the host's copy of the indices: scribbled over between the replays
        abi.call("epgf_gennorm_fit", P["x"], M, P.get("idx"), T, n, P["params"], P["fval"], P["info"], P["ws"], sp.nbytes("ws"), st)
    sp.call = call

    def verify(o):
        params, info = o["params"].reshape(T, 3), o["info"].reshape(T, 2)
        assert (info[:, 1] == flag).all() and (info[:, 0] <= ref.MAXFUN).all()
        for t in range(T):
            s = x[idx[t]] if with_idx else x
            assert abs(o["fval"][t] - scipy_nnlf(params[t], s)) <= ref.nnlf_bound(params[t], s)
            no_worse_than_scipy(params[t], s, "%s n=%d trial %d" % (family, n, t))
    sp.verify = verify
    return sp


def s_nnlf(abi, M, T):
    x = ref.sample("signedsq", M)
    p = nnlf_params(x, T)
    p[3] = INVALID[0]
    sp = Spec(18)
    sp.inp("x", x, mis=4)
    sp.inp("params", p, mis=8)
    sp.out("nnlf", F64, T, mis=8)
    sp.ws("ws", abi.call("epgf_gennorm_ws_bytes", M, T, 0))
    sp.call = lambda abi, P, st: abi.call("epgf_gennorm_nnlf", P["x"], M, P["params"], T, P["nnlf"], P["ws"], sp.nbytes("ws"), st)

    def verify(o):
        for t in range(T):
            if t == 3:
                assert o["nnlf"][t] == np.inf
            else:
                assert abs(o["nnlf"][t] - scipy_nnlf(p[t], x)) <= ref.nnlf_bound(p[t], x), t
    sp.verify = verify
    return sp


@pytest.mark.parametrize("k", [1, 6, 5], ids=["idx-n1025-T3", "all-n1025-T1", "idx-n2-T3"])
def test_fit_stream_contract(abi, k):
    stream_case(s_fit(abi, k), abi)


@pytest.mark.parametrize("M,T", [(1023, 8), (5000, 101)])
def test_nnlf_stream_contract(abi, M, T):
    stream_case(s_nnlf(abi, M, T), abi)
