"""Every engine wrapper refuses, by name and before the library is reached, a tensor argument of the wrong dtype, a non-contiguous
view of it, one that is an element short and a host tensor -- and accepts the call it was derived from (tests/engine_bindings.py:
the smallest valid shapes).  No kernel runs in the refusals: _abi.call raises for every entry point that takes a stream."""
import ctypes as C
import re

import pytest
import torch

from tests.engine_bindings import N, TABLE

pytestmark = pytest.mark.gpu

WRONG = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int64: torch.float64, torch.int32: torch.float32,
         torch.int16: torch.int32, torch.int8: torch.uint8, torch.uint8: torch.int8}


def _paths(v, path=()):
    if torch.is_tensor(v):
        yield path
    elif isinstance(v, (list, tuple)):
        for i, e in enumerate(v):
            yield from _paths(e, path + (i,))


def _at(v, path):
    return v if not path else _at(v[path[0]], path[1:])


def _with(v, path, new):
    if not path:
        return new
    seq = list(v)
    seq[path[0]] = _with(seq[path[0]], path[1:], new)
    return tuple(seq) if isinstance(v, tuple) else seq


def _mutations(t, pitched, short):
    yield "wrong dtype", t.to(WRONG[t.dtype])
    if pitched:                                                  # a column stride of 2
        yield "column stride 2", t.repeat_interleave(2, dim=1)[:, ::2]
    elif t.dim() >= 2 and t.shape[0] > 1 and t.shape[1] > 1:
        yield "transposed", t.transpose(0, 1).contiguous().transpose(0, 1)
    elif t.shape[-1] > 1:
        yield "[::2]", t.repeat_interleave(2, dim=-1)[..., ::2]
    # (a tensor of one element has no non-contiguous view)
    if short:
        yield "one short", t[:, :N - 1] if pitched else t[..., :-1].contiguous()
    yield "host", t.cpu()


@pytest.fixture()
def no_launch(monkeypatch):
    """_abi.call raises for every entry point that takes a stream; the size and constant queries pass through."""
    from epilogos_amd import _abi
    _abi.load()
    launches = {name for reg in (_abi.HEADERS, _abi.INTERNAL, _abi.WRITER, _abi.READER, _abi.METRICS) for h in reg.values()
                for name, (res, args) in h.prototypes.items() if res is C.c_int and args and args[-1] is C.c_void_p}
    assert len(launches) > 50
    real = _abi.call

    def call(name, *args):
        if name in launches:
            raise AssertionError("%s was reached" % name)
        return real(name, *args)
    monkeypatch.setattr(_abi, "call", call)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_a_wrapper_refuses_each_bad_tensor_by_name(name, no_launch):
    from epilogos_amd import engine
    case = TABLE[name]("cuda")
    tried, problems = 0, []
    for arg, value in case.kwargs.items():
        for path in _paths(value):
            for what, bad in _mutations(_at(value, path), arg in case.pitched, arg not in case.sizes | case.scratch):
                tried += 1
                try:
                    getattr(engine, name)(**{**case.kwargs, arg: _with(value, path, bad)})
                except ValueError as e:
                    if not re.search(r"engine\.%s\b.*\b%s\b" % (name, arg), str(e)):
                        problems.append("%s%s %s: the message does not name it: %s" % (arg, list(path), what, e))
                except AssertionError as e:
                    problems.append("%s%s %s: %s" % (arg, list(path), what, e))
                else:
                    problems.append("%s%s %s: accepted" % (arg, list(path), what))
    assert tried >= 3 and not problems, "\n".join(problems)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_a_wrapper_accepts_its_valid_call(name):
    from epilogos_amd import engine
    case = TABLE[name]("cuda")
    out = getattr(engine, name)(**case.kwargs)
    torch.cuda.synchronize()
    for t in (out if isinstance(out, (list, tuple)) else [out]):
        assert t is None or isinstance(t, (torch.Tensor, list, dict, int))
    assert case.check is None or case.check(out, case.kwargs)
