"""The binding rule of DESIGN.md ("One binding per entry point"), without a GPU: where the package may reach the library, and that
every engine wrapper refuses host tensors before it does."""
import ast
import re
from pathlib import Path

import pytest

from tests.engine_bindings import NOT_WRAPPERS, TABLE

PKG = Path(__file__).resolve().parents[1] / "epilogos_amd"
SOURCES = {p.name: p.read_text() for p in sorted(PKG.glob("*.py"))}


def _files_with(text):
    return {name for name, src in SOURCES.items() if text in src}


def test_the_library_is_reached_from_engine_and_the_three_batch_readers_only():
    assert _files_with("_abi.call(") <= {"_abi.py", "engine.py", "segments.py", "stateByLine.py", "textBatches.py"}
    assert _files_with("engine._ptr") == set() and _files_with("engine._stream") == set()
    assert _files_with(".data_ptr()") <= {"engine.py", "textBatches.py"}


def _functions_that_call_the_library():
    tree = ast.parse(SOURCES["engine.py"])
    lines = SOURCES["engine.py"].splitlines()
    return {f.name for f in tree.body if isinstance(f, ast.FunctionDef) and "_abi.call(" in "\n".join(lines[f.lineno - 1:f.end_lineno])}


def test_the_table_names_every_wrapper():
    """A wrapper added to engine.py needs a row in tests/engine_bindings.py."""
    assert _functions_that_call_the_library() == set(TABLE) | NOT_WRAPPERS


@pytest.fixture(scope="module")
def cases():
    return {name: factory("cpu") for name, factory in TABLE.items()}          # (before the patch: the factories ask for workspace sizes)


@pytest.fixture()
def no_library(monkeypatch):
    from epilogos_amd import _abi

    def reached(*a, **k):
        raise AssertionError("the library was reached: %r" % (a[:1],))
    monkeypatch.setattr(_abi, "call", reached)
    monkeypatch.setattr(_abi, "load", reached)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_a_wrapper_refuses_host_tensors_before_the_library_is_reached(name, cases, no_library):
    from epilogos_amd import engine
    with pytest.raises(ValueError, match=re.escape("engine.%s" % name)):
        getattr(engine, name)(**cases[name].kwargs)
