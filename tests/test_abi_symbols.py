"""CPU-side checks of the drop-in boundary: the library builds, loads, and exports exactly what every public header declares;
every header of _abi.HEADERS is bound by its table, type for type.  No compute calls (no GPU here)."""
import shutil
import subprocess

import pytest

from epilogos_amd import _abi, build
from tests.abi_headers import ctypes_of, header_prototypes

# what the headers declare today, pinned: the exact names, or their number and prefix
NAMES = {
    "groups": ["epg_bin_hist_groups"],
    "nulldraws": ["epg_null_dist_draws_parts", "epg_null_exceed", "epg_null_exceed_ws_bytes"],
    "simsearch_pick": ["epg_simsearch_pick", "epg_simsearch_pick_ws_bytes", "epg_simsearch_rank", "epg_simsearch_rank_ws_bytes",
                       "epg_simsearch_rolling_max", "epg_simsearch_rowscore"],
    "census": ["epg_state_census"],
    "concordance": ["epg_concordance", "epg_concordance_ws_bytes"],
    "gennorm": ["epgf_gennorm_fit", "epgf_gennorm_nnlf", "epgf_gennorm_ws_bytes"],
}
# (at least, at most, prefix)
COUNT_AND_PREFIX = {"scores_text": (2, None, "epgt_"), "statebyline": (4, 4, "epg_sbl_"), "segments": (4, 4, "epg_seg_")}
# the source file with the header's entry points, where it is not epg_<key>.hip
SOURCE = {"core": "epg_abi.hip", "nulldraws": "epg_null_exceed.hip"}


@pytest.fixture(scope="module")
def lib():
    if build.is_stale():
        if shutil.which("hipcc") is None:
            pytest.skip("hipcc not available and library not prebuilt")
        build.build_library()
    return _abi.load()


def test_the_registry_is_the_list_of_public_headers():
    assert list(_abi.HEADERS) == list(build.PUBLIC_HEADERS) and len(_abi.HEADERS) == 10
    assert set(NAMES) | set(COUNT_AND_PREFIX) | {"core"} == set(_abi.HEADERS)
    assert _abi.HEADERS["core"] == (_abi.HEADER, _abi.PROTOTYPES) and _abi.HEADER.name == "epilogos_amd.h"
    assert _abi.header_symbols() == _abi.header_symbols("core")
    assert _abi.ABI_VERSION == _abi.header_constant("core", "EPG_ABI_VERSION") == 2
    with pytest.raises(RuntimeError):
        _abi.header_constant("core", "EPG_NO_SUCH_CONSTANT")


def test_the_tables_are_pairwise_disjoint():
    """A header of its own: no other header, and no other table, knows its entry points."""
    keys = list(_abi.HEADERS)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not set(_abi.HEADERS[a].prototypes) & set(_abi.HEADERS[b].prototypes), (a, b)
            assert not set(_abi.header_symbols(a)) & set(_abi.header_symbols(b)), (a, b)


@pytest.mark.parametrize("which", list(_abi.HEADERS))
def test_header_and_binding_agree(which):
    header = _abi.HEADERS[which]
    hdr = _abi.header_symbols(which)
    assert hdr, "no prototypes parsed from %s" % header.path
    assert sorted(header.prototypes) == hdr
    protos = header_prototypes(which)
    assert sorted(protos) == hdr
    if which in NAMES:
        assert hdr == NAMES[which]
    if which in COUNT_AND_PREFIX:
        least, most, prefix = COUNT_AND_PREFIX[which]
        assert len(hdr) >= least and (most is None or len(hdr) <= most) and all(n.startswith(prefix) for n in hdr)
    for name, (res, args) in header.prototypes.items():
        ret, params = protos[name]
        assert res is ctypes_of(ret, returned=True), "%s returns %s in the header, %s in the binding" % (name, ret, res.__name__)
        assert len(args) == len(params), "%s: %d parameters in the header, %d in the binding" % (name, len(params), len(args))
        for i, (a, p) in enumerate(zip(args, params)):
            assert a is ctypes_of(p), "%s: parameter %d is `%s` in the header, %s in the binding" % (name, i, p, a.__name__)
    assert header.path in build.HEADERS and header.path.name == build.PUBLIC_HEADERS[which]
    assert SOURCE.get(which, "epg_%s.hip" % which) in build.SOURCES


@pytest.mark.parametrize("which", list(_abi.HEADERS))
def test_library_exports_every_header_symbol(lib, which):
    import ctypes
    fresh = ctypes.CDLL(str(_abi.lib_path()))                    # looked up by the plain name: a C++-mangled export would not be found
    for name in _abi.header_symbols(which):
        assert hasattr(lib, name) and hasattr(fresh, name), "libepilogos_hip.so does not export " + name


@pytest.mark.parametrize("which", list(_abi.HEADERS))
def test_exports_are_c_abi(lib, which):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    out = subprocess.run([nm, "-D", "--defined-only", str(_abi.lib_path())], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in _abi.header_symbols(which):
        assert name in exported          # unmangled => extern "C"


def test_version_and_argument_validation_without_gpu(lib):
    assert lib.epg_version() == _abi.ABI_VERSION == 2          # (the header's EPG_ABI_VERSION; bumped with every change of the ABI)
    # pure argument validation happens before any HIP call
    rc = lib.epg_bin_hist(None, -1, 10, 10, 18, None, None, None)
    assert rc == -1 and b"bad shape" in lib.epg_last_error()
    rc = lib.epg_bin_hist(None, 10, 10, 5, 18, None, None, None)       # ldx < N
    assert rc == -1
    rc = lib.epg_bin_hist(None, 10, 10, 16, 128, None, None, None)     # S > 127: states are int8
    assert rc == -2
    rc = lib.epg_bin_hist(None, 10, 10, 16, 40, None, None, None)      # a wide model is taken; X is NULL
    assert rc == -1
    assert lib.epg_ws_bytes(4, 10, 10, 18) == -1
    assert lib.epg_ws_bytes(1, 0, 833, 18) >= 834 * 18 * 12


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_abi, "_lib", None)
    monkeypatch.setattr(_abi, "lib_path", lambda: tmp_path / "nope.so")
    with pytest.raises(_abi.EpilogosHipError):
        _abi.load()


def test_engine_refuses_to_run_without_gpu():
    import torch
    from epilogos_amd import engine
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_abi.EpilogosHipError):
        engine.require_gpu()


def test_io_library_exports_its_header():
    import re
    from pathlib import Path
    from epilogos_amd import _io
    if build.io_is_stale():
        build.build_io_library()
    lib = _io.load()
    hdr = (Path(__file__).resolve().parents[1] / "include" / "epilogos_io.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(epgio_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 9
    for n in names:
        assert hasattr(lib, n), n


def test_console_script_of_pyproject_resolves():
    """pyproject.toml declares the reference's `epilogos` command (setup.py:28-33) as epilogos_amd.run:cli."""
    import importlib
    from pathlib import Path

    import tomli
    meta = tomli.loads((Path(__file__).resolve().parents[1] / "pyproject.toml").read_text())
    target = meta["project"]["scripts"]["epilogos"]
    mod, fn = target.split(":")
    assert callable(getattr(importlib.import_module(mod), fn))
    assert meta["tool"]["setuptools"]["dynamic"]["version"]["attr"] == "epilogos_amd.__version__"
