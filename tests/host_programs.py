"""The suite's stand-alone host programs (tests/*.cpp, each with its own main): one way to build them.  They are ordinary
executables, so a sanitizer is linked into them and nothing has to be preloaded."""
import re
import shutil
import subprocess

import pytest

from epilogos_amd import build

ROOT = build.ROOT
ASAN_UBSAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def build_program(tmp_path, name, sources, libs, flags=ASAN_UBSAN, skip_without_runtime=False):
    """-> the executable tmp_path/name, built from `sources` with `flags` (default: the address and undefined-behaviour sanitizers).
    Skips where there is no compiler; a build that fails is a failure, unless the caller asks to skip where the linker does not find
    the sanitizer's runtime."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / name
    cmd = [cxx, "-O1", "-g", *flags, "-std=c++17", "-pthread", "-I" + str(ROOT / "include"),
           "-I" + str(build.CSRC)] + [str(s) for s in sources] + libs + ["-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    missing = re.search(r"cannot find -l(asan|ubsan|tsan)|cannot find lib(asan|ubsan|tsan)", res.stderr)
    if res.returncode != 0 and missing and skip_without_runtime:
        pytest.skip("the sanitizer's runtime is not installed: " + missing.group(0))
    assert res.returncode == 0, res.stderr
    return exe
