"""csrc/epg_parts.h on the host: the packing loop of the multi-part launches and the cursor that the kernels walk the packed
table with, checked together by a stand-alone program (tests/parts_host_main.cpp) against expectations written as a direct loop
over parts and rows.  Built with AddressSanitizer and UBSan where the host compiler has their runtimes."""
import shutil
import subprocess
from pathlib import Path

import pytest

from epilogos_amd import build

MAIN = Path(__file__).resolve().parent / "parts_host_main.cpp"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _compile(cxx, flags, exe):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", *flags, "-I" + str(build.CSRC), str(MAIN), "-o", str(exe)]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_pack_parts_and_cursor_visit_every_row_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")          # the compiler build_io_library uses
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "parts_host"
    sanitized = _compile(cxx, SANITIZE, exe).returncode == 0
    if not sanitized:
        res = _compile(cxx, [], exe)
        assert res.returncode == 0, res.stdout + res.stderr
    print("parts_host built %s" % ("with -fsanitize=address,undefined" if sanitized else "WITHOUT sanitizers (no runtimes)"))
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(res.stdout + res.stderr)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
