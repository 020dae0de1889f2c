"""The native host I/O library (csrc/epg_io.cpp) through the stand-alone program tests/io_check.cpp (no GPU, nothing preloaded: the
program is an ordinary executable with the library's one source file compiled into it).  Three builds, each a test of its own: with
the address and undefined-behaviour sanitizers; with the thread sanitizer -- the worker threads of the readers, the writers and the
helpers all start in one function, run_workers --; and without a sanitizer but with an operator new that fails on demand, where
every entry point that allocates or starts threads must answer a refused allocation with its failure value and a message, never
with the end of the process.  What the program checks, and against what, is written at its top."""
import re
import subprocess

from epilogos_amd import build
from tests.host_programs import build_program

ROOT = build.ROOT
SOURCES = [ROOT / "tests" / "io_check.cpp", build.IO_SOURCE]
REPORT = re.compile(r"Sanitizer|runtime error|WARNING: ThreadSanitizer|data race")


def _run(exe, tmp_path, *passes):
    """The program once per entry of `passes` (its arguments after the directory), side by side, each in a directory of its own:
    exit status 0, "io_check: ok", no sanitizer report; -> the outputs."""
    runs = []
    for k, args in enumerate(passes or [()]):
        work = tmp_path / ("files%d" % k)
        work.mkdir(exist_ok=True)
        runs.append(subprocess.Popen([str(exe), str(work), *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [(r.communicate()[0], r.returncode) for r in runs]
    for out, rc in outs:
        assert rc == 0 and "io_check: ok" in out and not REPORT.search(out), out[-4000:]
    return [out for out, _rc in outs]


def test_the_library_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build_program(tmp_path, "io_check_asan", SOURCES, ["-lz"], skip_without_runtime=True)
    _run(exe, tmp_path, (), ("--bgzf",))                                        # --bgzf: EPILOGOS_BGZF=1, set by the program before its first thread


def test_the_library_under_the_thread_sanitizer(tmp_path):
    exe = build_program(tmp_path, "io_check_tsan", SOURCES, ["-lz"], flags=("-fsanitize=thread",), skip_without_runtime=True)
    _run(exe, tmp_path, (), ("--bgzf",))


ENTRY_POINTS = ["epgio_open_table_ex", "epgio_open_table_into", "epgio_open_text", "epgio_write_scores", "epgio_write_states", "epgio_write_metrics",
                "epgio_parse_locations", "epgio_row_sums_f32", "epgio_rolling_max_f64", "epgio_count_newlines", "epgio_gzip_fast"]
# the shapes of the sweep on which these run more than one worker
MULTI_THREADED = ["epgio_open_table_ex", "epgio_open_table_into", "epgio_write_scores", "epgio_write_states", "epgio_write_metrics",
                  "epgio_parse_locations", "epgio_row_sums_f32", "epgio_rolling_max_f64", "epgio_count_newlines"]


def test_a_refused_allocation_is_an_error_return_in_every_entry_point(tmp_path):
    """operator new throws std::bad_alloc at the k-th allocation of a call, k = 1, 2, ... until a call completes with no allocation
    refused: the sweep leaves out no k below that first success.  Every call succeeds with the right result or returns its failure
    value with a message; after a failed one no thread is left in the census, no file handle is open that was not before, and the
    same call succeeds (the program checks all of that and would exit with 1, or not at all, otherwise).  Here: every entry point saw
    at least one failure and one success, and where the call runs several workers at least one allocation was refused after the
    first of them had started -- in a worker, or in the caller on its way to start the next one."""
    exe = build_program(tmp_path, "io_check_new", SOURCES, ["-lz"], flags=("-DIO_CHECK_FAIL_NEW",))
    out, = _run(exe, tmp_path)
    seen = {}
    for name, failed, succeeded, late in re.findall(r"io_check: sweep (\w+)[^:]*: (\d+) failed, (\d+) succeeded, (\d+) after the first worker had started", out):
        f, s, l = seen.get(name, (0, 0, 0))
        seen[name] = (f + int(failed), s + int(succeeded), l + int(late))
    print(out)
    assert sorted(seen) == sorted(ENTRY_POINTS), sorted(seen)
    for name, (failed, succeeded, late) in seen.items():
        assert failed >= 1 and succeeded >= 1, (name, failed, succeeded)
        assert late >= 1 or name not in MULTI_THREADED, (name, failed, late)
