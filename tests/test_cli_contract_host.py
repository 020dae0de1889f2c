"""The `epilogos` command line as a contract (no GPU): which usage error a command line hears of when it trips several families of
checks at once, what has and has not happened by then, that the parent of `--gpus N` never loads torch, and, route by route, which
driver entry point and which STEP 4 are called with how many positional arguments and which keywords -- `host` choices adding none.
Every expectation is a literal recorded from the command line as it was before run.py was reshaped around its run record."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from epilogos_amd import __version__, driver, roiAndVisualPairwise, roiSingle, run, stateByLine as sbl
from tests.test_chromhmm_run_host import _numpy_builder, _states_file, calls  # noqa: F401  (calls: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = "/nonexistent"
CH = ["--chromhmm", "d", "--metadata", "m", "--chromsizes", "c"]
P = ["-m", "paired"]
NEEDS_CHROMHMM = "ERROR: [--chromhmm] is required with [%s]: the option describes a ChromHMM output directory\n"
GROUPINGS_ALONE = "ERROR: [--groupings] names the biosamples of every grouping itself; it cannot be combined with [%s]\n"
ONE_GPU = "ERROR: [--null-draws] greater than 1 runs on one GPU: the exceedance counts of several ranks are not added up yet; use [--gpus 1]\n"

# (command line, its whole output): every one trips two or more of the families chromhmm < null-draws < stage choices < groupings <
# columns < the reference's flags, or two checks of one family; the family that is looked at first speaks.  All exit 0.
PRECEDENCE = [
    (["--fit", "gpu", "--null-draws", "0"], "ERROR: [--null-draws] must be at least 1\n"),
    (["--metadata", "m", "--null-draws", "0"], NEEDS_CHROMHMM % "--metadata"),
    (P + ["--fit", "gpu", "--pvals", "gpu"], "ERROR: [--fit gpu] requires [-n, --null-distribution]: without it nothing is fitted\n"),
    (P + ["-n", "--fit", "gpu", "--null-draws", "3"],
     "ERROR: [--fit gpu] cannot be combined with [--null-draws] greater than 1: empirical p-values need no fit\n"),
    (P + ["-n", "--null-draws", "3", "--gpus", "2"], ONE_GPU),
    (["--metrics", "gpu", "--groupings", G], "ERROR: [--metrics gpu] is only valid in paired mode\n"),
    (["--groupings", G, "--columns", "1", "-i", "x"], GROUPINGS_ALONE % "--columns"),
    (["--groupings", G, "-i", "x"], "ERROR: [--groupings] cannot read the groupings file /nonexistent: No such file or directory\n"),
    (["--roi", "gpu"], "ERROR: [-i, --input-directory] is required in single mode\n"),
    (["--writer", "gpu", "-i", "x", "-o", "o"], "ERROR: [-j, --state-info] is required\n"),
    # one pair per adjacent pair of families: chromhmm | null-draws and null-draws | stage choices are the first two rows,
    # stage choices | groupings the sixth; groupings | columns, twice, and columns | flags, twice:
    (["--groupings", G, "--columns-a", "1"], GROUPINGS_ALONE % "--columns-a"),
    (P + ["--groupings", G, "--columns", "1", "-i", "x"], GROUPINGS_ALONE % "--columns"),
    (["--columns-a", "1"], "ERROR: [--columns-a] and [--columns-b] are only valid in paired mode; single mode takes [--columns]\n"),
    (P + ["--columns", "1"], "ERROR: [--columns] is only valid in single mode; paired mode takes [--columns-a] and [--columns-b]\n"),
    # chromhmm before every other family, and its own order
    (CH + ["-i", "x", "--null-draws", "0"], "ERROR: [--chromhmm] takes the place of the input directories; it cannot be combined with [-i]\n"),
    (["--chromhmm", "d", "--chromsizes", "c", "--fit", "gpu"], "ERROR: [--chromhmm] requires [--metadata]\n"),
    (["--segments", "--metrics", "gpu"], NEEDS_CHROMHMM % "--segments"),
    (["--bin-width", "100", "--groupings", G], NEEDS_CHROMHMM % "--bin-width"),
    (["--keep-matrices", "k", "--columns-a", "1"], NEEDS_CHROMHMM % "--keep-matrices"),
    (["--state-names", "n"], NEEDS_CHROMHMM % "--state-names"),
    (["--metadata", "m", "--chromsizes", "c"], NEEDS_CHROMHMM % "--metadata"),
    (CH + ["--gpus", "2", "--null-draws", "0"],
     "ERROR: [--chromhmm] runs on one GPU: it builds and holds the matrices, sharing them out over several ranks is not done yet; use [--gpus 1]\n"),
    (CH + ["--cache-dir", "k", "--gpus", "2"],
     "ERROR: [--chromhmm] cannot be combined with [--cache-dir]: the matrices are built on the GPU, there is no parsed text to cache\n"),
    # null-draws before the later ones
    (["--null-draws", "0", "--groupings", G], "ERROR: [--null-draws] must be at least 1\n"),
    (["--null-draws", "3", "--columns-a", "1"], "ERROR: [--null-draws] greater than 1 is only valid in paired mode\n"),
    (P + ["--null-draws", "3"], "ERROR: [--null-draws] greater than 1 requires [-n, --null-distribution]\n"),
    (["--null-draws", "0"], "ERROR: [--null-draws] must be at least 1\n"),
    # the stage choices before the later ones
    (["--pvals", "gpu", "--columns-a", "1"], "ERROR: [--pvals gpu] is only valid in paired mode\n"),
    (P + ["--pvals", "gpu"], "ERROR: [--pvals gpu] requires [-n, --null-distribution]: without it no p-value is computed\n"),
    (P + ["-n", "--pvals", "gpu", "--metrics", "gpu", "--columns", "1"],
     "ERROR: [--columns] is only valid in single mode; paired mode takes [--columns-a] and [--columns-b]\n"),
    (["--fit", "gpu"], "ERROR: [--fit gpu] is only valid in paired mode\n"),
    # groupings, columns and the flags
    (["--groupings", G], "ERROR: [-i, --input-directory] is required with [--groupings]\n"),
    (P + ["--groupings", G, "-a", "x", "-i", "y"], GROUPINGS_ALONE % "-a"),
    (P + ["--columns-a", "1"], "ERROR: [--columns-a] and [--columns-b] must be given together\n"),
    (P + ["--columns-a", "1", "--columns-b", "2", "-a", "x"],
     "ERROR: [--columns-a] and [--columns-b] select from [-i, --input-directory]; they cannot be combined with [-a] and [-b]\n"),
    (P + ["--columns-a", "1", "--columns-b", "2"], "ERROR: [-i, --input-directory] is required with [--columns-a] and [--columns-b]\n"),
    (P + ["--columns-a", "1", "--columns-b", "1", "-i", "x"], "ERROR: biosample 1 is in both [--columns-a] and [--columns-b]\n"),
    (["--columns", "0"], "ERROR: [--columns] biosample numbers start at 1, got '0'\n"),
    (P + ["--columns-a", "1-3", "--columns-b", "x", "-i", "d"],
     "ERROR: [--columns-b] malformed biosample list: 'x' is neither a number nor a range\n"),
    (["-i", "x", "-a", "y"], "ERROR: [-a] and [-b] are only valid in paired mode\n"),
    (P + ["-a", "x"], "ERROR: [-a, --directory-one] and [-b, --directory-two] are required in paired mode\n"),
    (P + ["-a", "x", "-b", "y", "-i", "z"], "ERROR: [-i] is only valid in single mode\n"),
    (["-i", "x"], "ERROR: [-o, --output-directory] is required\n"),
    (["-v", "--null-draws", "0"], "Version: %s\n" % __version__),
]
SIDE_EFFECTS = ("EPILOGOS_CACHE_DIR", "EPILOGOS_NUM_CORES")


def _invoke(args, **env):
    return CliRunner().invoke(run.main, [str(a) for a in args], env=env or None)


@pytest.fixture()
def clean(tmp_path, monkeypatch):
    """Relative paths everywhere and none of the variables the command line sets: what it makes or sets shows."""
    monkeypatch.chdir(tmp_path)
    for name in SIDE_EFFECTS + ("WORLD_SIZE", "RANK"):
        monkeypatch.setenv(name, "")                     # (so that what the command line sets is taken back after the test)
        monkeypatch.delenv(name)
    return tmp_path


# ---- (a) precedence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,output", PRECEDENCE, ids=[" ".join(a) for a, _o in PRECEDENCE])
def test_the_family_that_is_looked_at_first_speaks(clean, args, output):
    res = _invoke(args)
    assert (res.output, res.exit_code, res.exception) == (output, 0, None)
    assert not list(clean.iterdir())


def test_a_second_rank_counts_as_a_second_gpu(clean):
    assert _invoke(P + ["-n", "--null-draws", "3"], WORLD_SIZE="2").output == ONE_GPU


def test_the_state_file_is_read_before_the_number_of_gpus_is_looked_at(clean):
    res = _invoke(["-i", "x", "-o", "o", "-j", "j", "--gpus", "-2"])
    assert res.output == "" and res.exit_code == 1 and isinstance(res.exception, FileNotFoundError)
    assert not list(clean.iterdir())


# ---- (b) what has happened by then ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [a for a, _o in PRECEDENCE], ids=[" ".join(a) for a, _o in PRECEDENCE])
def test_a_usage_error_makes_no_directory_and_sets_no_variable(clean, args):
    """The same command lines with an output directory, a cache directory and a core budget added: they still end in a usage error
    of the flag checks (no state file is named), before the first of the three is made or set."""
    res = _invoke(args + ["-o", "o", "--cache-dir", "cache", "-c", "4"])
    assert res.exit_code == 0 and res.output.count("\n") == 1 and res.output.startswith("Version:" if "-v" in args else "ERROR: ")
    assert not list(clean.iterdir()) and not [n for n in SIDE_EFFECTS if n in os.environ]


def _matrix_dir(d, S=5, N=6):
    d.mkdir(parents=True)
    rng = np.random.default_rng(5)
    for c, R in (("chr1", 41), ("chr2", 17)):
        sbl.write_epgm(d / ("matrix_%s.epgm" % c), rng.integers(0, S, size=(R, N)).astype(np.int8), c, (1, S))
    return d


def test_the_number_of_gpus_is_looked_at_after_the_output_directory_is_made(clean):
    d, states = _matrix_dir(clean / "roadmap"), _states_file(clean / "states.tsv")
    res = _invoke(["-i", d, "-j", states, "-o", "out/deep", "--cache-dir", "cache", "-c", "4", "--gpus", "-2"])
    assert res.output == "ERROR: Number of GPUs must be positive or zero (0 means use all visible GPUs)\n" and res.exit_code == 0
    assert (clean / "out" / "deep").is_dir() and not list((clean / "out" / "deep").iterdir()) and not (clean / "cache").exists()
    assert os.environ["EPILOGOS_CACHE_DIR"] == str((clean / "cache").resolve()) and os.environ["EPILOGOS_NUM_CORES"] == "4"


# ---- (c) the parent of the ranks -----------------------------------------------------------------------------------------------------
IN_A_FRESH_PROCESS = """import sys
from epilogos_amd import run
run._ARGV = sys.argv[1:]
try:
    run.main(args=sys.argv[1:], standalone_mode=False)
except SystemExit as e:
    print("exit", e.code)
assert "torch" not in sys.modules, "torch was imported"
print("torch-free")
"""


def _fresh(args, **env):
    env = dict({k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")}, PYTHONPATH=ROOT, **env)
    res = subprocess.run([sys.executable, "-c", IN_A_FRESH_PROCESS] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_neither_a_usage_error_nor_the_launch_of_the_ranks_loads_torch(clean):
    assert _fresh(P + ["--fit", "gpu", "--pvals", "gpu"]) == PRECEDENCE[2][1] + "exit None\ntorch-free\n"
    d, states = _matrix_dir(clean / "roadmap"), _states_file(clean / "states.tsv")
    args = ["-l", "-i", d, "-j", states, "-o", clean / "out", "-s", "2"]
    out = _fresh(args[:3] + ["--gpus", "3"] + args[3:], EPILOGOS_LAUNCH_DRYRUN="1")
    assert re.sub(r"--master-port \d+ ", "--master-port PORT ", out) == (
        "%s -m torch.distributed.run --nnodes=1 --nproc-per-node 3 --master-addr 127.0.0.1 --master-port PORT -m epilogos_amd.run %s\n"
        "exit 0\ntorch-free\n" % (sys.executable, " ".join(str(a) for a in args)))
    assert (clean / "out").is_dir() and not list((clean / "out").iterdir())


# ---- (d) the routes ------------------------------------------------------------------------------------------------------------------
SINGLE_BANNER = "\nSTEP 1-3: background counts -> all-reduce -> scores (bin-range partition over 1 GPU(s))\n"
PAIRED_BANNER = "\nSTEP 1-3: background counts over [A|B] -> all-reduce -> scores, null groups, deltas (1 GPU(s))\n"
SINGLE_KW = ["checkStates", "columns", "defer_writes", "device", "keep_temp_scores", "verbose"]
PAIRED_KW = ["checkStates", "defer_writes", "device", "keep_temps", "nullDraws", "verbose"]
AB = ["--columns-a", "1-3", "--columns-b", "4-6"]
# route: (options next to the input, driver entry point, positional arguments, keywords, banner, STEP 4's positional arguments)
ROUTES = {
    "single": ([], "run_single_group", 5, SINGLE_KW, SINGLE_BANNER, 7),
    "single --columns": (["--columns", "2-5"], "run_single_group", 5, SINGLE_KW, SINGLE_BANNER, 7),
    "paired -a -b": (P, "run_paired_groups", 9, PAIRED_KW, PAIRED_BANNER, 11),
    "paired --columns-a --columns-b": (P + AB, "run_paired_columns", 10, PAIRED_KW, PAIRED_BANNER, 11),
    "--groupings": (["--groupings", "g.tsv"], "run_groupings", 9, PAIRED_KW,
                    "\nSTEP 1-3 of 2 grouping(s): background counts -> all-reduce -> scores, from one read of the matrices (1 GPU(s))\n"
                    "\nGrouping 1 of 2: left\n", 7),
    "--chromhmm": (P + AB, "run_groupings", 9, sorted(PAIRED_KW + ["flat", "resident"]), PAIRED_BANNER, 11),
}


class _Stop(Exception):
    pass


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_calls_its_driver_and_its_step4_as_it_always_did(clean, request, monkeypatch, route):
    """The drivers are stood in for by their results (none are needed: STEP 4 is stopped as it is entered); the call must still fit
    the real entry point's signature."""
    options, entry, npos, keywords, banner, step4_npos = ROUTES[route]
    monkeypatch.setenv("EPILOGOS_EARLY_READERS", "0")
    states = _states_file(clean / "states.tsv")
    (clean / "g.tsv").write_text("left\t1-3\nright\t4-6\n")
    if route == "--chromhmm":
        d, meta, sizes, _mats = request.getfixturevalue("calls")
        _numpy_builder(monkeypatch)
        inputs = ["--chromhmm", d, "--metadata", meta, "--chromsizes", sizes]
    elif route == "paired -a -b":
        inputs = ["-a", _matrix_dir(clean / "A" / "roadmap"), "-b", _matrix_dir(clean / "B" / "roadmap")]
    else:
        inputs = ["-i", _matrix_dir(clean / "roadmap")]
    paired = "-m" in options
    seen = []

    def stand_in(name, real, result):
        def called(*a, **k):
            inspect.signature(real).bind(*a, **k)
            seen.append((name, len(a), sorted(k)))
            return result()
        return called
    results = (lambda: (x for x in [("left", None, {}, {})])) if entry == "run_groupings" else (lambda: (None, {}))
    monkeypatch.setattr(driver, entry, stand_in(entry, getattr(driver, entry), results))

    def stop():
        raise _Stop()
    for module in (roiSingle, roiAndVisualPairwise):
        monkeypatch.setattr(module, "mainFromArrays", stand_in(module.__name__.rsplit(".", 1)[1], module.mainFromArrays, stop))
    step4 = "roiAndVisualPairwise" if paired else "roiSingle"
    args = inputs + ["-j", states, "-o", "out", "-w", "3", "--null-seed", "7"] + options
    for k, extra in enumerate(([], ["--writer", "host", "--roi", "host", "--fit", "host", "--pvals", "host", "--metrics", "host"])):
        res = _invoke(args + extra)
        assert isinstance(res.exception, _Stop), res.output
        assert seen[2 * k:] == [(entry, npos, keywords), (step4, step4_npos, [])]
        assert banner + "\nSTEP 4: " in res.output and res.output.count("STEP 1-3") == 1
    gpu = ["--writer", "gpu", "--roi", "gpu"] + (["-n", "--fit", "gpu", "--pvals", "gpu", "--metrics", "gpu"] if paired else [])
    res = _invoke(args + gpu)
    assert isinstance(res.exception, _Stop), res.output
    assert seen[4:] == [(entry, npos, sorted(keywords + ["writer"])),
                        (step4, step4_npos, ["fit", "metrics", "pvals", "roi", "seed"] if paired else ["roi"])]
