"""`python -m epilogos_amd.similaritySearch_run` -- similarity search, the option surface of the reference's
epilogos/similaritySearch_run.py (click options :72-111, main :112-140, buildSimSearch :143-219, querySimSearch :237-285, block
sizes :288-345).  -b runs the three stages in this process (STEP 2 on the GPU) instead of submitting SLURM jobs: -j, -p, -t,
--mm-mem, --calc-mem and --write-mem are accepted and ignored, as the `epilogos` command does with its SLURM options; -c caps
the host thread pools (torch's; the process is not pinned).  `--gpus N` (cli(), not an option of main: main's options are the
reference's) splits STEP 2 over N GPUs of the node instead: one child process per GPU, each running the module's argv interface
(the reference's SLURM job) on its contiguous share of the ROIs, while this process stays GPU-free and runs STEP 1 and 3.
`--step1 gpu` (cli() again; default `host`) picks the salient regions on the GPU instead (similaritySearch_step1.py: the same files);
with --gpus N > 1 as one fresh child process on GPU 0 that finishes before STEP 2's children start.
-q writes one similarity_search_region_*_recs.bed per query region: with -m, for the regions found in a built simsearch.bed.gz (the
reference's lookup); with -s and no -m, for ANY region, searched live on the GPU against the scores file
(similaritySearch_query.py)."""
import os
import re
import signal
import subprocess
import sys
import tempfile
import threading
from pathlib import Path
from time import sleep, time

import click
import numpy as np
import pandas as pd

from .helpers import splitGpusOption

STEP1_CHOICES = ("host", "gpu")
INFLATE_CHOICES = ("host", "gpu")

BLOCK_SIZES_200 = {5000: 1, 10000: 2, 25000: 5, 50000: 10, 75000: 15, 100000: 20}
BLOCK_SIZES_20 = {500: 1, 1000: 2, 2500: 5, 5000: 10, 7500: 15, 10000: 20}


def determineBlockSize200(windowBP):
    if windowBP not in BLOCK_SIZES_200:
        raise ValueError("Error: window size must be either 5000, 10000, 25000, 50000, 75000, or 100000 (in bp)")
    return BLOCK_SIZES_200[windowBP]


def determineBlockSize20(windowBP):
    if windowBP not in BLOCK_SIZES_20:
        raise ValueError("Error: window size must be either 500, 1000, 2500, 5000, 7500, or 10000 (in bp)")
    return BLOCK_SIZES_20[windowBP]


def determineBinSize(scoresPath):
    row1 = pd.read_table(scoresPath, sep="\t", header=None, usecols=[0, 1, 2], nrows=1)
    return int(row1.iloc[0, 2] - row1.iloc[0, 1])


def windowParameters(scoresPath, windowBP):
    """(windowBP, windowBins, blockSize) for the scores file's bin size (reference :173-184)."""
    binSize = determineBinSize(scoresPath)
    if binSize == 200:
        windowBP = 25000 if windowBP == -1 else windowBP
        return windowBP, int(windowBP / 200), determineBlockSize200(windowBP)
    if binSize == 20:
        windowBP = 2500 if windowBP == -1 else windowBP
        return windowBP, int(windowBP / 20), determineBlockSize20(windowBP)
    raise ValueError("Similarity Search is only compatible with bins of size 200bp or 20bp")


def generateRegionArr(query):
    """Query regions as an object array [n, 3] (reference helpers.py:197-221)."""
    if re.fullmatch("chr[a-zA-z\\d]+:[\\d]+-[\\d]+", query):
        chrom, rng = query.split(":")
        start, end = rng.split("-")
        return np.array([[chrom, int(start), int(end)]], dtype=object)
    elif Path(query).is_file():
        return pd.read_table(Path(query), sep="\t", header=None, usecols=[0, 1, 2]).to_numpy(dtype=object)
    raise ValueError("Please input valid query (region formatted as chr:start-end"
                     + "or path to bed file containing query regions)")


def buildSimSearch(scoresPath, outputDir, windowBP, nJobs, nCores, nDesiredMatches, filterState, filterScore, gpus=1, step1="host", inflate="host"):
    """STEP 1-3.  gpus > 1: STEP 2 as that many child processes, one per GPU (runChildren); nJobs (-j) is ignored either way.
    step1 "gpu": STEP 1 on the GPU (similaritySearch_step1), in this process with one GPU, as one child process (step1Job) with
    more: this process then stays GPU-free.  inflate "gpu" (with step1 "gpu" only): STEP 1 inflates a BGZF scores file on the device."""
    from . import similaritySearch_calc, similaritySearch_max_mean, similaritySearch_write
    if step1 not in STEP1_CHOICES:
        raise ValueError("step1 must be one of %s, not %r" % (", ".join(STEP1_CHOICES), step1))
    if inflate not in INFLATE_CHOICES or (inflate == "gpu" and step1 != "gpu"):
        raise ValueError("inflate must be one of %s (gpu only with step1 gpu), not %r" % (", ".join(INFLATE_CHOICES), inflate))
    more = {"inflate": inflate} if inflate != "host" else {}                  # `host` adds nothing to any call
    print("\n\n\n        Building Similarity Search Results...", flush=True)
    windowBP, windowBins, blockSize = windowParameters(scoresPath, windowBP)
    if gpus > 1:
        checkDevices(gpus)                       # before STEP 1, which takes minutes on a whole genome
    elif nCores > 0:                             # the host thread pools (the reference's -c sized its worker pool); no pinning
        import torch
        torch.set_num_threads(nCores)
    print("\n        STEP 1: Salient Region Selection", flush=True)
    if step1 == "host":
        similaritySearch_max_mean.main(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore)
    elif gpus > 1:
        runChildren([step1Job(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore, nCores, **more)], step="STEP 1")
    else:
        from . import similaritySearch_step1
        similaritySearch_step1.main(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore, **more)
    print("\n        STEP 2: Similarity Search Calculation", flush=True)
    if gpus > 1:
        for stale in Path(outputDir).glob("simsearch_indices_*.npy"):     # an earlier build's: STEP 3 would merge them in
            os.remove(stale)
        print("Splitting the regions over %d GPU processes..." % gpus, flush=True)
        try:
            runChildren(childJobs(outputDir, windowBins, blockSize, nCores, nDesiredMatches, gpus))
        except BaseException:                    # the children that finished wrote theirs: a later build must not merge them
            for part in Path(outputDir).glob("simsearch_indices_*.npy"):
                os.remove(part)
            raise
    else:
        similaritySearch_calc.main(outputDir, windowBins, blockSize, nCores, nDesiredMatches, 1, 0)
    print("\n        STEP 3: Writing results", flush=True)
    similaritySearch_write.main(outputDir, windowBins, blockSize, gpus, nDesiredMatches)


def checkDevices(gpus):
    """Refuse more children than visible GPUs (counted without torch: this process stays GPU-free), in the words of the
    `epilogos` command; EPILOGOS_DIST_BACKEND=gloo lets them share the GPUs (child i on device i % count)."""
    from . import run
    count = run._visible_gpus()
    if gpus > count and not os.environ.get("EPILOGOS_DIST_BACKEND", ""):
        raise SystemExit("ERROR: rank %d of this node has no GPU: %d rank(s) were started for %d usable device(s) "
                         "(--gpus / *_VISIBLE_DEVICES)" % (count, gpus, count))


def childJobs(outputDir, windowBins, blockSize, nCores, nDesiredMatches, gpus):
    """[(argv, env)] of the STEP 2 children: child i runs `python -m epilogos_amd.similaritySearch_calc` (the reference's SLURM
    job interface) for processTag i of nJobs = gpus, on GPU LOCAL_RANK = i, with an equal share of the host thread budget
    (the node's cores, capped by -c as the `epilogos` command's host budget is) as OMP_NUM_THREADS and nCores."""
    from ._io import node_cores
    budget = min(nCores, node_cores()) if nCores > 0 else node_cores()
    share = max(1, budget // gpus)
    root = str(Path(__file__).resolve().parents[1])
    jobs = []
    for i in range(gpus):
        env = dict(os.environ)
        env["LOCAL_RANK"] = str(i)
        env["OMP_NUM_THREADS"] = str(share)
        env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        argv = [sys.executable, "-m", "epilogos_amd.similaritySearch_calc", str(Path(outputDir).resolve()), str(windowBins),
                str(blockSize), str(share), str(nDesiredMatches), str(gpus), str(i)]
        jobs.append((argv, env))
    return jobs


def step1Job(outputDir, scoresPath, windowBins, blockSize, windowBP, filterState, filterScore, nCores, inflate="host"):
    """(argv, env) of the STEP 1 child of a `--gpus N --step1 gpu` build: `python -m epilogos_amd.similaritySearch_step1` on GPU
    LOCAL_RANK = 0, with the whole host thread budget (it runs alone, before STEP 2's children)."""
    from ._io import node_cores
    budget = min(nCores, node_cores()) if nCores > 0 else node_cores()
    root = str(Path(__file__).resolve().parents[1])
    env = dict(os.environ)
    env["LOCAL_RANK"] = "0"
    env["OMP_NUM_THREADS"] = str(budget)
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    argv = [sys.executable, "-m", "epilogos_amd.similaritySearch_step1", str(Path(outputDir).resolve()), str(Path(scoresPath).resolve()),
            str(windowBins), str(blockSize), str(windowBP), str(filterState), str(filterScore)]
    if inflate != "host":
        argv += ["--inflate", inflate]
    return argv, env


def _stop(procs, grace=10.0):
    """SIGTERM, up to `grace` seconds for all of them together, then SIGKILL."""
    for p in procs:
        if p.poll() is None:
            p.terminate()
    end = time() + grace
    for p in procs:
        try:
            p.wait(timeout=max(0.0, end - time()))
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()


def _status(rc):
    if rc < 0:
        try:
            return "was killed by signal %s (%d)" % (signal.Signals(-rc).name, -rc)
        except ValueError:
            return "was killed by signal %d" % -rc
    return "exited with status %d" % rc


def runChildren(jobs, poll=0.05, tail=20, step="STEP 2"):
    """Start every (argv, env) job, wait for all of them, and pass their stderr on.  The first that fails ends the build:
    the others are stopped (_stop) and SystemExit names the child, its status and the last lines of its stderr.  A failed
    child is never started again.  `step` names the children's step in that message.  A SIGTERM to this process ends the build the same way (the children are stopped)."""
    procs, errs = [], []

    def terminated(signum, _frame):
        raise SystemExit("ERROR: similarity search stopped by %s" % signal.Signals(signum).name)
    main_thread = threading.current_thread() is threading.main_thread()
    previous = signal.signal(signal.SIGTERM, terminated) if main_thread else None
    try:
        for argv, env in jobs:
            errs.append(tempfile.TemporaryFile())
            procs.append(subprocess.Popen(argv, env=env, stderr=errs[-1]))
        running = set(range(len(procs)))
        while running:
            for i in sorted(running):
                rc = procs[i].poll()
                if rc is None:
                    continue
                running.discard(i)
                errs[i].seek(0)
                err = errs[i].read().decode(errors="replace")
                if rc != 0:
                    _stop([procs[j] for j in running])
                    last = "\n".join(err.splitlines()[-tail:])
                    raise SystemExit("ERROR: similarity search %s child %d of %d %s; STEP 3 is skipped: no simsearch.bed.gz "
                                     "was written.%s" % (step, i, len(procs), _status(rc),
                                                         "\nLast lines of its stderr:\n" + last if last else ""))
                if err:
                    sys.stderr.write(err)
            if running:
                sleep(poll)
    finally:
        _stop(procs)                             # nothing outlives the build (an error or an interrupt in this process)
        for f in errs:
            f.close()
        if main_thread:
            signal.signal(signal.SIGTERM, signal.SIG_DFL if previous is None else previous)


def querySimSearch(query, simSearchPath, outputDir):
    print("\n\n\n        Reading in data...", flush=True); readTime = time()
    queryArr = generateRegionArr(query)
    matchesDF = pd.read_table(Path(simSearchPath), sep="\t", header=None)
    print("            Time:", format(time() - readTime, '.0f'), "seconds\n", flush=True)
    print("        Querying regions...", flush=True)
    for chrom, start, end in queryArr:
        index = np.where((matchesDF.iloc[:, 0] == chrom) & (matchesDF.iloc[:, 1] >= start) & (matchesDF.iloc[:, 2] <= end))[0]
        if index.size > 0:
            index = index[0]
            regionChr, regionStart, regionEnd = matchesDF.iloc[index, :3]
            outfile = Path(outputDir) / "similarity_search_region_{}_{}_{}_recs.bed".format(regionChr, regionStart, regionEnd)
            recs = matchesDF.iloc[index, 3][2:-2].split('", "')[1:]
            with open(outfile, "w+") as f:
                f.write("".join("{0[0]}\t{0[1]}\t{0[2]}\n".format(r.split(":")) for r in recs))
            print("            Found region {}:{}-{} within user query {}:{}-{}".format(regionChr, regionStart, regionEnd, chrom,
                                                                                        start, end))
            print("                See {} for matches\n".format(outfile), flush=True)
        else:
            print("            ValueError: Could not find region in given query range: {}:{}-{}\n".format(chrom, start, end))


@click.command(context_settings=dict(help_option_names=['-h', '--help']))
@click.option("-b", "--build", "buildBool", is_flag=True,
              help="If true builds the similarity search files needed to query regions")
@click.option("-s", "--scores", "scoresPath", type=str, help="Path to scores file to be used in similarity search")
@click.option("-o", "--output-directory", "outputDir", required=True, type=str,
              help="Path to desired similarity search output directory")
@click.option("-w", "--window-bp", "windowBP", type=int, default=-1, show_default=True,
              help="Window size (in BP) on which to perform similarity search [default: 25000]")
@click.option("-j", "--num-jobs", "nJobs", type=int, default=10, show_default=True,
              help="Accepted for compatibility (number of SLURM jobs); the build runs in this process")
@click.option("-c", "--num-cores", "nCores", type=int, default=1, show_default=True,
              help="Host threads for the build's thread pools (the process is not pinned). If set to 0, no cap.")
@click.option("-n", "--num-matches", "nDesiredMatches", type=int, default=100, show_default=True,
              help="Number of matches to be found by simsearch for each query region [default: 100]")
@click.option("-f", "--filter-state", "filterState", type=int, default=-1,
              help="If the max signal within a region is from the filter state, the region is removed from the region "
                   + "list. If set to 0, filtering is not done. [default: last state]")
@click.option("--filter-score", "filterScore", type=float, default=-1,
              help="If the max signal within a region is less than the filter score, the region is removed from the "
                   + "region list. [default: -1 == no filtering]")
@click.option("-p", "--partition", "partition", type=str, help="Accepted for compatibility (SLURM partition); ignored")
@click.option("-t", "--tag", "jobTag", type=str, default="", help="Accepted for compatibility (SLURM job tag); ignored")
@click.option("--mm-mem", "mmMem", type=str, default=10000, help="Accepted for compatibility (SLURM memory); ignored")
@click.option("--calc-mem", "calcMem", type=int, default=50000, help="Accepted for compatibility (SLURM memory); ignored")
@click.option("--write-mem", "writeMem", type=int, default=5000, help="Accepted for compatibility (SLURM memory); ignored")
@click.option("-q", "--query", "query", type=str, default="",
              help="Query region formatted as chr:start-end or path to tab-separated bed file containing query regions")
@click.option("-m", "--matches-file", "simSearchPath", type=str,
              help="Path to previously built simsearch.bed.gz file to be queried for matches (without it, -q searches the "
                   + "region live against the -s scores file)")
def main(buildBool, scoresPath, outputDir, windowBP, nJobs, nCores, nDesiredMatches, filterState, filterScore,
         partition, jobTag, mmMem, calcMem, writeMem, query, simSearchPath):
    if not buildBool and query == "":
        raise ValueError("Either -b or -q flag must be used to run simsearch")
    elif buildBool and query != "":
        raise ValueError("Both -b and -q flags cannot be used at the same time")
    gpus = (click.get_current_context().obj or {}).get("gpus")        # cli()'s --gpus: None when not given
    if gpus is not None and query != "":
        raise click.UsageError("--gpus applies to -b only: query mode does not use a GPU")
    step1 = (click.get_current_context().obj or {}).get("step1")      # cli()'s --step1: None when not given
    if step1 is not None and query != "":
        raise click.UsageError("--step1 applies to -b only: query mode builds no index")
    inflate = (click.get_current_context().obj or {}).get("inflate")  # cli()'s --inflate: None when not given
    if inflate is not None and query != "" and scoresPath is None:
        raise click.UsageError("--inflate applies to -q with -s (and to -b --step1 gpu): -q -m reads no scores file")
    if inflate is not None and buildBool and step1 != "gpu":
        raise click.UsageError("--inflate applies to -b only with --step1 gpu: the host's STEP 1 reads the scores file with pandas")
    if query != "" and simSearchPath is None and scoresPath is None:
        raise click.UsageError("-q needs either -m simsearch.bed.gz (look the region up in a built index) or -s scores.txt.gz "
                               "(search the region live on the GPU)")
    outputDir = Path(outputDir)
    if not outputDir.exists():
        outputDir.mkdir(parents=True)
    if not outputDir.is_dir():
        raise NotADirectoryError("Given path is not a directory: {}".format(str(outputDir)))
    if buildBool:
        buildSimSearch(scoresPath, outputDir, windowBP, nJobs, nCores, nDesiredMatches, filterState, filterScore,
                       gpus=1 if gpus is None else gpus, step1="host" if step1 is None else step1,
                       **({"inflate": inflate} if inflate not in (None, "host") else {}))
    elif simSearchPath is not None:
        querySimSearch(query, simSearchPath, outputDir)
    else:
        from . import similaritySearch_query
        similaritySearch_query.liveQuery(query, scoresPath, outputDir, windowBP, nDesiredMatches,
                                         **({"inflate": inflate} if inflate not in (None, "host") else {}))


def resolveGpus(value):
    """A --gpus value as written -> the number of GPU processes (0: every visible GPU, counted without torch)."""
    from . import run
    from .helpers import gpusCount
    n = gpusCount(value)
    return run._visible_gpus() if n == 0 else n


def splitOption(argv, name):
    """`name V` / `name=V`, anywhere in an argument list -> (V as written, the last one given; None when there is none; "" for a
    trailing `name`) and the list without them (splitGpusOption's rule)."""
    value, out, skip = None, [], False
    for a in argv:
        if skip:
            value, skip = a, False
        elif a == name:
            value, skip = "", True
        elif a.startswith(name + "="):
            value = a[len(name) + 1:]
        else:
            out.append(a)
    return value, out


def splitStep1Option(argv):
    """splitOption for `--step1`."""
    return splitOption(argv, "--step1")


def splitInflateOption(argv):
    """splitOption for `--inflate`."""
    return splitOption(argv, "--inflate")


def cli(argv=None):
    """`python -m epilogos_amd.similaritySearch_run`: main with `--gpus N` / `--gpus=N`, `--step1 {host,gpu}` and `--inflate {host,gpu}`
    taken out of the arguments first (main's click options stay the reference's); the values reach main through click's ctx.obj."""
    argv = sys.argv[1:] if argv is None else list(argv)
    value, rest = splitGpusOption(argv)
    step1, rest = splitStep1Option(rest)
    inflate, rest = splitInflateOption(rest)
    try:
        gpus = None if value is None else resolveGpus(value)
        if step1 is not None and step1 not in STEP1_CHOICES:
            raise click.UsageError("--step1 takes one of %s, not %r" % (", ".join(STEP1_CHOICES), step1))
        if inflate is not None and inflate not in INFLATE_CHOICES:
            raise click.UsageError("--inflate takes one of %s, not %r" % (", ".join(INFLATE_CHOICES), inflate))
    except click.UsageError as e:
        e.show()
        sys.exit(e.exit_code)
    main.main(args=rest, prog_name="python -m epilogos_amd.similaritySearch_run", obj={"gpus": gpus, "step1": step1, "inflate": inflate})


if __name__ == "__main__":
    cli()
