"""`epilogos` command line for the MI355X engine: the option surface of the reference's epilogos/run.py
(click options :18-73, checkFlags :328-375, checkArguments :378-451, fileTag/paths :158-165) for STEP 1-3.
The per-chromosome SLURM submission (run.py:454-585) is replaced by a bin-range partition across the GPUs of the
node: `--gpus N` starts one process per GPU (a child `python -m torch.distributed.run`, started before this process
touches a GPU) the way the reference's one command fans out over SLURM by itself; a process that finds itself under
torch.distributed.run (WORLD_SIZE set) joins the group.  Console script: `epilogos` (pyproject.toml -> run:cli).  Single mode
also runs STEP 4 (regionsOfInterest_*.txt, epilogos_amd/roiSingle.py); paired mode runs the STEP 4 of
epilogos_amd/roiAndVisualPairwise.py (pairwiseMetrics, regionsOfInterest, significantLoci; no figures).
`--chromhmm DIR --metadata FILE --chromsizes FILE` takes the place of `-i`: the matrices are built on the GPU from ChromHMM output by
epilogos-prep's own generator (preprocess.iter_matrices) and scored where they sit (driver.run_groupings(resident=...)); the run
sees them as the files matrix_{chr}.epgm of a directory named like DIR."""
import os
import re
import sys
import time as _time
from pathlib import Path, PurePath

_T_START = _time.time()

import click

from . import __version__
from .helpers import getNumStates, parseColumns


def _natural_key(p):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", Path(p).name)]


def checkArguments(mode, saliency, inputDirPath, inputDirPath2, outputDirPath, numProcesses, numStates, quiescentState,
                   groupSize, numTrials=101, samplingSize=100000, roiWidth=0):
    """Reference run.py:378-451; same exceptions and messages."""
    if mode == "paired" and saliency == 3:
        raise ValueError("Paired epilogos supports only a saliency of 1 or 2")
    if saliency not in (1, 2, 3):
        raise ValueError("Please ensure that saliency metric is either 1, 2, or 3")
    for d in [inputDirPath] + ([inputDirPath2] if mode == "paired" else []):
        if not d.exists():
            raise FileNotFoundError("Given path does not exist: {}".format(str(d)))
        if not d.is_dir():
            raise NotADirectoryError("Given path is not a directory: {}".format(str(d)))
        if not list(d.glob("*")):
            raise OSError("Ensure that directory is not empty: {}".format(str(d)))
    if outputDirPath == inputDirPath:
        print("ERROR: Output directory cannot be the same as the input directory")
        sys.exit()
    if not outputDirPath.exists():
        outputDirPath.mkdir(parents=True, exist_ok=True)       # every rank gets here; the first one creates it
    if not outputDirPath.is_dir():
        raise NotADirectoryError("Given path is not a directory: {}".format(str(outputDirPath)))
    if numProcesses < 0:
        print("ERROR: Number of cores must be positive or zero (0 means use all cores)")
        sys.exit()
    if numTrials <= 0:
        print("ERROR: Number of trials must be greater than zero")
        sys.exit()
    if samplingSize <= 0:
        print("ERROR: Sampling size must be greater than zero")
        sys.exit()
    if roiWidth < 0:
        print("ERROR: Group size value must be greater than 0")
        sys.exit()
    if quiescentState >= numStates:
        print("ERROR: Quiescent state must be a valid state (at most the number of states)")
        sys.exit()
    if groupSize < -1 or groupSize == 0:
        print("ERROR: Group size must be positive")
        sys.exit()


def _check_biosamples_exist(files, top):
    """The command line's pre-check of column groups: biosample top + 1, the largest asked for, is a column of every file."""
    from . import driver
    for f in files:
        try:
            n = driver._columns_of(f)
        except Exception:                                        # (an empty or unreadable file: the parse reports it, or it has no rows)
            continue
        if n and top >= n:
            print("ERROR: biosample {} is not in {}: the file has {} biosample columns".format(top + 1, f, n)); sys.exit()


def _check_chromhmm_flags(mode, chromhmm, metadata, chromsizes, segments, binWidth, stateNames, keepMatrices, inputDirectory,
                          inputDirectory1, inputDirectory2, columnsA, columnsB, groupingsFile, cacheDir, gpus):
    """The usage errors of [--chromhmm] and the options that go with it.  Silent for a command line that has none of them."""
    def refuse(text):
        print("ERROR: [--chromhmm] " + text); sys.exit()
    if chromhmm is None:
        for given, opt in ((metadata, "--metadata"), (chromsizes, "--chromsizes"), (segments or None, "--segments"), (binWidth, "--bin-width"),
                           (stateNames, "--state-names"), (keepMatrices, "--keep-matrices")):
            if given is not None:
                refuse("is required with [{}]: the option describes a ChromHMM output directory".format(opt))
        return
    for given, opt in ((inputDirectory, "-i"), (inputDirectory1, "-a"), (inputDirectory2, "-b")):
        if given is not None:
            refuse("takes the place of the input directories; it cannot be combined with [{}]".format(opt))
    for given, opt in ((metadata, "--metadata"), (chromsizes, "--chromsizes")):
        if given is None:
            refuse("requires [{}]".format(opt))
    for given, opt in ((binWidth, "--bin-width"), (stateNames, "--state-names")):
        if given is not None and not segments:
            refuse("[{}] goes with [--segments]".format(opt))
    if binWidth is not None and binWidth <= 0:
        refuse("the bin width must be positive")
    if mode == "paired" and columnsA is None and columnsB is None and groupingsFile is None:
        refuse("builds one set of matrices: paired mode needs [--columns-a] and [--columns-b], or [--groupings], to name the two groups")
    if cacheDir is not None:
        refuse("cannot be combined with [--cache-dir]: the matrices are built on the GPU, there is no parsed text to cache")
    if gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        refuse("runs on one GPU: it builds and holds the matrices, sharing them out over several ranks is not done yet; "
               "use [--gpus 1]")


def _selects_a_file(datadir, metadata, chromsizes, segments):
    """Whether epilogos-prep's selection rule finds any file of the directory (host only; two files for one biosample raise here
    what they raise there)."""
    from . import segments as segmentFiles, stateByLine
    if segments:
        return bool(segmentFiles.find_segments_named(datadir, metadata)[0])
    return any(files for _chrom, files, _names in stateByLine.iter_calls_named(datadir, metadata, chromsizes))


def _build_resident(chromhmm, metadata, chromsizes, segments, binWidth, stateNames, keepMatrices, numStates, checkStates):
    """[--chromhmm]: the matrices of the ChromHMM output directory, built on the device by epilogos-prep's own generator
    (preprocess.iter_matrices, which prints its progress lines) and kept there.  -> (files, resident): the virtual paths
    `matrix_{chr}.epgm` the run sees them under -- in OUTDIR with [--keep-matrices], where they are then also written, as built --
    in the natural-key order in which [-i] would run those files, and {path: (X, N, Locations)} for driver.run_groupings.
    Without [--check-states] a matrix is handed over as stateByLine.read_epgm would have read its file: what is no state of the
    parser's limit is -1.  A state range outside the model raises what the readers of the files raise.  The matrices must fit on
    the device next to a session by the resident store's own rule, applied once to their total; if not, the run ends here."""
    from . import _io, driver, preprocess, segments as segmentFiles, stateByLine
    _io.set_state_limit(numStates)
    table = segmentFiles.read_state_names(stateNames) if stateNames else None
    outdir = None
    if keepMatrices is not None:
        outdir = Path(keepMatrices)
        outdir.mkdir(parents=True, exist_ok=True)
    resident, ranges = {}, {}
    for chrom, X, N, name, rng, _names, width in preprocess.iter_matrices(chromhmm, metadata, chromsizes, sys.stdout, segments,
                                                                          binWidth or stateByLine.BIN_WIDTH, table):
        path = preprocess.matrix_path(outdir if outdir is not None else "", chrom)
        if outdir is not None:
            stateByLine.write_epgm(path, X[:, :N].contiguous(), name, rng, width)
        if not checkStates and rng[1] > _io.state_limit():       # (a byte is a state value - 1; the pad columns are -1 as built)
            X[(X >= _io.state_limit()) | (X < 0)] = -1
        resident[path] = (X, N, stateByLine.synth_locations(name, 0, X.shape[0], width))
        ranges[path] = rng
        del X
    files = sorted(resident, key=_natural_key)
    for f in files:
        driver._check_range(f, ranges[f], numStates)
    if files:
        nbytes = sum(driver._nbytes(resident[f][0]) for f in files)
        free = driver._device_free(resident[files[0]][0])
        if not driver._ResidentStore.fits(nbytes, free):
            print("ERROR: [--chromhmm] the matrices do not fit on the device next to a run: they are {} bytes and need {} bytes free "
                  "({} x the matrices + {}), {} bytes are free.  Use the two commands instead: epilogos-prep -o MATRICES, then "
                  "epilogos -i MATRICES".format(nbytes, driver._ResidentStore.FREE_FACTOR * nbytes + driver._ResidentStore.FREE_SLACK,
                                                driver._ResidentStore.FREE_FACTOR, driver._ResidentStore.FREE_SLACK, free))
            sys.exit(1)
    return files, resident


def _init_device_and_group(world, under_launcher):
    """Import torch, pick this rank's GPU and join the process group (also a group of one: the collective path is the same code).
    -> torch.device or None."""
    import torch
    device = None
    # EPILOGOS_DIST_BACKEND=gloo lets several ranks share one GPU (testing the multi-rank path on a 1-GPU box)
    dist_backend = os.environ.get("EPILOGOS_DIST_BACKEND", "")
    if torch.cuda.is_available():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if not dist_backend and local >= torch.cuda.device_count():
            raise SystemExit("ERROR: rank %d of this node has no GPU: %d rank(s) were started for %d usable device(s) "
                             "(--gpus / *_VISIBLE_DEVICES)" % (local, int(os.environ.get("LOCAL_WORLD_SIZE", "0") or 0), torch.cuda.device_count()))
        torch.cuda.set_device(local % torch.cuda.device_count() if dist_backend else local)
        device = torch.device("cuda", torch.cuda.current_device())
    if world > 1 or under_launcher:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = dist_backend or ("nccl" if device is not None else "gloo")
        # a collective whose partner never arrives (a rank that died where the launcher cannot see it) must end the job, not
        # hold seven GPUs forever; generous, because a rank legitimately waits while the others still parse their files
        import datetime
        limit = datetime.timedelta(seconds=int(os.environ.get("EPILOGOS_DIST_TIMEOUT", "1800")))
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=device, timeout=limit)
        else:
            dist.init_process_group(backend=backend, timeout=limit)
    return device


@click.command(context_settings=dict(help_option_names=["-h", "--help"]))
@click.option("-m", "--mode", "mode", type=click.Choice(["single", "paired"]), default="single", show_default=True,
              help="single for single group epilogos and paired for 2 group epilogos")
@click.option("-l", "--local", "commandLineBool", is_flag=True,
              help="Run in this process (always the case for the GPU engine; accepted for compatibility)")
@click.option("-i", "--input-directory", "inputDirectory", type=str, help="Directory with one matrix file per chromosome")
@click.option("-a", "--directory-one", "inputDirectory1", type=str, help="First input directory (paired mode)")
@click.option("-b", "--directory-two", "inputDirectory2", type=str, help="Second input directory (paired mode)")
@click.option("-o", "--output-directory", "outputDirectory", type=str, help="Output directory")
@click.option("-j", "--state-info", "stateInfo", type=str, help="State model info file")
@click.option("-s", "--saliency", "saliency", type=int, default=1, show_default=True, help="Saliency level (1, 2, or 3)")
@click.option("-c", "--num-cores", "numProcesses", type=int, default=0, show_default=True,
              help="Upper bound on the host cores the job uses for parsing, writing and STEP 4 (0 = all it may use); shared out "
                   "over the ranks of --gpus")
@click.option("-x", "--exit", "exitBool", is_flag=True, help="SLURM-only flag; accepted and ignored")
@click.option("-d", "--diagnostic-figures", "diagnosticBool", is_flag=True, help="Figures are not produced; accepted and ignored")
@click.option("-t", "--num-trials", "numTrials", type=int, default=101, show_default=True,
              help="Number of gennorm fits of the null distances (paired mode with -n); accepted and unused with --null-draws K > 1")
@click.option("-z", "--sampling-size", "samplingSize", type=int, default=100000, show_default=True,
              help="Size of the null sub-sample of each fit (paired mode with -n); accepted and unused with --null-draws K > 1")
@click.option("-q", "--quiescent-state", "quiescentState", type=int, default=-1,
              help="1-based quiescent state for paired filtering; 0 disables it [default: last state]")
@click.option("-g", "--group-size", "groupSize", type=int, default=-1, show_default=True,
              help="Size of the shuffled null groups in paired mode (default: the input group sizes)")
@click.option("-v", "--version", "version", is_flag=True, help="Print the version and exit")
@click.option("-p", "--partition", "partition", type=str, help="SLURM-only flag; accepted and ignored")
@click.option("-n", "--null-distribution", "pvalBool", is_flag=True,
              help="Paired mode: fit the null distances and report p-values instead of z-scores")
@click.option("-w", "--roi-width", "roiWidth", type=int, default=0, help="Bins per region of interest [default: 50 single, 125 paired]")
@click.option("-f", "--file-tag", "fileTag", type=str, default="null",
              help="Tag appended to output filenames [default: input-directory_saliency]")
@click.option("--exp-freq-mem", "expFreqMem", type=int, default=20000, help="SLURM-only; ignored")
@click.option("--exp-comb-mem", "expCombMem", type=int, default=8000, help="SLURM-only; ignored")
@click.option("--score-mem", "scoreMem", type=int, default=40000, help="SLURM-only; ignored")
@click.option("--roi-mem", "roiMem", type=int, default=-1, help="SLURM-only; ignored")
@click.option("--null-seed", "nullSeed", type=int, default=None, help="Seed for the paired-mode null shuffles (default: random)")
@click.option("--null-draws", "nullDraws", type=int, default=1, show_default=True,
              help="Paired mode with -n: draw every bin's null groups K times and report empirical p-values, "
                   "(1 + #{pooled null distances >= |distance|}) / (1 + K x non-quiescent bins), instead of fitting a distribution "
                   "(no fit: -t and -z are unused); one GPU only.  1: one draw and the fit")
@click.option("--fit", "fit", type=click.Choice(["host", "gpu"]), default="host", show_default=True,
              help="Paired mode with -n: where the [-t] generalised-normal fits of the null distances run.  host: scipy, on [-c] cores, "
                   "sub-samples from OS entropy.  gpu: on the device, sub-samples seeded from [--null-seed]: two runs with the same seed "
                   "write the same p-values")
@click.option("--pvals", "pvals", type=click.Choice(["host", "gpu"]), default="host", show_default=True,
              help="Paired mode with -n: where the p-values of the bins and their Benjamini-Hochberg adjustment are computed.  host: scipy "
                   "and numpy.  gpu: on the device (with [--null-draws] greater than 1 the adjustment only); the adjusted values are the "
                   "host's bit for bit, the p-values agree to about 1e-13")
@click.option("--writer", "writer", type=click.Choice(["host", "gpu"]), default="host", show_default=True,
              help="Where scores_*.txt.gz (single mode) and pairwiseDelta_*.txt.gz (paired mode) are formatted and compressed.  host: the "
                   "native writer threads (EPILOGOS_GZIP_LEVEL and EPILOGOS_BGZF are its settings).  gpu: on the device, always as BGZF; "
                   "only compressed bytes come back, and paired mode downloads no deltas.  The decompressed bytes are the same")
@click.option("--roi", "roi", type=click.Choice(["host", "gpu"]), default="host", show_default=True,
              help="Where STEP 4 searches the regions of interest.  host: sort and greedy walk in numpy.  gpu: rolling maximum, rank and "
                   "pick of the windows on the device; regionsOfInterest_*.txt is the same file.  A region above 1024 bins [-w] is "
                   "searched on the host")
@click.option("--metrics", "metrics", type=click.Choice(["host", "gpu"]), default="host", show_default=True,
              help="Paired mode: where pairwiseMetrics_*.txt.gz is formatted and compressed.  host: the native writer threads "
                   "(EPILOGOS_GZIP_LEVEL and EPILOGOS_BGZF are its settings).  gpu: on the device, always as BGZF, from the device's own "
                   "p-values with [--pvals gpu].  The decompressed bytes are the same")
@click.option("--gpus", "gpus", type=int, default=1, show_default=True,
              help="GPUs of this node to split the genome over (0 = all visible); replaces the SLURM fan-out of the reference")
@click.option("--cache-dir", "cacheDir", type=str, default=None,
              help="Keep parsed input matrices (int8 + coordinates) here; later runs on the same files skip the text parse")
@click.option("--columns", "columns", type=str, default=None,
              help="Single mode: score only these biosamples of the matrices: 1-based numbers and ranges (1-379,401) or @file")
@click.option("--columns-a", "columnsA", type=str, default=None,
              help="Paired mode with -i: the biosamples of group A (as --columns); the matrices are read once for both groups")
@click.option("--columns-b", "columnsB", type=str, default=None, help="Paired mode with -i: the biosamples of group B")
@click.option("--check-states", "checkStates", is_flag=True,
              help="Census every input matrix on the GPU and stop after STEP 1, before anything is written, if a byte of it is "
                   "not a state of the model; the message names the first such byte (file, row, biosample, value)")
@click.option("--groupings", "groupingsFile", type=str, default=None,
              help="Score many biosample groupings of the matrices of [-i] in one run: a tab-separated file with one line per grouping, "
                   "NAME<TAB>SPEC (single mode) or NAME<TAB>SPEC_A<TAB>SPEC_B (paired mode), SPEC as --columns takes it.  Every file is "
                   "read and uploaded once; grouping NAME is written to OUTPUT/NAME/ as its own --columns command would write it")
@click.option("--chromhmm", "chromhmm", type=str, default=None,
              help="In place of [-i]: score straight from a ChromHMM output directory (the first argument of epilogos-prep).  The state "
                   "matrices are built on the GPU and scored where they sit; no matrix file is written or read.  Needs [--metadata] and "
                   "[--chromsizes]; one GPU")
@click.option("--metadata", "metadata", type=str, default=None, help="With --chromhmm: the biosample table (the second argument of epilogos-prep)")
@click.option("--chromsizes", "chromsizes", type=str, default=None, help="With --chromhmm: the chromosome sizes (the third argument of epilogos-prep)")
@click.option("--segments", "segments", is_flag=True,
              help="With --chromhmm: the directory holds ChromHMM segment files (one *_segments.bed per biosample, whole genome)")
@click.option("--bin-width", "binWidth", type=int, default=None, help="With --chromhmm --segments: the bin width in bp  [default: 200]")
@click.option("--state-names", "stateNames", type=str, default=None,
              help="With --chromhmm --segments: a state metadata TSV (one_index, short_name) for labels that are names")
@click.option("--keep-matrices", "keepMatrices", type=str, default=None,
              help="With --chromhmm: also write the matrix_<chr>.epgm files of epilogos-prep here")
def main(mode, commandLineBool, inputDirectory, inputDirectory1, inputDirectory2, outputDirectory, stateInfo, saliency,
         numProcesses, exitBool, diagnosticBool, numTrials, samplingSize, quiescentState, groupSize, version, partition,
         pvalBool, roiWidth, fileTag, expFreqMem, expCombMem, scoreMem, roiMem, nullSeed, nullDraws, gpus, cacheDir, columns, columnsA, columnsB, checkStates,
         groupingsFile, chromhmm, metadata, chromsizes, segments, binWidth, stateNames, keepMatrices, fit="host", pvals="host", writer="host",
         roi="host", metrics="host"):
    """Information-theoretic navigation of multi-tissue functional genomic annotations -- MI355X scoring engine."""
    if version:
        print("Version:", __version__)
        sys.exit()
    # --chromhmm and what goes with it: its own combinations before all others, so that every command line without these options
    # gets today's messages; nothing is read and no directory is made
    _check_chromhmm_flags(mode, chromhmm, metadata, chromsizes, segments, binWidth, stateNames, keepMatrices, inputDirectory,
                          inputDirectory1, inputDirectory2, columnsA, columnsB, groupingsFile, cacheDir, gpus)
    if chromhmm is not None:
        inputDirectory = chromhmm                         # from here on the run's input directory: required-ness, tag, emptiness
    # --null-draws: its own combinations first, so that every command line without it gets today's messages
    if nullDraws < 1:
        print("ERROR: [--null-draws] must be at least 1"); sys.exit()
    if nullDraws > 1 and mode != "paired":
        print("ERROR: [--null-draws] greater than 1 is only valid in paired mode"); sys.exit()
    if nullDraws > 1 and not pvalBool:
        print("ERROR: [--null-draws] greater than 1 requires [-n, --null-distribution]"); sys.exit()
    if nullDraws > 1 and (gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        print("ERROR: [--null-draws] greater than 1 runs on one GPU: the exceedance counts of several ranks are not added up yet; "
              "use [--gpus 1]"); sys.exit()
    # --fit gpu: the same, so that every command line without it gets today's messages
    if fit == "gpu" and mode != "paired":
        print("ERROR: [--fit gpu] is only valid in paired mode"); sys.exit()
    if fit == "gpu" and not pvalBool:
        print("ERROR: [--fit gpu] requires [-n, --null-distribution]: without it nothing is fitted"); sys.exit()
    if fit == "gpu" and nullDraws > 1:
        print("ERROR: [--fit gpu] cannot be combined with [--null-draws] greater than 1: empirical p-values need no fit"); sys.exit()
    # --pvals gpu: the same
    if pvals == "gpu" and mode != "paired":
        print("ERROR: [--pvals gpu] is only valid in paired mode"); sys.exit()
    if pvals == "gpu" and not pvalBool:
        print("ERROR: [--pvals gpu] requires [-n, --null-distribution]: without it no p-value is computed"); sys.exit()
    # --metrics gpu: the same; single mode writes no such file (--roi gpu is valid in both modes)
    if metrics == "gpu" and mode != "paired":
        print("ERROR: [--metrics gpu] is only valid in paired mode"); sys.exit()
    # --groupings: as above, its own combinations and its file's errors before everything else -- nothing is read but that file
    groupings = None
    if groupingsFile is not None:
        from .helpers import parseGroupings
        for given, opt in ((columns, "--columns"), (columnsA, "--columns-a"), (columnsB, "--columns-b"), (inputDirectory1, "-a"),
                           (inputDirectory2, "-b")):
            if given is not None:
                print("ERROR: [--groupings] names the biosamples of every grouping itself; it cannot be combined with [{}]".format(opt))
                sys.exit()
        if inputDirectory is None:
            print("ERROR: [-i, --input-directory] is required with [--groupings]"); sys.exit()
        try:
            groupings = parseGroupings(groupingsFile, mode)
        except ValueError as e:
            print("ERROR: [--groupings] {}".format(e)); sys.exit()
    # column groups: the flag combinations that involve the new options come first, so that every combination without them
    # gets today's message
    pairedColumns = mode == "paired" and (columnsA is not None or columnsB is not None or groupings is not None)
    if mode == "single" and (columnsA is not None or columnsB is not None):
        print("ERROR: [--columns-a] and [--columns-b] are only valid in paired mode; single mode takes [--columns]"); sys.exit()
    if mode == "paired" and columns is not None:
        print("ERROR: [--columns] is only valid in single mode; paired mode takes [--columns-a] and [--columns-b]"); sys.exit()
    if pairedColumns and groupings is None:
        if columnsA is None or columnsB is None:
            print("ERROR: [--columns-a] and [--columns-b] must be given together"); sys.exit()
        if inputDirectory1 is not None or inputDirectory2 is not None:
            print("ERROR: [--columns-a] and [--columns-b] select from [-i, --input-directory]; they cannot be combined with [-a] and [-b]"); sys.exit()
        if inputDirectory is None:
            print("ERROR: [-i, --input-directory] is required with [--columns-a] and [--columns-b]"); sys.exit()
    cols = colsA = colsB = None
    try:
        what = "--columns"
        cols = parseColumns(columns) if columns is not None else None
        if pairedColumns and groupings is None:
            what = "--columns-a"
            colsA = parseColumns(columnsA)
            what = "--columns-b"
            colsB = parseColumns(columnsB)
    except ValueError as e:
        print("ERROR: [{}] {}".format(what, e)); sys.exit()
    if pairedColumns and groupings is None:
        both = sorted(set(colsA.tolist()) & set(colsB.tolist()))
        if both:
            print("ERROR: biosample {} is in both [--columns-a] and [--columns-b]".format(both[0] + 1)); sys.exit()
    # flag combinations (reference run.py:328-375)
    if mode == "single" and inputDirectory is None:
        print("ERROR: [-i, --input-directory] is required in single mode"); sys.exit()
    if mode == "single" and (inputDirectory1 is not None or inputDirectory2 is not None):
        print("ERROR: [-a] and [-b] are only valid in paired mode"); sys.exit()
    if mode == "paired" and not pairedColumns and (inputDirectory1 is None or inputDirectory2 is None):
        print("ERROR: [-a, --directory-one] and [-b, --directory-two] are required in paired mode"); sys.exit()
    if mode == "paired" and not pairedColumns and inputDirectory is not None:
        print("ERROR: [-i] is only valid in single mode"); sys.exit()
    if outputDirectory is None:
        print("ERROR: [-o, --output-directory] is required"); sys.exit()
    if stateInfo is None:
        print("ERROR: [-j, --state-info] is required"); sys.exit()

    if cacheDir:
        os.environ["EPILOGOS_CACHE_DIR"] = str(Path(cacheDir).resolve())
    if numProcesses > 0:                                      # the reference's core budget (run.py:36,148): see _io.host_budget
        os.environ["EPILOGOS_NUM_CORES"] = str(numProcesses)
    numStates = getNumStates(stateInfo)
    quiescentState = numStates - 1 if quiescentState == -1 else quiescentState - 1     # 1-based -> 0-based, 0 -> off
    inputDirPath = Path(inputDirectory if mode == "single" or pairedColumns else inputDirectory1)
    inputDirPath2 = (inputDirPath if pairedColumns else Path(inputDirectory2)) if mode == "paired" else Path("")
    if not PurePath(inputDirPath).is_absolute():
        inputDirPath = Path.cwd() / inputDirPath
    if mode == "paired" and not PurePath(inputDirPath2).is_absolute():
        inputDirPath2 = Path.cwd() / inputDirPath2
    outputDirPath = Path(outputDirectory)
    if not PurePath(outputDirPath).is_absolute():
        outputDirPath = Path.cwd() / outputDirPath
    if groupings is not None and inputDirPath.is_dir() and chromhmm is None:
        # the largest biosample number of the file against every matrix's columns, before the first directory is made
        _check_biosamples_exist(sorted(inputDirPath.glob("*"), key=_natural_key), max(int(c.max()) for g in groupings for c in g[1:]))
    if chromhmm is not None:
        for given, opt in ((metadata, "--metadata"), (chromsizes, "--chromsizes"), (stateNames, "--state-names")):
            if given is not None and not Path(given).is_file():
                print("ERROR: [{}] is not a file: {}".format(opt, given)); sys.exit()
        if inputDirPath.is_dir() and list(inputDirPath.glob("*")) and not _selects_a_file(inputDirPath, metadata, chromsizes, segments):
            # no file of the directory is anybody's: epilogos-prep would leave an empty directory, which [-i] refuses like this
            raise OSError("Ensure that directory is not empty: {}".format(str(inputDirPath)))
    checkArguments(mode, saliency, inputDirPath, inputDirPath2, outputDirPath, numProcesses, numStates, quiescentState,
                   groupSize, numTrials, samplingSize, roiWidth)
    if fileTag == "null":
        fileTag = ("{}_s{}".format(inputDirPath.name, saliency) if mode == "single"
                   else "{0}_A_{0}_B_s{1}".format(inputDirPath.name, saliency) if pairedColumns
                   else "{}_{}_s{}".format(inputDirPath.name, inputDirPath2.name, saliency))
    storedExpPath = outputDirPath / "exp_freq_{}.npy".format(fileTag)

    # --gpus N from a plain start: fan out into one process per GPU (the reference submits its own SLURM jobs,
    # run.py:190-279,454-505) -- as a CHILD process, before this one has imported torch or touched a GPU
    if gpus < 0:
        print("ERROR: Number of GPUs must be positive or zero (0 means use all visible GPUs)"); sys.exit()
    if "WORLD_SIZE" not in os.environ and gpus != 1:
        if gpus == 0:
            gpus = 1 if nullDraws > 1 else _visible_gpus()   # (--null-draws K > 1 runs on one GPU)
        if gpus > 1:
            sys.exit(_launch(gpus, sys.argv[1:] if _ARGV is None else _ARGV))

    # one process per GPU when launched under torch.distributed.run
    world = int(os.environ.get("WORLD_SIZE", "1"))
    under_launcher = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    files = sorted(inputDirPath.glob("*"), key=_natural_key) if chromhmm is None else []    # (--chromhmm: named once they are built)
    files2 = []
    if mode == "paired" and not pairedColumns:
        for file in files:
            if not list(inputDirPath2.glob(file.name)):
                raise FileNotFoundError("File not found: {}".format(str(inputDirPath2 / file.name))
                                        + " Please ensure corresponding files within input directories 1 and 2 have the same name")
            files2.append(next(inputDirPath2.glob(file.name)))
    from . import driver, _io
    if groupings is None and (cols is not None or pairedColumns):     # every biosample asked for must exist in every file
        _check_biosamples_exist(files, max(int(c.max()) for c in ((cols,) if cols is not None else (colsA, colsB))))
    if chromhmm is None and world == 1 and not under_launcher and os.environ.get("EPILOGOS_EARLY_READERS", "1") != "0":
        # A single process: the files' readers start NOW -- inflating needs neither torch nor the GPU, and importing the one and
        # initialising the other takes about a second, which a whole-genome run spent before its first byte was read.  A reader
        # asks for its (page-locked) destination only after its inflate; the session is attached when it exists.
        _io.set_state_limit(numStates)
        jobs = []
        for k, f in enumerate(files):
            jobs += [(f, 0, None)] + ([(files2[k], 0, None)] if files2 else [])
        driver.start_readers_early(jobs, raw=checkStates)     # (--check-states: .epgm bytes reach the device as they are)
    try:
        device = _init_device_and_group(world, under_launcher)
    except BaseException:
        driver.abort_early_readers()
        raise
    rank = int(os.environ.get("RANK", "0"))
    say = print if rank == 0 else (lambda *a, **k: None)
    if os.environ.get("EPILOGOS_TIMING") and rank == 0:
        import time
        print("    [timing] %-34s %7.2f s" % ("imports + device init (since process start)", time.time() - _T_START), flush=True)

    resident = None
    if chromhmm is not None:
        # epilogos-prep's part of the job, its progress lines included, before the run's own output
        t_build = _time.time()
        files, resident = _build_resident(inputDirPath, metadata, chromsizes, segments, binWidth, stateNames, keepMatrices, numStates,
                                          checkStates)
        if os.environ.get("EPILOGOS_TIMING"):
            print("    [timing] %-34s %7.2f s" % ("matrices built on the device", _time.time() - t_build), flush=True)
        if not files:                                            # (segment files that hold no chromosome of the sizes file)
            raise OSError("Ensure that directory is not empty: {}".format(str(inputDirPath)))
        asked = [c for g in groupings for c in g[1:]] if groupings is not None else [c for c in (cols, colsA, colsB) if c is not None]
        top = max([int(c.max()) for c in asked] + [-1])
        for f in files:
            n = resident[f][1]
            if n and top >= n:
                print("ERROR: biosample {} is not in {}: the matrix has {} biosample columns".format(top + 1, f, n)); sys.exit()

    say("State Model =", numStates, " Saliency level =", saliency, " GPUs =", world)
    def step4_single(results, outDir):
        try:
            if rank == 0:
                say("\nSTEP 4: Finding regions of interest", flush=True)
                import time
                t0 = time.perf_counter()
                from .roiSingle import mainFromArrays as roiSingle
                roiSingle(results, outDir, stateInfo, fileTag, outDir / storedExpPath.name, roiWidth if roiWidth else 50, False, **roiOptions())
                if os.environ.get("EPILOGOS_TIMING"):
                    print("    [timing] %-34s %7.2f s" % ("STEP 4", time.perf_counter() - t0), flush=True)
        finally:
            driver.finish_writes()                               # one process: the score text was still being written under STEP 4

    def fitOptions():
        # nothing for --fit host: STEP 4 is called exactly as before.  nullSeed is the run's one seed by now, drawn or given
        return dict(fit="gpu", seed=nullSeed) if fit == "gpu" else {}

    def pvalOptions():
        # nothing for --pvals host, as above
        return dict(pvals="gpu") if pvals == "gpu" else {}

    def roiOptions():
        # nothing for --roi host and --metrics host, as above
        return {**(dict(roi="gpu") if roi == "gpu" else {}), **(dict(metrics="gpu") if metrics == "gpu" else {})}

    def writerOptions():
        # nothing for --writer host, as above: the drivers are called exactly as before
        return dict(writer="gpu") if writer == "gpu" else {}

    def step4_paired(results, outDir):
        if pvalBool and max(numProcesses, 1) > 1 and nullDraws == 1 and fit != "gpu":
            driver.finish_writes()                               # -n -c K forks a pool for the fits: not with writer threads running
        try:
            if rank == 0:
                say("\nSTEP 4: Generating p-values & regions of interest (figures are not produced)", flush=True)
                import time
                t0 = time.perf_counter()
                from .roiAndVisualPairwise import mainFromArrays as roiPairwise
                roiPairwise(results, stateInfo, outDir, fileTag, max(numProcesses, 1), pvalBool, numTrials, samplingSize,
                            outDir / storedExpPath.name, roiWidth if roiWidth else 125, False, **fitOptions(), **pvalOptions(), **roiOptions())
                if os.environ.get("EPILOGOS_TIMING"):
                    print("    [timing] %-34s %7.2f s" % ("STEP 4", time.perf_counter() - t0), flush=True)
        finally:
            driver.finish_writes()

    if mode == "paired" and nullSeed is None:
        import numpy as np
        seed = np.array([int(np.random.SeedSequence().generate_state(1)[0])], dtype=np.int64)
        if world > 1:                                            # every rank must shuffle with the same seed
            import torch
            import torch.distributed as dist
            t = torch.from_numpy(seed)
            t = t.to(device) if device is not None else t
            dist.broadcast(t, src=0)
            seed = t.cpu().numpy()
        nullSeed = int(seed[0])                                  # (--groupings: the one seed of every grouping)
    if groupings is not None or resident is not None:
        # every file is parsed and uploaded once; the groupings then run one after another from the resident matrices, each with
        # STEP 4 and its text complete before the next begins (driver.run_groupings yields as it goes).  --chromhmm: the matrices
        # are resident before the first grouping, and a run without --groupings is one grouping written to the output directory itself
        flat = groupings is None
        if not flat:
            say("\nSTEP 1-3 of %d grouping(s): background counts -> all-reduce -> scores%s, from one read of the matrices (%d GPU(s))"
                % (len(groupings), ", null groups, deltas" if mode == "paired" else "", world))
        elif mode == "single":
            groupings = [("", cols)]
            say("\nSTEP 1-3: background counts -> all-reduce -> scores (bin-range partition over %d GPU(s))" % world)
        else:
            groupings = [("", colsA, colsB)]
            say("\nSTEP 1-3: background counts over [A|B] -> all-reduce -> scores, null groups, deltas (%d GPU(s))" % world)
        runs = driver.run_groupings(files, groupings, numStates, saliency, outputDirPath, fileTag, quiescentState, groupSize, nullSeed,
                                    verbose=False, device=device, keep_temps=False, defer_writes=True, nullDraws=nullDraws,
                                    checkStates=checkStates, **({} if resident is None else {"resident": resident, "flat": flat}),
                                    **writerOptions())
        resident = None                                          # (the store's from here on: gone with the run)
        try:
            for k, g in enumerate(groupings):
                if not flat:
                    say("\nGrouping %d of %d: %s" % (k + 1, len(groupings), g[0]), flush=True)
                name, _q, results, _info = next(runs)
                (step4_single if mode == "single" else step4_paired)(results, outputDirPath / name)
        finally:
            runs.close()
            driver.abort_early_readers()
            driver.finish_writes()
    elif mode == "single":
        from .driver import run_single_group
        say("\nSTEP 1-3: background counts -> all-reduce -> scores (bin-range partition over %d GPU(s))" % world)
        try:
            _, results = run_single_group(files, numStates, saliency, outputDirPath, fileTag, verbose=False, device=device,
                                          keep_temp_scores=False, defer_writes=True, columns=cols, checkStates=checkStates, **writerOptions())
        finally:
            driver.abort_early_readers()                         # (nothing to do once the stage driver has taken them over)
        step4_single(results, outputDirPath)
    else:
        from .driver import run_paired_columns, run_paired_groups
        say("\nSTEP 1-3: background counts over [A|B] -> all-reduce -> scores, null groups, deltas (%d GPU(s))" % world)
        try:
            if pairedColumns:
                _, results = run_paired_columns(files, colsA, colsB, numStates, saliency, outputDirPath, fileTag, quiescentState,
                                                groupSize, nullSeed, verbose=False, device=device, keep_temps=False, defer_writes=True,
                                                nullDraws=nullDraws, checkStates=checkStates, **writerOptions())
            else:
                _, results = run_paired_groups(files, files2, numStates, saliency, outputDirPath, fileTag, quiescentState, groupSize,
                                               nullSeed, verbose=False, device=device, keep_temps=False, defer_writes=True,
                                               nullDraws=nullDraws, checkStates=checkStates, **writerOptions())
        finally:
            driver.abort_early_readers()
        step4_paired(results, outputDirPath)
    from .helpers import flushCacheWrites
    flushCacheWrites()                                           # --cache-dir: files of first-time reads, written in the background
    if os.environ.get("EPILOGOS_TIMING") and rank == 0:
        import time
        print("    [timing] %-34s %7.2f s" % ("end of main (since process start)", time.time() - _T_START), flush=True)
        try:                                                     # what the process holds (and will have to give back at exit)
            st = dict(l.split(":", 1) for l in open("/proc/self/status").read().splitlines() if ":" in l)
            print("    [timing] memory at the end: " + ", ".join("%s %.1f GB" % (k, int(st[k].split()[0]) / 1048576.0)
                                                              for k in ("VmHWM", "VmRSS", "RssAnon", "RssFile", "RssShmem") if k in st), flush=True)
        except (OSError, ValueError):
            pass
    if world > 1 or under_launcher:
        import torch.distributed as dist
        dist.destroy_process_group()


_ARGV = None            # the argument list cli() was called with, when it is not sys.argv[1:]


def _visible_gpus():
    """GPUs this process could use, counted WITHOUT loading torch or touching HIP (the parent of the ranks must stay
    GPU-free): the KFD topology lists every compute node (a GPU has simd_count > 0, a CPU node 0), and the usual
    *_VISIBLE_DEVICES lists narrow it down."""
    n = 0
    try:
        for node in sorted(Path("/sys/class/kfd/kfd/topology/nodes").iterdir()):
            props = dict(l.split()[:2] for l in (node / "properties").read_text().splitlines() if len(l.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except (OSError, ValueError):
        n = 0
    # a container may see the host's whole KFD topology and only some of its render nodes: a GPU without an accessible
    # /dev/dri/renderD* cannot be opened (a rank on it would die in torch.cuda.set_device)
    try:
        usable = len([d for d in Path("/dev/dri").iterdir() if d.name.startswith("renderD") and os.access(d, os.R_OK | os.W_OK)])
        if n and usable:
            n = min(n, usable)
    except OSError:
        pass
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            listed = len([t for t in v.split(",") if t.strip()])
            n = min(n, listed) if n else listed
    return max(n, 1)


def _strip_gpus(argv):
    """The argument list without --gpus (the children learn their number from WORLD_SIZE)."""
    from .helpers import splitGpusOption
    return splitGpusOption(argv)[1]


def _launch_command(gpus, argv, port):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "epilogos_amd.run"] + _strip_gpus(argv)


def _launch(gpus, argv):
    """One process per GPU under torch.distributed.run, as a child of this (GPU-free) process; its exit code is ours."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or gpus) // gpus)))
    root = str(Path(__file__).resolve().parents[1])
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    cmd = _launch_command(gpus, argv, port)
    if os.environ.get("EPILOGOS_LAUNCH_DRYRUN"):
        print(" ".join(cmd))
        return 0
    return subprocess.call(cmd, env=env)


def cli(argv=None):
    """Entry point of the `epilogos` console script and of `python -m epilogos_amd.run`."""
    global _ARGV
    _ARGV = argv
    try:
        main(args=argv, standalone_mode=False)
    except click.exceptions.Abort:
        print("Aborted!", file=sys.stderr)
        _code = 1
    except click.ClickException as e:
        e.show()
        _code = e.exit_code
    except SystemExit as e:                                  # the reference's `print("ERROR ..."); sys.exit()` paths
        _code = e.code if isinstance(e.code, int) else (0 if e.code is None else 1)
    else:
        _code = 0
    # Everything is written, flushed and closed at this point.  Tearing the interpreter down -- the HIP context, 13 GB of
    # pinned and mapped host memory, torch's module state -- took 0.7 s of a 4.5 s whole-genome run: leave at once.
    # (EPILOGOS_FAST_EXIT=0 restores the ordinary exit, e.g. under a coverage tool.)
    try:                                                     # error exits too: let the --cache-dir writers finish their files
        from .helpers import flushCacheWrites
        flushCacheWrites()
    except Exception:
        pass
    sys.stdout.flush()
    sys.stderr.flush()
    if os.environ.get("EPILOGOS_FAST_EXIT", "1") != "0":
        os._exit(_code)
    sys.exit(_code)


if __name__ == "__main__":
    cli()
