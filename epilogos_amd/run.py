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
from collections import namedtuple
from contextlib import closing
from pathlib import Path, PurePath
from types import SimpleNamespace

_T_START = _time.time()

import click

from . import __version__
from .helpers import getNumStates, parseColumns, parseGroupings
from .launch import _launch, _launch_command, _strip_gpus, _visible_gpus  # noqa: F401


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


def _check_biosamples_exist(files, top, resident=None):
    """The command line's pre-check of column groups: biosample top + 1, the largest asked for, is a column of every file -- or of
    every matrix of `resident`, which [--chromhmm] built under these names."""
    from . import driver
    for f in files:
        try:
            n = driver._columns_of(f) if resident is None else resident[f][1]
        except Exception:                                        # (an empty or unreadable file: the parse reports it, or it has no rows)
            continue
        if n and top >= n:
            _usage("biosample {} is not in {}: the {} has {} biosample columns".format(top + 1, f, "file" if resident is None else "matrix", n))


def _check_chromhmm_flags(o):
    """The usage errors of [--chromhmm] and the options that go with it.  Silent for a command line that has none of them."""
    def refuse(text):
        print("ERROR: [--chromhmm] " + text); sys.exit()
    if o.chromhmm is None:
        for given, opt in ((o.metadata, "--metadata"), (o.chromsizes, "--chromsizes"), (o.segments or None, "--segments"), (o.binWidth, "--bin-width"),
                           (o.stateNames, "--state-names"), (o.keepMatrices, "--keep-matrices")):
            if given is not None:
                refuse("is required with [{}]: the option describes a ChromHMM output directory".format(opt))
        return
    for given, opt in ((o.inputDirectory, "-i"), (o.inputDirectory1, "-a"), (o.inputDirectory2, "-b")):
        if given is not None:
            refuse("takes the place of the input directories; it cannot be combined with [{}]".format(opt))
    for given, opt in ((o.metadata, "--metadata"), (o.chromsizes, "--chromsizes")):
        if given is None:
            refuse("requires [{}]".format(opt))
    for given, opt in ((o.binWidth, "--bin-width"), (o.stateNames, "--state-names")):
        if given is not None and not o.segments:
            refuse("[{}] goes with [--segments]".format(opt))
    if o.binWidth is not None and o.binWidth <= 0:
        refuse("the bin width must be positive")
    if o.mode == "paired" and o.columnsA is None and o.columnsB is None and o.groupingsFile is None:
        refuse("builds one set of matrices: paired mode needs [--columns-a] and [--columns-b], or [--groupings], to name the two groups")
    if o.cacheDir is not None:
        refuse("cannot be combined with [--cache-dir]: the matrices are built on the GPU, there is no parsed text to cache")
    if o.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        refuse("runs on one GPU: it builds and holds the matrices, sharing them out over several ranks is not done yet; "
               "use [--gpus 1]")


def _selects_a_file(datadir, metadata, chromsizes, segments):
    """Whether epilogos-prep's selection rule finds any file of the directory (host only; two files for one biosample raise here
    what they raise there)."""
    from . import segments as segmentFiles, stateByLine
    if segments:
        return bool(segmentFiles.find_segments_named(datadir, metadata)[0])
    return any(files for _chrom, files, _names in stateByLine.iter_calls_named(datadir, metadata, chromsizes))


def _usage(text):
    print("ERROR: " + text); sys.exit()


def _refuse(*family):
    """A family of usage errors as (whether it applies, its message), in the order they are looked for: the first one that applies
    is the one the user hears of."""
    for applies, text in family:
        if applies:
            _usage(text)


def _absolute(path):
    return Path(path) if PurePath(path).is_absolute() else Path.cwd() / path


def _world():
    return int(os.environ.get("WORLD_SIZE", "1"))


def _check_null_draws(o):
    many = o.nullDraws > 1
    _refuse((o.nullDraws < 1, "[--null-draws] must be at least 1"),
            (many and o.mode != "paired", "[--null-draws] greater than 1 is only valid in paired mode"),
            (many and not o.pvalBool, "[--null-draws] greater than 1 requires [-n, --null-distribution]"),
            (many and (o.gpus > 1 or _world() > 1), "[--null-draws] greater than 1 runs on one GPU: the exceedance counts of several ranks "
                                                    "are not added up yet; use [--gpus 1]"))


def _check_stage_choices(o):
    """[--fit gpu], [--pvals gpu], [--metrics gpu]: single mode fits nothing and writes no pairwiseMetrics file.  ([--writer gpu] and
    [--roi gpu] are valid in both modes.)"""
    fit, pvals, single = o.fit == "gpu", o.pvals == "gpu", o.mode != "paired"
    _refuse((fit and single, "[--fit gpu] is only valid in paired mode"),
            (fit and not o.pvalBool, "[--fit gpu] requires [-n, --null-distribution]: without it nothing is fitted"),
            (fit and o.nullDraws > 1, "[--fit gpu] cannot be combined with [--null-draws] greater than 1: empirical p-values need no fit"),
            (pvals and single, "[--pvals gpu] is only valid in paired mode"),
            (pvals and not o.pvalBool, "[--pvals gpu] requires [-n, --null-distribution]: without it no p-value is computed"),
            (o.metrics == "gpu" and single, "[--metrics gpu] is only valid in paired mode"))


def _check_groupings(o):
    """-> the parsed groupings of [--groupings], or None without the option.  Nothing is read but that file."""
    if o.groupingsFile is None:
        return None
    _refuse(*((given is not None, "[--groupings] names the biosamples of every grouping itself; it cannot be combined with [{}]".format(opt))
              for given, opt in ((o.columns, "--columns"), (o.columnsA, "--columns-a"), (o.columnsB, "--columns-b"),
                                 (o.inputDirectory1, "-a"), (o.inputDirectory2, "-b"))),
            (o.inputDirectory is None, "[-i, --input-directory] is required with [--groupings]"))
    try:
        return parseGroupings(o.groupingsFile, o.mode)
    except ValueError as e:
        _usage("[--groupings] {}".format(e))


def _parse_spec(opt, text):
    try:
        return parseColumns(text)
    except ValueError as e:
        _usage("[{}] {}".format(opt, e))


def _check_columns(o, groupings):
    """-> (pairedColumns, cols, colsA, colsB): whether both groups of a paired run come out of the one directory of [-i], and the
    parsed [--columns] (single mode) or [--columns-a] and [--columns-b] (paired mode, without [--groupings])."""
    a, b = o.columnsA is not None, o.columnsB is not None
    pairedColumns = o.mode == "paired" and (a or b or groupings is not None)
    _refuse((o.mode == "single" and (a or b), "[--columns-a] and [--columns-b] are only valid in paired mode; single mode takes [--columns]"),
            (o.mode == "paired" and o.columns is not None, "[--columns] is only valid in single mode; paired mode takes [--columns-a] and [--columns-b]"))
    cols = _parse_spec("--columns", o.columns) if o.columns is not None else None
    if not pairedColumns or groupings is not None:
        return pairedColumns, cols, None, None
    _refuse((not (a and b), "[--columns-a] and [--columns-b] must be given together"),
            (o.inputDirectory1 is not None or o.inputDirectory2 is not None,
             "[--columns-a] and [--columns-b] select from [-i, --input-directory]; they cannot be combined with [-a] and [-b]"),
            (o.inputDirectory is None, "[-i, --input-directory] is required with [--columns-a] and [--columns-b]"))
    colsA, colsB = _parse_spec("--columns-a", o.columnsA), _parse_spec("--columns-b", o.columnsB)
    both = sorted(set(colsA.tolist()) & set(colsB.tolist()))
    if both:
        _usage("biosample {} is in both [--columns-a] and [--columns-b]".format(both[0] + 1))
    return pairedColumns, cols, colsA, colsB


def _check_flags(o, pairedColumns):
    """The reference's flag combinations (run.py:328-375)."""
    single, dirs = o.mode == "single", o.mode == "paired" and not pairedColumns
    _refuse((single and o.inputDirectory is None, "[-i, --input-directory] is required in single mode"),
            (single and (o.inputDirectory1 is not None or o.inputDirectory2 is not None), "[-a] and [-b] are only valid in paired mode"),
            (dirs and (o.inputDirectory1 is None or o.inputDirectory2 is None),
             "[-a, --directory-one] and [-b, --directory-two] are required in paired mode"),
            (dirs and o.inputDirectory is not None, "[-i] is only valid in single mode"),
            (o.outputDirectory is None, "[-o, --output-directory] is required"),
            (o.stateInfo is None, "[-j, --state-info] is required"))


_AS_GIVEN = ("mode stateInfo saliency groupSize roiWidth numProcesses numTrials samplingSize pvalBool nullDraws nullSeed checkStates gpus "
             "metadata chromsizes segments binWidth stateNames keepMatrices fit pvals writer roi metrics").split()


class RunSpec(namedtuple("RunSpec", _AS_GIVEN + "fileTag inputDirPath inputDirPath2 outputDirPath numStates quiescentState cols colsA colsB "
                                                "groupings pairedColumns chromhmm".split())):
    """One run of the command line, checked: what `main` and everything after it read.  The options of _AS_GIVEN as they were given
    (fit, pvals, writer, roi and metrics are the five host|gpu stage choices), and: fileTag, given or the default; the absolute
    input, second input (paired: [-b], or inputDirPath when both groups are columns of its files) and output paths; numStates; the
    0-based quiescentState (-1: off); cols, colsA and colsB, 0-based as parseColumns gives them; the parsed groupings, or None;
    chromhmm, whether inputDirPath is a ChromHMM output directory.  Nothing in it changes; a paired run without [--null-seed]
    goes on with a copy that has the seed it drew."""
    __slots__ = ()

    @property
    def storedExpPath(self):
        return self.outputDirPath / "exp_freq_{}.npy".format(self.fileTag)

    def topBiosample(self):
        """The largest biosample asked for by column, 0-based; -1 when the run selects none."""
        asked = [c for g in self.groupings for c in g[1:]] if self.groupings is not None else [self.cols, self.colsA, self.colsB]
        return max([int(c.max()) for c in asked if c is not None] + [-1])

    def extra(self, *stages):
        """The keywords that the choices of these stages add to a call: none for `host`, so that a run without the options calls
        the drivers and STEP 4 exactly as it did before they existed.  The run's one seed travels with fit="gpu"."""
        kw = {s: "gpu" for s in stages if getattr(self, s) == "gpu"}
        return dict(kw, seed=self.nullSeed) if "fit" in kw else kw


def _describe_run(o):
    """The click options `o` -> RunSpec; every usage error of the command line comes out of here.  The order of checks and side
    effects is what users and tests see; nothing moves across another item:
     1. [-v].
     2. [--chromhmm] flag checks; the directory is the run's input directory from then on.
     3. [--null-draws] checks.
     4. [--fit], [--pvals] and [--metrics] checks.
     5. [--groupings] checks: incompatible options, [-i] required, file parse.
     6. Column checks and SPEC parse.
     7. The reference's flag combinations ([-i], [-a], [-b], [-o], [-j]).  Up to here nothing but the groupings file is read.
     8. EPILOGOS_CACHE_DIR / EPILOGOS_NUM_CORES are set.
     9. getNumStates reads the state file.
    10. Paths are made absolute.
    11. [--groupings]: its largest biosample against the headers of the files.
    12. [--chromhmm] file checks, and the OSError of a directory none of whose files is selected.
    13. checkArguments, which creates the output directory.
    14. The default file tag.
    15. [--gpus] below 0.  The record is complete; main goes on with it.
    16. The launcher fork, before torch is imported.
    17. File lists, and the FileNotFoundError of paired directories that do not match (_open_inputs, to 19).
    18. [--columns*]: the largest biosample against the headers of the files.
    19. The early readers start.
    20. Device and process group; on failure the early readers are aborted.
    21. [--chromhmm]: the matrices are built, with their own biosample check ("the matrix has").
    22. The "State Model" line.
    23. The null seed is drawn and broadcast.
    24. STEP 1-3 and STEP 4 of every route (_routes, _step4).
    25. flushCacheWrites, the timing and memory lines, destroy_process_group."""
    if o.version:
        print("Version:", __version__); sys.exit()
    _check_chromhmm_flags(o)
    if o.chromhmm is not None:
        o.inputDirectory = o.chromhmm                            # required-ness, tag, emptiness: all as for [-i]
    _check_null_draws(o)
    _check_stage_choices(o)
    groupings = _check_groupings(o)
    pairedColumns, cols, colsA, colsB = _check_columns(o, groupings)
    _check_flags(o, pairedColumns)
    if o.cacheDir:
        os.environ["EPILOGOS_CACHE_DIR"] = str(Path(o.cacheDir).resolve())
    if o.numProcesses > 0:                                       # the reference's core budget (run.py:36,148): see _io.host_budget
        os.environ["EPILOGOS_NUM_CORES"] = str(o.numProcesses)
    numStates = getNumStates(o.stateInfo)
    paired = o.mode == "paired"
    inputDirPath = _absolute(o.inputDirectory if not paired or pairedColumns else o.inputDirectory1)
    inputDirPath2 = (inputDirPath if pairedColumns else _absolute(o.inputDirectory2)) if paired else Path("")
    spec = RunSpec(**{name: getattr(o, name) for name in _AS_GIVEN}, fileTag=o.fileTag, inputDirPath=inputDirPath,
                   inputDirPath2=inputDirPath2, outputDirPath=_absolute(o.outputDirectory), numStates=numStates,
                   quiescentState=numStates - 1 if o.quiescentState == -1 else o.quiescentState - 1,       # 1-based -> 0-based, 0 -> off
                   cols=cols, colsA=colsA, colsB=colsB, groupings=groupings, pairedColumns=pairedColumns, chromhmm=o.chromhmm is not None)
    if groupings is not None and inputDirPath.is_dir() and not spec.chromhmm:
        _check_biosamples_exist(sorted(inputDirPath.glob("*"), key=_natural_key), spec.topBiosample())
    if spec.chromhmm:
        for given, opt in ((o.metadata, "--metadata"), (o.chromsizes, "--chromsizes"), (o.stateNames, "--state-names")):
            if given is not None and not Path(given).is_file():
                _usage("[{}] is not a file: {}".format(opt, given))
        if inputDirPath.is_dir() and list(inputDirPath.glob("*")) and not _selects_a_file(inputDirPath, o.metadata, o.chromsizes, o.segments):
            # no file of the directory is anybody's: epilogos-prep would leave an empty directory, which [-i] refuses like this
            raise OSError("Ensure that directory is not empty: {}".format(str(inputDirPath)))
    checkArguments(o.mode, o.saliency, inputDirPath, inputDirPath2, spec.outputDirPath, o.numProcesses, numStates, spec.quiescentState,
                   o.groupSize, o.numTrials, o.samplingSize, o.roiWidth)
    if o.fileTag == "null":
        spec = spec._replace(fileTag="{}_s{}".format(inputDirPath.name, o.saliency) if not paired
                             else "{0}_A_{0}_B_s{1}".format(inputDirPath.name, o.saliency) if pairedColumns
                             else "{}_{}_s{}".format(inputDirPath.name, inputDirPath2.name, o.saliency))
    if o.gpus < 0:
        _usage("Number of GPUs must be positive or zero (0 means use all visible GPUs)")
    return spec


def _build_resident(spec):
    """[--chromhmm]: the matrices of the ChromHMM output directory, built on the device by epilogos-prep's own generator
    (preprocess.iter_matrices, which prints its progress lines) and kept there.  -> _Inputs(files, [], resident): the virtual paths
    `matrix_{chr}.epgm` the run sees them under -- in OUTDIR with [--keep-matrices], where they are then also written, as built --
    in the natural-key order in which [-i] would run those files, and {path: (X, N, Locations)} for driver.run_groupings.
    Without [--check-states] a matrix is handed over as stateByLine.read_epgm would have read its file: what is no state of the
    parser's limit is -1.  A state range outside the model raises what the readers of the files raise.  The matrices must fit on
    the device next to a session by the resident store's own rule, applied once to their total; if not, the run ends here."""
    t_build = _time.time()
    from . import _io, driver, preprocess, segments as segmentFiles, stateByLine
    _io.set_state_limit(spec.numStates)
    table = segmentFiles.read_state_names(spec.stateNames) if spec.stateNames else None
    outdir = None
    if spec.keepMatrices is not None:
        outdir = Path(spec.keepMatrices)
        outdir.mkdir(parents=True, exist_ok=True)
    resident, ranges = {}, {}
    for chrom, X, N, name, rng, _names, width in preprocess.iter_matrices(spec.inputDirPath, spec.metadata, spec.chromsizes, sys.stdout,
                                                                          spec.segments, spec.binWidth or stateByLine.BIN_WIDTH, table):
        path = preprocess.matrix_path(outdir if outdir is not None else "", chrom)
        if outdir is not None:
            stateByLine.write_epgm(path, X[:, :N].contiguous(), name, rng, width)
        if not spec.checkStates and rng[1] > _io.state_limit():       # (a byte is a state value - 1; the pad columns are -1 as built)
            X[(X >= _io.state_limit()) | (X < 0)] = -1
        resident[path] = (X, N, stateByLine.synth_locations(name, 0, X.shape[0], width))
        ranges[path] = rng
        del X
    files = sorted(resident, key=_natural_key)
    for f in files:
        driver._check_range(f, ranges[f], spec.numStates)
    if files:
        nbytes = sum(driver._nbytes(resident[f][0]) for f in files)
        free = driver._device_free(resident[files[0]][0])
        if not driver._ResidentStore.fits(nbytes, free):
            print("ERROR: [--chromhmm] the matrices do not fit on the device next to a run: they are {} bytes and need {} bytes free "
                  "({} x the matrices + {}), {} bytes are free.  Use the two commands instead: epilogos-prep -o MATRICES, then "
                  "epilogos -i MATRICES".format(nbytes, driver._ResidentStore.FREE_FACTOR * nbytes + driver._ResidentStore.FREE_SLACK,
                                                driver._ResidentStore.FREE_FACTOR, driver._ResidentStore.FREE_SLACK, free))
            sys.exit(1)
    _timing("matrices built on the device", _time.time() - t_build)
    if not files:                                                # (segment files that hold no chromosome of the sizes file)
        raise OSError("Ensure that directory is not empty: {}".format(str(spec.inputDirPath)))
    _check_biosamples_exist(files, spec.topBiosample(), resident)
    return _Inputs(files, [], resident)


def _rank():
    return int(os.environ.get("RANK", "0"))


def _under_launcher():
    return "WORLD_SIZE" in os.environ and "RANK" in os.environ


def _say(*args, **kwargs):
    if _rank() == 0:
        print(*args, **kwargs)


def _timing(label, seconds):
    if os.environ.get("EPILOGOS_TIMING") and _rank() == 0:
        print("    [timing] %-34s %7.2f s" % (label, seconds), flush=True)


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


_Inputs = namedtuple("_Inputs", "files files2 resident")   # files of [-i] or [-a]; those of [-b]; [--chromhmm]: {path: (X, N, Locations)}


def _open_inputs(spec):
    """-> _Inputs: the files in the order they run in, every biosample asked for by column being a column of each.  In a single
    process their readers start NOW -- inflating needs neither torch nor the GPU, and importing the one and initialising the other
    takes about a second, which a whole-genome run spent before its first byte was read.  A reader asks for its (page-locked)
    destination only after its inflate; the session is attached when it exists."""
    files = sorted(spec.inputDirPath.glob("*"), key=_natural_key) if not spec.chromhmm else []    # (--chromhmm: named once they are built)
    files2 = []
    if spec.mode == "paired" and not spec.pairedColumns:
        for file in files:
            if not list(spec.inputDirPath2.glob(file.name)):
                raise FileNotFoundError("File not found: {}".format(str(spec.inputDirPath2 / file.name))
                                        + " Please ensure corresponding files within input directories 1 and 2 have the same name")
            files2.append(next(spec.inputDirPath2.glob(file.name)))
    from . import _io, driver
    if spec.groupings is None and spec.topBiosample() >= 0:
        _check_biosamples_exist(files, spec.topBiosample())
    if not spec.chromhmm and _world() == 1 and not _under_launcher() and os.environ.get("EPILOGOS_EARLY_READERS", "1") != "0":
        _io.set_state_limit(spec.numStates)
        jobs = [(f, 0, None) for pair in (zip(files, files2) if files2 else zip(files)) for f in pair]
        driver.start_readers_early(jobs, raw=spec.checkStates)   # (--check-states: .epgm bytes reach the device as they are)
    return _Inputs(files, files2, None)


def _draw_null_seed(device):
    """The seed of a paired run without [--null-seed]: every rank must shuffle with the same one (--groupings: every grouping too)."""
    import numpy as np
    seed = np.array([int(np.random.SeedSequence().generate_state(1)[0])], dtype=np.int64)
    if _world() > 1:
        import torch
        import torch.distributed as dist
        t = torch.from_numpy(seed)
        t = t.to(device) if device is not None else t
        dist.broadcast(t, src=0)
        seed = t.cpu().numpy()
    return int(seed[0])


def _routes(spec, inputs, device):
    """STEP 1-3 of every route of the command line -> generator of (subdirectory of the output directory, results), each to be followed
    by its STEP 4.  Flat runs over files go to driver.run_single_group, run_paired_groups ([-a] [-b]) or run_paired_columns, under
    the banner of their mode; [--groupings] and every run of [--chromhmm] to driver.run_groupings: every file is parsed and uploaded
    once (--chromhmm: is resident already), and the groupings run one after another from the resident matrices, each with its text
    complete before the next begins.  [--chromhmm] without [--groupings] is one grouping written to the output directory itself."""
    from . import driver
    world, paired = _world(), spec.mode == "paired"
    model = (spec.numStates, spec.saliency, spec.outputDirPath, spec.fileTag)
    null = (spec.quiescentState, spec.groupSize, spec.nullSeed)
    common = dict(verbose=False, device=device, defer_writes=True, checkStates=spec.checkStates, **spec.extra("writer"))
    shuffled = dict(common, keep_temps=False, nullDraws=spec.nullDraws)
    flat = spec.groupings is None
    if not flat:
        _say("\nSTEP 1-3 of %d grouping(s): background counts -> all-reduce -> scores%s, from one read of the matrices (%d GPU(s))"
             % (len(spec.groupings), ", null groups, deltas" if paired else "", world))
    elif paired:
        _say("\nSTEP 1-3: background counts over [A|B] -> all-reduce -> scores, null groups, deltas (%d GPU(s))" % world)
    else:
        _say("\nSTEP 1-3: background counts -> all-reduce -> scores (bin-range partition over %d GPU(s))" % world)
    if not flat or inputs.resident is not None:
        groupings = spec.groupings if not flat else [("", spec.colsA, spec.colsB)] if paired else [("", spec.cols)]
        runs = driver.run_groupings(inputs.files, groupings, *model, *null, **shuffled,
                                    **({} if inputs.resident is None else {"resident": inputs.resident, "flat": flat}))
        try:
            for k, g in enumerate(groupings):
                if not flat:
                    _say("\nGrouping %d of %d: %s" % (k + 1, len(groupings), g[0]), flush=True)
                name, _q, results, _info = next(runs)
                yield name, results
        finally:
            runs.close()
            driver.abort_early_readers()
            driver.finish_writes()
        return
    try:
        if not paired:
            _, results = driver.run_single_group(inputs.files, *model, **common, keep_temp_scores=False, columns=spec.cols)
        elif spec.pairedColumns:
            _, results = driver.run_paired_columns(inputs.files, spec.colsA, spec.colsB, *model, *null, **shuffled)
        else:
            _, results = driver.run_paired_groups(inputs.files, inputs.files2, *model, *null, **shuffled)
    finally:
        driver.abort_early_readers()                             # (nothing to do once the stage driver has taken them over)
    yield "", results


def _step4(spec, results, outDir):
    """STEP 4 of one grouping, on rank 0; every rank then waits for its writers (the score text is still being written under it)."""
    from . import driver
    paired = spec.mode == "paired"
    if paired and spec.pvalBool and max(spec.numProcesses, 1) > 1 and spec.nullDraws == 1 and spec.fit != "gpu":
        driver.finish_writes()                                   # -n -c K forks a pool for the fits: not with writer threads running
    try:
        if _rank() == 0:
            t0 = _time.perf_counter()
            if paired:
                print("\nSTEP 4: Generating p-values & regions of interest (figures are not produced)", flush=True)
                from .roiAndVisualPairwise import mainFromArrays as roiPairwise
                roiPairwise(results, spec.stateInfo, outDir, spec.fileTag, max(spec.numProcesses, 1), spec.pvalBool, spec.numTrials,
                            spec.samplingSize, outDir / spec.storedExpPath.name, spec.roiWidth or 125, False,
                            **spec.extra("fit", "pvals", "roi", "metrics"))
            else:
                print("\nSTEP 4: Finding regions of interest", flush=True)
                from .roiSingle import mainFromArrays as roiSingle
                roiSingle(results, outDir, spec.stateInfo, spec.fileTag, outDir / spec.storedExpPath.name, spec.roiWidth or 50, False,
                          **spec.extra("roi", "metrics"))
            _timing("STEP 4", _time.perf_counter() - t0)
    finally:
        driver.finish_writes()


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
def main(**options):
    """Information-theoretic navigation of multi-tissue functional genomic annotations -- MI355X scoring engine."""
    spec = _describe_run(SimpleNamespace(**options))             # items 1-15 of its order contract; the rest follow here
    if "WORLD_SIZE" not in os.environ and spec.gpus != 1:
        # --gpus N from a plain start: one process per GPU (the reference submits its own SLURM jobs, run.py:190-279,454-505) -- as
        # a CHILD process, before this one has imported torch or touched a GPU
        gpus = spec.gpus or (1 if spec.nullDraws > 1 else _visible_gpus())     # (0: all visible; --null-draws K > 1 runs on one GPU)
        if gpus > 1:
            sys.exit(_launch(gpus, sys.argv[1:] if _ARGV is None else _ARGV))
    inputs = _open_inputs(spec)
    from . import driver
    try:
        device = _init_device_and_group(_world(), _under_launcher())
    except BaseException:
        driver.abort_early_readers()
        raise
    _timing("imports + device init (since process start)", _time.time() - _T_START)
    if spec.chromhmm:
        inputs = _build_resident(spec)                           # epilogos-prep's part of the job, its progress lines included
    _say("State Model =", spec.numStates, " Saliency level =", spec.saliency, " GPUs =", _world())
    if spec.mode == "paired" and spec.nullSeed is None:
        spec = spec._replace(nullSeed=_draw_null_seed(device))
    runs = _routes(spec, inputs, device)
    del inputs                                                   # (--chromhmm: the matrices are the run's from here on, gone with it)
    with closing(runs):
        for name, results in runs:
            _step4(spec, results, spec.outputDirPath / name)
    from .helpers import flushCacheWrites
    flushCacheWrites()                                           # --cache-dir: files of first-time reads, written in the background
    _timing("end of main (since process start)", _time.time() - _T_START)
    if os.environ.get("EPILOGOS_TIMING") and _rank() == 0:
        try:                                                     # what the process holds (and will have to give back at exit)
            st = dict(l.split(":", 1) for l in open("/proc/self/status").read().splitlines() if ":" in l)
            print("    [timing] memory at the end: " + ", ".join("%s %.1f GB" % (k, int(st[k].split()[0]) / 1048576.0)
                                                              for k in ("VmHWM", "VmRSS", "RssAnon", "RssFile", "RssShmem") if k in st), flush=True)
        except (OSError, ValueError):
            pass
    if _world() > 1 or _under_launcher():
        import torch.distributed as dist
        dist.destroy_process_group()


_ARGV = None            # the argument list cli() was called with, when it is not sys.argv[1:]


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
