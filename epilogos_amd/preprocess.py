"""`python -m epilogos_amd.preprocess DATADIR METADATA CHROMSIZES -o OUTDIR` (console script `epilogos-prep`): ChromHMM
-printstatebyline calls -> one binary state matrix `matrix_<chr>.epgm` per chromosome, on the GPU (stateByLine.py).
`--segments` reads ChromHMM's default output instead, one `*_segments.bed` per biosample for the whole genome (segments.py).

The three arguments and the progress lines are those of the reference's bin/preprocess_data_ChromHMM.sh; what comes out is not
its `matrix_<chr>.txt` (1.7 KB of text per bin) but the matrix itself, 1 byte per cell, which `epilogos -i OUTDIR` reads directly.
Text matrices are not written.  There is no CPU fallback: without a GPU or the HIP library the command raises."""
import os
import sys
from pathlib import Path

import click

from . import segments as segmentFiles, stateByLine


class _Census:
    """--census FILE: the table of epilogos_amd.census from the matrices while they are on the device.  A matrix is censused with
    the states it holds itself (its range's upper end); the table's state columns are those of the widest, or of --state-names."""

    def __init__(self, path, state_names=None):
        self.path, self.entries = path, []
        self.table = state_names or {}

    def add(self, chrom, X, N, rng, names):
        """A finished matrix, still resident; names: the biosample of every column (what selected its file)."""
        from . import engine
        c, other, _fb = engine.state_census(X, N, min(max(int(rng[1]), 1), 127))
        self.entries.append((chrom, c, other, X.shape[0], list(names)))

    def write(self):
        import numpy as np
        from . import census
        S = max([e[1].shape[1] for e in self.entries] + [v for v in self.table.values() if 1 <= v <= 127] + [1])
        heads = [str(k) for k in range(1, S + 1)]
        for name, k in self.table.items():
            if 1 <= k <= S:
                heads[k - 1] = name
        wide = []
        for chrom, c, other, R, names in self.entries:
            full = np.zeros((c.shape[0], S), dtype=np.int64)
            full[:, :c.shape[1]] = c.cpu().numpy()
            wide.append((chrom, full, other.cpu().numpy(), R, names))
        census.write_table(self.path, wide, heads)


class _Concordance:
    """--concordance PREFIX: the two tables of epilogos_amd.concordance, summed over the matrices while they are on the device.  A
    matrix is counted with the states it holds itself (its range's upper end), as the census is."""

    def __init__(self, prefix):
        from . import concordance
        self.prefix, self.tally, self.names = prefix, concordance.Tally(), None

    def add(self, chrom, X, N, rng, names):
        self.tally.add(X if X.shape[0] else None, N, min(max(int(rng[1]), 1), 127), "the matrix of {}".format(chrom))
        if self.names is None:
            self.names = list(names)

    def write(self):
        self.tally.write(self.prefix, self.names)


def iter_matrices(datadir, metadata, chromsizes, out=sys.stdout, segments=False, width=stateByLine.BIN_WIDTH, table=None):
    """The matrices of a ChromHMM output directory as they are built, each still on the device: yields (chromosome of `chromsizes`,
    X int8 [R, ldx], N, the chromosome name the matrix file stores, (lo, hi), the biosample of every column, bin width) and writes
    the progress lines -- "Processing ...: n files found. " before a matrix is built, "Done." when the consumer comes back for the
    next, "Skipping." for a chromosome without files.  `epilogos-prep` is this plus write_epgm, --census and --concordance (run,
    run_segments); `epilogos --chromhmm` is this plus the hand-over to the run (epilogos_amd/run.py).  State-by-line calls: one
    chromosome is built at a time.  segments (table: the parsed --state-names, or None): every chromosome's matrix is built in
    one pass over the files, then handed out in `chromsizes` order.  A consumer that drops X frees it."""
    from . import engine
    engine.require_gpu()
    if segments:
        files, names = segmentFiles.find_segments_named(datadir, metadata)
        chroms, sizes = segmentFiles.read_chromsizes(chromsizes)
        mats = segmentFiles.build_matrices_device(files, chroms, width, sizes=sizes, state_names=table) if files else {}
        for chrom in dict.fromkeys(chroms):
            found = chrom in mats
            out.write("Processing {}: {} files found. ".format(chrom, len(files) if found else 0))
            out.flush()
            if not found:
                out.write("Skipping.\n")
                continue
            X, rng = mats.pop(chrom)
            yield chrom, X, len(files), chrom, rng, names, width
            del X
            out.write("Done.\n")
            out.flush()
        return
    for chrom, files, names in stateByLine.iter_calls_named(datadir, metadata, chromsizes):
        out.write("Processing {}: {} files found. ".format(chrom, len(files)))
        out.flush()
        if not files:
            out.write("Skipping.\n")
            continue
        # (the name inside the file is the calls' own, the script's chr=$2; the file is named after the chromsizes entry like the script's)
        X, N, name, rng = stateByLine.build_matrix_device(files)
        yield chrom, X, N, name, rng, names, stateByLine.BIN_WIDTH
        del X
        out.write("Done.\n")
        out.flush()


def matrix_path(outdir, chrom):
    return Path(outdir) / "matrix_{}{}".format(chrom, stateByLine.EXT)


def _write_all(matrices, outdir, tally, pairs):
    """run / run_segments behind their arguments: every matrix of `matrices` (iter_matrices) censused, tallied and written."""
    written = []
    for chrom, X, N, name, rng, names, width in matrices:
        if tally:
            tally.add(name, X, N, rng, names)
        if pairs:
            pairs.add(name, X, N, rng, names)
        written.append(stateByLine.write_epgm(matrix_path(outdir, chrom), X[:, :N].contiguous(), name, rng, width))
        del X
    if tally:
        tally.write()
    if pairs:
        pairs.write()
    return written


def run_segments(datadir, metadata, chromsizes, outdir, out=sys.stdout, width=stateByLine.BIN_WIDTH, state_names=None, census=None,
                 concordance=None):
    """`run` for segment files: every chromosome's matrix is built in one pass over the files, then written in `chromsizes` order."""
    from . import engine
    engine.require_gpu()
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    table = segmentFiles.read_state_names(state_names) if state_names else None
    tally = _Census(census, table) if census else None
    pairs = _Concordance(concordance) if concordance else None
    return _write_all(iter_matrices(datadir, metadata, chromsizes, out, True, width, table), outdir, tally, pairs)


def run(datadir, metadata, chromsizes, outdir, out=sys.stdout, segments=False, width=stateByLine.BIN_WIDTH, state_names=None, census=None,
        concordance=None):
    """-> the files written.  One progress line per chromosome of `chromsizes`, as the script prints them.  census: where the
    per-biosample state census of the matrices goes (epilogos_amd.census's table), None: none is taken.  concordance: the PREFIX
    of the pairwise tables of epilogos_amd.concordance, None: none are written."""
    if segments:
        return run_segments(datadir, metadata, chromsizes, outdir, out, width, state_names, census, concordance)
    from . import engine
    engine.require_gpu()
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    tally = _Census(census) if census else None
    pairs = _Concordance(concordance) if concordance else None
    return _write_all(iter_matrices(datadir, metadata, chromsizes, out), outdir, tally, pairs)


@click.command(context_settings={"help_option_names": ["-h", "--help"]})
@click.argument("datadir", type=click.Path(exists=True, file_okay=False))
@click.argument("metadata", type=click.Path(exists=True, dir_okay=False))
@click.argument("chromsizes", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output-directory", "outdir", required=True, type=click.Path(file_okay=False), help="Where the matrix_<chr>.epgm files go")
@click.option("-c", "--num-cores", "numCores", type=int, default=0, show_default=True,
              help="Upper bound on the host cores used for inflating the call files (0 = all the job may use)")
@click.option("--segments", is_flag=True, help="DATADIR holds ChromHMM segment files (one *_segments.bed per biosample, whole genome)")
@click.option("--bin-width", "binWidth", type=int, default=None, help="With --segments: the bin width in bp  [default: 200]")
@click.option("--state-names", "stateNames", type=click.Path(exists=True, dir_okay=False), default=None,
              help="With --segments: a state metadata TSV (one_index, short_name) for labels that are names")
@click.option("--census", "census", type=click.Path(dir_okay=False), default=None,
              help="Also write the per-biosample state census of the matrices (the table of `python -m epilogos_amd.census`) here")
@click.option("--concordance", "concordance", type=click.Path(dir_okay=False), default=None,
              help="Also write the pairwise biosample concordance of the matrices (the two tables of `python -m epilogos_amd.concordance`) "
                   "as PREFIX.agree.tsv and PREFIX.both.tsv")
def main(datadir, metadata, chromsizes, outdir, numCores, segments, binWidth, stateNames, census, concordance):
    """ChromHMM calls -> binary state matrices for `epilogos -i`: state-by-line files (one per biosample and chromosome) or,
    with --segments, segment files (one per biosample)."""
    if binWidth is not None and binWidth <= 0:
        raise click.UsageError("The bin width must be positive")
    if not segments and (binWidth is not None or stateNames is not None):
        raise click.UsageError("--bin-width and --state-names go with --segments")
    if numCores < 0:
        raise click.UsageError("Number of cores must be positive or zero (0 means use all cores)")
    if numCores > 0:
        os.environ["EPILOGOS_NUM_CORES"] = str(numCores)
    # without the option the call is, keyword for keyword, the one it was (tests/test_segments_host.py pins it)
    extra = {"census": census} if census else {}
    if concordance:
        extra["concordance"] = concordance
    run(datadir, metadata, chromsizes, outdir, segments=segments, width=binWidth or stateByLine.BIN_WIDTH, state_names=stateNames, **extra)


def cli(argv=None):
    main.main(args=argv, standalone_mode=True)


if __name__ == "__main__":
    cli()
