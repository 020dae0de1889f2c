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


def run_segments(datadir, metadata, chromsizes, outdir, out=sys.stdout, width=stateByLine.BIN_WIDTH, state_names=None):
    """`run` for segment files: every chromosome's matrix is built in one pass over the files, then written in `chromsizes` order."""
    from . import engine
    engine.require_gpu()
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    files = segmentFiles.find_segments(datadir, metadata)
    chroms, sizes = segmentFiles.read_chromsizes(chromsizes)
    table = segmentFiles.read_state_names(state_names) if state_names else None
    mats = segmentFiles.build_matrices_device(files, chroms, width, sizes=sizes, state_names=table) if files else {}
    written = []
    for chrom in dict.fromkeys(chroms):
        found = chrom in mats
        out.write("Processing {}: {} files found. ".format(chrom, len(files) if found else 0))
        out.flush()
        if not found:
            out.write("Skipping.\n")
            continue
        X, rng = mats.pop(chrom)
        written.append(stateByLine.write_epgm(outdir / "matrix_{}{}".format(chrom, stateByLine.EXT), X[:, :len(files)].contiguous(), chrom, rng, width))
        del X
        out.write("Done.\n")
        out.flush()
    return written


def run(datadir, metadata, chromsizes, outdir, out=sys.stdout, segments=False, width=stateByLine.BIN_WIDTH, state_names=None):
    """-> the files written.  One progress line per chromosome of `chromsizes`, as the script prints them."""
    if segments:
        return run_segments(datadir, metadata, chromsizes, outdir, out, width, state_names)
    from . import engine
    engine.require_gpu()
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    written = []
    for chrom, files in stateByLine.iter_calls(datadir, metadata, chromsizes):
        out.write("Processing {}: {} files found. ".format(chrom, len(files)))
        out.flush()
        if not files:
            out.write("Skipping.\n")
            continue
        X, N, name, rng = stateByLine.build_matrix_device(files)
        # (the name inside the file is the calls' own, the script's chr=$2; the file is named after the chromsizes entry like the script's)
        written.append(stateByLine.write_epgm(outdir / "matrix_{}{}".format(chrom, stateByLine.EXT), X[:, :N].contiguous(), name, rng))
        del X
        out.write("Done.\n")
        out.flush()
    return written


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
def main(datadir, metadata, chromsizes, outdir, numCores, segments, binWidth, stateNames):
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
    run(datadir, metadata, chromsizes, outdir, segments=segments, width=binWidth or stateByLine.BIN_WIDTH, state_names=stateNames)


def cli(argv=None):
    main.main(args=argv, standalone_mode=True)


if __name__ == "__main__":
    cli()
