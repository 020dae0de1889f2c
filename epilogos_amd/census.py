"""`python -m epilogos_amd.census -i matrices/ -j states.tsv [-o census.tsv] [--names metadata.txt]`: how many bins of every
biosample of every input matrix are in every state, and how many bytes of it are no state at all -- one pass of
epg_state_census (csrc/epg_census.hip) over each matrix on the GPU.  `epilogos-prep --census FILE` writes the same table from
the matrices it builds.

The table is tab-separated with one header line, `chrom column biosample bins not_a_state <S state columns>`: one line per file
and biosample column (files in the order `epilogos` runs them, columns 1-based as --columns numbers them), then -- when every
file has the same number of columns -- the genome-wide lines with chrom = `all`.  All values are integers and
bins == not_a_state + the sum of the state columns on every line.  The table is a report: the exit status is 0 whatever it
holds; a file with bytes that are no state gets one warning line on stderr that names the first.  There is no CPU fallback."""
import sys
from pathlib import Path

import click
import numpy as np

HEAD = ["chrom", "column", "biosample", "bins", "not_a_state"]


def state_headers(stateInfo, S):
    """The S state column heads: the short_name column of the -j file when it has one (and a name for every state), else 1 .. S."""
    plain = [str(k) for k in range(1, S + 1)]
    if stateInfo is None:
        return plain
    with open(Path(stateInfo), "r", newline=None) as fh:
        rows = [l.split("\t") for l in fh.read().splitlines() if l.strip(" ") != ""]
    if not rows or "short_name" not in [c.strip() for c in rows[0]]:
        return plain
    k = [c.strip() for c in rows[0]].index("short_name")
    names = [r[k].strip() if len(r) > k else "" for r in rows[1:S + 1]]
    return names if len(names) == S and all(names) else plain


def read_names(metadata):
    """Biosample names: column 1 of the metadata file behind its header line, the way the preprocessing command reads it."""
    from .textBatches import first_fields
    return first_fields(metadata, skip=1)


def table_lines(entries, heads):
    """entries: [(chrom, census int [N, S], other int [N], bins, names or None)] in file order -> the table's lines (no newline).
    names: the biosample of every column (short lists and None give `.`)."""
    S = len(heads)
    lines = ["\t".join(HEAD + list(heads))]
    total = None
    same = len({np.asarray(e[1]).shape[0] for e in entries}) <= 1

    def row(chrom, n, name, bins, other, counts):
        return "\t".join([chrom, str(n + 1), name, str(int(bins)), str(int(other))] + [str(int(c)) for c in counts])
    for chrom, census, other, bins, names in entries:
        census = np.asarray(census, dtype=np.int64).reshape(-1, S)
        other = np.asarray(other, dtype=np.int64).reshape(-1)
        N = census.shape[0]
        names = list(names or [])
        names += ["."] * (N - len(names))
        for n in range(N):
            lines.append(row(chrom, n, names[n] or ".", bins, other[n], census[n]))
        if same:
            if total is None:
                total = [census.copy(), other.copy(), int(bins), names]
            else:
                total[0] += census
                total[1] += other
                total[2] += int(bins)
                total[3] = [a if a == b else "." for a, b in zip(total[3], names)]
    if same and total is not None:
        for n in range(total[0].shape[0]):
            lines.append(row("all", n, total[3][n] or ".", total[2], total[1][n], total[0][n]))
    return lines


def write_table(path, entries, heads):
    text = "\n".join(table_lines(entries, heads)) + "\n"
    if path is None or str(path) == "-":
        sys.stdout.write(text)
        sys.stdout.flush()
    else:
        Path(path).write_text(text)


def offender_warning(path, S, other, first_bad, N, byte):
    return ("WARNING: {}: {} byte(s) are not a state of the {}-state model; the first is byte {} at row {} (0-based), biosample {}"
            .format(path, int(np.asarray(other).sum()), S, int(byte) & 0xff, int(first_bad) // N, int(first_bad) % N + 1))


def input_files(inputs):
    """Directories give their files in the order `epilogos` runs them; files stand for themselves."""
    from .run import _natural_key
    files = []
    for p in inputs:
        p = Path(p)
        files += sorted((f for f in p.glob("*") if f.is_file()), key=_natural_key) if p.is_dir() else [p]
    return files


def census_device(X, N, S):
    """(census [N, S], other [N], first_bad, the byte there or None) of a resident matrix as host values.  Synchronises."""
    from . import engine
    census, other, fb = engine.state_census(X, N, S)
    fb = int(fb.item())
    byte = None if fb == engine.FIRST_BAD_NONE else int(X[fb // N, fb % N].item()) & 0xff
    return census.cpu().numpy(), other.cpu().numpy(), fb, byte


def census_file(path, S, names=None, err=None):
    """One input file, read and uploaded once -> its entry of the table."""
    import torch
    from . import engine
    from .helpers import fileStem, readTable

    width = [0]

    def alloc(R, N):                                   # (called by the reader once it knows the file's shape)
        width[0] = N
        return np.empty((R, engine.padded_width(N)), dtype=np.int8)
    arr, loc = readTable(path, alloc=alloc, raw=True)        # a .epgm file's bytes as they are: the table counts what the file holds
    R, N = arr.shape[0], width[0]
    chrom = loc.slice(0, 1).to_object_array()[0, 0] if len(loc) else fileStem(path)
    if R == 0 or N == 0:
        return str(chrom), np.zeros((N, S), dtype=np.int64), np.zeros(N, dtype=np.int64), R, names
    X = torch.from_numpy(np.ascontiguousarray(arr)).to("cuda")
    census, other, fb, byte = census_device(X, N, S)
    if byte is not None:
        print(offender_warning(path, S, other, fb, N, byte), file=err or sys.stderr, flush=True)
    return str(chrom), census, other, R, names


def run(inputs, stateInfo, out=None, names=None, err=None):
    """The command: -> the table's entries."""
    from . import _io, engine
    from .helpers import getNumStates
    engine.require_gpu()
    S = getNumStates(stateInfo)
    if not 1 <= S <= 127:
        raise click.UsageError("the state model of {} has {} states: 1 .. 127 are supported".format(stateInfo, S))
    _io.set_state_limit(S)
    biosamples = read_names(names) if names else None
    entries = [census_file(f, S, biosamples, err) for f in input_files(inputs)]
    write_table(out, entries, state_headers(stateInfo, S))
    return entries


@click.command(context_settings={"help_option_names": ["-h", "--help"]})
@click.option("-i", "--input", "inputs", multiple=True, required=True, type=click.Path(exists=True),
              help="A directory of the matrix files `epilogos -i` takes (.epgm, .txt, .txt.gz), or single files; may be repeated")
@click.option("-j", "--state-info", "stateInfo", required=True, type=click.Path(exists=True, dir_okay=False), help="State model info file")
@click.option("-o", "--output", "out", type=click.Path(dir_okay=False), default=None, help="Where the table goes  [default: stdout]")
@click.option("--names", "names", type=click.Path(exists=True, dir_okay=False), default=None,
              help="Biosample metadata (column 1 behind the header line): line k names biosample column k")
def main(inputs, stateInfo, out, names):
    """Per-biosample state census of input matrices: bins per state and bytes that are no state, counted on the GPU."""
    run(inputs, stateInfo, out, names)


def cli(argv=None):
    main.main(args=argv, standalone_mode=True)


if __name__ == "__main__":
    cli()
