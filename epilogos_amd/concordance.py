"""`python -m epilogos_amd.concordance -i matrices/ -j states.tsv -o PREFIX [--names metadata.txt] [--columns SPEC]`: in how many
bins every PAIR of biosamples is in the same state (PREFIX.agree.tsv) and in how many both are in a state at all
(PREFIX.both.tsv, the denominator) -- epg_concordance (csrc/epg_concordance.hip) over each input matrix on the GPU, summed over
all files on the device.  `epilogos-prep --concordance PREFIX` writes the same two files from the matrices it builds.

Each file is a square, tab-separated table of integers: the header line `biosample` and the N names, then one line per biosample,
its name and its row.  Names are column 1 of --names behind its header line; a biosample the list does not name, and every one
without --names, is called by its 1-based column number.  --columns (the grammar of `epilogos --columns`) selects and orders the
rows and columns that are written; the counting and the warning are about the whole matrix.  The tables are a report: the exit
status is 0 whatever they hold.  Pairs of biosamples that hold a state in the same bins and the same state in every one of them
-- a file that was put in twice -- get one warning line on stderr.  There is no CPU fallback."""
import sys
from pathlib import Path

import click
import numpy as np


def biosample_names(N, names=None):
    """The N row / column heads: names[k] where the list has one, else the 1-based column number."""
    names = list(names or [])
    return [names[k] if k < len(names) and names[k] else str(k + 1) for k in range(N)]


def table_lines(M, names=None, cols=None):
    """M: int [N, N]; names: see biosample_names; cols: 0-based columns to write, in that order (None: all) -> the lines."""
    M = np.asarray(M, dtype=np.int64)
    N = M.shape[0]
    heads = biosample_names(N, names)
    cols = list(range(N)) if cols is None else [int(c) for c in cols]
    lines = ["\t".join(["biosample"] + [heads[c] for c in cols])]
    for r in cols:
        lines.append("\t".join([heads[r]] + [str(int(M[r, c])) for c in cols]))
    return lines


def write_tables(prefix, agree, both, names=None, cols=None):
    """-> the two paths written, PREFIX.agree.tsv and PREFIX.both.tsv."""
    paths = []
    for tag, M in (("agree", agree), ("both", both)):
        p = Path(str(prefix) + "." + tag + ".tsv")
        p.write_text("\n".join(table_lines(M, names, cols)) + "\n")
        paths.append(p)
    return paths


def duplicate_pairs(agree, both):
    """Pairs i < j with agree[i, j] == both[i, i] == both[j, j] > 0, in row-major order: [(i, j)]."""
    agree, both = np.asarray(agree, dtype=np.int64), np.asarray(both, dtype=np.int64)
    d = np.diag(both)
    same = (agree == d[:, None]) & (agree == d[None, :]) & (d[:, None] > 0)
    i, j = np.nonzero(np.triu(same, k=1))
    return list(zip(i.tolist(), j.tolist()))


def duplicate_warning(agree, both, names=None):
    """The one warning line about duplicate_pairs, None when there is none."""
    pairs = duplicate_pairs(agree, both)
    if not pairs:
        return None
    heads = biosample_names(np.asarray(agree).shape[0], names)
    i, j = pairs[0]
    return ("WARNING: {} pair(s) of biosamples hold a state in the same bins and the same state in every one of them; the first is "
            "{} (column {}) and {} (column {})".format(len(pairs), heads[i], i + 1, heads[j], j + 1))


def check_columns(cols, N):
    if cols is not None and len(cols) and int(max(cols)) >= N:
        raise click.UsageError("[--columns] biosample {} is not in the matrices: they have {} biosample columns".format(int(max(cols)) + 1, N))


class Tally:
    """The sums over matrices, on the device: add() every resident matrix, then finish()."""

    def __init__(self):
        self.agree = self.both = None
        self.N, self.first = 0, None

    def add(self, X, N, S, what):
        """X: a resident int8 matrix of N biosample columns and S states (None: a file without rows, only its width counts); what:
        its file (or chromosome), for the error."""
        from . import engine
        if X is None and N == 0:                           # (a file without a line has no width either)
            return
        if self.first is None:
            self.N, self.first = N, what
        elif N != self.N:
            raise click.UsageError("{} has {} biosample columns and {} has {}: the concordance sums over matrices of one width"
                                   .format(self.first, self.N, what, N))
        if X is not None and N > 0:
            self.agree, self.both = engine.concordance(X, N, S, agree=self.agree, both=self.both)

    def finish(self):
        """-> (agree, both) as host int64 [N, N].  Synchronises."""
        if self.agree is None:
            z = np.zeros((self.N, self.N), dtype=np.int64)
            return z, z.copy()
        return self.agree.cpu().numpy(), self.both.cpu().numpy()

    def write(self, prefix, names=None, cols=None, err=None):
        agree, both = self.finish()
        check_columns(cols, self.N)
        paths = write_tables(prefix, agree, both, names, cols)
        line = duplicate_warning(agree, both, names)
        if line:
            print(line, file=err or sys.stderr, flush=True)
        return paths


def upload(path):
    """One input file, read once as its bytes are -> (X resident int8 [R, ldx] or None when it has no cell, N)."""
    import torch
    from . import engine
    from .helpers import readTable
    width = [0]

    def alloc(R, N):                                   # (called by the reader once it knows the file's shape)
        width[0] = N
        return np.empty((R, engine.padded_width(N)), dtype=np.int8)
    arr, _loc = readTable(path, alloc=alloc, raw=True)
    R, N = arr.shape[0], width[0]
    if R == 0 or N == 0:
        return None, N
    return torch.from_numpy(np.ascontiguousarray(arr)).to("cuda"), N


def run(inputs, stateInfo, prefix, names=None, columns=None, err=None):
    """The command: -> (agree, both) of all files as host arrays."""
    from . import _io, census, engine
    from .helpers import getNumStates
    from .run import parseColumns
    engine.require_gpu()
    S = getNumStates(stateInfo)
    if not 1 <= S <= 127:
        raise click.UsageError("the state model of {} has {} states: 1 .. 127 are supported".format(stateInfo, S))
    try:
        cols = parseColumns(columns) if columns is not None else None
    except ValueError as e:
        raise click.UsageError("[--columns] {}".format(e))
    _io.set_state_limit(S)
    biosamples = census.read_names(names) if names else None
    tally = Tally()
    for f in census.input_files(inputs):
        X, N = upload(f)
        tally.add(X, N, S, f)
        del X
    tally.write(prefix, biosamples, cols, err)
    return tally.finish()


@click.command(context_settings={"help_option_names": ["-h", "--help"]})
@click.option("-i", "--input", "inputs", multiple=True, required=True, type=click.Path(exists=True),
              help="A directory of the matrix files `epilogos -i` takes (.epgm, .txt, .txt.gz), or single files; may be repeated")
@click.option("-j", "--state-info", "stateInfo", required=True, type=click.Path(exists=True, dir_okay=False), help="State model info file")
@click.option("-o", "--output", "prefix", required=True, type=click.Path(dir_okay=False), help="PREFIX of PREFIX.agree.tsv and PREFIX.both.tsv")
@click.option("--names", "names", type=click.Path(exists=True, dir_okay=False), default=None,
              help="Biosample metadata (column 1 behind the header line): line k names biosample column k")
@click.option("--columns", "columns", type=str, default=None,
              help="The biosamples to write, in this order: 1-based numbers and ranges (\"5,1-2\") or @file, as `epilogos --columns`")
def main(inputs, stateInfo, prefix, names, columns):
    """Pairwise concordance of biosamples: bins in the same state and bins both in a state, for every pair, counted on the GPU."""
    run(inputs, stateInfo, prefix, names, columns)


def cli(argv=None):
    main.main(args=argv, standalone_mode=True)


if __name__ == "__main__":
    cli()
