"""Similarity search, the live query: `similaritySearch_run -q REGION_OR_BED -s scores.txt.gz -o out/` searches any region
against the whole scores file on the GPU, with no built index.  The reference can only look a region up among the ones its -b
picked (similaritySearch_run.py:237-285 querySimSearch); here the scores file is gridded (to_grid), kept on the device, block-reduced
there (epg_simsearch_reduce), the query windows are sliced there (epg_simsearch_slices) and searched by the build's STEP 2
(epg_simsearch) -- the same exact integers, so a query at the coordinates of a region that -b picked writes the file the lookup
writes from the built index.

The window of a query chr:start-end (windowFirstBin): anchor = start + (end - start - windowBP) // 2 -- a region of exactly windowBP
is taken as given, a longer one gives its central window, a shorter one is grown around its centre; the first bin is the
chromosome's bin that contains the anchor; the window is the windowBins bins from there, shifted to lie inside the chromosome
when it would stick out at either end.  A chromosome's bins are contiguous rows of the scores file (as selfStarts assumes).

The scores file is read by readGrid: on the GPU as text (scoresText.read_scores_device, a strict parser), by pandas
(similaritySearch_max_mean.readScores) when there is no GPU or the file is outside the parser's grammar.

The device steps are module-level functions (readGrid, reduceGenome, slices, search): a host test puts numpy in place of the
last three."""
from pathlib import Path
from time import time

import numpy as np

from . import _abi
from . import similaritySearch_calc as calc
from . import similaritySearch_max_mean as mm
from . import similaritySearch_write as wr


def chromosomeTable(chroms, starts, ends):
    """{chromosome: (first row, starts int64 [n], ends int64 [n])} of a scores file's coordinate columns; every chromosome's bins
    are one run of rows (a chromosome that comes back after another is refused)."""
    chroms = np.asarray(chroms).astype(str)
    starts = np.asarray(starts).astype(np.int64)
    ends = np.asarray(ends).astype(np.int64)
    edges = np.concatenate(([0], np.where(chroms[1:] != chroms[:-1])[0] + 1, [len(chroms)])) if len(chroms) else np.array([0])
    table = {}
    for a, b in zip(edges[:-1], edges[1:]):
        if chroms[a] in table:
            raise ValueError("similarity search: the bins of %s are not contiguous rows of the scores file" % chroms[a])
        table[str(chroms[a])] = (int(a), starts[a:b], ends[a:b])
    return table


def windowFirstBin(table, chrom, start, end, windowBP, windowBins):
    """Row index (in the scores file) of the first bin of the window searched for chrom:start-end; ValueError when there is none
    (unknown chromosome, chromosome shorter than the window)."""
    if chrom not in table:
        raise ValueError("chromosome %s is not in the scores file" % chrom)
    row0, starts, _ends = table[chrom]
    if len(starts) < windowBins:
        raise ValueError("%s has %d bins, fewer than the %d of the window" % (chrom, len(starts), windowBins))
    anchor = int(start) + (int(end) - int(start) - int(windowBP)) // 2
    b = int(np.searchsorted(starts, anchor, side="right")) - 1          # the bin that contains the anchor
    b = min(max(b, 0), len(starts) - windowBins)
    return row0 + b


def readGrid(scoresPath, inflate="host"):
    """(coords object [R, 3]: chromosome, start, end; genome int64 [R, S]: the scores x 1e5), host arrays with the values of
    mm.readScores(scoresPath)'s inputArr[:, :3] and third result.  With a GPU the file is parsed there as text; a file the strict
    parser refuses gets one warning line and is read by mm.readScores, so that it behaves as it always did (to_grid's ValueError
    for values off the grid included).  inflate "gpu" (--inflate gpu): a BGZF file is inflated on the device too."""
    import torch
    from . import scoresText
    if torch.cuda.is_available() and _abi.lib_path().exists():
        try:
            x, start, end, runs = scoresText.read_scores_device(scoresPath, **({"inflate": inflate} if inflate != "host" else {}))
        except scoresText.NotStrict as e:
            print("            Warning: %s is not a plain \"%%.5f\" scores file (row %d: %s); reading it with pandas"
                  % (scoresPath, e.row, e.reason), flush=True)
        else:
            coords = np.empty((len(start), 3), dtype=object)
            for name, a, b in runs:
                coords[a:b, 0] = name
            coords[:, 1], coords[:, 2] = start, end
            return coords, x.cpu().numpy().astype(np.int64)
    _scores, inputArr, genome = mm.readScores(scoresPath)
    return inputArr[:, :3], genome


def reduceGenome(genome, blockSize):
    """genome int64 [R, S] (gridded scores) -> the device state of a query run: (x int32 [R, S], g int32 [ceil(R / blockSize), S]
    = its block reduction, g's state ranges), device tensors."""
    import torch
    from . import engine
    engine.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(np.ascontiguousarray(genome, dtype=np.int32)).to(dev)
    g = engine.simsearch_reduce(x, blockSize)
    return x, g, calc.tensor_ranges(g)


def slices(state, first, nblk, blockSize):
    """The block-reduced slices of the windows that start at rows `first` (int64 [B]): int32 [B, nblk, S], a device tensor."""
    from . import engine
    return engine.simsearch_slices(state[0], first, nblk, blockSize)


def search(state, first, nblk, blockSize, nDesiredMatches, ws_cap=None, batch=None):
    """Indices int32 [B, n] into the reduced genome of the matches of the windows that start at rows `first`: slices and STEP 2's
    search per batch under the build's workspace cap (similaritySearch_calc.WS_CAP_BYTES when ws_cap is None)."""
    import torch
    _x, g, g_range = state
    first = np.asarray(first, dtype=np.int64)

    def batch_of(r0, r1):
        ss = torch.from_numpy((first[r0:r1] // blockSize).astype(np.int32)).to(g.device)
        return slices(state, first[r0:r1], nblk, blockSize), ss
    idx, _mode = calc.search_on_device(g, g_range, len(first), int(nblk), nDesiredMatches, batch_of,
                                       calc.WS_CAP_BYTES if ws_cap is None else ws_cap, batch)
    return idx


def recsText(indices, reducedCoords, nblk):
    """The lines of a *_recs.bed file: chromosome and start of each match's first reduced bin, end of its last (the end rule of
    convertIndicesToCoords); -1 slots are dropped, as bedText drops them."""
    keep = indices[indices != -1]
    return "".join("{}\t{}\t{}\n".format(reducedCoords[i, 0], reducedCoords[i, 1], reducedCoords[i + nblk - 1, 2]) for i in keep)


def liveQuery(query, scoresPath, outputDir, windowBP, nDesiredMatches, inflate="host"):
    """One similarity_search_region_{chr}_{start}_{end}_recs.bed per query region, named by the window that was searched."""
    from .similaritySearch_run import generateRegionArr, windowParameters
    print("\n\n\n        Reading in data...", flush=True); readTime = time()
    queryArr = generateRegionArr(query)
    windowBP, windowBins, blockSize = windowParameters(scoresPath, windowBP)
    nblk = windowBins // blockSize
    coords, genome = readGrid(scoresPath, **({"inflate": inflate} if inflate != "host" else {}))
    table = chromosomeTable(coords[:, 0], coords[:, 1], coords[:, 2])
    print("            Time:", format(time() - readTime, '.0f'), "seconds\n", flush=True)
    print("        Querying regions...", flush=True)
    found, first = [], []
    for chrom, start, end in queryArr:
        try:
            first.append(windowFirstBin(table, str(chrom), start, end, windowBP, windowBins))
            found.append((chrom, start, end))
        except ValueError as e:
            print("            ValueError: Could not find region in given query range: {}:{}-{} ({})\n".format(chrom, start, end, e))
    if not found:
        return
    state = reduceGenome(genome, blockSize)
    indices = search(state, np.array(first, dtype=np.int64), nblk, blockSize, nDesiredMatches)
    reducedCoords = wr.reduceGenomeCoords(coords, blockSize)
    for (chrom, start, end), f, idx in zip(found, first, indices):
        regionChr, regionStart, regionEnd = coords[f, 0], coords[f, 1], coords[f + windowBins - 1, 2]
        outfile = Path(outputDir) / "similarity_search_region_{}_{}_{}_recs.bed".format(regionChr, regionStart, regionEnd)
        with open(outfile, "w+") as fh:
            fh.write(recsText(idx, reducedCoords, nblk))
        print("            Searched region {}:{}-{} for user query {}:{}-{}".format(regionChr, regionStart, regionEnd, chrom,
                                                                                    start, end))
        print("                See {} for matches\n".format(outfile), flush=True)
