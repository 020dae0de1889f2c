"""Similarity search STEP 3 -- results as coordinates.  Same signature and outputs as the reference's
epilogos/similaritySearch_write.py (main :14-41, reduceGenomeCoords :44-65, convertIndicesToCoords :88-115, writeResults
:118-170, cleanUpFiles :173-186): simsearch.bed.gz (BGZF), its tabix index simsearch.bed.gz.tbi (zero-based, bed preset) and
simsearch_indices.npy; genome_stats.npz and the per-job index files are removed.

There is no pysam here: the BGZF blocks and the tabix index (the binning and linear index of the SAM/tabix specification) are
written by this module."""
import json
import os
import struct
import sys
import zlib
from pathlib import Path
from time import time

import numpy as np

from .helpers import splitRows

BGZF_BLOCK = 0xff00                           # uncompressed bytes per BGZF block (what bgzip uses)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def reduceGenomeCoords(genomeCoords, blockSize):
    """(reference :44-65) chromosome and start of the first bin and end of the last bin of every block (a partial last block
    included).  genomeCoords: object [G, 3] -> object [ceil(G / blockSize), 3]."""
    G = len(genomeCoords)
    first = np.arange(0, G, blockSize)
    last = np.minimum(first + blockSize, G) - 1
    out = np.empty((len(first), 3), dtype=object)
    out[:, 0], out[:, 1], out[:, 2] = genomeCoords[first, 0], genomeCoords[first, 1], genomeCoords[last, 2]
    return out


def readSimsearchIndices(inputDir, nRegions, nDesiredMatches, nJobs):
    simsearchArr = np.zeros((nRegions, nDesiredMatches), dtype=np.int32)
    rowList = splitRows(nRegions, nJobs)
    for file in Path(inputDir).glob("simsearch_indices_*.npy"):
        i = int(file.stem.split("_")[-1])
        simsearchArr[rowList[i][0]:rowList[i][1]] = np.load(file, allow_pickle=True)
    return simsearchArr


def convertIndicesToCoords(simsearchArr, reducedGenomeCoords, roiCoords, windowBins, blockSize, nRegions, nDesiredMatches):
    """(reference :88-115) [nRegions, 1 + nDesiredMatches, 3]: the ROI, then its matches (index -1 reads the last reduced bin,
    as the reference's iloc does; those slots are dropped when written)."""
    flat = simsearchArr.reshape(-1)
    chrStart = reducedGenomeCoords[flat, :2]
    end = reducedGenomeCoords[flat + windowBins // blockSize - 1, 2].reshape(-1, 1)
    res = np.concatenate((chrStart, end), axis=1).reshape(nRegions, nDesiredMatches, 3)
    return np.concatenate((np.asarray(roiCoords, dtype=object).reshape(nRegions, 1, 3), res), axis=1)


def bedText(searchResults, simsearchArr, roiCoords):
    """The rows of simsearch.bed: chrom, start, stop, JSON list of "chr:start:end" (the ROI first, then its matches), sorted by
    (chrom, start) with string order on chrom (reference :132-150)."""
    rows = []
    keep = np.concatenate((np.ones((len(simsearchArr), 1)), simsearchArr), axis=1) != -1
    for (c, s, e), resultsRow, k in zip(roiCoords, searchResults, keep):
        recs = ['{}:{}:{}'.format(a, b, d) for a, b, d in resultsRow[np.where(k)[0]]]
        rows.append((str(c), int(s), int(e), json.dumps(recs)))
    rows.sort(key=lambda r: (r[0], r[1]))
    return "".join("%s\t%d\t%d\t%s\n" % r for r in rows)


def _bgzf_block(data):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    hdr = struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, ord("B"), ord("C"), 2, len(cdata) + 25)
    return hdr + cdata + struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data))


def bgzf_compress(data):
    """BGZF bytes of data and, per block, (compressed offset, uncompressed offset)."""
    out, blocks, coff = [], [], 0
    for u in range(0, len(data), BGZF_BLOCK):
        blk = _bgzf_block(data[u:u + BGZF_BLOCK])
        blocks.append((coff, u))
        out.append(blk)
        coff += len(blk)
    out.append(BGZF_EOF)
    blocks.append((coff, len(data)))
    return b"".join(out), blocks


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def tabix_index(text, blocks):
    """The .tbi (BGZF-compressed) of a zero-based bed text whose BGZF layout is `blocks` (bgzf_compress): tabix's bed preset,
    one binning index and one linear index (16 kb windows) per chromosome, the chromosomes in order of first appearance."""
    data = text.encode()
    ublk = np.array([u for _c, u in blocks], dtype=np.int64)

    def voff(u):
        i = int(np.searchsorted(ublk, u, side="right")) - 1
        if i == len(blocks) - 1 and i > 0 and u == ublk[i]:
            return blocks[i][0] << 16            # the end of the data: the EOF block
        return (blocks[i][0] << 16) | (u - blocks[i][1])

    refs, order = {}, []
    u = 0
    for line in data.split(b"\n")[:-1] if data.endswith(b"\n") else data.split(b"\n"):
        f = line.split(b"\t")
        name, beg, end = f[0].decode(), int(f[1]), int(f[2])
        if end <= beg:
            end = beg + 1
        v0, v1 = voff(u), voff(u + len(line) + 1)
        u += len(line) + 1
        if name not in refs:
            refs[name] = {"bins": {}, "lin": {}, "beg": v0, "end": v1, "n": 0}
            order.append(name)
        r = refs[name]
        chunks = r["bins"].setdefault(reg2bin(beg, end), [])
        if chunks and chunks[-1][1] == v0:
            chunks[-1][1] = v1                   # adjacent records of a bin share one chunk
        else:
            chunks.append([v0, v1])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if w not in r["lin"] or v0 < r["lin"][w]:
                r["lin"][w] = v0
        r["end"] = v1
        r["n"] += 1
    names = b"".join(n.encode() + b"\0" for n in order)
    out = [b"TBI\1", struct.pack("<i", len(order)), struct.pack("<iiiiii", 0x10000, 1, 2, 3, ord("#"), 0),
           struct.pack("<i", len(names)), names]
    for name in order:
        r = refs[name]
        out.append(struct.pack("<i", len(r["bins"]) + 1))
        for b in sorted(r["bins"]):
            ch = r["bins"][b]
            out.append(struct.pack("<Ii", b, len(ch)))
            out.extend(struct.pack("<QQ", c0, c1) for c0, c1 in ch)
        out.append(struct.pack("<Ii", 37450, 2) + struct.pack("<QQQQ", r["beg"], r["end"], r["n"], 0))   # htslib's pseudo-bin
        nw = max(r["lin"]) + 1 if r["lin"] else 0
        lin, nxt = [0] * nw, r["end"]
        for w in range(nw - 1, -1, -1):           # an empty window takes the next window's offset, as htslib fills it
            nxt = r["lin"].get(w, nxt)
            lin[w] = nxt
        out.append(struct.pack("<i", nw) + struct.pack("<%dQ" % nw, *lin))
    out.append(struct.pack("<Q", 0))
    return bgzf_compress(b"".join(out))[0]


def writeResults(outputDir, searchResults, simsearchArr, roiCoords, nRegions):
    outputDir = Path(outputDir)
    text = bedText(searchResults, simsearchArr, roiCoords)
    gz, blocks = bgzf_compress(text.encode())
    for fn, blob in (("simsearch.bed.gz", gz), ("simsearch.bed.gz.tbi", tabix_index(text, blocks))):
        tmp = outputDir / (fn + ".tmp")
        tmp.write_bytes(blob)
        os.replace(tmp, outputDir / fn)


def cleanUpFiles(outputDir, simsearchArr):
    outputDir = Path(outputDir)
    os.remove(outputDir / "genome_stats.npz")
    for file in outputDir.glob("simsearch_indices_*.npy"):
        os.remove(file)
    np.save(outputDir / "simsearch_indices.npy", simsearchArr, allow_pickle=True)


def main(outputDir, windowBins, blockSize, nJobs, nDesiredMatches):
    outputDir = Path(outputDir)
    print("Reducing genome coordinates...", flush=True); t = time()
    genomeCoords = np.load(outputDir / "genome_stats.npz", allow_pickle=True)["coords"]
    reducedGenomeCoords = reduceGenomeCoords(genomeCoords, blockSize)
    cube = np.load(outputDir / "simsearch_cube.npz", allow_pickle=True)
    nRegions = cube["scores"].shape[0]
    roiCoords = cube["coords"].reshape(nRegions, 3)
    simsearchArr = readSimsearchIndices(outputDir, nRegions, nDesiredMatches, nJobs)
    searchResults = convertIndicesToCoords(simsearchArr, reducedGenomeCoords, roiCoords, windowBins, blockSize, nRegions,
                                           nDesiredMatches)
    print("Writing search results...", flush=True)
    writeResults(outputDir, searchResults, simsearchArr, roiCoords, nRegions)
    cleanUpFiles(outputDir, simsearchArr)
    print("Total time:", format(time() - t, '.0f'), "seconds\n", flush=True)


if __name__ == "__main__":
    main(Path(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
