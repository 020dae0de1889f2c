"""numpy int64 restatement of the similarity search of one region of interest (the reference's runEuclideanDistance,
similaritySearch_calc.py:67-123, on exact integers): the yardstick of tests/test_hip_simsearch.py and of the golden generator."""
import numpy as np


def distances(G, q):
    """G int64 [Pg, S], q int64 [W, S] -> D int64 [Pg - W + 1], D[p] = sum (G[p:p+W] - q)^2."""
    W = q.shape[0]
    P = G.shape[0] - W + 1
    D = np.zeros(P, dtype=np.int64)
    for k in range(W):
        D += ((G[k:k + P] - q[k]) ** 2).sum(axis=1)
    return D


def mode(D):
    """scipy.stats.mode: the most frequent value, the smallest on ties."""
    vals, counts = np.unique(D, return_counts=True)
    return int(vals[np.argmax(counts)])


def pick(D, selfStart, W, n):
    """(indices int32 [n], mode): stable order, overlap test before the threshold test, -1 fill on the threshold, zeros when the
    candidates run out."""
    m = mode(D)
    out = np.zeros(n, dtype=np.int32)
    picked = [int(selfStart)]
    k = 0
    for h in np.argsort(D, kind="stable"):
        if any(abs(int(h) - p) < W for p in picked):
            continue
        if 2 * int(D[h]) > m:
            out[k:] = -1
            break
        out[k] = h
        picked.append(int(h))
        k += 1
        if k >= n:
            break
    return out, m


def search(G, Q, selfStarts, n):
    """All rows: (indices int32 [R, n], modes int64 [R])."""
    idx = np.zeros((len(Q), n), dtype=np.int32)
    modes = np.zeros(len(Q), dtype=np.int64)
    for r in range(len(Q)):
        idx[r], modes[r] = pick(distances(G, Q[r]), selfStarts[r], Q.shape[1], n)
    return idx, modes


def chr1_scores_file(path):
    """Write the S1 scores file of the chr1 example (tests/golden/chr1_full.npz: oracle scores, native writer) to `path` and
    check it against the reference's text by its SHA-256; returns path."""
    import gzip
    import hashlib
    from pathlib import Path

    from epilogos_amd import _io
    from oracle import oracle_np as onp
    g = np.load(Path(__file__).resolve().parent / "golden" / "chr1_full.npz")
    x = g["x"]
    R = x.shape[0]
    s32 = onp.score_s1(x, onp.normalise(onp.expected_s1(x, 18)), 18).astype(np.float32)
    start = int(g["start0"]) + 200 * np.arange(R, dtype=np.int64)
    blob = "".join("chr1\t%d\t%d\n" % (s, s + 200) for s in start).encode()
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum([len(line) + 1 for line in blob.decode().split("\n")[:-1]], out=off[1:])
    _io.write_scores(path, _io.Locations(np.frombuffer(blob, dtype=np.uint8).copy(), off), s32)
    with gzip.open(path, "rb") as fh:
        assert hashlib.sha256(fh.read()).digest() == g["text_sha256"].tobytes()
    return path
