"""Host reference of the paired-mode null-group draws: numpy and Python integers only, no torch, no GPU.

Written from the specification in the header comment of epilogos_amd/csrc/epg_null.hip, not from the kernels: Philox4x32-10, the
16-bit draw rule with its 48-bit tie rule (sample_from_hist: what epg_null_hist_from_binhist*, epg_pair_count_null_parts and
epg_null_dist_draws_parts draw) and the 32-bit rule of the matrix-scanning epg_null_hist (sample_from_matrix).
tests/test_null_sampler_ref.py shows on the CPU that the rule is exact and that it reproduces tests/golden/null_draws.json;
tests/test_hip_null_sampler_exact.py holds the kernels against it bit for bit.

The second half is the case list of tests/golden/null_draws.json and its input generators, shared with
tests/test_hip_null_draws.py (which runs them on the device)."""
import hashlib
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "null_draws.json"

U32 = 0xFFFFFFFF
TAG_DRAWS = 0x6E756C6C                         # "null": the main stream, eight 16-bit draws per call
TAG_TIES = 0x74696573                          # "ties": the second stream, one 32-bit word per tie
A, B, NEITHER, TIE = 0, 1, 2, 3                # what a draw decides


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123): counter = four and key = two 32-bit words, each an integer or an array of
    them (broadcast against one another) -> uint32 [..., 4]."""
    mask = np.uint64(U32)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & mask for x in counter])
    k0, k1 = (np.asarray(k, dtype=np.uint64) & mask for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2        # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _row_call(seed, keys, call, tag):
    """One call of a row stream for the rows with the shuffle keys `keys` (uint64 array): counter (key lo, key hi, call, tag)."""
    keys = np.asarray(keys, dtype=np.uint64)
    return philox4x32_10((keys, keys >> np.uint64(32), call, tag), (seed & U32, (seed >> 32) & U32))


def decide16(v, rem, needA, needAB):
    """What the 16 bits v decide for a column when `rem` columns are left and the groups still need needA / needAB - needA of
    them: u lies in [v, v + 1) / 65536 and u * rem in [t, t + rem) / 65536.  Integers or int64 arrays."""
    t = v * rem
    a = t + rem <= needA << 16
    b = (t >= needA << 16) & (t + rem <= needAB << 16)
    none = t >= needAB << 16
    return np.where(a, A, np.where(b, B, np.where(none, NEITHER, TIE)))


def tie_pick(v, w, rem):
    """The 48-bit uniform number (v, w) scaled to [0, rem).  Python integers."""
    return (((int(v) << 32) | int(w)) * int(rem)) >> 48


def from_pick(pick, needA, needAB):
    return A if pick < needA else (B if pick < needAB else NEITHER)


def sample_from_hist(hA, hB, n_cols, ga, gb, seed, key0):
    """The null groups of R rows from the real groups' histograms hA, hB (uint16 [R, S]); row r has the shuffle key key0 + r.
    -> (oA, oB uint16 [R, S], info); info counts the ties of the call: at the A threshold ("ties_A"), at the A-or-B threshold
    ("ties_AB"), and each of the two split into those of a row's last 1 .. 7 draws ("tail_A", "tail_AB") and those of a full
    call of eight ("full_A", "full_AB"); "edge_A" / "edge_AB" count the draws whose interval ENDS at the threshold,
    (v + 1) rem == need << 16, which are decided without a tie."""
    h = np.asarray(hA, dtype=np.int64) + np.asarray(hB, dtype=np.int64)
    R, S = h.shape
    rows = np.arange(R)
    modal = np.argmax(h, axis=1)                                           # the first maximum
    m = n_cols - h[rows, modal]                                            # positions that are drawn
    keys = (np.uint64(key0 & 0xFFFFFFFFFFFFFFFF) + rows.astype(np.uint64))
    needA, needAB = np.full(R, ga, dtype=np.int64), np.full(R, ga + gb, dtype=np.int64)
    M = int(m.max()) if R else 0
    out = np.full((R, M), NEITHER, dtype=np.int8)                          # the outcome at every position
    tie_words, tie_calls = {}, {}                                          # row -> its tie stream's unused words / calls made
    info = dict.fromkeys(("ties_A", "ties_AB", "tail_A", "tail_AB", "full_A", "full_AB", "edge_A", "edge_AB"), 0)
    for d in range(M):
        if d % 8 == 0:
            words = _row_call(seed, keys, d // 8, TAG_DRAWS).astype(np.int64)
        v = (words[:, (d % 8) // 2] >> (16 * (d % 2))) & 0xFFFF            # the low half of a word comes first
        rem = n_cols - d
        dec = decide16(v, rem, needA, needAB)
        live = d < m
        info["edge_A"] += int((live & (needA > 0) & ((v + 1) * rem == needA << 16)).sum())
        info["edge_AB"] += int((live & (needAB > needA) & (needAB < rem) & ((v + 1) * rem == needAB << 16)).sum())
        for r in np.nonzero(live & (dec == TIE))[0]:
            at = "A" if int(v[r]) * rem < int(needA[r]) << 16 else "AB"
            info["ties_" + at] += 1
            info[("tail_" if d >= m[r] // 8 * 8 else "full_") + at] += 1
            if not tie_words.get(r):                                       # the next call of the row's tie stream
                tie_words[r] = [int(w) for w in _row_call(seed, keys[r], tie_calls.get(r, 0), TAG_TIES)]
                tie_calls[r] = tie_calls.get(r, 0) + 1
            dec[r] = from_pick(tie_pick(v[r], tie_words[r].pop(0), rem), int(needA[r]), int(needAB[r]))
        dec = np.where(live, dec, NEITHER)
        out[:, d] = dec
        needA -= dec == A
        needAB -= dec != NEITHER
    # columns in the order [non-modal states ascending | columns without a state | modal]: a state's counts are those of its
    # range of positions; the modal state takes what the groups still need
    hn = h.copy()
    hn[rows, modal] = 0
    edge = np.concatenate([np.zeros((R, 1), dtype=np.int64), np.cumsum(hn, axis=1)], axis=1)
    oA, oB = np.zeros((R, S), dtype=np.int64), np.zeros((R, S), dtype=np.int64)
    for o, what in ((oA, A), (oB, B)):
        cum = np.concatenate([np.zeros((R, 1), dtype=np.int32), np.cumsum(out == what, axis=1, dtype=np.int32)], axis=1)
        o[:] = np.take_along_axis(cum, edge[:, 1:], axis=1) - np.take_along_axis(cum, edge[:, :-1], axis=1)
    oA[rows, modal] = needA
    oB[rows, modal] = needAB - needA
    return oA.astype(np.uint16), oB.astype(np.uint16), info


def sample_from_matrix(xa, xb, S, ga, gb, seed, row0):
    """epg_null_hist's rule: the null groups straight from the state matrices xa [R, NA], xb [R, NB] (int8; a byte outside
    0 .. S - 1 takes part in the draw and is not reported).  Column c of group g takes word c & 3 of the call with the counter
    (row key lo, hi, c >> 2, g); the columns are walked in the order A's, then B's.  -> (oA, oB uint16 [R, S])."""
    xa, xb = np.asarray(xa), np.asarray(xb)
    R = xa.shape[0]
    rows = np.arange(R)
    keys = np.uint64(row0 & 0xFFFFFFFFFFFFFFFF) + rows.astype(np.uint64)
    needA, needB = np.full(R, ga, dtype=np.int64), np.full(R, gb, dtype=np.int64)
    rem = xa.shape[1] + xb.shape[1]
    o = np.zeros((2, R, S + 1), dtype=np.int64)                            # column S: not a state
    for g, x in enumerate((xa, xb)):
        for c in range(x.shape[1]):
            if c % 4 == 0:
                words = philox4x32_10((keys, keys >> np.uint64(32), c >> 2, g), (seed & U32, (seed >> 32) & U32)).astype(np.int64)
            pick = (words[:, c % 4] * rem) >> 32                           # uniform in [0, rem)
            inA = pick < needA
            inB = ~inA & (pick < needA + needB)
            st = x[:, c].astype(np.int64)
            st = np.where((st >= 0) & (st < S), st, S)
            o[0, rows, st] += inA
            o[1, rows, st] += inB
            needA -= inA
            needB -= inB
            rem -= 1
    return o[0, :, :S].astype(np.uint16), o[1, :, :S].astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/golden/null_draws.json and their inputs
# ------------------------------------------------------------------------------------------------------------------------------
SEEDS = (77, 0x9E3779B97F4A7C15)
KEYS = (123456789012, 5, 40000000)             # row0 of the three parts (the second one is empty)

# histogram path: (NA, NB, S, rows of the parts); every entry runs with the default group sizes and with -g, with the library's
# own choice of kernel and with the column-by-column kernel forced, under both seeds
WIDTHS = ((16, 16), (17, 16), (379, 342), (1500, 1572), (1600, 1600), (3000, 3001), (2000, 1200))
HIST_CASES = [(na, nb, 18, (20011, 0, 71) if (na, nb) == (379, 342) else (130, 0, 71)) for na, nb in WIDTHS]
HIST_CASES += [(na, nb, s, (130, 0, 71)) for s in (5, 15, 25, 40) for na, nb in ((17, 16), (379, 342))]
HIST_CASES += [(379, 342, 18, (9,) * 50)]      # more parts than one launch takes
# fused count + draw: its own shapes only (one and four 128-byte groups per row for every S, the flagship's three)
FUSED_CASES = [(na, nb, s, (130, 0, 71)) for s in (15, 18, 25) for na, nb in ((100, 120), (400, 500))]
FUSED_CASES += [(379, 342, 18, (20011, 0, 71)), (379, 342, 18, (70,) * 40)]
FUSED_REFUSED = (100, 300, 18)                 # one and three groups per row: not the fused kernel's


def _states(rng, R, N, S):
    """[R, N] int8 states, one dominant state as in real data; row 3 is all one state, row 5 has columns without a state."""
    p = 1.0 / (1.0 + np.arange(S)[::-1]) ** 2
    x = np.searchsorted(np.cumsum(p / p.sum()), rng.random((R, N))).clip(0, S - 1).astype(np.int8)
    if R > 5:
        x[3, :] = 1
        x[5, ::3] = -1
    return x


def _hist(x, S):
    h = np.zeros((x.shape[0], S), dtype=np.uint16)
    for s in range(S):
        h[:, s] = (x == s).sum(axis=1)
    return h


def _parts(na, nb, S, rows):
    rng = np.random.default_rng([na, nb, S, len(rows)])
    return [(_states(rng, r, na, S), _states(rng, r, nb, S)) for r in rows]


dominant_states, hist = _states, _hist          # (the names other test modules use)


def exceed_inputs(seed, n, R=513):
    """A pool of n null distances (exact zeros of either sign, NaN = left out) and R observed ones with exact ties, zeros and
    values beyond every null: the inputs of the epg_null_exceed tests."""
    rng = np.random.default_rng([seed, n])
    x = (rng.normal(size=n) * 3).astype(np.float32)
    x[rng.random(n) < 0.3] = 0.0                                                # many exact zeros
    x[rng.random(n) < 0.1] = -0.0
    x[rng.random(n) < 0.2] = np.nan                                             # left out
    d = (rng.normal(size=R) * 3).astype(np.float32)
    d[:100] = rng.choice(x, 100) * rng.choice([-1.0, 1.0], 100).astype(np.float32)   # exact ties with pool values, either sign
    d[100:110] = 0.0
    d[110:115] = -0.0
    d[115:120] = np.float32(1e6)                                                # larger than every null: 0
    return x, d


def exceed_np(x, d):
    """#{non-NaN x : |x| >= |d[b]|} per b"""
    a = np.sort(np.abs(x[~np.isnan(x)]))
    return (len(a) - np.searchsorted(a, np.abs(d), side="left")).astype(np.int64)


def _keys(rows):
    return [KEYS[i] if len(rows) == len(KEYS) else 1000 * i for i in range(len(rows))]


def _rows_label(rows):
    return "+".join(map(str, rows)) if len(rows) <= 3 else "%dx%d" % (len(rows), rows[0])


def hist_group_sizes(na, nb):
    """The two group-size settings of a histogram case: the default and -g."""
    g = 6 if na + nb < 100 else 100
    return ((na, nb), (g, g))


def hist_label(na, nb, S, rows, ga, gb, force, seed):
    return "hist NA=%d NB=%d S=%d rows=%s ga=%d gb=%d force_seq=%d seed=%d" % (na, nb, S, _rows_label(rows), ga, gb, force, seed)


def fused_label(na, nb, S, rows, seed):
    return "fused NA=%d NB=%d S=%d rows=%s seed=%d" % (na, nb, S, _rows_label(rows), seed)


def digest_arrays(groups):
    """SHA-256 over lists of host arrays, in order."""
    h = hashlib.sha256()
    for arrays in groups:
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
