/*
 * epilogos_simsearch_pick.h -- C ABI of the device STEP 1 of `simsearch -b --step1 gpu` (csrc/epg_simsearch_pick.hip), part of
 * libepilogos_hip.so: the centre score of every bin, the rolling maximum, the rank of every window by (rolling max, rolling mean,
 * centre score) and the greedy pick of non-overlapping windows -- roiSingle.maxMean on the device, bit for bit.
 *
 * The pick.  The host walks the windows best first and takes a window when none of the W positions it covers is covered yet
 * (roiSingle.maxMean).  In the compacted index space two windows conflict iff |i - j| < W, so the walk's set is the fixed point of two
 * local rules over the states undecided / picked / dropped: an undecided i is PICKED when no undecided j with |i - j| < W has a
 * smaller rank, and DROPPED when a j with |i - j| < W is picked.  Both rules are monotone (a state never goes back), so they may be
 * applied in any order and on stale neighbour states: a workgroup iterates them to a fixed point inside a tile of EPG_PICK_TILE
 * positions held in LDS, with the states of the W - 1 halo positions on either side frozen at what the previous sweep left, and one
 * launch sweeps all tiles.  A stretch of tied windows (ranked by position) is resolved inside each tile: it costs a sweep per tile
 * it crosses, not one per W positions.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing.  EPG_ABI_VERSION of epilogos_amd.h is not changed by this header.  No grid here is sized by the device's
 * compute-unit count: epg_test_force(5, n) changes nothing.
 */
#ifndef EPILOGOS_SIMSEARCH_PICK_H
#define EPILOGOS_SIMSEARCH_PICK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Positions of a pick tile (a workgroup's share of a sweep); the halo on either side is W - 1 positions. */
#define EPG_PICK_TILE 2048
/* Largest window (in positions) of epg_simsearch_rolling_max and epg_simsearch_pick: tile and halos fit 48 KB of LDS. */
#define EPG_PICK_MAX_W 1024

/* score[r] = ((X[r, 0] / 1e5 + X[r, 1] / 1e5) + X[r, 2] / 1e5) + ... in float64, every division correctly rounded and the adds in
 * column order, never fused: the value of pandas' scores.iloc[:, 3:].sum(axis=1) on the "%.5f" file that X is the grid of.
 * X: device int32 [R, S], read; score: device float64 [R], written (8-byte aligned).  Nothing else is touched, no workspace.
 * EPG_ERR_INVALID_ARG: R < 0, S < 1, a NULL pointer with R > 0.  R == 0 does nothing. */
int epg_simsearch_rowscore(const int32_t* X, int64_t R, int32_t S, double* score, void* stream);

/* out[i] = max(v[i - W / 2 .. i + (W - 1) / 2]), NaN where that window leaves [0, n): pandas' Series.rolling(W, center=True).max()
 * (_io.rolling_max) for a vector without NaN.  v: device float64 [n], read; out: device float64 [n], written; they must not
 * overlap.  No workspace.  EPG_ERR_INVALID_ARG: n < 0, W < 1, a NULL pointer with n > 0; EPG_ERR_UNSUPPORTED: W > EPG_PICK_MAX_W. */
int epg_simsearch_rolling_max(const double* v, int64_t n, int32_t W, double* out, void* stream);

/* Workspace bytes of epg_simsearch_rank for n windows: two uint64 [n] key arrays, two uint32 [n] index arrays and the radix
 * sort's temporary (about 24 n bytes).  -1: n < 0 or beyond 2^31 - 1. */
int64_t epg_simsearch_rank_ws_bytes(int64_t n);

/* rank[i] = the position of i in np.lexsort((-score, -rmean, -rmax)): descending by rmax, then rmean, then score; equal triples in
 * index order (three stable descending radix sorts over order-preserving 64-bit images of the doubles, least significant key
 * first).  -0.0 and +0.0 are the same key.  The keys must hold no NaN.
 * rmax, rmean, score: device float64 [n], read; rank: device uint32 [n], written, a permutation of 0 .. n - 1.  ws: device
 * workspace of at least epg_simsearch_rank_ws_bytes(n) bytes, 256-byte aligned (EPG_ERR_WORKSPACE when smaller).
 * EPG_ERR_INVALID_ARG: n outside 0 .. 2^31 - 1, a NULL pointer with n > 0, a misaligned workspace.  n == 0 does nothing. */
int epg_simsearch_rank(const double* rmax, const double* rmean, const double* score, int64_t n, uint32_t* rank, void* ws,
                       int64_t ws_bytes, void* stream);

/* Workspace bytes of epg_simsearch_pick: two uint8 [n] state arrays, two uint32 [ceil(n / W)] arrays for the cap, two uint32
 * [ceil(n / EPG_PICK_TILE)] arrays of the compaction, the sweep counters and the radix sort's temporary (about 2 n bytes).
 * Negative: the code of a shape epg_simsearch_pick refuses. */
int64_t epg_simsearch_pick_ws_bytes(int64_t n, int32_t W);

/* The greedy pick.  rank: device uint32 [n], a permutation of 0 .. n - 1 (epg_simsearch_rank), read.  Position i is taken when,
 * walking the positions by ascending rank, no taken j has |i - j| < W; the walk stops after maxRegions picks.
 * picked: device int64 [ceil(n / W)] (two picks are W or more apart: there are never more); its first n_picked[0] entries are
 * written, the picked positions in ASCENDING order -- with more than maxRegions in the uncapped set, the maxRegions of smallest
 * rank.  n_picked: device int64 [1].  launches: HOST int32 [1], the number of sweeps over the tiles until nothing was undecided.
 * ws: device workspace of at least epg_simsearch_pick_ws_bytes(n, W) bytes, 256-byte aligned.
 *
 * Launches and synchronisations.  Sweeps are launched four at a time; each adds the positions it leaves undecided to a counter of
 * its own, and the host reads the four counters after the fourth (one stream synchronisation per four sweeps; a sweep over decided
 * tiles only copies their states).  Termination does not depend on which workgroups run together: there is no barrier between
 * workgroups, a sweep reads the previous sweep's states and writes its own.  A sweep decides every position whose chain of
 * better-ranked undecided neighbours stays inside its tile plus halo, so a chain costs one sweep for every tile boundary it
 * crosses.  Keys that are monotone over a stretch (a plateau of ties, a ramp) cross each boundary once: at most
 * ceil(n / EPG_PICK_TILE) sweeps, ceil(ceil(n / EPG_PICK_TILE) / 4) synchronisations.  Noise-like keys need 2 to 4 sweeps.  The
 * bound for ANY permutation is n sweeps (every sweep decides at least the best undecided position); EPG_ERR_HIP beyond it.
 * After the sweeps: the compaction of the picked positions (three kernels; with maxRegions below ceil(n / W) once more before, for
 * the picked ranks, with a radix sort of ceil(n / W) keys that finds the rank the cap cuts at), no further synchronisation.
 * The call returns after its last synchronisation; the outputs are complete when the stream's work is.
 *
 * EPG_ERR_INVALID_ARG: n outside 0 .. 2^31 - 2, W < 1, maxRegions < 0, a NULL pointer, a misaligned workspace;
 * EPG_ERR_UNSUPPORTED: W > EPG_PICK_MAX_W; EPG_ERR_WORKSPACE.  n == 0 or maxRegions == 0 writes n_picked[0] = 0, launches[0] = 0. */
int epg_simsearch_pick(const uint32_t* rank, int64_t n, int32_t W, int64_t maxRegions, int64_t* picked, int64_t* n_picked,
                       int32_t* launches, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_SIMSEARCH_PICK_H */
