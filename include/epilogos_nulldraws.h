/*
 * epilogos_nulldraws.h -- C ABI of the K-draw null of paired mode (csrc/epg_null.hip, csrc/epg_null_exceed.hip), part of
 * libepilogos_hip.so.
 *
 * Paired mode turns real distances into p-values through a null distribution.  The null groups of a bin are an exact
 * multivariate-hypergeometric draw from the bin's two histograms, a pure function of (seed, row key, histograms), and a whole
 * genome's draw costs milliseconds: with K draws per bin the pooled null is large enough to give every real distance an
 * EMPIRICAL p-value, p = (1 + #{null >= |d|}) / (1 + M).  Two entry points: the K draws of every bin as null DISTANCES in one
 * kernel, and the exceedance counts of the real distances against a chunk of them.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing.  EPG_ABI_VERSION of epilogos_amd.h is not changed by this header.
 */
#ifndef EPILOGOS_NULLDRAWS_H
#define EPILOGOS_NULLDRAWS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* K null distances per bin of several parts, paired S1.
 * HA, HB, R, row0: HOST arrays of nparts entries as for epg_null_hist_from_binhist_parts -- device uint16 [R[p], S] histograms of
 * the two real groups (16-byte aligned), the rows of the part and the shuffle key of its first row.
 * mask: HOST array of nparts device pointers, uint8 [R[p]], or NULL, or single entries NULL: a row whose byte is not 0 (a
 * quiescent bin) is not drawn and gets NaN, the value epg_null_exceed leaves out.
 * NA + NB: the columns of a row; ga, gb: the widths of the null groups (ga + gb <= NA + NB).  TnA, TnB: device float32
 * [ga + 1, S] and [gb + 1, S], the S1 score tables of the null groups' widths (as for epg_pair_scores_s1_parts).
 * seeds: HOST array of K seeds.  out: HOST array of nparts device pointers, float32 [K, R[p]].
 * out[p][k, b] is, bit for bit, the null distance that epg_null_hist_from_binhist_parts with seed seeds[k] followed by
 * epg_pair_scores_s1_parts gives for bin b of part p.  Rows of R[p] == 0 are skipped; nothing else is written.
 * EPG_ERR_INVALID_ARG: nparts < 0, S outside 1 .. 127, NA or NB outside 1 .. 65535, K < 1, ga or gb < 1, ga + gb > NA + NB, a NULL
 * pointer, a histogram that is not 16-byte aligned.  EPG_ERR_UNSUPPORTED (checked after the shape, before the pointers; nothing is
 * touched): S > 31; rows too wide for the bit-string sampler (more than 3072 columns when ga + gb == NA + NB, else more than
 * 1536); null tables that leave no room for four waves in a CU's 160 KB of LDS.  The caller then loops over the two calls
 * named above: the same values. */
int epg_null_dist_draws_parts(int32_t nparts, const uint16_t* const* HA, const uint16_t* const* HB, const int64_t* R, const int64_t* row0,
                              const uint8_t* const* mask, int32_t S, int32_t NA, int32_t NB, int32_t ga, int32_t gb, const float* TnA,
                              const float* TnB, const uint64_t* seeds, int32_t K, float* const* out, void* stream);

/* Workspace bytes of epg_null_exceed for n null distances: two uint32 [n] key arrays and the radix sort's temporary.
 * -1: n < 0 or beyond 2^31 - 1 (split the pool into chunks). */
int64_t epg_null_exceed_ws_bytes(int64_t n);

/* exceed[b] += #{ i < n : null[i] is not NaN and |null[i]| >= |d[b]| }, compared as float32 values, for b < R.
 * null: device float32 [n]; d: device float32 [R]; exceed: device int64 [R], ACCUMULATES (the caller zeroes it once and calls per
 * chunk of the pool).  A d[b] that is NaN counts nothing.  ws: device workspace of at least epg_null_exceed_ws_bytes(n) bytes,
 * 256-byte aligned (EPG_ERR_WORKSPACE when smaller).  One radix sort of the keys (the bit patterns of |x|, monotone for floats)
 * and one pass with a lane per real bin; no atomics.  n == 0 or R == 0 does nothing. */
int epg_null_exceed(const float* null, int64_t n, const float* d, int64_t R, int64_t* exceed, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_NULLDRAWS_H */
