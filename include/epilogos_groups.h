/*
 * epilogos_groups.h -- C ABI of the column-group count pass (csrc/epg_groups.hip), part of libepilogos_hip.so.
 *
 * The scoring commands take "a group of biosamples" as a matrix of its own.  Real inputs come as ONE matrix of all biosamples,
 * and the groups people score (male / female, tissue groups, any two of them in paired mode) are column subsets of it.  This
 * entry point counts up to four such subsets in one pass over the whole matrix: every row is read once and one per-bin
 * histogram is written per group.  Everything behind the count pass (scores, S2 pair counts, null draws, quiescence) works
 * from per-bin histograms already, so a group never has to exist as a matrix.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing and allocates no workspace.  EPG_ABI_VERSION of epilogos_amd.h is not changed by this header.
 *
 * Limits: 1 <= G <= EPG_GROUPS_MAX groups per call, S <= 31 states (the five-bit counting core), N <= 65535 columns.  A caller
 * with a wider model or with S3 (which needs the states, not the counts) gathers the columns into a matrix of their own.
 */
#ifndef EPILOGOS_GROUPS_H
#define EPILOGOS_GROUPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPG_GROUPS_MAX 4

/* X: int8 [R, ldx] states, the byte contract of epg_bin_hist (0 .. S-1 a state; S .. 31 and 0xFF counted nowhere; only N bytes
 * of a row are read as states, padding may hold anything).
 * member: device uint8 [N]; bit g of member[c] says that column c belongs to group g.  A column may belong to no group or to
 * several; bits G .. 7 are ignored.  A group without a column is legal: its rows are zeros.
 * H: HOST array of G device pointers, H[g] = uint16 [R, S], 16-byte aligned: H[g][b, s] = #{c < N : bit g of member[c] set and
 * X[b, c] == s}.  The array, or single entries, may be NULL: that histogram is not written.
 * counts: device int64 [G * S], counts[g * S + s] += sum over b of H_g[b, s]; may be NULL.
 * EPG_ERR_UNSUPPORTED: S > 31, G > EPG_GROUPS_MAX, N > 65535.  EPG_ERR_INVALID_ARG: R < 0, N < 1, S < 1, G < 1, ldx < N, X or member
 * NULL, an H[g] that is not 16-byte aligned (rows are stored as 16-byte vectors), H and counts both NULL.  Order of the checks: the
 * shape (R, N, ldx, S, G below their minimum) first, then the three unsupported sizes, then the pointers; a call with several
 * offences reports the first.  R == 0 does nothing. */
int epg_bin_hist_groups(const int8_t* X, int64_t R, int32_t N, int64_t ldx, int32_t S, int32_t G, const uint8_t* member,
                        uint16_t* const* H, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_GROUPS_H */
