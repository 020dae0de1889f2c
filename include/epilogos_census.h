/*
 * epilogos_census.h -- C ABI of the per-biosample state census (csrc/epg_census.hip), part of libepilogos_hip.so.
 *
 * Every count kernel of epilogos_amd.h reduces a state matrix per BIN (row) and decodes only the low five bits of a byte, so a
 * byte that is not a state can alias one (byte 33 counts as state 1 in an 18-state model) and the count check behind the
 * all-reduce cannot see it.  This entry point makes the one pass over X that reduces per COLUMN: how many bins of every
 * biosample are in every state, how many bytes of it are no state at all, and where the first such byte sits.  It is the
 * validator of the byte contract of epilogos_amd.h and the census behind `python -m epilogos_amd.census`.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing and allocates no workspace.  EPG_ABI_VERSION of epilogos_amd.h is not changed by this header.
 */
#ifndef EPILOGOS_CENSUS_H
#define EPILOGOS_CENSUS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* census[n*S + s] += #{ r < R : X[r*ldx + n] == s }            for n < N, s < S   (int64 [N, S], ACCUMULATES)
 * other[n]        += #{ r < R : (uint8) X[r*ldx + n] >= S }     for n < N          (int64 [N],    ACCUMULATES; may be NULL)
 * first_bad[0]     = min(first_bad[0], min{ r*N + n : (uint8) X[r*ldx + n] >= S }) (int64 [1]; caller initialises it to INT64_MAX;
 *                    may be NULL)
 * The WHOLE byte is compared (0xFF, S..31 and the aliasing bytes 32..254 are all "other"); bytes of columns n >= N (row padding) are
 * never counted, whatever they hold.  1 <= S <= 127, 0 <= N <= 65535, ldx >= max(N, 1), any alignment of X and ldx (the 16-byte
 * loads need X and ldx to be multiples of 16; every other call takes the byte path).  R == 0 or N == 0: nothing is touched.
 * All sums are integers: the result does not depend on the grid or on the order of the adds.
 * EPG_ERR_INVALID_ARG: R < 0, N < 0, S < 1, ldx < max(N, 1), census NULL, X NULL with R > 0 and N > 0.  EPG_ERR_UNSUPPORTED: S > 127,
 * N > 65535.  Order of the checks: the shape first, then the unsupported sizes, then the pointers. */
int epg_state_census(const int8_t* X, int64_t R, int32_t N, int64_t ldx, int32_t S, int64_t* census, int64_t* other,
                     int64_t* first_bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_CENSUS_H */
