/*
 * epilogos_concordance.h -- C ABI of the biosample concordance (csrc/epg_concordance.hip), part of libepilogos_hip.so.
 *
 * The census of epilogos_census.h says what ONE biosample column holds.  This entry point is about PAIRS of columns: in how many
 * bins two biosamples are in the same state, and in how many both are in a state at all.  It answers "which two columns are the
 * same file", "which biosample sits with the wrong tissue" and "which biosamples belong together in a group" without the
 * [N, N, S, S] co-occurrence counts of epg_hist_s3, whose trace over the state pairs is the same numbers at S times the work.
 *
 * Conventions are those of epilogos_amd.h: plain pointers and sizes, caller-owned buffers, the stream last, every argument
 * validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in epg_last_error().  The library
 * retains nothing; the workspace is the caller's.  EPG_ABI_VERSION of epilogos_amd.h is not changed by this header.
 */
#ifndef EPILOGOS_CONCORDANCE_H
#define EPILOGOS_CONCORDANCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace epg_concordance wants for a call of R bins, N columns and S states; never more than R * N + 2^20 (a call
 * whose bit planes do not fit walks the bins in chunks), never less than 256.  -1 on a shape epg_concordance refuses (R < 0,
 * N < 1 or > 65535, S < 1 or > 127). */
int64_t epg_concordance_ws_bytes(int64_t R, int32_t N, int32_t S);

/* agree[i*N + j] += #{ b < R : X[b*ldx + i] == X[b*ldx + j] and that byte is a state }      (int64 [N, N], ACCUMULATES)
 * both[i*N + j]  += #{ b < R : X[b*ldx + i] and X[b*ldx + j] are both states }              (int64 [N, N], ACCUMULATES; may be NULL)
 * A byte is a state iff, as a whole unsigned byte, it is in 0 .. S-1 (the rule of epg_state_census: 0xFF, S..31 and 32..254 are
 * all "no state").  Only the first N bytes of a row are read as states; the padding may hold anything.  Both triangles and the
 * diagonal are written: agree[i, i] == both[i, i] == the bins in which column i holds a state.  Zero the outputs once and call
 * per matrix.  All sums are integers and exact for any R; the result does not depend on the grid.
 * 1 <= S <= 127, 1 <= N <= 65535, ldx >= N, any alignment of X and ldx.  ws: device memory, 256-byte aligned, ws_bytes of it, at
 * least epg_concordance_ws_bytes(R, N, S); its contents are scratch.  R == 0 does nothing and looks at no pointer.
 * EPG_ERR_INVALID_ARG: R < 0, N < 1, S < 1, ldx < N; X, agree or ws NULL; ws not 256-byte aligned.  EPG_ERR_UNSUPPORTED: S > 127,
 * N > 65535.  EPG_ERR_WORKSPACE: ws_bytes below epg_concordance_ws_bytes(R, N, S).  Order of the checks: the shape (R, N, S, ldx)
 * first, then the two unsupported sizes, then R == 0 (EPG_OK), then the pointers, then the size of the workspace; a call with
 * several offences reports the first. */
int epg_concordance(const int8_t* X, int64_t R, int32_t N, int64_t ldx, int32_t S, int64_t* agree, int64_t* both, void* ws,
                    int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_CONCORDANCE_H */
