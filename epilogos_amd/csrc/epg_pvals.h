/*
 * epg_pvals.h -- C ABI of the p-value stage of paired mode with -n on the device (csrc/epg_pvals.hip), part of libepilogos_hip.so:
 * the two-sided p-value of every distance under the fitted generalised normal distribution, and the Benjamini-Hochberg adjustment
 * of the p-values.  On the host these are roiAndVisualPairwise.calculatePVals (scipy.stats.gennorm.cdf over every bin) and
 * roiAndVisualPairwise.benjaminiHochberg (an argsort of every p-value); epilogos --pvals gpu runs them here, in float64.
 *
 * PACKAGE-INTERNAL.  This header lives next to the kernels and not under include/: the binding tests pin the ten public headers
 * and their names (tests/test_abi_symbols.py), and every public prototype that ends in a stream has its capture case in the
 * tables of tests/test_hip_abi_contract.py / tests/test_hip_abi_streams.py.  The entry points are exported extern "C" with the
 * prefix epgf_, bound by the table _abi.INTERNAL["pvals"], held against this header by tests/test_pvals_host.py, and their stream
 * and arena cases live in tests/test_hip_pvals_streams.py.  A later change that may edit tests/test_abi_symbols.py should promote
 * this header to include/epilogos_pvals.h and its table to build.PUBLIC_HEADERS / _abi.HEADERS; nothing else has to move.
 *
 * Conventions are those of include/epilogos_gennorm.h: plain pointers and sizes (no floating-point value is passed by value),
 * caller-owned buffers, the stream last, every argument validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code
 * with the message in epg_last_error().  The library retains nothing, enqueues only on `stream` and waits for nothing; the
 * workspace is the caller's.  No floating-point atomics: the flag words are integer counts (integer adds commute), everything
 * else is written by exactly one thread, so two identical calls give identical bits.  EPG_ABI_VERSION is not changed.
 */
#ifndef EPG_PVALS_H
#define EPG_PVALS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* p[i] = the two-sided p-value of x[i] under gennorm(beta, loc, scale), params = (beta, loc, scale) float64 [3] in DEVICE memory
 * (a row of epgf_gennorm_fit's output: a fit on the device feeds this call without a read-back).  The arithmetic is that of
 * calculatePVals with scipy 1.15's gennorm._cdf, in this order:
 *     z   = ((double)x[i] - loc) / scale
 *     Q   = gammaincc(1 / beta, |z| ** beta)
 *     c   = 0.5 * sign(z)                       (sign(0) = 0)
 *     cdf = (0.5 + c) - c * Q
 *     p   = 2 * cdf  where (double)x[i] <= loc,  else 2 * (1 - cdf)
 * so that above loc p lies on the grid of 1 - (1 - Q / 2), as the host's does: p == 1 at x == loc, p == 0 at both infinities.
 * gammaincc(a, t), the regularised upper incomplete gamma function: 1 at t == 0, 0 at t == inf; for t < a + 1 it is 1 - P with P
 * from the series sum_n t^n / (a (a+1) .. (a+n)); otherwise the continued fraction of Q by the modified Lentz recurrence; both
 * times the prefactor exp(-t + a * log(t) - lgamma(a)), which is 0 where its exponent is below -709.782712893384 (scipy's underflow
 * cut).  An iteration stops when its term changes the sum by less than 2^-52 of it, or at the CAP of 2000 terms.  The kernel is
 * compiled without fused multiply-add contraction; tests/pvals_ref.py restates it in numpy, operation for operation, and records
 * how far that is from scipy.
 *     flags[0] = number of i whose p is NaN: x[i] is NaN, or the parameters are unusable (beta <= 0, scale <= 0 or a NaN in
 *                them: then every p is NaN and flags[0] == M)
 *     flags[1] = number of i on which an iteration stopped at the cap (p[i] is what the iteration had reached)
 * int32 [2]; the call sets them, it does not add to what they held.  No workspace.
 * Limits: 1 <= M < 2^31.  x, params, p and flags are device memory and need only their type's alignment; x and params are only
 * read.
 * EPG_ERR_INVALID_ARG: M < 1; x, params, p or flags NULL.  EPG_ERR_UNSUPPORTED: M >= 2^31.  Order of the checks: the shape (M),
 * then the unsupported size, then the pointers in the order x, params, p, flags; a call with several offences reports the first. */
int epgf_gennorm_pvals(const float* x, int64_t M, const double* params, double* p, int32_t* flags, void* stream);

/* Bytes of workspace of epgf_bh_adjust(p, M, ...): the sorted p-values and their positions, a running minimum per tile of 2048
 * and the radix sort's own storage.  A multiple of 256.  -1 (and a message) when M < 1 or M >= 2^31. */
int64_t epgf_bh_ws_bytes(int64_t M);

/* adj = the Benjamini-Hochberg adjusted p-values of p, float64 [M] each, BIT FOR BIT what benjaminiHochberg (statsmodels' fdr_bh)
 * returns: an ascending sort of p with positions; raw[k] = p_sorted[k] / ((double)(k + 1) / (double)M), two correctly rounded
 * divisions; the running minimum of raw from the right; values above 1 become 1; every value goes back to its position.  A p >= +0.0
 * sorts as its bit pattern read as an unsigned integer (one radix sort of 64-bit keys); the order among equal p does not matter --
 * the minimum from the right gives every member of a run of ties the value of its last member -- and is not numpy's.
 *     flags[0] = number of p that are NaN or have the sign bit set (negative values, -0.0 included).  When it is not 0, adj is
 *                unspecified (but every adj[i] is written and nothing else is).
 * int32 [1], set by the call.
 * Limits: 1 <= M < 2^31.  p, adj, flags and ws are device memory; p and adj need a double's alignment; ws is 256-byte aligned,
 * ws_bytes of it, at least epgf_bh_ws_bytes(M), its contents are scratch.  p is only read; p and adj must not overlap.
 * EPG_ERR_INVALID_ARG: M < 1; p, adj, flags or ws NULL; ws not 256-byte aligned.  EPG_ERR_UNSUPPORTED: M >= 2^31.
 * EPG_ERR_WORKSPACE: ws_bytes below epgf_bh_ws_bytes(M).  Order of the checks: the shape (M), then the unsupported size, then the
 * pointers in the order p, adj, flags, ws, then the alignment of ws, then its size. */
int epgf_bh_adjust(const double* p, int64_t M, double* adj, int32_t* flags, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPG_PVALS_H */
