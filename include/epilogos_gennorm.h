/*
 * epilogos_gennorm.h -- C ABI of the device fit of the paired null distribution (csrc/epg_gennorm.hip), part of libepilogos_hip.so.
 *
 * Paired mode with -n fits a generalised normal distribution to the null distances: numTrials maximum-likelihood fits on
 * sub-samples, the negative log-likelihood of ALL null distances under every trial's parameters, the trial with the median one
 * wins.  On the host that is scipy.stats.gennorm.fit (Nelder-Mead, a few hundred evaluations of a sum of |z|**beta over the
 * sub-sample) and scipy.stats.gennorm.nnlf per trial.  These entry points do both on the device, in float64.
 *
 * Conventions are those of epilogos_amd.h and epilogos_concordance.h: plain pointers and sizes, caller-owned buffers, the stream
 * last, every argument validated before the first HIP call, EPG_OK or a negative EPG_ERR_* code with the message in
 * epg_last_error().  The library retains nothing, enqueues only on `stream` and waits for nothing; the workspace is the caller's.
 * EPG_ABI_VERSION of epilogos_amd.h is not changed by this header.
 * The prefix is epgf_ ("fit"), as the text parser has epgt_ and the host library epgio_, because every epg_ / epgt_ prototype that
 * ends in a stream must have its capture case in the table of tests/test_hip_abi_streams.py, and these entry points' cases -- the
 * same capture procedure -- live in a file of their own, tests/test_hip_gennorm_streams.py; a change that edits that table can
 * fold them in.
 *
 * The objective, for a sample v[0..n), in float64 throughout (float inputs are widened, pow / log / lgamma of the device library):
 *     f(beta, loc, scale) = n * (log scale - log(beta / 2) + lgamma(1 / beta)) + sum_i |(v[i] - loc) / scale| ** beta
 * and +inf when beta <= 0 or scale <= 0 or a parameter is NaN or the sum is not a number.  That is scipy's penalised nnlf of
 * gennorm for finite terms.  Every sum is taken in a FIXED order (per-lane partial sums, a wave reduction, the waves in order; for
 * epgf_gennorm_nnlf chunks of 1024 values added in chunk order) and without floating-point atomics: the result of a trial does
 * not depend on T, on the other trials or on the grid, and two identical calls give identical bits.
 */
#ifndef EPILOGOS_GENNORM_H
#define EPILOGOS_GENNORM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace that serve BOTH epgf_gennorm_fit(x, M, idx, T, n, ...) and epgf_gennorm_nnlf(x, M, params, T, ...): the
 * larger of T copies of a sub-sample (n floats, rounded up to 256 bytes) and T partial sums per 1024 values of x.  n == 0 sizes
 * it for epgf_gennorm_nnlf alone.  A multiple of 256, never less than 256.  -1 on a shape the entry points refuse (M < 1 or
 * >= 2^31, T < 1, n not 0 and not in 2 .. M). */
int64_t epgf_gennorm_ws_bytes(int64_t M, int32_t T, int64_t n);

/* T maximum-likelihood fits of a generalised normal distribution.  Trial t fits the n values x[idx[t*n + i]], i < n; idx == NULL
 * means every trial fits x[0 .. n) and needs n == M.  One workgroup per trial; the sub-sample is gathered once into the workspace
 * and every evaluation streams it from there.
 *     params[t*3 ..] = (beta, loc, scale)   float64 [T, 3]
 *     fval[t]        = f at them             float64 [T]
 *     info[t*2 ..]   = (evaluations of f, flag)   int32 [T, 2]
 * flag 0: converged; 1: stopped at the cap of 600 evaluations or 600 iterations (the best vertex is returned, as scipy does);
 * 2: a degenerate sample -- its variance is 0 or a value is not finite --: params and fval are NaN, evaluations 0.
 * The algorithm restates scipy.stats.gennorm.fit (scipy 1.15: rv_continuous.fit, neither fit nor _fitstart overridden), so that
 * it ends in scipy's local optimum where the likelihood has many (beta < 1: a cusp at every data point):
 *   start (1, mean, sqrt(var / 2)), mean and population variance in float64 (scipy takes them in the data's float32);
 *   optimize.fmin's Nelder-Mead with its defaults: the initial simplex is the start and the start with one coordinate times 1.05
 *   (0.00025 where it is 0); reflection 1, expansion 2, contraction 0.5, shrink 0.5; vertices ordered by a stable sort; it stops
 *   when max |sim[1:] - sim[0]| <= 1e-4 and max |fsim[0] - fsim[1:]| <= 1e-4, or at maxiter = maxfun = 600.
 * Limits: 1 <= T, 2 <= n <= M < 2^31.  x, idx, params, fval, info and ws are device memory; x and idx need only their type's
 * alignment; ws is 256-byte aligned, ws_bytes of it, at least epgf_gennorm_ws_bytes(M, T, n), its contents are scratch.  x and idx
 * are only read.  An index outside 0 .. M-1 is the CALLER'S error: it is not checked here and reads outside x (the Python wrapper
 * engine.gennorm_fit checks it).
 * EPG_ERR_INVALID_ARG: T < 1, n < 2, M < n; idx NULL with n != M; x, params, fval, info or ws NULL; ws not 256-byte aligned.
 * EPG_ERR_UNSUPPORTED: M >= 2^31.  EPG_ERR_WORKSPACE: ws_bytes below epgf_gennorm_ws_bytes(M, T, n).  Order of the checks: the
 * shape (T, n, M) first, then the unsupported size, then idx NULL with n != M, then the pointers in the order x, params, fval,
 * info, ws, then the alignment of ws, then its size; a call with several offences reports the first. */
int epgf_gennorm_fit(const float* x, int64_t M, const int32_t* idx, int32_t T, int64_t n, double* params, double* fval, int32_t* info,
                     void* ws, int64_t ws_bytes, void* stream);

/* nnlf[t] = f(params[t*3 ..]) over ALL M values of x, for all T parameter sets in one pass over x: every value is read once.
 * Partial sums of chunks of 1024 values go to the workspace and a second kernel adds them in chunk order; the chunking depends on
 * M only.  A parameter set with beta <= 0, scale <= 0 or a NaN gives +inf.  float64 [T] out, params float64 [T, 3] in.
 * Limits: 1 <= T, 1 <= M < 2^31; ws as above, at least epgf_gennorm_ws_bytes(M, T, 0).
 * EPG_ERR_INVALID_ARG: T < 1, M < 1; x, params, nnlf or ws NULL; ws not 256-byte aligned.  EPG_ERR_UNSUPPORTED: M >= 2^31.
 * EPG_ERR_WORKSPACE: ws_bytes below epgf_gennorm_ws_bytes(M, T, 0).  Order of the checks: the shape (T, M), then the unsupported
 * size, then the pointers in the order x, params, nnlf, ws, then the alignment of ws, then its size. */
int epgf_gennorm_nnlf(const float* x, int64_t M, const double* params, int32_t T, double* nnlf, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EPILOGOS_GENNORM_H */
