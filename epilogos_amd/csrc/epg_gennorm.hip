// The null fit of paired mode on the device: T generalised-normal maximum-likelihood fits on sub-samples of the null distances and the
// negative log-likelihood of all of them under every fit (include/epilogos_gennorm.h).  gfx950 only.  All arithmetic is float64.
//
//   * k_gennorm_fit: ONE WORKGROUP PER TRIAL, the whole Nelder-Mead loop inside the kernel.  The sub-sample is gathered once into the
//     trial's slice of the workspace; a thread gathers exactly the 16-byte groups it later streams, so an evaluation is a loop of
//     dwordx4 loads of the thread's own stores.  An evaluation: per-lane partial sums over the thread's groups in group order, a
//     butterfly over the wave (every lane ends with the same bits), the waves' sums added in wave order from LDS by every thread.
//     Every thread therefore holds the same objective value and runs the three-number simplex logic redundantly: no broadcast, the
//     branches are uniform.  The vertices live in registers (the sort is an unrolled stable bubble sort of four).
//   * k_gennorm_nnlf_partial: a workgroup takes chunks of GN_CHUNK values of x, four per thread, read once; for every parameter set
//     the thread's four terms, a wave butterfly, the wave sums to LDS; after a tile of GN_TT sets one barrier and thread t adds the
//     four wave sums of set t in wave order into partial[chunk][t].
//   * k_gennorm_nnlf_finish: thread t adds partial[0 .. nchunks)[t] in chunk order and the n * (log scale - log(beta/2) + lgamma(1/beta)).
// No floating-point atomics anywhere: the bits depend on (x, idx, n) and M only, not on T, the grid or the other trials.
#include "epg_common.h"
#include "epilogos_gennorm.h"

#include <math.h>

namespace epg {

constexpr int GN_THREADS = 1024;           // the fit's workgroup: 16 waves stream one sub-sample
constexpr int GN_WAVES = GN_THREADS / 64;
constexpr int GN_MAXFUN = 600;             // fmin's maxfun and maxiter for three parameters
constexpr int GN_CHUNK = 1024;             // values of x per partial sum of the nnlf pass: 256 threads x 4
constexpr int GN_TT = 256;                 // parameter sets per LDS tile of the nnlf pass

static inline int64_t gn_stride(int64_t n) { return align_up(n, 64); }                 // floats of a trial's slice: whole 256 bytes
static inline int64_t gn_chunks(int64_t M) { return (M + GN_CHUNK - 1) / GN_CHUNK; }

static int64_t gn_ws_bytes(int64_t M, int32_t T, int64_t n) {
    const __int128 fit = n ? (__int128)T * gn_stride(n) * 4 : 0;
    const __int128 nn = ((__int128)gn_chunks(M) * T * 8 + 255) / 256 * 256;
    const __int128 need = fit > nn ? fit : nn;
    return need > INT64_MAX ? INT64_MAX / 256 * 256 : (need < 256 ? 256 : (int64_t)need);
}

__device__ __forceinline__ double gn_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double gn_term(float v, double beta, double mu, double sigma) { return pow(fabs(((double)v - mu) / sigma), beta); }

// sum over the workgroup of g(v) for the n values of xs, the same bits in every thread; s_red: GN_WAVES doubles
template <typename G>
__device__ __forceinline__ double gn_block_sum(const float* __restrict__ xs, long n, double* s_red, G g) {
    const int tid = threadIdx.x;
    const long n4 = n >> 2;
    double acc = 0.0;
    for (long q = tid; q < n4; q += GN_THREADS) {
        const float4 v = *reinterpret_cast<const float4*>(xs + 4 * q);
        acc += g(v.x);
        acc += g(v.y);
        acc += g(v.z);
        acc += g(v.w);
    }
    if (tid < (int)(n & 3)) acc += g(xs[4 * n4 + tid]);
    acc = gn_wave_sum(acc);
    if ((tid & 63) == 0) s_red[tid >> 6] = acc;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < GN_WAVES; ++w) s += s_red[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ double gn_const(double n, double beta, double sigma) { return n * (log(sigma) - log(0.5 * beta) + lgamma(1.0 / beta)); }

// the objective, ONE copy of the pow loop for the dozen places of the simplex step that evaluate (inlined there, the kernel
// spilled 385 registers); the call is once per evaluation, the loop inside is what runs
__device__ __noinline__ double gn_objective(const float* __restrict__ xs, long n, double beta, double mu, double sigma, double* s_red) {
    const double s = gn_block_sum(xs, n, s_red, [=](float v) { return gn_term(v, beta, mu, sigma); });
    const double f = gn_const((double)n, beta, sigma) + s;
    return f == f ? f : __builtin_inf();
}

struct GnVertex {
    double b, m, s, f;
};

__device__ __forceinline__ void gn_order(GnVertex& a, GnVertex& b) {                    // stable: equal values keep their order
    if (a.f > b.f) {
        const GnVertex t = a;
        a = b;
        b = t;
    }
}

__device__ __forceinline__ void gn_sort(GnVertex (&v)[4]) {
    gn_order(v[0], v[1]); gn_order(v[1], v[2]); gn_order(v[2], v[3]);
    gn_order(v[0], v[1]); gn_order(v[1], v[2]);
    gn_order(v[0], v[1]);
}

__global__ __launch_bounds__(GN_THREADS) void k_gennorm_fit(const float* __restrict__ x, const int* __restrict__ idx, long n, long stride,
                                                            float* __restrict__ ws, double* __restrict__ params, double* __restrict__ fval,
                                                            int* __restrict__ info) {
    __shared__ double s_red[GN_WAVES];
    const int tid = threadIdx.x;
    const long t = blockIdx.x;
    float* const xs = ws + t * stride;
    // the gather: a thread fills the groups it will read
    {
        const int* const ix = idx ? idx + t * n : nullptr;
        const long n4 = n >> 2;
        for (long q = tid; q < n4; q += GN_THREADS) {
            float4 v;
            if (ix) {
                v.x = x[ix[4 * q]]; v.y = x[ix[4 * q + 1]]; v.z = x[ix[4 * q + 2]]; v.w = x[ix[4 * q + 3]];
            } else {
                v.x = x[4 * q]; v.y = x[4 * q + 1]; v.z = x[4 * q + 2]; v.w = x[4 * q + 3];
            }
            *reinterpret_cast<float4*>(xs + 4 * q) = v;
        }
        if (tid < (int)(n & 3)) xs[4 * n4 + tid] = ix ? x[ix[4 * n4 + tid]] : x[4 * n4 + tid];
    }
    __syncthreads();
    const double dn = (double)n;
    const double mean = gn_block_sum(xs, n, s_red, [](float v) { return (double)v; }) / dn;
    const double var = gn_block_sum(xs, n, s_red, [mean](float v) { const double d = (double)v - mean; return d * d; }) / dn;
    if (!(var > 0.0) || !(fabs(mean) <= 1.79769313486231570e308) || !(var <= 1.79769313486231570e308)) {
        if (tid == 0) {                                                              // a constant sample, or a value that is not finite
            const double q = __builtin_nan("");
            params[3 * t] = params[3 * t + 1] = params[3 * t + 2] = fval[t] = q;
            info[2 * t] = 0;
            info[2 * t + 1] = 2;
        }
        return;
    }
    int evals = 0;
    // f at p, false (and nothing evaluated) once maxfun evaluations are spent
    auto f_at = [&](GnVertex& p) -> bool {
        if (evals >= GN_MAXFUN) return false;
        ++evals;
        const double beta = p.b, mu = p.m, sigma = p.s;
        if (!(beta > 0.0) || !(sigma > 0.0) || mu != mu) {
            p.f = __builtin_inf();
            return true;
        }
        p.f = gn_objective(xs, n, beta, mu, sigma, s_red);
        return true;
    };
    GnVertex v[4];
    const GnVertex x0 = {1.0, mean, sqrt(var * 0.5), __builtin_inf()};
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x0;
    v[1].b = 1.05 * x0.b;
    v[2].m = x0.m != 0.0 ? 1.05 * x0.m : 0.00025;
    v[3].s = 1.05 * x0.s;
#pragma unroll
    for (int k = 0; k < 4; ++k) f_at(v[k]);
    gn_sort(v);
    int iterations = 1;
    bool converged = false;
    while (evals < GN_MAXFUN && iterations < GN_MAXFUN) {
        bool small = true;
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            if (!(fabs(v[k].b - v[0].b) <= 1e-4) || !(fabs(v[k].m - v[0].m) <= 1e-4) || !(fabs(v[k].s - v[0].s) <= 1e-4)) small = false;
            if (!(fabs(v[0].f - v[k].f) <= 1e-4)) small = false;
        }
        if (small) {
            converged = true;
            break;
        }
        // one step; `done` false: the evaluation cap was met inside it and the step ends where it stands (scipy's _MaxFuncCallError)
        const double cb = ((v[0].b + v[1].b) + v[2].b) / 3.0, cm = ((v[0].m + v[1].m) + v[2].m) / 3.0, cs = ((v[0].s + v[1].s) + v[2].s) / 3.0;
        auto along = [&](double a, double b) { return GnVertex{a * cb + b * v[3].b, a * cm + b * v[3].m, a * cs + b * v[3].s, 0.0}; };
        bool done = false;
        do {
            GnVertex xr = along(2.0, -1.0);
            if (!f_at(xr)) break;
            bool shrink = false;
            if (xr.f < v[0].f) {
                GnVertex xe = along(3.0, -2.0);
                if (!f_at(xe)) break;
                v[3] = xe.f < xr.f ? xe : xr;
            } else if (xr.f < v[2].f) {
                v[3] = xr;
            } else if (xr.f < v[3].f) {
                GnVertex xc = along(1.5, -0.5);
                if (!f_at(xc)) break;
                if (xc.f <= xr.f) v[3] = xc;
                else shrink = true;
            } else {
                GnVertex xcc = along(0.5, 0.5);
                if (!f_at(xcc)) break;
                if (xcc.f < v[3].f) v[3] = xcc;
                else shrink = true;
            }
            if (shrink) {
                bool all = true;
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    if (!all) continue;
                    GnVertex y = {v[0].b + 0.5 * (v[k].b - v[0].b), v[0].m + 0.5 * (v[k].m - v[0].m), v[0].s + 0.5 * (v[k].s - v[0].s), v[k].f};
                    all = f_at(y);                                                   // (at the cap the vertex moves and keeps its old value)
                    v[k] = y;
                }
                if (!all) break;
            }
            done = true;
        } while (false);
        if (done) ++iterations;
        gn_sort(v);
    }
    if (tid == 0) {
        params[3 * t] = v[0].b;
        params[3 * t + 1] = v[0].m;
        params[3 * t + 2] = v[0].s;
        fval[t] = v[0].f;
        info[2 * t] = evals;
        info[2 * t + 1] = converged ? 0 : 1;
    }
}

__device__ __forceinline__ bool gn_valid(double beta, double mu, double sigma) { return beta > 0.0 && sigma > 0.0 && mu == mu; }

__global__ __launch_bounds__(256) void k_gennorm_nnlf_partial(const float* __restrict__ x, long M, const double* __restrict__ params, int T,
                                                              long nchunks, double* __restrict__ partial) {
    __shared__ double s_w[GN_TT][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long i0 = c * GN_CHUNK + 4L * tid;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < M ? x[i0 + j] : 0.0f;           // (any alignment of x; what is behind M adds nothing)
        const int nv = i0 >= M ? 0 : (M - i0 < 4 ? (int)(M - i0) : 4);
        for (int t0 = 0; t0 < T; t0 += GN_TT) {
            const int tt = T - t0 < GN_TT ? T - t0 : GN_TT;
            for (int k = 0; k < tt; ++k) {
                const double beta = params[3L * (t0 + k)], mu = params[3L * (t0 + k) + 1], sigma = params[3L * (t0 + k) + 2];   // wave-uniform
                double acc = 0.0;
                if (gn_valid(beta, mu, sigma)) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nv) acc += gn_term(v[j], beta, mu, sigma);
                    acc = gn_wave_sum(acc);
                }
                if (lane == 0) s_w[k][wave] = acc;
            }
            __syncthreads();
            if (tid < tt) partial[c * T + t0 + tid] = ((s_w[tid][0] + s_w[tid][1]) + s_w[tid][2]) + s_w[tid][3];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void k_gennorm_nnlf_finish(const double* __restrict__ partial, long M, const double* __restrict__ params, int T,
                                                             long nchunks, double* __restrict__ nnlf) {
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= T) return;
    const double beta = params[3 * t], mu = params[3 * t + 1], sigma = params[3 * t + 2];
    if (!gn_valid(beta, mu, sigma)) {
        nnlf[t] = __builtin_inf();
        return;
    }
    double s = 0.0;
    for (long c = 0; c < nchunks; ++c) s += partial[c * T + t];
    const double f = gn_const((double)M, beta, sigma) + s;
    nnlf[t] = f == f ? f : __builtin_inf();
}

static int gn_check_ws(const char* who, void* ws, int64_t ws_bytes, int64_t need) {
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "%s: ws is NULL", who);
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "%s: ws is not 256-byte aligned", who);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)ws_bytes, (long long)need);
    return EPG_OK;
}

extern "C" int64_t epgf_gennorm_ws_bytes(int64_t M, int32_t T, int64_t n) {
    if (M < 1 || M >= (1LL << 31) || T < 1 || (n != 0 && (n < 2 || n > M))) {
        fail(EPG_ERR_INVALID_ARG, "gennorm_ws_bytes: bad shape M=%lld T=%d n=%lld", (long long)M, T, (long long)n);
        return -1;
    }
    return gn_ws_bytes(M, T, n);
}

extern "C" int epgf_gennorm_fit(const float* x, int64_t M, const int32_t* idx, int32_t T, int64_t n, double* params, double* fval, int32_t* info,
                                void* ws, int64_t ws_bytes, void* stream) {
    if (T < 1 || n < 2 || M < n) return fail(EPG_ERR_INVALID_ARG, "gennorm_fit: bad shape T=%d n=%lld M=%lld", T, (long long)n, (long long)M);
    if (M >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "gennorm_fit: M=%lld >= 2^31", (long long)M);
    if (!idx && n != M) return fail(EPG_ERR_INVALID_ARG, "gennorm_fit: idx is NULL and n=%lld is not M=%lld", (long long)n, (long long)M);
    if (!x) return fail(EPG_ERR_INVALID_ARG, "gennorm_fit: x is NULL");
    if (!params) return fail(EPG_ERR_INVALID_ARG, "gennorm_fit: params is NULL");
    if (!fval) return fail(EPG_ERR_INVALID_ARG, "gennorm_fit: fval is NULL");
    if (!info) return fail(EPG_ERR_INVALID_ARG, "gennorm_fit: info is NULL");
    const int rc = gn_check_ws("gennorm_fit", ws, ws_bytes, gn_ws_bytes(M, T, n));
    if (rc != EPG_OK) return rc;
    hipLaunchKernelGGL(k_gennorm_fit, dim3((unsigned)T), dim3(GN_THREADS), 0, (hipStream_t)stream, x, idx, (long)n, (long)gn_stride(n),
                       static_cast<float*>(ws), params, fval, info);
    EPG_LAUNCH_CHECK("k_gennorm_fit");
    return EPG_OK;
}

extern "C" int epgf_gennorm_nnlf(const float* x, int64_t M, const double* params, int32_t T, double* nnlf, void* ws, int64_t ws_bytes, void* stream) {
    if (T < 1 || M < 1) return fail(EPG_ERR_INVALID_ARG, "gennorm_nnlf: bad shape T=%d M=%lld", T, (long long)M);
    if (M >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "gennorm_nnlf: M=%lld >= 2^31", (long long)M);
    if (!x) return fail(EPG_ERR_INVALID_ARG, "gennorm_nnlf: x is NULL");
    if (!params) return fail(EPG_ERR_INVALID_ARG, "gennorm_nnlf: params is NULL");
    if (!nnlf) return fail(EPG_ERR_INVALID_ARG, "gennorm_nnlf: nnlf is NULL");
    const int rc = gn_check_ws("gennorm_nnlf", ws, ws_bytes, gn_ws_bytes(M, T, 0));
    if (rc != EPG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long nchunks = gn_chunks(M);
    long grid = nchunks < (long)num_cus() * 8 ? nchunks : (long)num_cus() * 8;
    double* partial = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_gennorm_nnlf_partial, dim3((unsigned)grid), dim3(256), 0, st, x, (long)M, params, T, nchunks, partial);
    EPG_LAUNCH_CHECK("k_gennorm_nnlf_partial");
    hipLaunchKernelGGL(k_gennorm_nnlf_finish, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, partial, (long)M, params, T, nchunks, nnlf);
    EPG_LAUNCH_CHECK("k_gennorm_nnlf_finish");
    return EPG_OK;
}

}  // namespace epg
