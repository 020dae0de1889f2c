// The p-value stage of paired mode with -n on the device (epg_pvals.h): two-sided gennorm p-values and their Benjamini-Hochberg
// adjustment.  gfx950 only.  All arithmetic is float64, and NOTHING here is contracted into a fused multiply-add: the p-values are
// held against a numpy restatement of the same operations (tests/pvals_ref.py), the adjusted values against numpy bit for bit.
//
//   * k_gennorm_pvals: a lane per distance.  lgamma(1 / beta) once per thread (the parameters are wave-uniform), then per value one
//     pow, one log, one exp and the series or the continued fraction (a few dozen divisions; lanes of a wave run as long as their
//     slowest value).  NaN results and capped iterations are counted per thread, added over the wave by shuffles, and lane 0 does
//     one INTEGER atomic add per non-zero count.
//   * epgf_bh_adjust: rocprim's radix sort of (bit pattern of p, position) pairs, the positions from a counting iterator; then
//     three small kernels over tiles of BH_TILE sorted values.  raw[k] is recomputed where it is needed instead of stored:
//       k_bh_tile_min   the minimum of raw over each tile;
//       k_bh_carry      ONE workgroup turns the tile minima, in place, into "minimum of all tiles to the right" (a chunk of tiles
//                       per thread, the chunks combined through LDS), and counts the refused p from the sorted keys: NaN and
//                       values with the sign bit sort behind +inf, so their number is M minus a lower bound;
//       k_bh_scatter    the running minimum from the right inside each tile (per thread, per wave by shuffles, the waves through
//                       LDS), min with the tile's carry, the clamp at 1 and the store to the value's original position.
//     min is exact and associative: the shape of the scan cannot change a bit.
#include "epg_common.h"
#include "epg_pvals.h"

#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#pragma clang fp contract(off)

namespace epg {

constexpr int PV_ITMAX = 2000;                          // the cap of both iterations
constexpr double PV_EPS = 2.220446049250313e-16;        // 2^-52
constexpr double PV_FPMIN = 2.2250738585072014e-308 / PV_EPS;
constexpr double PV_MAXLOG = 7.09782712893383996843e2;  // scipy's underflow cut of the prefactor

constexpr int BH_THREADS = 256;
constexpr int BH_PER = 8;                               // consecutive sorted values per thread
constexpr int BH_TILE = BH_THREADS * BH_PER;
constexpr int BH_CARRY_THREADS = 1024;
constexpr u64 BH_ABOVE_INF = 0x7FF0000000000001ull;     // the first key that is not a p >= +0.0: NaN, then everything with the sign bit

__device__ __forceinline__ double pv_prefactor(double a, double gln, double t) {
    const double arg = -t + a * log(t) - gln;
    return arg < -PV_MAXLOG ? 0.0 : exp(arg);
}

// Q(a, t) for a > 0 or a == 0 (beta = inf) and t >= 0 or NaN; capped: set when an iteration ran PV_ITMAX terms
__device__ double pv_gammaincc(double a, double gln, double t, bool& capped) {
    if (t != t) return t;
    if (a == 0.0) return t > 0.0 ? 0.0 : __builtin_nan("");
    if (t == 0.0) return 1.0;
    if (t == __builtin_inf()) return 0.0;
    if (t < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        bool live = true;
        for (int n = 0; n < PV_ITMAX && live; ++n) {
            ap = ap + 1.0;
            del = del * (t / ap);
            sum = sum + del;
            live = !(fabs(del) < fabs(sum) * PV_EPS);
        }
        capped = live;
        return 1.0 - sum * pv_prefactor(a, gln, t);
    }
    double b = t + 1.0 - a, c = 1.0 / PV_FPMIN, d = 1.0 / b, h = d;
    bool live = true;
    for (int i = 1; i <= PV_ITMAX && live; ++i) {
        const double an = -(double)i * ((double)i - a);
        b = b + 2.0;
        d = an * d + b;
        if (fabs(d) < PV_FPMIN) d = PV_FPMIN;
        c = b + an / c;
        if (fabs(c) < PV_FPMIN) c = PV_FPMIN;
        d = 1.0 / d;
        const double del = d * c;
        h = h * del;
        live = !(fabs(del - 1.0) <= PV_EPS);
    }
    capped = live;
    return pv_prefactor(a, gln, t) * h;
}

__device__ __forceinline__ int pv_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_gennorm_pvals(const float* __restrict__ x, long M, const double* __restrict__ params,
                                                       double* __restrict__ p, int* __restrict__ flags) {
    const double beta = params[0], loc = params[1], scale = params[2];
    const bool valid = beta > 0.0 && scale > 0.0 && loc == loc;
    const double a = valid ? 1.0 / beta : 1.0;
    const double gln = valid && a > 0.0 ? lgamma(a) : 0.0;
    int n_nan = 0, n_cap = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long)gridDim.x * 256) {
        const double xd = (double)x[i];
        double pv = __builtin_nan("");
        if (valid) {
            const double z = (xd - loc) / scale;
            bool capped = false;
            const double q = pv_gammaincc(a, gln, pow(fabs(z), beta), capped);
            const double c = z > 0.0 ? 0.5 : (z < 0.0 ? -0.5 : (z == 0.0 ? 0.0 : z));     // 0.5 * sign(z); NaN stays NaN
            const double cdf = (0.5 + c) - c * q;
            pv = xd <= loc ? 2.0 * cdf : 2.0 * (1.0 - cdf);
            n_cap += capped ? 1 : 0;
        }
        n_nan += pv != pv ? 1 : 0;
        p[i] = pv;
    }
    n_nan = pv_wave_sum(n_nan);
    n_cap = pv_wave_sum(n_cap);
    if ((threadIdx.x & 63) == 0) {
        if (n_nan) atomicAdd(flags, n_nan);
        if (n_cap) atomicAdd(flags + 1, n_cap);
    }
}

// ---- Benjamini-Hochberg ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double bh_min(double a, double b) { return b < a ? b : a; }

// raw[k] of the sorted keys, +inf behind the end
__device__ __forceinline__ double bh_raw(const u64* __restrict__ keys, long k, long M, double dM) {
    return k < M ? __longlong_as_double((long long)keys[k]) / ((double)(k + 1) / dM) : __builtin_inf();
}

__global__ __launch_bounds__(BH_THREADS) void k_bh_tile_min(const u64* __restrict__ keys, long M, double* __restrict__ tmin) {
    __shared__ double s_w[BH_THREADS / 64];
    const int tid = threadIdx.x;
    const long k0 = (long)blockIdx.x * BH_TILE + (long)tid * BH_PER;
    const double dM = (double)M;
    double m = __builtin_inf();
#pragma unroll
    for (int j = 0; j < BH_PER; ++j) m = bh_min(m, bh_raw(keys, k0 + j, M, dM));
#pragma unroll
    for (int o = 32; o; o >>= 1) m = bh_min(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) s_w[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < BH_THREADS / 64; ++w) m = bh_min(m, s_w[w]);
        tmin[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(BH_CARRY_THREADS) void k_bh_carry(const u64* __restrict__ keys, long M, double* __restrict__ tmin, long ntiles,
                                                               int* __restrict__ flags) {
    __shared__ double s_m[BH_CARRY_THREADS];
    const int tid = threadIdx.x;
    const long chunk = (ntiles + BH_CARRY_THREADS - 1) / BH_CARRY_THREADS;
    const long lo = tid * chunk < ntiles ? tid * chunk : ntiles, hi = lo + chunk < ntiles ? lo + chunk : ntiles;
    double m = __builtin_inf();
    for (long b = lo; b < hi; ++b) m = bh_min(m, tmin[b]);
    s_m[tid] = m;
    __syncthreads();
    double run = __builtin_inf();                                   // the minimum of every tile right of this thread's chunk
    for (int t = tid + 1; t < BH_CARRY_THREADS; ++t) run = bh_min(run, s_m[t]);
    for (long b = hi - 1; b >= lo; --b) {
        const double own = tmin[b];
        tmin[b] = run;
        run = bh_min(run, own);
    }
    if (tid == 0) {                                                 // first sorted key that is no p >= +0.0
        long l = 0, h = M;
        while (l < h) {
            const long mid = l + ((h - l) >> 1);
            if (keys[mid] < BH_ABOVE_INF) l = mid + 1;
            else h = mid;
        }
        flags[0] = (int)(M - l);
    }
}

__global__ __launch_bounds__(BH_THREADS) void k_bh_scatter(const u64* __restrict__ keys, const u32* __restrict__ pos, long M,
                                                           const double* __restrict__ carry, double* __restrict__ adj) {
    __shared__ double s_w[BH_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long k0 = (long)blockIdx.x * BH_TILE + (long)tid * BH_PER;
    const double dM = (double)M;
    double v[BH_PER];
#pragma unroll
    for (int j = 0; j < BH_PER; ++j) v[j] = bh_raw(keys, k0 + j, M, dM);
#pragma unroll
    for (int j = BH_PER - 2; j >= 0; --j) v[j] = bh_min(v[j], v[j + 1]);
    double s = v[0];                                                // inclusive minimum from the right over the wave's threads
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_down(s, o);
        if (lane + o < 64) s = bh_min(s, y);
    }
    if (lane == 0) s_w[wave] = s;
    double right = __shfl_down(s, 1);                               // of the threads right of this one
    if (lane == 63) right = __builtin_inf();
    __syncthreads();
#pragma unroll
    for (int w = 1; w < BH_THREADS / 64; ++w)
        if (w > wave) right = bh_min(right, s_w[w]);
    right = bh_min(right, carry[blockIdx.x]);
#pragma unroll
    for (int j = 0; j < BH_PER; ++j) {
        if (k0 + j < M) {
            double r = bh_min(v[j], right);
            if (r > 1.0) r = 1.0;
            adj[pos[k0 + j]] = r;
        }
    }
}

struct BhLayout {
    int64_t keys, pos, tmin, temp, total, ntiles;
};

static int bh_layout(int64_t M, BhLayout& L) {
    L.ntiles = (M + BH_TILE - 1) / BH_TILE;
    L.keys = 0;
    L.pos = align_up(M * 8, 256);
    L.tmin = L.pos + align_up(M * 4, 256);
    L.temp = L.tmin + align_up(L.ntiles * 8, 256);
    size_t tb = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const u64*)nullptr, (u64*)nullptr, rocprim::counting_iterator<u32>(0), (u32*)nullptr,
                                             (size_t)M, 0, 64, (hipStream_t)0);
    if (e != hipSuccess) return fail(EPG_ERR_HIP, "bh_adjust: radix sort size query failed: %s", hipGetErrorString(e));
    L.total = align_up(L.temp + (int64_t)tb, 256);
    return EPG_OK;
}

extern "C" int epgf_gennorm_pvals(const float* x, int64_t M, const double* params, double* p, int32_t* flags, void* stream) {
    if (M < 1) return fail(EPG_ERR_INVALID_ARG, "gennorm_pvals: bad shape M=%lld", (long long)M);
    if (M >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "gennorm_pvals: M=%lld >= 2^31", (long long)M);
    if (!x) return fail(EPG_ERR_INVALID_ARG, "gennorm_pvals: x is NULL");
    if (!params) return fail(EPG_ERR_INVALID_ARG, "gennorm_pvals: params is NULL");
    if (!p) return fail(EPG_ERR_INVALID_ARG, "gennorm_pvals: p is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "gennorm_pvals: flags is NULL");
    hipStream_t st = (hipStream_t)stream;
    EPG_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), st));
    long blocks = (M + 255) / 256;
    if (blocks > num_cus() * 32L) blocks = num_cus() * 32L;
    hipLaunchKernelGGL(k_gennorm_pvals, dim3((unsigned)blocks), dim3(256), 0, st, x, (long)M, params, p, flags);
    EPG_LAUNCH_CHECK("k_gennorm_pvals");
    return EPG_OK;
}

extern "C" int64_t epgf_bh_ws_bytes(int64_t M) {
    if (M < 1 || M >= (1LL << 31)) {
        fail(EPG_ERR_INVALID_ARG, "bh_ws_bytes: bad shape M=%lld", (long long)M);
        return -1;
    }
    BhLayout L;
    return bh_layout(M, L) ? -1 : L.total;
}

extern "C" int epgf_bh_adjust(const double* p, int64_t M, double* adj, int32_t* flags, void* ws, int64_t ws_bytes, void* stream) {
    if (M < 1) return fail(EPG_ERR_INVALID_ARG, "bh_adjust: bad shape M=%lld", (long long)M);
    if (M >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "bh_adjust: M=%lld >= 2^31", (long long)M);
    if (!p) return fail(EPG_ERR_INVALID_ARG, "bh_adjust: p is NULL");
    if (!adj) return fail(EPG_ERR_INVALID_ARG, "bh_adjust: adj is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "bh_adjust: flags is NULL");
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "bh_adjust: ws is NULL");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "bh_adjust: ws is not 256-byte aligned");
    BhLayout L;
    const int rc = bh_layout(M, L);
    if (rc) return rc;
    if (ws_bytes < L.total) return fail(EPG_ERR_WORKSPACE, "bh_adjust: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    u64* keys = reinterpret_cast<u64*>(base + L.keys);
    u32* pos = reinterpret_cast<u32*>(base + L.pos);
    double* tmin = reinterpret_cast<double*>(base + L.tmin);
    size_t tb = (size_t)(L.total - L.temp);
    hipError_t e = rocprim::radix_sort_pairs(base + L.temp, tb, reinterpret_cast<const u64*>(p), keys, rocprim::counting_iterator<u32>(0), pos,
                                             (size_t)M, 0, 64, st);
    if (e != hipSuccess) return fail(EPG_ERR_HIP, "bh_adjust: radix sort failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_bh_tile_min, dim3((unsigned)L.ntiles), dim3(BH_THREADS), 0, st, keys, (long)M, tmin);
    EPG_LAUNCH_CHECK("k_bh_tile_min");
    hipLaunchKernelGGL(k_bh_carry, dim3(1), dim3(BH_CARRY_THREADS), 0, st, keys, (long)M, tmin, (long)L.ntiles, flags);
    EPG_LAUNCH_CHECK("k_bh_carry");
    hipLaunchKernelGGL(k_bh_scatter, dim3((unsigned)L.ntiles), dim3(BH_THREADS), 0, st, keys, pos, (long)M, tmin, adj);
    EPG_LAUNCH_CHECK("k_bh_scatter");
    return EPG_OK;
}

}  // namespace epg
