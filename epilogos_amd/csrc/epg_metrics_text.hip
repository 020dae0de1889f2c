// The device metrics writer (epg_metrics_text.h): the rows of pairwiseMetrics_*.txt.gz as text.  gfx950 only.
//
// Three launches on the caller's stream, the arrangement of epgw_format_scores (epg_textout.hip):
//   * k_mt_lengths   a thread per row: the row's fields are read and checked (mt_load: table indices and table entries against their
//                    bounds, the coordinates' sign, the distance against epg_fmt_f5.h, the p-values against epg_fmt_e5.h -- integer
//                    arithmetic only), refused fields OR-ed into the flag word and formatted as nothing or zero; the row's length,
//                    and the tile's sum by the workgroup scan of epg_text_scan.h;
//   * k_text_tile_offsets (epg_text_scan.h)  one workgroup: the exclusive scan of the tiles' sums, the text's size into row_off[R];
//   * k_mt_write     a workgroup per MT_ROWS rows, a thread per row: the rows' offsets into row_off, then the text.  The rows' text is
//                    put together in LDS, a window of MT_WIN bytes of the text at a time (a tile of 256 rows is ~20 KB: one window; a
//                    thread skips the bytes that lie outside the window), and every window goes out in 16-byte stores, aligned in the
//                    text: only the up to 15 bytes at a tile's two ends, which share their 16 bytes with the neighbouring tile, are
//                    stored byte by byte.  LDS: MT_WIN = 32 KB.
// Nothing synchronises.  Every read of a table goes through an index and an offset pair that were checked first; every byte of text
// lies below row_off[R] <= text_cap.
#include "epg_common.h"
#include "epg_metrics_text.h"
#include "epg_text_scan.h"
#include "epg_fmt_f5.h"
#include "epg_fmt_e5.h"

namespace epg {

constexpr int MT_ROWS = 256;
constexpr int MT_WIN = 32768;

struct MtArgs {
    const char* chrom;
    const long long* chrom_off;
    int n_chrom;
    long long chrom_bytes;
    const int* chrom_idx;
    const long long* start;
    const long long* end;
    const char* names;
    const long long* names_off;
    int n_names;
    long long names_bytes;
    const int* maxdiff;
    const float* dist;
    const double* pvals;
    const double* mh;
    long R;
};

// a row's fields, checked and scaled: what both passes need
struct MtRow {
    long long c_at, n_at;                                   // where the two names start in their blobs
    int c_len, n_len;
    u64 start, end;
    int s_dig, e_dig;
    u32 d_bits;                                             // |dist|
    uint64_t d_q;
    int d_len;
    char sign;
    u32 p_q, m_q;
    int p_k, m_k;
    int bad;
    u32 len;
};

__device__ __forceinline__ int mt_digits(u64 v) {
    int n = 1;
    while (v >= 10ull) {
        v /= 10ull;
        ++n;
    }
    return n;
}

// entry i of a table of n names in a blob of `bytes` bytes -> false when i or the entry is out of bounds
__device__ __forceinline__ bool mt_entry(const long long* off, int n, long long bytes, long long i, long long* at, int* len) {
    *at = 0;
    *len = 0;
    if (i < 0 || i >= n) return false;
    const long long o0 = off[i], o1 = off[i + 1];
    if (o0 < 0 || o1 < o0 || o1 > bytes || o1 - o0 > EPGM_NAME_MAX) return false;
    *at = o0;
    *len = (int)(o1 - o0);
    return true;
}

__device__ __forceinline__ void mt_load(const MtArgs& a, long r, MtRow& w) {
    w.bad = 0;
    if (!mt_entry(a.chrom_off, a.n_chrom, a.chrom_bytes, a.chrom_idx[r], &w.c_at, &w.c_len)) w.bad |= EPGM_FLAG_CHROM;
    if (!mt_entry(a.names_off, a.n_names, a.names_bytes, (long long)a.maxdiff[r] - 1, &w.n_at, &w.n_len)) w.bad |= EPGM_FLAG_STATE;
    long long s = a.start[r], e = a.end[r];
    if (s < 0 || e < 0) {
        w.bad |= EPGM_FLAG_COORD;
        s = s < 0 ? 0 : s;
        e = e < 0 ? 0 : e;
    }
    w.start = (u64)s;
    w.end = (u64)e;
    w.s_dig = mt_digits(w.start);
    w.e_dig = mt_digits(w.end);
    const float d = a.dist[r];
    w.d_bits = __float_as_uint(d) & 0x7fffffffu;
    if (!epgfmt::f5_scale(w.d_bits, &w.d_q)) w.bad |= EPGM_FLAG_DIST;
    w.d_len = epgfmt::f5_len(w.d_bits, w.d_q);
    w.sign = d >= 0.0f ? '+' : '-';
    w.len = (u32)(w.c_len + 1 + w.s_dig + 1 + w.e_dig + 1 + w.n_len + 1 + w.d_len + 1 + 1 + 1);
    w.p_q = w.m_q = 0u;
    w.p_k = w.m_k = 0;
    if (a.pvals) {
        if (!epgfmt::e5_scale((uint64_t)__double_as_longlong(a.pvals[r]), &w.p_q, &w.p_k)) w.bad |= EPGM_FLAG_PVAL;
        if (!epgfmt::e5_scale((uint64_t)__double_as_longlong(a.mh[r]), &w.m_q, &w.m_k)) w.bad |= EPGM_FLAG_PVAL;
        w.len += (u32)(1 + epgfmt::e5_len(w.p_k) + 1 + epgfmt::e5_len(w.m_k));
    }
}

__global__ __launch_bounds__(MT_ROWS) void k_mt_lengths(MtArgs a, u32* __restrict__ lens, u64* __restrict__ tile_sum, int* __restrict__ flags) {
    __shared__ u32 s_part[MT_ROWS / 64];
    const long r = (long)blockIdx.x * MT_ROWS + threadIdx.x;
    u32 len = 0;
    if (r < a.R) {
        MtRow w;
        mt_load(a, r, w);
        len = w.len;
        lens[r] = len;
        if (w.bad) atomicOr(flags, w.bad);
    }
    u32 total;
    st_block_scan<MT_ROWS / 64>(len, s_part, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(MT_ROWS) void k_mt_write(MtArgs a, const u32* __restrict__ lens, const u64* __restrict__ tile_off,
                                                      long long* __restrict__ row_off, char* __restrict__ text, long long text_cap,
                                                      int* __restrict__ flags) {
    __shared__ uint4 s_win4[MT_WIN / 16];
    __shared__ u32 s_part[MT_ROWS / 64];
    char* win = reinterpret_cast<char*>(s_win4);
    const int tid = threadIdx.x;
    const long R = a.R;
    const long r0 = (long)blockIdx.x * MT_ROWS, r1 = r0 + MT_ROWS < R ? r0 + MT_ROWS : R, r = r0 + tid;
    const u32 len = r < r1 ? lens[r] : 0u;
    u32 tile_len;
    const u32 before = st_block_scan<MT_ROWS / 64>(len, s_part, &tile_len);
    const long long T0 = (long long)tile_off[blockIdx.x], T1 = T0 + tile_len;
    const long long rs = T0 + before, re = rs + len;
    if (r < r1) row_off[r] = rs;
    if (row_off[R] > text_cap) {                             // (written by k_text_tile_offsets, before this kernel)
        if (blockIdx.x == 0 && tid == 0) atomicOr(flags, EPGM_FLAG_CAP);
        return;
    }
    MtRow w;
    if (r < r1) mt_load(a, r, w);
    for (long long w0 = T0 & ~15ll; w0 < T1; w0 += MT_WIN) {
        const long long w1 = w0 + MT_WIN;
        if (r < r1 && rs < w1 && re > w0) {
            auto put = [&](long long at, char c) {
                const long long k = at - w0;
                if (k >= 0 && k < MT_WIN) win[k] = c;
            };
            auto blob = [&](long long at, const char* src, int n) {          // n bytes of a table's blob, the window's part of them
                long long i0 = w0 - at, i1 = w1 - at;
                if (i0 < 0) i0 = 0;
                if (i1 > n) i1 = n;
                for (long long i = i0; i < i1; ++i) win[at + i - w0] = src[i];
            };
            auto number = [&](long long at, u64 v, int nd) {
                for (int k = nd - 1; k >= 0; --k) {
                    put(at + k, (char)('0' + (int)(v % 10ull)));
                    v /= 10ull;
                }
            };
            long long pos = rs;
            blob(pos, a.chrom + w.c_at, w.c_len);
            pos += w.c_len;
            put(pos++, '\t');
            number(pos, w.start, w.s_dig);
            pos += w.s_dig;
            put(pos++, '\t');
            number(pos, w.end, w.e_dig);
            pos += w.e_dig;
            put(pos++, '\t');
            blob(pos, a.names + w.n_at, w.n_len);
            pos += w.n_len;
            put(pos++, '\t');
            {
                const long long at = pos;
                epgfmt::f5_emit(w.d_bits, w.d_q, [&](int i, char c) { put(at + i, c); });
            }
            pos += w.d_len;
            put(pos++, '\t');
            put(pos++, w.sign);
            if (a.pvals) {
                put(pos++, '\t');
                {
                    const long long at = pos;
                    pos += epgfmt::e5_emit(w.p_q, w.p_k, [&](int i, char c) { put(at + i, c); });
                }
                put(pos++, '\t');
                {
                    const long long at = pos;
                    pos += epgfmt::e5_emit(w.m_q, w.m_k, [&](int i, char c) { put(at + i, c); });
                }
            }
            put(pos, '\n');
        }
        __syncthreads();
        const long long lo = w0 > T0 ? w0 : T0, hi = w1 < T1 ? w1 : T1;
        for (int c = tid; c < MT_WIN / 16; c += MT_ROWS) {
            const long long g = w0 + 16ll * c;
            if (g >= hi || g + 16 <= lo) continue;
            if (g >= lo && g + 16 <= hi) {
                *reinterpret_cast<uint4*>(text + g) = s_win4[c];
            } else {
                for (int j = 0; j < 16; ++j)
                    if (g + j >= lo && g + j < hi) text[g + j] = win[16 * c + j];
            }
        }
        __syncthreads();
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
struct MtLayout {
    int64_t lens, tiles, total, ntiles;
};

static void mt_layout(int64_t R, MtLayout& L) {
    L.ntiles = (R + MT_ROWS - 1) / MT_ROWS;
    L.lens = 0;
    L.tiles = align_up((R > 0 ? R : 1) * 4, 256);
    L.total = L.tiles + align_up((L.ntiles > 0 ? L.ntiles : 1) * 8, 256);
}

extern "C" int64_t epgm_text_bytes_max(int64_t R, int64_t chrom_max, int64_t name_max, int32_t with_p) {
    if (R < 0 || R >= (1LL << 31) || chrom_max < 0 || chrom_max > EPGM_NAME_MAX || name_max < 0 || name_max > EPGM_NAME_MAX) {
        fail(EPG_ERR_INVALID_ARG, "metrics text_bytes_max: bad shape R=%lld chrom_max=%lld name_max=%lld", (long long)R, (long long)chrom_max,
             (long long)name_max);
        return -1;
    }
    // name TAB 19 TAB 19 TAB name TAB 16 TAB sign [TAB 12 TAB 12] NEWLINE
    return R * (chrom_max + name_max + 1 + 19 + 1 + 19 + 1 + 1 + 16 + 1 + 1 + (with_p ? 26 : 0) + 1);
}

extern "C" int64_t epgm_format_ws_bytes(int64_t R) {
    if (R < 0 || R >= (1LL << 31)) {
        fail(EPG_ERR_INVALID_ARG, "metrics format_ws_bytes: bad shape R=%lld", (long long)R);
        return -1;
    }
    MtLayout L;
    mt_layout(R, L);
    return L.total;
}

extern "C" int epgm_format_metrics(const char* chrom, const int64_t* chrom_off, int32_t n_chrom, int64_t chrom_bytes, const int32_t* chrom_idx,
                                   const int64_t* start, const int64_t* end, const char* names, const int64_t* names_off, int32_t n_names,
                                   int64_t names_bytes, const int32_t* maxdiff, const float* dist, const double* pvals, const double* mh,
                                   int64_t R, char* text, int64_t text_cap, int64_t* row_off, int32_t* flags, void* ws, int64_t ws_bytes,
                                   void* stream) {
    if (R < 0 || n_chrom < 0 || n_names < 0 || chrom_bytes < 0 || names_bytes < 0)
        return fail(EPG_ERR_INVALID_ARG, "format_metrics: bad shape R=%lld n_chrom=%d chrom_bytes=%lld n_names=%d names_bytes=%lld", (long long)R, n_chrom,
                    (long long)chrom_bytes, n_names, (long long)names_bytes);
    if (R >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "format_metrics: R=%lld >= 2^31", (long long)R);
    if (R > 0 && !chrom) return fail(EPG_ERR_INVALID_ARG, "format_metrics: chrom is NULL");
    if (R > 0 && !chrom_off) return fail(EPG_ERR_INVALID_ARG, "format_metrics: chrom_off is NULL");
    if (R > 0 && !chrom_idx) return fail(EPG_ERR_INVALID_ARG, "format_metrics: chrom_idx is NULL");
    if (R > 0 && !start) return fail(EPG_ERR_INVALID_ARG, "format_metrics: start is NULL");
    if (R > 0 && !end) return fail(EPG_ERR_INVALID_ARG, "format_metrics: end is NULL");
    if (R > 0 && !names) return fail(EPG_ERR_INVALID_ARG, "format_metrics: names is NULL");
    if (R > 0 && !names_off) return fail(EPG_ERR_INVALID_ARG, "format_metrics: names_off is NULL");
    if (R > 0 && !maxdiff) return fail(EPG_ERR_INVALID_ARG, "format_metrics: maxdiff is NULL");
    if (R > 0 && !dist) return fail(EPG_ERR_INVALID_ARG, "format_metrics: dist is NULL");
    if ((pvals == nullptr) != (mh == nullptr)) return fail(EPG_ERR_INVALID_ARG, "format_metrics: pvals and mh go together, one of them is NULL");
    if (!text) return fail(EPG_ERR_INVALID_ARG, "format_metrics: text is NULL");
    if (!row_off) return fail(EPG_ERR_INVALID_ARG, "format_metrics: row_off is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "format_metrics: flags is NULL");
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "format_metrics: ws is NULL");
    if (reinterpret_cast<uintptr_t>(text) & 255) return fail(EPG_ERR_INVALID_ARG, "format_metrics: text is not 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "format_metrics: ws is not 256-byte aligned");
    if (text_cap < 0) return fail(EPG_ERR_INVALID_ARG, "format_metrics: text_cap=%lld < 0", (long long)text_cap);
    MtLayout L;
    mt_layout(R, L);
    if (ws_bytes < L.total) return fail(EPG_ERR_WORKSPACE, "format_metrics: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)L.total);
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    u32* lens = reinterpret_cast<u32*>(base + L.lens);
    u64* tiles = reinterpret_cast<u64*>(base + L.tiles);
    long long* roff = reinterpret_cast<long long*>(row_off);
    const MtArgs a = {chrom, reinterpret_cast<const long long*>(chrom_off), (int)n_chrom, (long long)chrom_bytes, chrom_idx,
                      reinterpret_cast<const long long*>(start), reinterpret_cast<const long long*>(end), names,
                      reinterpret_cast<const long long*>(names_off), (int)n_names, (long long)names_bytes, maxdiff, dist, pvals, mh, (long)R};
    EPG_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (L.ntiles) {
        hipLaunchKernelGGL(k_mt_lengths, dim3((unsigned)L.ntiles), dim3(MT_ROWS), 0, st, a, lens, tiles, flags);
        EPG_LAUNCH_CHECK("k_mt_lengths");
    }
    hipLaunchKernelGGL(k_text_tile_offsets<1024>, dim3(1), dim3(1024), 0, st, tiles, (long)L.ntiles, (long)R, roff);
    EPG_LAUNCH_CHECK("k_text_tile_offsets");
    if (L.ntiles) {
        hipLaunchKernelGGL(k_mt_write, dim3((unsigned)L.ntiles), dim3(MT_ROWS), 0, st, a, (const u32*)lens, (const u64*)tiles, roff, text,
                           (long long)text_cap, flags);
        EPG_LAUNCH_CHECK("k_mt_write");
    }
    return EPG_OK;
}

}  // namespace epg
