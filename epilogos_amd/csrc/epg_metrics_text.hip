// The device metrics writer (epg_metrics_text.h): the rows of pairwiseMetrics_*.txt.gz as text.  gfx950 only.
//
// The row writer of epg_text_rows.h (three launches on the caller's stream: lengths, tile offsets, write) with the metrics row as its
// policy, MtArgs.  load() reads and checks the row's fields: table indices and table entries against their bounds, the coordinates'
// sign, the distance against epg_fmt_f5.h, the p-values against epg_fmt_e5.h -- integer arithmetic only; refused fields are OR-ed into
// the flag word and formatted as nothing or zero.  A tile of 256 rows is ~20 KB: one window.
// Nothing synchronises.  Every read of a table goes through an index and an offset pair that were checked first.
#include "epg_common.h"
#include "epg_metrics_text.h"
#include "epg_text_rows.h"
#include "epg_fmt_f5.h"
#include "epg_fmt_e5.h"

namespace epg {

// a row's fields, checked and scaled: what both passes need
struct MtRow {
    long long c_at, n_at;                                   // where the two names start in their blobs
    int c_len, n_len;
    u64 start, end;
    int s_dig, e_dig;
    u32 d_bits;                                             // |dist|
    uint64_t d_q;
    char sign;
    u32 p_q, m_q;
    int p_k, m_k;
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
    using Row = MtRow;
    static constexpr int FLAG_CAP = EPGM_FLAG_CAP;

    __device__ __forceinline__ u32 load(long r, MtRow& w, int& bad) const {
        if (!mt_entry(chrom_off, n_chrom, chrom_bytes, chrom_idx[r], &w.c_at, &w.c_len)) bad |= EPGM_FLAG_CHROM;
        if (!mt_entry(names_off, n_names, names_bytes, (long long)maxdiff[r] - 1, &w.n_at, &w.n_len)) bad |= EPGM_FLAG_STATE;
        long long s = start[r], e = end[r];
        if (s < 0 || e < 0) {
            bad |= EPGM_FLAG_COORD;
            s = s < 0 ? 0 : s;
            e = e < 0 ? 0 : e;
        }
        w.start = (u64)s;
        w.end = (u64)e;
        w.s_dig = mt_digits(w.start);
        w.e_dig = mt_digits(w.end);
        const float d = dist[r];
        w.d_bits = __float_as_uint(d) & 0x7fffffffu;
        if (!epgfmt::f5_scale(w.d_bits, &w.d_q)) bad |= EPGM_FLAG_DIST;
        w.sign = d >= 0.0f ? '+' : '-';
        u32 len = (u32)(w.c_len + 1 + w.s_dig + 1 + w.e_dig + 1 + w.n_len + 1 + epgfmt::f5_len(w.d_bits, w.d_q) + 1 + 1 + 1);
        w.p_q = w.m_q = 0u;
        w.p_k = w.m_k = 0;
        if (pvals) {
            if (!epgfmt::e5_scale((uint64_t)__double_as_longlong(pvals[r]), &w.p_q, &w.p_k)) bad |= EPGM_FLAG_PVAL;
            if (!epgfmt::e5_scale((uint64_t)__double_as_longlong(mh[r]), &w.m_q, &w.m_k)) bad |= EPGM_FLAG_PVAL;
            len += (u32)(1 + epgfmt::e5_len(w.p_k) + 1 + epgfmt::e5_len(w.m_k));
        }
        return len;
    }

    __device__ __forceinline__ void emit(long, const MtRow& w, TextSink& sink) const {
        sink.bytes(chrom + w.c_at, w.c_len);
        sink.put('\t');
        sink.digits(w.start, w.s_dig);
        sink.put('\t');
        sink.digits(w.end, w.e_dig);
        sink.put('\t');
        sink.bytes(names + w.n_at, w.n_len);
        sink.put('\t');
        sink.skip(epgfmt::f5_emit(w.d_bits, w.d_q, sink.at()));
        sink.put('\t');
        sink.put(w.sign);
        if (pvals) {
            sink.put('\t');
            sink.skip(epgfmt::e5_emit(w.p_q, w.p_k, sink.at()));
            sink.put('\t');
            sink.skip(epgfmt::e5_emit(w.m_q, w.m_k, sink.at()));
        }
    }
};

// ---- entry points ----------------------------------------------------------------------------------------------------------------
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
    return text_rows_ws_bytes(R);
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
    if (const int rc = text_rows_check_out("format_metrics", text, text_cap, row_off, flags, ws, ws_bytes, text_rows_ws_bytes(R))) return rc;
    const MtArgs a = {chrom, reinterpret_cast<const long long*>(chrom_off), (int)n_chrom, (long long)chrom_bytes, chrom_idx,
                      reinterpret_cast<const long long*>(start), reinterpret_cast<const long long*>(end), names,
                      reinterpret_cast<const long long*>(names_off), (int)n_names, (long long)names_bytes, maxdiff, dist, pvals, mh, (long)R};
    return text_rows_launch(a, R, text, text_cap, row_off, flags, ws, (hipStream_t)stream, "k_mt_lengths", "k_mt_write");
}

}  // namespace epg
