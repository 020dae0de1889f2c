// The scores file read as text on the device (include/epilogos_scores_text.h): a chunk of whole rows -> the int32 grid values,
// the coordinates and the rows where the chromosome changes.  A "%.5f" value is an integer times 1e-5 written in decimal, so the
// grid value is its digits: nothing is rounded.  The parser is strict and reports, never guesses: the first row that is not of
// the grammar goes into the status word and the caller reads the file with the general reader instead.
//
//   k_st_index<false>  st_text_index of epg_text_scan.h over tabs and newlines: one workgroup per segment of ST_SEG bytes, the
//                      number of delimiters ('\t', '\n') of the segment.  A text whose last byte is not '\n' (the end of a file
//                      without a final newline) has a virtual '\n' at position nbytes, so positions 0 .. nbytes are indexed.
//   k_st_scan          one workgroup: exclusive scan of the segment counts in place (st_scan_segments), the total D behind them; the
//                      number of whole rows found (D / F) and, when the text holds more rows than the caller counted, the status.
//   k_st_index<true>   the same pass again: delim[i] = position of the i-th delimiter.
//   k_st_parse         one thread per field: field k of row r lies between delimiters r * F + k - 1 and r * F + k.  The row shape
//                      is checked field by field -- delimiter r * F + k must be '\t', or '\n' for k = F - 1 --, so the first
//                      malformed row is found exactly: every row before it has F - 1 tabs and a newline, hence the indexing
//                      holds up to it; what later rows report is larger and loses the atomic minimum.  The text of a
//                      workgroup's 256 fields is one contiguous span: it is staged in LDS with 16-byte loads (the LDS copy
//                      keeps the source's alignment modulo 16, the span's ragged ends go by bytes) when it fits ST_LDS_TEXT,
//                      and read from global memory when a workgroup meets fields that long.  Consecutive threads hold
//                      consecutive fields, so the X stores of a wave are runs of consecutive dwords broken only where a row's
//                      three coordinate fields sit.
//
// Nothing here reads outside text[0, nbytes) or writes outside rows row0 .. row0 + rows - 1 of the outputs, whatever the text
// holds: positions come from the index of THIS text, and every field's thread is bounded by G <= rows * F and by D.
#include "epg_common.h"
#include "epg_text_scan.h"
#include "epilogos_scores_text.h"

namespace epg {

static constexpr int ST_THREADS = 256;
static constexpr int ST_SEG = ST_THREADS * 16;       // bytes of text per workgroup of the index kernels
static constexpr int ST_SCAN_THREADS = 1024;
static constexpr int ST_LDS_TEXT = 16384;            // bytes of text a parse workgroup stages (256 fields: about 2 KB as a rule)
static constexpr int ST_MAX_SCORE_LEN = 24;
static constexpr int ST_MAX_FIELDS = 1 << 20;

template <bool FILL>
__global__ __launch_bounds__(ST_THREADS) void k_st_index(const char* __restrict__ text, long n, u32* __restrict__ seg,
                                                         u32* __restrict__ delim) {
    __shared__ u32 part[ST_THREADS / 64];
    st_text_index<FILL, ST_THREADS / 64>(text, n, seg, delim, 0xffffffffu, part, StIsTabOrNewline{});
}

__device__ __forceinline__ void st_report(unsigned long long* status, long row, int reason) {
    const unsigned long long word = ((unsigned long long)row << 4) | (unsigned)reason;
    if (word < *reinterpret_cast<volatile unsigned long long*>(status)) atomicMin(status, word);
}

// seg[0 .. nseg): counts -> exclusive offsets; seg[nseg] = D
__global__ __launch_bounds__(ST_SCAN_THREADS) void k_st_scan(u32* __restrict__ seg, int nseg, int F, long rows, long row0,
                                                             long long* __restrict__ status) {
    __shared__ u32 part[ST_SCAN_THREADS / 64];
    const u32 carry = st_scan_segments<ST_SCAN_THREADS / 64>(seg, nseg, part);
    if (threadIdx.x == 0) {
        seg[nseg] = carry;
        status[1] = (long long)(carry / (u32)F);
        if ((long)carry > rows * F) st_report(reinterpret_cast<unsigned long long*>(status), row0 + rows, EPGT_REASON_ROWS);
    }
}

struct StGlobal {
    const char* p;
    __device__ __forceinline__ u32 operator()(u32 i) const { return (unsigned char)p[i]; }
};
struct StLds {
    const unsigned char* lds;
    int bias;                                                    // text position of lds[0]; negative when the text starts misaligned
    __device__ __forceinline__ u32 operator()(u32 i) const { return lds[(int)i - bias]; }
};

__device__ __forceinline__ bool st_digit(u32 c) { return c - '0' < 10u; }

// Field k of a row, text[b, e): 0 and *val (coordinates and scores), or the reason it is not of the grammar.
template <class Rd>
__device__ __forceinline__ int st_parse_field(const Rd& rd, u32 b, u32 e, int k, long long* val) {
    if (e == b) return EPGT_REASON_EMPTY;
    for (u32 i = b; i < e; ++i) {
        const u32 c = rd(i);
        if (c < 0x21 || c > 0x7e) return EPGT_REASON_BYTE;
    }
    if (k == 0) {
        const u32 c = rd(b) | 0x20;                              // a letter or '_' first: nothing pandas could type as a number
        return (c - 'a' < 26u || rd(b) == '_') ? 0 : EPGT_REASON_CHROM;
    }
    if (k < 3) {
        if (e - b > 19) return EPGT_REASON_COORD;
        unsigned long long v = 0;
        for (u32 i = b; i < e; ++i) {
            const u32 c = rd(i);
            if (!st_digit(c)) return EPGT_REASON_COORD;
            v = v * 10 + (c - '0');                              // 19 digits stay below 2^64
        }
        if (v > (unsigned long long)INT64_MAX) return EPGT_REASON_COORD;
        *val = (long long)v;
        return 0;
    }
    if (e - b > ST_MAX_SCORE_LEN) return EPGT_REASON_SCORE;
    u32 i = b;
    const bool neg = rd(i) == '-';
    if (neg) ++i;
    unsigned long long ip = 0;
    int nd = 0;
    for (; i < e && st_digit(rd(i)); ++i, ++nd) {
        ip = ip * 10 + (rd(i) - '0');
        if (ip > (1ull << 40)) ip = 1ull << 40;                  // out of range already: stay there, never wrap
    }
    if (nd == 0) return EPGT_REASON_SCORE;
    u32 frac = 0;
    int nf = 0;
    if (i < e && rd(i) == '.') {
        ++i;
        for (; i < e && st_digit(rd(i)); ++i) {
            if (++nf > 5) return EPGT_REASON_SCORE;
            frac = frac * 10 + (rd(i) - '0');
        }
        if (nf == 0) return EPGT_REASON_SCORE;
    }
    if (i != e) return EPGT_REASON_SCORE;
    for (; nf < 5; ++nf) frac *= 10;
    const unsigned long long v = ip * 100000ull + frac;
    if (v >= (1ull << 31)) return EPGT_REASON_RANGE;
    *val = neg ? -(long long)v : (long long)v;
    return 0;
}

__global__ __launch_bounds__(ST_THREADS) void k_st_parse(const char* __restrict__ text, long n, int F, long rows, long row0,
                                                         int32_t* __restrict__ X, int64_t* __restrict__ start,
                                                         int64_t* __restrict__ end, int32_t* __restrict__ chrom_at,
                                                         const u32* __restrict__ delim, const u32* __restrict__ Dp, u32 G,
                                                         long long* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[ST_LDS_TEXT + 32];
    const int t = threadIdx.x;
    const u32 D = *Dp;
    const u32 g_lo = blockIdx.x * (u32)ST_THREADS;
    u32 g_hi = g_lo + ST_THREADS;
    if (g_hi > G) g_hi = G;
    if (g_hi > D) g_hi = D;

    // the span of this workgroup's fields, text[sb, se), into LDS when it fits (workgroup-uniform)
    bool staged = false;
    u32 sb = 0;
    int mis = 0;
    if (g_hi > g_lo) {
        sb = g_lo ? delim[g_lo - 1] + 1 : 0;
        u32 se = delim[g_hi - 1];
        if ((long)se > n) se = (u32)n;
        const u32 len = se - sb;
        if (len <= (u32)ST_LDS_TEXT) {
            staged = true;
            const char* src = text + sb;
            mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);  // lds[mis + i] = src[i]
            u32 head = mis ? 16u - (u32)mis : 0u;
            if (head > len) head = len;
            if ((u32)t < head) lds[mis + t] = (unsigned char)src[t];
            const u32 nvec = (len - head) >> 4;
            for (u32 v = t; v < nvec; v += ST_THREADS)
                *reinterpret_cast<uint4*>(lds + mis + head + 16 * v) = *reinterpret_cast<const uint4*>(src + head + 16 * v);
            for (u32 i = head + 16 * nvec + t; i < len; i += ST_THREADS) lds[mis + i] = (unsigned char)src[i];
        }
    }
    __syncthreads();

    const u32 g = g_lo + t;
    if (g >= G) return;
    const long r = g / (u32)F;
    const int k = (int)(g - (u32)r * (u32)F);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status);
    if (g >= D) {                                                // the text ends before this row does
        st_report(st, row0 + r, EPGT_REASON_FIELDS);
        return;
    }
    const u32 b = g ? delim[g - 1] + 1 : 0;
    const u32 e = delim[g];
    const u32 closing = (long)e < n ? (unsigned char)text[e] : '\n';
    if (closing != (k == F - 1 ? '\n' : '\t')) {
        st_report(st, row0 + r, EPGT_REASON_FIELDS);
        return;
    }
    long long val = 0;
    const int reason = staged ? st_parse_field(StLds{lds, (int)sb - mis}, b, e, k, &val) : st_parse_field(StGlobal{text}, b, e, k, &val);
    if (reason) {
        st_report(st, row0 + r, reason);
        return;
    }
    const long row = row0 + r;
    if (k >= 3) {
        X[row * (F - 3) + (k - 3)] = (int32_t)val;
    } else if (k == 2) {
        end[row] = val;
    } else if (k == 1) {
        start[row] = val;
    } else {
        bool same = false;
        if (r > 0) {                                             // the previous row's chromosome, out of global memory
            const u32 pb = g - (u32)F ? delim[g - (u32)F - 1] + 1 : 0;
            const u32 pe = delim[g - (u32)F];
            same = pe - pb == e - b;
            for (u32 i = 0; same && i < e - b; ++i) same = text[pb + i] == text[b + i];
        }
        chrom_at[row] = same ? -1 : (int32_t)b;
    }
}

static int64_t st_seg_bytes(int64_t nbytes) { return align_up((nbytes / ST_SEG + 2) * 4, 256); }

extern "C" int64_t epgt_scores_ws_bytes(int64_t nbytes) {
    if (nbytes < 0 || nbytes > EPGT_MAX_CHUNK_BYTES)
        return fail(EPG_ERR_INVALID_ARG, "scores_ws_bytes: %lld bytes outside 0..%lld", (long long)nbytes, (long long)EPGT_MAX_CHUNK_BYTES);
    return st_seg_bytes(nbytes) + align_up((nbytes + 1) * 4, 256);
}

extern "C" int epgt_scores_parse(const char* text, int64_t nbytes, int32_t F, int64_t rows, int64_t row0, int32_t* X, int64_t* start,
                                 int64_t* end, int32_t* chrom_at, void* ws, int64_t ws_bytes, int64_t* status, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (nbytes < 0 || nbytes > EPGT_MAX_CHUNK_BYTES)
        return fail(EPG_ERR_INVALID_ARG, "scores_parse: %lld bytes outside 0..%lld", (long long)nbytes, (long long)EPGT_MAX_CHUNK_BYTES);
    if (F < 4 || F > ST_MAX_FIELDS) return fail(EPG_ERR_INVALID_ARG, "scores_parse: %d fields per row outside 4..%d", F, ST_MAX_FIELDS);
    if (rows < 0 || rows > nbytes)
        return fail(EPG_ERR_INVALID_ARG, "scores_parse: %lld rows in %lld bytes", (long long)rows, (long long)nbytes);
    if (row0 < 0 || row0 > (INT64_MAX >> 5) - rows) return fail(EPG_ERR_INVALID_ARG, "scores_parse: bad row offset %lld", (long long)row0);
    if (nbytes == 0) return EPG_OK;
    if (!text || !ws || !status) return fail(EPG_ERR_INVALID_ARG, "scores_parse: NULL argument");
    if (rows > 0 && (!X || !start || !end || !chrom_at)) return fail(EPG_ERR_INVALID_ARG, "scores_parse: NULL output");
    if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(EPG_ERR_INVALID_ARG, "scores_parse: the workspace is not 16-byte aligned");
    const int64_t need = epgt_scores_ws_bytes(nbytes);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "scores_parse: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
    const int nseg = (int)(nbytes / ST_SEG + 1);
    u32* seg = reinterpret_cast<u32*>(ws);
    u32* delim = reinterpret_cast<u32*>(reinterpret_cast<char*>(ws) + st_seg_bytes(nbytes));
    hipLaunchKernelGGL(k_st_index<false>, dim3((unsigned)nseg), dim3(ST_THREADS), 0, st, text, (long)nbytes, seg, delim);
    EPG_LAUNCH_CHECK("k_st_index<count>");
    hipLaunchKernelGGL(k_st_scan, dim3(1), dim3(ST_SCAN_THREADS), 0, st, seg, nseg, (int)F, (long)rows, (long)row0,
                       reinterpret_cast<long long*>(status));
    EPG_LAUNCH_CHECK("k_st_scan");
    hipLaunchKernelGGL(k_st_index<true>, dim3((unsigned)nseg), dim3(ST_THREADS), 0, st, text, (long)nbytes, seg, delim);
    EPG_LAUNCH_CHECK("k_st_index<fill>");
    if (rows > 0) {
        // G fields get a thread: all of them, or -- rows that cannot all be whole, the text has nbytes + 1 delimiters at most --
        // enough to reach the first field behind the text's last delimiter, whose thread reports the short row
        const int64_t fields = rows * F < nbytes + 2 ? rows * F : nbytes + 2;
        hipLaunchKernelGGL(k_st_parse, dim3((unsigned)((fields + ST_THREADS - 1) / ST_THREADS)), dim3(ST_THREADS), 0, st, text,
                           (long)nbytes, (int)F, (long)rows, (long)row0, X, start, end, chrom_at, (const u32*)delim,
                           (const u32*)(seg + nseg), (u32)fields, reinterpret_cast<long long*>(status));
        EPG_LAUNCH_CHECK("k_st_parse");
    }
    return EPG_OK;
}

}  // namespace epg
