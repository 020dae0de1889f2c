// The device text writer (epg_textout.h): score text and its BGZF compression.  gfx950 only.
//
// Format: the row writer of epg_text_rows.h (three launches on the caller's stream: lengths, tile offsets, write) with the score row as
// its policy, TwRows: the location's bytes, then S times a tab and a "%.5f" value (epg_fmt_f5.h: integer arithmetic only).  Refused
// values and bad locations are OR-ed into the flag word.  A tile of 256 rows of an 18-state model is ~46 KB, two windows: the policy
// skips the values that lie in front of a window without formatting them and stops at the first one behind it.
// Compress, three launches (the phases are in epg_bgzf_block.h, which also says what is matched):
//   * k_bgzf_plan    a workgroup per block of 65 280 text bytes: histogram walk + CRC-32, one thread builds the code and the block
//                    header, second walk for the threads' bit counts, workgroup scan (epg_text_scan.h), the block's record (size,
//                    code, header bits, bit offsets: 2.3 KB) into the workspace.  LDS: ~9 KB.
//   * k_bgzf_offsets one workgroup: the exclusive scan of the blocks' sizes (st_scan_chunks of epg_text_scan.h), the stream's size
//                    into n_out.
//   * k_bgzf_emit    a workgroup per block (and one for the end-of-file block): the member is put together in 64 KB of zeroed LDS
//                    -- header, DEFLATE bits by atomic OR at the recorded bit offsets (third walk) or the stored bytes, CRC-32 and
//                    ISIZE -- shifted so that 16-byte chunks of LDS are 16-byte chunks of `out`, and stored by st_store_span
//                    (epg_text_scan.h).  LDS: 64 KB + 1 KB, two workgroups per CU.
// Nothing synchronises: the text's size reaches epgw_bgzf_compress as the host value n, see the header.
#include "epg_common.h"
#include "epg_textout.h"
#include "epg_text_rows.h"
#include "epg_fmt_f5.h"
#include "epg_bgzf_block.h"

namespace epg {

// the score row: its location and S values
struct TwRow {
    long long lo0, llen;                                     // the location's bytes in the blob, without their newline
};

struct TwRows {
    const float* scores;
    long R;
    int S;
    long ld;
    const char* loc;
    const long long* loc_off;
    using Row = TwRow;
    static constexpr int FLAG_CAP = 2;

    __device__ __forceinline__ u32 load(long r, TwRow& w, int& bad) const {
        w.lo0 = loc_off[r];
        long long L = loc_off[r + 1] - w.lo0 - 1;
        if (L < 0 || L > (1 << 20)) { L = 0; bad = 2; }      // (a location of a megabyte is no location: the tile's sum stays 32 bits)
        w.llen = L;
        const float* row = scores + r * ld;
        for (int s = 0; s < S; ++s) {
            const u32 bits = __float_as_uint(row[s]);
            uint64_t q;
            if (!epgfmt::f5_scale(bits, &q)) bad |= 1;
            L += 1 + epgfmt::f5_len(bits, q);
        }
        return (u32)(L + 1);
    }

    __device__ __forceinline__ void emit(long r, const TwRow& w, TextSink& sink) const {
        sink.bytes(loc + w.lo0, w.llen);
        const float* row = scores + r * ld;
        for (int s = 0; s < S && !sink.past(); ++s) {
            const u32 bits = __float_as_uint(row[s]);
            uint64_t q;
            epgfmt::f5_scale(bits, &q);
            const int L = 1 + epgfmt::f5_len(bits, q);
            if (sink.in_front(L)) {
                sink.skip(L);
            } else {
                sink.put('\t');
                sink.skip(epgfmt::f5_emit(bits, q, sink.at()));
            }
        }
    }
};

// ---- BGZF ----------------------------------------------------------------------------------------------------------------------------
using epgbg::BG_T;
using epgbg::BG_TEXT;
constexpr int BG_STAGE = 65536 + 64;
constexpr int BG_SCAN_THREADS = 1024;

__global__ __launch_bounds__(BG_T) void k_bgzf_plan(const unsigned char* __restrict__ text, long long n, const long long* __restrict__ row_off, long long R,
                                                    epgbg::Rec* __restrict__ recs) {
    __shared__ epgbg::Shared sh;
    __shared__ u32 s_part[BG_T / 64];
    const int t = threadIdx.x;
    const long long B0 = (long long)blockIdx.x * BG_TEXT, B1 = B0 + BG_TEXT < n ? B0 + BG_TEXT : n;
    const epgbg::Rows rw = epgbg::make_rows(row_off, R, n);
    epgbg::Rec& rec = recs[blockIdx.x];
    epgbg::plan_init(sh, t);
    __syncthreads();
    if (t == 0) epgbg::plan_rows(sh, rw, B0, B1);
    __syncthreads();
    epgbg::plan_hist(sh, text, rw, B0, B1, t);
    __syncthreads();
    if (t == 0) {
        sh.hist[256] += 1;                                  // the end-of-block symbol
        epgbg::build_block_code(sh);
    }
    __syncthreads();
    u32 total;
    const u32 before = st_block_scan<BG_T / 64>(epgbg::plan_bits(sh, text, rw, B0, B1, t), s_part, &total);
    rec.tbits[t] = sh.hdr_bits + before;
    for (int i = t; i < epgbg::BG_NSYM; i += BG_T) {
        rec.code[i] = sh.code[i];
        rec.len[i] = sh.len[i];
    }
    for (int i = t; i < epgbg::BG_HDR_WORDS; i += BG_T) rec.hdr[i] = sh.hdr[i];
    if (t == 0) epgbg::plan_finish(sh, rec, total, B0, B1);
}

__global__ __launch_bounds__(BG_SCAN_THREADS) void k_bgzf_offsets(const epgbg::Rec* __restrict__ recs, long nblocks, int eof, long long* __restrict__ blk_off,
                                                                  long long* __restrict__ n_out) {
    __shared__ u64 s_sum[BG_SCAN_THREADS];
    const long long run = (long long)st_scan_chunks<BG_SCAN_THREADS>(nblocks, s_sum, [&](long b) { return (u64)recs[b].size; },
                                                                     [&](long b, u64 x) { blk_off[b] = (long long)x; });
    if (threadIdx.x == BG_SCAN_THREADS - 1) {
        blk_off[nblocks] = run;
        n_out[0] = run + (eof ? 28 : 0);
    }
}

__global__ __launch_bounds__(BG_T) void k_bgzf_emit(const unsigned char* __restrict__ text, long long n, const long long* __restrict__ row_off, long long R,
                                                    const epgbg::Rec* __restrict__ recs, const long long* __restrict__ blk_off, long nblocks,
                                                    unsigned char* __restrict__ out, long long out_cap, int* __restrict__ flags) {
    extern __shared__ uint4 s_stage4[];
    __shared__ u16 s_code[epgbg::BG_NSYM];
    __shared__ unsigned char s_len[epgbg::BG_NSYM];
    const int t = threadIdx.x;
    if ((long)blockIdx.x == nblocks) {                       // the end-of-file block
        const unsigned char eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const long long at = blk_off[nblocks];
        if (at + 28 > out_cap) {
            if (t == 0) atomicOr(flags, 1);
        } else if (t < 28) {
            out[at + t] = eof_block[t];
        }
        return;
    }
    const epgbg::Rec& rec = recs[blockIdx.x];
    const long long at = blk_off[blockIdx.x];
    const u32 size = rec.size;
    if (at + size > out_cap) {
        if (t == 0) atomicOr(flags, 1);
        return;
    }
    const long long B0 = (long long)blockIdx.x * BG_TEXT, B1 = B0 + BG_TEXT < n ? B0 + BG_TEXT : n;
    const u32 a = (u32)(at & 15);
    u32* words = reinterpret_cast<u32*>(s_stage4);
    unsigned char* bytes = reinterpret_cast<unsigned char*>(s_stage4);
    const int nchunks = (int)((a + size + 15u) >> 4);
    for (int c = t; c < nchunks + 1; c += BG_T) s_stage4[c] = make_uint4(0, 0, 0, 0);
    for (int i = t; i < epgbg::BG_NSYM; i += BG_T) {
        s_code[i] = rec.code[i];
        s_len[i] = rec.len[i];
    }
    __syncthreads();
    epgbg::emit_frame(words, a, rec, t);
    const bool stored = rec.stored != 0;
    if (stored) {
        __syncthreads();                                    // the frame's atomics are done before bytes of the same words are stored
        for (u32 i = t; i < rec.n_text; i += BG_T) bytes[a + 23u + i] = text[B0 + i];
    } else {
        const epgbg::Rows rw = epgbg::make_rows(row_off, R, n);
        epgbg::emit_tokens(words, a, rec, s_code, s_len, text, rw, B0, B1, t);
    }
    __syncthreads();
    st_store_span(s_stage4, out + (at - a), a, size, t, BG_T);
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static int64_t bg_blocks(int64_t n) { return (n + BG_TEXT - 1) / BG_TEXT; }
static int64_t bg_recs_at(int64_t nblocks) { return align_up((nblocks + 1) * 8, 256); }

extern "C" int64_t epgw_text_bytes_max(int64_t R, int32_t S, int64_t loc_bytes) {
    if (R < 0 || S < 1 || S > 4096 || loc_bytes < 0 || R >= (1LL << 31) || loc_bytes >= (1LL << 61)) {
        fail(EPG_ERR_INVALID_ARG, "text_bytes_max: bad shape R=%lld S=%d loc_bytes=%lld", (long long)R, S, (long long)loc_bytes);
        return -1;
    }
    return loc_bytes + R * 18 * (int64_t)S;
}

extern "C" int64_t epgw_format_ws_bytes(int64_t R) {
    if (R < 0 || R >= (1LL << 31)) {
        fail(EPG_ERR_INVALID_ARG, "format_ws_bytes: bad shape R=%lld", (long long)R);
        return -1;
    }
    return text_rows_ws_bytes(R);
}

extern "C" int epgw_format_scores(const float* scores, int64_t R, int32_t S, int64_t ld, const char* loc, const int64_t* loc_off, char* text,
                                  int64_t text_cap, int64_t* row_off, int32_t* flags, void* ws, int64_t ws_bytes, void* stream) {
    if (R < 0 || S < 1 || S > 4096 || ld < S) return fail(EPG_ERR_INVALID_ARG, "format_scores: bad shape R=%lld S=%d ld=%lld", (long long)R, S, (long long)ld);
    if (R >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "format_scores: R=%lld >= 2^31", (long long)R);
    if (R > 0 && !scores) return fail(EPG_ERR_INVALID_ARG, "format_scores: scores is NULL");
    if (R > 0 && !loc) return fail(EPG_ERR_INVALID_ARG, "format_scores: loc is NULL");
    if (R > 0 && !loc_off) return fail(EPG_ERR_INVALID_ARG, "format_scores: loc_off is NULL");
    if (const int rc = text_rows_check_out("format_scores", text, text_cap, row_off, flags, ws, ws_bytes, text_rows_ws_bytes(R))) return rc;
    const TwRows p = {scores, (long)R, (int)S, (long)ld, loc, reinterpret_cast<const long long*>(loc_off)};
    return text_rows_launch(p, R, text, text_cap, row_off, flags, ws, (hipStream_t)stream, "k_tw_lengths", "k_tw_write");
}

extern "C" int64_t epgw_bgzf_bytes_max(int64_t n, int32_t eof) {
    if (n < 0 || n >= (1LL << 40)) {
        fail(EPG_ERR_INVALID_ARG, "bgzf_bytes_max: bad size n=%lld", (long long)n);
        return -1;
    }
    return n + bg_blocks(n) * (epgbg::BG_MEMBER_EXTRA + 5) + (eof ? 28 : 0);
}

extern "C" int64_t epgw_bgzf_ws_bytes(int64_t n) {
    if (n < 0 || n >= (1LL << 40)) {
        fail(EPG_ERR_INVALID_ARG, "bgzf_ws_bytes: bad size n=%lld", (long long)n);
        return -1;
    }
    const int64_t nb = bg_blocks(n);
    return align_up(bg_recs_at(nb) + nb * (int64_t)sizeof(epgbg::Rec), 256);
}

extern "C" int epgw_bgzf_compress(const char* text, int64_t n, const int64_t* row_off, int64_t R, int32_t eof, char* out, int64_t out_cap,
                                  int64_t* n_out, int32_t* flags, void* ws, int64_t ws_bytes, void* stream) {
    if (n < 0 || R < 0) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: bad shape n=%lld R=%lld", (long long)n, (long long)R);
    if (n >= (1LL << 40)) return fail(EPG_ERR_UNSUPPORTED, "bgzf_compress: n=%lld >= 2^40", (long long)n);
    if (R >= (1LL << 31)) return fail(EPG_ERR_UNSUPPORTED, "bgzf_compress: R=%lld >= 2^31", (long long)R);
    if (n > 0 && !text) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: text is NULL");
    if (R > 0 && !row_off) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: row_off is NULL");
    if (!out) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: out is NULL");
    if (!n_out) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: n_out is NULL");
    if (!flags) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: flags is NULL");
    if (!ws) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: ws is NULL");
    if (reinterpret_cast<uintptr_t>(out) & 255) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: out is not 256-byte aligned");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: ws is not 256-byte aligned");
    if (out_cap < 0) return fail(EPG_ERR_INVALID_ARG, "bgzf_compress: out_cap=%lld < 0", (long long)out_cap);
    const int64_t nb = bg_blocks(n);
    const int64_t need = align_up(bg_recs_at(nb) + nb * (int64_t)sizeof(epgbg::Rec), 256);
    if (ws_bytes < need) return fail(EPG_ERR_WORKSPACE, "bgzf_compress: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    long long* blk_off = reinterpret_cast<long long*>(base);
    epgbg::Rec* recs = reinterpret_cast<epgbg::Rec*>(base + bg_recs_at(nb));
    const unsigned char* txt = reinterpret_cast<const unsigned char*>(text);
    const long long* roff = reinterpret_cast<const long long*>(row_off);
    EPG_HIP(hipMemsetAsync(flags, 0, sizeof(int32_t), st));
    if (nb) {
        hipLaunchKernelGGL(k_bgzf_plan, dim3((unsigned)nb), dim3(BG_T), 0, st, txt, (long long)n, roff, (long long)R, recs);
        EPG_LAUNCH_CHECK("k_bgzf_plan");
    }
    hipLaunchKernelGGL(k_bgzf_offsets, dim3(1), dim3(BG_SCAN_THREADS), 0, st, (const epgbg::Rec*)recs, (long)nb, (int)eof, blk_off,
                       reinterpret_cast<long long*>(n_out));
    EPG_LAUNCH_CHECK("k_bgzf_offsets");
    const unsigned grid = (unsigned)(nb + (eof ? 1 : 0));
    if (grid) {
        static DynLds lds_attr;
        EPG_HIP(ensure_dyn_lds(lds_attr, reinterpret_cast<const void*>(k_bgzf_emit), BG_STAGE));
        hipLaunchKernelGGL(k_bgzf_emit, dim3(grid), dim3(BG_T), BG_STAGE, st, txt, (long long)n, roff, (long long)R, (const epgbg::Rec*)recs,
                           (const long long*)blk_off, (long)nb, reinterpret_cast<unsigned char*>(out), (long long)out_cap, flags);
        EPG_LAUNCH_CHECK("k_bgzf_emit");
    }
    return EPG_OK;
}

}  // namespace epg
