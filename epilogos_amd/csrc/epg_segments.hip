// ChromHMM segment files read on the device (include/epilogos_segments.h): the text of one biosample's whole-genome file -> the
// first bin and the state of every line and the run of lines of every chromosome of a table, and a chromosome's run -> its column
// of int8 states.  The columns go into the matrix with k_sbl_transpose (epg_statebyline.hip).
//
// The parser is the index / scan / fill split of epg_scores_text.hip with lines for fields (st_text_index and st_scan_segments of
// epg_text_scan.h), and a second scan over the lines:
//
//   k_seg_index<false>  st_text_index over newlines: one workgroup per segment of SEG_BLOCK bytes, the number of newlines of the
//                       segment.  A text whose last byte is not '\n' has a virtual '\n' at position nbytes, so positions
//                       0 .. nbytes are looked at.
//   k_seg_scan          one workgroup: exclusive scan of the segment counts in place (st_scan_segments), the number of lines behind
//                       them; info, runs and the per-chromosome words initialised.
//   k_seg_index<true>   the same pass again: nl[i] = position of the i-th newline.
//   k_seg_parse         one thread per line.  The text of a workgroup's 256 lines is one contiguous span, staged in LDS the way
//                       k_st_parse stages its fields (and read from global memory when a workgroup meets lines that long).  A
//                       thread reads its four fields, compares its chromosome field with the previous line's (out of global
//                       memory: the previous line of a workgroup's first thread is not in its span) and, only where the two
//                       differ -- a run starts: tens of lines of a file --, looks the name up in the table, a linear search, and
//                       leaves its line number in the chromosome's word by an atomic minimum.  meta[l] = (0: inside a run,
//                       1: starts a run of a chromosome outside the table, 2 + c: of chromosome c) << 8 | the state as written
//                       (0: outside the per-line grammar).  The workgroup's last run start goes into blk[].
//   k_seg_runs          one workgroup: maximum-scan of blk[] in place: the last run start up to the end of each workgroup's lines.
//   k_seg_link          one thread per line again.  A maximum-scan of the run starts gives every line the line its run starts
//                       at, hence its chromosome.  The cross-line rules, for the table's chromosomes: a run starts at 0, a chromosome's word holds the start
//                       of its FIRST run (the start of a second one is the offence), any other line starts at the end of the line
//                       before it.  The states of the table's chromosomes go into the range; the last line of a run writes
//                       runs[c].
//
// A line's verdict depends on itself and on the line before it, the one-run rule on the run starts before it: the first
// offending line is exact, what later lines report loses the atomic minimum (as in the scores-text reader).
//
// A line of the grammar is 8 bytes or more with its newline ("c\t0\t1\t1\n"), so a text of n bytes whose first n / 8 + 1 lines
// are of the grammar has no further line: the per-line arrays hold SEG_LINES(n) = n / 8 + 2 lines, and a text with more has
// its first offence among them.  info[0] is the count of all lines either way.
//
//   k_seg_expand        the hot path, driven from the output: one workgroup per SEG_TILE bins of the column, a thread per 16 bins
//                       and one 16-byte store.  The workgroup finds the lines of its first and last bin by two upper-bound
//                       searches over the run's first[] (interleaved: one chain of dependent loads deep, log2(lines) long) and
//                       stages the lines between them in LDS -- a tile holds SEG_TILE lines at most, every line being a bin or
//                       more.  A thread finds the line of its first bin by an upper-bound search in LDS; when the next line
//                       starts at or behind its 16th bin it stores a splat, else it walks forward one compare per bin.  Nothing
//                       loops over a run's length.  The run (first line, lines, R_c) is read from runs[] on the device; the
//                       grid covers the caller's R and workgroups behind R_c leave at once.
//
// Nothing here reads outside text[0, nbytes), the table, first/state[0, cap) or writes outside first/state[0, min(lines, cap)),
// runs, info, the workspace and col[0, min(R, R_c)).
#include "epg_common.h"
#include "epg_text_scan.h"
#include "epilogos_segments.h"

namespace epg {

static constexpr int SEG_THREADS = 256;
static constexpr int SEG_THREAD_BYTES = 16;
static constexpr int SEG_BLOCK = SEG_THREADS * SEG_THREAD_BYTES;   // bytes of text per workgroup of the index kernels
static constexpr int SEG_SCAN_THREADS = 1024;
static constexpr int SEG_LDS_TEXT = 16384;                         // bytes of text a parse workgroup stages (256 lines: about 6 KB as a rule)
static constexpr int SEG_TILE = SEG_THREADS * 16;                  // bins per workgroup of the expansion
static constexpr int SEG_MAX_CHROMS = 4096;
static constexpr int SEG_MIN_LINE = 8;

static inline int64_t seg_lines(int64_t nbytes) { return nbytes / SEG_MIN_LINE + 2; }

static_assert(SEG_THREAD_BYTES == 16, "st_text_index gives a thread 16 bytes of text");

template <bool FILL>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_index(const char* __restrict__ text, long n, u32* __restrict__ seg,
                                                           u32* __restrict__ nl, u32 lmax) {
    __shared__ u32 part[SEG_THREADS / 64];
    st_text_index<FILL, SEG_THREADS / 64>(text, n, seg, nl, lmax, part, StIsNewline{});
}

// seg[0 .. nseg): counts -> exclusive offsets; seg[nseg] = the number of lines; the outputs initialised
__global__ __launch_bounds__(SEG_SCAN_THREADS) void k_seg_scan(u32* __restrict__ seg, int nseg, long long* __restrict__ runs,
                                                               u32* __restrict__ cfirst, int nchrom, long long* __restrict__ info) {
    __shared__ u32 part[SEG_SCAN_THREADS / 64];
    const u32 carry = st_scan_segments<SEG_SCAN_THREADS / 64>(seg, nseg, part);
    for (int c = threadIdx.x; c < nchrom; c += SEG_SCAN_THREADS) {
        cfirst[c] = 0xffffffffu;
        runs[3 * c] = runs[3 * c + 1] = runs[3 * c + 2] = 0;
    }
    if (threadIdx.x == 0) {
        seg[nseg] = carry;
        info[0] = (long long)carry;
        info[1] = carry ? 128 : 0;
        info[2] = 0;
        info[3] = -1;
    }
}

// inclusive maximum-scan of v over the workgroup (`NW` waves); *total = the maximum.  `part` is LDS, NW words.
template <int NW>
__device__ __forceinline__ u32 seg_block_max_scan(u32 v, u32* part, u32* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 up = __shfl_up(inc, o);
        if (lane >= o && up > inc) inc = up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    u32 before = 0, all = 0;
    for (int w = 0; w < NW; ++w) {
        const u32 p = part[w];
        if (w < wave && p > before) before = p;
        if (p > all) all = p;
    }
    __syncthreads();
    *total = all;
    return before > inc ? before : inc;
}

struct SegGlobal {
    const char* p;
    __device__ __forceinline__ u32 operator()(u32 i) const { return (unsigned char)p[i]; }
};
struct SegLds {
    const unsigned char* lds;
    int bias;                                                    // text position of lds[0]; negative when the text starts misaligned
    __device__ __forceinline__ u32 operator()(u32 i) const { return lds[(int)i - bias]; }
};

// A coordinate at text[i, ..): 1 .. 10 digits, no leading zero unless it is "0", a tab behind it.  -> i behind the tab.
template <class Rd>
__device__ __forceinline__ bool seg_coordinate(const Rd& rd, u32& i, u32 e, u64* val) {
    const u32 b = i;
    u64 v = 0;
    while (i < e && i - b < 11u) {
        const u32 d = rd(i) - '0';
        if (d >= 10u) break;
        v = v * 10 + d;
        ++i;
    }
    const u32 nd = i - b;
    if (nd == 0 || nd > 10u) return false;
    if (nd > 1 && rd(b) == '0') return false;
    if (i >= e || rd(i) != '\t') return false;
    ++i;
    *val = v;
    return true;
}

// The line text[b, e).  -> the state as written (1 .. 127), 0 when the line is outside the per-line grammar; *len = the bytes of
// its chromosome field when that is one (1 .. 79 bytes and a tab behind them), else 0; *sb, *eb = start / W and end / W.
template <class Rd>
__device__ __forceinline__ u32 seg_parse_line(const Rd& rd, u32 b, u32 e, u32 W, u32* len, int* sb, int* eb) {
    *len = 0;
    u32 i = b;
    while (i < e && i - b < (u32)EPG_SEG_NAME_BYTES) {
        const u32 c = rd(i);
        if (c == '\t' || c == '\r') break;
        ++i;
    }
    if (i >= e || rd(i) != '\t' || i == b || i - b >= (u32)EPG_SEG_NAME_BYTES) return 0;
    *len = i - b;
    ++i;
    u64 s = 0, t = 0;
    if (!seg_coordinate(rd, i, e, &s) || !seg_coordinate(rd, i, e, &t)) return 0;
    if (t <= s || s % W || t % W || t / W >= (1ull << 31)) return 0;
    *sb = (int)(s / W);                                          // (the caller drops them when the label is none)
    *eb = (int)(t / W);
    if (i < e && (rd(i) | 0x20u) - 'a' < 26u) ++i;               // one optional letter
    u32 v = 0, nd = 0;
    if (i < e && rd(i) == '0') return 0;
    while (i < e && nd < 3u) {
        const u32 d = rd(i) - '0';
        if (d >= 10u) break;
        v = v * 10 + d;
        ++i, ++nd;
    }
    if (nd == 0 || v > 127u) return 0;
    u32 junk = 0;                                                // behind the number: nothing, or '_' and bytes that end no field
    if (i < e) {
        junk = rd(i) != '_';
        for (++i; i < e; ++i) {
            const u32 c = rd(i);
            junk |= (u32)(c == '\t') | (u32)(c == '\r');
        }
    }
    return junk ? 0 : v;
}

__device__ __forceinline__ void seg_report(long long* info, u32 bad) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 c = __shfl_xor(bad, o);
        bad = c < bad ? c : bad;
    }
    if ((threadIdx.x & 63) == 0 && bad != 0xffffffffu)
        atomicMin(reinterpret_cast<unsigned long long*>(info) + 3, (unsigned long long)bad);     // (-1 is the largest unsigned)
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_parse(const char* __restrict__ text, long n, const char* __restrict__ names,
                                                           int nchrom, u32 W, const u32* __restrict__ nl, const u32* __restrict__ Lp,
                                                           u32 lmax, int32_t* __restrict__ first, int8_t* __restrict__ state, long cap,
                                                           int* __restrict__ startb, int* __restrict__ endb, u32* __restrict__ meta,
                                                           u32* __restrict__ blk, u32* __restrict__ cfirst,
                                                           long long* __restrict__ info) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[SEG_LDS_TEXT + 32];
    __shared__ u32 part[SEG_THREADS / 64];
    const int t = threadIdx.x;
    u32 L = *Lp;
    if (L > lmax) L = lmax;
    const u32 g_lo = blockIdx.x * (u32)SEG_THREADS;
    if (g_lo >= L) {                                             // (workgroup-uniform)
        if (t == 0) blk[blockIdx.x] = 0;
        return;
    }
    u32 g_hi = g_lo + SEG_THREADS;
    if (g_hi > L) g_hi = L;

    // the span of this workgroup's lines, text[sb, se), into LDS when it fits (workgroup-uniform)
    bool staged = false;
    const u32 sb = g_lo ? nl[g_lo - 1] + 1 : 0;
    int mis = 0;
    {
        u32 se = nl[g_hi - 1];
        if ((long)se > n) se = (u32)n;
        const u32 len = se - sb;
        if (len <= (u32)SEG_LDS_TEXT) {
            staged = true;
            const char* src = text + sb;
            mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);  // lds[mis + i] = src[i]
            u32 head = mis ? 16u - (u32)mis : 0u;
            if (head > len) head = len;
            if ((u32)t < head) lds[mis + t] = (unsigned char)src[t];
            const u32 nvec = (len - head) >> 4;
            for (u32 v = t; v < nvec; v += SEG_THREADS)
                *reinterpret_cast<uint4*>(lds + mis + head + 16 * v) = *reinterpret_cast<const uint4*>(src + head + 16 * v);
            for (u32 i = head + 16 * nvec + t; i < len; i += SEG_THREADS) lds[mis + i] = (unsigned char)src[i];
        }
    }
    __syncthreads();

    const u32 l = g_lo + t;
    u32 bad = 0xffffffffu, mark = 0;
    if (l < L) {
        const u32 b = l ? nl[l - 1] + 1 : 0;
        u32 e = nl[l];
        if ((long)e > n) e = (u32)n;
        u32 len = 0;
        int s0 = -1, e0 = -1;
        const u32 v = staged ? seg_parse_line(SegLds{lds, (int)sb - mis}, b, e, W, &len, &s0, &e0)
                             : seg_parse_line(SegGlobal{text}, b, e, W, &len, &s0, &e0);
        if (!v) bad = l, s0 = e0 = -1;
        // the same chromosome as the line before?  (its field is a tab-ended prefix of that line)
        bool same = l > 0 && len > 0;
        if (same) {
            const u32 pb = l > 1 ? nl[l - 2] + 1 : 0, pe = nl[l - 1];
            same = pb + len < pe && text[pb + len] == '\t';
            for (u32 i = 0; same && i < len; ++i) same = text[pb + i] == text[b + i];
        }
        u32 code = 0;
        if (!same) {
            code = 1;
            if (len)
                for (int c = 0; c < nchrom; ++c) {
                    const char* name = names + (long)c * EPG_SEG_NAME_BYTES;
                    bool eq = name[len] == 0;
                    for (u32 i = 0; eq && i < len; ++i) eq = name[i] == text[b + i];
                    if (eq) {
                        code = 2 + (u32)c;
                        atomicMin(cfirst + c, l);
                        break;
                    }
                }
            mark = l + 1;
        }
        meta[l] = (code << 8) | v;
        startb[l] = s0;
        endb[l] = e0;
        if ((long)l < cap) {
            first[l] = s0;
            state[l] = (int8_t)((int)v - 1);
        }
    }
    seg_report(info, bad);
    u32 last;
    seg_block_max_scan<SEG_THREADS / 64>(mark, part, &last);
    if (t == 0) blk[blockIdx.x] = last;
}

// blk[0 .. nblk): the last run start (line + 1, 0: none) of each workgroup's lines -> of its lines and all the lines before them
__global__ __launch_bounds__(SEG_SCAN_THREADS) void k_seg_runs(u32* __restrict__ blk, int nblk) {
    __shared__ u32 part[SEG_SCAN_THREADS / 64];
    u32 carry = 0;
    for (int i0 = 0; i0 < nblk; i0 += SEG_SCAN_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        const u32 v = i < nblk ? blk[i] : 0;
        u32 all;
        const u32 inc = seg_block_max_scan<SEG_SCAN_THREADS / 64>(v, part, &all);
        if (i < nblk) blk[i] = inc > carry ? inc : carry;
        if (all > carry) carry = all;
    }
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_link(const u32* __restrict__ Lp, u32 lmax, long cap, const int* __restrict__ startb,
                                                          const int* __restrict__ endb, const u32* __restrict__ meta,
                                                          const u32* __restrict__ blk, const u32* __restrict__ cfirst,
                                                          long long* __restrict__ runs, long long* __restrict__ info) {
    __shared__ u32 part[SEG_THREADS / 64];
    const int t = threadIdx.x;
    u32 L = *Lp;
    if (L > lmax) L = lmax;
    const u32 g_lo = blockIdx.x * (u32)SEG_THREADS;
    if (g_lo >= L) return;                                       // (workgroup-uniform)
    const u32 l = g_lo + t;
    const bool live = l < L;
    const u32 m = live ? meta[l] : 0;
    const u32 code = m >> 8, v = m & 0xffu;
    u32 all;
    u32 rs1 = seg_block_max_scan<SEG_THREADS / 64>(code ? l + 1 : 0, part, &all);
    const u32 before = blockIdx.x ? blk[blockIdx.x - 1] : 0;
    if (before > rs1) rs1 = before;
    u32 bad = 0xffffffffu, vmin = 128, vmax = 0;
    if (live && rs1) {                                           // (line 0 starts a run: rs1 >= 1 for every line)
        const u32 rs = rs1 - 1;
        const int c = (int)(meta[rs] >> 8) - 2;                  // the run's chromosome of the table, < 0: none
        if (c >= 0) {                                            // (the other chromosomes' lines: the per-line grammar only)
            if (code) {
                if (v && startb[l] != 0) bad = l;
                if (cfirst[c] != l) bad = l;                     // the chromosome's second run
            } else if (startb[l] != endb[l - 1]) {
                bad = l;
            }
        }
        if (c >= 0 && v) vmin = vmax = v;
        const bool ends = l + 1 == L || (meta[l + 1] >> 8) != 0;
        if (ends && c >= 0 && cfirst[c] == rs && (long)l < cap) {
            runs[3 * c] = (long long)rs;
            runs[3 * c + 1] = (long long)(l - rs) + 1;
            runs[3 * c + 2] = (long long)endb[l];
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 a = __shfl_xor(vmin, o), b = __shfl_xor(vmax, o);
        vmin = a < vmin ? a : vmin;
        vmax = b > vmax ? b : vmax;
    }
    if ((t & 63) == 0) {
        unsigned long long* u = reinterpret_cast<unsigned long long*>(info);
        if (vmin < 128u) atomicMin(u + 1, (unsigned long long)vmin);
        if (vmax > 0u) atomicMax(u + 2, (unsigned long long)vmax);
    }
    seg_report(info, bad);
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_expand(const int32_t* __restrict__ first, const int8_t* __restrict__ state,
                                                            const long long* __restrict__ runs, int c, int8_t* __restrict__ col, long R) {
    __shared__ int lf[SEG_TILE];
    __shared__ __attribute__((aligned(16))) unsigned char ls[SEG_TILE];
    const int t = threadIdx.x;
    const long long l0 = runs[3 * c], nlines = runs[3 * c + 1], Rc = runs[3 * c + 2];
    const long lim = R < Rc ? R : (long)Rc;
    const long r0 = (long)blockIdx.x * SEG_TILE;
    if (r0 >= lim || nlines <= 0 || nlines > 0x7fffffffll) return;       // (workgroup-uniform)
    const int nl = (int)nlines;
    const int x0 = (int)r0;                                      // (R_c < 2^31)
    const int x1 = (int)((r0 + SEG_TILE < lim ? r0 + SEG_TILE : lim) - 1);
    const int32_t* f = first + l0;
    // the lines of the tile's first and last bin: a = the entries of f[] that are <= x0, b = those <= x1 (a fixed number of steps)
    int a = 0, b = 0;
    for (int s = 1 << (31 - __clz(nl)); s; s >>= 1) {
        const bool ta = a + s <= nl, tb = b + s <= nl;
        const int fa = ta ? f[a + s - 1] : 0, fb = tb ? f[b + s - 1] : 0;
        if (ta && fa <= x0) a += s;
        if (tb && fb <= x1) b += s;
    }
    const int ja = a > 0 ? a - 1 : 0;
    int cnt = (b > 0 ? b - 1 : 0) - ja + 1;
    if (cnt < 1) cnt = 1;
    if (cnt > SEG_TILE) cnt = SEG_TILE;                          // (lines of the grammar: a bin or more each)
    for (int i = t; i < cnt; i += SEG_THREADS) {
        lf[i] = f[ja + i];
        ls[i] = (unsigned char)state[l0 + ja + i];
    }
    __syncthreads();
    const long r = r0 + 16 * t;
    if (r >= lim) return;
    const int x = (int)r;
    int j = 0;                                                   // the entries of lf[] that are <= x
    for (int s = 1 << (31 - __clz(cnt)); s; s >>= 1)
        if (j + s <= cnt && lf[j + s - 1] <= x) j += s;
    j = j > 0 ? j - 1 : 0;
    u32 w[4];
    if (j + 1 >= cnt || (long)lf[j + 1] >= r + 16) {                   // inside one run: a splat
        w[0] = w[1] = w[2] = w[3] = 0x01010101u * ls[j];
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (j + 1 < cnt && (long)lf[j + 1] <= r + i) ++j;
            w[i >> 2] |= (u32)ls[j] << (8 * (i & 3));
        }
    }
    if (r + 16 <= lim) {
        *reinterpret_cast<uint4*>(col + r) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (r + i < lim) col[r + i] = (int8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// the workspace: seg[nseg + 1] | nl[lines] | startb[lines] | endb[lines] | meta[lines] | blk[line blocks] | cfirst[nchrom]
struct SegWs {
    int64_t nseg, lines, nblk, o_nl, o_start, o_end, o_meta, o_blk, o_cfirst, bytes;
};
static SegWs seg_ws(int64_t nbytes, int nchrom) {
    SegWs w;
    w.nseg = nbytes / SEG_BLOCK + 1;
    w.lines = seg_lines(nbytes);
    w.nblk = (w.lines + SEG_THREADS - 1) / SEG_THREADS;
    w.o_nl = align_up((w.nseg + 1) * 4, 256);
    w.o_start = w.o_nl + align_up(w.lines * 4, 256);
    w.o_end = w.o_start + align_up(w.lines * 4, 256);
    w.o_meta = w.o_end + align_up(w.lines * 4, 256);
    w.o_blk = w.o_meta + align_up(w.lines * 4, 256);
    w.o_cfirst = w.o_blk + align_up(w.nblk * 4, 256);
    w.bytes = w.o_cfirst + align_up((int64_t)nchrom * 4 + 4, 256);
    return w;
}

extern "C" int64_t epg_seg_ws_bytes(int64_t nbytes, int32_t nchrom) {
    if (nbytes < 0 || nbytes > EPG_SEG_MAX_TEXT_BYTES)
        return fail(EPG_ERR_INVALID_ARG, "seg_ws_bytes: %lld bytes outside 0..%lld", (long long)nbytes, (long long)EPG_SEG_MAX_TEXT_BYTES);
    if (nchrom < 0 || nchrom > SEG_MAX_CHROMS)
        return fail(EPG_ERR_INVALID_ARG, "seg_ws_bytes: a table of %d chromosomes outside 0..%d", nchrom, SEG_MAX_CHROMS);
    return seg_ws(nbytes, nchrom).bytes;
}

extern "C" int32_t epg_seg_constant(int32_t which) {
    switch (which) {
        case EPG_SEG_THREAD_BYTES: return SEG_THREAD_BYTES;
        case EPG_SEG_BLOCK_BYTES: return SEG_BLOCK;
        case EPG_SEG_EXPAND_TILE_BINS: return SEG_TILE;
        case EPG_SEG_MAX_CHROMS: return SEG_MAX_CHROMS;
    }
    return -1;
}

extern "C" int epg_seg_parse(const char* text, int64_t nbytes, const char* names, int32_t nchrom, int32_t width, int32_t* first,
                             int8_t* state, int64_t cap, int64_t* runs, int64_t* info, void* ws, int64_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (nbytes < 0 || nbytes > EPG_SEG_MAX_TEXT_BYTES)
        return fail(EPG_ERR_INVALID_ARG, "seg_parse: %lld bytes outside 0..%lld", (long long)nbytes, (long long)EPG_SEG_MAX_TEXT_BYTES);
    if (nchrom < 0 || nchrom > SEG_MAX_CHROMS)
        return fail(EPG_ERR_INVALID_ARG, "seg_parse: a table of %d chromosomes outside 0..%d", nchrom, SEG_MAX_CHROMS);
    if (width <= 0) return fail(EPG_ERR_INVALID_ARG, "seg_parse: a bin width of %d", width);
    if (cap < 0) return fail(EPG_ERR_INVALID_ARG, "seg_parse: room for %lld lines", (long long)cap);
    if ((nbytes > 0 && !text) || !ws || !info) return fail(EPG_ERR_INVALID_ARG, "seg_parse: NULL argument");
    if (nchrom > 0 && (!names || !runs)) return fail(EPG_ERR_INVALID_ARG, "seg_parse: NULL table");
    if (cap > 0 && (!first || !state)) return fail(EPG_ERR_INVALID_ARG, "seg_parse: NULL output");
    if (reinterpret_cast<uintptr_t>(ws) & 15) return fail(EPG_ERR_INVALID_ARG, "seg_parse: the workspace is not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(info) & 7) || (reinterpret_cast<uintptr_t>(runs) & 7))
        return fail(EPG_ERR_INVALID_ARG, "seg_parse: info or runs is not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(first) & 3) return fail(EPG_ERR_INVALID_ARG, "seg_parse: first is not 4-byte aligned");
    const SegWs w = seg_ws(nbytes, nchrom);
    if (ws_bytes < w.bytes)
        return fail(EPG_ERR_WORKSPACE, "seg_parse: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)w.bytes);
    char* base = reinterpret_cast<char*>(ws);
    u32* seg = reinterpret_cast<u32*>(base);
    u32* nl = reinterpret_cast<u32*>(base + w.o_nl);
    int* startb = reinterpret_cast<int*>(base + w.o_start);
    int* endb = reinterpret_cast<int*>(base + w.o_end);
    u32* meta = reinterpret_cast<u32*>(base + w.o_meta);
    u32* blk = reinterpret_cast<u32*>(base + w.o_blk);
    u32* cfirst = reinterpret_cast<u32*>(base + w.o_cfirst);
    long long* inf = reinterpret_cast<long long*>(info);
    long long* rn = reinterpret_cast<long long*>(runs);
    const int nseg = (int)w.nseg, nblk = (int)w.nblk;
    const u32 lmax = (u32)w.lines;
    hipLaunchKernelGGL(k_seg_index<false>, dim3((unsigned)nseg), dim3(SEG_THREADS), 0, st, text, (long)nbytes, seg, nl, lmax);
    EPG_LAUNCH_CHECK("k_seg_index<count>");
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(SEG_SCAN_THREADS), 0, st, seg, nseg, rn, cfirst, (int)nchrom, inf);
    EPG_LAUNCH_CHECK("k_seg_scan");
    hipLaunchKernelGGL(k_seg_index<true>, dim3((unsigned)nseg), dim3(SEG_THREADS), 0, st, text, (long)nbytes, seg, nl, lmax);
    EPG_LAUNCH_CHECK("k_seg_index<fill>");
    hipLaunchKernelGGL(k_seg_parse, dim3((unsigned)nblk), dim3(SEG_THREADS), 0, st, text, (long)nbytes, names, (int)nchrom, (u32)width,
                       (const u32*)nl, (const u32*)(seg + nseg), lmax, first, state, (long)cap, startb, endb, meta, blk, cfirst, inf);
    EPG_LAUNCH_CHECK("k_seg_parse");
    hipLaunchKernelGGL(k_seg_runs, dim3(1), dim3(SEG_SCAN_THREADS), 0, st, blk, nblk);
    EPG_LAUNCH_CHECK("k_seg_runs");
    hipLaunchKernelGGL(k_seg_link, dim3((unsigned)nblk), dim3(SEG_THREADS), 0, st, (const u32*)(seg + nseg), lmax, (long)cap,
                       (const int*)startb, (const int*)endb, (const u32*)meta, (const u32*)blk, (const u32*)cfirst, rn, inf);
    EPG_LAUNCH_CHECK("k_seg_link");
    return EPG_OK;
}

extern "C" int epg_seg_expand(const int32_t* first, const int8_t* state, const int64_t* runs, int32_t c, int8_t* col, int64_t R,
                              void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (c < 0 || c >= SEG_MAX_CHROMS) return fail(EPG_ERR_INVALID_ARG, "seg_expand: chromosome %d outside 0..%d", c, SEG_MAX_CHROMS - 1);
    if (R < 0 || R > 0x7fffffffll) return fail(EPG_ERR_INVALID_ARG, "seg_expand: a column of %lld bins", (long long)R);
    if (R == 0) return EPG_OK;
    if (!first || !state || !runs || !col) return fail(EPG_ERR_INVALID_ARG, "seg_expand: NULL argument");
    if (reinterpret_cast<uintptr_t>(col) & 15) return fail(EPG_ERR_INVALID_ARG, "seg_expand: the column is not 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(first) & 3) || (reinterpret_cast<uintptr_t>(runs) & 7))
        return fail(EPG_ERR_INVALID_ARG, "seg_expand: first or runs is not aligned");
    hipLaunchKernelGGL(k_seg_expand, dim3((unsigned)((R + SEG_TILE - 1) / SEG_TILE)), dim3(SEG_THREADS), 0, st, first, state,
                       reinterpret_cast<const long long*>(runs), (int)c, col, (long)R);
    EPG_LAUNCH_CHECK("k_seg_expand");
    return EPG_OK;
}

}  // namespace epg
