// One BGZF block of the device text writer (epg_textout.hip), as per-thread phases in plain C++: the kernels call the phases with
// workgroup barriers between them, tests/bgzf_block_check.cpp calls them thread by thread on the host and inflates the result with
// zlib.  A block is at most BG_TEXT bytes of text and BG_T threads work on it.
//
// Tokens.  The rows of the text are dealt to the threads in order, whole rows each (the block's first and last row may be cut by
// the block's borders).  A thread walks its rows byte by byte; at a position p of row r it compares with p - d, d = the length of
// row r - 1 ("the same column one row earlier"): BG_MINM or more equal bytes (at most 258, never past the row's end, never reaching
// before the block's start) are a match of distance d, anything else a literal.  The walk is deterministic, so it is simply done
// three times: for the histogram, for the threads' bit counts, and to emit.
// Code.  One thread builds the literal/length and distance codes from the histogram (two-queue Huffman over the sorted used symbols,
// lengths cut to 15 bits by moving leaves down until Kraft's sum is 1 again), the code-length code (7 bits) over the lengths with
// runs of zeros coded as 17 / 18, and the block header's bits.  A tree with fewer than two used symbols gets two codes of one bit,
// as zlib does: every inflater accepts a complete code.
// CRC-32.  Every thread takes a fixed slice of BG_T-th of the block through the byte table, advances its value over the bytes behind
// the slice (multiplication by x^(8 L) modulo the polynomial, square and multiply) and the block's value is the XOR of all.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BG_FN __host__ __device__ inline
#else
#define BG_FN inline
#endif

namespace epgbg {

typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t u8;
typedef unsigned long long u64;

constexpr int BG_TEXT = 65280;                               // text bytes per block (BGZF's own limit)
constexpr int BG_T = 256;                                    // threads per block
constexpr int BG_SLICE = BG_TEXT / BG_T;                     // 255: a thread's CRC slice
constexpr int BG_MINM = 6;                                   // shortest match worth its ~17 bits
constexpr int BG_NLL = 288, BG_NSYM = 320;                   // literal/length symbols 0 .. 287, distance symbols at 288 .. 319
constexpr int BG_HDR_WORDS = 80;                             // the header's bits: at most 17 + 57 + 316 * 7
constexpr u32 BG_POLY = 0xedb88320u;
constexpr int BG_MEMBER_EXTRA = 18 + 8;                      // gzip header with the BC subfield, CRC-32 and ISIZE
constexpr int BG_VROW = 256;                                 // without row offsets: pieces of this many bytes, no matches

BG_FN void atom_add(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BG_FN void atom_or(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
BG_FN void atom_xor(u32* p, u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicXor(p, v);
#else
    *p ^= v;
#endif
}
BG_FN int ilog2(u32 v) {                                     // v >= 1
    int n = 0;
    while (v >>= 1) ++n;
    return n;
}
BG_FN u32 bit_reverse(u32 c, int len) {
    u32 r = 0;
    for (int i = 0; i < len; ++i) r |= ((c >> i) & 1u) << (len - 1 - i);
    return r;
}

// what a block's record in the workspace keeps between the planning and the emitting kernel
struct Rec {
    u32 size, stored, crc, hdr_bits, eob_pos, deflate_bytes, n_text, pad;
    long long ra, nr;                                        // the block's rows: ra .. ra + nr - 1
    u32 tbits[BG_T];                                         // bit offset of every thread's tokens inside the DEFLATE stream
    u32 hdr[BG_HDR_WORDS];
    u16 code[BG_NSYM];
    u8 len[BG_NSYM];
};

// the row offsets as the block sees them: clamped into [0, n], row 0 at 0 and row R at n whatever the array says
struct Rows {
    const long long* off;
    long long R, n;
    BG_FN long long at(long long r) const {
        if (r <= 0) return 0;
        if (r >= R) return n;
        if (!off) return r * BG_VROW;
        const long long v = off[r];
        return v < 0 ? 0 : (v > n ? n : v);
    }
};
BG_FN Rows make_rows(const long long* off, long long R, long long n) {
    Rows rw;
    rw.off = R > 0 ? off : nullptr;
    rw.R = rw.off ? R : (n + BG_VROW - 1) / BG_VROW;
    rw.n = n;
    return rw;
}

// a block's shared state: LDS on the device
struct Shared {
    u32 hist[BG_NSYM];
    u32 crctab[256];
    u32 crc, bad, hdr_bits;
    long long ra, nr;
    u32 hdr[BG_HDR_WORDS];
    u16 code[BG_NSYM];
    u8 len[BG_NSYM];
    // the code builder's scratch (one thread)
    u32 w[BG_NLL], iw[BG_NLL];
    u16 sym[BG_NLL], lpar[BG_NLL], ipar[BG_NLL], idep[BG_NLL];
    u32 cnt[20], next[20], clfreq[20];
    u16 clcode[20];
    u8 cllen[20];
    u8 tsym[BG_NSYM], textra[BG_NSYM];
};

// ---- symbols ----------------------------------------------------------------------------------------------------------------------
BG_FN void len_symbol(int L, int& sym, int& ebits, u32& eval) {          // 3 <= L <= 258
    ebits = 0;
    eval = 0;
    if (L == 258) { sym = 285; return; }
    const u32 l = (u32)(L - 3);
    if (l < 8) { sym = 257 + (int)l; return; }
    const int nb = ilog2(l) - 2;
    sym = 261 + 4 * nb + (int)((l >> nb) & 3u);
    ebits = nb;
    eval = l & ((1u << nb) - 1u);
}
BG_FN void dist_symbol(int d, int& sym, int& ebits, u32& eval) {         // 1 <= d <= 32768
    ebits = 0;
    eval = 0;
    const u32 dd = (u32)(d - 1);
    if (dd < 4) { sym = (int)dd; return; }
    const int nb = ilog2(dd) - 1;
    sym = 2 * nb + 2 + (int)((dd >> nb) & 1u);
    ebits = nb;
    eval = dd & ((1u << nb) - 1u);
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------
// thread t's rows [f, l) and bytes [lo, hi) of the block [B0, B1) whose rows are ra .. ra + nr - 1
BG_FN void thread_span(const Rows& rw, long long ra, long long nr, long long B0, long long B1, int t, long long& f, long long& l, long long& lo,
                       long long& hi) {
    f = ra + (long long)t * nr / BG_T;
    l = ra + (long long)(t + 1) * nr / BG_T;
    lo = rw.at(f);
    hi = rw.at(l);
    if (t == 0 || lo < B0) lo = B0;
    if (t == BG_T - 1 || hi > B1) hi = B1;
    if (lo > B1) lo = B1;
    if (hi < lo) hi = lo;
}

// tok.lit(byte) / tok.match(length, distance) for every token of thread t, in text order; -> false when the rows are not in order
template <typename TOK>
BG_FN bool walk(const unsigned char* text, const Rows& rw, long long ra, long long nr, long long B0, long long B1, int t, TOK& tok) {
    long long f, l, lo, hi;
    thread_span(rw, ra, nr, B0, B1, t, f, l, lo, hi);
    bool ok = true;
    for (long long r = f; r < l; ++r) {
        const long long a = rw.at(r), b = rw.at(r + 1);
        if (b < a) ok = false;
        const long long s = a < lo ? lo : a, e = b > hi ? hi : b;
        const long long d = r > 0 ? a - rw.at(r - 1) : 0;
        const bool try_match = rw.off != nullptr && d >= 1 && d <= 32768;
        long long p = s;
        while (p < e) {
            int L = 0;
            if (try_match && p - d >= B0) {
                const long long room = e - p;
                const int maxL = room < 258 ? (int)room : 258;
                while (L < maxL && text[p + L] == text[p + L - d]) ++L;
            }
            if (L >= BG_MINM) {
                tok.match(L, (int)d);
                p += L;
            } else {
                tok.lit(text[p]);
                ++p;
            }
        }
    }
    return ok;
}

struct TokHist {
    u32* hist;
    BG_FN void lit(unsigned char c) { atom_add(hist + c, 1u); }
    BG_FN void match(int L, int d) {
        int s, eb;
        u32 ev;
        len_symbol(L, s, eb, ev);
        atom_add(hist + s, 1u);
        dist_symbol(d, s, eb, ev);
        atom_add(hist + BG_NLL + s, 1u);
    }
};
struct TokBits {
    const u8* len;
    u32 bits;
    BG_FN void lit(unsigned char c) { bits += len[c]; }
    BG_FN void match(int L, int d) {
        int s, eb;
        u32 ev;
        len_symbol(L, s, eb, ev);
        bits += (u32)len[s] + (u32)eb;
        dist_symbol(d, s, eb, ev);
        bits += (u32)len[BG_NLL + s] + (u32)eb;
    }
};
// bits into zeroed words shared with other threads: whole words and the two ragged ends alike by atomic OR
struct BitWriter {
    u32* words;
    u64 acc;
    int n;
    u32 word;
    BG_FN void start(u32* w, u32 bitpos) {
        words = w;
        acc = 0;
        n = (int)(bitpos & 31u);
        word = bitpos >> 5;
    }
    BG_FN void put(u32 v, int nb) {                          // nb <= 16
        acc |= (u64)v << n;
        n += nb;
        if (n >= 32) {
            atom_or(words + word, (u32)acc);
            ++word;
            acc >>= 32;
            n -= 32;
        }
    }
    BG_FN void finish() {
        if (n > 0) atom_or(words + word, (u32)acc);
    }
};
struct TokEmit {
    const u16* code;
    const u8* len;
    BitWriter bw;
    BG_FN void lit(unsigned char c) { bw.put(code[c], len[c]); }
    BG_FN void match(int L, int d) {
        int s, eb;
        u32 ev;
        len_symbol(L, s, eb, ev);
        bw.put(code[s], len[s]);
        if (eb) bw.put(ev, eb);
        dist_symbol(d, s, eb, ev);
        bw.put(code[BG_NLL + s], len[BG_NLL + s]);
        if (eb) bw.put(ev, eb);
    }
};
// nb <= 32 bits at any bit position of zeroed shared words
BG_FN void put_at(u32* words, u32 bitpos, u32 v, int nb) {
    const u64 x = (u64)(nb < 32 ? (v & ((1u << nb) - 1u)) : v) << (bitpos & 31u);
    atom_or(words + (bitpos >> 5), (u32)x);
    if ((x >> 32) != 0) atom_or(words + (bitpos >> 5) + 1, (u32)(x >> 32));
}

// ---- CRC-32 -----------------------------------------------------------------------------------------------------------------------
BG_FN u32 crc_table_entry(u32 i) {
    u32 c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (BG_POLY ^ (c >> 1)) : (c >> 1);
    return c;
}
// a(x) * b(x) modulo the polynomial, bit-reflected operands (bit 31 is x^0)
BG_FN u32 crc_mulmod(u32 a, u32 b) {
    u32 p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? ((b >> 1) ^ BG_POLY) : (b >> 1);
    }
    return p;
}
// the CRC-32 of `crc`'s message followed by L zero bytes' worth of shifting: what combines slices, crc(A B) = advance(crc(A), |B|) ^ crc(B)
BG_FN u32 crc_advance(u32 crc, u32 L) {
    u32 p = 0x80000000u, sq = 0x00800000u;                   // x^0 and x^8
    for (; L; L >>= 1) {
        if (L & 1u) p = crc_mulmod(sq, p);
        sq = crc_mulmod(sq, sq);
    }
    return crc_mulmod(p, crc);
}
BG_FN u32 crc_slice(const u32* tab, const unsigned char* p, long long n) {
    u32 c = 0xffffffffu;
    for (long long i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}

// ---- the code builder (one thread) ------------------------------------------------------------------------------------------------
// len[0 .. n) = code lengths <= maxlen of a complete prefix code for the symbols with freq != 0 (at least two symbols get a code)
BG_FN void build_lengths(Shared& sh, const u32* freq, int n, int maxlen, u8* len) {
    int nu = 0;
    for (int i = 0; i < n; ++i) {
        len[i] = 0;
        if (!freq[i]) continue;
        int k = nu++;
        const u32 f = freq[i];
        while (k > 0 && sh.w[k - 1] > f) {                  // ascending by (frequency, symbol)
            sh.w[k] = sh.w[k - 1];
            sh.sym[k] = sh.sym[k - 1];
            --k;
        }
        sh.w[k] = f;
        sh.sym[k] = (u16)i;
    }
    if (nu == 0) { len[0] = len[1] = 1; return; }
    if (nu == 1) { len[sh.sym[0]] = 1; len[sh.sym[0] == 0 ? 1 : 0] = 1; return; }
    int i = 0, j = 0;
    for (int k = 0; k < nu - 1; ++k) {                      // two queues: the sorted leaves and the internal nodes in order of creation
        u32 sum = 0;
        for (int rep = 0; rep < 2; ++rep) {
            if (i < nu && (j >= k || sh.w[i] <= sh.iw[j])) { sum += sh.w[i]; sh.lpar[i] = (u16)k; ++i; }
            else { sum += sh.iw[j]; sh.ipar[j] = (u16)k; ++j; }
        }
        sh.iw[k] = sum;
    }
    sh.idep[nu - 2] = 0;
    for (int k = nu - 3; k >= 0; --k) sh.idep[k] = (u16)(sh.idep[sh.ipar[k]] + 1);
    for (int l = 0; l <= maxlen; ++l) sh.cnt[l] = 0;
    for (int k = 0; k < nu; ++k) {
        const int d = sh.idep[sh.lpar[k]] + 1;
        sh.cnt[d < maxlen ? d : maxlen]++;
    }
    u32 total = 0;
    for (int l = maxlen; l >= 1; --l) total += sh.cnt[l] << (maxlen - l);
    while (total != (1u << maxlen)) {                       // over-subscribed by the cut: a leaf of the deepest level moves below a shallower one
        sh.cnt[maxlen]--;
        for (int l = maxlen - 1; l >= 1; --l)
            if (sh.cnt[l]) { sh.cnt[l]--; sh.cnt[l + 1] += 2; break; }
        --total;
    }
    int idx = 0;
    for (int l = maxlen; l >= 1; --l)                       // the rarest symbols take the longest codes
        for (u32 c = 0; c < sh.cnt[l]; ++c) len[sh.sym[idx++]] = (u8)l;
}

// canonical codes of the lengths, bit-reversed as DEFLATE packs them
BG_FN void build_codes(Shared& sh, const u8* len, int n, u16* code) {
    for (int b = 0; b <= 16; ++b) sh.cnt[b] = 0;
    for (int i = 0; i < n; ++i) sh.cnt[len[i]]++;
    sh.cnt[0] = 0;
    u32 c = 0;
    for (int b = 1; b <= 15; ++b) {
        c = (c + sh.cnt[b - 1]) << 1;
        sh.next[b] = c;
    }
    for (int i = 0; i < n; ++i) code[i] = len[i] ? (u16)bit_reverse(sh.next[len[i]]++, len[i]) : (u16)0;
}

struct HdrBits {
    u32* words;
    u32 pos;
    BG_FN void put(u32 v, int nb) {
        const u64 x = (u64)v << (pos & 31u);
        words[pos >> 5] |= (u32)x;
        if ((x >> 32) != 0) words[(pos >> 5) + 1] |= (u32)(x >> 32);
        pos += (u32)nb;
    }
};

// from sh.hist (with the end-of-block symbol counted): sh.len, sh.code, sh.hdr, sh.hdr_bits
BG_FN void build_block_code(Shared& sh) {
    const u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 286; i < BG_NLL; ++i) sh.hist[i] = 0;
    for (int i = BG_NLL + 30; i < BG_NSYM; ++i) sh.hist[i] = 0;
    build_lengths(sh, sh.hist, 286, 15, sh.len);
    sh.len[286] = sh.len[287] = 0;
    build_lengths(sh, sh.hist + BG_NLL, 30, 15, sh.len + BG_NLL);
    sh.len[BG_NLL + 30] = sh.len[BG_NLL + 31] = 0;
    build_codes(sh, sh.len, 286, sh.code);
    build_codes(sh, sh.len + BG_NLL, 30, sh.code + BG_NLL);
    int hlit = 286, hdist = 30;
    while (hlit > 257 && sh.len[hlit - 1] == 0) --hlit;
    while (hdist > 1 && sh.len[BG_NLL + hdist - 1] == 0) --hdist;
    const int nseq = hlit + hdist;
    int nt = 0;
    for (int k = 0; k < 19; ++k) sh.clfreq[k] = 0;
    for (int i = 0; i < nseq;) {
        const int v = i < hlit ? sh.len[i] : sh.len[BG_NLL + i - hlit];
        int run = 1;
        if (v == 0) {
            while (i + run < nseq && run < 138 && (i + run < hlit ? sh.len[i + run] : sh.len[BG_NLL + i + run - hlit]) == 0) ++run;
            if (run >= 11) { sh.tsym[nt] = 18; sh.textra[nt++] = (u8)(run - 11); sh.clfreq[18]++; }
            else if (run >= 3) { sh.tsym[nt] = 17; sh.textra[nt++] = (u8)(run - 3); sh.clfreq[17]++; }
            else {
                for (int k = 0; k < run; ++k) { sh.tsym[nt] = 0; sh.textra[nt++] = 0; sh.clfreq[0]++; }
            }
        } else {
            sh.tsym[nt] = (u8)v;
            sh.textra[nt++] = 0;
            sh.clfreq[v]++;
        }
        i += run;
    }
    build_lengths(sh, sh.clfreq, 19, 7, sh.cllen);
    build_codes(sh, sh.cllen, 19, sh.clcode);
    int hclen = 19;
    while (hclen > 4 && sh.cllen[order[hclen - 1]] == 0) --hclen;
    for (int k = 0; k < BG_HDR_WORDS; ++k) sh.hdr[k] = 0;
    HdrBits hb = {sh.hdr, 0};
    hb.put(1, 1);                                           // BFINAL
    hb.put(2, 2);                                           // dynamic Huffman
    hb.put((u32)(hlit - 257), 5);
    hb.put((u32)(hdist - 1), 5);
    hb.put((u32)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) hb.put(sh.cllen[order[k]], 3);
    for (int k = 0; k < nt; ++k) {
        const int s = sh.tsym[k];
        hb.put(sh.clcode[s], sh.cllen[s]);
        if (s == 17) hb.put(sh.textra[k], 3);
        if (s == 18) hb.put(sh.textra[k], 7);
    }
    sh.hdr_bits = hb.pos;
}

// ---- the planning phases ----------------------------------------------------------------------------------------------------------
BG_FN void plan_init(Shared& sh, int t) {
    for (int i = t; i < BG_NSYM; i += BG_T) sh.hist[i] = 0;
    sh.crctab[t] = crc_table_entry((u32)t);
    if (t == 0) { sh.crc = 0; sh.bad = 0; sh.hdr_bits = 0; }
}
// one thread: the block's rows
BG_FN void plan_rows(Shared& sh, const Rows& rw, long long B0, long long B1) {
    long long lo = 0, hi = rw.R - 1;
    while (lo < hi) {                                        // the last row that starts at or before B0
        const long long mid = lo + (hi - lo + 1) / 2;
        if (rw.at(mid) <= B0) lo = mid;
        else hi = mid - 1;
    }
    const long long ra = lo;
    hi = rw.R - 1;
    while (lo < hi) {                                        // the last row that starts before B1
        const long long mid = lo + (hi - lo + 1) / 2;
        if (rw.at(mid) < B1) lo = mid;
        else hi = mid - 1;
    }
    sh.ra = ra;
    sh.nr = lo - ra + 1;
    if (rw.at(ra) > B0 || rw.at(lo + 1) < B1) sh.bad = 1;
}
BG_FN void plan_hist(Shared& sh, const unsigned char* text, const Rows& rw, long long B0, long long B1, int t) {
    TokHist th = {sh.hist};
    if (!walk(text, rw, sh.ra, sh.nr, B0, B1, t, th)) atom_or(&sh.bad, 1u);
    const long long c0 = B0 + (long long)t * BG_SLICE;
    if (c0 < B1) {
        const long long c1 = c0 + BG_SLICE < B1 ? c0 + BG_SLICE : B1;
        atom_xor(&sh.crc, crc_advance(crc_slice(sh.crctab, text + c0, c1 - c0), (u32)(B1 - c1)));
    }
}
BG_FN u32 plan_bits(const Shared& sh, const unsigned char* text, const Rows& rw, long long B0, long long B1, int t) {
    TokBits tb = {sh.len, 0};
    walk(text, rw, sh.ra, sh.nr, B0, B1, t, tb);
    return tb.bits;
}
// one thread, after the scan: total = all threads' bits
BG_FN void plan_finish(const Shared& sh, Rec& rec, u32 total, long long B0, long long B1) {
    const u32 n = (u32)(B1 - B0);
    const u32 bits = sh.hdr_bits + total + sh.len[256];
    const u32 bytes = (bits + 7u) >> 3;
    rec.stored = (sh.bad || bytes >= n + 5u) ? 1u : 0u;
    rec.deflate_bytes = rec.stored ? n + 5u : bytes;
    rec.size = BG_MEMBER_EXTRA + rec.deflate_bytes;
    rec.crc = sh.crc;
    rec.hdr_bits = sh.hdr_bits;
    rec.eob_pos = sh.hdr_bits + total;
    rec.n_text = n;
    rec.pad = 0;
    rec.ra = sh.ra;
    rec.nr = sh.nr;
}

// ---- the emitting phases: `words` is the zeroed staging area, `a` the byte at which the member starts in it -------------------------
BG_FN void emit_frame(u32* words, u32 a, const Rec& rec, int t) {
    if (t == 0) {
        const u8 h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int i = 0; i < 16; ++i) put_at(words, 8u * (a + (u32)i), h[i], 8);
        put_at(words, 8u * (a + 16u), rec.size - 1u, 16);
        const u32 tail = a + 18u + rec.deflate_bytes;
        put_at(words, 8u * tail, rec.crc, 32);
        put_at(words, 8u * (tail + 4u), rec.n_text, 32);
        if (rec.stored) {
            put_at(words, 8u * (a + 18u), 1u, 8);            // BFINAL, stored
            put_at(words, 8u * (a + 19u), rec.n_text, 16);
            put_at(words, 8u * (a + 21u), ~rec.n_text & 0xffffu, 16);
        } else {
            put_at(words, 8u * (a + 18u) + rec.eob_pos, rec.code[256], rec.len[256]);
        }
    }
    if (!rec.stored) {
        for (int k = t; k < BG_HDR_WORDS; k += BG_T) {
            const int left = (int)rec.hdr_bits - 32 * k;
            if (left > 0) put_at(words, 8u * (a + 18u) + 32u * (u32)k, rec.hdr[k], left < 32 ? left : 32);
        }
    }
}
BG_FN void emit_tokens(u32* words, u32 a, const Rec& rec, const u16* code, const u8* len, const unsigned char* text, const Rows& rw,
                       long long B0, long long B1, int t) {
    TokEmit te;
    te.code = code;
    te.len = len;
    te.bw.start(words, 8u * (a + 18u) + rec.tbits[t]);
    walk(text, rw, rec.ra, rec.nr, B0, B1, t, te);
    te.bw.finish();
}

}  // namespace epgbg
