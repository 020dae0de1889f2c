// One BGZF member inflated (csrc/epg_bgzf_inflate.hip), as per-thread phases in plain C++: the kernel calls the phases with workgroup
// barriers between them, tests/bgzf_inflate_check.cpp calls them thread by thread on the host and holds every verdict against zlib.
// A member is at most BI_WIN bytes of text and the BI_T threads of ONE wave work on it.
//
// The structure.  The member's text is put together in a window of LDS (`win`, the whole member: a match only ever reads the window) and
// goes out to global memory once, in 16-byte stores, after its CRC-32 and size were held against the trailer.  The payload comes in
// through a ring of BI_IN bytes that all threads refill (inflate_refill).  Thread 0 alone walks the bits (inflate_decode): block
// headers, the code tables, the symbols.  It stores literals into the window itself and leaves every copy -- a match, or the bytes of a
// stored block -- as a token; when BI_NTOK tokens wait, when the ring runs low or when the stream ends it returns, and all threads
// perform the tokens one after the other (inflate_copy), byte i of a match by thread i % BI_T.  Byte i of a match of distance d reads
// win[dst - d + i % d], which lies before dst: the bytes of ONE token never depend on each other, however the match overlaps itself
// (distance 1, length 258), so a token is one step of all threads, and the barrier between two tokens orders a match behind whatever
// an earlier token or literal wrote.
// Codes.  A table of BI_LROOT (literal/length) or BI_DROOT (distance) bits answers every code that is not longer than the root with
// one load; a longer code (up to 15 bits) -- and a bit pattern that no code has -- goes through the canonical decode by counts
// (first code and number of codes of every length).
//
// Every loop is bounded by the inputs.  The bit position only moves forward and every read is held against the payload's end before
// its value is used (bytes behind the end read as zero from the ring, never from memory); the output position is held against
// ISIZE before every write; loops over code lengths run to HLIT + HDIST.  `steps` counts every turn of thread 0 that consumes bits
// (a block header, a code length, a symbol, a bit of the canonical decode): each consumes at least one bit of its own, except the
// at most 15 turns of the one canonical decode that finds no code, so steps <= 8 * payload bytes + 16.  Tokens and literals write
// every byte of the text once: isize writes.  The table builders run once per block header in a time that depends on nothing but
// the format's constants.  BI_STEP_SLACK is the constant of the bound 8 * payload_bytes + isize + BI_STEP_SLACK that
// tests/bgzf_inflate_check.cpp asserts for steps + bytes written; the kernel's phase loop is cut off at the same bound.
// Nothing is trusted: whatever the payload holds, the member ends with one of the reason codes below, and no phase reads outside
// [payload, payload + payload_bytes) or writes outside the window's first isize bytes.
#pragma once
#include "epg_bgzf_block.h"

namespace epgbi {

using epgbg::u16;
using epgbg::u32;
using epgbg::u64;
using epgbg::u8;

constexpr int BI_T = 64;                                     // threads per member: one wave
constexpr int BI_WIN = 65536;                                // the largest ISIZE
constexpr int BI_IN = 4096;                                  // the payload ring (a power of two)
constexpr int BI_HDR_BYTES = 576;                            // a dynamic block's header: at most 17 + 57 + 316 * 14 bits = 563 bytes
constexpr int BI_SYM_BYTES = 16;                             // a length and a distance with their extra bits: at most 48 bits
constexpr int BI_NTOK = 32;                                  // tokens per turn
constexpr int BI_LROOT = 10, BI_DROOT = 8, BI_CROOT = 7;
constexpr int BI_STEP_SLACK = 64;

// a member's status: 0 or why it was given up
enum Reason {
    BI_OK = 0,
    BI_E_ROW = 1,            // the table's row: payload outside comp, output outside out, ISIZE above 65 536, a CRC beyond 32 bits
    BI_E_BTYPE = 2,          // block type 3
    BI_E_STORED_LEN = 3,     // a stored block whose LEN and NLEN are not complements
    BI_E_OVERSUBSCRIBED = 4, // a code with more codes than its lengths allow
    BI_E_INCOMPLETE = 5,     // an incomplete code, other than no distance code at all and the single code of one bit
    BI_E_REPEAT_FIRST = 6,   // repeat symbol 16 with no length before it
    BI_E_REPEAT_RUN = 7,     // a run of lengths past HLIT + HDIST
    BI_E_LITLEN_SYM = 8,     // literal/length symbol 286 or 287
    BI_E_DIST_SYM = 9,       // distance symbol 30 or 31
    BI_E_DIST_FAR = 10,      // a distance that reaches before the member's first byte
    BI_E_OUTPUT = 11,        // output beyond ISIZE
    BI_E_BITS = 12,          // bits past the payload
    BI_E_CRC = 13,           // the text's CRC-32 is not the trailer's
    BI_E_ISIZE = 14,         // the stream ends with fewer bytes than ISIZE
    BI_E_CODE = 15,          // bits that are no code of the block's (an incomplete code's unused pattern, a distance where there is no distance code)
    BI_E_HEADER = 16,        // HLIT above 286, HDIST above 30, or no code for the end-of-block symbol
    BI_E_TRAILING = 17,      // the stream ends before the payload's last byte
    BI_REASONS = 18
};

enum { BI_ST_HEADER = 0, BI_ST_CODES = 1, BI_ST_DONE = 2 };
enum { BI_KIND_CODELEN = 0, BI_KIND_LITLEN = 1, BI_KIND_DIST = 2 };

// a member's shared state: LDS on the device
struct Shared {
    alignas(16) u32 win4[(BI_WIN + 32) / 4];                 // the text, `a` bytes in: 16-byte chunks of it are 16-byte chunks of `out`
    u32 in4[BI_IN / 4];                                      // payload byte p at byte p % BI_IN
    u32 crctab[256];
    u16 lroot[1 << BI_LROOT], droot[1 << BI_DROOT], croot[1 << BI_CROOT];        // (symbol << 4) | length, 0 = not in the root
    u16 lsym[288], dsym[32], csym[32];                       // symbols in canonical order
    u16 lcnt[16], dcnt[16], ccnt[16];                        // codes per length
    u16 offs[16], next[16];                                  // the builders' scratch
    u8 lens[320], cl[32];
    u32 tok_dst[BI_NTOK], tok_len[BI_NTOK], tok_from[BI_NTOK];                   // tok_from: the distance, or 0x80000000 | payload offset
    u32 bitpos, end_bits, payload_bytes, in_hi, out_pos, isize, a;
    u32 state, last, status, ntok, crc, steps, phases;
};

BG_FN u8* window(Shared& sh) { return reinterpret_cast<u8*>(sh.win4) + sh.a; }

// ---- the set-up and the ring (all threads) ----------------------------------------------------------------------------------------
BG_FN void inflate_init(Shared& sh, u32 payload_bytes, u32 isize, u32 a, int t) {
    for (int i = t; i < 256; i += BI_T) sh.crctab[i] = epgbg::crc_table_entry((u32)i);
    if (t == 0) {
        sh.bitpos = 0;
        sh.end_bits = 8u * payload_bytes;
        sh.payload_bytes = payload_bytes;
        sh.in_hi = 0;
        sh.out_pos = 0;
        sh.isize = isize;
        sh.a = a & 15u;
        sh.state = BI_ST_HEADER;
        sh.last = 0;
        sh.status = BI_OK;
        sh.ntok = 0;
        sh.crc = 0;
        sh.steps = 0;
        sh.phases = 0;
    }
}
// the ring's end after this refill: BI_IN bytes from the byte the bits stand in
BG_FN u32 refill_end(const Shared& sh) { return (sh.bitpos >> 3) + (u32)BI_IN; }
// payload bytes [max(in_hi, byte position), refill_end) into the ring, zeros behind the payload's end
BG_FN void inflate_refill(Shared& sh, const u8* payload, int t) {
    const u32 at = sh.bitpos >> 3, hi = refill_end(sh);
    const u32 lo = sh.in_hi > at ? sh.in_hi : at;
    u8* ring = reinterpret_cast<u8*>(sh.in4);
    for (u32 p = lo + (u32)t; p < hi; p += BI_T) ring[p & (BI_IN - 1)] = p < sh.payload_bytes ? payload[p] : (u8)0;
}
// one thread, after all threads' refill
BG_FN void inflate_refilled(Shared& sh) { sh.in_hi = refill_end(sh); }

// ---- bits (thread 0) --------------------------------------------------------------------------------------------------------------
// what thread 0 keeps in registers during a turn (Shared is LDS: every field of it read in the symbol loop would be a round trip)
struct Cursor {
    u32 bitpos, end_bits, out_pos, isize, steps, ntok;
};
BG_FN void cursor_load(const Shared& sh, Cursor& c) {
    c.bitpos = sh.bitpos;
    c.end_bits = sh.end_bits;
    c.out_pos = sh.out_pos;
    c.isize = sh.isize;
    c.steps = sh.steps;
    c.ntok = 0;
}
BG_FN void cursor_store(Shared& sh, const Cursor& c) {
    sh.bitpos = c.bitpos;
    sh.out_pos = c.out_pos;
    sh.steps = c.steps;
    sh.ntok = c.ntok;
}
// the 32 bits from the bit position on; the ring holds them when in_hi - byte position >= 8
BG_FN u32 peek(const Shared& sh, const Cursor& c) {
    const u32 w = c.bitpos >> 5, m = BI_IN / 4 - 1;
    const u64 x = ((u64)sh.in4[(w + 1) & m] << 32) | sh.in4[w & m];
    return (u32)(x >> (c.bitpos & 31u));
}
BG_FN bool give_up(Shared& sh, u32 why) {
    sh.status = why;
    sh.state = BI_ST_DONE;
    return false;
}
// n bits are consumed: false (and the member ends) when they reach past the payload
BG_FN bool take(Shared& sh, Cursor& c, int n) {
    if (c.bitpos + (u32)n > c.end_bits) return give_up(sh, BI_E_BITS);
    c.bitpos += (u32)n;
    return true;
}
// the next n <= 16 bits as a number, consumed
BG_FN bool bits(Shared& sh, Cursor& c, int n, u32& v) {
    v = peek(sh, c) & ((1u << n) - 1u);
    return take(sh, c, n);
}

// ---- codes (thread 0) -------------------------------------------------------------------------------------------------------------
// from lens[0 .. n): cnt, sym, root.  0 or the reason the code is refused.
BG_FN u32 build_table(Shared& sh, const u8* lens, int n, u16* cnt, u16* sym, u16* root, int rootbits, int kind) {
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int i = 0; i < n; ++i) cnt[lens[i] & 15]++;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return BI_E_OVERSUBSCRIBED;
    }
    const int used = n - (int)cnt[0];
    if (left > 0) {                                          // incomplete: only "no code at all" (a block without distances) and the one code of one bit pass
        const bool single = used == 1 && cnt[1] == 1;
        if (kind == BI_KIND_CODELEN || !(single || (used == 0 && kind == BI_KIND_DIST))) return BI_E_INCOMPLETE;
    }
    u32 code = 0;
    sh.offs[1] = 0;
    cnt[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + cnt[l - 1]) << 1;
        sh.next[l] = (u16)code;
        if (l < 15) sh.offs[l + 1] = (u16)(sh.offs[l] + cnt[l]);
    }
    const int size = 1 << rootbits;
    for (int k = 0; k < size; ++k) root[k] = 0;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (!l) continue;
        sym[sh.offs[l]++] = (u16)i;
        const u32 c = sh.next[l]++;
        if (l <= rootbits) {
            const u16 e = (u16)((i << 4) | l);
            for (u32 k = epgbg::bit_reverse(c, l); k < (u32)size; k += 1u << l) root[k] = e;
        }
    }
    return BI_OK;
}

// the code at the bit position, by the root or by counts: its symbol, consumed.  false: the member has ended.
BG_FN bool decode_symbol(Shared& sh, Cursor& c, const u16* root, int rootbits, const u16* cnt, const u16* sym, int& s) {
    const u32 b = peek(sh, c);
    const u32 e = root[b & ((1u << rootbits) - 1u)];
    ++c.steps;
    if (e) {
        s = (int)(e >> 4);
        return take(sh, c, (int)(e & 15u));
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((b >> (l - 1)) & 1u);
        const int count = cnt[l];
        if (code - count < first) {
            s = sym[index + (code - first)];
            return take(sh, c, l);
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
        ++c.steps;
    }
    if (c.bitpos + 15u > c.end_bits) return give_up(sh, BI_E_BITS);          // (the pattern was cut short by the payload's end)
    return give_up(sh, BI_E_CODE);
}

BG_FN bool push_token(Shared& sh, Cursor& c, u32 len, u32 from) {
    if (len > c.isize - c.out_pos) return give_up(sh, BI_E_OUTPUT);
    if (len) {
        sh.tok_dst[c.ntok] = c.out_pos;
        sh.tok_len[c.ntok] = len;
        sh.tok_from[c.ntok] = from;
        ++c.ntok;
        c.out_pos += len;
    }
    return true;
}

// a block's header: the stored block whole (its bytes become a token), the codes of a fixed or dynamic block
BG_FN bool block_header(Shared& sh, Cursor& c) {
    u32 v;
    ++c.steps;
    if (!bits(sh, c, 3, v)) return false;
    sh.last = v & 1u;
    const u32 type = v >> 1;
    if (type == 3) return give_up(sh, BI_E_BTYPE);
    if (type == 0) {
        c.bitpos = (c.bitpos + 7u) & ~7u;
        if (c.bitpos + 32u > c.end_bits) return give_up(sh, BI_E_BITS);
        const u32 w = peek(sh, c), len = w & 0xffffu;
        c.bitpos += 32u;
        if (len != (~(w >> 16) & 0xffffu)) return give_up(sh, BI_E_STORED_LEN);
        const u32 at = c.bitpos >> 3;
        if (len > sh.payload_bytes - at) return give_up(sh, BI_E_BITS);
        if (!push_token(sh, c, len, 0x80000000u | at)) return false;
        c.bitpos += 8u * len;
        sh.state = sh.last ? BI_ST_DONE : BI_ST_HEADER;
        return true;
    }
    int hlit = 288, hdist = 32;
    if (type == 1) {
        for (int i = 0; i < 288; ++i) sh.lens[i] = (u8)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) sh.lens[288 + i] = 5;
    } else {
        u32 hclen;
        if (!bits(sh, c, 14, v)) return false;
        hlit = 257 + (int)(v & 31u);
        hdist = 1 + (int)((v >> 5) & 31u);
        hclen = 4 + (v >> 10);
        if (hlit > 286 || hdist > 30) return give_up(sh, BI_E_HEADER);
        const u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (int k = 0; k < 19; ++k) sh.cl[k] = 0;
        for (u32 k = 0; k < hclen; ++k) {
            if (!bits(sh, c, 3, v)) return false;
            sh.cl[order[k]] = (u8)v;
        }
        const u32 why = build_table(sh, sh.cl, 19, sh.ccnt, sh.csym, sh.croot, BI_CROOT, BI_KIND_CODELEN);
        if (why) return give_up(sh, why);
        const int total = hlit + hdist;
        for (int i = 0; i < total;) {
            int s;
            if (!decode_symbol(sh, c, sh.croot, BI_CROOT, sh.ccnt, sh.csym, s)) return false;
            if (s < 16) {
                sh.lens[i++] = (u8)s;
                continue;
            }
            u32 fill = 0, rep;
            if (s == 16) {
                if (i == 0) return give_up(sh, BI_E_REPEAT_FIRST);
                fill = sh.lens[i - 1];
                if (!bits(sh, c, 2, rep)) return false;
                rep += 3;
            } else if (s == 17) {
                if (!bits(sh, c, 3, rep)) return false;
                rep += 3;
            } else {
                if (!bits(sh, c, 7, rep)) return false;
                rep += 11;
            }
            if ((u32)i + rep > (u32)total) return give_up(sh, BI_E_REPEAT_RUN);
            for (u32 k = 0; k < rep; ++k) sh.lens[i++] = (u8)fill;
        }
        if (sh.lens[256] == 0) return give_up(sh, BI_E_HEADER);
    }
    u32 why = build_table(sh, sh.lens, hlit, sh.lcnt, sh.lsym, sh.lroot, BI_LROOT, BI_KIND_LITLEN);
    if (!why) why = build_table(sh, sh.lens + hlit, hdist, sh.dcnt, sh.dsym, sh.droot, BI_DROOT, BI_KIND_DIST);
    if (why) return give_up(sh, why);
    sh.state = BI_ST_CODES;
    return true;
}

// the symbols of a block until it ends, BI_NTOK tokens wait or the ring runs low.  false: the member has ended with a reason.
BG_FN bool decode_codes(Shared& sh, Cursor& c, u32 in_hi, u32 last) {
    u8* w = window(sh);
    while (c.ntok < (u32)BI_NTOK && (int)in_hi - (int)(c.bitpos >> 3) >= BI_SYM_BYTES) {
        int s;
        if (!decode_symbol(sh, c, sh.lroot, BI_LROOT, sh.lcnt, sh.lsym, s)) return false;
        if (s < 256) {
            if (c.out_pos >= c.isize) return give_up(sh, BI_E_OUTPUT);
            w[c.out_pos++] = (u8)s;
            continue;
        }
        if (s == 256) {
            sh.state = last ? BI_ST_DONE : BI_ST_HEADER;
            return true;
        }
        if (s >= 286) return give_up(sh, BI_E_LITLEN_SYM);
        s -= 257;
        u32 len, dist, ev;
        if (s < 8) len = 3u + (u32)s;
        else if (s == 28) len = 258;
        else {
            const int eb = (s >> 2) - 1;
            if (!bits(sh, c, eb, ev)) return false;
            len = 3u + ((4u + (u32)(s & 3)) << eb) + ev;
        }
        if (!decode_symbol(sh, c, sh.droot, BI_DROOT, sh.dcnt, sh.dsym, s)) return false;
        if (s >= 30) return give_up(sh, BI_E_DIST_SYM);
        if (s < 4) dist = 1u + (u32)s;
        else {
            const int eb = (s >> 1) - 1;
            if (!bits(sh, c, eb, ev)) return false;
            dist = 1u + ((2u + (u32)(s & 1)) << eb) + ev;
        }
        if (dist > c.out_pos) return give_up(sh, BI_E_DIST_FAR);
        if (!push_token(sh, c, len, dist)) return false;
    }
    return true;
}

// thread 0: on from where the last turn stopped, until BI_NTOK tokens wait, the ring runs low or the member ends
BG_FN void inflate_decode(Shared& sh) {
    ++sh.phases;
    Cursor c;
    cursor_load(sh, c);
    const u32 in_hi = sh.in_hi;
    u32 state = sh.state;
    while (state != BI_ST_DONE && c.ntok < (u32)BI_NTOK) {
        const int have = (int)in_hi - (int)(c.bitpos >> 3);
        if (state == BI_ST_HEADER) {
            if (have < BI_HDR_BYTES) break;
            block_header(sh, c);
        } else {
            if (have < BI_SYM_BYTES) break;
            decode_codes(sh, c, in_hi, sh.last);
            if (sh.state == BI_ST_CODES) break;              // the block goes on: the tokens are full or the ring is low
        }
        state = sh.state;
    }
    cursor_store(sh, c);
    if (sh.state == BI_ST_DONE && sh.status == BI_OK) {      // the stream's end: all of the text, and all of the payload
        if (c.out_pos != c.isize) sh.status = BI_E_ISIZE;
        else if (((c.bitpos + 7u) >> 3) != sh.payload_bytes) sh.status = BI_E_TRAILING;
    }
}

// ---- the copies (all threads, token by token) -------------------------------------------------------------------------------------
BG_FN void inflate_copy(Shared& sh, const u8* payload, int k, int t) {
    u8* w = window(sh) + sh.tok_dst[k];
    const u32 len = sh.tok_len[k], from = sh.tok_from[k];
    if (from & 0x80000000u) {
        const u8* src = payload + (from & 0x7fffffffu);
        for (u32 i = (u32)t; i < len; i += BI_T) w[i] = src[i];
    } else if (from >= len) {
        for (u32 i = (u32)t; i < len; i += BI_T) w[i] = *(w + i - from);
    } else if (from == 1) {
        const u8 c = *(w - 1);
        for (u32 i = (u32)t; i < len; i += BI_T) w[i] = c;
    } else {
        for (u32 i = (u32)t; i < len; i += BI_T) w[i] = *(w + (i % from) - from);
    }
}

// ---- the trailer ------------------------------------------------------------------------------------------------------------------
BG_FN void inflate_crc(Shared& sh, int t) {
    const u32 n = sh.isize, slice = (n + BI_T - 1) / BI_T, c0 = (u32)t * slice;
    if (sh.status != BI_OK || c0 >= n) return;
    const u32 c1 = c0 + slice < n ? c0 + slice : n;
    epgbg::atom_xor(&sh.crc, epgbg::crc_advance(epgbg::crc_slice(sh.crctab, window(sh) + c0, (long long)(c1 - c0)), n - c1));
}
// one thread: the member's status
BG_FN u32 inflate_finish(Shared& sh, u32 crc) {
    if (sh.status == BI_OK && sh.crc != crc) sh.status = BI_E_CRC;
    return sh.status;
}

}  // namespace epgbi
