// Stand-alone host program: the per-thread phases of the device BGZF compressor (csrc/epg_bgzf_block.h, compiled here for the host and
// run thread by thread in the order the kernels' barriers give) on synthetic score text, inflated again with zlib.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iepilogos_amd/csrc tests/bgzf_block_check.cpp -lz \
//       -o bgzf_block_check && ./bgzf_block_check
// Every case must round-trip through zlib's inflate (which checks each member's CRC-32 and ISIZE), every member must be at most
// 65 536 bytes with BSIZE = its size - 1, and the cases with repeated rows must come out below their zeroth-order entropy.
// The hostile families of tests/bgzf_hostile.py are built here again from the same recipes (deep alphabets that need the 15-bit and
// the 7-bit cut, a ladder of every match length and of both ends of every distance symbol, one-byte, long and empty rows, rows across
// block borders); for the two deep alphabets the code's depth is asserted on the builder's own state.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "epg_bgzf_block.h"
#include "epg_fmt_f5.h"

using namespace epgbg;

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}

static int g_max_len, g_max_cllen;                                             // over the blocks of the last compress(): the deepest codes

static std::vector<unsigned char> compress(const std::vector<unsigned char>& text, const std::vector<long long>* rows, bool eof, long long* stored_blocks) {
    const long long n = (long long)text.size();
    const long long nb = (n + BG_TEXT - 1) / BG_TEXT;
    const Rows rw = make_rows(rows ? rows->data() : nullptr, rows ? (long long)rows->size() - 1 : 0, n);
    std::vector<Rec> recs((size_t)nb);
    *stored_blocks = 0;
    g_max_len = g_max_cllen = 0;
    for (long long b = 0; b < nb; ++b) {
        const long long B0 = b * BG_TEXT, B1 = B0 + BG_TEXT < n ? B0 + BG_TEXT : n;
        static Shared sh;
        Rec& rec = recs[(size_t)b];
        for (int t = 0; t < BG_T; ++t) plan_init(sh, t);
        plan_rows(sh, rw, B0, B1);
        for (int t = 0; t < BG_T; ++t) plan_hist(sh, text.data(), rw, B0, B1, t);
        sh.hist[256] += 1;
        build_block_code(sh);
        for (int i = 0; i < BG_NSYM; ++i) g_max_len = sh.len[i] > g_max_len ? sh.len[i] : g_max_len;
        for (int i = 0; i < 19; ++i) g_max_cllen = sh.cllen[i] > g_max_cllen ? sh.cllen[i] : g_max_cllen;
        u32 total = 0;
        for (int t = 0; t < BG_T; ++t) {
            rec.tbits[t] = sh.hdr_bits + total;
            total += plan_bits(sh, text.data(), rw, B0, B1, t);
        }
        memcpy(rec.code, sh.code, sizeof(rec.code));
        memcpy(rec.len, sh.len, sizeof(rec.len));
        memcpy(rec.hdr, sh.hdr, sizeof(rec.hdr));
        plan_finish(sh, rec, total, B0, B1);
        *stored_blocks += rec.stored;
    }
    std::vector<unsigned char> out;
    for (long long b = 0; b < nb; ++b) {
        const long long B0 = b * BG_TEXT, B1 = B0 + BG_TEXT < n ? B0 + BG_TEXT : n;
        const Rec& rec = recs[(size_t)b];
        const u32 a = (u32)(out.size() & 15);
        std::vector<u32> words((a + rec.size + 3) / 4 + 5, 0u);          // exactly what the kernel zeroes, so ASan sees a write beyond it
        for (int t = 0; t < BG_T; ++t) emit_frame(words.data(), a, rec, t);
        unsigned char* bytes = reinterpret_cast<unsigned char*>(words.data());
        if (rec.stored) memcpy(bytes + a + 23, text.data() + B0, (size_t)(B1 - B0));
        else
            for (int t = 0; t < BG_T; ++t) emit_tokens(words.data(), a, rec, rec.code, rec.len, text.data(), rw, B0, B1, t);
        out.insert(out.end(), bytes + a, bytes + a + rec.size);
    }
    if (eof) {
        const unsigned char e[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        out.insert(out.end(), e, e + 28);
    }
    return out;
}

static bool inflate_all(const std::vector<unsigned char>& z, std::vector<unsigned char>& out) {
    out.clear();
    size_t at = 0;
    while (at < z.size()) {
        if (z.size() - at < 28 || z[at] != 0x1f || z[at + 12] != 'B') return false;
        const size_t bsize = (size_t)z[at + 16] + ((size_t)z[at + 17] << 8) + 1;
        if (bsize > 65536 || at + bsize > z.size()) return false;
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
        std::vector<unsigned char> buf(65536 + 64);
        zs.next_in = (Bytef*)z.data() + at;
        zs.avail_in = (uInt)bsize;
        zs.next_out = buf.data();
        zs.avail_out = (uInt)buf.size();
        const int rc = inflate(&zs, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && zs.avail_in == 0 && zs.total_out <= 65280;
        out.insert(out.end(), buf.data(), buf.data() + zs.total_out);
        inflateEnd(&zs);
        if (!ok) { printf("  member at %zu: inflate rc %d (%s), %u bytes left\n", at, rc, zs.msg ? zs.msg : "", zs.avail_in); return false; }
        at += bsize;
    }
    return true;
}

static void make_text(int R, int S, int mode, const char* chrom, std::vector<unsigned char>& text, std::vector<long long>& rows) {
    text.clear();
    rows.assign(1, 0);
    std::vector<float> row((size_t)S);
    for (int r = 0; r < R; ++r) {
        char buf[64];
        const int n = snprintf(buf, sizeof buf, "%s\t%d\t%d", chrom, 9800 + r * 200, 10000 + r * 200);
        text.insert(text.end(), buf, buf + n);
        if (mode != 2 || r % 30 == 0)
            for (int s = 0; s < S; ++s) {
                const float u = (float)((rnd() % 200001) - 100000) / 100000.0f;
                row[(size_t)s] = mode == 1 && rnd() % 10 < 6 ? 0.0f : mode == 3 ? 0.25f : u * u * u * 3.0f;
            }
        for (int s = 0; s < S; ++s) {
            uint32_t bits;
            memcpy(&bits, &row[(size_t)s], 4);
            uint64_t q;
            epgfmt::f5_scale(bits, &q);
            char num[24];
            const int L = epgfmt::f5_emit(bits, q, [&](int at, char c) { num[at] = c; });
            text.push_back('\t');
            text.insert(text.end(), num, num + L);
        }
        text.push_back('\n');
        rows.push_back((long long)text.size());
    }
}

static double h0_bytes(const std::vector<unsigned char>& t) {
    double c[256] = {0}, h = 0;
    for (unsigned char b : t) c[b] += 1;
    for (double v : c)
        if (v > 0) h -= v * log2(v / (double)t.size());
    return h / 8;
}

static int check(const char* what, const std::vector<unsigned char>& text, const std::vector<long long>* rows, int want_stored, bool below_h0) {
    long long stored = 0;
    for (int eof = 0; eof < 2; ++eof) {
        const std::vector<unsigned char> z = compress(text, rows, eof != 0, &stored);
        std::vector<unsigned char> back;
        const long long nb = ((long long)text.size() + BG_TEXT - 1) / BG_TEXT;
        if (!inflate_all(z, back) || back != text) { printf("%s: does not round-trip\n", what); return 1; }
        if (want_stored >= 0 && (stored == nb) != (want_stored != 0)) { printf("%s: %lld of %lld blocks stored\n", what, stored, nb); return 1; }
        if (z.size() > text.size() + (size_t)nb * 31 + 28 * (size_t)eof) { printf("%s: above the bound\n", what); return 1; }
        if (below_h0 && (double)z.size() >= h0_bytes(text)) { printf("%s: %zu bytes, not below H0 %.0f\n", what, z.size(), h0_bytes(text)); return 1; }
        if (!eof) printf("%-34s text %9zu  out %9zu  ratio %.4f  H0 %.4f  stored %lld/%lld\n", what, text.size(), z.size(),
                         text.empty() ? 0.0 : (double)z.size() / (double)text.size(), text.empty() ? 0.0 : h0_bytes(text) / (double)text.size(), stored, nb);
    }
    return 0;
}

// ---- the hostile families (tests/bgzf_hostile.py) ------------------------------------------------------------------------------------
static const unsigned char ALPHA[17] = "0123456789.-\tchr";
static unsigned char letter() { return ALPHA[rnd() % 16]; }
static unsigned char other(unsigned char c) {                                  // a letter that is not c
    int k = 0;
    while (k < 16 && ALPHA[k] != c) ++k;
    return ALPHA[(k + 1 + (int)(rnd() % 15)) % 16];
}
static void end_row(const std::vector<unsigned char>& text, std::vector<long long>& rows) { rows.push_back((long long)text.size()); }

static void ladder_lengths(std::vector<unsigned char>& text, std::vector<long long>& rows) {
    text.clear();
    rows.assign(1, 0);
    for (int k = 0; k < 300; ++k) text.push_back(letter());
    end_row(text, rows);
    for (int r = 0; r < 255; ++r) {                                            // 222 and 223 again: the first block's border takes their rows
        const int L = r < 253 ? 6 + r : 222 + (r - 253);
        for (int k = 0; k < 300; ++k) {
            const unsigned char up = text[text.size() - 300];
            text.push_back(k < L ? up : other(up));
        }
        end_row(text, rows);
    }
}
static void ladder_distances(std::vector<unsigned char>& text, std::vector<long long>& rows) {
    std::vector<int> ds = {1, 2, 3, 4};
    for (int sym = 4; sym < 30; ++sym) {
        const int nb = sym / 2 - 1, lo = 1 + ((2 + (sym & 1)) << nb);
        ds.push_back(lo);
        ds.push_back(lo + (1 << nb) - 1);
    }
    ds.push_back(32769);
    ds.push_back(40000);
    text.clear();
    rows.assign(1, 0);
    for (int d : ds) {
        for (int k = 0; k < d; ++k) text.push_back(text.size() >= 40 ? other(text[text.size() - 40]) : letter());
        end_row(text, rows);
        for (int k = 0; k < 40; ++k) text.push_back(text[text.size() - (size_t)d]);
        end_row(text, rows);
    }
}
static void shuffle(std::vector<unsigned char>& t) {
    for (size_t i = t.size(); i > 1; --i) {
        const size_t j = rnd() % i;
        const unsigned char x = t[i - 1];
        t[i - 1] = t[j];
        t[j] = x;
    }
}
static void chain(std::vector<unsigned char>& text) {
    text.clear();
    long long a = 1, b = 2;
    for (int k = 0; k < 21; ++k) {
        text.insert(text.end(), (size_t)a, (unsigned char)k);
        const long long c = a + b;
        a = b;
        b = c;
    }
    shuffle(text);
}
static void dyadic(std::vector<unsigned char>& text) {
    const int per[16] = {0, 0, 0, 0, 6, 12, 5, 16, 5, 7, 1, 16, 0, 1, 1, 153};
    text.clear();
    int v = 0;
    for (int L = 4; L <= 15; ++L)
        for (int c = 0; c < per[L]; ++c) text.insert(text.end(), (size_t)1 << (15 - L), (unsigned char)v++);
    shuffle(text);
}
static void one_byte_rows(std::vector<unsigned char>& text, std::vector<long long>& rows) {
    text.clear();
    rows.assign(1, 0);
    for (int r = 0; r < 70000; ++r) {
        text.push_back(r > 0 && rnd() % 3 < 2 ? text.back() : letter());
        end_row(text, rows);
    }
}
static void long_rows(std::vector<unsigned char>& text, std::vector<long long>& rows) {
    text.clear();
    rows.assign(1, 0);
    std::vector<unsigned char> a(50000), b(32768);
    for (auto& c : a) c = letter();
    for (auto& c : b) c = letter();
    for (int r = 0; r < 8; ++r) {
        const std::vector<unsigned char>& row = r < 3 ? a : b;
        text.insert(text.end(), row.begin(), row.end());
        end_row(text, rows);
    }
}
static void empty_rows(std::vector<unsigned char>& text, std::vector<long long>& rows) {
    text.clear();
    rows.assign(1, 0);
    for (int r = 0; r < 3000; ++r) {
        if (r % 4 == 1) {
            const std::vector<unsigned char> up(text.end() - 57, text.end());
            text.insert(text.end(), up.begin(), up.end());
        } else if (r % 4 != 2)
            for (int k = 0; k < 57; ++k) text.push_back(letter());
        end_row(text, rows);
    }
}
static void border(int pad, std::vector<unsigned char>& text, std::vector<long long>& rows) {
    text.clear();
    rows.assign(1, 0);
    std::vector<unsigned char> row(300);
    for (auto& c : row) c = letter();
    if (pad) {
        for (int k = 0; k < pad; ++k) text.push_back(letter());
        end_row(text, rows);
    }
    for (int r = 0; r < 652; ++r) {
        text.insert(text.end(), row.begin(), row.end());
        end_row(text, rows);
    }
}

// a deep alphabet: one block, not stored, the literal/length code exactly 15 bits deep, the code-length code want_cl (0: any)
static int check_deep(const char* what, const std::vector<unsigned char>& text, int want_cl) {
    if (check(what, text, nullptr, 0, false)) return 1;
    if (text.size() > (size_t)BG_TEXT || g_max_len != 15 || (want_cl && g_max_cllen != want_cl)) {
        printf("%s: deepest code %d bits (wanted 15), code-length code %d (wanted %d)\n", what, g_max_len, g_max_cllen, want_cl);
        return 1;
    }
    return 0;
}

int main() {
    std::vector<unsigned char> text;
    std::vector<long long> rows;
    int bad = 0;
    make_text(0, 18, 0, "chr1", text, rows);
    bad |= check("no rows", text, &rows, -1, false);
    make_text(1, 1, 0, "1", text, rows);
    bad |= check("one row, one value", text, &rows, -1, false);
    make_text(4097, 25, 0, "chrUn_gl000220", text, rows);
    bad |= check("random scores 4097 x 25", text, &rows, 0, false);
    make_text(20001, 18, 0, "1", text, rows);
    bad |= check("random scores 20001 x 18", text, &rows, 0, false);
    make_text(20001, 18, 1, "chr1", text, rows);
    bad |= check("60 % zeros", text, &rows, 0, false);
    make_text(20001, 18, 2, "chr1", text, rows);
    bad |= check("runs of 30 equal rows", text, &rows, 0, true);
    make_text(700, 127, 3, "chr1", text, rows);
    bad |= check("all rows equal, 127 values", text, &rows, 0, true);
    bad |= check("the same without row offsets", text, nullptr, 0, false);
    std::vector<long long> hostile = rows;
    for (size_t i = 1; i + 1 < hostile.size(); i += 7) hostile[i] = (long long)(rnd() % (text.size() + 100)) - 50;
    bad |= check("row offsets out of order", text, &hostile, -1, false);
    for (size_t n : {(size_t)70001, (size_t)65281, (size_t)65280, (size_t)1, (size_t)255, (size_t)257}) {
        text.resize(n);
        for (auto& b : text) b = (unsigned char)rnd();
        bad |= check("random bytes", text, nullptr, n >= 4096 ? 1 : -1, false);
    }
    text.assign(200000, 'a');
    bad |= check("one byte repeated, no rows", text, nullptr, 0, false);
    chain(text);
    bad |= check_deep("chain: Fibonacci weights", text, 0);
    dyadic(text);
    bad |= check_deep("dyadic: 15 bits, nothing to cut", text, 7);
    ladder_lengths(text, rows);
    bad |= check("ladder of lengths 6 .. 258", text, &rows, 0, false);
    ladder_distances(text, rows);
    bad |= check("ladder of distances", text, &rows, 0, false);
    one_byte_rows(text, rows);
    bad |= check("70000 rows of one byte", text, &rows, 0, false);
    long_rows(text, rows);
    bad |= check("rows of 50000 and 32768 bytes", text, &rows, 0, false);
    empty_rows(text, rows);
    bad |= check("every fourth row empty", text, &rows, 0, false);
    for (int pad : {0, 180, 179}) {
        border(pad, text, rows);
        bad |= check("equal rows across block borders", text, &rows, 0, true);
    }
    printf(bad ? "bgzf_block_check: FAILED\n" : "bgzf_block_check: ok\n");
    return bad;
}
