// Stand-alone host program: the per-thread phases of the device BGZF inflater (csrc/epg_bgzf_inflate_block.h, compiled here for the host
// and run thread by thread in the order the kernel's barriers give) on DEFLATE streams made by zlib and by hand, every verdict held
// against zlib's own raw inflate.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iepilogos_amd/csrc tests/bgzf_inflate_check.cpp -lz \
//       -o bgzf_inflate_check && ./bgzf_inflate_check
// A member is "good" exactly when zlib's raw inflate of its payload ends the stream with the payload's last byte, yields ISIZE bytes
// and their CRC-32 is the trailer's: then the phases must give status 0 and the same bytes, otherwise a status that is not 0 (the
// hand-made corruptions: the very reason).  Every run checks that no byte of the window behind ISIZE changed, that the payload is
// read inside an allocation of exactly its size (the address sanitizer watches), and the bound on the decoder's turns.
// With `--members FILE` the program runs the members of that file instead (tests/bgzf_streams.py writes it for tests/test_inflate_host.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <utility>
#include <vector>

#include "epg_bgzf_inflate_block.h"

using namespace epgbi;
typedef std::vector<unsigned char> Bytes;

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}

struct Member {
    Bytes payload;
    uint32_t isize, crc;
};

// ---- the phases, as the kernel runs them ---------------------------------------------------------------------------------------------
static int g_runs = 0;
static uint32_t run_phases(const Member& m, Bytes& text, bool* bound_ok) {
    Shared* sh = new Shared;
    memset(sh, 0xA5, sizeof(Shared));
    const uint32_t a = (uint32_t)(g_runs++ % 16);
    Bytes payload(m.payload);                                                  // exactly its size: a read beyond it is the sanitizer's
    const u8* p = payload.empty() ? reinterpret_cast<const u8*>(sh) : payload.data();
    const uint32_t pbytes = (uint32_t)payload.size();
    for (int t = 0; t < BI_T; ++t) inflate_init(*sh, pbytes, m.isize, a, t);
    uint64_t written = 0;
    const uint64_t bound = 8ull * pbytes + m.isize + BI_STEP_SLACK;
    bool done = false;
    uint64_t turns = 0;
    while (!done && turns < 2 * bound) {
        ++turns;
        for (int t = 0; t < BI_T; ++t) inflate_refill(*sh, p, t);
        inflate_refilled(*sh);
        const uint32_t before = sh->out_pos;
        inflate_decode(*sh);
        written += sh->out_pos - before;
        done = sh->state == BI_ST_DONE;
        for (uint32_t k = 0; k < sh->ntok; ++k)
            for (int t = 0; t < BI_T; ++t) inflate_copy(*sh, p, (int)k, t);
    }
    *bound_ok = done && sh->steps + written <= bound && sh->phases <= sh->steps + 2 && written <= m.isize;
    if (!*bound_ok) printf("  the bound: done %d steps %u written %llu phases %u bound %llu\n", (int)done, sh->steps, (unsigned long long)written, sh->phases,
                           (unsigned long long)bound);
    for (int t = 0; t < BI_T; ++t) inflate_crc(*sh, t);
    const uint32_t why = inflate_finish(*sh, m.crc);
    const u8* w = reinterpret_cast<const u8*>(sh->win4);
    for (uint32_t i = 0; i < sizeof(sh->win4); ++i)
        if ((i < a || i >= a + m.isize) && w[i] != 0xA5) {
            printf("  window byte %u outside [%u, %u) was written\n", i, a, a + m.isize);
            *bound_ok = false;
            break;
        }
    text.assign(w + a, w + a + m.isize);
    delete sh;
    return why;
}

// ---- zlib ------------------------------------------------------------------------------------------------------------------------------
static bool zlib_good(const Member& m, Bytes& text) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) abort();
    Bytes in(m.payload);
    text.assign((size_t)m.isize + 1, 0);
    zs.next_in = in.empty() ? (Bytef*)"" : in.data();
    zs.avail_in = (uInt)in.size();
    zs.next_out = text.data();
    zs.avail_out = (uInt)text.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_in == 0 && zs.total_out == m.isize && crc32(0, text.data(), m.isize) == m.crc;
    inflateEnd(&zs);
    text.resize(m.isize);
    return ok;
}

static Member deflate_member(const Bytes& text, int level, int strategy, size_t flush_at = 0) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, strategy) != Z_OK) abort();
    Member m;
    m.payload.assign(text.size() + text.size() / 8 + 256, 0);
    zs.next_out = m.payload.data();
    zs.avail_out = (uInt)m.payload.size();
    Bytes in(text);
    if (flush_at) {
        zs.next_in = in.data();
        zs.avail_in = (uInt)flush_at;
        if (deflate(&zs, Z_FULL_FLUSH) != Z_OK) abort();
    }
    zs.next_in = in.empty() ? (Bytef*)"" : in.data() + flush_at;
    zs.avail_in = (uInt)(in.size() - flush_at);
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) abort();
    m.payload.resize(zs.total_out);
    deflateEnd(&zs);
    m.isize = (uint32_t)text.size();
    m.crc = (uint32_t)crc32(0, text.data(), (uInt)text.size());
    return m;
}

// ---- streams by hand -----------------------------------------------------------------------------------------------------------------
struct BitW {
    Bytes out;
    uint32_t nbits = 0;
    void put(uint32_t v, int n) {
        for (int i = 0; i < n; ++i, ++nbits) {
            if ((nbits & 7) == 0) out.push_back(0);
            out.back() |= (unsigned char)(((v >> i) & 1u) << (nbits & 7));
        }
    }
    void code(uint32_t c, int len) {                                          // a Huffman code: most significant bit first
        for (int i = len - 1; i >= 0; --i) put((c >> i) & 1u, 1);
    }
    void align() { nbits = (nbits + 7) & ~7u; }
};
static void canon(const int* lens, int n, uint32_t* codes) {
    int cnt[16] = {0};
    uint32_t next[16] = {0}, c = 0;
    for (int i = 0; i < n; ++i) cnt[lens[i]]++;
    cnt[0] = 0;
    for (int l = 1; l < 16; ++l) {
        c = (c + cnt[l - 1]) << 1;
        next[l] = c;
    }
    for (int i = 0; i < n; ++i) codes[i] = lens[i] ? next[lens[i]]++ : 0;
}
// the code-length code of every hand-made header: symbols 0 .. 12 in four bits, 13 .. 18 in five (complete)
static const int CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
struct Hand {
    BitW w;
    int llen[288] = {0}, dlen[32] = {0};
    uint32_t lcode[288], dcode[32], clcode[19];
    int cllen[19];
    int hlit = 257, hdist = 1;
    Hand() {
        for (int i = 0; i < 19; ++i) cllen[i] = i < 13 ? 4 : 5;
        canon(cllen, 19, clcode);
    }
    void cl(int s) { w.code(clcode[s], cllen[s]); }
    // the header of a dynamic block; `first16`: the lengths start with repeat symbol 16
    void header(int bfinal, bool first16 = false) {
        w.put((uint32_t)bfinal, 1);
        w.put(2, 2);
        w.put((uint32_t)(hlit - 257), 5);
        w.put((uint32_t)(hdist - 1), 5);
        w.put(15, 4);
        for (int k = 0; k < 19; ++k) w.put((uint32_t)cllen[CL_ORDER[k]], 3);
        if (first16) { cl(16); w.put(0, 2); }
        for (int i = 0; i < hlit; ++i) cl(llen[i]);
        for (int i = 0; i < hdist; ++i) cl(dlen[i]);
        canon(llen, 288, lcode);
        canon(dlen, 32, dcode);
    }
    void lit(int s) { w.code(lcode[s], llen[s]); }
    void dist(int s) { w.code(dcode[s], dlen[s]); }
};
static Member member_of(const BitW& w, const Bytes& text) {
    Member m;
    m.payload = w.out;
    m.isize = (uint32_t)text.size();
    m.crc = (uint32_t)crc32(0, text.empty() ? (const Bytef*)"" : text.data(), (uInt)text.size());
    return m;
}
static void fixed_lit(BitW& w, int s) {                                        // a literal/length symbol of the fixed code
    if (s < 144) w.code(0x30 + (uint32_t)s, 8);
    else if (s < 256) w.code(0x190 + (uint32_t)(s - 144), 9);
    else if (s < 280) w.code((uint32_t)(s - 256), 7);
    else w.code(0xC0 + (uint32_t)(s - 280), 8);
}

// ---- the checks ------------------------------------------------------------------------------------------------------------------------
static int g_bad = 0, g_cases = 0;
// want: -1 = whatever zlib says, 0 = good, otherwise the reason
static void check(const char* what, const Member& m, int want, const Bytes* text = nullptr) {
    Bytes ours, theirs;
    bool bound_ok;
    const uint32_t why = run_phases(m, ours, &bound_ok);
    const bool good = zlib_good(m, theirs);
    ++g_cases;
    bool ok = bound_ok && (why == BI_OK) == good && why < BI_REASONS;
    if (good && ours != theirs) ok = false;
    if (good && text && ours != *text) ok = false;
    if (want >= 0 && (int)why != want) ok = false;
    if (!ok) {
        printf("%s: status %u, wanted %d, zlib says %s%s\n", what, why, want, good ? "good" : "bad", good && ours != theirs ? ", the bytes differ" : "");
        ++g_bad;
    }
}

static Bytes score_text(int rows) {
    Bytes t;
    for (int r = 0; r < rows; ++r) {
        char buf[512];
        int n = snprintf(buf, sizeof buf, "chr%d\t%d\t%d", 1 + r / 5000, 9800 + r * 200, 10000 + r * 200);
        for (int s = 0; s < 18; ++s) n += snprintf(buf + n, sizeof buf - (size_t)n, "\t%.5f", (rnd() % 10 < 4) ? 0.0 : ((int)(rnd() % 200001) - 100000) / 31000.0);
        buf[n++] = '\n';
        t.insert(t.end(), buf, buf + n);
    }
    return t;
}

static void fuzz(const char* what, const Member& base, int count) {
    char name[128];
    for (int k = 0; k < count && !base.payload.empty(); ++k) {
        Member m = base;
        const size_t at = rnd() % m.payload.size();
        // the first 48 bytes hold the headers: half of the mutations go there
        const size_t pos = (k & 1) ? at : at % (m.payload.size() < 48 ? m.payload.size() : 48);
        if (k % 3 == 0) m.payload[pos] = (unsigned char)rnd();
        else m.payload[pos] ^= (unsigned char)(1u << (rnd() % 8));
        snprintf(name, sizeof name, "%s, mutation %d at byte %zu", what, k, pos);
        check(name, m, -1);
    }
}

// `--members FILE`: the members of tests/bgzf_streams.py (what the GPU tests run), a record each of four little-endian uint32 -- payload
// bytes, ISIZE, CRC-32, the reason wanted -- and the payload
static int check_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    uint32_t h[4];
    char name[64];
    while (fread(h, 4, 4, f) == 4) {
        Member m;
        m.payload.resize(h[0]);
        if (h[0] && fread(m.payload.data(), 1, h[0], f) != h[0]) { printf("%s is cut short\n", path); fclose(f); return 1; }
        m.isize = h[1];
        m.crc = h[2];
        snprintf(name, sizeof name, "member %d of the file", g_cases);
        check(name, m, (int)h[3]);
    }
    fclose(f);
    printf("%d members of %s, %d wrong\n", g_cases, path, g_bad);
    printf(g_bad || !g_cases ? "bgzf_inflate_check: FAILED\n" : "bgzf_inflate_check: ok\n");
    return g_bad || !g_cases ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 2 && !strcmp(argv[1], "--members")) return check_file(argv[2]);
    const int nfuzz = argc > 1 ? atoi(argv[1]) : 1500;
    Bytes text = score_text(600);
    text.resize(65280);
    // (a) zlib's own streams
    for (int level : {1, 6, 9}) check("zlib level", deflate_member(text, level, Z_DEFAULT_STRATEGY), 0, &text);
    check("Z_FIXED", deflate_member(text, 6, Z_FIXED), 0, &text);
    check("Z_HUFFMAN_ONLY", deflate_member(text, 6, Z_HUFFMAN_ONLY), 0, &text);
    check("stored", deflate_member(text, 0, Z_DEFAULT_STRATEGY), 0, &text);
    check("a full flush in the middle", deflate_member(text, 6, Z_DEFAULT_STRATEGY, 30001), 0, &text);
    Bytes t(65536, 'x');
    check("65 536 equal bytes", deflate_member(t, 6, Z_DEFAULT_STRATEGY), 0, &t);
    for (size_t i = 0; i < 32768; ++i) t[i] = t[i + 32768] = (unsigned char)rnd();
    check("a period of 32 768 bytes", deflate_member(t, 9, Z_DEFAULT_STRATEGY), 0, &t);
    {
        BitW w;                                                                // zlib never reaches back more than 32 506 bytes: by hand, a stored block and 127
        w.put(0, 3); w.align();                                                // matches of 258 bytes at distance 32 768
        w.out.push_back(0); w.out.push_back(0x80); w.out.push_back(0xff); w.out.push_back(0x7f);
        w.out.insert(w.out.end(), t.begin(), t.begin() + 32768);
        w.nbits = 8 * (uint32_t)w.out.size();
        w.put(1, 1); w.put(1, 2);
        for (int k = 0; k < 127; ++k) { fixed_lit(w, 285); w.code(29, 5); w.put(8191, 13); }
        fixed_lit(w, 256);
        Bytes far(t.begin(), t.begin() + 32768 + 127 * 258);
        check("distance 32 768", member_of(w, far), 0, &far);
    }
    t.clear();
    uint32_t fa = 1, fb = 1;
    for (int s = 0; s < 22; ++s) {                                             // Fibonacci weights: a code of depth 21, cut to 15 bits
        t.insert(t.end(), fa, (unsigned char)('A' + s));
        const uint32_t fc = fa + fb;
        fa = fb;
        fb = fc;
    }
    for (size_t i = t.size() - 1; i > 0; --i) std::swap(t[i], t[rnd() % (i + 1)]);
    const Member fib = deflate_member(t, 6, Z_HUFFMAN_ONLY);
    check("a Fibonacci-weighted alphabet", fib, 0, &t);
    t.assign(text.begin(), text.begin() + 3000);
    for (auto& b : t) b = (unsigned char)rnd();
    check("literals only", deflate_member(t, 6, Z_DEFAULT_STRATEGY), 0, &t);
    t.assign(1, 'q');
    check("one byte", deflate_member(t, 6, Z_DEFAULT_STRATEGY), 0, &t);
    t.clear();
    check("zero bytes", deflate_member(t, 6, Z_DEFAULT_STRATEGY), 0, &t);
    {
        Member eof;
        eof.payload = {3, 0};
        eof.isize = 0;
        eof.crc = 0;
        check("the end-of-file block", eof, 0);
    }
    t = score_text(700);
    t.resize(65536);
    check("exactly 65 536 bytes", deflate_member(t, 6, Z_DEFAULT_STRATEGY), 0, &t);
    check("exactly 65 536 bytes, stored", deflate_member(t, 0, Z_DEFAULT_STRATEGY), 0, &t);
    // (b) by hand: what zlib never writes but accepts
    Bytes aaaa(1 + 3 * 40, 'a');
    Member single;
    {
        Hand h;                                                                // one distance code of one bit
        h.llen['a'] = 1; h.llen[256] = 2; h.llen[257] = 2; h.hlit = 258; h.dlen[0] = 1; h.hdist = 1;
        h.header(1);
        h.lit('a');
        for (int k = 0; k < 40; ++k) { h.lit(257); h.dist(0); }
        h.lit(256);
        single = member_of(h.w, aaaa);
        check("a distance tree with a single code", single, 0, &aaaa);
    }
    Member nodist;
    {
        Hand h;                                                                // no distance code, and a second block behind the first
        h.llen['a'] = 1; h.llen[256] = 1; h.hlit = 257;
        h.header(0);
        for (int k = 0; k < 60; ++k) h.lit('a');
        h.lit(256);
        h.header(1);
        for (int k = 0; k < 61; ++k) h.lit('a');
        h.lit(256);
        nodist = member_of(h.w, aaaa);
        check("blocks with no distance code", nodist, 0, &aaaa);
    }
    {
        Hand h;                                                                // only the end-of-block symbol has a code: incomplete, and allowed
        h.llen[256] = 1; h.hlit = 257;
        h.header(1);
        h.lit(256);
        check("an end-of-block code alone", member_of(h.w, Bytes()), 0);
    }
    // (c) every corruption, by a known edit
    {
        BitW w;
        w.put(1, 1); w.put(3, 2);
        check("block type 3", member_of(w, Bytes()), BI_E_BTYPE);
    }
    {
        Member m = deflate_member(text, 0, Z_DEFAULT_STRATEGY);
        m.payload[3] ^= 1;                                                     // NLEN's lowest bit
        check("LEN / NLEN", m, BI_E_STORED_LEN);
    }
    {
        Hand h;
        h.llen['a'] = 1; h.llen['b'] = 1; h.llen[256] = 1; h.hlit = 257;
        h.header(1);
        check("an over-subscribed code", member_of(h.w, Bytes()), BI_E_OVERSUBSCRIBED);
    }
    {
        Hand h;
        h.llen['a'] = 2; h.llen[256] = 2; h.hlit = 257;
        h.header(1);
        h.lit(256);
        check("an incomplete code", member_of(h.w, Bytes()), BI_E_INCOMPLETE);
        Hand g;
        g.llen['a'] = 1; g.llen[256] = 1; g.hlit = 257; g.dlen[0] = 2; g.dlen[1] = 2; g.hdist = 2;
        g.header(1);
        g.lit(256);
        check("an incomplete distance code of two codes", member_of(g.w, Bytes()), BI_E_INCOMPLETE);
    }
    {
        Hand h;
        h.llen['a'] = 1; h.llen[256] = 1; h.hlit = 257;
        h.header(1, true);
        check("repeat symbol 16 first", member_of(h.w, Bytes()), BI_E_REPEAT_FIRST);
        Hand g;
        g.llen['a'] = 1; g.llen[256] = 1; g.hlit = 257;
        g.w.put(1, 1); g.w.put(2, 2); g.w.put(0, 5); g.w.put(29, 5); g.w.put(15, 4);      // HLIT 257, HDIST 30: 287 lengths
        for (int k = 0; k < 19; ++k) g.w.put((uint32_t)g.cllen[CL_ORDER[k]], 3);
        for (int i = 0; i < 257; ++i) g.cl(g.llen[i]);
        g.cl(18); g.w.put(127, 7);                                             // 138 zeros where 30 lengths are left
        check("a run past HLIT + HDIST", member_of(g.w, Bytes()), BI_E_REPEAT_RUN);
    }
    for (int s : {286, 287}) {
        BitW w;
        w.put(1, 1); w.put(1, 2);
        fixed_lit(w, 'a');
        fixed_lit(w, s);
        w.code(0, 5);
        fixed_lit(w, 256);
        check("literal/length symbol 286 / 287", member_of(w, Bytes(1, 'a')), BI_E_LITLEN_SYM);
    }
    for (int s : {30, 31}) {
        BitW w;
        w.put(1, 1); w.put(1, 2);
        fixed_lit(w, 'a');
        fixed_lit(w, 257);
        w.code((uint32_t)s, 5);
        fixed_lit(w, 256);
        check("distance symbol 30 / 31", member_of(w, Bytes(4, 'a')), BI_E_DIST_SYM);
    }
    {
        BitW w;
        w.put(1, 1); w.put(1, 2);
        fixed_lit(w, 'a');
        fixed_lit(w, 257);
        w.code(1, 5);                                                          // distance 2 behind one byte
        fixed_lit(w, 256);
        check("a distance before the first byte", member_of(w, Bytes(4, 'a')), BI_E_DIST_FAR);
        BitW v;
        v.put(1, 1); v.put(1, 2);
        fixed_lit(v, 'a');
        fixed_lit(v, 257);
        v.code(0, 5);
        fixed_lit(v, 256);
        check("the same stream with distance 1", member_of(v, Bytes(4, 'a')), 0);
    }
    {
        Member m = deflate_member(text, 6, Z_DEFAULT_STRATEGY);
        Member cut = m;
        cut.isize -= 1;
        cut.crc = (uint32_t)crc32(0, text.data(), cut.isize);
        check("output beyond ISIZE", cut, BI_E_OUTPUT);
        Member more = m;
        more.isize += 1;
        check("fewer bytes than ISIZE", more, BI_E_ISIZE);
        Member crc = m;
        crc.crc ^= 0x00010000u;
        check("the CRC-32", crc, BI_E_CRC);
        Member shortm = m;
        shortm.payload.resize(m.payload.size() - 1);
        check("bits past the payload", shortm, BI_E_BITS);
        shortm.payload.resize(m.payload.size() / 2);
        check("half the payload", shortm, BI_E_BITS);
        shortm.payload.clear();
        check("no payload", shortm, BI_E_BITS);
        Member longm = m;
        longm.payload.push_back(0);
        check("a byte behind the stream", longm, BI_E_TRAILING);
        Member st = deflate_member(text, 0, Z_DEFAULT_STRATEGY);
        st.payload.resize(st.payload.size() - 7);
        check("a stored block cut short", st, BI_E_BITS);
    }
    {
        Hand h;                                                                // the unused half of a one-code distance tree
        h.llen['a'] = 1; h.llen[256] = 2; h.llen[257] = 2; h.hlit = 258; h.dlen[0] = 1; h.hdist = 1;
        h.header(1);
        h.lit('a'); h.lit(257); h.w.put(1, 1); h.lit(256); h.w.put(0, 16);                    // (16 more bits: the pattern is not cut short)
        check("the bit no distance code has", member_of(h.w, Bytes(4, 'a')), BI_E_CODE);
        Hand g;                                                                // a match where no distance code exists
        g.llen['a'] = 1; g.llen[256] = 2; g.llen[257] = 2; g.hlit = 258;
        g.header(1);
        g.lit('a'); g.lit(257); g.w.put(0, 1); g.lit(256); g.w.put(0, 16);
        check("a match without a distance code", member_of(g.w, Bytes(4, 'a')), BI_E_CODE);
    }
    // (d) the differential fuzz: a fixed seed, a fixed count
    const int before = g_cases;
    t = score_text(40);
    fuzz("level 6", deflate_member(t, 6, Z_DEFAULT_STRATEGY), nfuzz);
    fuzz("level 1", deflate_member(t, 1, Z_DEFAULT_STRATEGY), nfuzz);
    fuzz("fixed", deflate_member(t, 6, Z_FIXED), nfuzz);
    fuzz("huffman only", deflate_member(t, 6, Z_HUFFMAN_ONLY), nfuzz);
    fuzz("stored", deflate_member(t, 0, Z_DEFAULT_STRATEGY), nfuzz / 4);
    fuzz("full flush", deflate_member(t, 9, Z_DEFAULT_STRATEGY, 2000), nfuzz);
    {
        Bytes ft;
        uint32_t a = 1, b = 1;
        for (int s = 0; s < 19; ++s) { ft.insert(ft.end(), a, (unsigned char)('A' + s)); const uint32_t c = a + b; a = b; b = c; }
        for (size_t i = ft.size() - 1; i > 0; --i) std::swap(ft[i], ft[rnd() % (i + 1)]);
        fuzz("long codes", deflate_member(ft, 6, Z_HUFFMAN_ONLY), nfuzz);
    }
    fuzz("single distance code", single, nfuzz / 2);
    fuzz("no distance code", nodist, nfuzz / 2);
    printf("%d cases, %d of them mutations, %d wrong\n", g_cases, g_cases - before, g_bad);
    printf(g_bad ? "bgzf_inflate_check: FAILED\n" : "bgzf_inflate_check: ok\n");
    return g_bad ? 1 : 0;
}
