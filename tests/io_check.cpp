// Stand-alone host program: the native host I/O library (csrc/epg_io.cpp, through include/epilogos_io.h alone) against plain loops,
// printf and zlib -- an ordinary executable, so that the sanitizers can be linked into it.
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -pthread -Iinclude -Iepilogos_amd/csrc
//       tests/io_check.cpp epilogos_amd/csrc/epg_io.cpp -lz -o io_check && ./io_check DIR && ./io_check DIR --bgzf
//   (the same with -fsanitize=thread; and without a sanitizer but with -DIO_CHECK_FAIL_NEW)
// DIR takes the program's files.  --bgzf sets EPILOGOS_BGZF=1 before any thread exists and runs the writers and the census only.
// Readers: one table text as plain text, one- and three-member gzip, BGZF with and without its end marker, with CRLF line ends,
// without the final newline and empty, read with 1, 3, 16 and "shared" threads over five row ranges, into the table's own matrix and
// into a caller's wider one; the rows the parser must refuse.  Writers: scores, states and metrics around their chunk sizes, with 1
// and 5 threads at levels 0, 1 and 6, inflated member by member.  Helpers against loops; the census around a call.
// With -DIO_CHECK_FAIL_NEW the program replaces the global operator new by one that throws std::bad_alloc at the k-th allocation
// after arming and, after all the above, sweeps k = 1, 2, ... over every entry point that allocates or starts threads: each call
// succeeds with the right result or returns its failure value with a message, and the process lives.
// Exit code 0 and "io_check: ok" at the end; the first mismatch prints "io_check: FAILED ..." and exits with 1.
#include <dirent.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "epilogos_io.h"

#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("io_check: FAILED line %d: %s: ", __LINE__, #cond); \
            printf(__VA_ARGS__);                                      \
            printf("\n");                                             \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static std::string g_dir;
static bool g_bgzf = false;

static void lap(const char* what) {                               // how long each part took: the suite runs this program three times
    static struct timespec t0 = {0, 0};
    struct timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (t0.tv_sec) printf("io_check: %-12s %6.2f s\n", what, (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec));
    t0 = t1;
}

static std::string in_dir(const std::string& name) { return g_dir + "/" + name; }

static void write_file(const std::string& path, const std::string& data) {
    FILE* f = fopen(path.c_str(), "wb");
    CHECK(f != nullptr, "cannot create %s", path.c_str());
    CHECK(fwrite(data.data(), 1, data.size(), f) == data.size() && fclose(f) == 0, "cannot write %s", path.c_str());
}

static std::string read_file(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    CHECK(f != nullptr, "cannot open %s", path.c_str());
    std::string s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

// ---- zlib: what the files are made with and judged by --------------------------------------------------------------------------------
// one member: wbits 31 = gzip, -15 = raw deflate
static std::string deflate_all(const std::string& text, int wbits, int level = 6) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    CHECK(deflateInit2(&zs, level, Z_DEFLATED, wbits, 8, Z_DEFAULT_STRATEGY) == Z_OK, "deflateInit2");
    std::string out(deflateBound(&zs, (uLong)text.size()) + 64, '\0');
    zs.next_in = (Bytef*)text.data();
    zs.avail_in = (uInt)text.size();
    zs.next_out = (Bytef*)&out[0];
    zs.avail_out = (uInt)out.size();
    CHECK(deflate(&zs, Z_FINISH) == Z_STREAM_END, "deflate");
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

static const unsigned char BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static void put32(std::string& s, uint32_t v) {
    for (int i = 0; i < 4; ++i) s.push_back((char)(v >> (8 * i)));
}

static std::string bgzf_file(const std::string& text, size_t block, bool eof) {
    std::string out;
    for (size_t off = 0; off < text.size(); off += block) {
        const std::string piece = text.substr(off, block), raw = deflate_all(piece, -15);
        const size_t total = 18 + raw.size() + 8;
        CHECK(total <= 65536, "block too large");
        const unsigned char hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (unsigned char)((total - 1) & 0xff), (unsigned char)((total - 1) >> 8)};
        out.append((const char*)hdr, 18);
        out += raw;
        put32(out, (uint32_t)crc32(0L, (const Bytef*)piece.data(), (uInt)piece.size()));
        put32(out, (uint32_t)piece.size());
    }
    if (eof) out.append((const char*)BGZF_EOF, 28);
    return out;
}

// the text of a gzip file, member by member; members: every member's first byte and one entry for the end
static std::string gunzip(const std::string& file, std::vector<size_t>* members) {
    std::string text;
    std::vector<char> buf(1 << 20);
    size_t pos = 0;
    if (members) members->clear();
    while (pos < file.size()) {
        if (members) members->push_back(pos);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        CHECK(inflateInit2(&zs, 31) == Z_OK, "inflateInit2");
        zs.next_in = (Bytef*)file.data() + pos;
        zs.avail_in = (uInt)(file.size() - pos);
        int rc;
        do {
            zs.next_out = (Bytef*)buf.data();
            zs.avail_out = (uInt)buf.size();
            rc = inflate(&zs, Z_NO_FLUSH);
            CHECK(rc == Z_OK || rc == Z_STREAM_END, "member at byte %zu does not inflate (%d)", pos, rc);
            text.append(buf.data(), buf.size() - zs.avail_out);
        } while (rc != Z_STREAM_END);
        pos += zs.total_in;
        inflateEnd(&zs);
    }
    if (members) members->push_back(pos);
    return text;
}

// ---- the census ----------------------------------------------------------------------------------------------------------------------
static void census_reset() { epgio_thread_census(nullptr, nullptr, 1); }
static void census_check(const char* what, int T) {
    int32_t live = -1, peak = -1;
    epgio_thread_census(&live, &peak, 0);
    CHECK(live == 0, "%s: %d threads still counted after the call", what, live);
    CHECK(peak >= 1 && peak <= T, "%s: peak %d with %d threads (the waiting caller does not count)", what, peak, T);
}

// ---- the reader's reference: a plain loop over the text ------------------------------------------------------------------------------
struct Ref {
    int64_t rows = 0;
    int cols = 0;
    std::vector<long> val;             // [rows * cols], as written
    std::vector<std::string> loc;      // "chr\tstart\tend\n"
};

static Ref reference_parse(const std::string& text) {
    Ref ref;
    size_t p = 0;
    for (;;) {
        const size_t nl = text.find('\n', p);
        if (nl == std::string::npos) break;                       // a dangling last line does not exist
        std::string line = text.substr(p, nl - p);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        size_t at = 0;
        for (int k = 0; k < 3; ++k) at = line.find('\t', at) + 1;
        ref.loc.push_back(line.substr(0, at - 1) + "\n");
        int n = 0;
        const char* q = line.c_str() + at;
        for (;;) {
            char* e = nullptr;
            ref.val.push_back(strtol(q, &e, 10));
            CHECK(e != q, "the program's own text has a bad value in row %lld", (long long)ref.rows);
            ++n;
            if (*e != '\t') break;
            q = e + 1;
        }
        if (ref.rows == 0) ref.cols = n;
        CHECK(n == ref.cols, "the program's own text has a ragged row");
        ++ref.rows;
        p = nl + 1;
    }
    return ref;
}

static std::string table_text(int R, int N, const char* eol) {
    static const int special[] = {0, 31, 32, 100, -3, 127, 128, 1, 30};
    std::string s;
    char num[64];
    for (int r = 0; r < R; ++r) {
        snprintf(num, sizeof num, "chr%d\t%d\t%d", 1 + r * 3 / R, r * 200, r * 200 + 200);
        s += num;
        for (int c = 0; c < N; ++c) {
            const uint32_t x = rnd();
            snprintf(num, sizeof num, "\t%d", x % 16 == 0 ? special[(x >> 8) % 9] : 1 + (int)((x >> 8) % 30));
            s += num;
        }
        s += eol;
    }
    return s;
}

struct Dest {                                                     // a caller's destination, wider than the rows
    std::vector<int8_t> buf;
    int64_t pitch = 0;
    int extra = 3;
};
static int8_t* dest_alloc(int64_t rows, int32_t cols, int64_t* ldx, void* user) {
    Dest* d = (Dest*)user;
    d->pitch = cols + d->extra;
    if ((size_t)(rows * d->pitch + 1) > d->buf.size()) return nullptr;     // (sized before the call: nothing is allocated in here)
    memset(d->buf.data(), 0x55, d->buf.size());
    *ldx = d->pitch;
    return d->buf.data();
}

// the table t against rows [lo, hi) of ref (already clipped); dest: where the states were parsed into, or nullptr
static void check_table(const char* what, epgio_table* t, const Ref& ref, int64_t lo, int64_t hi, int max_state, const Dest* dest) {
    CHECK(t != nullptr, "%s: %s", what, epgio_last_error());
    const int64_t rows = hi - lo;
    CHECK(epgio_table_rows(t) == rows, "%s: %lld rows, want %lld", what, (long long)epgio_table_rows(t), (long long)rows);
    if (ref.rows == 0) {
        const int64_t* off = nullptr;
        epgio_table_locations(t, &off);
        CHECK(epgio_table_cols(t) == 0 && off && off[0] == 0, "%s: the empty table", what);
        return;
    }
    const int cols = ref.cols, max0 = (max_state > 31 ? 127 : 31) - 1;
    CHECK(epgio_table_cols(t) == cols, "%s: %d columns, want %d", what, epgio_table_cols(t), cols);
    const int64_t pitch = dest ? dest->pitch : cols + 2;
    std::vector<int8_t> own;
    const int8_t* got = dest ? dest->buf.data() : nullptr;
    if (dest) CHECK(epgio_table_copy_states(t, (int8_t*)dest->buf.data(), pitch) == 0, "%s: copy_states of a caller's destination", what);
    else {
        own.assign((size_t)(rows * pitch) + 1, 0x55);
        CHECK(epgio_table_copy_states(t, own.data(), pitch) == 0, "%s: copy_states: %s", what, epgio_last_error());
        got = own.data();
    }
    const int64_t* off = nullptr;
    const char* loc = epgio_table_locations(t, &off);
    CHECK(off != nullptr && off[0] == 0, "%s: offsets", what);
    long vlo = 0, vhi = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const std::string& want = ref.loc[(size_t)(lo + r)];
        CHECK(off[r + 1] - off[r] == (int64_t)want.size() && memcmp(loc + off[r], want.data(), want.size()) == 0, "%s: location of row %lld", what, (long long)r);
        for (int c = 0; c < cols; ++c) {
            const long v = ref.val[(size_t)((lo + r) * cols + c)];
            if (r == 0 && c == 0) vlo = vhi = v;
            vlo = v < vlo ? v : vlo;
            vhi = v > vhi ? v : vhi;
            const int want_state = v - 1 < 0 || v - 1 > max0 ? -1 : (int)(v - 1);
            CHECK(got[r * pitch + c] == want_state, "%s: row %lld column %d: %d, want %d (written %ld)", what, (long long)r, c, got[r * pitch + c], want_state, v);
        }
        for (int64_t c = cols; c < pitch; ++c) CHECK((unsigned char)got[r * pitch + c] == 0xff, "%s: pad byte %lld of row %lld", what, (long long)c, (long long)r);
    }
    CHECK((unsigned char)got[rows * pitch] == 0x55, "%s: a byte behind the last row was written", what);
    int32_t slo = -7, shi = -7;
    CHECK(epgio_table_state_range(t, &slo, &shi) == 0 && slo == vlo && shi == vhi, "%s: state range %d..%d, want %ld..%ld", what, slo, shi, vlo, vhi);
}

static void clip(const Ref& ref, int64_t& lo, int64_t& hi) {
    if (hi < 0 || hi > ref.rows) hi = ref.rows;
    if (lo < 0) lo = 0;
    if (lo > hi) lo = hi;
}

static void check_readers(int R, int N, bool all_forms) {
    const std::string text = table_text(R, N, "\n"), crlf = table_text(R, N, "\r\n"), cut = text.substr(0, text.size() - 1);
    struct Form { std::string name, file; const std::string* text; };
    std::vector<Form> forms;
    char tag[64];
    snprintf(tag, sizeof tag, "t%d_", N);
    forms.push_back({"plain.txt", text, &text});
    forms.push_back({"one.txt.gz", deflate_all(text, 31), &text});
    if (all_forms) {
        const size_t a = text.size() / 3, b = 2 * text.size() / 3;
        forms.push_back({"three.txt.gz", deflate_all(text.substr(0, a), 31, 1) + deflate_all(text.substr(a, b - a), 31, 9) + deflate_all(text.substr(b), 31), &text});
        forms.push_back({"bgzf.txt.gz", bgzf_file(text, 1024, true), &text});
        forms.push_back({"bgzf_noeof.txt.gz", bgzf_file(text, 65280, false), &text});
        forms.push_back({"crlf.txt", crlf, &crlf});
        forms.push_back({"crlf.txt.gz", deflate_all(crlf, 31), &crlf});
        forms.push_back({"cut.txt", cut, &cut});
        forms.push_back({"cut.txt.gz", bgzf_file(cut, 1024, true), &cut});
        forms.push_back({"empty.txt", "", nullptr});
    }
    const std::string empty;
    Dest dest;
    dest.buf.resize((size_t)R * (N + dest.extra) + 1);
    const int thread_counts[] = {1, 3, 16, 0};
    for (const Form& f : forms) {
        const std::string path = in_dir(tag + f.name);
        write_file(path, f.file);
        const Ref ref = reference_parse(f.text ? *f.text : empty);
        CHECK(ref.rows == (f.text == &cut ? R - 1 : f.text ? R : 0), "the program's own parse of %s", f.name.c_str());
        CHECK(epgio_count_rows(path.c_str()) == ref.rows, "%s: count_rows", f.name.c_str());
        const int64_t ranges[5][2] = {{0, -1}, {0, 0}, {1, ref.rows - 1}, {ref.rows - 1, ref.rows}, {ref.rows, ref.rows + 5}};
        for (int threads : thread_counts)
            for (const auto& range : ranges) {
                int64_t lo = range[0], hi = range[1];
                clip(ref, lo, hi);
                char what[256];
                snprintf(what, sizeof what, "%s%s threads %d rows [%lld, %lld)", tag, f.name.c_str(), threads, (long long)range[0], (long long)range[1]);
                if (threads == 0) epgio_set_reader_plan(4);
                census_reset();
                epgio_table* t = epgio_open_table(path.c_str(), range[0], range[1], threads);
                if (threads > 0) census_check(what, threads);
                check_table(what, t, ref, lo, hi, 31, nullptr);
                epgio_close_table(t);
                t = epgio_open_table_into(path.c_str(), range[0], range[1], threads, 127, dest_alloc, &dest);
                check_table(what, t, ref, lo, hi, 127, ref.rows ? &dest : nullptr);
                epgio_close_table(t);
                epgio_set_reader_plan(0);
            }
        // the whole text, as the GPU parsers are fed it
        epgio_text* h = epgio_open_text(path.c_str(), 3);
        CHECK(h != nullptr, "%s: open_text: %s", f.name.c_str(), epgio_last_error());
        int64_t size = -1;
        const char* data = epgio_text_data(h, &size);
        const std::string& want = f.text ? *f.text : empty;
        CHECK(size == (int64_t)want.size() && (size == 0 || memcmp(data, want.data(), want.size()) == 0), "%s: open_text: %lld bytes, want %zu", f.name.c_str(), (long long)size, want.size());
        epgio_close_text(h);
    }
    epgio_table* t = epgio_open_table_ex(in_dir(tag + std::string("plain.txt")).c_str(), 0, -1, 2, 127);
    const Ref ref = reference_parse(text);
    check_table("own matrix, wide model", t, ref, 0, ref.rows, 127, nullptr);
    epgio_close_table(t);
}

static void check_malformed() {
    const char* bad[] = {"chr1\t1400\t1600\t3\t1.5\t7\t2\n", "chr1\t1400\t1600\t3\t1x5\t7\t2\n", "chr1\t1400\t1600\t3\t1 5\t7\t2\n", "chr1\t1400\t1600\t3\t4\t7\n",
                         "chr1\t1400\t1600\t3\t4\t7\t2\t9\n", "\t\t\n"};
    for (size_t k = 0; k < sizeof bad / sizeof bad[0]; ++k) {
        std::string text;
        char row[64];
        for (int r = 0; r < 12; ++r) {
            snprintf(row, sizeof row, "chr1\t%d\t%d\t3\t14\t7\t2\n", r * 200, r * 200 + 200);
            text += r == 7 ? bad[k] : row;
        }
        const std::string path = in_dir("malformed.txt");
        write_file(path, text);
        for (int threads : {1, 3})
            for (int64_t lo : {0, 2, 7}) {
                epgio_table* t = epgio_open_table(path.c_str(), lo, -1, threads);
                CHECK(t == nullptr, "malformed row %zu was read (threads %d, from row %lld)", k, threads, (long long)lo);
                CHECK(strstr(epgio_last_error(), "malformed line at row 7 ") != nullptr, "malformed row %zu: message `%s`", k, epgio_last_error());
            }
        epgio_table* t = epgio_open_table(path.c_str(), 8, -1, 3);            // the bad row is not among those asked for
        CHECK(t != nullptr && epgio_table_rows(t) == 4, "rows behind malformed row %zu", k);
        epgio_close_table(t);
    }
    write_file(in_dir("narrow.txt"), "chr1\t0\t200\nchr1\t200\t400\n");
    CHECK(epgio_open_table(in_dir("narrow.txt").c_str(), 0, -1, 2) == nullptr && strstr(epgio_last_error(), "found 3") != nullptr, "a file without state columns");
    CHECK(epgio_open_table(in_dir("missing.txt").c_str(), 0, -1, 2) == nullptr && strstr(epgio_last_error(), "cannot open") != nullptr, "a missing file");
}

// ---- the writers ---------------------------------------------------------------------------------------------------------------------
static const float SPECIAL[] = {-0.0f, 1e-6f, -1e-6f, 0.000005f, 123456.789f, 2147483520.0f, 0.0f, -2147483520.0f, 0.5f, -1.0f};

static float some_float(int64_t i) {
    if (i % 7 == 0) return SPECIAL[(i / 7) % 10];
    return ((int)(rnd() % 2000001) - 1000000) * 3e-6f;
}

// the written file against the text; BGZF: every member at most 64 KiB with its BC subfield, the end marker once, at the end
static void check_file(const char* what, const std::string& path, const std::string& file, const std::string& want, bool compressed, int64_t chunks) {
    if (!compressed) {
        CHECK(file == want, "%s: the plain file differs", what);
        return;
    }
    std::vector<size_t> members;
    const std::string text = gunzip(file, &members);
    CHECK(text == want, "%s: %zu bytes of text, want %zu", what, text.size(), want.size());
    const size_t n = members.size() - 1;
    if (!g_bgzf) {
        CHECK((int64_t)n == (chunks ? chunks : 1), "%s: %zu members, want %lld", what, n, (long long)(chunks ? chunks : 1));
        return;
    }
    const bool gz = path.size() >= 2 && path.compare(path.size() - 2, 2, "gz") == 0;
    size_t markers = 0;
    for (size_t k = 0; k < n; ++k) {
        const unsigned char* h = (const unsigned char*)file.data() + members[k];
        const size_t len = members[k + 1] - members[k];
        CHECK(len <= 65536 && len >= 28 && h[3] == 4 && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0 &&
                  (size_t)(h[16] | h[17] << 8) + 1 == len, "%s: member %zu is not a BGZF block", what, k);
        if (len == 28 && memcmp(h, BGZF_EOF, 28) == 0) {
            ++markers;
            CHECK(k == n - 1, "%s: an end marker in the middle", what);
        }
    }
    CHECK(markers == (gz ? 1u : 0u), "%s: %zu end markers", what, markers);
}

struct Scores {
    int64_t R;
    int S;
    std::string loc, want;
    std::vector<int64_t> off;
    std::vector<float> v;
    Scores(int64_t R_, int S_) : R(R_), S(S_), off(1, 0), v((size_t)(R_ * S_)) {
        char num[400];
        for (int64_t r = 0; r < R; ++r) {
            snprintf(num, sizeof num, "c%d\t%lld\t%lld", (int)(r % 3), (long long)r, (long long)r + 1);
            loc += num;
            loc += '\n';
            off.push_back((int64_t)loc.size());
            want += num;
            for (int s = 0; s < S; ++s) {
                const float f = v[(size_t)(r * S + s)] = some_float(r * S + s);
                snprintf(num, sizeof num, "\t%.5f", (double)f);
                want += num;
            }
            want += '\n';
        }
    }
    int write(const std::string& path, int threads, int level) const { return epgio_write_scores(path.c_str(), loc.data(), off.data(), v.data(), R, S, threads, level); }
};

struct States {
    int64_t R;
    int N;
    int64_t pitch;
    std::string want;
    std::vector<int8_t> x;
    States(int64_t R_, int N_) : R(R_), N(N_), pitch(N_ + 2), x((size_t)(R_ * (N_ + 2)) + 1, 0x55) {
        char num[64];
        for (int64_t r = 0; r < R; ++r) {
            snprintf(num, sizeof num, "chrX\t%lld\t%lld", (long long)(1000 + r * 200), (long long)(1000 + (r + 1) * 200));
            want += num;
            for (int c = 0; c < N; ++c) {
                const uint32_t u = rnd();
                const int8_t s = x[(size_t)(r * pitch + c)] = (int8_t)(u % 16 == 0 ? (int)(u >> 8) % 256 - 128 : (int)(u >> 8) % 30);
                snprintf(num, sizeof num, "\t%d", (int)s + 1);
                want += num;
            }
            want += '\n';
        }
    }
    int write(const std::string& path, int threads, int level) const { return epgio_write_states(path.c_str(), "chrX", 1000, 200, x.data(), R, N, pitch, threads, level); }
};

struct Metrics {
    int64_t R;
    bool pv;
    std::string chrom = "c1c10X", names = "TssAQuiesEnh", want;
    std::vector<int64_t> chrom_off = {0, 2, 5, 6}, names_off = {0, 4, 9, 12}, start, end;
    std::vector<int32_t> ci, md;
    std::vector<float> dist;
    std::vector<double> p, mh;
    Metrics(int64_t R_, bool pv_) : R(R_), pv(pv_) {
        char num[400];
        for (int64_t r = 0; r < R; ++r) {
            ci.push_back((int32_t)(r * 3 / (R ? R : 1)));
            md.push_back(1 + (int32_t)(rnd() % 3));
            start.push_back(r * 200);
            end.push_back(r * 200 + 200);
            dist.push_back(some_float(r));
            p.push_back(r % 5 == 0 ? 1.0 : (rnd() % 100000) * 1e-9);
            mh.push_back(r % 11 == 0 ? 0.0 : (rnd() % 100000) * 1e-5);
            const float d = dist.back();
            snprintf(num, sizeof num, "%s\t%lld\t%lld\t%s\t%.5f\t%c", chrom.substr((size_t)chrom_off[ci.back()], (size_t)(chrom_off[ci.back() + 1] - chrom_off[ci.back()])).c_str(),
                     (long long)start.back(), (long long)end.back(), names.substr((size_t)names_off[md.back() - 1], (size_t)(names_off[md.back()] - names_off[md.back() - 1])).c_str(),
                     (double)fabsf(d), d >= 0.0f ? '+' : '-');
            want += num;
            if (pv) {
                snprintf(num, sizeof num, "\t%.5e\t%.5e", p.back(), mh.back());
                want += num;
            }
            want += '\n';
        }
    }
    int write(const std::string& path, int threads, int level) const {
        return epgio_write_metrics(path.c_str(), chrom.data(), chrom_off.data(), ci.data(), start.data(), end.data(), names.data(), names_off.data(), md.data(), dist.data(),
                                   pv ? p.data() : nullptr, pv ? mh.data() : nullptr, R, threads, level);
    }
};

// one writer at one size: 1 and 5 threads, levels 0, 1 and 6; the two thread counts give the same bytes
template <class W>
static void check_writer(const char* kind, const W& w, const std::string& name, bool compressed, int64_t CH) {
    const int64_t chunks = (w.R + CH - 1) / CH;
    for (int level : {0, 1, 6}) {
        std::string first;
        for (int threads : {1, 5}) {
            char what[256];
            snprintf(what, sizeof what, "%s %s: %lld rows, level %d, threads %d%s", kind, name.c_str(), (long long)w.R, level, threads, g_bgzf ? ", BGZF" : "");
            const std::string path = in_dir(name);
            census_reset();
            CHECK(w.write(path, threads, level) == 0, "%s: %s", what, epgio_last_error());
            census_check(what, threads);
            const std::string file = read_file(path);
            check_file(what, path, file, w.want, compressed, chunks);
            if (threads == 1) first = file;
            else CHECK(file == first, "%s: not the bytes that one thread writes", what);
        }
    }
}

static void check_writers() {
    const int64_t CH = 32768, CHS = 8192;
    for (int64_t R : {(int64_t)0, (int64_t)1, CH - 1, CH, CH + 1, 2 * CH + 5}) {
        check_writer("scores", Scores(R, 1), "scores.txt.gz", true, CH);
        check_writer("metrics", Metrics(R, R == 1 || R == CH), "metrics.txt.gz", true, CH);
    }
    check_writer("metrics", Metrics(CH + 1, true), "metrics_p.txt.gz", true, CH);
    check_writer("scores", Scores(700, 18), "scores_no_suffix.txt", true, CH);     // compressed whatever the name; BGZF: no end marker
    // (6 CHS + 5 rows: seven chunks, two rounds of five threads)
    for (int64_t R : {(int64_t)0, (int64_t)1, CHS - 1, CHS, CHS + 1, 2 * CHS + 5, 6 * CHS + 5}) {
        check_writer("states", States(R, 5), "states.txt.gz", true, CHS);
        check_writer("states", States(R, 5), "states.txt", false, CHS);
    }
    check_writer("states", States(300, 61), "states61.txt.gz", true, CHS);
    // what the writer wrote, the reader reads
    const States s(CHS + 1, 7);
    CHECK(s.write(in_dir("round.txt.gz"), 3, 0) == 0, "write_states: %s", epgio_last_error());
    const Ref ref = reference_parse(s.want);
    epgio_table* t = epgio_open_table_ex(in_dir("round.txt.gz").c_str(), 0, -1, 3, 127);
    check_table("the writer's file read back", t, ref, 0, ref.rows, 127, nullptr);
    epgio_close_table(t);
}

// ---- the helpers ---------------------------------------------------------------------------------------------------------------------
struct LocText {
    std::string loc;
    std::vector<int64_t> off, start, end;
    explicit LocText(int64_t R, bool one_chrom = true) : off(1, 0) {
        char row[96];
        for (int64_t r = 0; r < R; ++r) {
            start.push_back(r % 1000 == 3 ? -(r * 200) : r * 200);
            end.push_back(r * 200 + 200);
            snprintf(row, sizeof row, "%s\t%lld\t%lld%s\n", one_chrom || r < R - 1 ? "chr12" : "chr13", (long long)start[(size_t)r], (long long)end[(size_t)r], r % 5 == 0 ? "\r" : "");
            loc += row;
            off.push_back((int64_t)loc.size());
        }
    }
};

static float row_sum(const float* p, int S) {                     // numpy's order for a contiguous row (epilogos_io.h)
    if (S < 8) {
        float res = 0.f;
        for (int i = 0; i < S; ++i) res += p[i];
        return res;
    }
    float q[8];
    const int n8 = S - S % 8;
    for (int j = 0; j < 8; ++j) q[j] = p[j];
    for (int i = 8; i < n8; i += 8)
        for (int j = 0; j < 8; ++j) q[j] += p[i + j];
    float res = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    for (int i = n8; i < S; ++i) res += p[i];
    return res;
}

static void check_helpers() {
    for (int64_t R : {(int64_t)0, (int64_t)1, (int64_t)777, (int64_t)140000})
        for (int threads : {1, 4}) {
            const LocText lt(R);
            std::vector<int64_t> start((size_t)R + 1, -7), end((size_t)R + 1, -7);
            int32_t same = -1;
            census_reset();
            CHECK(epgio_parse_locations(lt.loc.data(), lt.off.data(), R, start.data(), end.data(), &same, threads) == 0, "parse_locations: %s", epgio_last_error());
            census_check("parse_locations", threads);
            start.pop_back();
            end.pop_back();
            CHECK(start == lt.start && end == lt.end && same == 1, "parse_locations: %lld rows, %d threads", (long long)R, threads);
        }
    {
        const LocText two(140000, false);
        std::vector<int64_t> start(140000), end(140000);
        int32_t same = -1;
        CHECK(epgio_parse_locations(two.loc.data(), two.off.data(), 140000, start.data(), end.data(), &same, 4) == 0 && same == 0 && end == two.end, "parse_locations: two names");
        LocText bad(140000);
        bad.loc[(size_t)bad.off[139000] + 6] = '.';
        CHECK(epgio_parse_locations(bad.loc.data(), bad.off.data(), 140000, start.data(), end.data(), &same, 4) == -1 && epgio_last_error()[0], "parse_locations: a float must be refused");
    }
    for (int S : {5, 18, 61})
        for (int64_t R : {(int64_t)1, (int64_t)(S == 18 ? 140000 : 66000)})
            for (int threads : {1, 4}) {
                const int64_t lda = S + 3;
                std::vector<float> a((size_t)(R * lda)), out((size_t)R + 1, -7.f);
                for (size_t i = 0; i < a.size(); ++i) a[i] = some_float((int64_t)i);
                census_reset();
                CHECK(epgio_row_sums_f32(a.data(), R, S, lda, out.data(), threads) == 0, "row_sums: %s", epgio_last_error());
                census_check("row_sums", threads);
                for (int64_t r = 0; r < R; ++r) {
                    const float want = row_sum(a.data() + r * lda, S);
                    CHECK(memcmp(&out[(size_t)r], &want, 4) == 0, "row_sums: row %lld of %lld, S %d: %a, want %a", (long long)r, (long long)R, S, out[(size_t)r], want);
                }
                CHECK(out[(size_t)R] == -7.f, "row_sums wrote behind its output");
            }
    for (int64_t n : {(int64_t)5, (int64_t)3000, (int64_t)2200000})
        for (int W : {1, 4, 7, 50}) {
            if (W == 50 && n > 3000) continue;                    // (the loop below is n * W)
            std::vector<double> x((size_t)n), one((size_t)n, -7.0), four((size_t)n, -7.0);
            for (auto& v : x) v = (double)(rnd() % 1000);
            CHECK(epgio_rolling_max_f64(x.data(), n, W, one.data(), 1) == 0, "rolling_max: %s", epgio_last_error());
            census_reset();
            CHECK(epgio_rolling_max_f64(x.data(), n, W, four.data(), 4) == 0, "rolling_max: %s", epgio_last_error());
            census_check("rolling_max", 4);
            CHECK(memcmp(one.data(), four.data(), (size_t)n * 8) == 0, "rolling_max: 1 and 4 threads differ (n %lld, W %d)", (long long)n, W);
            for (int64_t i = 0; i < n; ++i) {
                const int64_t lo = i - W / 2, hi = i + (W - 1) / 2;
                if (lo < 0 || hi >= n) { CHECK(std::isnan(one[(size_t)i]), "rolling_max: element %lld of %lld, W %d, is not NaN", (long long)i, (long long)n, W); continue; }
                double m = x[(size_t)lo];
                for (int64_t k = lo + 1; k <= hi; ++k) m = x[(size_t)k] > m ? x[(size_t)k] : m;
                CHECK(one[(size_t)i] == m, "rolling_max: element %lld of %lld, W %d: %g, want %g", (long long)i, (long long)n, W, one[(size_t)i], m);
            }
        }
    std::string big((size_t)17 << 20, 'x');
    int64_t want = 0;
    for (size_t i = 0; i < big.size(); i += 1 + rnd() % 150) { big[i] = '\n'; ++want; }
    for (size_t i : {big.size() - 1, (size_t)17 << 19, ((size_t)17 << 19) - 1})                          // the end, the pieces' border
        if (big[i] != '\n') { big[i] = '\n'; ++want; }
    for (int threads : {1, 4}) {
        census_reset();
        CHECK(epgio_count_newlines(big.data(), (int64_t)big.size(), threads) == want, "count_newlines with %d threads", threads);
        census_check("count_newlines", threads);
    }
    want = 0;
    for (int i = 0; i < 1000; ++i) want += big[(size_t)i] == '\n';
    CHECK(epgio_count_newlines(big.data(), 1000, 4) == want && epgio_count_newlines(big.data(), 0, 4) == 0, "count_newlines of a short text");
    const std::string text = table_text(500, 9, "\n");
    std::string z(text.size() + text.size() / 8 + 1100, '\0');
    const int64_t zn = epgio_gzip_fast(text.data(), (int64_t)text.size(), &z[0], (int64_t)z.size());
    CHECK(zn > 0, "gzip_fast: %s", epgio_last_error());
    z.resize((size_t)zn);
    CHECK(gunzip(z, nullptr) == text, "gzip_fast does not inflate to its input");
}

#ifdef IO_CHECK_FAIL_NEW
// ---- operator new that fails on demand -----------------------------------------------------------------------------------------------
static std::atomic<bool> g_armed{false};
static std::atomic<long> g_left{0};
static std::atomic<int> g_fired{0}, g_fired_late{0};
static pthread_t g_main;

static int dir_entries(const char* path) {
    DIR* d = opendir(path);
    if (!d) return -1;
    int n = 0;
    while (readdir(d)) ++n;
    closedir(d);
    return n;
}

static void* new_or_throw(size_t n) {
    if (g_armed.load() && g_left.fetch_sub(1) == 1) {
        g_fired.store(1);
        // after the first worker had started: thrown on a worker, or on the caller while a worker was there (a worker that has
        // come and gone already is not seen: this undercounts, it never overcounts)
        if (!pthread_equal(pthread_self(), g_main) || dir_entries("/proc/self/task") > 3) g_fired_late.store(1);
        throw std::bad_alloc();
    }
    void* p = malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void* operator new(size_t n) { return new_or_throw(n); }
void* operator new[](size_t n) { return new_or_throw(n); }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }

// k = 1, 2, ... -- no k below the first success is left out -- until a call completes without the failure firing.  run() makes the
// call and nothing else (no allocation of the program's own while armed) and says whether it succeeded; check() judges and
// releases the result of a call that did.
template <class Run, class Check>
static void sweep(const char* entry, bool multi, Run&& run, Check&& check) {
    int failed = 0, succeeded = 0, late = 0;
    for (long k = 1;; ++k) {
        CHECK(k < 100000, "%s: the sweep does not end", entry);
        const int fds = dir_entries("/proc/self/fd");
        census_reset();
        g_fired.store(0);
        g_fired_late.store(0);
        g_left.store(k);
        g_armed.store(true);
        const bool ok = run();
        g_armed.store(false);
        int32_t live = -1;
        epgio_thread_census(&live, nullptr, 0);
        CHECK(live == 0, "%s: k = %ld: %d threads still counted", entry, k, live);
        if (ok) {
            check();
            ++succeeded;
        } else {
            CHECK(g_fired.load(), "%s: k = %ld: failed with no allocation refused: %s", entry, k, epgio_last_error());
            CHECK(epgio_last_error()[0] != 0, "%s: k = %ld: failure without a message", entry, k);
            ++failed;
            late += g_fired_late.load();
            CHECK(dir_entries("/proc/self/fd") == fds, "%s: k = %ld: a file handle was leaked", entry, k);
            CHECK(run(), "%s: k = %ld: the call after the failed one: %s", entry, k, epgio_last_error());
            check();
        }
        if (!g_fired.load()) break;
    }
    printf("io_check: sweep %s: %d failed, %d succeeded, %d after the first worker had started\n", entry, failed, succeeded, late);
    CHECK(failed >= 1 && succeeded >= 1, "%s: the sweep saw %d failures and %d successes", entry, failed, succeeded);
    if (multi) CHECK(late >= 1, "%s: no failure fell after the first worker had started", entry);
}

static void check_failing_new() {
    g_main = pthread_self();
    const int T = 4;
    const std::string text = table_text(3000, 9, "\n");
    const Ref ref = reference_parse(text);
    const std::string plain = in_dir("sweep.txt"), three = in_dir("sweep3.txt.gz"), blocks = in_dir("sweep_bgzf.txt.gz");
    write_file(plain, text);
    write_file(three, deflate_all(text.substr(0, 1000), 31) + deflate_all(text.substr(1000, 5000), 31) + deflate_all(text.substr(6000), 31));
    write_file(blocks, bgzf_file(text, 2048, true));
    epgio_table* t = nullptr;
    sweep("epgio_open_table_ex", true, [&] { return (t = epgio_open_table_ex(plain.c_str(), 1, -1, T, 31)) != nullptr; },
          [&] { check_table("sweep: open_table_ex", t, ref, 1, ref.rows, 31, nullptr); epgio_close_table(t); });
    Dest dest;
    dest.buf.resize((size_t)ref.rows * (ref.cols + dest.extra) + 1);
    sweep("epgio_open_table_into", true, [&] { return (t = epgio_open_table_into(blocks.c_str(), 0, -1, T, 127, dest_alloc, &dest)) != nullptr; },
          [&] { check_table("sweep: open_table_into", t, ref, 0, ref.rows, 127, &dest); epgio_close_table(t); });
    epgio_text* h = nullptr;
    // (a refused allocation in the BGZF block workers is no failure of the call: the general reader takes the file and succeeds)
    for (const std::string* path : {&blocks, &three})
        sweep(path == &blocks ? "epgio_open_text (BGZF)" : "epgio_open_text (gzip)", false, [&] { return (h = epgio_open_text(path->c_str(), T)) != nullptr; }, [&] {
            int64_t size = -1;
            const char* data = epgio_text_data(h, &size);
            CHECK(size == (int64_t)text.size() && memcmp(data, text.data(), text.size()) == 0, "sweep: open_text");
            epgio_close_text(h);
        });
    // (levels 1..9 compress in zlib, which does not allocate through operator new; the states go through the library's own compressor)
    const Scores sc(32768 + 1, 2);
    const States st(2 * 8192 + 5, 5);
    const Metrics me(32768 + 1, true);
    const std::string out = in_dir("sweep_out.txt.gz"), out_plain = in_dir("sweep_out.txt");
    sweep("epgio_write_scores", true, [&] { return sc.write(out, T, 1) == 0; }, [&] { check_file("sweep: write_scores", out, read_file(out), sc.want, true, 2); });
    sweep("epgio_write_states", true, [&] { return st.write(out, T, 0) == 0; }, [&] { check_file("sweep: write_states", out, read_file(out), st.want, true, 3); });
    sweep("epgio_write_states (plain)", true, [&] { return st.write(out_plain, T, 1) == 0; }, [&] { check_file("sweep: write_states", out_plain, read_file(out_plain), st.want, false, 3); });
    sweep("epgio_write_metrics", true, [&] { return me.write(out, T, 1) == 0; }, [&] { check_file("sweep: write_metrics", out, read_file(out), me.want, true, 2); });
    const LocText lt(200000);
    std::vector<int64_t> start(200000), end(200000);
    sweep("epgio_parse_locations", true, [&] { return epgio_parse_locations(lt.loc.data(), lt.off.data(), 200000, start.data(), end.data(), nullptr, T) == 0; },
          [&] { CHECK(start == lt.start && end == lt.end, "sweep: parse_locations"); start.assign(200000, -7); });
    std::vector<float> a(200000 * 18), sums(200000);
    for (size_t i = 0; i < a.size(); ++i) a[i] = some_float((int64_t)i);
    sweep("epgio_row_sums_f32", true, [&] { return epgio_row_sums_f32(a.data(), 200000, 18, 18, sums.data(), T) == 0; }, [&] {
        for (int64_t r = 0; r < 200000; ++r) CHECK(sums[(size_t)r] == row_sum(a.data() + r * 18, 18), "sweep: row_sums row %lld", (long long)r);
        sums.assign(200000, -7.f);
    });
    std::vector<double> x(2200000), mx(2200000);
    for (auto& v : x) v = (double)(rnd() % 1000);
    sweep("epgio_rolling_max_f64", true, [&] { return epgio_rolling_max_f64(x.data(), 2200000, 3, mx.data(), T) == 0; }, [&] {
        for (int64_t i = 1; i + 1 < 2200000; ++i) CHECK(mx[(size_t)i] == std::max(x[(size_t)i - 1], std::max(x[(size_t)i], x[(size_t)i + 1])), "sweep: rolling_max element %lld", (long long)i);
        CHECK(std::isnan(mx[0]) && std::isnan(mx[2199999]), "sweep: rolling_max ends");
        mx.assign(2200000, -7.0);
    });
    std::string big((size_t)33 << 20, 'x');                       // four pieces of 8 MiB: four workers
    for (size_t i = 0; i < big.size(); i += 4099) big[i] = '\n';
    const int64_t lines = (int64_t)((big.size() + 4098) / 4099);
    int64_t got = -1;
    sweep("epgio_count_newlines", true, [&] { return (got = epgio_count_newlines(big.data(), (int64_t)big.size(), T)) >= 0; }, [&] { CHECK(got == lines, "sweep: count_newlines"); });
    std::string z(text.size() + text.size() / 8 + 1100, '\0'), inflated;
    sweep("epgio_gzip_fast", false, [&] { return (got = epgio_gzip_fast(text.data(), (int64_t)text.size(), &z[0], (int64_t)z.size())) > 0; },
          [&] { CHECK(gunzip(z.substr(0, (size_t)got), nullptr) == text, "sweep: gzip_fast"); });
}
#endif

int main(int argc, char** argv) {
    if (argc < 2) {
        printf("usage: io_check DIR [--bgzf]\n");
        return 2;
    }
    g_dir = argv[1];
    g_bgzf = argc > 2 && strcmp(argv[2], "--bgzf") == 0;
    if (g_bgzf) setenv("EPILOGOS_BGZF", "1", 1);                  // before the first thread: the writers' workers read it
    else unsetenv("EPILOGOS_BGZF");
    setvbuf(stdout, nullptr, _IOLBF, 0);
    lap("start");
    if (!g_bgzf) {
        check_readers(1500, 13, true);
        check_readers(600, 61, false);
        check_readers(2000, 5, false);
        check_malformed();
        lap("readers");
        check_helpers();
        lap("helpers");
    }
    check_writers();
    lap("writers");
#ifdef IO_CHECK_FAIL_NEW
    if (!g_bgzf) check_failing_new();
    lap("sweeps");
#endif
    printf("io_check: ok\n");
    return 0;
}
