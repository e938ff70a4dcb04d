// fastq_text.hpp -- the host half of the FASTQ reader (fastq_device.hip): the inflated text of a file in one buffer,
// the two trims at its end, the format detection, the record names and the message of a malformed file. Nothing here touches a
// GPU, so a stand-alone program can run all of it under a sanitizer (tests/tools/fastq_text_check.cpp).
#pragma once

#include <sys/stat.h>
#include <zlib.h>

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hugebuf.hpp"

namespace mtg {
namespace fq {

// why a file is refused, in the order in which the rules are applied to one record (the smaller code wins inside a record)
enum : uint32_t { TRUNCATED = 1, BAD_HEADER = 2, BAD_SEPARATOR = 3, BAD_LENGTH = 4, BAD_QUALITY = 5, LINE_TOO_LONG = 6 };
constexpr unsigned long long NO_ERROR = ~0ull;
inline unsigned long long pack_error(uint64_t record, uint32_t reason) { return (unsigned long long)record << 8 | reason; }

inline const char *reason_text(uint32_t reason) {
    switch (reason) {
        case TRUNCATED: return "the file ends inside the record (its line count is not a multiple of 4)";
        case BAD_HEADER: return "the header line does not begin with '@'";
        case BAD_SEPARATOR: return "the separator line does not begin with '+'";
        case BAD_LENGTH: return "the sequence and the quality line differ in length";
        case BAD_QUALITY: return "a quality character is outside '!' .. '~'";
        case LINE_TOO_LONG: return "a sequence line is longer than 2^32 - 1 characters";
        default: return "unknown reason";
    }
}
// the 1-based line the message names: the line of the record that breaks the rule; for a truncated record the last line of the file
inline uint64_t reason_line(uint64_t record, uint32_t reason, uint64_t n_lines) {
    switch (reason) {
        case TRUNCATED: return n_lines;
        case BAD_HEADER: return 4 * record + 1;
        case BAD_SEPARATOR: return 4 * record + 3;
        case LINE_TOO_LONG: return 4 * record + 2;
        default: return 4 * record + 4;
    }
}
inline void format_error(const char *path, unsigned long long packed, uint64_t n_lines, char *err, uint64_t cap) {
    if (!err || !cap) return;
    const uint64_t record = packed >> 8;
    const uint32_t reason = (uint32_t)(packed & 0xFF);
    std::snprintf(err, cap, "%s: record %llu (line %llu): %s", path, (unsigned long long)record,
                  (unsigned long long)reason_line(record, reason, n_lines), reason_text(reason));
}

// The inflated bytes of a file (gzopen also reads plain files) in one buffer with at least two spare bytes behind them.
struct Text {
    std::unique_ptr<HugeBuf<char>> buf;
    uint64_t n = 0;
    uint64_t n_one_more = 0;  // after normalise(): n and one empty line behind it (0 for an empty text)
    char *data() const { return buf ? buf->p : nullptr; }
};

inline Text read_inflated(const char *path) {
    gzFile f = gzopen(path, "rb");
    if (!f) MTG_DIE("cannot open %s", path);
    gzbuffer(f, 1 << 20);
    struct stat sb;
    const uint64_t file_bytes = stat(path, &sb) == 0 && sb.st_size > 0 ? (uint64_t)sb.st_size : 0;
    // a plain file needs its size; a compressed one starts at four times its size and doubles when that runs out
    uint64_t cap = (gzdirect(f) ? file_bytes : 4 * file_bytes) + (1u << 16);
    Text t;
    t.buf.reset(new HugeBuf<char>(cap));
    for (;;) {
        if (t.n + 2 >= cap) {
            std::unique_ptr<HugeBuf<char>> bigger(new HugeBuf<char>(2 * cap));
            std::memcpy(bigger->p, t.buf->p, t.n);
            t.buf = std::move(bigger);
            cap *= 2;
        }
        const uint64_t want = cap - 2 - t.n;
        const int got = gzread(f, t.buf->p + t.n, (unsigned)(want < (1u << 30) ? want : (1u << 30)));
        if (got < 0) MTG_DIE("cannot read %s: %s", path, gzerror(f, nullptr));
        if (got == 0) break;
        t.n += (uint64_t)got;
    }
    gzclose(f);
    return t;
}

// A text without a final "\n" gets one (a spare byte); empty lines at the end -- "\n" or "\r\n" -- are dropped. Afterwards the
// text is empty or ends with the "\n" of a line that is not empty. The end of the text may still be the quality line of a read of
// length 0, written with or without its "\n": one empty line is put behind the text (the other spare byte, or the place of a
// dropped line), n_one_more takes it in, and the reader keeps it when it completes a record.
inline void normalise(Text &t) {
    char *p = t.data();
    uint64_t n = t.n;
    if (n && p[n - 1] != '\n') p[n++] = '\n';
    while (n >= 2) {
        if (p[n - 2] == '\n') n -= 1;
        else if (p[n - 2] == '\r' && n >= 3 && p[n - 3] == '\n') n -= 2;
        else if (p[n - 2] == '\r' && n == 2) n = 0;
        else break;
    }
    if (n == 1) n = 0;
    t.n = n;
    t.n_one_more = 0;
    if (n) {
        p[n] = '\n';
        t.n_one_more = n + 1;
    }
}

// 0: nothing but line ends, 1: FASTA (`>`), 2: FASTQ (`@`), -1: anything else -- by the first byte that is not a line end
inline int format_of(const char *p, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        if (p[i] == '\n' || p[i] == '\r') continue;
        return p[i] == '>' ? 1 : p[i] == '@' ? 2 : -1;
    }
    return 0;
}
inline int format_of_file(const char *path) {
    gzFile f = gzopen(path, "rb");
    if (!f) MTG_DIE("cannot open %s", path);
    char buf[1 << 12];
    int fmt = 0;
    for (;;) {
        const int got = gzread(f, buf, sizeof buf);
        if (got < 0) MTG_DIE("cannot read %s: %s", path, gzerror(f, nullptr));
        if (got == 0) break;
        fmt = format_of(buf, (uint64_t)got);
        if (fmt != 0) break;
    }
    gzclose(f);
    return fmt;
}

// The names of the records whose header lines start at header_start[0 .. n_records): the text behind the `@` up to the first white
// space, as read_fasta_records_named takes it behind `>`; an empty line has an empty name. The text ends with "\n", so every name
// ends inside it.
inline void slice_names(const char *text, uint64_t n, const uint64_t *header_start, uint64_t n_records, std::string &data,
                        std::vector<uint64_t> &off) {
    data.clear();
    off.assign(1, 0);
    for (uint64_t r = 0; r < n_records; r++) {
        uint64_t b = header_start[r], e = b;
        while (e < n && !std::isspace((unsigned char)text[e])) e++;
        if (e > b + 1) data.append(text + b + 1, e - b - 1);
        off.push_back(data.size());
    }
}

}  // namespace fq
}  // namespace mtg
