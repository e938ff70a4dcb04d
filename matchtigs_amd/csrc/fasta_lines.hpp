// fasta_lines.hpp -- the line reader of the two FASTA input routes (bcalm2.cpp, fasta_in.cpp): one line of a zlib stream (gzopen
// also reads plain files), any length, without its "\n" / "\r\n". Returns false at the end of the stream.
#pragma once

#include <zlib.h>

#include <cstring>
#include <string>

namespace mtg {

inline bool read_line(gzFile f, std::string &line) {
    line.clear();
    char buf[1 << 16];
    for (;;) {
        if (!gzgets(f, buf, sizeof buf)) return !line.empty();
        const size_t n = std::strlen(buf);
        line.append(buf, n);
        if (n && buf[n - 1] == '\n') break;
    }
    while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
    return true;
}

}  // namespace mtg
