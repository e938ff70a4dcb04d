// fastq_text_check.cpp -- the host half of the FASTQ reader (matchtigs_amd/csrc/fastq_text.hpp) on its own: the file buffer, the
// trims, the format detection, the name slicing and the error message, with the line starts found by a plain loop instead of the
// GPU. A stand-alone program, so that it can be built with -fsanitize=address,undefined and run as it is (tests/test_fastq_ref.py).
// Usage: fastq_text_check FILE...   prints per file: format, normalised bytes (and with one more empty line), lines, then one line per record name.
#include <cstdio>
#include <string>
#include <vector>

#include "../../matchtigs_amd/csrc/fastq_text.hpp"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        const int fmt = mtg::fq::format_of_file(argv[i]);
        mtg::fq::Text t = mtg::fq::read_inflated(argv[i]);
        const int fmt_buffer = mtg::fq::format_of(t.data(), t.n);
        mtg::fq::normalise(t);
        std::vector<uint64_t> line_start(1, 0);
        for (uint64_t p = 0; p < t.n; p++)
            if (t.data()[p] == '\n') line_start.push_back(p + 1);
        const uint64_t lines = line_start.size() - 1, records = lines / 4;
        std::vector<uint64_t> header(records);
        for (uint64_t r = 0; r < records; r++) header[r] = line_start[4 * r];
        std::string names;
        std::vector<uint64_t> off;
        mtg::fq::slice_names(t.data(), t.n, header.data(), records, names, off);
        std::printf("file %d %d %llu %llu %llu %llu\n", fmt, fmt_buffer, (unsigned long long)t.n, (unsigned long long)t.n_one_more,
                    (unsigned long long)lines, (unsigned long long)records);
        for (uint64_t r = 0; r < records; r++) std::printf("name %s\n", names.substr(off[r], off[r + 1] - off[r]).c_str());
        char small[24], large[512];  // a message is cut to the capacity it is given
        mtg::fq::format_error(argv[i], mtg::fq::pack_error(records, mtg::fq::TRUNCATED), lines, small, sizeof small);
        mtg::fq::format_error(argv[i], mtg::fq::pack_error(0, mtg::fq::BAD_QUALITY), lines, large, sizeof large);
        mtg::fq::format_error(argv[i], mtg::fq::pack_error(1, mtg::fq::BAD_HEADER), lines, nullptr, 0);
        std::printf("error %zu %s\n", std::strlen(small), large);
    }
    return 0;
}
