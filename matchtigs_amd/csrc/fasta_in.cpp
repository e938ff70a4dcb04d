// fasta_in.cpp -- the plain unitig FASTA input route (`--fa-in X -k K`, bin.rs:71-75, 891-901): the host half. Parses the records
// into the sequence store; the graph comes from the (k-1)-mer join on the GPU (fasta_in_device.hip, whose header states the
// contract).
//
// Format: `>` header lines with any text (BCALM2's `L:` annotations included: they are not read), then the sequence on one or
// more lines, either case. Empty lines are skipped, `.gz` inputs are inflated with zlib (gzopen also reads plain files). The same
// line reader and alphabet rule as the BCALM2 route (bcalm2.cpp). read_fasta_records is that reader on its own (mtg_read_sequences:
// a tig file someone else wrote, for the k-mer set comparison), read_fasta_records_split the same reader where a run of characters
// outside ACGT (the `N` of real assemblies) ends a piece instead of aborting (mtg_read_sequences_split, `--seq-in`), read_fasta_records_named the reader
// without an alphabet rule that also hands out the record names (mtg_read_sequences_named, `--query-fa`); read_fasta adds the length rule and the join.
#include <zlib.h>

#include <cctype>
#include <chrono>
#include <string>

#include "device.hpp"
#include "fasta_lines.hpp"
#include "host_graph.hpp"

namespace mtg {

UnitigStore *read_fasta_records(const char *path) {
    gzFile f = gzopen(path, "rb");
    if (!f) MTG_DIE("cannot open %s", path);
    gzbuffer(f, 1 << 20);
    UnitigStore *st = new UnitigStore();
    st->off.push_back(0);
    std::string line;
    bool have_record = false;
    while (read_line(f, line)) {
        if (line.empty()) continue;
        if (line[0] == '>') {
            if (have_record) st->off.push_back(st->data.size());
            have_record = true;
        } else {
            if (!have_record) MTG_DIE("%s: sequence data before the first header", path);
            for (char &c : line) {
                if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A');
                if (c != 'A' && c != 'C' && c != 'G' && c != 'T') MTG_DIE("%s: character '%c' is not in the DNA alphabet", path, c);
            }
            st->data += line;
        }
    }
    gzclose(f);
    if (have_record) st->off.push_back(st->data.size());
    return st;
}

UnitigStore *read_fasta_records_named(const char *path, UnitigStore **names_out) {
    gzFile f = gzopen(path, "rb");
    if (!f) MTG_DIE("cannot open %s", path);
    gzbuffer(f, 1 << 20);
    UnitigStore *st = new UnitigStore(), *names = new UnitigStore();
    st->off.push_back(0);
    names->off.push_back(0);
    std::string line;
    bool have_record = false;
    while (read_line(f, line)) {
        if (line.empty()) continue;
        if (line[0] == '>') {
            if (have_record) st->off.push_back(st->data.size());
            have_record = true;
            size_t end = 1;
            while (end < line.size() && !std::isspace((unsigned char)line[end])) end++;
            names->data.append(line, 1, end - 1);
            names->off.push_back(names->data.size());
        } else {
            if (!have_record) MTG_DIE("%s: sequence data before the first header", path);
            st->data += line;
        }
    }
    gzclose(f);
    if (have_record) st->off.push_back(st->data.size());
    *names_out = names;
    return st;
}

UnitigStore *read_fasta_records_split(const char *path, uint64_t *pieces_cut) {
    gzFile f = gzopen(path, "rb");
    if (!f) MTG_DIE("cannot open %s", path);
    gzbuffer(f, 1 << 20);
    UnitigStore *st = new UnitigStore();
    st->off.push_back(0);
    std::string line;
    bool have_record = false, in_run = false;
    uint64_t cuts = 0;
    auto end_piece = [&]() {
        if (st->data.size() > st->off.back()) st->off.push_back(st->data.size());
    };
    while (read_line(f, line)) {
        if (line.empty()) continue;
        if (line[0] == '>') {
            end_piece();
            have_record = true;
            in_run = false;
        } else {
            if (!have_record) MTG_DIE("%s: sequence data before the first header", path);
            for (char c : line) {
                if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A');
                if (c == 'A' || c == 'C' || c == 'G' || c == 'T') {
                    st->data.push_back(c);
                    in_run = false;
                } else if (!in_run) {  // the first character of a run: the piece ends here
                    end_piece();
                    in_run = true;
                    cuts++;
                }
            }
        }
    }
    gzclose(f);
    end_piece();
    if (pieces_cut) *pieces_cut = cuts;
    return st;
}

HostGraph *read_fasta(const char *path, uint64_t k, int device_id, UnitigStore **store_out, FastaJoinTimes *times) {
    if (!path || !store_out) MTG_DIE("mtg_read_fasta: null argument");
    if (k < 2) MTG_DIE("mtg_read_fasta: k must be >= 2");
    const auto t0 = std::chrono::steady_clock::now();
    UnitigStore *st = read_fasta_records(path);
    const uint64_t U = st->off.size() - 1;
    for (uint64_t u = 0; u < U; u++) {
        const uint64_t len = st->off[u + 1] - st->off[u];
        if (len < k) MTG_DIE("%s: record %llu has length %llu < k = %llu", path, (unsigned long long)u, (unsigned long long)len, (unsigned long long)k);
    }
    const double parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HostGraph *g = device_graph_from_sequences(st->data.data(), st->off.data(), U, k, device_id, times);
    if (times) times->parse_ms = parse_ms;
    *store_out = st;
    return g;
}

}  // namespace mtg
