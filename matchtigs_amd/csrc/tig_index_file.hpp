// tig_index_file.hpp -- the sparse minimizer index as a file (`.mtgx`, format version 1): what the host translation
// unit (tig_index_file.cpp: the header, its checks, mtg_tig_index_file_info) and the device one (tig_index_file_device.hpp: the
// sections, their digests, the validator) share. No HIP here.
//
// A file is  [Header, HEADER_BYTES] [u64 meta_len] [meta bytes] [zeros up to ALIGN] then, per section in the order of Section, the
// bytes of the device array as they are, each at a multiple of ALIGN, zeros between and up to the file's length, itself a multiple
// of ALIGN. Every integer is little-endian. A section the index does not have has count 0 and takes no bytes (its offset is where
// the next one starts).
//
// The digest of n_bytes bytes: w_0 .. w_(n-1) their little-endian 64-bit words, the tail zero-padded, n = ceil(n_bytes / 8);
//   n XOR sum_i mix(w_i XOR (i + 1) * 0x9E3779B97F4A7C15)  mod 2^64,  mix = splitmix64's finaliser (a bijection).
#pragma once
#include <cstdint>
#include <string>

#include "../../include/mtg_engine.h"

namespace mtg {
namespace tf {

constexpr uint32_t VERSION = 1;
constexpr uint32_t BYTE_ORDER_MARK = 0x01020304u;  // read as 0x04030201 by a host of the other byte order
constexpr uint64_t ALIGN = 4096;
constexpr uint64_t DIGEST_STEP = 0x9E3779B97F4A7C15ull;
constexpr uint64_t POS_LIMIT = (1ull << 40) - 1;  // kw::POS_LIMIT: global positions are below this

enum Section : int { PACKED, OFF, DIR, ENTRIES, TABLE, HEAVY_WHERE, WIN_OFF, W_DENSE, W_START, W_VALUE, C_DENSE, C_START, C_VALUE, N_SECTIONS };
inline const char *section_name(int s) {
    static const char *const names[N_SECTIONS] = {"packed", "off", "dir", "entries", "table", "heavy_where", "win_off", "weights.dense",
                                                  "weights.start", "weights.value", "colors.dense", "colors.start", "colors.value"};
    return s >= 0 && s < N_SECTIONS ? names[s] : "?";
}

struct SectionEntry {
    uint64_t id;         // Section + 1
    uint64_t elem_size;  // bytes per element
    uint64_t count;      // elements
    uint64_t offset;     // in the file, a multiple of ALIGN
    uint64_t digest;     // of its elem_size * count bytes
};

// the first HEADER_BYTES bytes of a file, field for field (every member is 8-byte aligned: no padding)
struct Header {
    char magic[8];  // "MTGTIGIX"
    uint32_t version, byte_order;
    uint64_t header_len;  // HEADER_BYTES
    uint64_t file_len;
    uint64_t meta_len, meta_digest;
    uint64_t info[11];  // mtg_tig_index_info without device_bytes: k, m, records, characters, occurrences, anchors, buckets,
                        // bucket_limit, heavy_buckets, heavy_windows, table_slots
    uint64_t shift, locating, n_colors;
    mtg_tig_payload weights, colors;  // layout, width, windows, runs, device_bytes
    uint64_t win_offset_bytes;
    uint64_t n_sections;  // N_SECTIONS
    SectionEntry sec[N_SECTIONS];
    uint64_t header_digest;  // of the bytes before it
};
constexpr uint64_t HEADER_BYTES = 784;
static_assert(sizeof(Header) == HEADER_BYTES, "the file header has no padding");
static_assert(sizeof(mtg_tig_index_info) == 12 * 8 && sizeof(mtg_tig_payload) == 5 * 8, "the info structs are plain 64-bit fields");

#ifdef __HIPCC__
#define MTG_TF_HD __host__ __device__
#else
#define MTG_TF_HD
#endif
MTG_TF_HD inline uint64_t mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
uint64_t digest_bytes(const void *p, uint64_t n_bytes);  // on the host: the header's and the metadata's

inline uint64_t align_up(uint64_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

// elem_size and count of every section as the header's other fields imply them (id set, offset and digest left 0)
void implied_sections(const Header &h, SectionEntry out[N_SECTIONS]);
// fills magic .. n_sections (but for the sections' digests and meta_digest, which the caller has set or sets) from the index's
// fields, lays the sections out behind a metadata blob of meta_len bytes and sets file_len
void header_fill(Header &h, const mtg_tig_index_info &info, uint64_t shift, bool locating, const mtg_tig_payload_info &pl, uint64_t meta_len);
void header_seal(Header &h);  // header_digest
void header_info(const Header &h, mtg_tig_index_info *info, mtg_tig_payload_info *pl);  // device_bytes recomputed as the builder counts them

// The host checks of a load, in order; false: `why` names the check (and the section where there is one). file_len: the file's
// actual length; have: the bytes of it in `h` (a file shorter than the header is refused first).
bool header_check(const Header &h, uint64_t have, uint64_t file_len, std::string &why);
// opens, reads and checks the header and the metadata; false: err = "<path>: <why>"
bool header_read(const char *path, Header &h, std::string &meta, std::string &err);

}  // namespace tf
}  // namespace mtg
