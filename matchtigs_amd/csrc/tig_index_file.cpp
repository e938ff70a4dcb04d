// tig_index_file.cpp -- the header of an index file and its host checks (tig_index_file.hpp). A host translation unit:
// nothing here touches HIP, so mtg_tig_index_file_info works on a machine without a GPU and a damaged header is refused before any
// device allocation.
#include "tig_index_file.hpp"

#include <cerrno>
#include <cinttypes>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "host_graph.hpp"

namespace mtg {
namespace tf {

uint64_t digest_bytes(const void *p, uint64_t n_bytes) {
    const unsigned char *b = static_cast<const unsigned char *>(p);
    const uint64_t n = (n_bytes + 7) / 8;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t w = 0;
        const uint64_t len = n_bytes - 8 * i < 8 ? n_bytes - 8 * i : 8;
        std::memcpy(&w, b + 8 * i, len);
        sum += mix(w ^ ((i + 1) * DIGEST_STEP));
    }
    return n ^ sum;
}

namespace {
enum { K, M, RECORDS, CHARACTERS, OCCURRENCES, ANCHORS, BUCKETS, BUCKET_LIMIT, HEAVY_BUCKETS, HEAVY_WINDOWS, TABLE_SLOTS };

void payload_sections(const mtg_tig_payload &p, uint64_t value_size, SectionEntry *dense, SectionEntry *start, SectionEntry *value) {
    dense->elem_size = p.layout == 1 ? p.width : 1;
    dense->count = p.layout == 1 ? p.windows : 0;
    start->elem_size = 8;
    value->elem_size = value_size;
    start->count = value->count = p.layout == 2 ? p.runs : 0;
}

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// the checks of one payload's fields against each other and the index's; value_size: 4 (weights) or 8 (masks)
bool payload_check(const char *name, const mtg_tig_payload &p, uint64_t occurrences, uint64_t value_size, uint64_t n_colors, std::string &why) {
    if (p.layout == 0) {
        if (p.width || p.windows || p.runs || p.device_bytes) { why = fmt("count: %s is absent but its fields are not zero", name); return false; }
        return true;
    }
    if (p.layout > 2) { why = fmt("count: %s has the layout %" PRIu64 "; 1 (dense) and 2 (runs) exist", name, p.layout); return false; }
    bool legal = p.width == 1 || p.width == 2 || p.width == 4;
    if (value_size == 8) legal = p.width == (n_colors <= 8 ? 1u : n_colors <= 16 ? 2u : n_colors <= 32 ? 4u : 8u);
    if (!legal) { why = fmt("limits: %s has the dense width %" PRIu64, name, p.width); return false; }
    if (p.windows != occurrences) { why = fmt("count: %s has %" PRIu64 " windows, the index %" PRIu64, name, p.windows, occurrences); return false; }
    if (p.runs > p.windows || (p.windows && !p.runs)) { why = fmt("count: %s has %" PRIu64 " runs over %" PRIu64 " windows", name, p.runs, p.windows); return false; }
    const uint64_t bytes = p.layout == 1 ? p.width * p.windows : (8 + value_size) * p.runs;
    if (p.device_bytes != bytes) { why = fmt("count: %s says %" PRIu64 " bytes, its layout takes %" PRIu64, name, p.device_bytes, bytes); return false; }
    return true;
}
}  // namespace

void implied_sections(const Header &h, SectionEntry out[N_SECTIONS]) {
    for (int s = 0; s < N_SECTIONS; s++) out[s] = SectionEntry{(uint64_t)s + 1, 8, 0, 0, 0};
    const bool payloads = h.weights.layout || h.colors.layout;
    out[PACKED].elem_size = 4;
    out[PACKED].count = (h.info[CHARACTERS] + 15) / 16 + 2;
    out[OFF].count = h.info[RECORDS] + 1;
    out[DIR].count = h.info[BUCKETS] + 1;
    out[ENTRIES].count = h.info[ANCHORS];
    out[TABLE].count = h.info[TABLE_SLOTS];
    out[HEAVY_WHERE].count = h.locating ? h.info[TABLE_SLOTS] : 0;
    out[WIN_OFF].count = payloads ? h.info[RECORDS] + 1 : 0;
    payload_sections(h.weights, 4, &out[W_DENSE], &out[W_START], &out[W_VALUE]);
    payload_sections(h.colors, 8, &out[C_DENSE], &out[C_START], &out[C_VALUE]);
}

void header_fill(Header &h, const mtg_tig_index_info &info, uint64_t shift, bool locating, const mtg_tig_payload_info &pl, uint64_t meta_len) {
    SectionEntry digests[N_SECTIONS];
    std::memcpy(digests, h.sec, sizeof digests);
    const uint64_t meta_digest = h.meta_digest;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, "MTGTIGIX", 8);
    h.version = VERSION;
    h.byte_order = BYTE_ORDER_MARK;
    h.header_len = HEADER_BYTES;
    h.meta_len = meta_len;
    h.meta_digest = meta_digest;
    std::memcpy(h.info, &info, sizeof h.info);
    h.shift = shift;
    h.locating = locating ? 1 : 0;
    h.n_colors = pl.n_colors;
    h.weights = pl.weights;
    h.colors = pl.colors;
    h.win_offset_bytes = pl.win_offset_bytes;
    h.n_sections = N_SECTIONS;
    implied_sections(h, h.sec);
    uint64_t at = align_up(HEADER_BYTES + 8 + meta_len);
    for (int s = 0; s < N_SECTIONS; s++) {
        h.sec[s].offset = at;
        h.sec[s].digest = digests[s].digest;
        at = align_up(at + h.sec[s].elem_size * h.sec[s].count);
    }
    h.file_len = at;
}

void header_seal(Header &h) { h.header_digest = digest_bytes(&h, offsetof(Header, header_digest)); }

void header_info(const Header &h, mtg_tig_index_info *info, mtg_tig_payload_info *pl) {
    if (info) {
        std::memcpy(info, h.info, sizeof h.info);
        // (device_tig_index_build's count: entries takes one element at the least)
        info->device_bytes = ((h.info[CHARACTERS] + 15) / 16 + 2) * 4 + (h.info[RECORDS] + 1) * 8 + (h.info[BUCKETS] + 1) * 8 +
                             (h.info[ANCHORS] ? h.info[ANCHORS] : 1) * 8 + h.info[TABLE_SLOTS] * 8 + (h.locating ? h.info[TABLE_SLOTS] * 8 : 0) +
                             h.win_offset_bytes + h.weights.device_bytes + h.colors.device_bytes;
    }
    if (pl) {
        *pl = mtg_tig_payload_info{};
        pl->weights = h.weights;
        pl->colors = h.colors;
        pl->n_colors = h.n_colors;
        pl->win_offset_bytes = h.win_offset_bytes;
    }
}

bool header_check(const Header &h, uint64_t have, uint64_t file_len, std::string &why) {
    if (have < HEADER_BYTES) { why = fmt("header: the file has %" PRIu64 " bytes, shorter than the header's %" PRIu64, file_len, HEADER_BYTES); return false; }
    if (std::memcmp(h.magic, "MTGTIGIX", 8) != 0) { why = "magic: not an index file (the first 8 bytes are not MTGTIGIX)"; return false; }
    if (h.byte_order == __builtin_bswap32(BYTE_ORDER_MARK)) { why = "byte order: the file was written by a host of the other byte order"; return false; }
    if (h.version != VERSION) {
        if (h.version > VERSION) why = fmt("version: the file has format version %u, this build reads version %u and no later one", h.version, VERSION);
        else why = fmt("version: format version %u does not exist", h.version);
        return false;
    }
    if (h.byte_order != BYTE_ORDER_MARK) { why = fmt("byte order: the mark is 0x%08x, not 0x%08x", h.byte_order, BYTE_ORDER_MARK); return false; }
    if (h.header_len != HEADER_BYTES) { why = fmt("header: its length field says %" PRIu64 ", version 1 has %" PRIu64, h.header_len, HEADER_BYTES); return false; }
    if (h.header_digest != digest_bytes(&h, offsetof(Header, header_digest))) { why = "header digest: the header's bytes do not give the digest it ends with"; return false; }
    // extents: everything inside the file's actual length
    if (h.file_len != file_len) { why = fmt("extent: the header says the file has %" PRIu64 " bytes, it has %" PRIu64, h.file_len, file_len); return false; }
    if (h.meta_len > file_len || HEADER_BYTES + 8 + h.meta_len > file_len) { why = fmt("extent: the metadata (%" PRIu64 " bytes) reaches past the end of the file", h.meta_len); return false; }
    if (h.n_sections != N_SECTIONS) { why = fmt("count: %" PRIu64 " sections, version 1 has %d", h.n_sections, (int)N_SECTIONS); return false; }
    for (int s = 0; s < N_SECTIONS; s++) {
        const SectionEntry &e = h.sec[s];
        if (e.id != (uint64_t)s + 1) { why = fmt("count: section %d has the id %" PRIu64, s + 1, e.id); return false; }
        if (e.elem_size != 1 && e.elem_size != 2 && e.elem_size != 4 && e.elem_size != 8) { why = fmt("section %s: count: elements of %" PRIu64 " bytes", section_name(s), e.elem_size); return false; }
        if (e.offset % ALIGN || e.offset < HEADER_BYTES + 8 + h.meta_len) { why = fmt("section %s: extent: the offset %" PRIu64 " is not a multiple of %" PRIu64 " behind the metadata", section_name(s), e.offset, ALIGN); return false; }
        if (e.offset > file_len || e.count > (file_len - e.offset) / e.elem_size) {
            why = fmt("section %s: extent: %" PRIu64 " elements of %" PRIu64 " bytes at offset %" PRIu64 " reach past the end of the file (%" PRIu64 " bytes)", section_name(s),
                      e.count, e.elem_size, e.offset, file_len);
            return false;
        }
        if (s && e.offset < h.sec[s - 1].offset + h.sec[s - 1].elem_size * h.sec[s - 1].count) { why = fmt("section %s: extent: it overlaps the section before", section_name(s)); return false; }
    }
    // counts: what the info fields imply. The fields that become sizes are bounded first, so that no sum below wraps.
    const uint64_t *in = h.info;
    if (in[CHARACTERS] >= POS_LIMIT) { why = fmt("limits: %" PRIu64 " bases; the limit is 2^40 - 2", in[CHARACTERS]); return false; }
    if (in[RECORDS] > file_len || in[BUCKETS] > file_len || in[ANCHORS] > in[CHARACTERS] || in[OCCURRENCES] > in[CHARACTERS] || in[HEAVY_WINDOWS] > in[OCCURRENCES] ||
        in[HEAVY_BUCKETS] > in[BUCKETS]) {
        why = "count: the info fields contradict each other (records, buckets, anchors, occurrences or the heavy counts exceed what holds them)";
        return false;
    }
    if (h.locating > 1) { why = fmt("count: locating is %" PRIu64, h.locating); return false; }
    if (!payload_check("weights", h.weights, in[OCCURRENCES], 4, h.n_colors, why)) return false;
    if (h.n_colors > 64) { why = fmt("limits: n_colors is %" PRIu64 "; 1 .. 64 are served", h.n_colors); return false; }
    if ((h.colors.layout != 0) != (h.n_colors != 0)) { why = fmt("count: n_colors is %" PRIu64 " and the colours' layout %" PRIu64, h.n_colors, h.colors.layout); return false; }
    if (!payload_check("colors", h.colors, in[OCCURRENCES], 8, h.n_colors, why)) return false;
    const bool payloads = h.weights.layout || h.colors.layout;
    if (payloads && !h.locating) { why = "count: an index with payloads is a locating one"; return false; }
    if (h.win_offset_bytes != (payloads ? (in[RECORDS] + 1) * 8 : 0)) { why = fmt("count: win_offset_bytes is %" PRIu64, h.win_offset_bytes); return false; }
    SectionEntry want[N_SECTIONS];
    implied_sections(h, want);
    for (int s = 0; s < N_SECTIONS; s++)
        if (h.sec[s].count != want[s].count || h.sec[s].elem_size != want[s].elem_size) {
            why = fmt("section %s: count: %" PRIu64 " elements of %" PRIu64 " bytes, the info fields imply %" PRIu64 " of %" PRIu64, section_name(s), h.sec[s].count,
                      h.sec[s].elem_size, want[s].count, want[s].elem_size);
            return false;
        }
    // limits: the build's own
    if (in[K] < 1 || in[K] > 0xFFFFFFFFull) { why = fmt("limits: k is %" PRIu64, in[K]); return false; }
    if (in[M] < 1 || in[M] > in[K] || in[M] > 31) { why = fmt("limits: the minimizer length %" PRIu64 " is outside 1 .. min(k, 31), k = %" PRIu64, in[M], in[K]); return false; }
    if (in[BUCKET_LIMIT] < 1 || in[BUCKET_LIMIT] > 65536) { why = fmt("limits: bucket_limit is %" PRIu64 "; 1 .. 65536 are served", in[BUCKET_LIMIT]); return false; }
    if (in[BUCKETS] < 8 || (in[BUCKETS] & (in[BUCKETS] - 1)) || h.shift != (uint64_t)__builtin_clzll(in[BUCKETS]) + 1) {
        why = fmt("limits: %" PRIu64 " buckets with the shift %" PRIu64 " (a power of two from 8 on, shift = 64 - log2)", in[BUCKETS], h.shift);
        return false;
    }
    const uint64_t slots = in[HEAVY_BUCKETS] ? ((2 * in[HEAVY_WINDOWS] + 7) / 8 * 8 > 8 ? (2 * in[HEAVY_WINDOWS] + 7) / 8 * 8 : 8) : 0;
    if (in[TABLE_SLOTS] != slots || (!in[HEAVY_BUCKETS] && in[HEAVY_WINDOWS])) {
        why = fmt("limits: %" PRIu64 " table slots for %" PRIu64 " heavy windows in %" PRIu64 " heavy buckets", in[TABLE_SLOTS], in[HEAVY_WINDOWS], in[HEAVY_BUCKETS]);
        return false;
    }
    return true;
}

bool header_read(const char *path, Header &h, std::string &meta, std::string &err) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { err = std::string(path) + ": cannot open: " + std::strerror(errno); return false; }
    std::string why;
    bool ok = false;
    do {
        if (std::fseek(f, 0, SEEK_END) != 0) { why = "cannot seek"; break; }
        const long end = std::ftell(f);
        if (end < 0) { why = "cannot tell the file's length"; break; }
        std::rewind(f);
        std::memset(&h, 0, sizeof h);
        const uint64_t have = std::fread(&h, 1, sizeof h, f);
        if (!header_check(h, have, (uint64_t)end, why)) break;
        uint64_t len = 0;
        if (std::fread(&len, 1, 8, f) != 8 || len != h.meta_len) { why = "metadata: its length prefix is not the header's meta_len"; break; }
        meta.assign(h.meta_len, '\0');
        if (h.meta_len && std::fread(&meta[0], 1, h.meta_len, f) != h.meta_len) { why = "metadata: cannot read it"; break; }
        if (digest_bytes(meta.data(), meta.size()) != h.meta_digest) { why = "metadata: digest: its bytes do not give the digest in the header"; break; }
        ok = true;
    } while (false);
    std::fclose(f);
    if (!ok) err = std::string(path) + ": " + why;
    return ok;
}

}  // namespace tf
}  // namespace mtg

using namespace mtg;

static void put_error(const std::string &msg, char *err, uint64_t err_len) {
    if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
}

extern "C" int mtg_tig_index_file_info(const char *path, mtg_tig_index_info *info, mtg_tig_payload_info *payload, int *locating, char *meta,
                                       uint64_t meta_cap, uint64_t *meta_len, char *err, uint64_t err_len) {
    if (!path) MTG_DIE("mtg_tig_index_file_info: null argument");
    tf::Header h;
    std::string blob, why;
    if (!tf::header_read(path, h, blob, why)) {
        put_error(why, err, err_len);
        return 2;
    }
    tf::header_info(h, info, payload);
    if (locating) *locating = (int)h.locating;
    if (meta_len) *meta_len = blob.size();
    if (meta && meta_cap) std::memcpy(meta, blob.data(), blob.size() < meta_cap ? blob.size() : meta_cap);
    return 0;
}
