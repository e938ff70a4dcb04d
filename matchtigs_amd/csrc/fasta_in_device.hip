// fasta_in_device.hip -- the plain unitig FASTA input route (`--fa-in X -k K`, bin.rs:71-75, 891-901): the edge-centric bigraph
// from the (k-1)-mer overlaps of the unitig ends, joined on the GPU.
//
// The contract (unpinned against the Rust reader, whose numbering cannot be seen here): occurrence o = 2u is the first
// k-1 bases of unitig u (P_u), o = 2u + 1 its last k-1 bases (S_u). Nodes are oriented (k-1)-mers, the mirror of x is rc(x); a class
// {x, rc(x)} takes ids in increasing order of its CREATOR, the occurrence with the smallest o in it: two consecutive ids (the
// creator's orientation first) or one for a palindrome. Edge 2u runs node(P_u) -> node(S_u), edge 2u + 1 mirror(node(S_u)) ->
// mirror(node(P_u)), both of weight len + 1 - k (bin.rs:369): the edge layout of every graph of the library (mtg_engine.h).
//
// The join, in six kernels on one stream:
//   pack     ASCII -> 2-bit packed store (pack_device.hpp, the spelling path's kernel)
//   extract  per occurrence: orientation of its canonical form (lexicographically smaller of x and rc(x)), palindrome flag and a
//            64-bit hash of the canonical bases. For k - 1 <= 32 the hash is a bijective mix of the canonical 2-bit code, so equal
//            hashes ARE equal bases; for longer (k-1)-mers it only places keys, and identity is decided base by base in the store.
//   insert   open addressing, 64-bit slots (hash tag << 32 | o), at least 2 slots per occurrence: an empty slot is claimed by CAS,
//            a slot of the same class takes atomicMin -- every slot only ever holds occurrences of one class, so the tag is fixed
//            and the minimum is the class's creator whatever order the threads arrive in
//   lookup   per occurrence: its class's slot -> creator; ids the creator owns (2, 1 for a palindrome, 0 for the others)
//   scan     exclusive scan of those counts in o order (hip_util.hpp) -> first id of each class, total = node count
//   edges    per unitig: mirror entries of the classes it creates, both edges and their weights
// Nothing depends on the order in which atomics land: the slots end holding the class minima, and everything after is a function of
// those. There is no host fallback; a missing GPU is an error.
//
// Device memory, per unitig of mean length l: peak = max(1.25 l + 26, l / 4 + 106) bytes -- the ASCII upload (freed once packed),
// then packed store + offsets + hash + flags + table (32-64 B: a power of two >= 4 U slots), then the scan and the output arrays
// (mirror sized for the 4 U ids that are the most there can be).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "device.hpp"
#include "hip_util.hpp"
#include "pack_device.hpp"

namespace mtg {

namespace {

constexpr unsigned long long EMPTY_SLOT = ~0ull;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64's finaliser: a bijection of 64-bit words
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct JoinArgs {
    const uint32_t *packed;
    const unsigned long long *off;  // [U + 1] base offsets of the records
    unsigned long long *hash;       // [2 U]
    uint8_t *flags;                 // [2 U] bit 0: the canonical form is rc(x); bit 1: x == rc(x)
    unsigned long long *table;      // [mask + 1]
    uint64_t mask;
    uint64_t n_occ;                 // 2 U
    uint32_t L;                     // k - 1
};

__device__ __forceinline__ uint64_t occ_start(const JoinArgs &a, uint64_t o) {
    const uint64_t u = o >> 1;
    return (o & 1) ? a.off[u + 1] - a.L : a.off[u];
}
// base i of the canonical form of the (k-1)-mer at `pos`
__device__ __forceinline__ uint32_t canon_base(const JoinArgs &a, uint64_t pos, bool flip, uint32_t i) {
    return flip ? 3u - packed_base(a.packed, pos + a.L - 1 - i) : packed_base(a.packed, pos + i);
}

__global__ __launch_bounds__(hu::EB) void extract_kernel(JoinArgs a) {
    const uint64_t o = hu::gid();
    if (o >= a.n_occ) return;
    const uint64_t pos = occ_start(a, o);
    bool flip, pal;
    uint64_t h;
    if (a.L <= 32) {
        uint64_t fwd = 0, rc = 0;  // first base in the highest bits: numeric order is lexicographic order
        for (uint32_t i = 0; i < a.L; i++) {
            const uint64_t c = packed_base(a.packed, pos + i);
            fwd = (fwd << 2) | c;
            rc |= (3ull - c) << (2 * i);
        }
        flip = rc < fwd;
        pal = rc == fwd;
        h = mix64(flip ? rc : fwd);
    } else {
        int cmp = 0;
        for (uint32_t i = 0; i < a.L && !cmp; i++) {
            const uint32_t x = packed_base(a.packed, pos + i), y = 3u - packed_base(a.packed, pos + a.L - 1 - i);
            cmp = x < y ? -1 : (x > y ? 1 : 0);
        }
        flip = cmp > 0;
        pal = cmp == 0;
        h = a.L;
        uint64_t w = 0;
        for (uint32_t i = 0; i < a.L; i++) {
            w = (w << 2) | canon_base(a, pos, flip, i);
            if ((i & 31) == 31 || i == a.L - 1) {
                h = mix64(h ^ w) + 0x9e3779b97f4a7c15ull;
                w = 0;
            }
        }
    }
    a.hash[o] = h;
    a.flags[o] = (uint8_t)((flip ? 1 : 0) | (pal ? 2 : 0));
}

// occurrences o and p hold the same class (k - 1 <= 32: the hash is exact)
__device__ __forceinline__ bool same_class(const JoinArgs &a, uint64_t o, uint64_t p) {
    if (a.hash[o] != a.hash[p]) return false;
    if (a.L <= 32) return true;
    const uint64_t po = occ_start(a, o), pp = occ_start(a, p);
    const bool fo = a.flags[o] & 1, fp = a.flags[p] & 1;
    for (uint32_t i = 0; i < a.L; i++)
        if (canon_base(a, po, fo, i) != canon_base(a, pp, fp, i)) return false;
    return true;
}

__global__ __launch_bounds__(hu::EB) void insert_kernel(JoinArgs a, unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o >= a.n_occ) return;
    const uint64_t h = a.hash[o];
    const unsigned long long mine = (h & 0xFFFFFFFF00000000ull) | o;
    uint64_t s = h & a.mask;
    for (uint64_t probe = 0; probe <= a.mask; probe++, s = (s + 1) & a.mask) {
        unsigned long long cur = __hip_atomic_load(&a.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY_SLOT) {
            const unsigned long long prev = atomicCAS(&a.table[s], EMPTY_SLOT, mine);
            if (prev == EMPTY_SLOT) return;
            cur = prev;
        }
        if ((cur >> 32) == (mine >> 32) && same_class(a, o, cur & 0xFFFFFFFFull)) {
            atomicMin(&a.table[s], mine);
            return;
        }
    }
    atomicOr(err, 1u);  // (a table of >= 2 slots per occurrence is never full)
}

__global__ __launch_bounds__(hu::EB) void lookup_kernel(JoinArgs a, uint32_t *creator, uint32_t *count, unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o >= a.n_occ) return;
    const uint64_t h = a.hash[o];
    uint64_t s = h & a.mask;
    for (uint64_t probe = 0; probe <= a.mask; probe++, s = (s + 1) & a.mask) {
        const unsigned long long cur = a.table[s];
        if (cur == EMPTY_SLOT) break;
        if ((cur >> 32) == (h >> 32) && same_class(a, o, cur & 0xFFFFFFFFull)) {
            const uint32_t c = (uint32_t)cur;
            creator[o] = c;
            count[o] = c == o ? ((a.flags[o] & 2) ? 1u : 2u) : 0u;
            return;
        }
    }
    creator[o] = (uint32_t)o;  // (unreachable: every occurrence was inserted)
    count[o] = 0;
    atomicOr(err, 2u);
}

__global__ __launch_bounds__(hu::EB) void edges_kernel(JoinArgs a, const uint32_t *creator, const uint64_t *first_id, uint32_t *mirror,
                                                        uint32_t *from, uint32_t *to, uint64_t *weight) {
    const uint64_t u = hu::gid();
    if (2 * u >= a.n_occ) return;
    uint32_t node[2], mir[2];
    for (int s = 0; s < 2; s++) {
        const uint64_t o = 2 * u + s;
        const uint32_t c = creator[o];
        const uint64_t b = first_id[c];
        const uint8_t f = a.flags[o];
        if (f & 2) {
            node[s] = mir[s] = (uint32_t)b;
        } else {
            const uint32_t same = ((f ^ a.flags[c]) & 1) == 0;
            node[s] = (uint32_t)(b + 1 - same);
            mir[s] = (uint32_t)(b + same);
        }
        if (c == o) {
            if (f & 2) mirror[b] = (uint32_t)b;
            else {
                mirror[b] = (uint32_t)(b + 1);
                mirror[b + 1] = (uint32_t)b;
            }
        }
    }
    from[2 * u] = node[0];
    to[2 * u] = node[1];
    from[2 * u + 1] = mir[1];
    to[2 * u + 1] = mir[0];
    const uint64_t w = a.off[u + 1] - a.off[u] - a.L;  // len + 1 - k
    weight[2 * u] = w;
    weight[2 * u + 1] = w;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

HostGraph *device_graph_from_sequences(const char *data, const uint64_t *off, uint64_t U, uint64_t k, int device_id, FastaJoinTimes *times) {
    if (!off || (U && !data)) MTG_DIE("mtg_graph_from_sequences: null argument");
    if (k < 2) MTG_DIE("mtg_graph_from_sequences: k must be >= 2");
    if (off[0] != 0) MTG_DIE("mtg_graph_from_sequences: offsets must start at 0");
    if (U >= (NONE - 1) / 2) MTG_DIE("mtg_graph_from_sequences: %llu unitigs; edge ids are 32-bit", (unsigned long long)U);
    for (uint64_t u = 0; u < U; u++) {
        if (off[u + 1] < off[u]) MTG_DIE("mtg_graph_from_sequences: offsets decrease at record %llu", (unsigned long long)u);
        if (off[u + 1] - off[u] < k)
            MTG_DIE("record %llu has length %llu < k = %llu", (unsigned long long)u, (unsigned long long)(off[u + 1] - off[u]), (unsigned long long)k);
    }
    if (k - 1 > 0xFFFFFFFFull) MTG_DIE("mtg_graph_from_sequences: k too large");
    FastaJoinTimes t{};
    if (U == 0) {
        const auto t0 = std::chrono::steady_clock::now();
        HostGraph *g = graph_from_edges(0, nullptr, 0, nullptr, nullptr, nullptr);
        t.build_ms = ms_since(t0);
        if (times) *times = t;
        return g;
    }
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the plain-FASTA join (there is no CPU path)", device_id);
    HIP_CHECK(hipSetDevice(device_id));
    hipStream_t st = nullptr;
    const uint64_t n_bases = off[U], n_words = (n_bases + 15) / 16, n_occ = 2 * U, max_ids = 2 * n_occ;
    uint64_t slots = 64;
    while (slots < 2 * n_occ) slots *= 2;

    auto t0 = std::chrono::steady_clock::now();
    char *d_ascii = nullptr;
    uint32_t *d_packed = nullptr;
    unsigned long long *d_off = nullptr, *d_hash = nullptr, *d_table = nullptr, *d_bad = nullptr;
    uint8_t *d_flags = nullptr;
    unsigned int *d_err = nullptr;
    hu::device_malloc(&d_ascii, n_bases);
    hu::device_malloc(&d_packed, n_words * 4);
    hu::device_malloc(&d_off, (U + 1) * 8);
    hu::device_malloc(&d_bad, 16);
    d_err = reinterpret_cast<unsigned int *>(d_bad + 1);
    HIP_CHECK(hipMemcpyAsync(d_ascii, data, n_bases, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_off, off, (U + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, st));
    HIP_CHECK(hipMemsetAsync(d_err, 0, 4, st));
    HIP_CHECK(hipStreamSynchronize(st));
    t.upload_ms = ms_since(t0);

    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, st));
    pack_kernel<<<hu::grid_for(n_words), hu::EB, 0, st>>>(d_ascii, n_bases, d_packed, d_bad);
    hu::device_malloc(&d_hash, n_occ * 8);
    hu::device_malloc(&d_flags, n_occ);
    JoinArgs a{};
    a.packed = d_packed; a.off = d_off; a.hash = d_hash; a.flags = d_flags; a.n_occ = n_occ; a.L = (uint32_t)(k - 1);
    extract_kernel<<<hu::grid_for(n_occ), hu::EB, 0, st>>>(a);
    HIP_CHECK(hipGetLastError());
    hu::device_free(d_ascii);  // (synchronises: the pack is done)
    hu::device_malloc(&d_table, slots * 8);
    HIP_CHECK(hipMemsetAsync(d_table, 0xFF, slots * 8, st));
    a.table = d_table;
    a.mask = slots - 1;
    uint32_t *d_creator = nullptr, *d_count = nullptr;
    hu::device_malloc(&d_creator, n_occ * 4);
    hu::device_malloc(&d_count, n_occ * 4);
    insert_kernel<<<hu::grid_for(n_occ), hu::EB, 0, st>>>(a, d_err);
    lookup_kernel<<<hu::grid_for(n_occ), hu::EB, 0, st>>>(a, d_creator, d_count, d_err);
    HIP_CHECK(hipGetLastError());
    hu::device_free(d_table);
    hu::device_free(d_hash);
    a.table = nullptr;
    a.hash = nullptr;  // (not read after the lookup)
    uint64_t *d_first = nullptr, *d_bsum = nullptr;
    hu::device_malloc(&d_first, n_occ * 8);
    hu::device_malloc(&d_bsum, (hu::scan_blocks(n_occ) + 2) * 8);
    hu::scan_u32<uint64_t>(st, d_count, n_occ, d_first, d_bsum, d_bsum + hu::scan_blocks(n_occ) + 1);
    uint32_t *d_mirror = nullptr, *d_from = nullptr, *d_to = nullptr;
    uint64_t *d_weight = nullptr;
    hu::device_malloc(&d_mirror, max_ids * 4);
    hu::device_malloc(&d_from, n_occ * 4);
    hu::device_malloc(&d_to, n_occ * 4);
    hu::device_malloc(&d_weight, n_occ * 8);
    edges_kernel<<<hu::grid_for(U), hu::EB, 0, st>>>(a, d_creator, d_first, d_mirror, d_from, d_to, d_weight);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(e1, st));
    unsigned long long h_bad[2] = {0, 0}, n_nodes = 0;
    HIP_CHECK(hipMemcpyAsync(h_bad, d_bad, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&n_nodes, d_bsum + hu::scan_blocks(n_occ) + 1, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    float f = 0.f;
    HIP_CHECK(hipEventElapsedTime(&f, e0, e1));
    t.kernel_ms = f;
    HIP_CHECK(hipEventDestroy(e0));
    HIP_CHECK(hipEventDestroy(e1));
    if (h_bad[0] != EMPTY_SLOT) MTG_DIE("sequences: character at offset %llu is not in the DNA alphabet (ACGT)", h_bad[0]);
    if ((h_bad[1] & 0xFFFFFFFFull) != 0) MTG_DIE("plain-FASTA join: internal error %llu (hash table)", h_bad[1] & 0xFFFFFFFFull);
    if (n_nodes > max_ids || n_nodes >= NONE) MTG_DIE("%llu nodes; node ids are 32-bit", n_nodes);

    t0 = std::chrono::steady_clock::now();
    PodVec<uint32_t> mirror(std::max<uint64_t>(n_nodes, 1)), from(n_occ), to(n_occ);
    PodVec<uint64_t> weight(n_occ);
    HIP_CHECK(hipMemcpyAsync(mirror.data(), d_mirror, n_nodes * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(from.data(), d_from, n_occ * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(to.data(), d_to, n_occ * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(weight.data(), d_weight, n_occ * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    t.download_ms = ms_since(t0);
    for (void *p : {(void *)d_packed, (void *)d_off, (void *)d_bad, (void *)d_flags, (void *)d_creator, (void *)d_count, (void *)d_first,
                    (void *)d_bsum, (void *)d_mirror, (void *)d_from, (void *)d_to, (void *)d_weight})
        hu::device_free(p);

    t0 = std::chrono::steady_clock::now();
    HostGraph *g = graph_from_edges(n_nodes, mirror.data(), n_occ, from.data(), to.data(), weight.data());
    t.build_ms = ms_since(t0);
    // What the join kernels must move at the least: ASCII read + packed store written once, per occurrence the packed words of its
    // (k-1)-mer (read by extract, and twice more by insert / lookup beyond k - 1 = 32), hash + flags written, the table's
    // slot touched by insert and lookup plus the occupant's hash, creator + count written and read back, the scan's u32 in and u64
    // out, per unitig its offsets twice, the six output words and the mirror entries.
    const uint64_t words_per_occ = (k - 1 + 15) / 16 + 1;
    t.bytes = n_bases + n_words * 4 + n_occ * (words_per_occ * 4 * (k - 1 > 32 ? 3 : 1) + 8 + 9 + 2 * (8 + 8 + 8) + 8 + 4 + 8 + 8 + 1) +
              U * (2 * 16 + 2 * 4 + 2 * 8) + n_nodes * 4;
    if (times) *times = t;
    return g;
}

}  // namespace mtg
