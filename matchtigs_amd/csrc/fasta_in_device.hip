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
//   pack     ASCII -> 2-bit packed store (SeqStore, pack_device.hpp)
//   extract  per occurrence: the key of its class (kw::class_key, kmer_window_device.hpp): orientation of the canonical form,
//            palindrome flag and the 64-bit hash, kept in hash[] / flags[]
//   insert   into the table of classes (kw::find_slot, where the exactness and order-independence argument is written down).
//            Slot = low 32 bits of the hash << 32 | o, 2 slots per occurrence; "same class" is a tag match, then equal hashes
//            (which settles it for k - 1 <= 32) and kw::same_class in the store beyond. A slot of the same class takes atomicMin: the
//            tag is fixed per class, so the minimum is the class's creator. Occurrence order is position order (a record is at
//            least k long: prefix < suffix < the next record's prefix), so the creator is also the class's first position.
//   lookup   per occurrence: its class's slot -> creator; ids the creator owns (2, 1 for a palindrome, 0 for the others)
//   scan     exclusive scan of those counts in o order (hip_util.hpp) -> first id of each class, total = node count
//   edges    per unitig: mirror entries of the classes it creates, both edges and their weights
// There is no host fallback; a missing GPU is an error.
//
// Device memory, per unitig of mean length l: peak = max(1.25 l + 8, l / 4 + 90) bytes -- the ASCII upload (freed once packed),
// then packed store + offsets + hash + flags + table (32 B: 4 U slots) + creator + count, then the scan and the output arrays
// (mirror sized for the 4 U ids that are the most there can be).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"

namespace mtg {

namespace {

struct JoinArgs {
    const uint32_t *packed;
    const unsigned long long *off;  // [U + 1] base offsets of the records
    unsigned long long *hash;       // [2 U]
    uint8_t *flags;                 // [2 U] bit 0: the canonical form is rc(x); bit 1: x == rc(x)
    unsigned long long *table;      // [slots]
    uint64_t slots;
    uint64_t n_occ;                 // 2 U
    uint32_t L;                     // k - 1
};

__device__ __forceinline__ uint64_t occ_start(const JoinArgs &a, uint64_t o) {
    const uint64_t u = o >> 1;
    return (o & 1) ? a.off[u + 1] - a.L : a.off[u];
}

__global__ __launch_bounds__(hu::EB) void extract_kernel(JoinArgs a) {
    const uint64_t o = hu::gid();
    if (o >= a.n_occ) return;
    const kw::ClassKey key = kw::class_key(a.packed, occ_start(a, o), a.L);
    a.hash[o] = key.hash;
    a.flags[o] = (uint8_t)((key.flip ? 1 : 0) | (key.pal ? 2 : 0));
}

// the slot of the class of occurrence o, whose word would be `mine`
template <bool CLAIM>
__device__ __forceinline__ kw::Found find_class(const JoinArgs &a, uint64_t o, uint64_t h, unsigned long long mine) {
    return kw::find_slot<CLAIM>(a.table, a.slots, h, mine, [&](unsigned long long cur) {
        const uint64_t p = cur & 0xFFFFFFFFull;
        return (cur >> 32) == (mine >> 32) && a.hash[p] == h && (a.L <= 32 || kw::same_class(a.packed, occ_start(a, o), occ_start(a, p), a.L));
    });
}

__global__ __launch_bounds__(hu::EB) void insert_kernel(JoinArgs a, unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o >= a.n_occ) return;
    const uint64_t h = a.hash[o];
    const unsigned long long mine = (h << 32) | o;
    const kw::Found f = find_class<true>(a, o, h, mine);
    if (f.slot == a.slots) atomicOr(err, 1u);  // (a table of 2 slots per occurrence is never full)
    else if (f.word != kw::EMPTY_SLOT && mine < f.word) atomicMin(&a.table[f.slot], mine);
}

__global__ __launch_bounds__(hu::EB) void lookup_kernel(JoinArgs a, uint32_t *creator, uint32_t *count, unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o >= a.n_occ) return;
    const uint64_t h = a.hash[o];
    const kw::Found f = find_class<false>(a, o, h, (h << 32) | o);
    if (f.slot == a.slots) {  // (unreachable: every occurrence was inserted)
        creator[o] = (uint32_t)o;
        count[o] = 0;
        atomicOr(err, 2u);
        return;
    }
    const uint32_t c = (uint32_t)f.word;
    creator[o] = c;
    count[o] = c == o ? ((a.flags[o] & 2) ? 1u : 2u) : 0u;
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
    const uint64_t n_occ = 2 * U, max_ids = 2 * n_occ, slots = std::max<uint64_t>(8, 2 * n_occ);

    SeqStore store("sequences", data, off, U, st, device_id);
    t.upload_ms = store.upload_ms;
    PhaseEvents<2> ev;
    ev.mark(0, st);
    JoinArgs a{};
    a.packed = store.packed; a.off = store.off; a.n_occ = n_occ; a.L = (uint32_t)(k - 1); a.slots = slots;
    hu::DeviceArray<unsigned long long> d_hash(n_occ);
    hu::DeviceArray<uint8_t> d_flags(n_occ);
    hu::DeviceArray<unsigned long long> d_table(slots);
    a.hash = d_hash; a.flags = d_flags; a.table = d_table;
    HIP_CHECK(hipMemsetAsync(a.table, 0xFF, slots * 8, st));
    hu::DeviceArray<uint32_t> d_creator(n_occ), d_count(n_occ);
    extract_kernel<<<hu::grid_for(n_occ), hu::EB, 0, st>>>(a);
    insert_kernel<<<hu::grid_for(n_occ), hu::EB, 0, st>>>(a, store.small.err());
    lookup_kernel<<<hu::grid_for(n_occ), hu::EB, 0, st>>>(a, d_creator, d_count, store.small.err());
    HIP_CHECK(hipGetLastError());
    d_table.release();  // (before the next group is taken)
    d_hash.release();
    a.table = nullptr;
    a.hash = nullptr;  // (not read after the lookup)
    hu::DeviceArray<uint64_t> d_first(n_occ);
    hu::ScanScratch<uint64_t> scan(n_occ);
    scan.scan(st, d_count, n_occ, d_first);
    hu::DeviceArray<uint32_t> d_mirror(max_ids), d_from(n_occ), d_to(n_occ);
    hu::DeviceArray<uint64_t> d_weight(n_occ);
    edges_kernel<<<hu::grid_for(U), hu::EB, 0, st>>>(a, d_creator, d_first, d_mirror, d_from, d_to, d_weight);
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);
    unsigned long long n_nodes = 0;
    HIP_CHECK(hipMemcpyAsync(&n_nodes, scan.total(), 8, hipMemcpyDeviceToHost, st));
    store.small.read(st, "plain-FASTA join");
    t.kernel_ms = store.pack_ms + ev.ms(0, 1);
    if (n_nodes > max_ids || n_nodes >= NONE) MTG_DIE("%llu nodes; node ids are 32-bit", n_nodes);

    auto t0 = std::chrono::steady_clock::now();
    PodVec<uint32_t> mirror(std::max<uint64_t>(n_nodes, 1)), from(n_occ), to(n_occ);
    PodVec<uint64_t> weight(n_occ);
    HIP_CHECK(hipMemcpyAsync(mirror.data(), d_mirror, n_nodes * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(from.data(), d_from, n_occ * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(to.data(), d_to, n_occ * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(weight.data(), d_weight, n_occ * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    t.download_ms = ms_since(t0);
    d_flags.release(); d_creator.release(); d_count.release(); d_first.release(); scan.sums.release();  // (before the host builds the graph)
    d_mirror.release(); d_from.release(); d_to.release(); d_weight.release();

    t0 = std::chrono::steady_clock::now();
    HostGraph *g = graph_from_edges(n_nodes, mirror.data(), n_occ, from.data(), to.data(), weight.data());
    t.build_ms = ms_since(t0);
    // What the join kernels must move at the least: ASCII read + packed store written once, per occurrence the packed words of its
    // (k-1)-mer (read by extract, and twice more by insert / lookup beyond k - 1 = 32), hash + flags written, the table's
    // slot touched by insert and lookup plus the occupant's hash, creator + count written and read back, the scan's u32 in and u64
    // out, per unitig its offsets twice, the six output words and the mirror entries.
    const uint64_t words_per_occ = (k - 1 + 15) / 16 + 1;
    t.bytes = store.n_bases + store.n_words * 4 + n_occ * (words_per_occ * 4 * (k - 1 > 32 ? 3 : 1) + 8 + 9 + 2 * (8 + 8 + 8) + 8 + 4 + 8 + 8 + 1) +
              U * (2 * 16 + 2 * 4 + 2 * 8) + n_nodes * 4;
    if (times) *times = t;
    return g;
}

}  // namespace mtg
