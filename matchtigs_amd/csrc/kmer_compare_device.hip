// kmer_compare_device.hip -- do two sequence sets spell the same k-mer set? (`--verify`, mtg_compare_kmer_sets)
//
// The contract: a set is concatenated ASCII plus n + 1 offsets. Its k-mers are the windows of length k that lie inside one record;
// windows are compared by their canonical form (the lexicographically smaller of x and rc(x), A < C < G < T, either case). Records
// shorter than k contribute nothing, a character outside ACGT aborts, k >= 1 (even k and palindromes included). The result
// (mtg_kmer_comparison) holds exact integers only: occurrences and distinct canonical k-mers per set, |A n B|, |A \ B|, |B \ A|,
// and per side the occurrence with the smallest (record, position) whose k-mer the other set lacks.
//
// Both sets live in ONE packed store (A's bases, then B's) with one offsets array, so a window is named by its global base position.
//   pack      ASCII -> 2 bits per base (SeqStore, pack_device.hpp), which also finds the first character outside ACGT
//   insert A  every window of A into one open-addressing table in HBM, membership bit 0
//   insert B  every window of B into the same table, membership bit 1 (an occupied slot of the same k-mer is only marked)
//   count     one pass over the table: slots with bit 0, with bit 1, with both
//   witness   only when a difference exists: every window of a side looks its slot up, and those whose slot lacks the other
//             side's bit take atomicMin on one word -> the smallest global position, which the host turns into (record, position)
// The walk over the windows, the table's probe loop and the argument why the table is exact and why no output depends on the order
// the atomics land in are shared with the compaction and the join: kmer_window_device.hpp. What is particular here:
// k <= 31: a slot holds the canonical code itself (code << 2 | membership bits). k >= 32 (a 64-bit code leaves no room for the two
// bits, so k = 32 goes this way too): kw::tagged_pos of one occurrence << 2 | the bits, identity by kw::same_class. A class has one
// slot, its bits are set by atomicOr, the counts are integer sums over slots, and a witness is a minimum over positions.
//
// Table: 64-bit slots, 2 per window of A and B together, linear probing from umulhi(hash, slots). The load is therefore at most
// 0.5 (disjoint sets without repeats) and at most 0.25 for what the check is for, B spelling A's set: 1.2 slots per successful and
// 1.4 per unsuccessful probe, so 19 of 20 operations end in the 64-byte line they start in.
//
// Limits: fewer than 2^40 - 1 bases in A and B together (the position field of a slot), k < 2^32. Beyond them the call aborts.
// Device memory (arena, hip_util.hpp), per base of A and B together with w = windows per base (<= 1): 1 B ASCII (freed once packed)
// + 0.25 B packed + 16 w B table + 8 B per record; the peak is max(1.25, 0.25 + 16 w) B per base + 8 B per record.
// There is no host path: without a GPU a non-empty comparison aborts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"

namespace mtg {

namespace {

constexpr unsigned long long NO_WITNESS = ~0ull;
using kw::EMPTY_SLOT;
using kw::RUN;
using kw::POS_LIMIT;
using kw::for_each_window;
using kw::Window;

struct CompareArgs : kw::WindowArgs {  // packed: A's bases, then B's; off: [records_a + records_b + 1]
    unsigned long long *table;  // [slots]
    uint64_t slots;
};

// the slot of w's class (CLAIM: taken with `mine` if the class has none)
template <bool WIDE, bool CLAIM>
__device__ __forceinline__ kw::Found find_window(const CompareArgs &a, const Window &w, unsigned long long mine) {
    return kw::find_slot<CLAIM>(a.table, a.slots, w.hash, mine, [&](unsigned long long cur) {
        if (!WIDE) return (cur >> 2) == w.ident;
        return (cur >> 42) == (w.ident >> 40) && kw::same_class(a.packed, w.ident & POS_LIMIT, (cur >> 2) & POS_LIMIT, a.k);
    });
}

template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void insert_kernel(CompareArgs a, uint64_t set_lo, uint64_t set_hi, uint64_t rec_lo, uint64_t rec_hi,
                                                         unsigned long long bit, unsigned int *err) {
    const uint64_t p0 = set_lo + hu::gid() * RUN;
    if (p0 >= set_hi) return;
    for_each_window<WIDE>(a, p0, p0 + RUN < set_hi ? p0 + RUN : set_hi, rec_lo, rec_hi,
                          [&](uint64_t, uint64_t, const Window &w) {  // afterwards the slot of w's class has `bit` set
                              const kw::Found f = find_window<WIDE, true>(a, w, (w.ident << 2) | bit);
                              if (f.slot == a.slots) atomicOr(err, 1u);  // (2 slots per window: never full)
                              else if (f.word != EMPTY_SLOT && !(f.word & bit)) atomicOr(&a.table[f.slot], bit);
                          });
}

// *witness = the smallest window start of this set whose class lacks `other_bit`
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void witness_kernel(CompareArgs a, uint64_t set_lo, uint64_t set_hi, uint64_t rec_lo, uint64_t rec_hi,
                                                          unsigned other_bit, unsigned long long *witness, unsigned int *err) {
    const uint64_t p0 = set_lo + hu::gid() * RUN;
    if (p0 >= set_hi) return;
    if (p0 >= __hip_atomic_load(witness, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // (a smaller one is known already)
    bool found = false;
    for_each_window<WIDE>(a, p0, p0 + RUN < set_hi ? p0 + RUN : set_hi, rec_lo, rec_hi, [&](uint64_t q, uint64_t, const Window &w) {
        if (found) return;  // (positions ascend within a thread)
        const kw::Found f = find_window<WIDE, false>(a, w, 0);
        if (f.slot == a.slots) atomicOr(err, 2u);  // (unreachable: every window was inserted)
        else if (!(f.word & other_bit)) {
            found = true;
            atomicMin(witness, (unsigned long long)q);
        }
    });
}

// counts[0] += slots with bit 0, [1] += slots with bit 1, [2] += slots with both
__global__ __launch_bounds__(hu::EB) void count_kernel(const unsigned long long *table, uint64_t slots, unsigned long long *counts) {
    unsigned long long na = 0, nb = 0, nc = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = hu::gid(); s < slots / 2; s += stride) {  // (slots is a multiple of 8)
        const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(table)[s];
        const unsigned fx = v.x == EMPTY_SLOT ? 0u : (unsigned)(v.x & 3), fy = v.y == EMPTY_SLOT ? 0u : (unsigned)(v.y & 3);
        na += (fx & 1) + (fy & 1);
        nb += (fx >> 1) + (fy >> 1);
        nc += (fx == 3) + (fy == 3);
    }
    for (int d = warpSize / 2; d > 0; d /= 2) {
        na += __shfl_down(na, d);
        nb += __shfl_down(nb, d);
        nc += __shfl_down(nc, d);
    }
    if ((threadIdx.x & (warpSize - 1)) == 0) {
        if (na) atomicAdd(&counts[0], na);
        if (nb) atomicAdd(&counts[1], nb);
        if (nc) atomicAdd(&counts[2], nc);
    }
}

// offsets of one set: start at 0, do not decrease; returns its windows
uint64_t check_offsets(const char *what, const char *data, const uint64_t *off, uint64_t n, uint64_t k) {
    if (!off || (n && off[n] && !data)) MTG_DIE("mtg_compare_kmer_sets: null argument (%s)", what);
    if (off[0] != 0) MTG_DIE("mtg_compare_kmer_sets: offsets of %s must start at 0", what);
    uint64_t occ = 0;
    for (uint64_t u = 0; u < n; u++) {
        if (off[u + 1] < off[u]) MTG_DIE("mtg_compare_kmer_sets: offsets of %s decrease at record %llu", what, (unsigned long long)u);
        const uint64_t len = off[u + 1] - off[u];
        if (len >= k) occ += len - k + 1;
    }
    return occ;
}

}  // namespace

void device_compare_kmer_sets(const char *seq_a, const uint64_t *off_a, uint64_t n_a, const char *seq_b, const uint64_t *off_b, uint64_t n_b,
                              uint64_t k, int device_id, mtg_kmer_comparison *out, KmerCompareTimes *times) {
    if (!out) MTG_DIE("mtg_compare_kmer_sets: null argument");
    if (k < 1) MTG_DIE("mtg_compare_kmer_sets: k must be >= 1");
    if (k > 0xFFFFFFFFull) MTG_DIE("mtg_compare_kmer_sets: k too large");
    const auto t_total = std::chrono::steady_clock::now();
    mtg_kmer_comparison r{};
    r.records_a = n_a;
    r.records_b = n_b;
    r.occurrences_a = check_offsets("A", seq_a, off_a, n_a, k);
    r.occurrences_b = check_offsets("B", seq_b, off_b, n_b, k);
    r.characters_a = off_a[n_a];
    r.characters_b = off_b[n_b];
    r.first_only_in_a_record = r.first_only_in_a_pos = r.first_only_in_b_record = r.first_only_in_b_pos = UINT64_MAX;
    KmerCompareTimes t{};
    const uint64_t chars_a = r.characters_a, n_bases = chars_a + r.characters_b, n_rec = n_a + n_b;
    if (n_bases == 0) {  // nothing to look at
        *out = r;
        t.total_ms = ms_since(t_total);
        if (times) *times = t;
        return;
    }
    if (n_bases >= POS_LIMIT)
        MTG_DIE("mtg_compare_kmer_sets: %llu bases in A and B together; the limit is 2^40 - 2", (unsigned long long)n_bases);
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the k-mer set comparison (there is no CPU path)", device_id);
    HIP_CHECK(hipSetDevice(device_id));
    hipStream_t st = nullptr;
    const bool wide = k >= 32;
    const uint64_t n_occ = r.occurrences_a + r.occurrences_b;
    const uint64_t slots = std::max<uint64_t>(8, (2 * n_occ + 7) / 8 * 8);

    std::vector<uint64_t> off_all(n_rec + 1);
    for (uint64_t u = 0; u <= n_a; u++) off_all[u] = off_a[u];
    for (uint64_t u = 1; u <= n_b; u++) off_all[n_a + u] = chars_a + off_b[u];
    SeqStore store("sequences", seq_a, off_all.data(), n_rec, st, device_id, seq_b, r.characters_b);
    ScalarBlock &small = store.small;  // [2..4] counts, [5] witness of A, [6] of B
    HIP_CHECK(hipMemsetAsync(small.d + 5, 0xFF, 16, st));
    t.upload_ms = store.upload_ms;
    t.pack_ms = store.pack_ms;
    PhaseEvents<4> ev;
    ev.mark(0, st);
    hu::DeviceArray<unsigned long long> d_table(slots);

    CompareArgs a{};
    a.packed = store.packed; a.off = store.off; a.table = d_table; a.slots = slots; a.k = k;
    kw::window_args_set_k(a, k);
    // the sets as position and record ranges; a set without windows is not walked
    const uint64_t lo[2] = {0, chars_a}, hi[2] = {chars_a, n_bases}, rlo[2] = {0, n_a}, rhi[2] = {n_a, n_rec};
    const uint64_t occ[2] = {r.occurrences_a, r.occurrences_b};
    auto insert = [&](int s) {
        if (!occ[s]) return;
        const unsigned grid = hu::grid_for((hi[s] - lo[s] + RUN - 1) / RUN);
        if (wide) insert_kernel<true><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 1ull << s, small.err());
        else insert_kernel<false><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 1ull << s, small.err());
        HIP_CHECK(hipGetLastError());
    };
    HIP_CHECK(hipMemsetAsync(d_table, 0xFF, slots * 8, st));
    insert(0);
    ev.mark(1, st);
    insert(1);
    ev.mark(2, st);
    count_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(slots / 2), 8192), hu::EB, 0, st>>>(d_table, slots, small.d + 2);
    HIP_CHECK(hipGetLastError());
    small.read(st, "k-mer set comparison");
    r.distinct_a = small.h[2];
    r.distinct_b = small.h[3];
    r.common = small.h[4];
    r.only_in_a = r.distinct_a - r.common;
    r.only_in_b = r.distinct_b - r.common;
    for (int s = 0; s < 2; s++) {  // the witnesses: a pass of their own, and only for a side that has one
        if (!(s ? r.only_in_b : r.only_in_a)) continue;
        const unsigned grid = hu::grid_for((hi[s] - lo[s] + RUN - 1) / RUN);
        if (wide) witness_kernel<true><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 2u >> s, small.d + 5 + s, small.err());
        else witness_kernel<false><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 2u >> s, small.d + 5 + s, small.err());
        HIP_CHECK(hipGetLastError());
    }
    ev.mark(3, st);
    small.read(st, "k-mer set comparison");
    t.insert_a_ms = ev.ms(0, 1);  // (with the table's fill)
    t.insert_b_ms = ev.ms(1, 2);
    t.count_ms = ev.ms(2, 3);     // (with the witness passes, if any)
    d_table.release();
    for (int s = 0; s < 2; s++) {
        const unsigned long long w = small.h[5 + s];
        if ((s ? r.only_in_b : r.only_in_a) == 0) continue;
        if (w == NO_WITNESS) MTG_DIE("k-mer set comparison: internal error (no witness for a difference)");
        // the record that holds position w: the last one that starts at or before it
        const uint64_t rec = (uint64_t)(std::upper_bound(off_all.begin() + rlo[s], off_all.begin() + rhi[s] + 1, w) - off_all.begin()) - 1;
        (s ? r.first_only_in_b_record : r.first_only_in_a_record) = rec - rlo[s];
        (s ? r.first_only_in_b_pos : r.first_only_in_a_pos) = w - off_all[rec];
    }
    *out = r;
    t.total_ms = ms_since(t_total);
    if (times) *times = t;
}

}  // namespace mtg
