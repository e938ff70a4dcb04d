// kmer_compare_device.hip -- do two sequence sets spell the same k-mer set? (`--verify`, mtg_compare_kmer_sets)
//
// The contract: a set is concatenated ASCII plus n + 1 offsets. Its k-mers are the windows of length k that lie inside one record;
// windows are compared by their canonical form (the lexicographically smaller of x and rc(x), A < C < G < T, either case). Records
// shorter than k contribute nothing, a character outside ACGT aborts, k >= 1 (even k and palindromes included). The result
// (mtg_kmer_comparison) holds exact integers only: occurrences and distinct canonical k-mers per set, |A n B|, |A \ B|, |B \ A|,
// and per side the occurrence with the smallest (record, position) whose k-mer the other set lacks.
//
// Both sets live in ONE packed store (A's bases, then B's) with one offsets array, so a window is named by its global base position.
//   pack      ASCII -> 2 bits per base (pack_device.hpp), which also finds the first character outside ACGT
//   insert A  every window of A into one open-addressing table in HBM, membership bit 0
//   insert B  every window of B into the same table, membership bit 1 (an occupied slot of the same k-mer is only marked)
//   count     one pass over the table: slots with bit 0, with bit 1, with both
//   witness   only when a difference exists: every window of a side looks its slot up, and those whose slot lacks the other
//             side's bit take atomicMin on one word -> the smallest global position, which the host turns into (record, position)
// The walk over the windows (kmer_window_device.hpp, shared with the compaction): a thread owns RUN consecutive start positions. It finds the record of the first one by a binary search
// in the offsets and then cuts its run at every record end it meets (no per-base flag array). Inside a record it reads the packed
// words once, front to back, and ROLLS the window: for k <= 31 the forward and the reverse-complement 2-bit codes (2 bits in, 2 bits
// out), beyond that two polynomial hashes mod 2^64 of the forward and the reverse-complement string (one base in, one base out,
// whatever k is; a second reader k bases behind supplies the base that leaves).
//
// Exactness. k <= 31: the slot holds the canonical code itself (code << 2 | membership bits), placed by mix64(code), a bijection --
// equal slots ARE equal k-mers. The all-ones word marks an empty slot: its code would be T...T, which is never canonical.
// k >= 32 (a 64-bit code leaves no room for the two bits, so k = 32 goes this way too): the slot holds a 22-bit tag, the global
// position of one occurrence and the bits; the hash (symmetric in the two strand hashes, so both orientations of a class meet) only
// places and pre-filters -- identity is decided base by base in the packed store, x == y or x == rc(y), 16 bases per compare.
// Nothing probabilistic remains: a hash collision costs a compare, never a wrong answer.
//
// Order independence. Which occurrence represents a class in a slot, and which slot a class ends in, depends on the order the CAS
// land in; no output does: a class has exactly one slot, its bits are set by atomicOr, the counts are integer sums over slots, and a
// witness is a minimum over positions.
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

constexpr unsigned long long EMPTY_SLOT = ~0ull;
constexpr unsigned long long NO_WITNESS = ~0ull;
using kw::RUN;
using kw::POS_LIMIT;
using kw::same_class;
using kw::for_each_window;


struct CompareArgs : kw::WindowArgs {  // packed: A's bases, then B's; off: [records_a + records_b + 1]
    unsigned long long *table;  // [slots]
    uint64_t slots;
};

using kw::Window;
template <bool WIDE>
__device__ __forceinline__ bool slot_holds(const CompareArgs &a, unsigned long long cur, const Window &w) {
    if (!WIDE) return (cur >> 2) == w.ident;
    return (cur >> 42) == (w.ident >> 40) && same_class(a.packed, w.ident & POS_LIMIT, (cur >> 2) & POS_LIMIT, a.k);
}

// insert or mark: afterwards the slot of w's class has `bit` set
template <bool WIDE>
__device__ __forceinline__ void insert_window(const CompareArgs &a, const Window &w, unsigned long long bit, unsigned int *err) {
    const unsigned long long mine = (w.ident << 2) | bit;
    uint64_t s = __umul64hi(w.hash, a.slots);
    for (uint64_t probe = 0; probe < a.slots; probe++) {
        unsigned long long cur = __hip_atomic_load(&a.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY_SLOT) {
            const unsigned long long prev = atomicCAS(&a.table[s], EMPTY_SLOT, mine);
            if (prev == EMPTY_SLOT) return;
            cur = prev;
        }
        if (slot_holds<WIDE>(a, cur, w)) {
            if (!(cur & bit)) atomicOr(&a.table[s], bit);
            return;
        }
        if (++s == a.slots) s = 0;
    }
    atomicOr(err, 1u);  // (2 slots per window: never full)
}
// the membership bits of w's class (every window was inserted)
template <bool WIDE>
__device__ __forceinline__ unsigned lookup_window(const CompareArgs &a, const Window &w, unsigned int *err) {
    uint64_t s = __umul64hi(w.hash, a.slots);
    for (uint64_t probe = 0; probe < a.slots; probe++) {
        const unsigned long long cur = a.table[s];
        if (cur == EMPTY_SLOT) break;
        if (slot_holds<WIDE>(a, cur, w)) return (unsigned)(cur & 3u);
        if (++s == a.slots) s = 0;
    }
    atomicOr(err, 2u);
    return 3u;
}

template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void insert_kernel(CompareArgs a, uint64_t set_lo, uint64_t set_hi, uint64_t rec_lo, uint64_t rec_hi,
                                                         unsigned long long bit, unsigned int *err) {
    const uint64_t p0 = set_lo + hu::gid() * RUN;
    if (p0 >= set_hi) return;
    for_each_window<WIDE>(a, p0, p0 + RUN < set_hi ? p0 + RUN : set_hi, rec_lo, rec_hi,
                          [&](uint64_t, const Window &w) { insert_window<WIDE>(a, w, bit, err); });
}

// *witness = the smallest window start of this set whose class lacks `other_bit`
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void witness_kernel(CompareArgs a, uint64_t set_lo, uint64_t set_hi, uint64_t rec_lo, uint64_t rec_hi,
                                                          unsigned other_bit, unsigned long long *witness, unsigned int *err) {
    const uint64_t p0 = set_lo + hu::gid() * RUN;
    if (p0 >= set_hi) return;
    if (p0 >= __hip_atomic_load(witness, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;  // (a smaller one is known already)
    bool found = false;
    for_each_window<WIDE>(a, p0, p0 + RUN < set_hi ? p0 + RUN : set_hi, rec_lo, rec_hi, [&](uint64_t q, const Window &w) {
        if (found) return;  // (positions ascend within a thread)
        if (!(lookup_window<WIDE>(a, w, err) & other_bit)) {
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

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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
    const uint64_t n_words = (n_bases + 15) / 16, n_occ = r.occurrences_a + r.occurrences_b;
    const uint64_t slots = std::max<uint64_t>(8, (2 * n_occ + 7) / 8 * 8);

    auto t0 = std::chrono::steady_clock::now();
    std::vector<unsigned long long> off_all(n_rec + 1);
    for (uint64_t u = 0; u <= n_a; u++) off_all[u] = off_a[u];
    for (uint64_t u = 1; u <= n_b; u++) off_all[n_a + u] = chars_a + off_b[u];
    char *d_ascii = nullptr;
    uint32_t *d_packed = nullptr;
    unsigned long long *d_off = nullptr, *d_table = nullptr, *d_small = nullptr;
    hu::device_malloc(&d_ascii, n_bases);
    hu::device_malloc(&d_packed, (n_words + 2) * 4);
    hu::device_malloc(&d_off, (n_rec + 1) * 8);
    hu::device_malloc(&d_small, 8 * 8);  // [0] first bad character, [1] error bits, [2..4] counts, [5] witness of A, [6] of B
    HIP_CHECK(hipMemcpyAsync(d_off, off_all.data(), (n_rec + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(d_small, 0, 8 * 8, st));
    HIP_CHECK(hipMemsetAsync(d_small, 0xFF, 8, st));
    HIP_CHECK(hipMemsetAsync(d_small + 5, 0xFF, 16, st));
    HIP_CHECK(hipMemsetAsync(d_packed + n_words, 0, 8, st));
    if (chars_a) hu::upload_sliced(d_ascii, seq_a, chars_a, st, device_id);
    if (r.characters_b) hu::upload_sliced(d_ascii + chars_a, seq_b, r.characters_b, st, device_id);
    HIP_CHECK(hipStreamSynchronize(st));
    t.upload_ms = ms_since(t0);

    hipEvent_t ev[5];
    for (hipEvent_t &e : ev) HIP_CHECK(hipEventCreate(&e));
    unsigned int *d_err = reinterpret_cast<unsigned int *>(d_small + 1);
    HIP_CHECK(hipEventRecord(ev[0], st));
    pack_kernel<<<hu::grid_for(n_words), hu::EB, 0, st>>>(d_ascii, n_bases, d_packed, d_small);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev[1], st));
    hu::device_free(d_ascii);  // (synchronises: the pack is done)
    hu::device_malloc(&d_table, slots * 8);

    CompareArgs a{};
    a.packed = d_packed; a.off = d_off; a.table = d_table; a.slots = slots; a.k = k;
    kw::window_args_set_k(a, k);
    // the sets as position and record ranges; a set without windows is not walked
    const uint64_t lo[2] = {0, chars_a}, hi[2] = {chars_a, n_bases}, rlo[2] = {0, n_a}, rhi[2] = {n_a, n_rec};
    const uint64_t occ[2] = {r.occurrences_a, r.occurrences_b};
    auto insert = [&](int s) {
        if (!occ[s]) return;
        const unsigned grid = hu::grid_for((hi[s] - lo[s] + RUN - 1) / RUN);
        if (wide) insert_kernel<true><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 1ull << s, d_err);
        else insert_kernel<false><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 1ull << s, d_err);
        HIP_CHECK(hipGetLastError());
    };
    HIP_CHECK(hipMemsetAsync(d_table, 0xFF, slots * 8, st));
    insert(0);
    HIP_CHECK(hipEventRecord(ev[2], st));
    insert(1);
    HIP_CHECK(hipEventRecord(ev[3], st));
    count_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(slots / 2), 8192), hu::EB, 0, st>>>(d_table, slots, d_small + 2);
    HIP_CHECK(hipGetLastError());
    unsigned long long h_small[8];
    HIP_CHECK(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (h_small[0] != EMPTY_SLOT) MTG_DIE("sequences: character at offset %llu is not in the DNA alphabet (ACGT)", h_small[0]);
    r.distinct_a = h_small[2];
    r.distinct_b = h_small[3];
    r.common = h_small[4];
    r.only_in_a = r.distinct_a - r.common;
    r.only_in_b = r.distinct_b - r.common;
    for (int s = 0; s < 2; s++) {  // the witnesses: a pass of their own, and only for a side that has one
        if (!(s ? r.only_in_b : r.only_in_a)) continue;
        const unsigned grid = hu::grid_for((hi[s] - lo[s] + RUN - 1) / RUN);
        if (wide) witness_kernel<true><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 2u >> s, d_small + 5 + s, d_err);
        else witness_kernel<false><<<grid, hu::EB, 0, st>>>(a, lo[s], hi[s], rlo[s], rhi[s], 2u >> s, d_small + 5 + s, d_err);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(ev[4], st));
    HIP_CHECK(hipMemcpyAsync(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    float f = 0.f;
    HIP_CHECK(hipEventElapsedTime(&f, ev[0], ev[1])); t.pack_ms = f;
    HIP_CHECK(hipEventElapsedTime(&f, ev[1], ev[2])); t.insert_a_ms = f;  // (with the table's fill)
    HIP_CHECK(hipEventElapsedTime(&f, ev[2], ev[3])); t.insert_b_ms = f;
    HIP_CHECK(hipEventElapsedTime(&f, ev[3], ev[4])); t.count_ms = f;     // (with the witness passes, if any)
    for (hipEvent_t &e : ev) HIP_CHECK(hipEventDestroy(e));
    for (void *p : {(void *)d_packed, (void *)d_off, (void *)d_table, (void *)d_small}) hu::device_free(p);
    if (h_small[1] & 0xFFFFFFFFull) MTG_DIE("k-mer set comparison: internal error %llu (hash table)", h_small[1] & 0xFFFFFFFFull);
    for (int s = 0; s < 2; s++) {
        const unsigned long long w = h_small[5 + s];
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
