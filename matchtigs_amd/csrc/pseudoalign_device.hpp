// pseudoalign_device.hpp -- from per-colour counters to one colour set per fragment and the dictionary of those sets
//
// The colour probes (color_query_kernel on the table, tig_locate_kernel + tp::color_gather_kernel on the sparse index) leave, per query
// record r and colour c < C, hits[r C + c] = the found windows of r whose class's mask has bit c, and per record valid[r] and found[r].
// A FRAGMENT is one record, or -- with mates -- record r of the reads and record r of the mates: both probes are launched into the
// same zeroed arrays and their atomics accumulate, so a row holds the fragment's sums. This header turns the rows into the answer
// without downloading them.
//
// The rule (exact integers; include/mtg_engine.h states it too). denom = found or valid of the fragment (rule.over_valid). Colour c
// is ASSIGNED iff denom >= min_kmers, hits[c] > 0 and hits[c] * 1000 >= permille * denom, in 64 bits (hits < 2^32, denom < 2^41,
// permille <= 1000: both products stay below 2^51). mask[f] = the bits of the assigned colours.
//
//   mask        pseudoalign_mask_kernel: one row per wave per iteration. Lane c loads hits[f C + c] (lanes >= C: 0), every lane
//               evaluates the rule against the fragment's denom, __ballot is the mask; lane 0 stores it. eligible (denom >=
//               min_kmers), assigned (mask != 0) and ambiguous (more than one bit) are wave-uniform and stay in registers; the wave
//               leaves by one atomic instruction, lanes 0..2 adding one total each.
//   dictionary  an open-addressing table keyed by the mask, 0 = empty (unassigned fragments are never inserted), slots = the least
//               power of two >= 2 n and >= 8. pseudoalign_dict_kernel: a thread per fragment; the lanes of a wave that hold the same
//               mask combine first (the loop of unitig_components_device.hip: ballot the pending lanes, broadcast the leader's key,
//               ballot its group), then the leader alone claims the slot by a 64-bit CAS and adds the group's size to fragments[slot]
//               and atomicMin's first[slot] with its own ordinal -- the lowest lane of a group has the lowest ordinal. One CAS / add /
//               min per distinct mask per wave.
//   compact     dict_flag_kernel marks the occupied slots, hu::scan_u32 ranks them, dict_emit_kernel writes (mask, fragments, first)
//               at each rank. Only those triples and the n masks are downloaded.
// Sums, minima and a set of keys: nothing depends on the launch geometry or on the order the atomics land in; the ORDER of the
// triples does (it is the table's), so the host sorts by `first`, which is unique per class.
//
// No LDS, no scratch. The kernels are static: every translation unit that includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device.hpp"
#include "hip_util.hpp"
#include "pack_device.hpp"

namespace mtg {
namespace pa {

using Rule = PseudoalignRule;  // (device.hpp) permille, min_kmers, over_valid: the denominator, 0 found, 1 valid

// counts: [2 n] valid then found; hits: [n C]; masks: [n]; totals: [3] eligible, assigned, ambiguous (zeroed)
static __global__ __launch_bounds__(hu::EB) void pseudoalign_mask_kernel(const uint32_t *hits, const unsigned long long *counts, uint64_t n, uint32_t C,
                                                                         Rule rule, unsigned long long *masks, unsigned long long *totals) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = hu::gid() >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long *denoms = counts + (rule.over_valid ? 0 : n);
    uint32_t eligible = 0, assigned = 0, ambiguous = 0;  // (of this wave's rows; wave-uniform)
    for (uint64_t f = wave; f < n; f += waves) {
        const uint64_t denom = denoms[f];
        const uint64_t h = lane < C ? hits[f * C + lane] : 0;
        const bool on = denom >= rule.min_kmers && h > 0 && h * 1000 >= rule.permille * denom;
        const unsigned long long m = __ballot(on);
        if (lane == 0) masks[f] = m;
        eligible += denom >= rule.min_kmers;
        assigned += m != 0;
        ambiguous += (m & (m - 1)) != 0;
    }
    const uint32_t mine = lane == 0 ? eligible : lane == 1 ? assigned : ambiguous;
    if (lane < 3 && mine) atomicAdd(&totals[lane], (unsigned long long)mine);
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // (splitmix64's finaliser)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// key / fragments: [slots] zeroed, first: [slots] all ones; slots a power of two >= 2 n; fragment i has the ordinal base + i.
// err: bit 0 set if the table was full (2 slots per fragment: never)
static __global__ __launch_bounds__(hu::EB) void pseudoalign_dict_kernel(const unsigned long long *masks, uint64_t n, uint64_t base, uint64_t slots,
                                                                         unsigned long long *key, unsigned long long *fragments, unsigned long long *first,
                                                                         unsigned int *err) {
    const uint64_t i = hu::gid();
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long m = i < n ? masks[i] : 0ull;
    bool pending = m != 0;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int lead = __ffsll(todo) - 1;
        const unsigned long long lead_m = __shfl(m, lead, 64);
        const bool mine = pending && m == lead_m;
        const unsigned long long group = __ballot(mine);
        if (lane == (uint32_t)lead) {  // (the lowest lane of the group: the smallest ordinal)
            uint64_t s = mix64(m) & (slots - 1), tries = 0;
            for (; tries < slots; tries++, s = (s + 1) & (slots - 1)) {
                const unsigned long long cur = atomicCAS(&key[s], 0ull, m);
                if (cur == 0 || cur == m) break;
            }
            if (tries == slots) {
                atomicOr(err, 1u);
            } else {
                atomicAdd(&fragments[s], (unsigned long long)__popcll(group));
                atomicMin(&first[s], (unsigned long long)(base + i));
            }
        }
        if (mine) pending = false;
    }
}

static __global__ __launch_bounds__(hu::EB) void dict_flag_kernel(const unsigned long long *key, uint64_t slots, uint32_t *head) {
    const uint64_t s = hu::gid();
    if (s < slots) head[s] = key[s] != 0;
}

// out: [3 cap] mask, fragments, first; rank[s] = the occupied slots before s
static __global__ __launch_bounds__(hu::EB) void dict_emit_kernel(const unsigned long long *key, const unsigned long long *fragments,
                                                                  const unsigned long long *first, uint64_t slots, const unsigned long long *rank,
                                                                  uint64_t cap, unsigned long long *out) {
    const uint64_t s = hu::gid();
    if (s >= slots || !key[s]) return;
    const uint64_t r = rank[s];
    if (r >= cap) return;  // (at most one class per fragment: never)
    out[r] = key[s];
    out[cap + r] = fragments[s];
    out[2 * cap + r] = first[s];
}

// The rows of n >= 1 fragments (d_hits: [n C], d_counts: [2 n], both complete on st) -> masks[n] on the host and *out (its classes in the table's order, the totals, the last three phases). fn: the caller's name.
inline void reduce(const char *fn, const uint32_t *d_hits, const unsigned long long *d_counts, uint64_t n, uint32_t C, const Rule &rule, uint64_t base,
                   hipStream_t st, int device_id, uint64_t *masks, PseudoalignCall *out) {
    uint64_t slots = 8;
    while (slots < 2 * n) slots *= 2;
    hu::DeviceArray<unsigned long long> d_masks(n), d_totals(3), d_table(3 * slots), d_rank(slots), d_out(3 * n);
    hu::DeviceArray<uint32_t> d_head(slots), d_err(1);
    hu::ScanScratch<unsigned long long> scan(slots);
    unsigned long long *key = d_table, *fragments = d_table + slots, *first = d_table + 2 * slots;
    PhaseEvents<3> ev;
    ev.mark(0, st);
    HIP_CHECK(hipMemsetAsync(d_totals, 0, 3 * 8, st));
    // (a wave per row, up to 2048 blocks of 4 waves -- the waves 256 CUs hold at once; beyond that a wave strides, and fewer waves
    // mean fewer atomics on the three totals)
    const unsigned mask_grid = (unsigned)std::min<uint64_t>(hu::grid_for(n * 64), 2048);
    pseudoalign_mask_kernel<<<mask_grid, hu::EB, 0, st>>>(d_hits, d_counts, n, C, rule, d_masks, d_totals);
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);
    HIP_CHECK(hipMemsetAsync(d_table, 0, 2 * slots * 8, st));
    HIP_CHECK(hipMemsetAsync(first, 0xFF, slots * 8, st));
    HIP_CHECK(hipMemsetAsync(d_err, 0, 4, st));
    pseudoalign_dict_kernel<<<hu::grid_for(n), hu::EB, 0, st>>>(d_masks, n, base, slots, key, fragments, first, d_err);
    dict_flag_kernel<<<hu::grid_for(slots), hu::EB, 0, st>>>(key, slots, d_head);
    HIP_CHECK(hipGetLastError());
    scan.scan(st, d_head, slots, d_rank.get());
    dict_emit_kernel<<<hu::grid_for(slots), hu::EB, 0, st>>>(key, fragments, first, slots, d_rank, n, d_out);
    HIP_CHECK(hipGetLastError());
    ev.mark(2, st);
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long totals[3] = {0, 0, 0}, classes = 0;
    unsigned int err = 0;
    HIP_CHECK(hipMemcpyAsync(totals, d_totals, 3 * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&classes, scan.total(), 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (err || classes > n) MTG_DIE("%s: internal error (the mask dictionary: %u, %llu classes of %llu fragments)", fn, err, classes, (unsigned long long)n);
    hu::download_sliced(masks, d_masks.get(), n * 8, st, device_id);
    out->mask.resize(classes);
    out->fragments.resize(classes);
    out->first.resize(classes);
    hu::download_sliced(out->mask.data(), d_out.get(), classes * 8, st, device_id);
    hu::download_sliced(out->fragments.data(), d_out + n, classes * 8, st, device_id);
    hu::download_sliced(out->first.data(), d_out + 2 * n, classes * 8, st, device_id);
    out->eligible = totals[0];
    out->assigned = totals[1];
    out->ambiguous = totals[2];
    out->mask_ms = ev.ms(0, 1);
    out->dictionary_ms = ev.ms(1, 2);
    out->download_ms = ms_since(t0);
}

}  // namespace pa
}  // namespace mtg
