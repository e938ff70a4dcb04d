// kmer_query_device.hip -- which k-mers of these sequences are in that set? (`--query-fa`, mtg_kmer_index_*)
//
// The contract. The INDEX is a sequence set in the comparison's sense (kmer_compare_device.hip): concatenated ASCII plus n + 1
// offsets, its k-mers the windows of length k inside one record, taken by their canonical form (the lexicographically smaller of x
// and rc(x), A < C < G < T, either case); records shorter than k contribute nothing, a character outside ACGT aborts, k >= 1.
// A QUERY is n records of arbitrary bytes. For record r of length L: kmers[r] = max(0, L - k + 1) windows; a window is VALID iff
// all k of its characters are in ACGTacgt; valid[r] counts the valid windows and found[r] those whose canonical form is in the
// index. Optionally two bit arrays over the global base positions of the query: bit p & 63 of word p >> 6 of valid_bits is set iff
// a valid window starts at p, of present_bits iff that window is in the index; every other bit is 0. Exact integers only, and
// nothing depends on the launch geometry or on the order atomics land in (the counts are integer sums; a bit-array word has one
// writer).
//
// Build (once per index):
//   pack      ASCII -> 2 bits per base (SeqStore), which also finds the first character outside ACGT
//   insert    every window into one open-addressing table in HBM (kw::find_slot), 2 slots per window. A slot names its class as
//             in the comparison: k <= 31 the canonical code itself, k >= 32 kw::tagged_pos of one occurrence, identity settled by
//             kw::same_class in the packed store
//   count     one sweep over the table: the occupied slots are the distinct k-mers
// The index then keeps the table and -- for k >= 32, where a slot points into them -- the packed bases; the ASCII, the offsets
// and, for k <= 31, the packed bases go back to the arena. Both live until mtg_kmer_index_free: they are live ranges of the device
// arena, which gives only entirely free chunks back to the driver (mtg_release_device_memory included).
//
// Query (any number of calls per index, read-only):
//   pack      ASCII -> 2 bits per base plus one "bad" bit per base for what is not ACGT (MaskedSeqStore; packed as A)
//   probe     a thread owns kw::RUN = 64 window starts, p0 = 64 gid: exactly one word of each bit array, which it writes with one
//             plain store. It rolls over its windows (kw::for_each_window). Validity comes from the bad mask: the thread keeps
//             `clear_from`, one past the last bad base at or before the window's last base q + k - 1; where the walk jumps (the
//             start of the run, a new record) it finds that by scanning the mask words over [q, q + k - 1), from then on one bit
//             per step. A window is valid iff clear_from <= q. Invalid windows are not probed. Valid ones are looked up
//             (find_slot<false>: no write to the table); for k >= 32 identity compares the QUERY's packed bases with the INDEX's
//             (the two-store kw::same_class). valid / found accumulate in registers and leave by one atomicAdd each per
//             (thread, record), skipped when zero.
//
// Limits: fewer than 2^40 - 1 bases in the index and in one query call (the position field of a slot, the walk), k < 2^32.
// Device memory of an index: 16 B per window (+ 0.25 B per base for k >= 32); its build peaks like the comparison. A query call
// takes 1 B (ASCII, freed once packed) + 0.25 B + 0.125 B per base, 8 + 16 B per record and 0.25 B per base for the bit arrays.
// There is no host path.
//
// Locate (a LOCATING index only, mtg_kmer_index_build_locating). Such an index also keeps where[slots], the smallest
// window start of every class (atomicMin in the insert kernel), the packed bases for every k and the record offsets: 16 B more per
// window, 0.25 B per base, 8 B per record. A locate call answers like a query without bit arrays and adds the maximal collinear
// runs of the found windows (include/mtg_engine.h states the contract):
//   pack      as the query
//   probe     locate_kernel: the query's walk (probe_run, shared with query_kernel); per found window hit[p] = (t << 1) | strand,
//             t = where[slot], strand from a forward compare of the query's packed bases with the index's at t
//   runs      (kmer_runs_device.hpp, shared with the sparse index) run_flag_kernel marks the windows that do not continue their
//             predecessor, hu::scan_u32 ranks them, run_mark_kernel notes the first and last position of every run, run_emit_kernel
//             writes the fields of each
// Only the runs and the counts are downloaded. A call takes 8 + 4 + 8 B per query base beside the query's store.
//
// Thread (a LOCATING index only). The same pack, probe and runs, the runs left on the device (kr::RunStage), then
//   walks     (kmer_walks_device.hpp, shared with the sparse index) the runs joined across record ends into walks, those of at least
//             min_kmers windows compacted with their steps
// Only the kept walks, their steps and the counts are downloaded.
//
// Abundance (a WEIGHTED index only, mtg_kmer_index_build_weighted). The caller gives one uint32 per window of the indexed
// sequences, in window order; weight(class) = the weight of the class's smallest window start, loc of DESIGN.md 18 -- a function of
// the input alone. The build runs the locating insert and then weight_gather_kernel, one sweep over the slots: weight[s] =
// weights[ordinal(where[s])], 4 B per slot = 8 B per window more. An index that is not also locating then gives where[], the offsets
// and, for k <= 31, the packed bases back to the arena. An abundance call answers like a query without bit arrays and adds per record
// the sum (64-bit), the smallest and the largest weight over its found windows, and optionally the weight at every window start:
//   pack      as the query
//   probe     abundance_kernel: the query's walk (probe_run); per found window weight[slot], folded into three registers per
//             (thread, record) that leave by one atomicAdd, one atomicMin and one atomicMax when the record changes, never per window.
//             per_window: a thread is the only writer of its RUN positions, zeros included
// A call takes 8 + 4 + 4 B per record and, with per_window, 4 B per query base beside the query's store.
//
// Colours (a COLOURED index only, mtg_kmer_index_build_annotated). The caller gives one 64-bit mask per window of the
// indexed sequences; color(class) = the mask of the class's smallest window start, gathered like the weights (color_gather_kernel,
// 8 B per slot; an index with both payloads runs both gathers off one where[]). A colour call answers like a query without bit arrays
// and adds per record and colour c < n_colors the found windows whose class's mask has bit c, and optionally the mask at every window:
//   probe     color_query_kernel: the query's walk (probe_run); the thread keeps (record, mask, run length): a found window with the
//             same record and mask only lengthens the run -- absent and invalid windows in between do not break it, only sums leave
//             --, and a change of either, or the end of the walk, flushes it: one atomicAdd(per_color[r C + c], run) per set bit c.
//             Worst case: masks that alternate from window to window cost popcount(mask) atomics per window.
// A call takes 4 C B per record and, with per_window, 8 B per query base beside the query's store.
//
// Tally (any index, mtg_kmer_tally_*). The opposite question: how often did these reads see each k-mer of the set? A
// tally is one 64-bit counter per slot of one index, 8 B per slot = 16 B per window, zero at creation; the index is not changed.
//   add       tally_kernel: the query's walk (probe_run); per found window tally[slot] += 1. The thread keeps (slot, run length):
//             a found window on the same slot only lengthens the run, a change of slot or the end of the walk flushes one 64-bit
//             atomicAdd(&tally[slot], run) whose result is not read. A homopolymer costs one atomic per thread; distinct k-mers
//             one random 8-byte atomic per found window
//   coverage  coverage_kernel: abundance_kernel reading tally[slot] for weight[slot]; per (thread, record) covered / sum / max in
//             registers, out by two atomicAdds and one 64-bit atomicMax when the record changes. per_window as there, 64-bit
// Integer sums and maxima: nothing depends on the launch geometry or on the order the atomics land in. A call is limited like a
// query (fewer than 2^40 - 1 bases), so a counter cannot overflow. Coverage takes 8 + 8 + 8 B per record and, with per_window,
// 8 B per base beside the query's store.
//
// Pseudoalignment (a COLOURED index only, mtg_pseudoaligner_*). The colour call's counters stay on the device: the
// unchanged color_query_kernel runs once for the reads and, with mates, once more for the mates into the same per_color and counts,
// and pseudoalign_device.hpp turns every row into one mask and the masks into their dictionary. Only 4 x 8 B per fragment and the
// classes come back. A call takes (4 C + 16) B per fragment beside one side's store, then at most 180 B per fragment for the masks and the dictionary.
//
// Correction (any index, mtg_kmer_index_correct). The way back: the unchanged query_kernel gives both bit arrays, and
// kmer_correct_device.hpp flags the bases no present window covers, tries the three other bases of each on the table, one wave per
// candidate, and XORs the accepted substitutions into the reads' packed store; the query pass then runs again, per round and once
// more for found_after. Only five words per record and the substitutions come back. A call takes 0.25 B per base for the bit arrays,
// 0.3 B per base for the candidate words and their ranks, 8 + 16 + 16 B per record and 21 B per candidate beside the query's store.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_correct_device.hpp"
#include "kmer_runs_device.hpp"
#include "kmer_walks_device.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"
#include "pseudoalign_device.hpp"

namespace mtg {

namespace {

using kr::NO_HIT;
using kr::record_of;
using kr::same_forward;
using kw::EMPTY_SLOT;
using kw::POS_LIMIT;
using kw::RUN;
using kw::Window;

struct IndexArgs : kw::WindowArgs {  // packed / off: the sequences that are walked (build: the index's, query: the query's)
    const uint32_t *index_packed;    // k >= 32: the bases the slots point into
    unsigned long long *table;       // [slots]
    uint64_t slots;
};

// the slot of w's class; w is a window of a.packed (CLAIM: taken with w.ident if the class has none)
template <bool WIDE, bool CLAIM>
__device__ __forceinline__ kw::Found find_window(const IndexArgs &a, const Window &w) {
    return kw::find_slot<CLAIM>(a.table, a.slots, w.hash, w.ident, [&](unsigned long long cur) {
        if (!WIDE) return cur == w.ident;
        if ((cur >> 40) != (w.ident >> 40)) return false;
        if (CLAIM) return kw::same_class(a.packed, w.ident & POS_LIMIT, cur & POS_LIMIT, a.k);
        return kw::same_class(a.packed, w.ident & POS_LIMIT, a.index_packed, cur & POS_LIMIT, a.k);
    });
}

// LOCATE: where[slot of the class] = the smallest window start of the class (where: [slots], all ones before). A claimed slot keeps
// its class, and the minimum over the occurrences of a class does not depend on the order they arrive in.
template <bool WIDE, bool LOCATE>
__global__ __launch_bounds__(hu::EB) void index_insert_kernel(IndexArgs a, uint64_t n_bases, uint64_t n_rec, unsigned int *err,
                                                              unsigned long long *where) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    kw::for_each_window<WIDE>(a, p0, p0 + RUN < n_bases ? p0 + RUN : n_bases, 0, n_rec, [&](uint64_t q, uint64_t, const Window &w) {
        const uint64_t slot = find_window<WIDE, true>(a, w).slot;
        if (slot == a.slots) atomicOr(err, 1u);  // (2 slots per window: never full)
        else if (LOCATE) atomicMin(&where[slot], (unsigned long long)q);
    });
}

// *count += occupied slots
__global__ __launch_bounds__(hu::EB) void index_count_kernel(const unsigned long long *table, uint64_t slots, unsigned long long *count) {
    unsigned long long n = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = hu::gid(); s < slots / 2; s += stride) {  // (slots is a multiple of 8)
        const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(table)[s];
        n += (v.x != EMPTY_SLOT) + (v.y != EMPTY_SLOT);
    }
    for (int d = warpSize / 2; d > 0; d /= 2) n += __shfl_down(n, d);
    if ((threadIdx.x & (warpSize - 1)) == 0 && n) atomicAdd(count, n);
}

// one past the last base of [lo, hi) whose bit is set in `bad`; lo if there is none
__device__ __forceinline__ uint64_t past_last_bad(const unsigned long long *bad, uint64_t lo, uint64_t hi) {
    if (hi <= lo) return lo;
    uint64_t w = (hi - 1) >> 6;
    const uint64_t w_lo = lo >> 6;
    unsigned long long m = bad[w] & (~0ull >> (63 - ((hi - 1) & 63)));
    for (;;) {
        if (w == w_lo) m &= ~0ull << (lo & 63);
        if (m) return (w << 6) + 64 - (uint64_t)__clzll((long long)m);
        if (w == w_lo) return lo;
        m = bad[--w];
    }
}

// The walk of both query kernels over the RUN window starts from p0 on: validity from the bad mask, the read-only lookup of the valid
// windows, valid / found per record into counts ([2 n_rec], valid then found). vbits / pbits: bit q - p0 set for a valid / a found
// window at q. hit(q, r, slot) is called for every found window with its record and the slot of its class.
template <bool WIDE, typename Hit>
__device__ __forceinline__ void probe_run(const IndexArgs &a, const unsigned long long *bad, uint64_t p0, uint64_t n_bases, uint64_t n_rec,
                                          unsigned long long *counts, unsigned long long &vbits, unsigned long long &pbits, Hit hit) {
    uint64_t rec = ~0ull, next_q = ~0ull, clear_from = 0;
    uint32_t n_valid = 0, n_found = 0;  // (of the current record; at most RUN)
    auto flush = [&]() {
        if (n_valid) atomicAdd(&counts[rec], (unsigned long long)n_valid);
        if (n_found) atomicAdd(&counts[n_rec + rec], (unsigned long long)n_found);
        n_valid = n_found = 0;
    };
    kw::for_each_window<WIDE>(a, p0, p0 + RUN < n_bases ? p0 + RUN : n_bases, 0, n_rec, [&](uint64_t q, uint64_t r, const Window &w) {
        const uint64_t last = q + a.k - 1;  // the window's last base
        if (r != rec) {
            flush();
            rec = r;
        }
        if (q != next_q) clear_from = past_last_bad(bad, q, last);  // the walk jumped: what it knew lies behind q
        next_q = q + 1;
        if ((bad[last >> 6] >> (last & 63)) & 1) clear_from = last + 1;
        if (clear_from > q) return;  // a bad base inside the window
        const unsigned long long bit = 1ull << (q - p0);
        n_valid++;
        vbits |= bit;
        const uint64_t slot = find_window<WIDE, false>(a, w).slot;
        if (slot != a.slots) {
            n_found++;
            pbits |= bit;
            hit(q, r, slot);
        }
    });
    flush();
}

// counts: [2 n_rec], valid then found; valid_bits / present_bits: [(n_bases + 63) / 64] or null
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void query_kernel(IndexArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                       unsigned long long *counts, unsigned long long *valid_bits,
                                                       unsigned long long *present_bits) {
    const uint64_t gid = hu::gid(), p0 = gid * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0;
    probe_run<WIDE>(a, bad, p0, n_bases, n_rec, counts, vbits, pbits, [](uint64_t, uint64_t, uint64_t) {});
    if (valid_bits) valid_bits[gid] = vbits;
    if (present_bits) present_bits[gid] = pbits;
}

// ---- locate ----
// (NO_HIT, same_forward and everything from the hits to the runs: kmer_runs_device.hpp, shared with the sparse index)

// query_kernel's walk; per found window at q: hit[q] = (t << 1) | strand, t = the smallest window start of its class in the index
// (where[slot]), strand 0 iff the query's bases equal the index's at t one by one -- otherwise, the classes being equal, they are the
// reverse complement. hit: [n_bases], NO_HIT before.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void locate_kernel(IndexArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                        unsigned long long *counts, const unsigned long long *where, unsigned long long *hit) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0;
    probe_run<WIDE>(a, bad, p0, n_bases, n_rec, counts, vbits, pbits, [&](uint64_t q, uint64_t, uint64_t slot) {
        const uint64_t t = where[slot];
        hit[q] = (t << 1) | (same_forward(a.packed, q, a.index_packed, t, a.k) ? 0ull : 1ull);
    });
}

// ---- abundance ----
// weight[s] = the caller's weight of the window where[s], the smallest window start of the slot's class; 0 for an empty slot.
// win_off[r] = the windows of the records before r, so the window at t of record r has the ordinal win_off[r] + t - off[r].
__global__ __launch_bounds__(hu::EB) void weight_gather_kernel(const unsigned long long *table, const unsigned long long *where,
                                                                const unsigned long long *off, uint64_t n_rec, const unsigned long long *win_off,
                                                                const uint32_t *weights, uint64_t n_weights, uint64_t slots, uint32_t *weight,
                                                                unsigned int *err) {
    const uint64_t s = hu::gid();
    if (s >= slots) return;
    uint32_t w = 0;
    if (table[s] != EMPTY_SLOT) {
        const uint64_t t = where[s], r = record_of(off, n_rec, t), i = win_off[r] + (t - off[r]);
        if (i < n_weights) w = weights[i];
        else atomicOr(err, 2u);  // (every occupied slot has a window's position: never)
    }
    weight[s] = w;
}

// query_kernel's walk; per found window the weight of its class. counts: [3 n_rec] valid, found, then the sum of the weights;
// minmax: [2 n_rec] the smallest (all ones before) and the largest (0 before) weight; per_window: [n_bases] or null.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void abundance_kernel(IndexArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                           unsigned long long *counts, const uint32_t *weight, uint32_t *minmax,
                                                           uint32_t *per_window) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0;
    uint64_t rec = 0, sum = 0, next_p = p0;  // next_p: the first position of the run that per_window has not been told yet
    uint32_t lo = ~0u, hi = 0, hits = 0;     // (of the record `rec`; at most RUN hits)
    auto flush = [&]() {
        if (!hits) return;
        atomicAdd(&counts[2 * n_rec + rec], (unsigned long long)sum);
        atomicMin(&minmax[rec], lo);
        atomicMax(&minmax[n_rec + rec], hi);
        sum = 0; lo = ~0u; hi = 0; hits = 0;
    };
    probe_run<WIDE>(a, bad, p0, n_bases, n_rec, counts, vbits, pbits, [&](uint64_t q, uint64_t r, uint64_t slot) {
        if (r != rec) {
            flush();
            rec = r;
        }
        const uint32_t w = weight[slot];
        sum += w;
        lo = w < lo ? w : lo;
        hi = w > hi ? w : hi;
        hits++;
        if (per_window) {
            for (; next_p < q; next_p++) per_window[next_p] = 0;
            per_window[next_p++] = w;
        }
    });
    flush();
    if (per_window)
        for (const uint64_t end = p0 + RUN < n_bases ? p0 + RUN : n_bases; next_p < end; next_p++) per_window[next_p] = 0;
}

// ---- colours ----
// weight_gather_kernel for a 64-bit payload: color[s] = the caller's mask of the window where[s]; 0 for an empty slot
__global__ __launch_bounds__(hu::EB) void color_gather_kernel(const unsigned long long *table, const unsigned long long *where,
                                                               const unsigned long long *off, uint64_t n_rec, const unsigned long long *win_off,
                                                               const unsigned long long *colors, uint64_t n_colors_words, uint64_t slots,
                                                               unsigned long long *color, unsigned int *err) {
    const uint64_t s = hu::gid();
    if (s >= slots) return;
    unsigned long long c = 0;
    if (table[s] != EMPTY_SLOT) {
        const uint64_t t = where[s], r = record_of(off, n_rec, t), i = win_off[r] + (t - off[r]);
        if (i < n_colors_words) c = colors[i];
        else atomicOr(err, 2u);  // (every occupied slot has a window's position: never)
    }
    color[s] = c;
}

// query_kernel's walk; per found window the mask of its class. counts: [2 n_rec] valid, found; per_color: [n_rec * C], zeroed;
// (no mask has a bit from C on: the build checked); per_window: [n_bases] or null.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void color_query_kernel(IndexArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                             unsigned long long *counts, const unsigned long long *color, uint32_t C,
                                                             uint32_t *per_color, unsigned long long *per_window) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0, mask = 0;
    uint64_t rec = 0, next_p = p0;  // next_p: the first position of the run that per_window has not been told yet
    uint32_t run = 0;               // found windows of record `rec` with the mask `mask` since the last flush (at most RUN)
    auto flush = [&]() {
        for (unsigned long long m = run ? mask : 0ull; m; m &= m - 1)
            atomicAdd(&per_color[rec * C + (uint32_t)__builtin_ctzll(m)], run);
        run = 0;
    };
    probe_run<WIDE>(a, bad, p0, n_bases, n_rec, counts, vbits, pbits, [&](uint64_t q, uint64_t r, uint64_t slot) {
        const unsigned long long m = color[slot];
        if (r != rec || m != mask) {
            flush();
            rec = r;
            mask = m;
        }
        run++;
        if (per_window) {
            for (; next_p < q; next_p++) per_window[next_p] = 0;
            per_window[next_p++] = m;
        }
    });
    flush();
    if (per_window)
        for (const uint64_t end = p0 + RUN < n_bases ? p0 + RUN : n_bases; next_p < end; next_p++) per_window[next_p] = 0;
}

// ---- tally ----
// query_kernel's walk; per found window tally[slot of its class] += 1 (tally: [slots], 64-bit). The thread keeps (slot, run length):
// a found window on the slot of the found window before it only lengthens the run -- absent and invalid windows and a change of
// record in between do not break it, only sums leave --, and a change of slot, or the end of the walk, flushes it: one
// atomicAdd(&tally[slot], run) whose result nobody reads. Worst case: classes that alternate from window to window, one atomic each.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void tally_kernel(IndexArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                       unsigned long long *counts, unsigned long long *tally) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0;
    uint64_t cur = 0;  // the slot of the run (a slot is < a.slots: the walk calls hit only with one it found)
    uint32_t run = 0;  // found windows on `cur` since the last flush (at most RUN)
    probe_run<WIDE>(a, bad, p0, n_bases, n_rec, counts, vbits, pbits, [&](uint64_t, uint64_t, uint64_t slot) {
        if (slot != cur) {
            if (run) atomicAdd(&tally[cur], (unsigned long long)run);
            cur = slot;
            run = 0;
        }
        run++;
    });
    if (run) atomicAdd(&tally[cur], (unsigned long long)run);
}

// abundance_kernel with tally[slot] in place of weight[slot]. counts: [5 n_rec] valid, found, then the found windows whose class
// has a tally > 0, the sum of the tallies and the largest tally (all 0 before); per_window: [n_bases] or null.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void coverage_kernel(IndexArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                          unsigned long long *counts, const unsigned long long *tally,
                                                          unsigned long long *per_window) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0;
    uint64_t rec = 0, sum = 0, hi = 0, next_p = p0;  // next_p: the first position of the run that per_window has not been told yet
    uint32_t covered = 0, hits = 0;                  // (of the record `rec`; at most RUN hits)
    auto flush = [&]() {
        if (!hits) return;
        if (covered) {  // (else the sum and the largest are 0 too)
            atomicAdd(&counts[2 * n_rec + rec], (unsigned long long)covered);
            atomicAdd(&counts[3 * n_rec + rec], (unsigned long long)sum);
            atomicMax(&counts[4 * n_rec + rec], (unsigned long long)hi);
        }
        sum = 0; hi = 0; covered = 0; hits = 0;
    };
    probe_run<WIDE>(a, bad, p0, n_bases, n_rec, counts, vbits, pbits, [&](uint64_t q, uint64_t r, uint64_t slot) {
        if (r != rec) {
            flush();
            rec = r;
        }
        const uint64_t t = tally[slot];
        covered += t != 0;
        sum += t;
        hi = t > hi ? t : hi;
        hits++;
        if (per_window) {
            for (; next_p < q; next_p++) per_window[next_p] = 0;
            per_window[next_p++] = t;
        }
    });
    flush();
    if (per_window)
        for (const uint64_t end = p0 + RUN < n_bases ? p0 + RUN : n_bases; next_p < end; next_p++) per_window[next_p] = 0;
}

// offsets of one set: start at 0, do not decrease; returns its windows
uint64_t check_offsets(const char *fn, const char *data, const uint64_t *off, uint64_t n, uint64_t k) {
    if (!off || (n && off[n] && !data)) MTG_DIE("%s: null argument", fn);
    if (off[0] != 0) MTG_DIE("%s: offsets must start at 0", fn);
    uint64_t occ = 0;
    for (uint64_t u = 0; u < n; u++) {
        if (off[u + 1] < off[u]) MTG_DIE("%s: offsets decrease at record %llu", fn, (unsigned long long)u);
        const uint64_t len = off[u + 1] - off[u];
        if (len >= k) occ += len - k + 1;
    }
    return occ;
}

}  // namespace

struct KmerIndex {
    mtg_kmer_index_info info{};
    int device_id = 0;
    hu::DeviceArray<uint32_t> packed;            // k >= 32, or locating
    hu::DeviceArray<unsigned long long> table;   // [info.slots]
    bool locating = false;
    hu::DeviceArray<unsigned long long> where;   // locating: [info.slots] the smallest window start of the slot's class
    hu::DeviceArray<unsigned long long> off;     // locating: [info.records + 1]
    hu::DeviceArray<uint32_t> weight;            // weighted: [info.slots] the weight of the slot's class
    hu::DeviceArray<unsigned long long> color;   // coloured: [info.slots] the colour mask of the slot's class
    uint64_t n_colors = 0;                // coloured: 1 .. 64
};

namespace {

// What the probe calls of an index share (query, abundance, colors, locate). probe_windows: the checks of the query, kmers[] filled,
// valid[] and found[] zeroed; returns the query's bases (missing: an out-pointer of the caller's own is null).
uint64_t probe_windows(const char *fn, uint64_t k, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                       bool missing) {
    (void)check_offsets(fn, seq, off, n, k);
    if (missing || (n && (!kmers || !valid || !found))) MTG_DIE("%s: null argument", fn);
    if (off[n] >= POS_LIMIT) MTG_DIE("%s: %llu bases; the limit is 2^40 - 2", fn, (unsigned long long)off[n]);
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = off[r + 1] - off[r];
        kmers[r] = len >= k ? len - k + 1 : 0;
        valid[r] = found[r] = 0;
    }
    return off[n];
}

int on_device(int device_id) {
    HIP_CHECK(hipSetDevice(device_id));
    return device_id;
}

// ... and one probe of a query that has bases: the query on the index's device, the kernels' arguments and the counters ([words * n]:
// valid, found, then the caller's own). The caller allocates what else it needs, calls start(), launches its kernels between the marks
// of ev and fetches valid and found with download_counts(); the phases every probe reports are in booked().
template <int EVENTS = 2>
struct Probe {
    const uint64_t n, words;
    const bool wide;  // the kernels' WIDE
    const int device_id;
    hipStream_t st = nullptr;
    MaskedSeqStore store;
    hu::DeviceArray<unsigned long long> d_counts;
    IndexArgs a{};
    PhaseEvents<EVENTS> ev;

    Probe(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t words)
        : n(n), words(words), wide(ix->info.k >= 32), device_id(on_device(ix->device_id)), store(seq, off, n, st, device_id) {
        d_counts.alloc(words * n);
        a.packed = store.packed; a.off = store.off; a.index_packed = ix->packed; a.table = ix->table; a.slots = ix->info.slots;
        kw::window_args_set_k(a, ix->info.k);
    }
    unsigned run_grid() const { return hu::grid_for((store.n_bases + RUN - 1) / RUN); }  // one thread per run of window starts
    void start() {
        ev.mark(0, st);
        HIP_CHECK(hipMemsetAsync(d_counts, 0, words * n * 8, st));
    }
    void download_counts(uint64_t *valid, uint64_t *found) {
        HIP_CHECK(hipMemcpyAsync(valid, d_counts, n * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(found, d_counts + n, n * 8, hipMemcpyDeviceToHost, st));
    }
    void booked(double *upload_ms, double *pack_ms, double *probe_ms) {
        *upload_ms = store.upload_ms;
        *pack_ms = store.pack_ms;
        *probe_ms = ev.ms(0, 1);
    }
};

}  // namespace

KmerIndex *device_kmer_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, int device_id, bool locating,
                                   KmerQueryTimes *times, const KmerWeights *weights, const KmerColors *colors) {
    if (k < 1) MTG_DIE("mtg_kmer_index_build: k must be >= 1");
    if (k > 0xFFFFFFFFull) MTG_DIE("mtg_kmer_index_build: k too large");
    KmerIndex *ix = new KmerIndex();
    mtg_kmer_index_info &info = ix->info;
    info.k = k;
    info.records = n;
    info.occurrences = check_offsets("mtg_kmer_index_build", seq, off, n, k);
    info.characters = off[n];
    if (info.characters >= POS_LIMIT)
        MTG_DIE("mtg_kmer_index_build: %llu bases; the limit is 2^40 - 2", (unsigned long long)info.characters);
    if (weights && weights->n != info.occurrences)
        MTG_DIE("mtg_kmer_index_build_weighted: %llu weights for %llu windows", (unsigned long long)weights->n, (unsigned long long)info.occurrences);
    if (weights && weights->n && !weights->w) MTG_DIE("mtg_kmer_index_build_weighted: null argument");
    if (colors && (colors->n_colors < 1 || colors->n_colors > 64))
        MTG_DIE("mtg_kmer_index_build_annotated: %llu colours; 1 .. 64 are served", (unsigned long long)colors->n_colors);
    if (colors && colors->n != info.occurrences)
        MTG_DIE("mtg_kmer_index_build_annotated: %llu colour words for %llu windows", (unsigned long long)colors->n, (unsigned long long)info.occurrences);
    if (colors && colors->n && !colors->c) MTG_DIE("mtg_kmer_index_build_annotated: null argument");
    if (colors && colors->n_colors < 64)  // (the probe adds into per_color[r C + c] for every set bit c)
        for (uint64_t i = 0; i < colors->n; i++)
            if (colors->c[i] >> colors->n_colors)
                MTG_DIE("mtg_kmer_index_build_annotated: mask %llu has a colour beyond the %llu given", (unsigned long long)i,
                        (unsigned long long)colors->n_colors);
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the k-mer index (there is no CPU path)", device_id);
    HIP_CHECK(hipSetDevice(device_id));
    ix->device_id = device_id;
    hipStream_t st = nullptr;
    const bool wide = k >= 32;
    info.slots = std::max<uint64_t>(8, (2 * info.occurrences + 7) / 8 * 8);

    SeqStore store("indexed sequences", seq, off, n, st, device_id);
    PhaseEvents<2> ev;
    ev.mark(0, st);
    ix->table.alloc(info.slots);
    HIP_CHECK(hipMemsetAsync(ix->table, 0xFF, info.slots * 8, st));
    ix->locating = locating;
    const bool positions = locating || weights || colors;  // the insert notes the smallest window start of every class
    if (positions) {
        ix->where.alloc(info.slots);
        HIP_CHECK(hipMemsetAsync(ix->where, 0xFF, info.slots * 8, st));
    }
    if (info.occurrences) {
        IndexArgs a{};
        a.packed = a.index_packed = store.packed; a.off = store.off; a.table = ix->table; a.slots = info.slots;
        kw::window_args_set_k(a, k);
        const unsigned grid = hu::grid_for((store.n_bases + RUN - 1) / RUN);
        if (positions) {
            if (wide) index_insert_kernel<true, true><<<grid, hu::EB, 0, st>>>(a, store.n_bases, n, store.small.err(), ix->where);
            else index_insert_kernel<false, true><<<grid, hu::EB, 0, st>>>(a, store.n_bases, n, store.small.err(), ix->where);
        } else {
            if (wide) index_insert_kernel<true, false><<<grid, hu::EB, 0, st>>>(a, store.n_bases, n, store.small.err(), nullptr);
            else index_insert_kernel<false, false><<<grid, hu::EB, 0, st>>>(a, store.n_bases, n, store.small.err(), nullptr);
        }
        HIP_CHECK(hipGetLastError());
        index_count_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(info.slots / 2), 8192), hu::EB, 0, st>>>(ix->table, info.slots, store.small.d + 2);
        HIP_CHECK(hipGetLastError());
    }
    if (weights || colors) {  // (also for an index without windows: its zeroed table is still probed)
        if (weights) ix->weight.alloc(info.slots);
        if (colors) {
            ix->color.alloc(info.slots);
            ix->n_colors = colors->n_colors;
        }
        if (info.occurrences) {
            std::vector<unsigned long long> win_off(n + 1, 0);
            for (uint64_t r = 0; r < n; r++) win_off[r + 1] = win_off[r] + (off[r + 1] - off[r] >= k ? off[r + 1] - off[r] - k + 1 : 0);
            hu::DeviceArray<unsigned long long> d_win_off(n + 1), d_colors;
            hu::DeviceArray<uint32_t> d_weights;
            hu::upload_sliced(d_win_off, win_off.data(), (n + 1) * 8, st, device_id);
            if (weights) {
                d_weights.alloc(weights->n);
                hu::upload_sliced(d_weights, weights->w, weights->n * 4, st, device_id);
                weight_gather_kernel<<<hu::grid_for(info.slots), hu::EB, 0, st>>>(ix->table, ix->where, store.off, n, d_win_off, d_weights, weights->n,
                                                                                 info.slots, ix->weight, store.small.err());
            }
            if (colors) {
                d_colors.alloc(colors->n);
                hu::upload_sliced(d_colors, colors->c, colors->n * 8, st, device_id);
                color_gather_kernel<<<hu::grid_for(info.slots), hu::EB, 0, st>>>(ix->table, ix->where, store.off, n, d_win_off, d_colors, colors->n,
                                                                                info.slots, ix->color, store.small.err());
            }
            HIP_CHECK(hipGetLastError());
            // (the three uploads go back here, which synchronises: the gathers are done)
        } else {
            if (weights) HIP_CHECK(hipMemsetAsync(ix->weight, 0, info.slots * 4, st));
            if (colors) HIP_CHECK(hipMemsetAsync(ix->color, 0, info.slots * 8, st));
        }
    }
    ev.mark(1, st);
    store.small.read(st, "k-mer index");
    info.distinct = store.small.h[2];
    if (times) {
        times->build_upload_ms = store.upload_ms;
        times->build_pack_ms = store.pack_ms;
        times->build_insert_ms = ev.ms(0, 1);  // (with the table's fill and the count; weighted: the weights' upload and the gather)
    }
    info.device_bytes = info.slots * 8;
    if (locating || (wide && info.occurrences)) {
        ix->packed = store.take_packed();
        info.device_bytes += (store.n_words + 2) * 4;
    }
    if (locating) {
        ix->off = store.take_off();
        info.device_bytes += info.slots * 8 + (n + 1) * 8;
    } else {
        ix->where.release();  // weighted or coloured only: the positions have done their work
    }
    if (weights) info.device_bytes += info.slots * 4;
    if (colors) info.device_bytes += info.slots * 8;
    return ix;
}

bool device_kmer_index_is_locating(const KmerIndex *ix) { return ix->locating; }
bool device_kmer_index_is_weighted(const KmerIndex *ix) { return ix->weight.get() != nullptr; }
uint64_t device_kmer_index_n_colors(const KmerIndex *ix) { return ix->color ? ix->n_colors : 0; }

void device_kmer_index_info(const KmerIndex *ix, mtg_kmer_index_info *out) { *out = ix->info; }

void device_kmer_index_free(KmerIndex *ix) {
    if (!ix) return;
    int cur = 0;  // (an index may die on a thread whose current device is another one)
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(ix->device_id);
    delete ix;
    (void)hipSetDevice(cur);
}

void device_kmer_index_query(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, uint64_t *present_bits, uint64_t *valid_bits, KmerQueryTimes *times) {
    const uint64_t n_bases = probe_windows("mtg_kmer_index_query", ix->info.k, seq, off, n, kmers, valid, found, false);
    const uint64_t bit_words = (n_bases + 63) / 64;
    if (times) times->query_upload_ms = times->query_pack_ms = times->query_probe_ms = 0;
    if (n_bases == 0) return;  // nothing to look at
    Probe<> p(ix, seq, off, n, 2);
    hu::DeviceArray<unsigned long long> d_bits;  // valid_bits, then present_bits (those asked for)
    const int n_arrays = (valid_bits != nullptr) + (present_bits != nullptr);
    if (n_arrays) d_bits.alloc(n_arrays * bit_words);
    unsigned long long *d_valid_bits = valid_bits ? d_bits.get() : nullptr;
    unsigned long long *d_present_bits = present_bits ? d_bits + (valid_bits ? bit_words : 0) : nullptr;
    p.start();
    const unsigned grid = hu::grid_for(bit_words);  // (one thread per word: every word of the bit arrays is written)
    if (p.wide) query_kernel<true><<<grid, hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, d_valid_bits, d_present_bits);
    else query_kernel<false><<<grid, hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, d_valid_bits, d_present_bits);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(1, p.st);
    p.download_counts(valid, found);
    if (valid_bits) HIP_CHECK(hipMemcpyAsync(valid_bits, d_valid_bits, bit_words * 8, hipMemcpyDeviceToHost, p.st));
    if (present_bits) HIP_CHECK(hipMemcpyAsync(present_bits, d_present_bits, bit_words * 8, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipStreamSynchronize(p.st));
    if (times) p.booked(&times->query_upload_ms, &times->query_pack_ms, &times->query_probe_ms);  // (the build fields stay)
}

void device_kmer_index_abundance(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                                 uint64_t *found, uint64_t *sum, uint32_t *min, uint32_t *max, uint32_t *per_window, KmerAbundanceTimes *times) {
    if (!ix->weight) MTG_DIE("mtg_kmer_index_abundance: the index keeps no weights (build it with mtg_kmer_index_build_weighted)");
    const uint64_t n_bases = probe_windows("mtg_kmer_index_abundance", ix->info.k, seq, off, n, kmers, valid, found, n && (!sum || !min || !max));
    std::fill(sum, sum + n, 0ull);
    std::fill(min, min + n, 0u);
    std::fill(max, max + n, 0u);
    if (times) *times = KmerAbundanceTimes();
    if (n_bases == 0) return;  // nothing to look at
    Probe<> p(ix, seq, off, n, 3);  // valid, found, sum
    hu::DeviceArray<uint32_t> d_minmax(2 * n), d_per_window;
    if (per_window) d_per_window.alloc(n_bases);
    p.start();
    HIP_CHECK(hipMemsetAsync(d_minmax, 0xFF, n * 4, p.st));
    HIP_CHECK(hipMemsetAsync(d_minmax + n, 0, n * 4, p.st));
    // (one thread per run: every word of per_window is written)
    if (p.wide) abundance_kernel<true><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, ix->weight, d_minmax, d_per_window);
    else abundance_kernel<false><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, ix->weight, d_minmax, d_per_window);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(1, p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    const auto t0 = std::chrono::steady_clock::now();
    p.download_counts(valid, found);
    HIP_CHECK(hipMemcpyAsync(sum, p.d_counts + 2 * n, n * 8, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipMemcpyAsync(min, d_minmax, n * 4, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipMemcpyAsync(max, d_minmax + n, n * 4, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipStreamSynchronize(p.st));
    if (per_window) hu::download_sliced(per_window, d_per_window, n_bases * 4, p.st, p.device_id);
    for (uint64_t r = 0; r < n; r++)
        if (!found[r]) min[r] = 0;  // (nothing lowered the all-ones word)
    if (times) {
        p.booked(&times->upload_ms, &times->pack_ms, &times->probe_ms);
        times->download_ms = ms_since(t0);
    }
}

void device_kmer_index_colors(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                              uint64_t *found, uint32_t *per_color, uint64_t *per_window, KmerColorTimes *times) {
    if (!ix->color) MTG_DIE("mtg_kmer_index_colors: the index keeps no colours (build it with mtg_kmer_index_build_annotated)");
    const uint64_t C = ix->n_colors;
    const uint64_t n_bases = probe_windows("mtg_kmer_index_colors", ix->info.k, seq, off, n, kmers, valid, found, n && !per_color);
    for (uint64_t r = 0; r < n; r++)
        if (kmers[r] >> 32) MTG_DIE("mtg_kmer_index_colors: record %llu has %llu windows; the per-colour counters are 32-bit",
                                    (unsigned long long)r, (unsigned long long)kmers[r]);
    std::fill(per_color, per_color + n * C, 0u);
    if (times) times->upload_ms = times->pack_ms = times->probe_ms = times->download_ms = 0;
    if (n_bases == 0) return;  // nothing to look at
    Probe<> p(ix, seq, off, n, 2);
    hu::DeviceArray<uint32_t> d_per_color(n * C);
    hu::DeviceArray<unsigned long long> d_per_window;
    if (per_window) d_per_window.alloc(n_bases);
    p.start();
    HIP_CHECK(hipMemsetAsync(d_per_color, 0, n * C * 4, p.st));
    // (one thread per run: every word of per_window is written)
    if (p.wide) color_query_kernel<true><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, ix->color, (uint32_t)C, d_per_color, d_per_window);
    else color_query_kernel<false><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, ix->color, (uint32_t)C, d_per_color, d_per_window);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(1, p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    const auto t0 = std::chrono::steady_clock::now();
    p.download_counts(valid, found);
    HIP_CHECK(hipStreamSynchronize(p.st));
    hu::download_sliced(per_color, d_per_color, n * C * 4, p.st, p.device_id);
    if (per_window) hu::download_sliced(per_window, d_per_window, n_bases * 8, p.st, p.device_id);
    if (times) {
        p.booked(&times->upload_ms, &times->pack_ms, &times->probe_ms);
        times->download_ms = ms_since(t0);
    }
}

// ---- pseudoalignment ----
// color_query_kernel, unchanged, once per side into one pair of arrays that stay on the device; pa::reduce does the rest.
void device_kmer_index_pseudoalign(const KmerIndex *ix, const PseudoalignRule &rule, uint64_t base, const char *seq, const uint64_t *off, uint64_t n,
                                   const char *mate_seq, const uint64_t *mate_off, uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks,
                                   PseudoalignCall *out) {
    const char *fn = "mtg_pseudoaligner_align";
    if (!ix->color) MTG_DIE("%s: the index keeps no colours (build it with mtg_kmer_index_build_annotated)", fn);
    const uint64_t C = ix->n_colors, k = ix->info.k;
    const bool paired = mate_off != nullptr;
    uint64_t side_bases[2] = {probe_windows(fn, k, seq, off, n, kmers, valid, found, n && !masks), 0};
    if (paired) {
        std::vector<uint64_t> mk(n), mv(n), mf(n);
        side_bases[1] = probe_windows(fn, k, mate_seq, mate_off, n, mk.data(), mv.data(), mf.data(), false);
        for (uint64_t r = 0; r < n; r++) kmers[r] += mk[r];
    }
    for (uint64_t r = 0; r < n; r++)
        if (kmers[r] >> 32) MTG_DIE("%s: fragment %llu has %llu windows; the per-colour counters are 32-bit", fn, (unsigned long long)r,
                                    (unsigned long long)kmers[r]);
    std::fill(masks, masks + n, 0ull);
    *out = PseudoalignCall();
    if (side_bases[0] + side_bases[1] == 0) return;  // nothing to look at: no fragment is eligible
    on_device(ix->device_id);
    hipStream_t st = nullptr;
    hu::DeviceArray<unsigned long long> d_counts(2 * n);
    hu::DeviceArray<uint32_t> d_hits(n * C);
    HIP_CHECK(hipMemsetAsync(d_counts, 0, 2 * n * 8, st));
    HIP_CHECK(hipMemsetAsync(d_hits, 0, n * C * 4, st));
    for (int side = 0; side < 2; side++) {
        const uint64_t n_bases = side_bases[side];
        if (!n_bases) continue;
        MaskedSeqStore store(side ? mate_seq : seq, side ? mate_off : off, n, st, ix->device_id);
        IndexArgs a{};
        a.packed = store.packed; a.off = store.off; a.index_packed = ix->packed; a.table = ix->table; a.slots = ix->info.slots;
        kw::window_args_set_k(a, k);
        PhaseEvents<2> ev;
        ev.mark(0, st);
        const unsigned grid = hu::grid_for((n_bases + RUN - 1) / RUN);
        if (k >= 32) color_query_kernel<true><<<grid, hu::EB, 0, st>>>(a, store.bad, n_bases, n, d_counts, ix->color, (uint32_t)C, d_hits, nullptr);
        else color_query_kernel<false><<<grid, hu::EB, 0, st>>>(a, store.bad, n_bases, n, d_counts, ix->color, (uint32_t)C, d_hits, nullptr);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        out->upload_ms += store.upload_ms;
        out->pack_ms += store.pack_ms;
        out->probe_ms += ev.ms(0, 1);  // (waits: the side's store may go)
    }
    pa::reduce(fn, d_hits, d_counts, n, (uint32_t)C, rule, base, st, ix->device_id, masks, out);
    const auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipMemcpyAsync(valid, d_counts, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(found, d_counts + n, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    out->download_ms += ms_since(t0);
}

// ---- correction ----
// query_kernel, unchanged, once on the input and once after every round that substituted; kc::rounds does the rest.
void device_kmer_index_correct(const KmerIndex *ix, uint32_t min_solid, uint32_t rounds, const char *seq, const uint64_t *off, uint64_t n,
                               uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *found_after, uint64_t *candidates, uint64_t *ambiguous,
                               uint64_t *corrected, KmerCorrectCall *out) {
    const auto t_call = std::chrono::steady_clock::now();
    const char *fn = "mtg_kmer_index_correct";
    const uint64_t n_bases = probe_windows(fn, ix->info.k, seq, off, n, kmers, valid, found, n && (!found_after || !candidates || !ambiguous || !corrected));
    for (uint64_t *column : {found_after, candidates, ambiguous, corrected}) std::fill(column, column + n, 0ull);
    *out = KmerCorrectCall();
    if (n_bases == 0) return;  // nothing to look at
    const uint64_t bit_words = (n_bases + 63) / 64;
    Probe<> p(ix, seq, off, n, 2);
    hipStream_t st = p.st;
    hu::DeviceArray<unsigned long long> d_bits(2 * bit_words), d_rec(2 * n);  // valid then present; candidates, ambiguous
    HIP_CHECK(hipMemsetAsync(d_rec, 0, 2 * n * 8, st));
    auto query_pass = [&]() {
        p.start();
        const unsigned grid = hu::grid_for(bit_words);  // (one thread per word: every word of the bit arrays is written)
        if (p.wide) query_kernel<true><<<grid, hu::EB, 0, st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, d_bits, d_bits + bit_words);
        else query_kernel<false><<<grid, hu::EB, 0, st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, d_bits, d_bits + bit_words);
        HIP_CHECK(hipGetLastError());
        p.ev.mark(1, st);
        out->query_ms += p.ev.ms(0, 1);  // (waits: the pass is done)
    };
    query_pass();
    p.download_counts(valid, found);
    HIP_CHECK(hipStreamSynchronize(st));  // (the next pass zeroes the counters)
    kc::Args a{};
    a.packed = p.store.packed; a.off = p.store.off; a.vbits = d_bits; a.pbits = d_bits + bit_words; a.index_packed = ix->packed;
    a.table = ix->table; a.slots = ix->info.slots; a.n_bases = n_bases; a.n_rec = n; a.k = ix->info.k;
    a.kmask = p.a.kmask; a.pow_k1 = p.a.pow_k1; a.inv_base = p.a.inv_base;
    kc::rounds(a, p.store.packed.get(), p.wide, min_solid, rounds, st, p.device_id, d_rec.get(), query_pass, out);
    const auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipMemcpyAsync(found_after, p.d_counts + n, n * 8, hipMemcpyDeviceToHost, st));  // (of the last pass: the final text)
    HIP_CHECK(hipMemcpyAsync(candidates, d_rec, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(ambiguous, d_rec + n, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    // the positions whose base is no longer the input's (a later round may have put a base back), and how many each record has
    size_t kept = 0;
    for (size_t i = 0, r = 0; i < out->positions.size(); i++) {
        const uint64_t pos = out->positions[i];
        if ((uint8_t)(seq[pos] & ~0x20) == out->bases[i]) continue;
        while (off[r + 1] <= pos) r++;
        corrected[r]++;
        out->positions[kept] = pos;
        out->bases[kept++] = out->bases[i];
    }
    out->positions.resize(kept);
    out->bases.resize(kept);
    out->download_ms += ms_since(t0);
    out->upload_ms = p.store.upload_ms;
    out->pack_ms = p.store.pack_ms;
    out->total_ms = ms_since(t_call);
}

// ---- tally ----
struct KmerTally {
    const KmerIndex *ix;  // (the caller keeps it alive for add and coverage; reset and free do without it)
    int device_id;
    uint64_t slots;
    hu::DeviceArray<unsigned long long> count;  // [slots] the windows added on the slot's class
};

KmerTally *device_kmer_tally_create(const KmerIndex *ix) {
    on_device(ix->device_id);
    KmerTally *t = new KmerTally{ix, ix->device_id, ix->info.slots, {}};
    t->count.alloc(t->slots);
    device_kmer_tally_reset(t);
    return t;
}

uint64_t device_kmer_tally_device_bytes(const KmerTally *t) { return t->slots * 8; }

void device_kmer_tally_reset(KmerTally *t) {
    on_device(t->device_id);
    HIP_CHECK(hipMemsetAsync(t->count, 0, t->slots * 8, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
}

void device_kmer_tally_free(KmerTally *t) {
    if (!t) return;
    int cur = 0;  // (as an index: it may die on a thread whose current device is another one)
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(t->device_id);
    delete t;
    (void)hipSetDevice(cur);
}

void device_kmer_tally_add(KmerTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                           KmerTallyTimes *times) {
    const KmerIndex *ix = t->ix;
    const uint64_t n_bases = probe_windows("mtg_kmer_tally_add", ix->info.k, seq, off, n, kmers, valid, found, false);
    if (times) *times = KmerTallyTimes();
    if (n_bases == 0) return;  // nothing to look at
    Probe<> p(ix, seq, off, n, 2);
    p.start();
    if (p.wide) tally_kernel<true><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, t->count);
    else tally_kernel<false><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, t->count);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(1, p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    const auto t0 = std::chrono::steady_clock::now();
    p.download_counts(valid, found);
    HIP_CHECK(hipStreamSynchronize(p.st));
    if (times) {
        p.booked(&times->upload_ms, &times->pack_ms, &times->probe_ms);
        times->download_ms = ms_since(t0);
    }
}

void device_kmer_tally_coverage(const KmerTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                                uint64_t *found, uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window, KmerTallyTimes *times) {
    const KmerIndex *ix = t->ix;
    const uint64_t n_bases = probe_windows("mtg_kmer_tally_coverage", ix->info.k, seq, off, n, kmers, valid, found, n && (!covered || !sum || !max));
    std::fill(covered, covered + n, 0ull);
    std::fill(sum, sum + n, 0ull);
    std::fill(max, max + n, 0ull);
    if (times) *times = KmerTallyTimes();
    if (n_bases == 0) return;  // nothing to look at
    Probe<> p(ix, seq, off, n, 5);  // valid, found, covered, sum, max
    hu::DeviceArray<unsigned long long> d_per_window;
    if (per_window) d_per_window.alloc(n_bases);
    p.start();
    // (one thread per run: every word of per_window is written)
    if (p.wide) coverage_kernel<true><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, t->count, d_per_window);
    else coverage_kernel<false><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, n, p.d_counts, t->count, d_per_window);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(1, p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    const auto t0 = std::chrono::steady_clock::now();
    p.download_counts(valid, found);
    HIP_CHECK(hipStreamSynchronize(p.st));
    hu::download_sliced(covered, p.d_counts + 2 * n, n * 8, p.st, p.device_id);
    hu::download_sliced(sum, p.d_counts + 3 * n, n * 8, p.st, p.device_id);
    hu::download_sliced(max, p.d_counts + 4 * n, n * 8, p.st, p.device_id);
    if (per_window) hu::download_sliced(per_window, d_per_window, n_bases * 8, p.st, p.device_id);
    if (times) {
        p.booked(&times->upload_ms, &times->pack_ms, &times->probe_ms);
        times->download_ms = ms_since(t0);
    }
}

namespace {
// the probe of locate and thread, between the marks 0 and 1 of p.ev: d_hit[n_bases] = NO_HIT, then the hits of the found windows
template <int EVENTS>
void queue_locate_probe(Probe<EVENTS> &p, const KmerIndex *ix, unsigned long long *d_hit) {
    const uint64_t n_bases = p.store.n_bases;
    p.start();
    HIP_CHECK(hipMemsetAsync(d_hit, 0xFF, n_bases * 8, p.st));
    if (p.wide) locate_kernel<true><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, p.n, p.d_counts, ix->where, d_hit);
    else locate_kernel<false><<<p.run_grid(), hu::EB, 0, p.st>>>(p.a, p.store.bad, n_bases, p.n, p.d_counts, ix->where, d_hit);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(1, p.st);
}
}  // namespace

void device_kmer_index_locate(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                              uint64_t *found, KmerRuns *runs, KmerLocateTimes *times) {
    if (!ix->locating) MTG_DIE("mtg_kmer_index_locate: the index keeps no positions (build it with mtg_kmer_index_build_locating)");
    const uint64_t k = ix->info.k;
    const uint64_t n_bases = probe_windows("mtg_kmer_index_locate", k, seq, off, n, kmers, valid, found, !runs);
    *runs = KmerRuns();
    if (times) *times = KmerLocateTimes();
    if (n_bases == 0) return;  // nothing to look at
    Probe<3> p(ix, seq, off, n, 2);
    hipStream_t st = p.st;
    hu::DeviceArray<unsigned long long> d_hit(n_bases);
    queue_locate_probe(p, ix, d_hit);
    const kr::RunArgs ra{d_hit, p.store.off, ix->off, n_bases, n, ix->info.records, k};
    kr::runs_from_hits(ra, st, p.device_id, runs, [&](hipStream_t) {
        p.ev.mark(2, st);
        p.download_counts(valid, found);
    });
    if (times) {
        p.booked(&times->upload_ms, &times->pack_ms, &times->probe_ms);
        times->runs_ms = p.ev.ms(1, 2);
    }
}

// ---- thread: locate's probe and run stage, then the walks from the runs where they are (kmer_walks_device.hpp) ----
void device_kmer_index_thread(const KmerIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers, uint64_t *kmers,
                              uint64_t *valid, uint64_t *found, KmerWalks *walks, KmerThreadTimes *times) {
    if (!ix->locating) MTG_DIE("mtg_kmer_index_thread: the index keeps no positions (build it with mtg_kmer_index_build_locating)");
    const uint64_t k = ix->info.k;
    const uint64_t n_bases = probe_windows("mtg_kmer_index_thread", k, seq, off, n, kmers, valid, found, !walks);
    *walks = KmerWalks();
    if (times) *times = KmerThreadTimes();
    if (n_bases == 0) return;  // nothing to look at
    Probe<4> p(ix, seq, off, n, 2);
    hipStream_t st = p.st;
    hu::DeviceArray<unsigned long long> d_hit(n_bases);
    queue_locate_probe(p, ix, d_hit);
    const kr::RunArgs ra{d_hit, p.store.off, ix->off, n_bases, n, ix->info.records, k};
    kr::RunStage stage(n_bases);
    stage.queue(ra, st);
    p.ev.mark(2, st);
    kwk::walks_from_runs(stage, ix->off, k, min_kmers, st, p.device_id, walks, [&](hipStream_t) {
        p.ev.mark(3, st);
        p.download_counts(valid, found);
    });
    if (times) {
        p.booked(&times->upload_ms, &times->pack_ms, &times->probe_ms);
        times->runs_ms = p.ev.ms(1, 2);
        times->walks_ms = p.ev.ms(2, 3);
    }
}

}  // namespace mtg
