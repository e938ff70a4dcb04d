// tig_tally_device.hpp -- tallies hung off text positions: the read counters of the sparse minimizer index
//
// The table's tally (kmer_query_device.hip) keeps a 64-bit counter per table slot. The sparse index has no slot per
// k-mer, but its locate probe gives, per found window, the smallest window start t of its class in the indexed text, and
// tp::gather_run (tig_payload_device.hpp) turns t into the window's ORDINAL win_off[r] + (t - off[r]). t is a function of the class
// alone -- the minimum over all its occurrences on both strands -- so counter[ordinal(t)] is the table's per-class counter with no
// slot anywhere: one counter per window of the text, 8 B each, and a window that is not the first occurrence of its class stays 0.
//
// Two passes, as the payloads: tig_locate_kernel, unchanged, has filled hit[q] = (t << 1) | strand; then
//   add       tig_tally_add_kernel: a thread owns kw::RUN consecutive query positions and keeps (ordinal, run length): a hit on the
//             ordinal of the hit before only lengthens the run -- absent and invalid windows and a change of query record in between
//             do not break it, only sums leave --, and a change of ordinal, or the end of the positions, flushes it: one
//             atomicAdd(&counter[ord], run) whose result nobody reads (tally_kernel's rule). A homopolymer costs one atomic per thread.
//   coverage  tig_coverage_gather_kernel: abundance_gather_kernel reading counter[ord]; per (thread, query record) covered / sum / max
//             in registers, out by one atomicAdd each and one atomicMax when the record changes, none where nothing of the record was
//             covered (coverage_kernel's rule). per_window has one writer per position, zeros included.
// Sums and maxima of integers: the results do not depend on the launch geometry or the order the atomics land in.
//
// The kernels are static: every translation unit that includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_util.hpp"
#include "kmer_window_device.hpp"
#include "tig_payload_device.hpp"

namespace mtg {
namespace tt {

// counter: [windows]; per found window counter[its ordinal] += 1
static __global__ __launch_bounds__(hu::EB) void tig_tally_add_kernel(tp::GatherArgs g, uint64_t windows, unsigned long long *counter) {
    uint64_t cur = 0;  // the ordinal of the run (< windows: gather_run hands out no other)
    uint32_t run = 0;  // found windows on `cur` since the last flush (at most RUN)
    tp::gather_run(g, windows, (unsigned long long *)nullptr, [&](uint64_t, uint64_t, uint64_t ord) {
        if (ord != cur) {
            if (run) atomicAdd(&counter[cur], (unsigned long long)run);
            cur = ord;
            run = 0;
        }
        run++;
    });
    if (run) atomicAdd(&counter[cur], (unsigned long long)run);
}

// out: [3 q_rec] per query record the found windows whose counter is > 0, the sum of the counters and the largest (all 0 before);
// per_window: [n_bases] or null
static __global__ __launch_bounds__(hu::EB) void tig_coverage_gather_kernel(tp::GatherArgs g, uint64_t windows, const unsigned long long *counter,
                                                                            unsigned long long *out, unsigned long long *per_window) {
    uint64_t rec = 0, sum = 0, hi = 0;
    uint32_t covered = 0;  // (of the record `rec`; at most RUN)
    auto flush = [&]() {
        if (!covered) return;  // (then the sum and the largest are 0 too)
        atomicAdd(&out[rec], (unsigned long long)covered);
        atomicAdd(&out[g.q_rec + rec], (unsigned long long)sum);
        atomicMax(&out[2 * g.q_rec + rec], (unsigned long long)hi);
        sum = 0; hi = 0; covered = 0;
    };
    tp::gather_run(g, windows, per_window, [&](uint64_t p, uint64_t r, uint64_t ord) {
        if (r != rec) {
            flush();
            rec = r;
        }
        const uint64_t t = counter[ord];
        covered += t != 0;
        sum += t;
        hi = t > hi ? t : hi;
        if (per_window) per_window[p] = t;
    });
    flush();
}

}  // namespace tt
}  // namespace mtg
