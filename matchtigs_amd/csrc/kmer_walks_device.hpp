// kmer_walks_device.hpp -- from the runs of a query to its walks through the indexed records
//
// What both locating indexes share behind kmer_runs_device.hpp. Over unitigs every k-mer occurs once, so every found window has one
// place, and two neighbouring found windows of a query are neighbours in the de Bruijn graph: the runs of a record, in order, are
// the segments of a path, and joining them needs no look at the graph -- only at where a run ends in its record. With W(u) = the
// windows of index record u, a run (q, n, strand s, u, t)
//   enters at the head   s = + : t == 0         s = - : t + n == W(u)
//   leaves at the tail   s = + : t + n == W(u)  s = - : t == 0
// and run r + 1 continues run r iff both lie in one query record, q[r + 1] == q[r] + n[r], r leaves at the tail and r + 1 enters at the
// head. A walk is a maximal chain of continuing runs. walks_from_runs works on the runs where kr::RunStage left them:
//   flag     walk_flag_kernel marks the runs that do not continue their predecessor and notes W(u) of every run, in two 32-bit halves
//   scan     hu::scan_u32 ranks the runs into walks; two more over the halves of W(u) give its prefix sums -- a walk's path length is
//            a difference of two of them, whatever its number of steps (a haplotype is one walk of millions)
//   mark     walk_mark_kernel notes the first run of every walk
//   emit     walk_emit_kernel writes the nine fields of every walk and whether min_kmers keeps it
//   compact  two scans (kept walks, their steps), walk_compact_kernel moves the kept walks together and walk_steps_kernel writes
//            their steps, (t_record << 1) | strand per run
// and a sliced download of the kept walks and their steps alone. A call takes 12 + 8 + 16 = 36 B per run beside the runs, 72 + 8 + 8 + 16
// = 104 B per walk, and 72 B per kept walk and 8 B per step of what goes back. The kernels are static: every translation unit that
// includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_runs_device.hpp"

namespace mtg {
namespace kwk {

constexpr int FIELDS = 9;  // q_record, q_start, q_end, kmers, steps, first_step, path_len, path_start, path_end
enum { Q_RECORD, Q_START, Q_END, KMERS, STEPS, FIRST_STEP, PATH_LEN, PATH_START, PATH_END };

// what the walk kernels read: the runs as run_emit_kernel wrote them, the record offsets of the index
struct WalkArgs {
    const unsigned long long *run;  // five arrays of n_runs words: q_record, q_start, kmers, t_record, t_start
    const unsigned char *strand;    // [n_runs]
    const unsigned long long *t_off;
    uint64_t n_runs, k;
};
__device__ __forceinline__ uint64_t windows_of(const WalkArgs &a, uint64_t u) { return a.t_off[u + 1] - a.t_off[u] - a.k + 1; }
// starts[r] = 1 iff a walk starts at run r; w_lo / w_hi: the halves of W(t_record[r])
static __global__ __launch_bounds__(hu::EB) void walk_flag_kernel(WalkArgs a, uint32_t *starts, uint32_t *w_lo, uint32_t *w_hi) {
    const uint64_t r = hu::gid();
    if (r >= a.n_runs) return;
    const uint64_t R = a.n_runs;
    const uint64_t n = a.run[2 * R + r], t = a.run[4 * R + r], W = windows_of(a, a.run[3 * R + r]);
    w_lo[r] = (uint32_t)W;
    w_hi[r] = (uint32_t)(W >> 32);
    bool cont = false;
    if (r > 0 && a.run[r - 1] == a.run[r]) {
        const uint64_t np = a.run[2 * R + r - 1], tp = a.run[4 * R + r - 1];
        const bool tail = a.strand[r - 1] ? tp == 0 : tp + np == windows_of(a, a.run[3 * R + r - 1]);
        const bool head = a.strand[r] ? t + n == W : t == 0;
        cont = tail && head && a.run[R + r] == a.run[R + r - 1] + np;
    }
    starts[r] = !cont;
}
// first[w] = the first run of walk w; first[n_walks] = n_runs
static __global__ __launch_bounds__(hu::EB) void walk_mark_kernel(uint64_t n_runs, uint64_t n_walks, const uint32_t *starts,
                                                                  const unsigned long long *rank, unsigned long long *first) {
    const uint64_t r = hu::gid();
    if (r >= n_runs) return;
    if (r == 0) first[n_walks] = n_runs;
    if (starts[r] && rank[r] < n_walks) first[rank[r]] = r;
}
// The fields of walk w, runs [first[w], first[w + 1]), into out: FIELDS arrays of n_walks words (first_step is set by the compaction).
// p_lo / p_hi: the exclusive prefix sums of w_lo / w_hi, tot_lo / tot_hi their totals. keep[w] = the walk has min_kmers windows,
// keep_steps[w] = its steps if so.
static __global__ __launch_bounds__(hu::EB) void walk_emit_kernel(WalkArgs a, uint64_t n_walks, uint64_t min_kmers, const unsigned long long *first,
                                                                  const unsigned long long *p_lo, const unsigned long long *p_hi,
                                                                  const unsigned long long *tot_lo, const unsigned long long *tot_hi,
                                                                  unsigned long long *out, uint32_t *keep, uint32_t *keep_steps) {
    const uint64_t w = hu::gid();
    if (w >= n_walks) return;
    const uint64_t R = a.n_runs, b = first[w], e = first[w + 1];
    const uint64_t q_start = a.run[R + b], K = a.run[R + e - 1] + a.run[2 * R + e - 1] - q_start, span = K + a.k - 1;
    const uint64_t sum_b = p_lo[b] + (p_hi[b] << 32), sum_e = e < R ? p_lo[e] + (p_hi[e] << 32) : *tot_lo + (*tot_hi << 32);
    const uint64_t n = a.run[2 * R + b], t = a.run[4 * R + b];
    const uint64_t path_start = a.strand[b] ? windows_of(a, a.run[3 * R + b]) - (t + n) : t;
    out[Q_RECORD * n_walks + w] = a.run[b];
    out[Q_START * n_walks + w] = q_start;
    out[Q_END * n_walks + w] = q_start + span;
    out[KMERS * n_walks + w] = K;
    out[STEPS * n_walks + w] = e - b;
    out[FIRST_STEP * n_walks + w] = 0;
    out[PATH_LEN * n_walks + w] = sum_e - sum_b + a.k - 1;
    out[PATH_START * n_walks + w] = path_start;
    out[PATH_END * n_walks + w] = path_start + span;
    const bool kept = K >= min_kmers;
    keep[w] = kept;
    keep_steps[w] = kept ? (uint32_t)(e - b) : 0;
}
// kept walk w goes to slot[w] of `to` (FIELDS arrays of n_kept words), its first_step = step0[w]
static __global__ __launch_bounds__(hu::EB) void walk_compact_kernel(uint64_t n_walks, uint64_t n_kept, const uint32_t *keep, const unsigned long long *slot,
                                                                     const unsigned long long *step0, const unsigned long long *from,
                                                                     unsigned long long *to) {
    const uint64_t w = hu::gid();
    if (w >= n_walks || !keep[w]) return;
    const uint64_t i = slot[w];
    if (i >= n_kept) return;
    for (int f = 0; f < FIELDS; f++) to[f * n_kept + i] = f == FIRST_STEP ? step0[w] : from[f * n_walks + w];
}
// run r is step r - first[w] of its walk w = rank[r] + starts[r] - 1: steps[step0[w] + that] = (t_record << 1) | strand if w is kept
static __global__ __launch_bounds__(hu::EB) void walk_steps_kernel(WalkArgs a, uint64_t n_walks, uint64_t n_steps, const uint32_t *starts,
                                                                   const unsigned long long *rank, const unsigned long long *first, const uint32_t *keep,
                                                                   const unsigned long long *step0, unsigned long long *steps) {
    const uint64_t r = hu::gid();
    if (r >= a.n_runs) return;
    const uint64_t w = rank[r] + starts[r] - 1;  // (run 0 starts a walk, so this is never below 0)
    if (w >= n_walks || !keep[w]) return;
    const uint64_t i = step0[w] + (r - first[w]);
    if (i < n_steps) steps[i] = (a.run[3 * a.n_runs + r] << 1) | a.strand[r];
}

// The walks of the runs that `stage` holds (queued on st) with at least min_kmers windows into *walks, in ascending query position.
// t_off: the index's record offsets. done(st) is called once the kernels are queued, before the stream is waited for the last time.
template <typename Done>
inline void walks_from_runs(const kr::RunStage &stage, const unsigned long long *t_off, uint64_t k, uint64_t min_kmers, hipStream_t st, int device_id,
                            KmerWalks *walks, Done done) {
    const uint64_t R = stage.n_runs;
    if (R > 0xFFFFFFFFull) MTG_DIE("thread: %llu runs; the limit is 2^32 - 1", (unsigned long long)R);
    if (!R) {
        done(st);
        HIP_CHECK(hipStreamSynchronize(st));
        return;
    }
    const WalkArgs a{stage.out(), stage.strand(), t_off, R, k};
    hu::DeviceArray<uint32_t> d_flags(3 * R);  // starts, w_lo, w_hi
    hu::DeviceArray<unsigned long long> d_rank(R), d_prefix(2 * R);
    hu::ScanScratch<unsigned long long> scan(R), scan_lo(R), scan_hi(R);
    uint32_t *d_starts = d_flags, *d_w_lo = d_flags + R, *d_w_hi = d_flags + 2 * R;
    const unsigned run_grid = hu::grid_for(R);
    walk_flag_kernel<<<run_grid, hu::EB, 0, st>>>(a, d_starts, d_w_lo, d_w_hi);
    HIP_CHECK(hipGetLastError());
    scan.scan(st, d_starts, R, d_rank);
    scan_lo.scan(st, d_w_lo, R, d_prefix);
    scan_hi.scan(st, d_w_hi, R, d_prefix + R);
    uint64_t n_walks = 0;
    HIP_CHECK(hipMemcpyAsync(&n_walks, scan.total(), 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_walks < 1 || n_walks > R) MTG_DIE("thread: internal error (%llu walks of %llu runs)", (unsigned long long)n_walks, (unsigned long long)R);

    hu::DeviceArray<unsigned long long> d_first(n_walks + 1), d_all(FIELDS * n_walks), d_slot(2 * n_walks);  // d_slot: kept rank, first step
    hu::DeviceArray<uint32_t> d_keep(2 * n_walks);                                                          // keep, keep_steps
    hu::ScanScratch<unsigned long long> scan_keep(n_walks), scan_steps(n_walks);
    const unsigned walk_grid = hu::grid_for(n_walks);
    walk_mark_kernel<<<run_grid, hu::EB, 0, st>>>(R, n_walks, d_starts, d_rank, d_first);
    walk_emit_kernel<<<walk_grid, hu::EB, 0, st>>>(a, n_walks, min_kmers, d_first, d_prefix, d_prefix + R, scan_lo.total(), scan_hi.total(), d_all, d_keep,
                                                   d_keep + n_walks);
    HIP_CHECK(hipGetLastError());
    scan_keep.scan(st, d_keep, n_walks, d_slot);
    scan_steps.scan(st, d_keep + n_walks, n_walks, d_slot + n_walks);
    uint64_t n_kept = 0, n_steps = 0;
    HIP_CHECK(hipMemcpyAsync(&n_kept, scan_keep.total(), 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&n_steps, scan_steps.total(), 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_kept > n_walks || n_steps > R) MTG_DIE("thread: internal error (%llu walks kept of %llu)", (unsigned long long)n_kept, (unsigned long long)n_walks);

    hu::DeviceArray<unsigned long long> d_kept, d_steps;
    if (n_kept) {
        d_kept.alloc(FIELDS * n_kept);
        d_steps.alloc(n_steps);
        walk_compact_kernel<<<walk_grid, hu::EB, 0, st>>>(n_walks, n_kept, d_keep, d_slot, d_slot + n_walks, d_all, d_kept);
        walk_steps_kernel<<<run_grid, hu::EB, 0, st>>>(a, n_walks, n_steps, d_starts, d_rank, d_first, d_keep, d_slot + n_walks, d_steps);
        HIP_CHECK(hipGetLastError());
    }
    done(st);
    HIP_CHECK(hipStreamSynchronize(st));
    if (n_kept) {
        walks->fields.resize(FIELDS * n_kept);
        hu::download_sliced(walks->fields.data(), d_kept, FIELDS * n_kept * 8, st, device_id);
        walks->steps.resize(n_steps);
        hu::download_sliced(walks->steps.data(), d_steps, n_steps * 8, st, device_id);
    }
    walks->n = n_kept;
}

}  // namespace kwk
}  // namespace mtg
