// kmer_runs_device.hpp -- from the hits of a query's window starts to its maximal collinear runs
//
// What both locating indexes share: the table's (kmer_query_device.hip) and the sparse minimizer index's (tig_index_device.hip). Each
// has a probe kernel of its own that fills hit[n_bases], NO_HIT before: per found window at q, hit[q] = (t << 1) | strand, t = the
// smallest window start of its class in the index, strand 0 iff the query's bases equal the index's at t one by one (same_forward) --
// otherwise, the classes being equal, they are the reverse complement. runs_from_hits then is
//   flag   run_flag_kernel marks the windows that do not continue their predecessor
//   scan   hu::scan_u32 ranks them
//   mark   run_mark_kernel notes the first and last position of every run
//   emit   run_emit_kernel writes the fields of each
// (RunStage, whose arrays the walk stage of kmer_walks_device.hpp reads where they are) and a sliced download of the runs alone. A call takes 4 + 8 B per query base beside the hits. The kernels are static: every
// translation unit that includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_window_device.hpp"

namespace mtg {
namespace kr {

constexpr unsigned long long NO_HIT = ~0ull;

// the k bases at p of the store px equal those at q of the store py, 16 bases per compare (the first half of kw::same_class)
__device__ inline bool same_forward(const uint32_t *px, uint64_t p, const uint32_t *py, uint64_t q, uint64_t k) {
    for (uint64_t i = 0; i < k; i += 16) {
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        if ((kw::bases16(px, p + i) ^ kw::bases16(py, q + i)) & m) return false;
    }
    return true;
}

// what the run kernels read: the hits of the query's positions, the record offsets of the query and of the index
struct RunArgs {
    const unsigned long long *hit;    // [n_bases]
    const unsigned long long *q_off;  // [q_rec + 1]
    const unsigned long long *t_off;  // [t_rec + 1]
    uint64_t n_bases, q_rec, t_rec, k;
};
// the last record that starts at or before x (n_rec >= 1)
__device__ __forceinline__ uint64_t record_of(const unsigned long long *off, uint64_t n_rec, uint64_t x) {
    uint64_t lo = 0, hi = n_rec;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The found window at p (h = hit[p]) continues the window at p - 1: found too, same strand, the next location in the strand's
// direction, and both pairs inside one record. For k >= 2 two neighbouring window starts always share their record (the last k - 1
// bases of a record start no window), so only k = 1 has to look the records up.
__device__ __forceinline__ bool continues(const RunArgs &a, uint64_t p, unsigned long long h) {
    if (p == 0) return false;
    const unsigned long long g = a.hit[p - 1];
    if (g == NO_HIT || ((g ^ h) & 1)) return false;
    const uint64_t t = h >> 1, tp = g >> 1;
    if ((h & 1) ? t + 1 != tp : tp + 1 != t) return false;
    if (a.k > 1) return true;
    const uint64_t tl = t < tp ? t : tp;
    return p < a.q_off[record_of(a.q_off, a.q_rec, p - 1) + 1] && tl + 1 < a.t_off[record_of(a.t_off, a.t_rec, tl) + 1];
}
// starts[p] = 1 iff a run starts at p
static __global__ __launch_bounds__(hu::EB) void run_flag_kernel(RunArgs a, uint32_t *starts) {
    const uint64_t p = hu::gid();
    if (p >= a.n_bases) return;
    const unsigned long long h = a.hit[p];
    starts[p] = h != NO_HIT && !continues(a, p, h);
}
// rank[p] = the runs that start before p. Run i starts at first[i] and ends at last[i] (starts and ends alternate, so the end at p
// belongs to the run rank[p] + starts[p] - 1).
static __global__ __launch_bounds__(hu::EB) void run_mark_kernel(RunArgs a, const uint32_t *starts, const unsigned long long *rank, uint64_t n_runs,
                                                                 unsigned long long *first, unsigned long long *last) {
    const uint64_t p = hu::gid();
    if (p >= a.n_bases) return;
    const unsigned long long h = a.hit[p];
    if (h == NO_HIT) return;
    const uint32_t s = starts[p];
    const uint64_t i = rank[p];
    if (s && i < n_runs) first[i] = p;
    bool end = p + 1 == a.n_bases;
    if (!end) {
        const unsigned long long hn = a.hit[p + 1];
        end = hn == NO_HIT || !continues(a, p + 1, hn);
    }
    if (end && i + s >= 1 && i + s - 1 < n_runs) last[i + s - 1] = p;
}
// the fields of run i; out: five arrays of n_runs words each -- q_record, q_start, kmers, t_record, t_start --, strand: [n_runs]
static __global__ __launch_bounds__(hu::EB) void run_emit_kernel(RunArgs a, uint64_t n_runs, const unsigned long long *first,
                                                                 const unsigned long long *last, unsigned long long *out, unsigned char *strand) {
    const uint64_t i = hu::gid();
    if (i >= n_runs) return;
    const uint64_t qs = first[i], qe = last[i];
    const unsigned long long hs = a.hit[qs], he = a.hit[qe];
    const uint64_t t = (hs & 1) ? he >> 1 : hs >> 1;  // the leftmost index base: on the reverse strand the last window's
    const uint64_t qr = record_of(a.q_off, a.q_rec, qs), tr = record_of(a.t_off, a.t_rec, t);
    out[i] = qr;
    out[n_runs + i] = qs - a.q_off[qr];
    out[2 * n_runs + i] = qe - qs + 1;
    out[3 * n_runs + i] = tr;
    out[4 * n_runs + i] = t - a.t_off[tr];
    strand[i] = (unsigned char)(hs & 1);
}

// The run stage's device arrays, which own themselves. queue() leaves the runs of ra.hit (filled on st) on the device -- out(): five
// arrays of n_runs words, strand(): [n_runs] -- for whoever works on from them there (kmer_walks_device.hpp); download() brings them to
// the host once the stream has been waited for.
struct RunStage {
    uint64_t n_runs = 0;
    hu::DeviceArray<uint32_t> d_starts;
    hu::DeviceArray<unsigned long long> d_rank;
    hu::ScanScratch<unsigned long long> scan;
    hu::DeviceArray<unsigned long long> d_ends;  // first then last position of every run
    hu::DeviceArray<unsigned char> d_out_bytes;  // five 64-bit fields per run, then the strands

    explicit RunStage(uint64_t n_bases) : d_starts(n_bases), d_rank(n_bases), scan(n_bases) {}
    unsigned long long *out() const { return reinterpret_cast<unsigned long long *>(d_out_bytes.get()); }
    unsigned char *strand() const { return d_out_bytes.get() + 5 * n_runs * 8; }
    void queue(const RunArgs &ra, hipStream_t st) {
        const uint64_t n_bases = ra.n_bases;
        const unsigned base_grid = hu::grid_for(n_bases);
        run_flag_kernel<<<base_grid, hu::EB, 0, st>>>(ra, d_starts);
        HIP_CHECK(hipGetLastError());
        scan.scan(st, d_starts, n_bases, d_rank);
        HIP_CHECK(hipMemcpyAsync(&n_runs, scan.total(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (n_runs) {
            d_ends.alloc(2 * n_runs);
            d_out_bytes.alloc(5 * n_runs * 8 + n_runs);
            run_mark_kernel<<<base_grid, hu::EB, 0, st>>>(ra, d_starts, d_rank, n_runs, d_ends, d_ends + n_runs);
            run_emit_kernel<<<hu::grid_for(n_runs), hu::EB, 0, st>>>(ra, n_runs, d_ends, d_ends + n_runs, out(), strand());
            HIP_CHECK(hipGetLastError());
        }
    }
    void download(hipStream_t st, int device_id, KmerRuns *runs) const {
        if (!n_runs) return;
        std::vector<uint64_t> *fields[5] = {&runs->q_record, &runs->q_start, &runs->kmers, &runs->t_record, &runs->t_start};
        for (int f = 0; f < 5; f++) {
            fields[f]->resize(n_runs);
            hu::download_sliced(fields[f]->data(), out() + f * n_runs, n_runs * 8, st, device_id);
        }
        runs->strand.resize(n_runs);
        hu::download_sliced(runs->strand.data(), strand(), n_runs, st, device_id);
    }
};

// The runs of ra.hit (filled on st) into *runs, in ascending query position. done(st) is called once the kernels are queued, before
// the stream is waited for: the caller's event mark and the downloads it wants in the same wait.
template <typename Done>
inline void runs_from_hits(const RunArgs &ra, hipStream_t st, int device_id, KmerRuns *runs, Done done) {
    RunStage stage(ra.n_bases);
    stage.queue(ra, st);
    done(st);
    HIP_CHECK(hipStreamSynchronize(st));
    stage.download(st, device_id, runs);
}

}  // namespace kr
}  // namespace mtg
