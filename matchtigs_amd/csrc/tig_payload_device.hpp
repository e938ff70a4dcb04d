// tig_payload_device.hpp -- payloads hung off text positions: the weights and colour masks of the sparse minimizer index
//
// The table index keeps a weight or a mask per table slot; the sparse index (tig_index_device.hip) has no slot per k-mer, but its
// locate probe gives, per found window, the smallest window start t of its class in the indexed text -- the very position whose
// weight or mask the table keeps. So the payload is kept once per WINDOW of the indexed text and looked up by t.
//
// Addressing. A payload is addressed by window ORDINAL, the order the caller gives it in: the windows of record 0 from left to right,
// then record 1's; a record shorter than k has none. The window at global base start t of record r has the ordinal
// win_off[r] + (t - off[r]) (weight_gather_kernel's rule), win_off[r] = the windows of the records before r.
//
// Layouts, chosen per payload from the byte counts alone (W windows, R runs):
//   dense   one element per window, WIDTH bytes: weights the narrowest of 1, 2, 4 that holds the largest, masks the narrowest of 1,
//           2, 4, 8 that holds n_colors bits; value[ordinal]. WIDTH * W bytes.
//   runs    the maximal runs of equal consecutive values over the ordinals (a run may cross a record border): start[R] (64-bit,
//           ascending, start[0] == 0) and value[R] (V); the largest i with start[i] <= ordinal, by binary search. (8 + sizeof V) R bytes.
// runs iff (8 + sizeof V) R < WIDTH W, dense otherwise (a tie is dense); a caller may force either.
//
// Build (payload_build), all on the device from the uploaded V per window:
//   reduce  payload_max_kernel: the largest value (weights: the width)
//   flag    payload_flag_kernel: head[w] = (w == 0 || v[w] != v[w - 1]); hu::scan_u32 ranks the heads, its total is R
//   compact payload_compact_kernel: (start, value)[rank[w]] = (w, v[w]) at every head -- or --
//   narrow  payload_narrow_kernel: dense[w] = (T) v[w]
// The uploaded array (4 or 8 B per window), the heads (4 B) and their ranks (8 B) are transient and go back to the arena: the build
// peak beside the index is 16 or 20 B per window plus the payload itself.
//
// Gather (two passes: tig_locate_kernel has filled hit[q] = (t << 1) | strand first). A thread owns kw::RUN consecutive query
// positions; per found window: t, the index record of t (the last [lo, hi) and its win_off are kept), the ordinal, the value -- a
// Cursor keeps the last run [lo, hi) and its value in registers, so a window that lands in the run of the one before costs no search.
// abundance_gather_kernel folds sum / min / max per (thread, query record) and leaves by one atomicAdd, atomicMin, atomicMax when
// the record changes (abundance_kernel's rule); color_gather_kernel keeps (record, mask, run length) and flushes one atomicAdd per
// set bit (color_query_kernel's rule). per_window has one writer per position, zeros included. Sums of integers, minima and maxima:
// the results do not depend on the launch geometry or the order the atomics land in.
//
// The kernels are static: every translation unit that includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_runs_device.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"

namespace mtg {
namespace tp {

constexpr uint32_t LAYOUT_AUTO = 0, LAYOUT_DENSE = 1, LAYOUT_RUNS = 2;

// what a kernel reads of a payload of V (uint32_t weights, unsigned long long masks)
template <typename V>
struct View {
    const unsigned char *dense;       // dense: [windows * width]
    const unsigned long long *start;  // runs: [runs]
    const V *value;                   // runs: [runs]
    uint64_t windows, runs;
    uint32_t width;  // dense: bytes per element; 0: the runs layout
};

// a payload on the device, owned by its index
template <typename V>
struct Payload {
    mtg_tig_payload info{};  // layout 0: there is none
    hu::DeviceArray<unsigned char> dense;
    hu::DeviceArray<unsigned long long> start;
    hu::DeviceArray<V> value;
    bool present() const { return info.layout != 0; }
    View<V> view() const { return View<V>{dense, start, value, info.windows, info.runs, info.layout == LAYOUT_DENSE ? (uint32_t)info.width : 0u}; }
};

struct PayloadBuildTimes {
    double upload_ms = 0, reduce_ms = 0, flag_scan_ms = 0, store_ms = 0;  // store: compact or narrow
};

// *out = max(*out, v[w]) over all w; *out zeroed before. A thread strides over the array and leaves by one atomicMax.
template <typename V>
static __global__ __launch_bounds__(hu::EB) void payload_max_kernel(const V *v, uint64_t n, unsigned long long *out) {
    unsigned long long best = 0;
    for (uint64_t w = hu::gid(), step = (uint64_t)gridDim.x * blockDim.x; w < n; w += step) best = v[w] > best ? (unsigned long long)v[w] : best;
    if (best) atomicMax(out, best);
}
template <typename V>
static __global__ __launch_bounds__(hu::EB) void payload_flag_kernel(const V *v, uint64_t n, uint32_t *head) {
    const uint64_t w = hu::gid();
    if (w < n) head[w] = w == 0 || v[w] != v[w - 1];
}
// rank[w] = the heads before w
template <typename V>
static __global__ __launch_bounds__(hu::EB) void payload_compact_kernel(const V *v, uint64_t n, const uint32_t *head, const unsigned long long *rank,
                                                                        uint64_t n_runs, unsigned long long *start, V *value) {
    const uint64_t w = hu::gid();
    if (w >= n || !head[w]) return;
    const uint64_t i = rank[w];
    if (i >= n_runs) return;  // (the scan counted exactly the heads: never)
    start[i] = w;
    value[i] = v[w];
}
template <typename V, typename T>
static __global__ __launch_bounds__(hu::EB) void payload_narrow_kernel(const V *v, uint64_t n, T *dense) {
    const uint64_t w = hu::gid();
    if (w < n) dense[w] = (T)v[w];
}

inline uint32_t width_of_weight(uint64_t largest) { return largest < (1ull << 8) ? 1 : largest < (1ull << 16) ? 2 : 4; }
inline uint32_t width_of_mask(uint64_t n_colors) { return n_colors <= 8 ? 1 : n_colors <= 16 ? 2 : n_colors <= 32 ? 4 : 8; }

// The payload of the host array v[n_windows]; mask_colors: 0 for weights (the width comes from the largest), else n_colors.
// layout: LAYOUT_AUTO or the forced one.
template <typename V>
inline void payload_build(Payload<V> &p, const V *v, uint64_t n_windows, uint64_t mask_colors, uint32_t layout, hipStream_t st, int device_id,
                          PayloadBuildTimes *times) {
    mtg_tig_payload &info = p.info;
    info = mtg_tig_payload{};
    info.windows = n_windows;
    info.width = mask_colors ? width_of_mask(mask_colors) : 1;
    uint64_t n_runs = 0;
    PhaseEvents<4> ev;
    hu::DeviceArray<V> d_v;
    hu::DeviceArray<uint32_t> d_head;
    hu::DeviceArray<unsigned long long> d_rank;
    const auto t0 = std::chrono::steady_clock::now();
    if (n_windows) {
        d_v.alloc(n_windows);
        hu::upload_sliced(d_v, v, n_windows * sizeof(V), st, device_id);
    }
    const double upload_ms = ms_since(t0);
    ev.mark(0, st);
    if (n_windows) {
        const unsigned grid = hu::grid_for(n_windows);
        if (!mask_colors) {
            hu::DeviceArray<unsigned long long> d_max(1);
            unsigned long long largest = 0;
            HIP_CHECK(hipMemsetAsync(d_max, 0, 8, st));
            payload_max_kernel<V><<<grid < 1024 ? grid : 1024, hu::EB, 0, st>>>(d_v, n_windows, d_max);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(&largest, d_max, 8, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            info.width = width_of_weight(largest);
        }
        ev.mark(1, st);
        d_head.alloc(n_windows);
        d_rank.alloc(n_windows);
        hu::ScanScratch<unsigned long long> scan(n_windows);
        payload_flag_kernel<V><<<grid, hu::EB, 0, st>>>(d_v, n_windows, d_head);
        HIP_CHECK(hipGetLastError());
        scan.scan(st, d_head, n_windows, d_rank);
        HIP_CHECK(hipMemcpyAsync(&n_runs, scan.total(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    } else {
        ev.mark(1, st);
    }
    ev.mark(2, st);
    info.runs = n_runs;
    const uint64_t runs_bytes = (8 + sizeof(V)) * n_runs, dense_bytes = info.width * n_windows;
    info.layout = layout == LAYOUT_AUTO ? (runs_bytes < dense_bytes ? LAYOUT_RUNS : LAYOUT_DENSE) : layout;
    if (info.layout == LAYOUT_RUNS) {
        info.device_bytes = runs_bytes;
        p.start.alloc(n_runs ? n_runs : 1);  // (an index without windows: never read)
        p.value.alloc(n_runs ? n_runs : 1);
        if (n_windows) payload_compact_kernel<V><<<hu::grid_for(n_windows), hu::EB, 0, st>>>(d_v, n_windows, d_head, d_rank, n_runs, p.start, p.value);
    } else {
        info.device_bytes = dense_bytes;
        p.dense.alloc(dense_bytes ? dense_bytes : 1);
        const unsigned grid = hu::grid_for(n_windows);
        if (!n_windows) {
        } else if (info.width == 1) {
            payload_narrow_kernel<V, uint8_t><<<grid, hu::EB, 0, st>>>(d_v, n_windows, reinterpret_cast<uint8_t *>(p.dense.get()));
        } else if (info.width == 2) {
            payload_narrow_kernel<V, uint16_t><<<grid, hu::EB, 0, st>>>(d_v, n_windows, reinterpret_cast<uint16_t *>(p.dense.get()));
        } else if (info.width == 4) {
            payload_narrow_kernel<V, uint32_t><<<grid, hu::EB, 0, st>>>(d_v, n_windows, reinterpret_cast<uint32_t *>(p.dense.get()));
        } else {
            payload_narrow_kernel<V, unsigned long long><<<grid, hu::EB, 0, st>>>(d_v, n_windows, reinterpret_cast<unsigned long long *>(p.dense.get()));
        }
    }
    HIP_CHECK(hipGetLastError());
    ev.mark(3, st);
    HIP_CHECK(hipStreamSynchronize(st));  // (the transient arrays go back only once the kernels are through)
    if (times) *times = PayloadBuildTimes{upload_ms, ev.ms(0, 1), ev.ms(1, 2), ev.ms(2, 3)};
}

// The value at an ordinal. The last run [lo, hi) and its value stay in registers (dense: not used).
template <typename V>
struct Cursor {
    uint64_t lo = 1, hi = 0;  // none yet
    V val = 0;
    __device__ __forceinline__ V at(const View<V> &p, uint64_t ord) {
        if (p.width) {
            switch (p.width) {
            case 1: return (V)p.dense[ord];
            case 2: return (V) reinterpret_cast<const uint16_t *>(p.dense)[ord];
            case 4: return (V) reinterpret_cast<const uint32_t *>(p.dense)[ord];
            default: return (V) reinterpret_cast<const unsigned long long *>(p.dense)[ord];
            }
        }
        if (ord < lo || ord >= hi) {
            uint64_t a = 0, b = p.runs;  // start[0] == 0 <= ord: the largest i with start[i] <= ord
            while (b - a > 1) {
                const uint64_t mid = a + (b - a) / 2;
                if (p.start[mid] <= ord) a = mid;
                else b = mid;
            }
            lo = p.start[a];
            hi = a + 1 < p.runs ? p.start[a + 1] : p.windows;
            val = p.value[a];
        }
        return val;
    }
};

// what the gather kernels read beside the payload: the hits of the query's positions, the record offsets of the query and of the
// index, the windows before every index record
struct GatherArgs {
    const unsigned long long *hit;      // [n_bases]
    const unsigned long long *q_off;    // [q_rec + 1]
    const unsigned long long *t_off;    // [t_rec + 1]
    const unsigned long long *win_off;  // [t_rec + 1]
    uint64_t n_bases, q_rec, t_rec;
    unsigned int *err;  // bit 0: an ordinal beyond the payload (never)
};

// the found windows of a thread's positions in ascending order: each(p, query record, ordinal); per_window positions without a hit
// are zeroed on the way. The query record and the index record of the window before are kept: neighbours mostly share both.
template <typename PW, typename Each>
__device__ __forceinline__ void gather_run(const GatherArgs &g, uint64_t windows, PW *per_window, Each each) {
    const uint64_t p0 = hu::gid() * kw::RUN;
    if (p0 >= g.n_bases) return;
    const uint64_t end = p0 + kw::RUN < g.n_bases ? p0 + kw::RUN : g.n_bases;
    uint64_t q_lo = 1, q_hi = 0, q_r = 0;             // the query record of the last hit: none yet
    uint64_t t_lo = 1, t_hi = 0, t_win = 0;           // the index record of the last hit and the windows before it
    for (uint64_t p = p0; p < end; p++) {
        const unsigned long long h = g.hit[p];
        if (h == kr::NO_HIT) {
            if (per_window) per_window[p] = 0;
            continue;
        }
        const uint64_t t = h >> 1;
        if (p < q_lo || p >= q_hi) {
            q_r = kr::record_of(g.q_off, g.q_rec, p);
            q_lo = g.q_off[q_r];
            q_hi = g.q_off[q_r + 1];
        }
        if (t < t_lo || t >= t_hi) {
            const uint64_t r = kr::record_of(g.t_off, g.t_rec, t);
            t_lo = g.t_off[r];
            t_hi = g.t_off[r + 1];
            t_win = g.win_off[r];
        }
        const uint64_t ord = t_win + (t - t_lo);
        if (ord >= windows) {  // (a hit is a window start of the index: never)
            atomicOr(g.err, 1u);
            if (per_window) per_window[p] = 0;
            continue;
        }
        each(p, q_r, ord);
    }
}

// sum: [q_rec] zeroed; minmax: [2 q_rec] the smallest (all ones before) and the largest (0 before) weight; per_window: [n_bases] or null
static __global__ __launch_bounds__(hu::EB) void abundance_gather_kernel(GatherArgs g, View<uint32_t> pl, unsigned long long *sum, uint32_t *minmax,
                                                                         uint32_t *per_window) {
    Cursor<uint32_t> cur;
    uint64_t rec = 0, total = 0;
    uint32_t lo = ~0u, hi = 0, hits = 0;  // (of the record `rec`; at most RUN hits)
    auto flush = [&]() {
        if (!hits) return;
        atomicAdd(&sum[rec], (unsigned long long)total);
        atomicMin(&minmax[rec], lo);
        atomicMax(&minmax[g.q_rec + rec], hi);
        total = 0; lo = ~0u; hi = 0; hits = 0;
    };
    gather_run(g, pl.windows, per_window, [&](uint64_t p, uint64_t r, uint64_t ord) {
        if (r != rec) {
            flush();
            rec = r;
        }
        const uint32_t w = cur.at(pl, ord);
        total += w;
        lo = w < lo ? w : lo;
        hi = w > hi ? w : hi;
        hits++;
        if (per_window) per_window[p] = w;
    });
    flush();
}

// per_color: [q_rec * C], zeroed (no mask has a bit from C on: the build checked); per_window: [n_bases] or null
static __global__ __launch_bounds__(hu::EB) void color_gather_kernel(GatherArgs g, View<unsigned long long> pl, uint32_t C, uint32_t *per_color,
                                                                     unsigned long long *per_window) {
    Cursor<unsigned long long> cur;
    unsigned long long mask = 0;
    uint64_t rec = 0;
    uint32_t run = 0;  // found windows of record `rec` with the mask `mask` since the last flush (at most RUN)
    auto flush = [&]() {
        for (unsigned long long m = run ? mask : 0ull; m; m &= m - 1) atomicAdd(&per_color[rec * C + (uint32_t)__builtin_ctzll(m)], run);
        run = 0;
    };
    gather_run(g, pl.windows, per_window, [&](uint64_t p, uint64_t r, uint64_t ord) {
        const unsigned long long m = cur.at(pl, ord);
        if (r != rec || m != mask) {
            flush();
            rec = r;
            mask = m;
        }
        run++;
        if (per_window) per_window[p] = m;
    });
    flush();
}

}  // namespace tp
}  // namespace mtg
