// unitig_components_device.hip -- the connected components of the unitig graph, labelled and measured on the GPU.
//
// Contract. Unitig u is edge 2u forwards and edge 2u + 1 backwards (host_graph.hpp); only the ORIGINAL edges count. Unitigs u and v
// are adjacent iff some orientation of the one links to some orientation of the other by the rule of DESIGN.md 26,
// from(edge o') == to(edge o); a component is a class of the closure of that. Components are numbered by their smallest unitig,
// ascending. Per component, in exact integers: its first unitig, its unitigs, k-mers and abundance, its link entries (those whose
// source orientation lies in it), its dead ends (orientations with no link) and its irregular orientations (those whose number of
// links is not 1; none: the component is a closed ring).
//
// Method. The link lists are never built: the links of o are the orientations that start at to(o), so
//   rep[x] = the smallest unitig with an orientation that starts at node x (one atomicMin per orientation), deg[x] = their number;
//   every orientation o whose end node x has a rep does union(o >> 1, rep[x]): all that END at x meet at the smallest that starts
//     there. Those that START at x end, mirrored, at mirror(x), where the same rule joins them to the smallest unitig that starts at
//     mirror(x), that is to one that ends at x. So wherever a link exists, both its sides are joined, and where nothing ends at a node
//     or nothing starts there, nothing is (hand case `siblings`);
//   the union-find is union_find_device.hpp's (roots hang below smaller ids: the final root is the component's smallest unitig in
//     any interleaving), flattened by one find per unitig; the roots are flagged, the flags scanned into component numbers.
// Statistics: one thread per unitig, links(o) = deg[to(o)], integer sums into per-component counters with atomics (any order gives
// the same sums). A read graph is one giant component plus dust, so the adds are aggregated first: the lanes of a wave that share
// the label of the first pending lane are reduced by shuffles, the waves of a block that hold the same label are summed in LDS and
// added once; a group of fewer than AGG_MIN lanes adds by itself. A node id outside the graph sets an error bit and is never an address.
// Limit: fewer than 2^31 unitigs.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "device.hpp"
#include "hip_util.hpp"
#include "pack_device.hpp"
#include "union_find_device.hpp"

namespace mtg {

namespace {

typedef unsigned long long u64;

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int ST_BLOCK = 1024;  // threads of a statistics block: its waves' sums meet in LDS
constexpr int AGG_MIN = 4;  // lanes of one label in a wave from which the reduction is cheaper than their own atomics

enum : unsigned { ERR_NODE_RANGE = 1 };
unsigned int *stage_err(const ScalarBlock &s) { return reinterpret_cast<unsigned int *>(s.d + 2); }

__global__ __launch_bounds__(hu::EB) void identity_kernel(uint32_t *parent, uint64_t U) {
    const uint64_t u = hu::gid();
    if (u < U) parent[u] = (uint32_t)u;
}

// rep[x] = the smallest unitig that starts at x, deg[x] = the orientations that start at x
__global__ __launch_bounds__(hu::EB) void node_kernel(const uint32_t *from, const uint32_t *to, uint64_t E, uint64_t V, uint32_t *rep, uint32_t *deg,
                                                      unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o >= E) return;
    const uint32_t n = from[o];
    if (n >= V || to[o] >= V) { atomicOr(err, ERR_NODE_RANGE); return; }
    atomicMin(&rep[n], (uint32_t)(o >> 1));
    atomicAdd(&deg[n], 1u);
}

__global__ __launch_bounds__(hu::EB) void union_kernel(const uint32_t *to, uint64_t E, uint64_t V, const uint32_t *rep, uint32_t *parent) {
    const uint64_t o = hu::gid();
    if (o >= E) return;
    const uint32_t n = to[o];
    if (n >= V) return;
    const uint32_t r = rep[n];
    if (r != NONE && r != (uint32_t)(o >> 1)) uf_union(parent, (uint32_t)(o >> 1), r);
}

// root[u] = the smallest unitig of u's component; flag[u] = 1 for the roots, 0 at u = U
__global__ __launch_bounds__(hu::EB) void flatten_kernel(uint32_t *parent, uint64_t U, uint32_t *root, uint32_t *flag) {
    const uint64_t u = hu::gid();
    if (u > U) return;
    if (u == U) { flag[u] = 0; return; }
    const uint32_t r = uf_find(parent, (uint32_t)u);
    root[u] = r;
    flag[u] = r == (uint32_t)u ? 1u : 0u;
}

// number[] = the exclusive scan of the flags; root[] becomes component_of[] in place (a thread reads its own word only)
__global__ __launch_bounds__(hu::EB) void number_kernel(uint32_t *root, uint64_t U, const uint32_t *number) {
    const uint64_t u = hu::gid();
    if (u < U) root[u] = number[root[u]];
}

struct Counters {
    uint32_t *first_unitig, *unitigs, *dead_ends, *irregular;
    u64 *kmers, *abundance, *links;
};

// what one unitig adds to its component; n packs {unitigs, dead ends, irregular} in 8 bits each (a wave sums at most 64, 128, 128)
struct Share {
    uint32_t n;
    u64 kmers, abundance, links;
};
// the sums of a group of unitigs of one component
struct Sum {
    uint32_t unitigs, dead_ends, irregular;
    u64 kmers, abundance, links;
};
__device__ __forceinline__ Sum sum_of(const Share &s) { return Sum{s.n & 0xFFu, (s.n >> 8) & 0xFFu, s.n >> 16, s.kmers, s.abundance, s.links}; }
__device__ __forceinline__ void add_sum(const Counters &c, uint32_t label, const Sum &s) {
    atomicAdd(&c.unitigs[label], s.unitigs);
    if (s.dead_ends) atomicAdd(&c.dead_ends[label], s.dead_ends);
    if (s.irregular) atomicAdd(&c.irregular[label], s.irregular);
    atomicAdd(&c.kmers[label], s.kmers);
    atomicAdd(&c.abundance[label], s.abundance);
    if (s.links) atomicAdd(&c.links[label], s.links);
}

// One thread per unitig. AGGREGATE: the lanes of a wave that share the label of the first pending lane are reduced by shuffles; the
// first such group of every wave goes to LDS, where the waves of the block that hold the same label are summed and added once (the
// giant component costs one set of atomics per ST_BLOCK unitigs); further groups of a wave are added by their lane 0, groups of
// fewer than AGG_MIN lanes by the lanes themselves.
template <bool AGGREGATE>
__global__ __launch_bounds__(ST_BLOCK) void stats_kernel(const uint32_t *component_of, const uint32_t *number, const uint32_t *to, const uint32_t *deg,
                                                         const u64 *kmers, const u64 *kc, uint64_t U, Counters c) {
    __shared__ uint32_t s_label[ST_BLOCK / 64];
    __shared__ Sum s_sum[ST_BLOCK / 64];
    const uint64_t u = hu::gid();
    const bool valid = u < U;  // (no early return: every lane of a wave takes part in the shuffles below)
    uint32_t label = NONE;
    Share s{0, 0, 0, 0};
    if (valid) {
        label = component_of[u];
        if (number[u + 1] != number[u]) c.first_unitig[label] = (uint32_t)u;  // a root: the one writer of this word
        const uint32_t d0 = deg[to[2 * u]], d1 = deg[to[2 * u + 1]];  // (the node ids were checked by node_kernel)
        s.n = 1u | (((d0 == 0) + (d1 == 0)) << 8) | (((d0 != 1) + (d1 != 1)) << 16);
        s.kmers = kmers[u];
        s.abundance = kc ? kc[u] : s.kmers;
        s.links = (u64)d0 + d1;
    }
    if (!AGGREGATE) {
        if (valid) add_sum(c, label, sum_of(s));
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_label[wave] = NONE;
    bool pending = valid, first = true;
    for (;;) {
        const u64 todo = __ballot(pending);
        if (!todo) break;
        const int lead = __ffsll(todo) - 1;
        const uint32_t lead_label = __shfl(label, lead, 64);
        const bool mine = pending && label == lead_label;
        const u64 group = __ballot(mine);
        if (__popcll(group) >= AGG_MIN) {  // (wave-uniform: `group` is the same in every lane)
            Share t = mine ? s : Share{0, 0, 0, 0};
            for (int d = 32; d > 0; d >>= 1) {
                t.n += __shfl_down(t.n, d, 64);
                t.kmers += __shfl_down(t.kmers, d, 64);
                t.abundance += __shfl_down(t.abundance, d, 64);
                t.links += __shfl_down(t.links, d, 64);
            }
            if (lane == 0) {
                if (first) { s_label[wave] = lead_label; s_sum[wave] = sum_of(t); }
                else add_sum(c, lead_label, sum_of(t));
            }
            first = false;
        } else if (mine) {
            add_sum(c, label, sum_of(s));
        }
        pending = pending && !mine;
    }
    __syncthreads();
    if (threadIdx.x < ST_BLOCK / 64) {  // the first wave that holds a label adds for the later ones
        const int w = threadIdx.x;
        const uint32_t l = s_label[w];
        bool owner = l != NONE;
        for (int v = 0; v < w; v++) owner = owner && s_label[v] != l;
        if (owner) {
            Sum t = s_sum[w];
            for (int v = w + 1; v < ST_BLOCK / 64; v++)
                if (s_label[v] == l) {
                    t.unitigs += s_sum[v].unitigs; t.dead_ends += s_sum[v].dead_ends; t.irregular += s_sum[v].irregular;
                    t.kmers += s_sum[v].kmers; t.abundance += s_sum[v].abundance; t.links += s_sum[v].links;
                }
            add_sum(c, l, t);
        }
    }
}

void need_device(int device_id, const char *who) {
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for %s", device_id, who);
    HIP_CHECK(hipSetDevice(device_id));
}

template <typename T>
T *host_array(uint64_t n) {
    T *p = static_cast<T *>(big_malloc((n + 1) * sizeof(T)));
    if (!p) MTG_DIE("out of memory (%llu components)", (unsigned long long)n);
    return p;
}

}  // namespace

uint64_t device_unitig_components(const HostGraph &g, const uint64_t *unitig_kmers, const uint64_t *unitig_kc, int device_id, bool aggregate,
                                  uint32_t **component_of_out, UnitigComponentArrays *out, UnitigComponentsTimes *times) {
    if (!g.built) MTG_DIE("mtg_unitig_components: graph is not built");
    const uint64_t E = g.n_original_edges, U = E / 2, V = g.node_count();
    if (E & 1) MTG_DIE("mtg_unitig_components: %llu original edges are not two per unitig", (unsigned long long)E);
    if (U >= (1ull << 31) || V >= 0xFFFFFFFFull) MTG_DIE("mtg_unitig_components: the graph is too large (%llu unitigs; the limit is 2^31 - 1)", (unsigned long long)U);
    if (U && !unitig_kmers) MTG_DIE("mtg_unitig_components: null argument");
    need_device(device_id, "the unitig components");
    device_arena_reset_peak(device_id);
    hipStream_t st = nullptr;
    UnitigComponentsTimes t;
    t.unitigs = U;
    uint64_t C = 0;
    {
        ScalarBlock small(st);
        const auto t0 = std::chrono::steady_clock::now();
        hu::DeviceArray<uint32_t> from(E + 1), to(E + 1);
        hu::DeviceArray<u64> d_kmers(U + 1), d_kc;
        hu::upload_sliced(from, g.e_from.data(), E * 4, st, device_id);
        hu::upload_sliced(to, g.e_to.data(), E * 4, st, device_id);
        hu::upload_sliced(d_kmers, unitig_kmers, U * 8, st, device_id);
        if (unitig_kc) {
            d_kc.alloc(U + 1);
            hu::upload_sliced(d_kc, unitig_kc, U * 8, st, device_id);
        }
        t.upload_ms = ms_since(t0);
        hu::DeviceArray<uint32_t> rep(V + 1), deg(V + 1), parent(U + 1), label(U + 1), number(U + 1);
        hu::ScanScratch<uint32_t> scan(U + 1);
        PhaseEvents<6> ev;  // 0 rep / degree 4 unions 5 flatten, scan, numbers 1 | 2 statistics 3
        ev.mark(0, st);
        HIP_CHECK(hipMemsetAsync(rep, 0xFF, (V + 1) * 4, st));
        HIP_CHECK(hipMemsetAsync(deg, 0, (V + 1) * 4, st));
        if (U) {
            identity_kernel<<<hu::grid_for(U), hu::EB, 0, st>>>(parent, U);
            node_kernel<<<hu::grid_for(E), hu::EB, 0, st>>>(from, to, E, V, rep, deg, stage_err(small));
            ev.mark(4, st);
            union_kernel<<<hu::grid_for(E), hu::EB, 0, st>>>(to, E, V, rep, parent);
            ev.mark(5, st);
        }
        flatten_kernel<<<hu::grid_for(U + 1), hu::EB, 0, st>>>(parent, U, label, number);
        scan.scan(st, number, U + 1, number.get());
        if (U) number_kernel<<<hu::grid_for(U), hu::EB, 0, st>>>(label, U, number);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        uint32_t n_comp = 0;
        HIP_CHECK(hipMemcpyAsync(&n_comp, scan.total(), 4, hipMemcpyDeviceToHost, st));
        small.read(st, "unitig components");
        if (small.h[2] & ERR_NODE_RANGE) MTG_DIE("unitig components: an edge names a node outside the graph");
        C = n_comp;
        hu::DeviceArray<uint32_t> c32(4 * C + 1);
        hu::DeviceArray<u64> c64(3 * C + 1);
        Counters c{c32.get(), c32.get() + C, c32.get() + 2 * C, c32.get() + 3 * C, c64.get(), c64.get() + C, c64.get() + 2 * C};
        ev.mark(2, st);
        HIP_CHECK(hipMemsetAsync(c32, 0, (4 * C + 1) * 4, st));
        HIP_CHECK(hipMemsetAsync(c64, 0, (3 * C + 1) * 8, st));
        if (U) {
            if (aggregate) stats_kernel<true><<<hu::grid_for(U, ST_BLOCK), ST_BLOCK, 0, st>>>(label, number, to, deg, d_kmers, unitig_kc ? d_kc.get() : nullptr, U, c);
            else stats_kernel<false><<<hu::grid_for(U, ST_BLOCK), ST_BLOCK, 0, st>>>(label, number, to, deg, d_kmers, unitig_kc ? d_kc.get() : nullptr, U, c);
        }
        HIP_CHECK(hipGetLastError());
        ev.mark(3, st);
        HIP_CHECK(hipStreamSynchronize(st));
        t.label_ms = ev.ms(0, 1);
        if (U) { t.rep_ms = ev.ms(0, 4); t.union_ms = ev.ms(4, 5); t.flatten_ms = ev.ms(5, 1); }
        t.stats_ms = ev.ms(2, 3);
        const auto td = std::chrono::steady_clock::now();
        uint32_t *component_of = host_array<uint32_t>(U);
        out->first_unitig = host_array<uint32_t>(C); out->unitigs = host_array<uint32_t>(C);
        out->dead_ends = host_array<uint32_t>(C); out->irregular = host_array<uint32_t>(C);
        out->kmers = host_array<uint64_t>(C); out->abundance = host_array<uint64_t>(C); out->links = host_array<uint64_t>(C);
        hu::download_sliced(component_of, label.get(), U * 4, st, device_id);
        hu::download_sliced(out->first_unitig, c.first_unitig, C * 4, st, device_id);
        hu::download_sliced(out->unitigs, c.unitigs, C * 4, st, device_id);
        hu::download_sliced(out->dead_ends, c.dead_ends, C * 4, st, device_id);
        hu::download_sliced(out->irregular, c.irregular, C * 4, st, device_id);
        hu::download_sliced(out->kmers, c.kmers, C * 8, st, device_id);
        hu::download_sliced(out->abundance, c.abundance, C * 8, st, device_id);
        hu::download_sliced(out->links, c.links, C * 8, st, device_id);
        t.download_ms = ms_since(td);
        *component_of_out = component_of;
    }
    t.components = C;
    uint64_t arena[4];
    device_arena_stats(device_id, arena);
    t.peak_arena_bytes = arena[2];
    if (times) *times = t;
    return C;
}

}  // namespace mtg
