// unitig_links_device.hip -- the unitig graph with its links, made on the GPU: the link lists of every oriented
// unitig and the whole text of a BCALM2/GGCAT FASTA file (`>u LN:i: KC:i: km:f: L:+:v:-`) or of a GFA1 file (`S` and `L` lines).
//
// Contract. Unitig u (record u of the store) is edge 2u forwards and edge 2u + 1 backwards (host_graph.hpp). Oriented unitig o links
// to o' iff from(edge o') == to(edge o), over the ORIGINAL edges only; the links of o are listed in ascending o'. link_off[2U + 1]
// (64-bit) and link_to[N] (32-bit edge ids) are indexed by o. A record lists the links of (u,+), then those of (u,-).
//
// Link stage: out-degree per node (atomics), scan, fill (atomics: any order), then every list is put into ascending order by a rank
// sort into a second array -- one thread per node for lists of at most LK_SMALL entries, one WORKGROUP per longer list (tiles of the
// list in LDS; any length) --, link_off = 64-bit scan of outdeg(to(o)), and an output-centric copy of the lists.
// Text stage, built like spell_device.hip: packed store (SeqStore), one extent per record, a 64-bit exclusive scan, and one
// output-centric kernel for both formats: a workgroup sweeps the bytes of the joint region of its 256 records (coalesced stores),
// each byte finds its record by binary search over the 257 region starts in LDS and then decodes which field, digit, link or base
// it is. The bytes of a record's links are found through a 64-bit scan of the per-link byte counts.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>

#include "device.hpp"
#include "hip_util.hpp"
#include "pack_device.hpp"

namespace mtg {

namespace {

constexpr int LK_BLOCK = 256;
constexpr int LK_SMALL = 8;      // lists up to this length are sorted by one thread in registers
constexpr int LK_TILE = 1024;    // keys of a long list held in LDS at a time
constexpr int LK_BIG_GRID = 1024;

typedef unsigned long long u64;

// error bits of this stage's kernels, in word 2 of the scalar block
enum : unsigned { ERR_NODE_RANGE = 1, ERR_EXTENT = 2 };
unsigned int *stage_err(const ScalarBlock &s) { return reinterpret_cast<unsigned int *>(s.d + 2); }

__global__ void out_degree_kernel(const uint32_t *from, uint64_t E, uint64_t V, uint32_t *deg, unsigned int *err) {
    const uint64_t e = hu::gid();
    if (e >= E) return;
    const uint32_t n = from[e];
    if (n >= V) { atomicOr(err, ERR_NODE_RANGE); return; }
    atomicAdd(&deg[n], 1u);
}

__global__ void fill_kernel(const uint32_t *from, uint64_t E, uint64_t V, const uint32_t *row, uint32_t *cursor, uint32_t *adj) {
    const uint64_t e = hu::gid();
    if (e >= E) return;
    const uint32_t n = from[e];
    if (n >= V) return;
    adj[row[n] + atomicAdd(&cursor[n], 1u)] = (uint32_t)e;
}

// lists of at most LK_SMALL edges: rank of every key among the (distinct) keys of its list; longer lists go to the work list
__global__ void sort_small_kernel(const uint32_t *row, uint64_t V, const uint32_t *adj, uint32_t *sorted, uint32_t *big, uint32_t *n_big) {
    const uint64_t n = hu::gid();
    if (n >= V) return;
    const uint32_t b = row[n], d = row[n + 1] - b;
    if (d == 0) return;
    if (d > (uint32_t)LK_SMALL) { big[atomicAdd(n_big, 1u)] = (uint32_t)n; return; }
    uint32_t key[LK_SMALL];
    for (int i = 0; i < LK_SMALL; i++) key[i] = (uint32_t)i < d ? adj[b + i] : 0xFFFFFFFFu;
    for (int i = 0; i < LK_SMALL; i++) {
        if ((uint32_t)i >= d) break;
        uint32_t r = 0;
        for (int j = 0; j < LK_SMALL; j++) r += key[j] < key[i] ? 1u : 0u;
        sorted[b + r] = key[i];
    }
}

// a workgroup per long list: every thread ranks its keys against the whole list, which passes through LDS tile by tile
__global__ __launch_bounds__(LK_BLOCK) void sort_big_kernel(const uint32_t *row, const uint32_t *adj, uint32_t *sorted, const uint32_t *big,
                                                          const uint32_t *n_big) {
    __shared__ uint32_t s_key[LK_TILE];
    const uint32_t nb = *n_big;
    for (uint32_t bi = blockIdx.x; bi < nb; bi += gridDim.x) {
        const uint32_t n = big[bi];
        const uint32_t b = row[n], d = row[n + 1] - b;
        for (uint32_t i0 = 0; i0 < d; i0 += LK_BLOCK) {
            const uint32_t i = i0 + threadIdx.x;
            const uint32_t mine = i < d ? adj[b + i] : 0u;
            uint32_t r = 0;
            for (uint32_t t0 = 0; t0 < d; t0 += LK_TILE) {
                __syncthreads();
                for (uint32_t x = threadIdx.x; x < (uint32_t)LK_TILE; x += LK_BLOCK) s_key[x] = t0 + x < d ? adj[b + t0 + x] : 0xFFFFFFFFu;
                __syncthreads();
                const uint32_t m = d - t0 < (uint32_t)LK_TILE ? d - t0 : (uint32_t)LK_TILE;
                if (i < d)
                    for (uint32_t x = 0; x < m; x++) r += s_key[x] < mine ? 1u : 0u;
            }
            if (i < d) sorted[b + r] = mine;
        }
    }
}

// cnt[o] = out-degree of to(edge o), 0 at o = E
__global__ void link_count_kernel(const uint32_t *to, uint64_t E, uint64_t V, const uint32_t *row, uint32_t *cnt, unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o > E) return;
    if (o == E) { cnt[o] = 0; return; }
    const uint32_t n = to[o];
    if (n >= V) { atomicOr(err, ERR_NODE_RANGE); cnt[o] = 0; return; }
    cnt[o] = row[n + 1] - row[n];
}

// a workgroup copies the lists of LK_BLOCK consecutive oriented unitigs, link by link in output order
__global__ __launch_bounds__(LK_BLOCK) void link_copy_kernel(const uint32_t *to, uint64_t E, const uint32_t *row, const uint32_t *sorted, const u64 *link_off,
                                                           uint32_t *link_to) {
    __shared__ u64 s_start[LK_BLOCK + 1];
    const uint64_t o0 = (uint64_t)blockIdx.x * LK_BLOCK;
    const uint32_t n_here = (uint32_t)(E - o0 < (uint64_t)LK_BLOCK ? E - o0 : (uint64_t)LK_BLOCK);
    for (uint32_t t = threadIdx.x; t <= n_here; t += LK_BLOCK) s_start[t] = link_off[o0 + t];
    __syncthreads();
    const u64 B0 = s_start[0], B1 = s_start[n_here];
    for (u64 j = B0 + threadIdx.x; j < B1; j += LK_BLOCK) {
        uint32_t lo = 0, hi = n_here;  // largest t with s_start[t] <= j
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_start[mid] <= j) lo = mid; else hi = mid;
        }
        link_to[j] = sorted[row[to[o0 + lo]] + (uint32_t)(j - s_start[lo])];
    }
}

// ---- text ----

__device__ __forceinline__ uint32_t digits_of(uint64_t v) {
    uint32_t d = 1;
    for (uint64_t p = 10; d < 20 && v >= p; p *= 10) d++;  // (no division: this runs for every byte of the text)
    return d;
}
// digit i (0 = most significant) of v, which has nd digits
__device__ __forceinline__ char digit_at(uint64_t v, uint32_t nd, uint32_t i) {
    for (uint32_t q = nd - 1 - i; q > 0; q--) v /= 10;
    return (char)('0' + v % 10);
}

struct TextArgs {
    const u64 *seq_off;        // [U + 1]
    const uint32_t *packed;
    const u64 *kc;             // [U] or null: the number of k-mers
    const u64 *link_off;       // [2U + 1]
    const uint32_t *link_to;   // [N]
    const u64 *link_bytes;     // [N + 1] exclusive scan of the bytes of every link's text
    uint64_t n_rec;            // U
    uint32_t k;
    uint32_t dk1;              // digits of k - 1
    int gfa;
    uint64_t head_bytes;       // the GFA header line in front of everything
};

// what a record's text consists of
struct Rec {
    uint64_t len, kc, t;       // t = round-half-up(10 KC / kmers)
    uint32_t du, dlen, dkc, dq;  // digits of u, len, KC and t / 10
    uint64_t lb;               // bytes of its links
    u64 l0, l1;                // its links
};
__device__ __forceinline__ Rec record_of(const TextArgs &a, uint64_t u) {
    Rec r;
    r.len = a.seq_off[u + 1] - a.seq_off[u];
    const uint64_t kmers = r.len + 1 - a.k;  // (>= 1: checked on the host)
    r.kc = kmers; r.t = 10;  // without abundances: one per k-mer, km 1.0
    if (a.kc) {  // (10 KC + kmers / 2) / kmers without the product 10 KC: KC = q kmers + m
        r.kc = a.kc[u];
        const uint64_t q = r.kc / kmers, m = r.kc % kmers;
        r.t = 10 * q + (10 * m + kmers / 2) / kmers;
    }
    r.du = digits_of(u); r.dlen = digits_of(r.len); r.dkc = digits_of(r.kc); r.dq = digits_of(r.t / 10);
    r.l0 = a.link_off[2 * u]; r.l1 = a.link_off[2 * u + 2];
    r.lb = a.link_bytes[r.l1] - a.link_bytes[r.l0];
    return r;
}
__device__ __forceinline__ uint32_t tags_bytes(const Rec &r) { return 18u + r.dlen + r.dkc + r.dq + 2u; }  // 3 x "{sep}XX:x:" + the values
__device__ __forceinline__ uint64_t record_bytes(const TextArgs &a, const Rec &r) {
    // BCALM2: ">" u tags links "\n" seq "\n"        GFA1: "S\t" u "\t" seq tags "\n" links
    return a.gfa ? 2u + r.du + 1u + r.len + tags_bytes(r) + 1u + r.lb : 1u + r.du + tags_bytes(r) + r.lb + 1u + r.len + 1u;
}
// byte i of "{sep}LN:i:{len}{sep}KC:i:{KC}{sep}km:f:{t / 10}.{t % 10}"
__device__ __forceinline__ char tag_char(const Rec &r, uint32_t i, char sep) {
    if (i < 6) return i == 0 ? sep : "LN:i:"[i - 1];
    i -= 6;
    if (i < r.dlen) return digit_at(r.len, r.dlen, i);
    i -= r.dlen;
    if (i < 6) return i == 0 ? sep : "KC:i:"[i - 1];
    i -= 6;
    if (i < r.dkc) return digit_at(r.kc, r.dkc, i);
    i -= r.dkc;
    if (i < 6) return i == 0 ? sep : "km:f:"[i - 1];
    i -= 6;
    if (i < r.dq) return digit_at(r.t / 10, r.dq, i);
    return i == r.dq ? '.' : (char)('0' + r.t % 10);
}
__device__ __forceinline__ char base_char(const TextArgs &a, uint64_t u, uint64_t i) { return "ACGT"[packed_base(a.packed, a.seq_off[u] + i)]; }
// byte i of the text of the links of record u
__device__ __forceinline__ char link_char(const TextArgs &a, const Rec &r, uint64_t u, uint64_t i) {
    const u64 want = a.link_bytes[r.l0] + i;
    u64 lo = r.l0, hi = r.l1;  // largest j with link_bytes[j] <= want
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (a.link_bytes[mid] <= want) lo = mid; else hi = mid;
    }
    uint32_t x = (uint32_t)(want - a.link_bytes[lo]);
    const uint32_t tgt = a.link_to[lo];
    const uint64_t v = tgt >> 1;
    const uint32_t dv = digits_of(v);
    const char sa = lo >= a.link_off[2 * u + 1] ? '-' : '+', sb = (tgt & 1u) ? '-' : '+';
    if (!a.gfa) {  // " L:{a}:{v}:{b}"
        if (x < 3) return " L:"[x];
        if (x == 3) return sa;
        if (x == 4) return ':';
        x -= 5;
        if (x < dv) return digit_at(v, dv, x);
        return x == dv ? ':' : sb;
    }
    // "L\t{u}\t{a}\t{v}\t{b}\t{k-1}M\n"
    if (x < 2) return x == 0 ? 'L' : '\t';
    x -= 2;
    if (x < r.du) return digit_at(u, r.du, x);
    x -= r.du;
    if (x < 3) return x == 1 ? sa : '\t';
    x -= 3;
    if (x < dv) return digit_at(v, dv, x);
    x -= dv;
    if (x < 3) return x == 1 ? sb : '\t';
    x -= 3;
    if (x < a.dk1) return digit_at(a.k - 1, a.dk1, x);
    return x == a.dk1 ? 'M' : '\n';
}

// bytes of the text of link j; the GFA line also names the record, found by binary search over link_off
__global__ void link_bytes_kernel(TextArgs a, uint64_t N, uint32_t *out) {
    const uint64_t j = hu::gid();
    if (j > N) return;
    if (j == N) { out[j] = 0; return; }
    const uint32_t dv = digits_of(a.link_to[j] >> 1);
    if (!a.gfa) { out[j] = 7u + dv; return; }
    uint64_t lo = 0, hi = 2 * a.n_rec;  // largest o with link_off[o] <= j
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.link_off[mid] <= j) lo = mid; else hi = mid;
    }
    out[j] = 10u + digits_of(lo >> 1) + dv + a.dk1;
}

__global__ void record_extent_kernel(TextArgs a, uint32_t *ext, unsigned int *err) {
    const uint64_t u = hu::gid();
    if (u > a.n_rec) return;
    if (u == a.n_rec) { ext[u] = 0; return; }
    const uint64_t b = record_bytes(a, record_of(a, u));
    if (b > 0xFFFFFFFFull) atomicOr(err, ERR_EXTENT);
    ext[u] = (uint32_t)b;
}

// a workgroup writes the joint region of LK_BLOCK consecutive records, byte by byte in output order
__global__ __launch_bounds__(LK_BLOCK) void graph_text_kernel(TextArgs a, const u64 *start, char *out) {
    __shared__ u64 s_start[LK_BLOCK + 1];
    const uint64_t u0 = (uint64_t)blockIdx.x * LK_BLOCK;
    const uint32_t n_here = (uint32_t)(a.n_rec - u0 < (uint64_t)LK_BLOCK ? a.n_rec - u0 : (uint64_t)LK_BLOCK);
    for (uint32_t t = threadIdx.x; t <= n_here; t += LK_BLOCK) s_start[t] = start[u0 + t];
    __syncthreads();
    const u64 B0 = s_start[0], B1 = s_start[n_here];
    for (u64 b = B0 + threadIdx.x; b < B1; b += LK_BLOCK) {
        uint32_t lo = 0, hi = n_here;  // largest t with s_start[t] <= b
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_start[mid] <= b) lo = mid; else hi = mid;
        }
        const uint64_t u = u0 + lo;
        const Rec r = record_of(a, u);
        uint64_t i = b - s_start[lo];
        const uint32_t tb = tags_bytes(r);
        char c;
        if (!a.gfa) {  // ">" u tags links "\n" seq "\n"
            if (i == 0) c = '>';
            else if ((i -= 1) < r.du) c = digit_at(u, r.du, (uint32_t)i);
            else if ((i -= r.du) < tb) c = tag_char(r, (uint32_t)i, ' ');
            else if ((i -= tb) < r.lb) c = link_char(a, r, u, i);
            else if ((i -= r.lb) == 0) c = '\n';
            else if ((i -= 1) < r.len) c = base_char(a, u, i);
            else c = '\n';
        } else {  // "S\t" u "\t" seq tags "\n" links
            if (i < 2) c = i == 0 ? 'S' : '\t';
            else if ((i -= 2) < r.du) c = digit_at(u, r.du, (uint32_t)i);
            else if ((i -= r.du) == 0) c = '\t';
            else if ((i -= 1) < r.len) c = base_char(a, u, i);
            else if ((i -= r.len) < tb) c = tag_char(r, (uint32_t)i, '\t');
            else if ((i -= tb) == 0) c = '\n';
            else c = link_char(a, r, u, i - 1);
        }
        out[a.head_bytes + b] = c;
    }
}

// The link lists of g's original edges on the current device. Leaves the stream idle.
struct DeviceLinks {
    hu::DeviceArray<u64> off;       // [E + 1]
    hu::DeviceArray<uint32_t> to;   // [max(N, 1)]
    uint64_t n_links = 0;
    double upload_ms = 0, kernel_ms = 0;
};

void build_links(const HostGraph &g, hipStream_t st, int device_id, ScalarBlock &small, DeviceLinks &L) {
    const uint64_t E = g.n_original_edges, V = g.node_count();
    if (E >= 0xFFFFFFFFull || V >= 0xFFFFFFFFull) MTG_DIE("unitig links: the graph is too large (%llu edges)", (unsigned long long)E);
    const auto t0 = std::chrono::steady_clock::now();
    hu::DeviceArray<uint32_t> from(E + 1), to(E + 1);
    hu::upload_sliced(from, g.e_from.data(), E * 4, st, device_id);
    hu::upload_sliced(to, g.e_to.data(), E * 4, st, device_id);
    L.upload_ms = ms_since(t0);
    hu::DeviceArray<uint32_t> deg(V + 1), row(V + 1), adj(E + 1), sorted(E + 1), big(E / (LK_SMALL + 1) + 2), cnt(E + 1);
    uint32_t *n_big = big.get() + E / (LK_SMALL + 1) + 1;
    L.off.alloc(E + 1);
    hu::ScanScratch<uint32_t> scan32(V + 1);
    hu::ScanScratch<u64> scan64(E + 1);
    PhaseEvents<3> ev;
    ev.mark(0, st);
    HIP_CHECK(hipMemsetAsync(deg, 0, (V + 1) * 4, st));
    HIP_CHECK(hipMemsetAsync(n_big, 0, 4, st));
    if (E) out_degree_kernel<<<hu::grid_for(E), hu::EB, 0, st>>>(from, E, V, deg, stage_err(small));
    scan32.scan(st, deg, V + 1, row.get());
    HIP_CHECK(hipMemsetAsync(deg, 0, (V + 1) * 4, st));  // (now the fill's cursors)
    if (E) fill_kernel<<<hu::grid_for(E), hu::EB, 0, st>>>(from, E, V, row, deg, adj);
    if (V) sort_small_kernel<<<hu::grid_for(V), hu::EB, 0, st>>>(row, V, adj, sorted, big, n_big);
    sort_big_kernel<<<LK_BIG_GRID, LK_BLOCK, 0, st>>>(row, adj, sorted, big, n_big);
    link_count_kernel<<<hu::grid_for(E + 1), hu::EB, 0, st>>>(to, E, V, row, cnt, stage_err(small));
    scan64.scan(st, cnt, E + 1, L.off.get());
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);
    u64 n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, scan64.total(), 8, hipMemcpyDeviceToHost, st));
    small.read(st, "unitig links");
    if (small.h[2] & ERR_NODE_RANGE) MTG_DIE("unitig links: an edge names a node outside the graph");
    L.n_links = n;
    L.to.alloc(n + 1);
    if (n) link_copy_kernel<<<hu::grid_for(E, LK_BLOCK), LK_BLOCK, 0, st>>>(to, E, row, sorted, L.off, L.to);
    HIP_CHECK(hipGetLastError());
    ev.mark(2, st);
    HIP_CHECK(hipStreamSynchronize(st));
    L.kernel_ms = ev.ms(0, 1) + ev.ms(1, 2);
}

void need_device(int device_id, const char *who) {
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for %s", device_id, who);
    HIP_CHECK(hipSetDevice(device_id));
}

}  // namespace

uint64_t device_unitig_links(const HostGraph &g, int device_id, uint64_t **link_off_out, uint32_t **link_to_out, UnitigGraphTimes *times) {
    if (!g.built) MTG_DIE("mtg_unitig_links: graph is not built");
    need_device(device_id, "the unitig links");
    device_arena_reset_peak(device_id);
    hipStream_t st = nullptr;
    UnitigGraphTimes t;
    const uint64_t E = g.n_original_edges;
    uint64_t N = 0;
    {
        ScalarBlock small(st);
        DeviceLinks L;
        build_links(g, st, device_id, small, L);
        N = L.n_links;
        t.upload_ms = L.upload_ms; t.link_ms = L.kernel_ms; t.links = N;
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t *off = static_cast<uint64_t *>(big_malloc((E + 1) * 8));
        uint32_t *to = static_cast<uint32_t *>(big_malloc((N + 1) * 4));
        if (!off || !to) MTG_DIE("out of memory (%llu links)", (unsigned long long)N);
        hu::download_sliced(off, L.off.get(), (E + 1) * 8, st, device_id);
        hu::download_sliced(to, L.to.get(), N * 4, st, device_id);
        t.download_ms = ms_since(t0);
        *link_off_out = off;
        *link_to_out = to;
    }
    uint64_t arena[4];
    device_arena_stats(device_id, arena);
    t.peak_arena_bytes = arena[2];
    if (times) *times = t;
    return N;
}

uint64_t device_write_unitig_graph_text(const HostGraph &g, const char *seqs, const uint64_t *seq_off, uint64_t n_unitigs, uint64_t k,
                                        const uint64_t *kc, bool gfa, int device_id, char **out_buf, UnitigGraphTimes *times) {
    if (!g.built) MTG_DIE("mtg_write_unitig_graph_text: graph is not built");
    if (k < 1 || k > 0xFFFFFFFFull) MTG_DIE("mtg_write_unitig_graph_text: k = %llu is out of range", (unsigned long long)k);
    const uint64_t U = g.n_original_edges / 2;
    if (n_unitigs != U) MTG_DIE("mtg_write_unitig_graph_text: %llu sequences for a graph of %llu unitigs", (unsigned long long)n_unitigs, (unsigned long long)U);
    if (seq_off[0] != 0) MTG_DIE("mtg_write_unitig_graph_text: the sequence offsets must start at 0");
    for (uint64_t u = 0; u < U; u++)
        if (seq_off[u + 1] < seq_off[u] + k) MTG_DIE("mtg_write_unitig_graph_text: unitig %llu is shorter than k = %llu", (unsigned long long)u, (unsigned long long)k);
    need_device(device_id, "the unitig graph text");
    device_arena_reset_peak(device_id);
    hipStream_t st = nullptr;
    UnitigGraphTimes t;
    const std::string head = gfa ? "H\tVN:Z:1.0\tKL:Z:" + std::to_string(k) + "\n" : std::string();
    uint64_t total = head.size();
    char *out = nullptr;
    if (U) {
        SeqStore seq("unitig sequences", seqs, seq_off, U, st, device_id);
        DeviceLinks L;
        build_links(g, st, device_id, seq.small, L);
        const uint64_t N = L.n_links;
        t.upload_ms = L.upload_ms + seq.upload_ms; t.link_ms = L.kernel_ms; t.links = N;
        const auto tu = std::chrono::steady_clock::now();
        hu::DeviceArray<u64> d_kc;
        if (kc) {
            d_kc.alloc(U);
            hu::upload_sliced(d_kc, kc, U * 8, st, device_id);
        }
        t.upload_ms += ms_since(tu);
        hu::DeviceArray<uint32_t> lens(N + 1), ext(U + 1);
        hu::DeviceArray<u64> link_bytes(N + 1), start(U + 1);
        hu::ScanScratch<u64> scan(std::max(N, U) + 1);
        TextArgs a{};
        a.seq_off = seq.off; a.packed = seq.packed; a.kc = kc ? d_kc.get() : nullptr; a.link_off = L.off; a.link_to = L.to;
        a.link_bytes = link_bytes; a.n_rec = U; a.k = (uint32_t)k; a.gfa = gfa ? 1 : 0; a.head_bytes = head.size();
        a.dk1 = (uint32_t)std::to_string(k - 1).size();
        PhaseEvents<3> ev;
        ev.mark(0, st);
        link_bytes_kernel<<<hu::grid_for(N + 1), hu::EB, 0, st>>>(a, N, lens);
        scan.scan(st, lens, N + 1, link_bytes.get());
        record_extent_kernel<<<hu::grid_for(U + 1), hu::EB, 0, st>>>(a, ext, stage_err(seq.small));
        scan.scan(st, ext, U + 1, start.get());
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        u64 body = 0;
        HIP_CHECK(hipMemcpyAsync(&body, scan.total(), 8, hipMemcpyDeviceToHost, st));
        seq.small.read(st, "unitig graph text");
        if (seq.small.h[2] & ERR_EXTENT) MTG_DIE("mtg_write_unitig_graph_text: the text of one unitig with its links exceeds 4 GiB");
        total += body;
        hu::DeviceArray<char> d_out(total);
        if (head.size()) HIP_CHECK(hipMemcpyAsync(d_out, head.data(), head.size(), hipMemcpyHostToDevice, st));
        graph_text_kernel<<<hu::grid_for(U, LK_BLOCK), LK_BLOCK, 0, st>>>(a, start, d_out);
        HIP_CHECK(hipGetLastError());
        ev.mark(2, st);
        HIP_CHECK(hipStreamSynchronize(st));
        t.text_prepare_ms = ev.ms(0, 1);
        t.text_ms = ev.ms(1, 2);
        const auto td = std::chrono::steady_clock::now();
        out = static_cast<char *>(big_malloc(total + 1));
        if (!out) MTG_DIE("out of memory (%llu bytes)", (unsigned long long)total);
        hu::download_sliced(out, d_out.get(), total, st, device_id);
        t.download_ms = ms_since(td);
        // what the text kernel must move: the text once, the packed bases once, per record its start and offsets, per link its target and byte offset
        t.text_min_bytes = total + seq.n_bases / 4 + U * (8 + 8 + 16 + (kc ? 8 : 0)) + N * (4 + 8);
    } else {
        out = static_cast<char *>(std::malloc(total + 1));
        if (!out) MTG_DIE("out of memory");
        std::memcpy(out, head.data(), total);
    }
    out[total] = '\0';
    t.bytes = total;
    uint64_t arena[4];
    device_arena_stats(device_id, arena);
    t.peak_arena_bytes = arena[2];
    if (times) *times = t;
    *out_buf = out;
    return total;
}

}  // namespace mtg
