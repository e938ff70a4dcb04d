// unitig_bubbles_device.hip -- the bubbles of the unitig graph as variant calls, found and described on the GPU.
//
// Contract. Unitig u (record u of the store) is edge 2u forwards and edge 2u + 1 backwards (host_graph.hpp); only the ORIGINAL edges
// count. With x = from(2u), y = to(2u) and n(u) = len - k + 1, u is a CANDIDATE ARM iff n(u) < L and none of x = mirror(x),
// y = mirror(y), x = y, x = mirror(y) holds (DESIGN.md 25's rule: no self-mirror end, no loop, no hairpin). Its key is the smaller of
// the node-id pairs (x, y) and (mirror(y), mirror(x)); the candidates of one key are a bundle, a bundle of two or more a BUBBLE.
// Arm a is better than b iff kc[a] n(b) > kc[b] n(a) (128-bit products), on equality the smaller unitig; the best arm r is the
// reference arm, and the bubble is read in r's + orientation: arm a has strand 0 (+) iff it is canonical the same way round as r,
// else 1 (-), and its allele is the oriented unitig 2a + strand. Bubbles are numbered by their smallest unitig, ascending; inside a
// bubble r is arm 0 and the others follow ascending by unitig. Per non-reference arm, against R = seq(2r): suffix = the longest
// common suffix (at most the shorter length), prefix = the longest common prefix of what is left (at most the shorter length less
// the suffix: indels come out left-aligned), differences = the differing positions between them where the lengths agree, else 0.
// carried[arm, c] = the arm's k-mers whose colour mask has bit c. Nothing depends on the order in which atomics land.
//
// Method. keys: one thread per unitig. group: an open-addressing table over the keys (2 slots per unitig, claimed by CAS, full keys
// compared) that keeps per slot the member count, the smallest member (atomicMin) and, by a CAS loop under the order above, the best
// arm. number: the slots of two or more members are flagged at their smallest member; a scan of the flags numbers the bubbles, a
// 64-bit scan of the member counts gives arm_off; the members land in their segment in any order and a wave per bubble ranks each
// against the others (quadratic in the arms of one bubble: a hub of some hundred arms is 10^5 comparisons). alleles: one wave per
// arm; a record is read in either orientation 16 bases at a time (a backwards read is the word reversed and complemented), the
// common suffix is the common prefix of the two reverse complements, so one loop serves both: 64 lanes x 16 bases per step, a ballot
// of the lanes with a non-zero XOR, the first such lane's trailing zeros / 2. carriers: one wave per arm, 64 masks per step, one
// ballot per colour. A node id outside the graph sets an error bit and is never an address.
// Limit: fewer than 2^31 - 1 unitigs (the table's 2 U + 2 slot numbers stay below the 32-bit "no slot"), arms of fewer than 2^31
// k-mers (L is clamped), at most 64 colours.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "device.hpp"
#include "hip_util.hpp"
#include "pack_device.hpp"

namespace mtg {

namespace {

typedef unsigned long long u64;

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr u64 NO_KEY = ~0ull;
constexpr int WAVE = 64;
constexpr int WB = 256;  // threads of a block of the wave-per-item kernels: four waves

enum : unsigned { ERR_NODE_RANGE = 1, ERR_TABLE = 2 };
unsigned int *stage_err(const ScalarBlock &s) { return reinterpret_cast<unsigned int *>(s.d + 2); }

struct Table {
    u64 *key;          // [slots] NO_KEY: empty
    uint32_t *count;   // [slots] members
    uint32_t *least;   // [slots] the smallest member
    uint32_t *best;    // [slots] the best member
    uint64_t slots;
};

__device__ __forceinline__ u64 mix64(u64 x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

__device__ __forceinline__ uint32_t kmers_of(const u64 *off, uint64_t u, uint32_t k) { return (uint32_t)(off[u + 1] - off[u] - (k - 1)); }

// key[u] = the canonical node pair of a candidate (NO_KEY: none), flip[u] = 1 iff the mirrored pair is the canonical one
__global__ __launch_bounds__(hu::EB) void keys_kernel(const uint32_t *from, const uint32_t *to, const uint32_t *mirror, const u64 *off, uint64_t U,
                                                      uint64_t V, uint32_t k, uint64_t L, u64 *key, uint8_t *flip, unsigned int *err) {
    const uint64_t u = hu::gid();
    if (u >= U) return;
    key[u] = NO_KEY;
    flip[u] = 0;
    const uint32_t x = from[2 * u], y = to[2 * u];
    if (x >= V || y >= V) { atomicOr(err, ERR_NODE_RANGE); return; }
    const uint32_t mx = mirror[x], my = mirror[y];
    if (mx >= V || my >= V) { atomicOr(err, ERR_NODE_RANGE); return; }
    if (off[u + 1] - off[u] - (k - 1) >= L) return;
    if (x == mx || y == my || x == y || x == my) return;
    const u64 a = ((u64)x << 32) | y, b = ((u64)my << 32) | mx;
    key[u] = a < b ? a : b;
    flip[u] = b < a ? 1 : 0;
}

// a better than b: kc[a] n(b) > kc[b] n(a) in 128 bits, then the smaller unitig
__device__ __forceinline__ bool arm_better(const u64 *kc, const u64 *off, uint32_t k, uint32_t a, uint32_t b) {
    const u64 na = kmers_of(off, a, k), nb = kmers_of(off, b, k);
    const u64 ka = kc ? kc[a] : na, kb = kc ? kc[b] : nb;
    const u64 lh = __umul64hi(ka, nb), ll = ka * nb, rh = __umul64hi(kb, na), rl = kb * na;
    if (lh != rh) return lh > rh;
    if (ll != rl) return ll > rl;
    return a < b;
}

// A claimed slot keeps its key for good, so every key owns one slot; the count is a sum, the least a minimum and the best the
// maximum of a total order: the same in any interleaving.
__global__ __launch_bounds__(hu::EB) void group_kernel(const u64 *key, const u64 *kc, const u64 *off, uint64_t U, uint32_t k, Table t, uint32_t *slot_of,
                                                       unsigned int *err) {
    const uint64_t g = hu::gid();
    if (g >= U) return;
    const uint32_t u = (uint32_t)g;
    slot_of[u] = NONE;
    const u64 mine = key[u];
    if (mine == NO_KEY) return;
    uint64_t s = __umul64hi(mix64(mine), t.slots);
    for (uint64_t probe = 0; probe < t.slots; probe++) {
        u64 cur = __hip_atomic_load(&t.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == NO_KEY) {
            cur = atomicCAS(&t.key[s], NO_KEY, mine);
            if (cur == NO_KEY) cur = mine;
        }
        if (cur == mine) {
            slot_of[u] = (uint32_t)s;
            atomicAdd(&t.count[s], 1u);
            atomicMin(&t.least[s], u);
            uint32_t b = __hip_atomic_load(&t.best[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (b == NONE || arm_better(kc, off, k, u, b)) {
                const uint32_t prev = atomicCAS(&t.best[s], b, u);
                if (prev == b) break;
                b = prev;
            }
            return;
        }
        if (++s == t.slots) s = 0;
    }
    atomicOr(err, ERR_TABLE);  // (2 slots per unitig: never full)
}

// flag[u] = 1 and arms[u] = the members where u is the smallest member of a bundle of two or more; both 0 elsewhere and at u = U
__global__ __launch_bounds__(hu::EB) void flag_kernel(const uint32_t *slot_of, Table t, uint64_t U, uint32_t *flag, uint32_t *arms) {
    const uint64_t u = hu::gid();
    if (u > U) return;
    uint32_t f = 0, a = 0;
    if (u < U) {
        const uint32_t s = slot_of[u];
        if (s != NONE && t.least[s] == (uint32_t)u && t.count[s] >= 2) { f = 1; a = t.count[s]; }
    }
    flag[u] = f;
    arms[u] = a;
}

// number[]: the exclusive scan of the flags, base[]: that of the member counts. The first member writes arm_off and the bubble's
// slot; every member takes a place of its bubble's segment (any order).
__global__ __launch_bounds__(hu::EB) void scatter_kernel(const uint32_t *slot_of, Table t, uint64_t U, const uint32_t *number, const u64 *base, uint64_t B,
                                                         uint64_t A, u64 *arm_off, uint32_t *slot_of_bubble, uint32_t *cursor, uint32_t *unsorted) {
    const uint64_t u = hu::gid();
    if (u == U) arm_off[B] = A;
    if (u >= U) return;
    const uint32_t s = slot_of[u];
    if (s == NONE || t.count[s] < 2) return;
    const uint32_t first = t.least[s];
    if (first == (uint32_t)u) {
        arm_off[number[u]] = base[u];
        slot_of_bubble[number[u]] = s;
    }
    unsorted[base[first] + atomicAdd(&cursor[s], 1u)] = (uint32_t)u;
}

struct Arms {
    uint32_t *unitig, *kmers, *ref;  // ref: the bubble's reference unitig, for the allele kernel
    uint8_t *strand;
    u64 *abundance;
};

// A wave per bubble: member m goes to 0 if it is the reference arm r, else to 1 + the members below it, r apart.
__global__ __launch_bounds__(WB) void order_kernel(const u64 *arm_off, const uint32_t *slot_of_bubble, Table t, const uint32_t *unsorted, const uint8_t *flip,
                                                   const u64 *kc, const u64 *off, uint32_t k, uint64_t B, Arms out) {
    const uint64_t b = hu::gid() / WAVE;
    if (b >= B) return;  // (wave-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const u64 lo = arm_off[b];
    const uint32_t d = (uint32_t)(arm_off[b + 1] - lo), r = t.best[slot_of_bubble[b]];
    for (uint32_t i = lane; i < d; i += WAVE) {
        const uint32_t m = unsorted[lo + i];
        uint32_t at = 0;
        if (m != r) {
            at = 1;
            for (uint32_t j = 0; j < d; j++) {
                const uint32_t o = unsorted[lo + j];
                at += (o != r && o < m) ? 1u : 0u;
            }
        }
        const uint32_t n = kmers_of(off, m, k);
        out.unitig[lo + at] = m;
        out.kmers[lo + at] = n;
        out.ref[lo + at] = r;
        out.strand[lo + at] = flip[m] != flip[r] ? 1 : 0;
        out.abundance[lo + at] = kc ? kc[m] : n;
    }
}

// ---- alleles ----

// A record of the store read in one orientation (rc: backwards and complemented).
struct Oriented {
    u64 begin, len;
    bool rc;
};
__device__ __forceinline__ uint32_t reverse_bases(uint32_t w) {  // base t <-> base 15 - t
    w = __brev(w);
    return ((w >> 1) & 0x55555555u) | ((w & 0x55555555u) << 1);
}
__device__ __forceinline__ uint32_t store_word(const uint32_t *packed, u64 b) {  // the 16 bases from base b on (one word of overread)
    const u64 w = b >> 4;
    const u64 v = (u64)packed[w] | ((u64)packed[w + 1] << 32);
    return (uint32_t)(v >> (2 * (b & 15)));
}
// the bases [i, i + 16) of the oriented record, i < len; those from len on are undefined
__device__ __forceinline__ uint32_t bases16(const uint32_t *packed, const Oriented &o, u64 i) {
    if (!o.rc) return store_word(packed, o.begin + i);
    const u64 left = o.len - i;
    const uint32_t m = left < 16 ? (uint32_t)left : 16u;  // bases [i, i + m) are the store's [len - i - m, len - i), backwards
    return ~reverse_bases(store_word(packed, o.begin + left - m)) >> (2 * (16 - m));
}
__device__ __forceinline__ uint32_t low_bases(uint32_t x, u64 n) { return n >= 16 ? x : x & ((1u << (2 * n)) - 1u); }

// the longest common prefix of a and b, at most cap (cap <= both lengths); the whole wave calls it with the same arguments
__device__ __forceinline__ u64 common_prefix(const uint32_t *packed, const Oriented &a, const Oriented &b, u64 cap, int lane) {
    for (u64 i0 = 0; i0 < cap; i0 += WAVE * 16) {  // (wave-uniform bounds)
        const u64 i = i0 + (u64)lane * 16;
        uint32_t x = 0;
        if (i < cap) x = low_bases(bases16(packed, a, i) ^ bases16(packed, b, i), cap - i);
        const u64 hit = __ballot(x != 0);
        if (hit) {
            const int first = __ffsll(hit) - 1;
            const uint32_t w = __shfl(x, first, WAVE);
            return i0 + (u64)first * 16 + (uint32_t)(__ffs(w) - 1) / 2;
        }
    }
    return cap;
}

// A wave per arm. Arm 0 of a bubble gets zeros.
__global__ __launch_bounds__(WB) void allele_kernel(const uint32_t *packed, const u64 *off, Arms arms, uint64_t A, uint32_t *prefix, uint32_t *suffix,
                                                    uint32_t *differences) {
    const uint64_t a = hu::gid() / WAVE;
    if (a >= A) return;  // (wave-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t u = arms.unitig[a], r = arms.ref[a];
    u64 p = 0, s = 0;
    uint32_t diff = 0;
    if (u != r) {
        const bool minus = arms.strand[a] != 0;
        const Oriented R{off[r], off[r + 1] - off[r], false}, X{off[u], off[u + 1] - off[u], minus};
        const Oriented Rr{R.begin, R.len, true}, Xr{X.begin, X.len, !minus};
        const u64 shorter = R.len < X.len ? R.len : X.len;
        s = common_prefix(packed, Rr, Xr, shorter, lane);
        p = common_prefix(packed, R, X, shorter - s, lane);
        if (R.len == X.len) {
            const u64 span = R.len - s - p;
            for (u64 i0 = 0; i0 < span; i0 += WAVE * 16) {
                const u64 i = i0 + (u64)lane * 16;
                if (i < span) {
                    uint32_t x = low_bases(bases16(packed, R, p + i) ^ bases16(packed, X, p + i), span - i);
                    x = (x | (x >> 1)) & 0x55555555u;
                    diff += __popc(x);
                }
            }
            for (int d = WAVE / 2; d > 0; d >>= 1) diff += __shfl_down(diff, d, WAVE);
        }
    }
    if (lane == 0) {
        prefix[a] = (uint32_t)p;
        suffix[a] = (uint32_t)s;
        differences[a] = diff;
    }
}

// A wave per arm: lane c counts the arm's k-mers whose mask has bit c. The k-mers of record u lie at off[u] - u (k - 1) in window order.
__global__ __launch_bounds__(WB) void carrier_kernel(const u64 *masks, const u64 *off, uint32_t k, Arms arms, uint64_t A, uint32_t n_colors, uint32_t *carried) {
    const uint64_t a = hu::gid() / WAVE;
    if (a >= A) return;  // (wave-uniform)
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t u = arms.unitig[a], n = arms.kmers[a];
    const u64 *m = masks + (off[u] - (u64)u * (k - 1));
    uint32_t mine = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {
        const u64 v = i0 + lane < n ? m[i0 + lane] : 0ull;
        for (uint32_t c = 0; c < n_colors; c++) {
            const uint32_t have = __popcll(__ballot((v >> c) & 1ull));
            if ((uint32_t)lane == c) mine += have;
        }
    }
    if ((uint32_t)lane < n_colors) carried[a * n_colors + lane] = mine;
}

void need_device(int device_id, const char *who) {
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for %s", device_id, who);
    HIP_CHECK(hipSetDevice(device_id));
}

template <typename T>
T *host_array(uint64_t n) {
    T *p = static_cast<T *>(big_malloc((n + 1) * sizeof(T)));
    if (!p) MTG_DIE("out of memory (%llu arms)", (unsigned long long)n);
    return p;
}

}  // namespace

uint64_t device_unitig_bubbles(const HostGraph &g, const char *seqs, const uint64_t *seq_off, uint64_t n_unitigs, uint64_t k, uint64_t max_arm_kmers,
                               const uint64_t *unitig_kc, const uint64_t *kmer_colors, uint32_t n_colors, int device_id, UnitigBubbleArrays *out,
                               UnitigBubblesTimes *times) {
    if (!g.built) MTG_DIE("mtg_unitig_bubbles: graph is not built");
    const uint64_t E = g.n_original_edges, U = E / 2, V = g.node_count();
    if (E & 1) MTG_DIE("mtg_unitig_bubbles: %llu original edges are not two per unitig", (unsigned long long)E);
    if (U >= (1ull << 31) - 1 || V >= 0xFFFFFFFFull) MTG_DIE("mtg_unitig_bubbles: the graph is too large (%llu unitigs; the limit is 2^31 - 2)", (unsigned long long)U);
    if (k < 1 || k > 0x7FFFFFFFull) MTG_DIE("mtg_unitig_bubbles: k = %llu is out of range", (unsigned long long)k);
    if (n_unitigs != U) MTG_DIE("mtg_unitig_bubbles: %llu sequences for a graph of %llu unitigs", (unsigned long long)n_unitigs, (unsigned long long)U);
    if (kmer_colors && (n_colors < 1 || n_colors > 64)) MTG_DIE("mtg_unitig_bubbles: n_colors = %u is not in 1..64", n_colors);
    if (seq_off[0] != 0) MTG_DIE("mtg_unitig_bubbles: the sequence offsets must start at 0");
    for (uint64_t u = 0; u < U; u++)
        if (seq_off[u + 1] < seq_off[u] + k) MTG_DIE("mtg_unitig_bubbles: unitig %llu is shorter than k = %llu", (unsigned long long)u, (unsigned long long)k);
    need_device(device_id, "the unitig bubbles");
    device_arena_reset_peak(device_id);
    const uint64_t L = max_arm_kmers < (1ull << 31) ? max_arm_kmers : (1ull << 31);  // an arm has fewer than 2^31 k-mers
    const bool colours = kmer_colors != nullptr;
    hipStream_t st = nullptr;
    UnitigBubblesTimes t;
    uint64_t B = 0, A = 0;
    *out = UnitigBubbleArrays();
    if (U && L > 1) {
        SeqStore seq("unitig sequences", seqs, seq_off, U, st, device_id);
        const uint64_t n_kmers = seq.n_bases - U * (k - 1);
        const auto t0 = std::chrono::steady_clock::now();
        hu::DeviceArray<uint32_t> from(E), to(E), mirror(V + 1);
        hu::DeviceArray<u64> d_kc, d_masks;
        hu::upload_sliced(from, g.e_from.data(), E * 4, st, device_id);
        hu::upload_sliced(to, g.e_to.data(), E * 4, st, device_id);
        hu::upload_sliced(mirror, g.mirror.data(), V * 4, st, device_id);
        if (unitig_kc) {
            d_kc.alloc(U);
            hu::upload_sliced(d_kc, unitig_kc, U * 8, st, device_id);
        }
        if (colours) {
            d_masks.alloc(n_kmers + 1);
            hu::upload_sliced(d_masks, kmer_colors, n_kmers * 8, st, device_id);
        }
        t.upload_ms = seq.upload_ms + ms_since(t0);
        const uint64_t slots = 2 * U + 2;
        hu::DeviceArray<u64> key(U), t_key(slots), base(U + 1);
        hu::DeviceArray<uint8_t> flip(U);
        hu::DeviceArray<uint32_t> t32(3 * slots), slot_of(U), flag(U + 1), arms_of(U + 1), cursor(slots);
        hu::ScanScratch<uint32_t> scan32(U + 1);
        hu::ScanScratch<u64> scan64(U + 1);
        const Table tab{t_key.get(), t32.get(), t32.get() + slots, t32.get() + 2 * slots, slots};
        const u64 *kc = unitig_kc ? d_kc.get() : nullptr;
        PhaseEvents<4> ev;  // 0 keys, group, number 1 alleles 2 carriers 3
        ev.mark(0, st);
        HIP_CHECK(hipMemsetAsync(t_key, 0xFF, slots * 8, st));
        HIP_CHECK(hipMemsetAsync(tab.count, 0, slots * 4, st));
        HIP_CHECK(hipMemsetAsync(tab.least, 0xFF, 2 * slots * 4, st));  // (least and best)
        HIP_CHECK(hipMemsetAsync(cursor, 0, slots * 4, st));
        keys_kernel<<<hu::grid_for(U), hu::EB, 0, st>>>(from, to, mirror, seq.off, U, V, (uint32_t)k, L, key, flip, stage_err(seq.small));
        group_kernel<<<hu::grid_for(U), hu::EB, 0, st>>>(key, kc, seq.off, U, (uint32_t)k, tab, slot_of, stage_err(seq.small));
        flag_kernel<<<hu::grid_for(U + 1), hu::EB, 0, st>>>(slot_of, tab, U, flag, arms_of);
        scan32.scan(st, flag, U + 1, flag.get());
        scan64.scan(st, arms_of, U + 1, base.get());
        HIP_CHECK(hipGetLastError());
        uint32_t n_bubbles = 0;
        u64 n_arms = 0;
        HIP_CHECK(hipMemcpyAsync(&n_bubbles, scan32.total(), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(&n_arms, scan64.total(), 8, hipMemcpyDeviceToHost, st));
        seq.small.read(st, "unitig bubbles");
        if (seq.small.h[2] & ERR_NODE_RANGE) MTG_DIE("unitig bubbles: an edge names a node outside the graph");
        if (seq.small.h[2] & ERR_TABLE) MTG_DIE("unitig bubbles: internal error (the key table is full)");
        B = n_bubbles; A = n_arms;
        hu::DeviceArray<u64> arm_off(B + 1), abundance(A + 1);
        hu::DeviceArray<uint32_t> slot_of_bubble(B + 1), unsorted(A + 1), a32(6 * (A + 1)), carried;
        hu::DeviceArray<uint8_t> strand(A + 1);
        uint32_t *prefix = a32.get() + 3 * (A + 1), *suffix = a32.get() + 4 * (A + 1), *differences = a32.get() + 5 * (A + 1);
        const Arms ordered{a32.get(), a32.get() + (A + 1), a32.get() + 2 * (A + 1), strand.get(), abundance.get()};
        scatter_kernel<<<hu::grid_for(U + 1), hu::EB, 0, st>>>(slot_of, tab, U, flag, base, B, A, arm_off, slot_of_bubble, cursor, unsorted);
        if (B) order_kernel<<<hu::grid_for(B * WAVE, WB), WB, 0, st>>>(arm_off, slot_of_bubble, tab, unsorted, flip, kc, seq.off, (uint32_t)k, B, ordered);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        if (A) allele_kernel<<<hu::grid_for(A * WAVE, WB), WB, 0, st>>>(seq.packed, seq.off, ordered, A, prefix, suffix, differences);
        HIP_CHECK(hipGetLastError());
        ev.mark(2, st);
        if (colours) {
            carried.alloc(A * n_colors + 1);
            if (A) carrier_kernel<<<hu::grid_for(A * WAVE, WB), WB, 0, st>>>(d_masks, seq.off, (uint32_t)k, ordered, A, n_colors, carried);
            HIP_CHECK(hipGetLastError());
        }
        ev.mark(3, st);
        HIP_CHECK(hipStreamSynchronize(st));
        t.group_ms = ev.ms(0, 1); t.allele_ms = ev.ms(1, 2); t.carrier_ms = ev.ms(2, 3);
        const auto td = std::chrono::steady_clock::now();
        out->arm_off = host_array<uint64_t>(B + 1);
        out->arm_unitig = host_array<uint32_t>(A); out->arm_strand = host_array<uint8_t>(A); out->arm_kmers = host_array<uint32_t>(A);
        out->arm_abundance = host_array<uint64_t>(A);
        out->prefix = host_array<uint32_t>(A); out->suffix = host_array<uint32_t>(A); out->differences = host_array<uint32_t>(A);
        hu::download_sliced(out->arm_off, arm_off.get(), (B + 1) * 8, st, device_id);
        hu::download_sliced(out->arm_unitig, ordered.unitig, A * 4, st, device_id);
        hu::download_sliced(out->arm_strand, ordered.strand, A, st, device_id);
        hu::download_sliced(out->arm_kmers, ordered.kmers, A * 4, st, device_id);
        hu::download_sliced(out->arm_abundance, ordered.abundance, A * 8, st, device_id);
        hu::download_sliced(out->prefix, prefix, A * 4, st, device_id);
        hu::download_sliced(out->suffix, suffix, A * 4, st, device_id);
        hu::download_sliced(out->differences, differences, A * 4, st, device_id);
        if (colours) {
            out->carried = host_array<uint32_t>(A * n_colors);
            hu::download_sliced(out->carried, carried.get(), A * n_colors * 4, st, device_id);
        }
        t.download_ms = ms_since(td);
    } else {  // nothing can be an arm
        out->arm_off = host_array<uint64_t>(1);
        out->arm_off[0] = 0;
        out->arm_unitig = host_array<uint32_t>(0); out->arm_strand = host_array<uint8_t>(0); out->arm_kmers = host_array<uint32_t>(0);
        out->arm_abundance = host_array<uint64_t>(0);
        out->prefix = host_array<uint32_t>(0); out->suffix = host_array<uint32_t>(0); out->differences = host_array<uint32_t>(0);
        if (colours) out->carried = host_array<uint32_t>(0);
    }
    t.bubbles = B; t.arms = A;
    uint64_t arena[4];
    device_arena_stats(device_id, arena);
    t.peak_arena_bytes = arena[2];
    if (times) *times = t;
    return B;
}

}  // namespace mtg
