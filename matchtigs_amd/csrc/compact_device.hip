// compact_device.hip -- the maximal unitigs of the k-mer set of arbitrary sequences (`--seq-in`, mtg_compact_unitigs)
//
// The contract (stated in full in DESIGN.md 16). Input: concatenated ASCII plus n + 1 offsets, either case; a window is a start
// position whose k bases lie inside one record; S is the set of canonical k-mers of all windows. creator(x) is the smallest window
// start whose k-mer is x or rc(x), reading(x) the string there. G(S) is the bigraph mtg_graph_from_sequences builds from the readings:
// nodes are oriented (k-1)-mers, every k-mer is the edge P -> S and its mirror. A node is PASSABLE iff it is not its own mirror and
// has in-degree 1 and out-degree 1 over all directed edges. A unitig is a maximal walk whose inner nodes are passable (closed when
// the node between its last and first edge is passable too); its leader is the k-mer with the smallest creator; of the walk and its
// mirror the one that holds reading(leader) is emitted, a closed walk from its leader on, in increasing order of the leaders'
// creators, spelled as the first edge's k bases plus the last base of every further edge.
//
// Kernels, on one stream:
//   pack      ASCII -> 2 bits per base (SeqStore, pack_device.hpp), which also finds the first character outside ACGT
//   insert    every window (kw::for_each_window) into a table of classes (kw::find_slot in kmer_window_device.hpp, where the
//             exactness and order-independence argument of both tables here is written down): slot = kw::tagged_pos of a window
//             start, identity by kw::same_class for every k. A slot of the same class takes atomicMin: the tag is fixed per class,
//             so the slot ends holding the class's creator.
//   ids       the creators' positions are flagged from the table's slots and scanned: dense k-mer ids in creator order, so "smallest
//             creator" is "smallest id"; kpos[id] = creator. The table is freed. Oriented k-mer 2 i is reading(i), 2 i + 1 its mirror.
//   nodes     a table of (k-1)-mer classes fed by two insertions per distinct k-mer (prefix and suffix). Per class and side (edges
//             that leave / enter the class's canonical orientation) one word: none, the one incident oriented k-mer, or "several".
//             Key: kw::class_key (the canonical 2-bit code for k - 1 <= 32, else tagged_pos with same_class over k - 1 bases).
//   succ      per distinct k-mer two lookups: succ[o] = the one edge that leaves the head node of o if that node is passable, else
//             none. pred(o) = mirror(succ(mirror(o))), so one array serves both directions.
//   rank      pointer jumping over (jump, rank) pairs held in one 64-bit word, updated in place: a pair always says "jump is the
//             rank-th predecessor", so any interleaving of the threads keeps it true, and the final state (jump = the walk's head,
//             rank = the distance from it) is unique. A round at least doubles every open distance: ceil(log2(longest walk)) + 1
//             rounds. What still moves after ceil(log2(2 N)) + 2 rounds lies on a closed walk; those elements are listed, the
//             minimum oriented id of each cycle is found by doubling windows (ping-pong buffers), the cycle is cut in front of that
//             element and ranked like a chain. No kernel walks a chain sequentially.
//   emit      per walk the minimum oriented id (atomicMin at the head, one per wave where a wave lies on one walk) and the length
//             (written by the tail); a walk is emitted iff that minimum is even (it holds the reading of its leader). Leaders'
//             lengths are scanned in id order -> unitig numbers and character offsets; every oriented k-mer of an emitted walk writes
//             its last base at offset + rank + k - 1, the head the first k - 1 bases too.
// Nothing depends on the order in which atomics land: the k-mer slots end holding class minima, the node words depend only on
// the multiset of insertions, the (jump, rank) fixpoint is unique, and the rest are minima, sums and scans.
//
// Limits: fewer than 2^40 - 1 bases, fewer than 2^31 - 1 distinct k-mers (oriented k-mer ids are 32-bit), 2 <= k < 2^31.
// Device memory (arena, hip_util.hpp) per input base b, window w, distinct k-mer N: pack 1.25 b; insert 0.25 b + 16 w + 4 b;
// later 0.25 b + N (8 kpos + 32 + 16 node table + 8 succ + 16 pairs [+ 16 + 8 with closed walks] + 8 wmin/wlen + 16 leaders).
// There is no host path: without a GPU a non-empty call aborts.
//
// Counted calls (mtg_compact_unitigs_counted): abundance(x) = the windows whose k-mer is x or rc(x); the contract above
// is applied to S_m = { x : abundance(x) >= m }, creators and readings still taken over ALL windows. insert<COUNTED> adds 1 to
// count[slot] for every window behind the slot find_slot returns (a claimed slot keeps its class: the sum per slot is the class's
// abundance in any order); one sweep of count[] gives the spectrum (256 bins in LDS per workgroup, then at most one global atomicAdd
// per non-empty bin and workgroup), the largest abundance and the kept occurrences; mark<COUNTED> flags a creator only where count >= m
// and kpos<COUNTED> carries kcount[id] = count[slot]; from there N = |S_m| and nodes, succ, rank and emit run unchanged. Per-unitig
// sums: every kept k-mer writes its count at its place in unitig order (k-mer offset of its unitig + rank), one scan to 64 bits, and
// differences at the unitig boundaries -- no atomic at all. Fewer than 2^32 windows (32-bit counters cannot wrap).
// Memory added by a counted call: 4 B per slot (8 w) while inserting, freed with the table; 4 N (kcount) afterwards; 12 N + 8 per
// unitig for the sums at the end of emit. A call that hands out the count of every kept k-mer (mtg_compact_unitigs_counted_kmers,
// DESIGN.md 20) downloads that array in unitig order, which is the store's window order, instead of freeing it after the scan.
//
// Coloured calls (mtg_compact_unitigs_colored): every record has a colour below C <= 64; colors(x) = the 64-bit mask of the
// colours of the windows whose k-mer is x or rc(x). It is a counted call that hands out the counts, plus: insert<COLORED> ORs the
// record's bit into colors[slot] (a plain read first, atomicOr only where the bit is missing: bits only appear, so a stale read costs
// one redundant atomic; the final word is an OR over the class's windows in any order); kpos<COLORED> carries kcolor[id] = colors[slot];
// color_stats_kernel sweeps kcolor[N] once for per-colour counts, the C x C matrix of shared k-mers and the occupancy histogram, as a
// product of 64 x 64 bit blocks (ballots, popcounts), never a loop over set bits; order_kernel<uint64_t> puts the masks into unitig
// order, which is downloaded. Memory added: 8 B per slot (16 w) while inserting, freed with the table; 8 N (kcolor) and 8 N (ordered).
//
// Calls with colour classes (mtg_compact_unitigs_colored_classes): a coloured call plus the dictionary of the ordered
// masks (the kernels under "colour classes" below: per run of equal masks, never per k-mer), and with split = 1 succ_kernel<true>,
// which keeps a successor only where both k-mers have one mask, so that every unitig is monochromatic; rank, emit, sums, counts and
// ordered masks follow from succ unchanged. Memory added after emit: 12 N + 48 per run + 32 per class.
//
// Cleaned calls (mtg_compact_unitigs_cleaned): tips and isolated unitigs leave the k-mer set T (at first S_m) in rounds
// before the final pass. A round is nodes, succ<false> (decisions are taken on unsplit unitigs) and rank over the N k-mers of T, then
// clean_decide_kernel: the thread of every oriented k-mer without a successor -- the last edge of an open walk; cut cycles have none
// -- reads the walk's length from its rank, looks up the node classes of the walk's two ends (find_node<false>; the node table
// stays alive through rank for this), derives free / anchored / through from the two "none / one / several" words, and writes the
// verdict at the walk's first element; the mirror walk's thread derives the same verdict for its own first element, so every word
// has one writer. clean_keep_kernel turns verdicts into a keep flag per k-mer, the scan of the flags gives the new dense ids (creator
// order is kept: "smallest id" stays "smallest creator"), clean_move_kernel carries kpos, kcount and kcolor over, and the next pass
// runs over N' <= N. The counters of a round are reduced per block; a block issues at most one global atomic per counter. The
// rounds end when one removes nothing (its succ and ranks are then the final ones, unless the unitigs are to be split: succ<true>
// and rank run once more on the same node table) or when the last allowed round has removed something (then one more pass runs
// over the survivors). emit and everything behind it see the final set only. With no length given the call runs the kernels of
// its rung and nothing else. Memory added per round: the node table with its words (64 N) lives on beside the pairs (16 N) instead
// of being freed in front of rank; 2 N verdict bytes, 4 N keep flags; then, with table, succ and pairs freed, 4 N new ids and the
// second copy of kpos / kcount / kcolor (8 + 4 + 8 B per survivor).
//
// Simplified calls (mtg_compact_unitigs_simplified): a round also pops the weaker arms of simple bubbles, between
// clean_decide_kernel and clean_keep_kernel and on the same snapshot. An arm is an open walk of fewer than L_bub k-mers from its tail
// node u to its head node v (no self-mirror end, u != v, u != rc(v)); the arms with one (u, v) form a bundle, the mirror counting
// once; the best arm has the largest mean abundance (sum_a n_b > sum_b n_a), then the smallest end k-mer id; another arm a goes iff
// sum_B n_a >= R sum_a n_B. bubble_flag_kernel: the threads of clean_decide_kernel's entry condition whose walk is short flag the smaller
// of the walk pair's two first elements; the scan numbers the M list slots. bubble_list_kernel: two find_node<false> probes per short
// walk end give the oriented node ids (2 slot + orientation: 34 bits each, so a key is two 64-bit words), and the thread with the
// smaller of the two mirror keys fills the slot. bubble_counts_kernel: every k-mer of an arm writes its count at the arm's offset (the
// scan of the lengths) + its rank -- no thread walks an arm --, a 64-bit scan and bubble_sums_kernel give the sums by differences.
// bubble_choose_kernel: open addressing over 2 M 32-bit table slots, a CAS loop that replaces a key's arm only by a better one, so the
// table ends at the maxima. bubble_verdict_kernel: every arm that is not its key's best and passes the ratio test (right side in 128
// bits) writes VERDICT_BUBBLE at its own first element and its mirror's, and counts itself once. clean_keep_kernel<true> counts arm
// k-mers and occurrences apart. With max_arm_kmers 0 none of this runs and clean_keep_kernel<false> is the cleaned call's kernel.
// Memory added while a round pops: 8 N (flags / list slots per oriented k-mer), 44 B per list slot (36 entry + 8 table), 12 B per
// k-mer of a candidate arm (4 ordered count + 8 prefix); all freed before the keep flags are scanned.
//
// Selected calls (mtg_compact_unitigs_selected): of S_m only the k-mers that pass five rules, in this order and each
// counted under the first it fails, reach nodes, succ and everything behind them: forbid (colors & forbid == 0), require (colors &
// require == require), carriers (min <= popcount(colors) <= max), subtract (sub < A) and intersect (int >= B), where sub(x) / int(x) =
// the windows of the subtract / intersect records of a second store, the FILTER records, whose k-mer is x or rc(x). The filter store is
// packed on its own and only looked up: filter_probe_kernel runs between insert and ids, while the table lives, one thread per RUN
// window starts of the filter store, find_slot<false> with the two-store same_class behind the tag (as exact as the insertion for
// every k), and a hit adds 1 to sub[slot] or inter[slot] by the role of its record; a filter window claims no slot, so it creates,
// counts and colours nothing. kpos_filter_kernel carries the two counters to dense arrays over S_m beside kcount and kcolor.
// In front of the first pass, over the ids of S_m: color_stats_kernel (a selected call's colour statistics are those of S_m: they are
// how a carrier threshold is chosen), then select_keep_kernel, which writes the keep flag and reduces the five rejection counts, the
// selected k-mers, their occurrences and the per-colour selected counts (ballots and popcounts, never a loop over set bits) per
// block; the scan of the flags and clean_move_kernel carry kpos, kcount and kcolor to the new ids in creator order, exactly as a
// cleaning round's move does, and pass, clean_rounds, emit, sums_and_colors and download run over S_sel unchanged. Sums and flags:
// nothing depends on how the atomics land. Memory added: 0.25 B per filter base (plus 1 B per base while it is packed) and 4 B per
// slot and role while the table lives, all back before ids ends; 4 N per role until the keep kernel has run; then the move's 4 N
// keep flags, 4 N new ids and second copy of kpos / kcount / kcolor. The probe is booked under filter_ms (ids_ms leaves it out),
// the keep kernel, the scan and the move under select_ms. Fewer than 2^32 filter windows per role, fewer than 2^40 - 1 filter bases.
// A call without a Selected queues exactly the kernels it queued before there was one.
//
// All of these enter through device_compact_unitigs(CompactRequest) (device.hpp): one rung of the ladder per pointer of the request --
// Counted, Colored, Classed --, null where the call does not climb that far; Cleaned stands beside the ladder and goes with any rung,
// Bubbled beside a Cleaned and a Counted, Selected beside any rung from Counted on (and a Colored where a colour rule is set). On the host a call is check_request (no device call), then run() over a Work (the store, the
// current k-mer set, its node table, succ, pairs) through one function per stage -- insert, filter_probe, ids, select, pass (build_nodes,
// succ, rank with rank_closed_walks), clean_rounds (clean_round, move_survivors), emit, sums_and_colors, download --, then finish(), the one way
// out. Every device array belongs to a hu::DeviceArray and goes back where its owner's scope ends; every scan's block sums and
// total belong to a hu::ScanScratch, which checks that a scan fits it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"

namespace mtg {

namespace {

using kw::POS_LIMIT;
using kw::RUN;
using kw::EMPTY_SLOT;
constexpr uint32_t NONE32 = 0xFFFFFFFFu;   // no incident edge / no successor
constexpr uint32_t MULTI32 = 0xFFFFFFFEu;  // two or more incident edges
constexpr uint64_t MAX_KMERS = 0x7FFFFFFEull;

struct KmerArgs : kw::WindowArgs {
    unsigned long long *table;  // [slots] kw::tagged_pos of the class's creator
    uint64_t slots;
};

__device__ __forceinline__ uint64_t pair_of(uint32_t jump, uint32_t rank) { return ((uint64_t)rank << 32) | jump; }
__device__ __forceinline__ uint64_t load64(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store64(unsigned long long *p, uint64_t v) { __hip_atomic_store(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// COUNTED: count[slot] += 1 per window (the class's abundance once the kernel has finished)
// COLORED: colors[slot] |= 1 << record_colors[record of the window] (record_colors: [n_rec], each < 64; colors: [slots], zeroed). The
// record's colour is read again only where the record changes inside the thread's run.
template <bool WIDE, bool COUNTED, bool COLORED>
__global__ __launch_bounds__(hu::EB) void insert_kernel(KmerArgs a, uint64_t n_bases, uint64_t n_rec, unsigned int *err, uint32_t *count,
                                                         const uint8_t *record_colors, unsigned long long *colors) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    uint64_t bit_rec = ~0ull;
    unsigned long long bit = 0;
    kw::for_each_window<WIDE>(a, p0, p0 + RUN < n_bases ? p0 + RUN : n_bases, 0, n_rec, [&](uint64_t q, uint64_t r, const kw::Window &w) {
        const unsigned long long mine = kw::tagged_pos(w.hash, q);
        const kw::Found f = kw::find_slot<true>(a.table, a.slots, w.hash, mine, [&](unsigned long long cur) {
            return (cur >> 40) == (mine >> 40) && kw::same_class(a.packed, q, cur & POS_LIMIT, a.k);
        });
        if (f.slot == a.slots) {
            atomicOr(err, 1u);  // (2 slots per window: never full)
            return;
        }
        if (f.word != EMPTY_SLOT && mine < f.word) atomicMin(&a.table[f.slot], mine);
        if (COUNTED) atomicAdd(&count[f.slot], 1u);
        if (COLORED) {
            if (r != bit_rec) {
                bit_rec = r;
                bit = 1ull << record_colors[r];
            }
            if (!(colors[f.slot] & bit)) atomicOr(&colors[f.slot], bit);
        }
    });
}

// flag[creator] = 1 for every occupied slot; *count += occupied slots (grid-stride: one atomic per wave of the whole grid)
// COUNTED: only the slots whose class has abundance >= m
template <bool COUNTED>
__global__ __launch_bounds__(hu::EB) void mark_kernel(const unsigned long long *table, uint64_t slots, uint32_t *flag, unsigned long long *count,
                                                       const uint32_t *abundance, uint64_t m) {
    unsigned long long n = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = hu::gid(); s < slots; s += stride) {
        const unsigned long long cur = table[s];
        if (cur == EMPTY_SLOT) continue;
        if (COUNTED && abundance[s] < m) continue;
        flag[cur & POS_LIMIT] = 1u;
        n++;
    }
    for (int d = warpSize / 2; d > 0; d /= 2) n += __shfl_down(n, d);
    if (n && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(count, n);
}
// COUNTED: kcount[id] = the abundance of k-mer id; COLORED (counted calls): kcolor[id] = its colour mask
template <bool COUNTED, bool COLORED>
__global__ __launch_bounds__(hu::EB) void kpos_kernel(const unsigned long long *table, uint64_t slots, const uint32_t *id_of_pos, unsigned long long *kpos,
                                                       const uint32_t *abundance, uint64_t m, uint32_t *kcount, const unsigned long long *colors,
                                                       unsigned long long *kcolor) {
    const uint64_t s = hu::gid();
    if (s >= slots) return;
    const unsigned long long cur = table[s];
    if (cur == EMPTY_SLOT) return;
    if (!COUNTED) {
        kpos[id_of_pos[cur & POS_LIMIT]] = cur & POS_LIMIT;
    } else if (abundance[s] >= m) {
        const uint32_t id = id_of_pos[cur & POS_LIMIT];
        kpos[id] = cur & POS_LIMIT;
        kcount[id] = abundance[s];
        if (COLORED) kcolor[id] = colors[s];
    }
}

// One sweep over the abundances of the table's slots (0 = empty). out[0 .. 256): the spectrum, bin min(c, 255); out[256] = the largest
// abundance; out[257] = the sum of the abundances >= m. A workgroup counts into 256 bins in LDS and then issues at most one global
// atomicAdd per non-empty bin; the maximum and the sum are reduced per wave, then per workgroup, and cost one atomic each.
constexpr int SPECTRUM_BINS = 256;
__global__ __launch_bounds__(hu::EB) void spectrum_kernel(const uint32_t *abundance, uint64_t slots, uint64_t m, unsigned long long *out) {
    __shared__ uint32_t bins[SPECTRUM_BINS];  // (a workgroup sweeps fewer than 2^32 slots)
    __shared__ unsigned long long wave_sum[hu::EB / 64];
    __shared__ uint32_t wave_max[hu::EB / 64];
    static_assert(hu::EB == SPECTRUM_BINS, "one thread per bin");
    bins[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long sum = 0;
    uint32_t top = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = hu::gid(); s < slots; s += stride) {
        const uint32_t c = abundance[s];
        if (!c) continue;
        atomicAdd(&bins[c < SPECTRUM_BINS - 1 ? c : SPECTRUM_BINS - 1], 1u);
        top = c > top ? c : top;
        if (c >= m) sum += c;
    }
    for (int d = warpSize / 2; d > 0; d /= 2) {
        sum += __shfl_down(sum, d);
        const uint32_t o = __shfl_down(top, d);
        top = o > top ? o : top;
    }
    const int lane = threadIdx.x & (warpSize - 1), wave = threadIdx.x / warpSize;
    if (lane == 0) {
        wave_sum[wave] = sum;
        wave_max[wave] = top;
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
    if (threadIdx.x == 0) {
        for (int w = 1; w < hu::EB / warpSize; w++) {
            sum += wave_sum[w];
            top = wave_max[w] > top ? wave_max[w] : top;
        }
        if (sum) atomicAdd(&out[SPECTRUM_BINS + 1], sum);
        if (top) atomicMax(&out[SPECTRUM_BINS], (unsigned long long)top);
    }
}

// One sweep over the colour masks of the kept k-mers. out[i * 64 + j], i, j < C: the k-mers whose mask has bits i and
// j (the diagonal: bit i); out[COLOR_OCC + n], n <= 64: the k-mers with n bits set. A wave takes 64 masks at a time, one per lane (0
// behind N): T_i = the ballot of bit i is column i of that 64 x 64 bit block, kept by lane i, and lane i adds popcount(T_i & T_j) for
// every j < C to its accumulator j, T_j coming from lane j by readlane -- C ballots and C (readlane, and, popcount, add) per block
// whatever the masks hold. The accumulators (fewer than 2^31 k-mers: they cannot wrap) stay in registers over all blocks of the wave,
// are then added up per workgroup in LDS and leave by at most one global atomicAdd per non-zero entry and workgroup.
constexpr int MAX_COLORS = 64, COLOR_OCC = MAX_COLORS * MAX_COLORS, COLOR_STATS_WORDS = COLOR_OCC + MAX_COLORS + 1;
__global__ __launch_bounds__(hu::EB) void color_stats_kernel(const unsigned long long *kcolor, uint64_t N, int C, unsigned long long *out) {
    __shared__ uint32_t mat[COLOR_OCC];
    __shared__ uint32_t occ[MAX_COLORS + 1];
    for (int e = threadIdx.x; e < COLOR_OCC; e += hu::EB) mat[e] = 0;
    if (threadIdx.x <= MAX_COLORS) occ[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    uint32_t acc[MAX_COLORS];
#pragma unroll
    for (int j = 0; j < MAX_COLORS; j++) acc[j] = 0;
    const uint64_t stride = (uint64_t)gridDim.x * hu::EB;  // (a multiple of 64: the lanes of a wave leave the loop together)
    for (uint64_t at = hu::gid() - lane; at < N; at += stride) {
        const bool live = at + lane < N;
        const unsigned long long mask = live ? kcolor[at + lane] : 0ull;
        if (live) atomicAdd(&occ[__popcll(mask)], 1u);
        unsigned long long mine = 0;
        for (int i = 0; i < C; i++) {
            const unsigned long long t = __ballot((mask >> i) & 1);
            mine = lane == i ? t : mine;
        }
        const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
#pragma unroll
        for (int j = 0; j < MAX_COLORS; j++) {
            if (j < C) {  // (uniform)
                const uint32_t tl = __builtin_amdgcn_readlane(lo, j), th = __builtin_amdgcn_readlane(hi, j);
                acc[j] += __popc(lo & tl) + __popc(hi & th);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MAX_COLORS; j++)
        if (j < C && acc[j]) atomicAdd(&mat[j * MAX_COLORS + lane], acc[j]);  // (entry (j, lane) of a symmetric matrix: one bank per lane)
    __syncthreads();
    for (int e = threadIdx.x; e < COLOR_OCC; e += hu::EB)
        if (mat[e]) atomicAdd(&out[e], (unsigned long long)mat[e]);
    if (threadIdx.x <= MAX_COLORS && occ[threadIdx.x]) atomicAdd(&out[COLOR_OCC + threadIdx.x], (unsigned long long)occ[threadIdx.x]);
}

struct NodeArgs {
    const uint32_t *packed;
    const unsigned long long *kpos;  // [N]
    unsigned long long *table;       // [slots]
    uint32_t *out_e, *in_e;          // [slots] the edge that leaves / enters the canonical orientation of the slot's class
    uint32_t *succ;                  // [2 N]
    uint64_t slots, N, L;            // L = k - 1
};

// The slot of the (k-1)-mer at pos (INSERT: claimed if absent) and its key (flip, pal).
template <bool INSERT>
__device__ __forceinline__ uint64_t find_node(const NodeArgs &a, uint64_t pos, kw::ClassKey &key, unsigned int *err) {
    key = kw::class_key(a.packed, pos, a.L);
    const kw::Found f = kw::find_slot<INSERT>(a.table, a.slots, key.hash, key.ident, [&](unsigned long long cur) {
        return a.L <= 32 ? cur == key.ident : ((cur >> 40) == (key.ident >> 40) && kw::same_class(a.packed, pos, cur & POS_LIMIT, a.L));
    });
    if (f.slot < a.slots) return f.slot;
    atomicOr(err, INSERT ? 4u : 8u);
    return 0;
}
// none -> o -> several
__device__ __forceinline__ void add_incident(uint32_t *word, uint32_t o) {
    const uint32_t prev = atomicCAS(word, NONE32, o);
    if (prev != NONE32 && prev != MULTI32) atomicExch(word, MULTI32);
}

__global__ __launch_bounds__(hu::EB) void node_insert_kernel(NodeArgs a, unsigned int *err) {
    const uint64_t i = hu::gid();
    if (i >= a.N) return;
    const uint64_t p = a.kpos[i];
    const uint32_t fw = (uint32_t)(2 * i), mi = fw + 1;
    kw::ClassKey key;
    const uint64_t sa = find_node<true>(a, p, key, err);  // the reading leaves its prefix; its mirror enters the prefix's mirror
    if (!key.flip) add_incident(&a.out_e[sa], fw);
    else add_incident(&a.in_e[sa], mi);
    const uint64_t sb = find_node<true>(a, p + 1, key, err);  // the reading enters its suffix; its mirror leaves the suffix's mirror
    if (!key.flip) add_incident(&a.in_e[sb], fw);
    else add_incident(&a.out_e[sb], mi);
}

// SPLIT: a successor is kept only where its k-mer has the mask of this one (kcolor: [N]) -- the node between them is
// passable only if the k-mer that enters it and the one that leaves it have equal masks. Masks belong to canonical k-mers, so the
// rule holds for the mirror walk too and pred(o) = mirror(succ(mirror(o))) stays true.
template <bool SPLIT>
__global__ __launch_bounds__(hu::EB) void succ_kernel(NodeArgs a, unsigned int *err, const unsigned long long *kcolor) {
    const uint64_t i = hu::gid();
    if (i >= a.N) return;
    const uint64_t p = a.kpos[i];
    kw::ClassKey key;
    const uint64_t sb = find_node<false>(a, p + 1, key, err);  // head of the reading: its suffix as read
    uint32_t oe = a.out_e[sb], ie = a.in_e[sb];
    uint32_t s = (!key.pal && oe < MULTI32 && ie < MULTI32) ? (key.flip ? ie ^ 1u : oe) : NONE32;
    if (SPLIT && s != NONE32 && kcolor[s >> 1] != kcolor[i]) s = NONE32;
    a.succ[2 * i] = s;
    const uint64_t sa = find_node<false>(a, p, key, err);  // head of the mirror: the reverse complement of the prefix
    oe = a.out_e[sa];
    ie = a.in_e[sa];
    s = (!key.pal && oe < MULTI32 && ie < MULTI32) ? (key.flip ? oe : ie ^ 1u) : NONE32;
    if (SPLIT && s != NONE32 && kcolor[s >> 1] != kcolor[i]) s = NONE32;
    a.succ[2 * i + 1] = s;
}

__device__ __forceinline__ uint32_t pred_of(const uint32_t *succ, uint32_t o) {
    const uint32_t s = succ[o ^ 1u];
    return s == NONE32 ? NONE32 : s ^ 1u;
}

__global__ __launch_bounds__(hu::EB) void rank_init_kernel(const uint32_t *succ, uint64_t n, unsigned long long *pairs) {
    const uint64_t o = hu::gid();
    if (o >= n) return;
    const uint32_t pr = pred_of(succ, (uint32_t)o);
    pairs[o] = pair_of(pr, pr != NONE32);
}
// one round of pointer jumping over all n elements, or over those of `list`; stops in front of the head: jump ends as the head itself
__global__ __launch_bounds__(hu::EB) void jump_kernel(unsigned long long *pairs, uint64_t n, const uint32_t *list, unsigned int *changed) {
    const uint64_t g = hu::gid();
    if (g >= n) return;
    const uint64_t o = list ? list[g] : g;
    const uint64_t mine = load64(&pairs[o]);
    const uint32_t j = (uint32_t)mine;
    if (j == NONE32) return;
    const uint64_t theirs = load64(&pairs[j]);
    if ((uint32_t)theirs == NONE32) return;
    store64(&pairs[o], pair_of((uint32_t)theirs, (uint32_t)(mine >> 32) + (uint32_t)(theirs >> 32)));
    *changed = 1u;
}
// the elements that still move after every chain has settled: jump is not a head
__global__ __launch_bounds__(hu::EB) void cycle_list_kernel(const unsigned long long *pairs, const uint32_t *succ, uint64_t n, uint32_t *list,
                                                             unsigned long long *count) {
    const uint64_t o = hu::gid();
    if (o >= n) return;
    const uint32_t j = (uint32_t)pairs[o];
    if (j != NONE32 && succ[j ^ 1u] != NONE32) list[atomicAdd(count, 1ull)] = (uint32_t)o;
}
__global__ __launch_bounds__(hu::EB) void cycle_min_init_kernel(const uint32_t *succ, const uint32_t *list, uint64_t n, unsigned long long *buf) {
    const uint64_t g = hu::gid();
    if (g >= n) return;
    const uint32_t o = list[g];
    buf[o] = pair_of(pred_of(succ, o), o);  // (jump, minimum over the window that ends at o)
}
__global__ __launch_bounds__(hu::EB) void cycle_min_kernel(const unsigned long long *src, unsigned long long *dst, const uint32_t *list, uint64_t n) {
    const uint64_t g = hu::gid();
    if (g >= n) return;
    const uint32_t o = list[g];
    const uint64_t mine = src[o], theirs = src[(uint32_t)mine];
    dst[o] = pair_of((uint32_t)theirs, min((uint32_t)(mine >> 32), (uint32_t)(theirs >> 32)));
}
// cut every cycle in front of its minimum: that element becomes a head
__global__ __launch_bounds__(hu::EB) void cycle_cut_kernel(const unsigned long long *mins, const uint32_t *succ, const uint32_t *list, uint64_t n,
                                                            unsigned long long *pairs) {
    const uint64_t g = hu::gid();
    if (g >= n) return;
    const uint32_t o = list[g];
    const uint32_t m = (uint32_t)(mins[o] >> 32);
    const uint32_t pr = o == m ? NONE32 : pred_of(succ, o);
    pairs[o] = pair_of(pr, pr != NONE32);
}

// wmin[head] = the smallest oriented id on the walk, wlen[head] = its edges
__global__ __launch_bounds__(hu::EB) void walk_kernel(const unsigned long long *pairs, const uint32_t *succ, uint64_t n, uint32_t *wmin, uint32_t *wlen) {
    const uint64_t o = hu::gid();
    const bool live = o < n;
    uint32_t h = NONE32;
    if (live) {
        const uint64_t pr = pairs[o];
        h = (uint32_t)pr == NONE32 ? (uint32_t)o : (uint32_t)pr;
        const uint32_t s = succ[o];
        if (s == NONE32 || s == h) wlen[h] = (uint32_t)(pr >> 32) + 1u;
    }
    const uint32_t h0 = __shfl(h, 0);
    if (__all(live && h == h0)) {  // the whole wave lies on one walk: its first lane holds the smallest id
        if ((threadIdx.x & (warpSize - 1)) == 0) atomicMin(&wmin[h], (uint32_t)o);
    } else if (live) {
        atomicMin(&wmin[h], (uint32_t)o);
    }
}
// ---- tip clipping and isolated unitigs (cleaned calls) ----
// counters of one round: [0] tips, [1] isolated walks, [2] tip k-mers, [3] isolated k-mers, [4] removed occurrences; of a round that
// pops bubbles also [5] arm k-mers, [6] their occurrences, [7] popped arms
constexpr int CLEAN_COUNTERS = 8;
constexpr uint8_t VERDICT_TIP = 1, VERDICT_ISOLATED = 2, VERDICT_BUBBLE = 3;
enum EndState : int { END_FREE = 0, END_ANCHORED = 1, END_THROUGH = 2 };

// 0, 1 or 2 (= two or more) incident edges
__device__ __forceinline__ int incident_count(uint32_t word) { return word == NONE32 ? 0 : (word == MULTI32 ? 2 : 1); }

// The state of the end behind oriented k-mer o, i.e. of o's head node v: the suffix of the reading as read (o even) or the reverse
// complement of its prefix (o odd). The slot's words belong to the canonical orientation c of v's class: out(v) is out_e for v = c
// and (mirrored) in_e for v = rc(c); the prefix as read is rc(v), which turns the roles once more. At a self-mirror node an
// incident k-mer is recorded once, under in_e where its reading ends in v and under out_e where it starts there, and each stands
// for one edge that leaves v: |out(v)| is the sum of both words.
__device__ __forceinline__ int end_state(const NodeArgs &a, uint32_t o, unsigned int *err) {
    kw::ClassKey key;
    const uint64_t s = find_node<false>(a, a.kpos[o >> 1] + ((o & 1u) ? 0 : 1), key, err);
    const int oc = incident_count(a.out_e[s]), ic = incident_count(a.in_e[s]);
    if (key.pal) return oc + ic <= 1 ? END_FREE : END_ANCHORED;  // beyond = beside = |out(v)| - 1
    const bool turned = key.flip != (bool)(o & 1u);
    const int beyond = turned ? ic : oc, into = turned ? oc : ic;
    return into >= 2 ? END_ANCHORED : (beyond == 0 ? END_FREE : END_THROUGH);
}

// sums[c] += the block's total of v[c], c < n: per wave by shuffles, per block through LDS, then at most one global atomic per counter
template <int n>
__device__ __forceinline__ void block_add(unsigned long long (&v)[n], unsigned long long *sums) {
    __shared__ unsigned long long part[n][hu::EB / 64];
    const int lane = threadIdx.x & (warpSize - 1), wave = threadIdx.x / warpSize;
#pragma unroll
    for (int c = 0; c < n; c++) {
        for (int d = warpSize / 2; d > 0; d /= 2) v[c] += __shfl_down(v[c], d);
        if (lane == 0) part[c][wave] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < n) {
        unsigned long long t = 0;
        for (int w = 0; w < hu::EB / 64; w++) t += part[threadIdx.x][w];
        if (t) atomicAdd(&sums[threadIdx.x], t);
    }
}

// ---- the filter probe (selected calls) ----
// One thread owns RUN window starts of the FILTER store f (packed on its own) and looks every window up in the k-mer table of the
// main store a: lookup only (find_slot<false>), so nothing is claimed and no filter k-mer ever enters the table. The tag pre-filters,
// the two-store kw::same_class decides identity base by base: as exact as the insertion, for every k. A hit adds 1 to sub[slot] or
// inter[slot] by the role of the window's record (roles: [n_rec], 0 subtract, 1 intersect; read again only where the record changes
// inside the run; each array is there only if its role occurs). Sums: nothing depends on how the atomics land. hits[0 / 1] += the
// windows of either role whose class is in the table, reduced per wave and per block: at most one global atomic per counter and block.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void filter_probe_kernel(KmerArgs a, kw::WindowArgs f, uint64_t n_bases, uint64_t n_rec, const uint8_t *roles,
                                                               uint32_t *sub, uint32_t *inter, unsigned long long *hits) {
    const uint64_t p0 = hu::gid() * RUN;
    unsigned long long sub_hits = 0, inter_hits = 0;
    if (p0 < n_bases) {
        uint64_t role_rec = ~0ull;
        uint32_t role = 0;
        kw::for_each_window<WIDE>(f, p0, p0 + RUN < n_bases ? p0 + RUN : n_bases, 0, n_rec, [&](uint64_t q, uint64_t r, const kw::Window &w) {
            const unsigned long long tag = kw::tagged_pos(w.hash, 0) >> 40;
            const kw::Found found = kw::find_slot<false>(a.table, a.slots, w.hash, 0ull, [&](unsigned long long cur) {
                return (cur >> 40) == tag && kw::same_class(f.packed, q, a.packed, cur & POS_LIMIT, a.k);
            });
            if (found.slot == a.slots) return;
            if (r != role_rec) {
                role_rec = r;
                role = roles[r];
            }
            if (role) {
                atomicAdd(&inter[found.slot], 1u);
                inter_hits++;
            } else {
                atomicAdd(&sub[found.slot], 1u);
                sub_hits++;
            }
        });
    }
    unsigned long long c[2] = {sub_hits, inter_hits};
    block_add<2>(c, hits);
}
// ksub[id] / kint[id] = the filter counters of k-mer id, carried to the dense ids as kpos_kernel carries kcount (null: the role does not occur)
__global__ __launch_bounds__(hu::EB) void kpos_filter_kernel(const unsigned long long *table, uint64_t slots, const uint32_t *id_of_pos,
                                                              const uint32_t *abundance, uint64_t m, const uint32_t *sub, const uint32_t *inter,
                                                              uint32_t *ksub, uint32_t *kint) {
    const uint64_t s = hu::gid();
    if (s >= slots) return;
    const unsigned long long cur = table[s];
    if (cur == EMPTY_SLOT || abundance[s] < m) return;
    const uint32_t id = id_of_pos[cur & POS_LIMIT];
    if (sub) ksub[id] = sub[s];
    if (inter) kint[id] = inter[s];
}

// The five rules over the ids of S_m, in their order (include/mtg_engine.h): keep[i] = 1 where k-mer i passes them all. kcolor: null in
// a call without colours (the mask counts as empty: check_request lets no colour rule through then); ksub / kint: null where the
// role has no record (the rule does not apply). counters: [0 .. 5) the k-mers rejected by forbid, require, carriers, subtract,
// intersect -- each under the first rule it fails --, [5] the selected k-mers, [6] their occurrences, [SELECT_COLOR + c] the selected
// k-mers with bit c. The scalars are reduced per wave and block (block_add). Per colour: a wave holds 64 masks, one per lane; the
// ballot of (selected and bit c) is column c of that 64 x 64 bit block and its popcount the wave's count, kept by lane c -- C ballots
// per wave, never a loop over set bits --, added per workgroup in LDS and leaving by at most one global atomic per colour and block.
struct SelectArgs {
    uint64_t require, forbid, min_colors, max_colors, sub_min, int_min;
};
constexpr int SELECT_SCALARS = 7, SELECT_COLOR = 8, SELECT_WORDS = SELECT_COLOR + 64;
__global__ __launch_bounds__(hu::EB) void select_keep_kernel(const unsigned long long *kcolor, const uint32_t *kcount, const uint32_t *ksub,
                                                              const uint32_t *kint, SelectArgs p, int C, uint64_t N, uint32_t *keep,
                                                              unsigned long long *counters) {
    __shared__ uint32_t per_color[64];
    if (threadIdx.x < 64) per_color[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = hu::gid();
    const int lane = threadIdx.x & 63;
    unsigned long long c[SELECT_SCALARS] = {};
    unsigned long long mask = 0;
    bool kept = false;
    if (i < N) {
        mask = kcolor ? kcolor[i] : 0ull;
        const uint64_t carriers = (uint64_t)__popcll(mask);
        int fail = 5;
        if (mask & p.forbid) fail = 0;
        else if ((mask & p.require) != p.require) fail = 1;
        else if (carriers < p.min_colors || carriers > p.max_colors) fail = 2;
        else if (ksub && ksub[i] >= p.sub_min) fail = 3;
        else if (kint && kint[i] < p.int_min) fail = 4;
        kept = fail == 5;
        keep[i] = kept;
#pragma unroll
        for (int r = 0; r < 6; r++) c[r] = fail == r;
        c[6] = kept ? kcount[i] : 0u;
    }
    uint32_t mine = 0;
    for (int b = 0; b < C; b++) {  // (uniform: every lane of the wave takes part in the ballot)
        const unsigned long long t = __ballot(kept && ((mask >> b) & 1));
        mine = lane == b ? (uint32_t)__popcll(t) : mine;
    }
    if (mine) atomicAdd(&per_color[lane], mine);
    __syncthreads();
    if (threadIdx.x < 64 && per_color[threadIdx.x]) atomicAdd(&counters[SELECT_COLOR + threadIdx.x], (unsigned long long)per_color[threadIdx.x]);
    block_add<SELECT_SCALARS>(c, counters);
}

// One thread per oriented k-mer that ends an open walk (succ == none; the last element of a cut cycle has its head as successor and
// never gets here). The walk e_1 .. e_n has n = rank + 1 k-mers and e_1 = jump; its two ends are the head node of e_n and the head
// node of e_1's mirror. The verdict goes to verdict[e_1]. The thread at the end of the mirror walk sees the same two states in the
// other order, so it writes the same verdict to its own first element: no word has two writers, and a walk is counted by the one of
// the two threads with the smaller id (a walk is never its own mirror: the two ids differ).
__global__ __launch_bounds__(hu::EB) void clean_decide_kernel(NodeArgs a, const unsigned long long *pairs, uint64_t n, uint64_t tip_kmers,
                                                               uint64_t isolated_kmers, uint8_t *verdict, unsigned long long *counters,
                                                               unsigned int *err) {
    const uint64_t o = hu::gid();
    unsigned long long c[2] = {0, 0};  // tips, isolated walks
    if (o < n && a.succ[o] == NONE32) {
        const uint64_t pr = pairs[o];
        const uint32_t first = (uint32_t)pr == NONE32 ? (uint32_t)o : (uint32_t)pr;
        const uint64_t len = (pr >> 32) + 1;
        if ((len < tip_kmers || len < isolated_kmers) && a.succ[first ^ 1u] == NONE32) {  // (the second clause: e_1 has no predecessor)
            const int here = end_state(a, (uint32_t)o, err), there = end_state(a, first ^ 1u, err);
            uint8_t v = 0;
            if (len < tip_kmers && here + there == END_FREE + END_ANCHORED) v = VERDICT_TIP;  // (0 + 1: no other pair of states sums to 1)
            if (len < isolated_kmers && here == END_FREE && there == END_FREE) v = VERDICT_ISOLATED;
            if (v) {
                verdict[first] = v;
                if ((uint32_t)o < (first ^ 1u)) c[v - 1] = 1;
            }
        }
    }
    block_add<2>(c, counters);
}

// ---- bubble popping (simplified calls) ----
// A short open walk W = e_1 .. e_n (n < L_bub) from its tail node u (the prefix of e_1 as read) to its head node v (the suffix of
// e_n) is a candidate ARM unless u or v is self-mirror, u = v or u = rc(v); the arms with one (u, v) form a BUNDLE, an arm and its
// mirror (from rc(v) to rc(u)) counting once. An ORIENTED NODE ID is 2 * (the class's slot in the node table) + (the node is the
// reverse complement of the class's canonical form): rc(x) has id(x) ^ 1, and the exclusions read "u or v self-mirror, or one slot".
// Slots reach 2^33, so the two ids of a key do not fit one 64-bit word: a key is kept as two words (tail, head), the table of the
// choose step holds 32-bit LIST SLOTS and compares the keys behind them.
// The list of a round has one slot per short open walk, the walk and its mirror counting once: bubble_flag_kernel flags the
// smaller of the two walks' first elements (e_1 and mirror(e_n)), the scan of the flags numbers the slots (M of them), and of the
// two threads at the walks' ends the one whose key (tail, head) is the lexicographically smaller of (u, v) and (rc(v), rc(u)) fills
// the slot -- the keys are equal only in the excluded hairpin case. An excluded walk leaves its slot a hole (n = 0).
struct ArmArgs {
    unsigned long long *tail, *head;  // [M] oriented node ids
    uint32_t *first, *last;           // [M] e_1 and e_n of the walk whose thread made the entry
    uint32_t *n;                      // [M] the arm's k-mers; 0: a hole
    uint32_t *off;                    // [M] the exclusive scan of n: the arm's place among the K k-mers of all arms
    uint32_t *sum;                    // [M] the sum of the arm's abundances (below 2^32: fewer than 2^32 windows)
    uint32_t *table;                  // [slots] a list slot of the best arm seen of a key, or none
    uint64_t M, slots;
};

// the end element o of an open walk shorter than max_arm: its first element, else none
__device__ __forceinline__ uint32_t short_walk_first(const uint32_t *succ, const unsigned long long *pairs, uint64_t o, uint64_t max_arm, uint64_t *len) {
    if (succ[o] != NONE32) return NONE32;
    const uint64_t pr = pairs[o];
    const uint32_t first = (uint32_t)pr == NONE32 ? (uint32_t)o : (uint32_t)pr;
    *len = (pr >> 32) + 1;
    return *len < max_arm && succ[first ^ 1u] == NONE32 ? first : NONE32;
}
// flag[min(e_1, mirror(e_n))] = 1 per short open walk; written by the one of the two end threads whose e_1 is the smaller (a walk is
// never its own mirror: the two differ)
__global__ __launch_bounds__(hu::EB) void bubble_flag_kernel(const uint32_t *succ, const unsigned long long *pairs, uint64_t n, uint64_t max_arm, uint32_t *flag) {
    const uint64_t o = hu::gid();
    if (o >= n) return;
    uint64_t len;
    const uint32_t first = short_walk_first(succ, pairs, o, max_arm, &len);
    if (first != NONE32 && first < ((uint32_t)o ^ 1u)) flag[first] = 1u;
}
// slot_of: the exclusive scan of the flags. The two probes give the ids; the thread with the smaller key fills the slot.
__global__ __launch_bounds__(hu::EB) void bubble_list_kernel(NodeArgs a, const unsigned long long *pairs, uint64_t n, uint64_t max_arm, const uint32_t *slot_of,
                                                              ArmArgs b, unsigned int *err) {
    const uint64_t o = hu::gid();
    if (o >= n) return;
    uint64_t len;
    const uint32_t first = short_walk_first(a.succ, pairs, o, max_arm, &len);
    if (first == NONE32) return;
    kw::ClassKey key;
    // v: the suffix of the reading (o even) or the reverse complement of its prefix; u: the prefix of e_1's reading or rc(its suffix)
    const uint64_t sv = find_node<false>(a, a.kpos[o >> 1] + ((o & 1u) ? 0 : 1), key, err);
    const bool pal_v = key.pal;
    const uint64_t head = 2 * sv + (uint64_t)(key.flip != (bool)(o & 1u));
    const uint64_t su = find_node<false>(a, a.kpos[first >> 1] + ((first & 1u) ? 1 : 0), key, err);
    const uint64_t tail = 2 * su + (uint64_t)(key.flip != (bool)(first & 1u));
    if (pal_v || key.pal || su == sv) return;  // a self-mirror end; u = v (a loop at one node); u = rc(v) (a hairpin)
    if (tail > (head ^ 1ull)) return;          // the mirror key (rc(v), rc(u)) is the smaller: its thread makes the entry
    const uint32_t mf = (uint32_t)o ^ 1u;      // (the first elements cannot be equal: tail = head ^ 1 means one slot)
    const uint32_t e = slot_of[first < mf ? first : mf];
    if (e >= b.M) return;  // (never: that element was flagged)
    b.tail[e] = tail;
    b.head[e] = head;
    b.first[e] = first;
    b.last[e] = (uint32_t)o;
    b.n[e] = (uint32_t)len;
}
// Every k-mer of an arm writes its abundance at off[arm] + its rank on the entry's walk: no thread walks a chain. The k-mer's two
// orientations lie on the walk and its mirror at ranks r and n - 1 - r, so n = rank(2 i) + rank(2 i + 1) + 1 without a lookup, and
// only the k-mers of short walks look for a list slot: the one flagged at the smaller of their two heads.
__global__ __launch_bounds__(hu::EB) void bubble_counts_kernel(const unsigned long long *pairs, const uint32_t *kcount, uint64_t N, uint64_t max_arm,
                                                                const uint32_t *slot_of, ArmArgs b, uint32_t *ordered) {
    const uint64_t i = hu::gid();
    if (i >= N) return;
    const uint64_t p0 = pairs[2 * i], p1 = pairs[2 * i + 1];
    if ((p0 >> 32) + (p1 >> 32) + 1 >= max_arm) return;
    const uint32_t h0 = (uint32_t)p0 == NONE32 ? (uint32_t)(2 * i) : (uint32_t)p0, h1 = (uint32_t)p1 == NONE32 ? (uint32_t)(2 * i + 1) : (uint32_t)p1;
    const uint32_t at = h0 < h1 ? h0 : h1, e = slot_of[at];
    if (e >= b.M || b.n[e] == 0) return;  // (a closed walk's ranks may look short: its heads hold no slot) / a hole
    const uint32_t f = b.first[e], mf = b.last[e] ^ 1u;
    if ((f < mf ? f : mf) != at) return;  // the slot flagged at `at` and no earlier one
    const uint32_t rank = (uint32_t)((h0 == f ? p0 : p1) >> 32);
    if (rank < b.n[e]) ordered[b.off[e] + rank] = kcount[i];  // (always: the guard keeps the write inside the arm's range)
}
// prefix: the exclusive scan of `ordered` to 64 bits, *total its end
__global__ __launch_bounds__(hu::EB) void bubble_sums_kernel(ArmArgs b, const unsigned long long *prefix, const unsigned long long *total, uint64_t K) {
    const uint64_t e = hu::gid();
    if (e >= b.M || b.n[e] == 0) return;
    const uint64_t lo = b.off[e], hi = lo + b.n[e];
    b.sum[e] = (uint32_t)((hi < K ? prefix[hi] : *total) - prefix[lo]);
}

__device__ __forceinline__ uint64_t arm_hash(uint64_t tail, uint64_t head) { return kw::mix64(kw::mix64(tail) + head); }
// The order inside a bundle: the larger mean abundance (sum_x n_y > sum_y n_x, below 2^63: exact in 64 bits), then the smaller of
// the two end k-mers' ids (ids are in creator order; arms of one bundle share no k-mer, so the order is total; both are the same on
// either strand).
__device__ __forceinline__ bool arm_better(const ArmArgs &b, uint32_t x, uint32_t y) {
    const uint64_t l = (uint64_t)b.sum[x] * b.n[y], r = (uint64_t)b.sum[y] * b.n[x];
    if (l != r) return l > r;
    const uint32_t tx = b.first[x] < b.last[x] ? b.first[x] : b.last[x], ty = b.first[y] < b.last[y] ? b.first[y] : b.last[y];
    return (tx >> 1) < (ty >> 1);
}
// Open addressing over 2 M table slots, linear probing from the key's hash. An empty slot is claimed by CAS; a claimed slot keeps its
// key for good (it is only ever replaced by a better arm of the same key), so every key owns one slot, and the CAS loop replaces
// the slot's arm only by a better one: the final state is the bundle's maximum in any interleaving.
__global__ __launch_bounds__(hu::EB) void bubble_choose_kernel(ArmArgs b, unsigned int *err) {
    const uint64_t g = hu::gid();
    if (g >= b.M || b.n[g] == 0) return;
    const uint32_t e = (uint32_t)g;
    const uint64_t tail = b.tail[e], head = b.head[e];
    uint64_t s = __umul64hi(arm_hash(tail, head), b.slots);
    for (uint64_t probe = 0; probe < b.slots; probe++) {
        uint32_t cur = __hip_atomic_load(&b.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == NONE32) {
            cur = atomicCAS(&b.table[s], NONE32, e);
            if (cur == NONE32) return;
        }
        if (b.tail[cur] == tail && b.head[cur] == head) {
            while (arm_better(b, e, cur)) {
                const uint32_t prev = atomicCAS(&b.table[s], cur, e);
                if (prev == cur) return;
                cur = prev;
            }
            return;
        }
        if (++s == b.slots) s = 0;
    }
    atomicOr(err, 32u);  // (2 table slots per arm: never full)
}
// Every arm that is not its bundle's best B and has sum_B n_a >= R sum_a n_B is popped: the verdict goes to the first elements of
// its walk and of the mirror walk, the arm is counted once. R sum_a < 2^40 and n_B < 2^31: the right side is taken in 128 bits.
__global__ __launch_bounds__(hu::EB) void bubble_verdict_kernel(ArmArgs b, uint64_t ratio, uint8_t *verdict, unsigned long long *arms, unsigned int *err) {
    const uint64_t g = hu::gid();
    unsigned long long c[1] = {0};
    if (g < b.M && b.n[g] != 0) {
        const uint32_t e = (uint32_t)g;
        const uint64_t tail = b.tail[e], head = b.head[e];
        uint64_t s = __umul64hi(arm_hash(tail, head), b.slots);
        uint32_t best = NONE32;
        for (uint64_t probe = 0; probe < b.slots && best == NONE32; probe++) {
            const uint32_t cur = b.table[s];
            if (cur == NONE32) break;
            if (b.tail[cur] == tail && b.head[cur] == head) best = cur;
            if (++s == b.slots) s = 0;
        }
        if (best == NONE32) {
            atomicOr(err, 32u);  // (every arm's key was put in)
        } else if (best != e) {
            const uint64_t left = (uint64_t)b.sum[best] * b.n[e], m = ratio * b.sum[e];
            if (__umul64hi(m, (uint64_t)b.n[best]) == 0 && left >= m * b.n[best]) {
                verdict[b.first[e]] = VERDICT_BUBBLE;
                verdict[b.last[e] ^ 1u] = VERDICT_BUBBLE;
                c[0] = 1;
            }
        }
    }
    block_add<1>(c, arms);
}

// keep[i] = 0 where the walk of k-mer i has a verdict (read at the first element of the reading's walk: the mirror walk holds the
// same); the removed k-mers and their abundances are counted on the way (kcount: null in a call that does not count). POP: popped
// arms' k-mers and occurrences go to counters of their own.
template <bool POP>
__global__ __launch_bounds__(hu::EB) void clean_keep_kernel(const unsigned long long *pairs, const uint8_t *verdict, const uint32_t *kcount, uint64_t N,
                                                             uint32_t *keep, unsigned long long *counters) {
    const uint64_t i = hu::gid();
    unsigned long long c[POP ? 5 : 3] = {};  // tip k-mers, isolated k-mers, their occurrences [, arm k-mers, their occurrences]
    if (i < N) {
        const uint32_t j = (uint32_t)pairs[2 * i];
        const uint8_t v = verdict[j == NONE32 ? 2 * i : j];
        keep[i] = v == 0;
        if (POP && v == VERDICT_BUBBLE) {
            c[POP ? 3 : 0] = 1;
            c[POP ? 4 : 0] = kcount[i];
        } else if (v) {
            c[v - 1] = 1;
            c[2] = kcount ? kcount[i] : 0;
        }
    }
    block_add<POP ? 5 : 3>(c, counters + 2);
}
// the kept k-mers move to their new ids (new_id: the exclusive scan of keep -- creator order is kept)
__global__ __launch_bounds__(hu::EB) void clean_move_kernel(const uint32_t *keep, const uint32_t *new_id, uint64_t N, const unsigned long long *kpos,
                                                             const uint32_t *kcount, const unsigned long long *kcolor, unsigned long long *kpos_to,
                                                             uint32_t *kcount_to, unsigned long long *kcolor_to) {
    const uint64_t i = hu::gid();
    if (i >= N || !keep[i]) return;
    const uint32_t to = new_id[i];
    kpos_to[to] = kpos[i];
    if (kcount) kcount_to[to] = kcount[i];
    if (kcolor) kcolor_to[to] = kcolor[i];
}

// heads of emitted walks (the minimum is even: the walk holds the reading of its leader) leave their length at the leader's id
// stats: [0] closed walks, [1] k-mers of the longest unitig
__global__ __launch_bounds__(hu::EB) void leader_kernel(const unsigned long long *pairs, const uint32_t *succ, uint64_t n, const uint32_t *wmin,
                                                         const uint32_t *wlen, uint32_t k, uint32_t *lead_flag, uint32_t *lead_chars,
                                                         unsigned long long *stats) {
    const uint64_t o = hu::gid();
    if (o >= n || (uint32_t)pairs[o] != NONE32) return;
    const uint32_t m = wmin[o];
    if (m & 1u) return;
    lead_flag[m >> 1] = 1u;
    lead_chars[m >> 1] = wlen[o] + k - 1;
    if (succ[o ^ 1u] != NONE32) atomicAdd(&stats[0], 1ull);  // a head with a predecessor: a cut cycle
    if (wlen[o] > load64(&stats[1])) atomicMax(&stats[1], (unsigned long long)wlen[o]);  // (after a plain read: only improving lengths reach the atomic)
}
__global__ __launch_bounds__(hu::EB) void offsets_kernel(const uint32_t *lead_chars, const uint32_t *unitig_of, const uint64_t *char_off, uint64_t N,
                                                          unsigned long long *out_off) {
    const uint64_t i = hu::gid();
    if (i < N && lead_chars[i]) out_off[unitig_of[i]] = char_off[i];
}
__global__ __launch_bounds__(hu::EB) void spell_kernel(const uint32_t *packed, const unsigned long long *kpos, const unsigned long long *pairs,
                                                        const uint32_t *wmin, const uint64_t *char_off, uint64_t n, uint64_t k, char *out) {
    const uint64_t o = hu::gid();
    if (o >= n) return;
    const uint64_t pr = pairs[o];
    const uint32_t h = (uint32_t)pr == NONE32 ? (uint32_t)o : (uint32_t)pr, m = wmin[h];
    if (m & 1u) return;
    const uint64_t at = char_off[m >> 1], rank = pr >> 32, pos = kpos[o >> 1];
    const bool mir = o & 1;
    const char *abc = "ACGT";
    out[at + rank + k - 1] = abc[mir ? 3u - packed_base(packed, pos) : packed_base(packed, pos + k - 1)];
    if (rank == 0)
        for (uint64_t j = 0; j + 1 < k; j++) out[at + j] = abc[mir ? 3u - packed_base(packed, pos + k - 1 - j) : packed_base(packed, pos + j)];
}

// ---- per-unitig abundance sums (counted calls) ----
// Every oriented k-mer of an emitted walk writes its k-mer's abundance at its place in unitig order: unitig u starts at character
// offset char_off, i.e. at k-mer offset char_off - (k - 1) u, and the k-mer is `rank` steps behind the walk's head.
// (T: uint32_t abundances, unsigned long long colour masks)
template <typename T>
__global__ __launch_bounds__(hu::EB) void order_counts_kernel(const unsigned long long *pairs, const uint32_t *wmin, const uint64_t *char_off,
                                                               const uint32_t *unitig_of, const T *kcount, uint64_t n, uint64_t k, T *ordered) {
    const uint64_t o = hu::gid();
    if (o >= n) return;
    const uint64_t pr = pairs[o];
    const uint32_t h = (uint32_t)pr == NONE32 ? (uint32_t)o : (uint32_t)pr, m = wmin[h];
    if (m & 1u) return;
    ordered[char_off[m >> 1] - (k - 1) * unitig_of[m >> 1] + (pr >> 32)] = kcount[o >> 1];
}
// sums[u] = prefix[first k-mer of u + 1] - prefix[first k-mer of u] over the exclusive 64-bit prefix sums of `ordered`
__global__ __launch_bounds__(hu::EB) void unitig_sums_kernel(const unsigned long long *out_off, const uint64_t *prefix, const uint64_t *total,
                                                              uint64_t n_unitigs, uint64_t k, unsigned long long *sums) {
    const uint64_t u = hu::gid();
    if (u >= n_unitigs) return;
    const uint64_t lo = prefix[out_off[u] - (k - 1) * u];
    sums[u] = (u + 1 < n_unitigs ? prefix[out_off[u + 1] - (k - 1) * (u + 1)] : *total) - lo;
}

// ---- colour classes ----
// A RUN is a maximal stretch of consecutive windows of one unitig with equal masks; the classes are the distinct masks, numbered in
// the order of the first window that shows them. Everything is computed per run, never per k-mer, and no kernel walks a run.
//   heads     head[i] = 1 where window i opens a unitig (one thread per unitig) or its mask differs from that of window i - 1 (one
//             thread per window); the exclusive scan of head is, at a head, its run's number; run_start[r] = the head of run r.
//   table     one insertion per run into an open-addressing table keyed by the mask (0 = empty, kept masks are never 0; 2 slots per
//             run). The slot keeps the smallest run number by atomicMin behind a plain compare -- run starts ascend with the run
//             number, so that is the run of the class's first window, and as runs arrive in ascending order almost every later one
//             fails the compare and issues no atomic (the insert idiom of the k-mer table above).
//   ids       every occupied slot flags its smallest run; the scan of the flags numbers the classes in first-appearance order.
//   counts    a grid-stride sweep over the runs: kmers[c] += length, runs[c] += 1. Equal classes are combined inside the wave first,
//             then in an LDS table per workgroup indexed by the class number, which leaves by at most one 64-bit global atomicAdd per
//             touched class, counter and workgroup; classes from CLASS_LDS on go to global memory directly.
//   window    kmer_class[i] = the class of window i's run.
// Order independence: a slot's key is written once (CAS from 0) and compared by value, so which slot a mask ends in may vary with the
// order but nothing that leaves the table does: the smallest run is a minimum, the ids come from a scan over run numbers, the
// counters are integer sums, and run_start, run_slot, run_class, the per-class words and kmer_class are single-writer words.
constexpr int CLASS_LDS = 2048;   // classes 0 .. CLASS_LDS - 1 are counted in LDS (16 KiB per workgroup)
constexpr int CLASS_GRID = 512;   // the counts kernel's largest grid
constexpr int CLASS_PEEL = 2;     // classes combined across the wave before the lanes left add on their own

__device__ __forceinline__ uint64_t mask_hash(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    return x ^ (x >> 33);
}
__global__ __launch_bounds__(hu::EB) void unitig_heads_kernel(const unsigned long long *out_off, uint64_t n_unitigs, uint64_t k, uint32_t *head) {
    const uint64_t u = hu::gid();
    if (u < n_unitigs) head[out_off[u] - (k - 1) * u] = 1u;
}
__global__ __launch_bounds__(hu::EB) void run_heads_kernel(const unsigned long long *ordered, uint64_t N, uint32_t *head) {
    const uint64_t i = hu::gid();
    if (i && i < N && ordered[i] != ordered[i - 1]) head[i] = 1u;
}
__global__ __launch_bounds__(hu::EB) void run_starts_kernel(const uint32_t *head, const uint32_t *run_of, uint64_t N, uint64_t R, uint32_t *run_start) {
    const uint64_t i = hu::gid();
    if (i < N && head[i]) run_start[run_of[i]] = (uint32_t)i;
    if (i == 0) run_start[R] = (uint32_t)N;
}
__global__ __launch_bounds__(hu::EB) void class_insert_kernel(const unsigned long long *ordered, const uint32_t *run_start, uint64_t R,
                                                               unsigned long long *keys, uint32_t *min_run, uint64_t slots, uint32_t *run_slot,
                                                               unsigned int *err) {
    const uint64_t r = hu::gid();
    if (r >= R) return;
    const unsigned long long mask = ordered[run_start[r]];
    uint64_t s = mask_hash(mask) % slots;
    for (uint64_t probe = 0; probe < slots; probe++, s = s + 1 == slots ? 0 : s + 1) {
        unsigned long long cur = load64(&keys[s]);
        if (cur == 0) {
            cur = atomicCAS(&keys[s], 0ull, mask);
            if (cur == 0) cur = mask;
        }
        if (cur != mask) continue;
        run_slot[r] = (uint32_t)s;
        if ((uint32_t)r < __hip_atomic_load(&min_run[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&min_run[s], (uint32_t)r);
        return;
    }
    atomicOr(err, 16u);  // (2 slots per run: never full)
}
__global__ __launch_bounds__(hu::EB) void class_flag_kernel(const unsigned long long *keys, const uint32_t *min_run, uint64_t slots, uint32_t *flag) {
    const uint64_t s = hu::gid();
    if (s < slots && keys[s]) flag[min_run[s]] = 1u;
}
// per occupied slot: its class number, and the class's mask and first window
__global__ __launch_bounds__(hu::EB) void class_ids_kernel(const unsigned long long *keys, const uint32_t *min_run, uint64_t slots, const uint32_t *id_of_run,
                                                            const uint32_t *run_start, uint32_t *slot_class, unsigned long long *masks,
                                                            unsigned long long *first) {
    const uint64_t s = hu::gid();
    if (s >= slots || !keys[s]) return;
    const uint32_t c = id_of_run[min_run[s]];
    slot_class[s] = c;
    masks[c] = keys[s];
    first[c] = run_start[min_run[s]];
}
// out: [0 .. n_classes) kmers, [n_classes .. 2 n_classes) runs
__global__ __launch_bounds__(hu::EB) void class_counts_kernel(const uint32_t *run_start, const uint32_t *run_slot, const uint32_t *slot_class, uint64_t R,
                                                               uint64_t n_classes, uint32_t *run_class, unsigned long long *out) {
    __shared__ uint32_t lds_kmers[CLASS_LDS];  // (fewer than 2^31 k-mers: they cannot wrap)
    __shared__ uint32_t lds_runs[CLASS_LDS];
    for (int e = threadIdx.x; e < CLASS_LDS; e += hu::EB) lds_kmers[e] = lds_runs[e] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * hu::EB;  // (a multiple of 64: the lanes of a wave leave the loop together)
    for (uint64_t at = hu::gid() - lane; at < R; at += stride) {
        const uint64_t r = at + lane;
        bool todo = r < R;
        uint32_t c = 0, len = 0;
        if (todo) {
            c = slot_class[run_slot[r]];
            len = run_start[r + 1] - run_start[r];
            run_class[r] = c;
        }
        for (int round = 0; round < CLASS_PEEL; round++) {  // the class of the first lane left, summed over the wave by a butterfly
            const unsigned long long left = __ballot(todo);
            if (!left) break;  // (uniform)
            const int leader = __ffsll(left) - 1;
            const uint32_t cl = __shfl(c, leader);
            const bool same = todo && c == cl;
            const unsigned long long group = __ballot(same);
            if (__popcll(group) < 4) break;  // (uniform) too few to be worth the butterfly
            uint32_t sum = same ? len : 0u;
            for (int d = 32; d > 0; d /= 2) sum += __shfl_xor(sum, d);
            if (lane == leader) {
                if (cl < CLASS_LDS) {
                    atomicAdd(&lds_kmers[cl], sum);
                    atomicAdd(&lds_runs[cl], (uint32_t)__popcll(group));
                } else {
                    atomicAdd(&out[cl], (unsigned long long)sum);
                    atomicAdd(&out[n_classes + cl], (unsigned long long)__popcll(group));
                }
            }
            todo = todo && !same;
        }
        if (todo) {
            if (c < CLASS_LDS) {
                atomicAdd(&lds_kmers[c], len);
                atomicAdd(&lds_runs[c], 1u);
            } else {
                atomicAdd(&out[c], (unsigned long long)len);
                atomicAdd(&out[n_classes + c], 1ull);
            }
        }
    }
    __syncthreads();
    for (uint64_t e = threadIdx.x; e < CLASS_LDS && e < n_classes; e += hu::EB) {
        if (lds_runs[e]) {
            atomicAdd(&out[e], (unsigned long long)lds_kmers[e]);
            atomicAdd(&out[n_classes + e], (unsigned long long)lds_runs[e]);
        }
    }
}
__global__ __launch_bounds__(hu::EB) void window_class_kernel(const uint32_t *head, const uint32_t *run_of, const uint32_t *run_class, uint64_t N,
                                                               uint32_t *kmer_class) {
    const uint64_t i = hu::gid();
    if (i < N) kmer_class[i] = run_class[run_of[i] + head[i] - 1u];  // (exclusive scan: a head has its own number, the others the next one)
}

int log2_ceil(uint64_t n) {
    int r = 0;
    while ((1ull << r) < n) r++;
    return r;
}

// The class dictionary of a store's masks in window order (ordered: [N], out_off: the unitigs' character offsets). Device memory, all
// from the arena: 8 B per k-mer (head, run number) and 4 B more for kmer_class; per run R 4 (start) + 4 (slot) + 4 (class) + 4 (flag,
// scanned in place) + 2 x (8 + 4 + 4) (the table: key, smallest run, class per slot); per class 32 B. All of it goes back at the end.
void color_classes(const unsigned long long *d_ordered, const unsigned long long *d_out_off, uint64_t N, uint64_t n_unitigs, uint64_t k, bool split,
                   hipStream_t st, ScalarBlock &small, int device_id, ColorClasses *out, ColorClassTimes *times) {
    const char *const stage = "colour classes";
    PhaseEvents<5> ev;
    ev.mark(0, st);
    // ---- run heads ----
    hu::DeviceArray<uint32_t> head(N), run_of(N);
    hu::ScanScratch<uint32_t> scan(N);
    HIP_CHECK(hipMemsetAsync(head, 0, N * 4, st));
    unitig_heads_kernel<<<hu::grid_for(n_unitigs), hu::EB, 0, st>>>(d_out_off, n_unitigs, k, head);
    run_heads_kernel<<<hu::grid_for(N), hu::EB, 0, st>>>(d_ordered, N, head);
    scan.scan(st, head, N, run_of);
    uint32_t n_runs = 0;
    HIP_CHECK(hipMemcpyAsync(&n_runs, scan.total(), 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const uint64_t R = n_runs;
    if (R < n_unitigs || R > N || (split && R != n_unitigs))
        MTG_DIE("colour classes: internal error (%llu runs in %llu unitigs of %llu k-mers%s)", (unsigned long long)R, (unsigned long long)n_unitigs,
                (unsigned long long)N, split ? ", split" : "");
    hu::DeviceArray<uint32_t> run_start(R + 1);
    run_starts_kernel<<<hu::grid_for(N), hu::EB, 0, st>>>(head, run_of, N, R, run_start);
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);
    // ---- the class table: one insertion per run ----
    const uint64_t slots = std::max<uint64_t>(8, 2 * R);
    hu::DeviceArray<unsigned long long> keys(slots);
    hu::DeviceArray<uint32_t> min_run(slots), run_slot(R);
    HIP_CHECK(hipMemsetAsync(keys, 0, slots * 8, st));
    HIP_CHECK(hipMemsetAsync(min_run, 0xFF, slots * 4, st));
    class_insert_kernel<<<hu::grid_for(R), hu::EB, 0, st>>>(d_ordered, run_start, R, keys, min_run, slots, run_slot, small.err());
    HIP_CHECK(hipGetLastError());
    ev.mark(2, st);
    // ---- class ids in first-appearance order ----
    hu::DeviceArray<uint32_t> flag(R);
    hu::ScanScratch<uint32_t> scan_runs(R);
    hu::DeviceArray<uint32_t> slot_class(slots);
    HIP_CHECK(hipMemsetAsync(flag, 0, R * 4, st));
    class_flag_kernel<<<hu::grid_for(slots), hu::EB, 0, st>>>(keys, min_run, slots, flag);
    scan_runs.scan(st, flag, R, flag);
    uint32_t n_classes32 = 0;
    HIP_CHECK(hipMemcpyAsync(&n_classes32, scan_runs.total(), 4, hipMemcpyDeviceToHost, st));
    small.read(st, stage);
    const uint64_t n_classes = n_classes32;
    if (n_classes == 0 || n_classes > R) MTG_DIE("colour classes: internal error (%llu classes in %llu runs)", (unsigned long long)n_classes, (unsigned long long)R);
    hu::DeviceArray<unsigned long long> masks(n_classes), first(n_classes), sums(2 * n_classes);
    HIP_CHECK(hipMemsetAsync(sums, 0, 2 * n_classes * 8, st));
    class_ids_kernel<<<hu::grid_for(slots), hu::EB, 0, st>>>(keys, min_run, slots, flag, run_start, slot_class, masks, first);
    HIP_CHECK(hipGetLastError());
    ev.mark(3, st);
    // ---- counts per class, and the class of every window ----
    hu::DeviceArray<uint32_t> run_class(R), kmer_class(N);
    class_counts_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(R), CLASS_GRID), hu::EB, 0, st>>>(run_start, run_slot, slot_class, R, n_classes, run_class, sums);
    window_class_kernel<<<hu::grid_for(N), hu::EB, 0, st>>>(head, run_of, run_class, N, kmer_class);
    HIP_CHECK(hipGetLastError());
    ev.mark(4, st);
    HIP_CHECK(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint64_t> h_sums(2 * n_classes);
    out->masks.resize(n_classes);
    out->first.resize(n_classes);
    out->kmer_class.resize(N);
    hu::download_sliced(out->masks.data(), masks, n_classes * 8, st, device_id);
    hu::download_sliced(out->first.data(), first, n_classes * 8, st, device_id);
    hu::download_sliced(h_sums.data(), sums, 2 * n_classes * 8, st, device_id);
    hu::download_sliced(out->kmer_class.data(), kmer_class, N * 4, st, device_id);
    out->kmers.assign(h_sums.begin(), h_sums.begin() + n_classes);
    out->runs.assign(h_sums.begin() + n_classes, h_sums.end());
    out->n_runs = R;
    times->download_ms = ms_since(t0);
    times->heads_ms = ev.ms(0, 1);
    times->table_ms = ev.ms(1, 2);
    times->ids_ms = ev.ms(2, 3);
    times->counts_ms = ev.ms(3, 4);
}

// The bubble verdicts of one round over the N k-mers behind `na` (node table, succ) and `pairs`: list, sums, choose, verdict.
// verdict: [2 N], written only where an arm is popped; *arms += the popped arms. Leaves the stream idle.
void pop_bubbles(const NodeArgs &na, const unsigned long long *d_pairs, const uint32_t *d_kcount, const mtg_bubble_params &p, uint8_t *d_verdict,
                 unsigned long long *d_arms, unsigned int *d_err, hipStream_t st) {
    const uint64_t N = na.N, n_or = 2 * N;
    hu::DeviceArray<uint32_t> slot_of(n_or);
    hu::ScanScratch<uint32_t> scan(n_or);
    HIP_CHECK(hipMemsetAsync(slot_of, 0, n_or * 4, st));
    bubble_flag_kernel<<<hu::grid_for(n_or), hu::EB, 0, st>>>(na.succ, d_pairs, n_or, p.max_arm_kmers, slot_of);
    scan.scan(st, slot_of, n_or, slot_of);
    uint32_t M = 0, K = 0;
    HIP_CHECK(hipMemcpyAsync(&M, scan.total(), 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ArmArgs b{};
    b.M = M;
    hu::DeviceArray<unsigned long long> tail, head;
    hu::DeviceArray<uint32_t> first, last, n, off;
    if (M) {
        b.tail = tail.alloc(M);
        b.head = head.alloc(M);
        b.first = first.alloc(M);
        b.last = last.alloc(M);
        b.n = n.alloc(M);
        b.off = off.alloc(M);
        HIP_CHECK(hipMemsetAsync(b.n, 0, (uint64_t)M * 4, st));
        bubble_list_kernel<<<hu::grid_for(n_or), hu::EB, 0, st>>>(na, d_pairs, n_or, p.max_arm_kmers, slot_of, b, d_err);
        scan.scan(st, b.n, M, b.off);  // (M <= N, which the scratch checks; K <= N < 2^31)
        HIP_CHECK(hipMemcpyAsync(&K, scan.total(), 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (K) {
        b.slots = std::max<uint64_t>(8, 2 * (uint64_t)M);
        hu::DeviceArray<uint32_t> ordered(K);
        hu::DeviceArray<unsigned long long> prefix(K);
        hu::ScanScratch<unsigned long long> scan64(K);
        hu::DeviceArray<uint32_t> sum(M), table(b.slots);
        b.sum = sum;
        b.table = table;
        HIP_CHECK(hipMemsetAsync(ordered, 0, (uint64_t)K * 4, st));
        HIP_CHECK(hipMemsetAsync(b.table, 0xFF, b.slots * 4, st));
        bubble_counts_kernel<<<hu::grid_for(N), hu::EB, 0, st>>>(d_pairs, d_kcount, N, p.max_arm_kmers, slot_of, b, ordered);
        scan64.scan(st, ordered, K, prefix);
        bubble_sums_kernel<<<hu::grid_for(M), hu::EB, 0, st>>>(b, prefix, scan64.total(), K);
        bubble_choose_kernel<<<hu::grid_for(M), hu::EB, 0, st>>>(b, d_err);
        bubble_verdict_kernel<<<hu::grid_for(M), hu::EB, 0, st>>>(b, p.min_ratio, d_verdict, d_arms, d_err);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipGetLastError());
}

// ---- the compaction: what a call was asked for and hands back (Call), its device state (Work), one function per stage in the
// order of the header's list of kernels, and the driver (run) ----
constexpr const char *STAGE = "unitig compaction";
struct Call {
    const CompactRequest &rq;
    uint64_t m = 0;  // min_abundance of a counted call
    bool popping = false, cleaning = false, split = false;
    std::chrono::steady_clock::time_point t_total;
    mtg_compaction r{};
    CompactTimes t{};
    mtg_abundance ab{};
    mtg_cleaning clean{};
    mtg_bubbles popped{};
    mtg_selection sel{};
    bool selecting = false;  // a Selected is given: the select stage runs, and the colour statistics are taken in front of it
    double clean_ms = 0, bubble_ms = 0;
    uint64_t filter_records[2] = {0, 0};  // by role
    UnitigStore *store = nullptr;
};

// Stage 1, host only: the request's checks, the window count, the out-parameters emptied. No device call.
void check_request(Call &c) {
    const CompactRequest &q = c.rq;
    const Counted *counted = q.counted;
    const Colored *colored = q.colored;
    const Cleaned *cleaned = q.cleaned;
    const uint64_t n_rec = q.n_rec, k = q.k;
    if (!q.off || (n_rec && q.off[n_rec] && !q.data)) MTG_DIE("mtg_compact_unitigs: null argument");
    if (k < 2) MTG_DIE("mtg_compact_unitigs: k must be >= 2");
    if (k >= (1ull << 31)) MTG_DIE("mtg_compact_unitigs: k too large");
    if (q.off[0] != 0) MTG_DIE("mtg_compact_unitigs: offsets must start at 0");
    c.t_total = std::chrono::steady_clock::now();
    c.r.records = n_rec;
    for (uint64_t u = 0; u < n_rec; u++) {
        if (q.off[u + 1] < q.off[u]) MTG_DIE("mtg_compact_unitigs: offsets decrease at record %llu", (unsigned long long)u);
        const uint64_t len = q.off[u + 1] - q.off[u];
        if (len >= k) c.r.windows += len - k + 1;
    }
    c.r.characters = q.off[n_rec];
    c.store = new UnitigStore();
    c.store->off.push_back(0);
    if (counted) {
        if (counted->m == 0) MTG_DIE("mtg_compact_unitigs_counted: min_abundance must be >= 1");
        if (c.r.windows >= (1ull << 32)) MTG_DIE("mtg_compact_unitigs_counted: %llu windows; the abundance counters are 32-bit, the limit is 2^32 - 1",
                                                 (unsigned long long)c.r.windows);
        c.m = counted->m;
        counted->sums->clear();
        if (counted->kmer_counts) counted->kmer_counts->clear();
    }
    if (colored) {
        if (colored->n_colors < 1 || colored->n_colors > MAX_COLORS)
            MTG_DIE("mtg_compact_unitigs_colored: %llu colours; 1 .. %d are served", (unsigned long long)colored->n_colors, MAX_COLORS);
        if (n_rec && !colored->record_colors) MTG_DIE("mtg_compact_unitigs_colored: null argument");
        for (uint64_t u = 0; u < n_rec; u++)
            if (colored->record_colors[u] >= colored->n_colors)
                MTG_DIE("mtg_compact_unitigs_colored: record %llu has colour %u of %llu", (unsigned long long)u, (unsigned)colored->record_colors[u],
                        (unsigned long long)colored->n_colors);
        colored->kmer_colors->clear();
        *colored->stats = mtg_color_stats{};
        colored->stats->n_colors = colored->n_colors;
        *colored->stats_ms = 0;
    }
    if (q.classed) {
        *q.classed->out = ColorClasses{};
        *q.classed->times = ColorClassTimes{};
    }
    if (cleaned && (cleaned->params.rounds < 1 || cleaned->params.rounds > 64))
        MTG_DIE("mtg_compact_unitigs_cleaned: %llu rounds; 1 .. 64 are served", (unsigned long long)cleaned->params.rounds);
    c.popping = q.bubbles && q.bubbles->params.max_arm_kmers;
    if (c.popping) {
        if (!cleaned) MTG_DIE("mtg_compact_unitigs_simplified: null argument");
        if (!counted) MTG_DIE("mtg_compact_unitigs_simplified: popping bubbles compares abundances and needs the abundance and sums out-pointers");
        if (q.bubbles->params.min_ratio < 1 || q.bubbles->params.min_ratio > 255)
            MTG_DIE("mtg_compact_unitigs_simplified: min_ratio %llu; 1 .. 255 are served", (unsigned long long)q.bubbles->params.min_ratio);
    }
    c.cleaning = (cleaned && (cleaned->params.tip_kmers || cleaned->params.isolated_kmers)) || c.popping;
    if (const Selected *sel = q.selected) {
        const char *const who = "mtg_compact_unitigs_selected";
        const mtg_selection_params &p = sel->params;
        if (p.subtract_min_abundance < 1) MTG_DIE("%s: subtract_min_abundance must be >= 1", who);
        if (p.intersect_min_abundance < 1) MTG_DIE("%s: intersect_min_abundance must be >= 1", who);
        if (p.require & p.forbid) MTG_DIE("%s: require and forbid share colour %d", who, __builtin_ctzll(p.require & p.forbid));
        if (p.max_colors > MAX_COLORS) MTG_DIE("%s: max_colors %llu; at most %d", who, (unsigned long long)p.max_colors, MAX_COLORS);
        if (p.min_colors > p.max_colors) MTG_DIE("%s: min_colors %llu exceeds max_colors %llu", who, (unsigned long long)p.min_colors, (unsigned long long)p.max_colors);
        if (!counted) MTG_DIE("%s: a selection reports occurrences and needs the abundance and sums out-pointers", who);
        const bool colour_rule = p.require || p.forbid || p.min_colors > 0 || p.max_colors < MAX_COLORS;
        if (colour_rule && !colored) MTG_DIE("%s: require, forbid, min_colors and max_colors need the colours' out-pointers", who);
        if (colored && colored->n_colors < MAX_COLORS) {
            if (p.require >> colored->n_colors) MTG_DIE("%s: require names colour %d of %llu", who, 63 - __builtin_clzll(p.require), (unsigned long long)colored->n_colors);
            if (p.forbid >> colored->n_colors) MTG_DIE("%s: forbid names colour %d of %llu", who, 63 - __builtin_clzll(p.forbid), (unsigned long long)colored->n_colors);
        }
        const uint64_t fn = sel->filter_n;
        if (fn && (!sel->filter_off || !sel->filter_roles || (sel->filter_off[fn] && !sel->filter_data))) MTG_DIE("%s: null argument (filter records)", who);
        if (fn && sel->filter_off[0] != 0) MTG_DIE("%s: filter offsets must start at 0", who);
        for (uint64_t u = 0; u < fn; u++) {
            if (sel->filter_off[u + 1] < sel->filter_off[u]) MTG_DIE("%s: filter offsets decrease at record %llu", who, (unsigned long long)u);
            if (sel->filter_roles[u] > 1) MTG_DIE("%s: filter record %llu has role %u; 0 (subtract) and 1 (intersect) are served", who, (unsigned long long)u,
                                                  (unsigned)sel->filter_roles[u]);
            const uint64_t len = sel->filter_off[u + 1] - sel->filter_off[u];
            c.filter_records[sel->filter_roles[u]]++;
            if (len >= k) (sel->filter_roles[u] ? c.sel.intersect_windows : c.sel.subtract_windows) += len - k + 1;
        }
        if (c.sel.subtract_windows >= (1ull << 32) || c.sel.intersect_windows >= (1ull << 32))
            MTG_DIE("%s: %llu subtract and %llu intersect windows; the filter counters are 32-bit, the limit is 2^32 - 1 per role", who,
                    (unsigned long long)c.sel.subtract_windows, (unsigned long long)c.sel.intersect_windows);
        if (fn && sel->filter_off[fn] >= POS_LIMIT) MTG_DIE("%s: %llu filter bases; the limit is 2^40 - 2", who, (unsigned long long)sel->filter_off[fn]);
        c.selecting = true;
    }
    c.split = q.classed && q.classed->split;
}
// The one way out of a call, wherever its stages ended: the statistics, the times, the cleaning and the bubble results.
UnitigStore *finish(Call &c) {
    const CompactRequest &q = c.rq;
    c.t.total_ms = ms_since(c.t_total);
    if (q.stats_out) *q.stats_out = c.r;
    if (q.counted && q.counted->abundance) *q.counted->abundance = c.ab;
    if (q.times) *q.times = c.t;
    if (q.cleaned) {
        *q.cleaned->out = c.clean;
        *q.cleaned->clean_ms = c.clean_ms;
    }
    if (q.bubbles) {
        *q.bubbles->out = c.popped;
        *q.bubbles->bubble_ms = c.bubble_ms;
    }
    if (q.selected) *q.selected->out = c.sel;
    return c.store;
}
// The (k-1)-mer classes of the current k-mer set: key, and per side the incident oriented k-mer (NodeArgs). Assigning an empty one frees it.
struct NodeTable {
    hu::DeviceArray<unsigned long long> table;
    hu::DeviceArray<uint32_t> out_e, in_e;
};
// The device state of a call. Its constructor uploads and packs. The current k-mer set T has N k-mers (they shrink with the rounds of
// a cleaned call): kpos, and kcount / kcolor where the call counts / colours; `nodes`, succ and the (jump, rank) pairs are those of T.
struct Work {
    Call &c;
    hipStream_t st;
    SeqStore seq;
    ScalarBlock &small;  // [2] distinct k-mers, [3] changed, [4] cycle elements, [5] closed, [6] longest
    PhaseEvents<5> ev;   // the marks around insert, ids, (nodes, rank and the rounds), emit
    const uint64_t k, n_bases;
    uint64_t slots = 0, N = 0;  // slots of the k-mer table
    hu::DeviceArray<unsigned long long> kpos, kcolor;
    hu::DeviceArray<uint32_t> kcount;
    hu::DeviceArray<uint32_t> ksub, kint;  // selected calls, from ids to select: the filter counters of S_m's k-mers (empty: the role has no record)
    bool color_stats_done = false;         // selected calls: the statistics were taken over S_m and are with the caller already
    NodeTable nodes;
    hu::DeviceArray<uint32_t> succ;
    hu::DeviceArray<unsigned long long> pairs;
    int rankings = 0;
    Work(Call &call, hipStream_t stream)
        : c(call), st(stream), seq("sequences", call.rq.data, call.rq.off, call.rq.n_rec, stream, call.rq.device_id), small(seq.small), k(call.rq.k),
          n_bases(seq.n_bases) {}
    uint64_t n_or() const { return 2 * N; }
    unsigned int *err() const { return small.err(); }
    NodeArgs node_args() const {
        NodeArgs a{};
        a.packed = seq.packed; a.kpos = kpos; a.table = nodes.table; a.out_e = nodes.out_e; a.in_e = nodes.in_e; a.succ = succ;
        a.slots = std::max<uint64_t>(8, 4 * N);  // at most 2 N classes
        a.N = N; a.L = k - 1;
        return a;
    }
};
// The k-mer table of insert and what the rungs keep per slot: alive until ids has numbered the creators.
struct KmerTable {  // (members go back last to first: the table before the equally large masks, the order the arena's best fit has seen so far)
    KmerArgs ka{};
    hu::DeviceArray<unsigned long long> colors;  // [slots] coloured calls: the mask
    hu::DeviceArray<uint8_t> rec_colors;         // [n_rec] coloured calls
    hu::DeviceArray<uint32_t> count;             // [slots] counted calls: the abundance
    hu::DeviceArray<unsigned long long> table;   // [slots] = ka.table
};
// the instance of a kernel for the rung of the call (the arrays of a rung the call does not climb are null) and for k
void launch_insert(const Work &w, const KmerTable &kt) {
    const bool wide = w.k >= 32;
    auto *kernel = kt.colors  ? (wide ? insert_kernel<true, true, true> : insert_kernel<false, true, true>)
                   : kt.count ? (wide ? insert_kernel<true, true, false> : insert_kernel<false, true, false>)
                              : (wide ? insert_kernel<true, false, false> : insert_kernel<false, false, false>);
    kernel<<<hu::grid_for((w.n_bases + RUN - 1) / RUN), hu::EB, 0, w.st>>>(kt.ka, w.n_bases, w.c.rq.n_rec, w.err(), kt.count, kt.rec_colors, kt.colors);
    HIP_CHECK(hipGetLastError());
}
void launch_mark(const Work &w, const KmerTable &kt, uint32_t *flag) {
    auto *kernel = kt.count ? mark_kernel<true> : mark_kernel<false>;
    kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(w.slots), 16384), hu::EB, 0, w.st>>>(kt.table, w.slots, flag, w.small.d + 2, kt.count, w.c.m);
    HIP_CHECK(hipGetLastError());
}
void launch_kpos(const Work &w, const KmerTable &kt, const uint32_t *id_of_pos) {
    auto *kernel = kpos_kernel<true, true>;
    if (!kt.colors) kernel = kt.count ? kpos_kernel<true, false> : kpos_kernel<false, false>;
    kernel<<<hu::grid_for(w.slots), hu::EB, 0, w.st>>>(kt.table, w.slots, id_of_pos, w.kpos, kt.count, w.c.m, w.kcount, kt.colors, w.kcolor);
    HIP_CHECK(hipGetLastError());
}

// Stage 2, insert: the creator of every k-mer class; a counted call also gets, from one sweep of the abundances per slot, the spectrum
// before the filter (booked under ids_ms: mark 1 lies in front of it).
KmerTable insert(Work &w) {
    Call &c = w.c;
    const uint64_t slots = w.slots = std::max<uint64_t>(8, (2 * c.r.windows + 7) / 8 * 8), n_rec = c.rq.n_rec;
    KmerTable kt;
    kt.ka.packed = w.seq.packed; kt.ka.off = w.seq.off; kt.ka.slots = slots;
    kw::window_args_set_k(kt.ka, w.k);
    kt.ka.table = kt.table.alloc(slots);
    HIP_CHECK(hipMemsetAsync(kt.table, 0xFF, slots * 8, w.st));
    if (c.rq.counted) {
        kt.count.alloc(slots);
        HIP_CHECK(hipMemsetAsync(kt.count, 0, slots * 4, w.st));
    }
    if (c.rq.colored) {
        kt.rec_colors.alloc(n_rec);
        kt.colors.alloc(slots);
        hu::upload_sliced(kt.rec_colors, c.rq.colored->record_colors, n_rec, w.st, c.rq.device_id);
        HIP_CHECK(hipMemsetAsync(kt.colors, 0, slots * 8, w.st));
    }
    launch_insert(w, kt);
    w.ev.mark(1, w.st);
    if (c.rq.counted) {
        std::vector<unsigned long long> h_spec(SPECTRUM_BINS + 2);
        hu::DeviceArray<unsigned long long> spec(h_spec.size());
        HIP_CHECK(hipMemsetAsync(spec, 0, h_spec.size() * 8, w.st));
        spectrum_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(slots), 4096), hu::EB, 0, w.st>>>(kt.count, slots, c.m, spec);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(h_spec.data(), spec, h_spec.size() * 8, hipMemcpyDeviceToHost, w.st));
        HIP_CHECK(hipStreamSynchronize(w.st));
        for (int b = 0; b < SPECTRUM_BINS; b++) c.ab.distinct_all += c.ab.spectrum[b] = h_spec[b];
        c.ab.max_abundance = h_spec[SPECTRUM_BINS];
        c.ab.kept_occurrences = h_spec[SPECTRUM_BINS + 1];
    }
    return kt;
}

// The filter counters per slot of the k-mer table (selected calls): zeroed, one array per role that occurs. They go back with the table.
struct FilterCounts {
    hu::DeviceArray<uint32_t> sub, inter;  // [slots]
};
// Stage 2b, filter (selected calls with filter records): the filter store packed on its own, every window of it looked
// up in the live table. Its packed text goes back here, the counters with the caller's scope. Books filter_ms and the hits.
FilterCounts filter_probe(Work &w, const KmerTable &kt) {
    Call &c = w.c;
    const Selected &sel = *c.rq.selected;
    FilterCounts fc;
    PhaseEvents<2> fe;
    if (c.filter_records[0]) {
        fc.sub.alloc(w.slots);
        HIP_CHECK(hipMemsetAsync(fc.sub, 0, w.slots * 4, w.st));
    }
    if (c.filter_records[1]) {
        fc.inter.alloc(w.slots);
        HIP_CHECK(hipMemsetAsync(fc.inter, 0, w.slots * 4, w.st));
    }
    unsigned long long h_hits[2] = {0, 0};
    if (c.sel.subtract_windows + c.sel.intersect_windows) {  // (else no record is as long as k: the counters stay zero)
        SeqStore fs("filter sequences", sel.filter_data, sel.filter_off, sel.filter_n, w.st, c.rq.device_id);
        fe.mark(0, w.st);
        hu::DeviceArray<uint8_t> roles(sel.filter_n);
        hu::DeviceArray<unsigned long long> hits(2);
        hu::upload_sliced(roles, sel.filter_roles, sel.filter_n, w.st, c.rq.device_id);
        HIP_CHECK(hipMemsetAsync(hits, 0, sizeof h_hits, w.st));
        kw::WindowArgs fa{};
        fa.packed = fs.packed; fa.off = fs.off;
        kw::window_args_set_k(fa, w.k);
        auto *kernel = w.k >= 32 ? filter_probe_kernel<true> : filter_probe_kernel<false>;
        kernel<<<hu::grid_for((fs.n_bases + RUN - 1) / RUN), hu::EB, 0, w.st>>>(kt.ka, fa, fs.n_bases, sel.filter_n, roles, fc.sub, fc.inter, hits);
        HIP_CHECK(hipGetLastError());
        fe.mark(1, w.st);
        HIP_CHECK(hipMemcpyAsync(h_hits, hits, sizeof h_hits, hipMemcpyDeviceToHost, w.st));
        HIP_CHECK(hipStreamSynchronize(w.st));
        c.t.filter_ms = fe.ms(0, 1);
    }
    c.sel.subtract_hits = h_hits[0];
    c.sel.intersect_hits = h_hits[1];
    if (h_hits[0] > c.sel.subtract_windows || h_hits[1] > c.sel.intersect_windows)
        MTG_DIE("unitig compaction: internal error (%llu and %llu filter hits in %llu and %llu windows)", h_hits[0], h_hits[1],
                (unsigned long long)c.sel.subtract_windows, (unsigned long long)c.sel.intersect_windows);
    return fc;
}

// Stage 3, ids: the creators flagged and scanned -> dense ids in creator order: N, kpos (kcount, kcolor). false: no k-mer is kept
// (a counted call whose threshold none reaches). The flags and the scan's scratch go back here, the table with the caller's scope.
bool ids(Work &w, const KmerTable &kt, const FilterCounts &fc) {
    Call &c = w.c;
    hu::DeviceArray<uint32_t> id_of_pos(w.n_bases);
    HIP_CHECK(hipMemsetAsync(id_of_pos, 0, w.n_bases * 4, w.st));
    launch_mark(w, kt, id_of_pos);
    w.small.read(w.st, STAGE);
    c.t.insert_ms = w.ev.ms(0, 1);  // (over: the read has waited for the stream)
    const uint64_t N = w.N = c.r.distinct_kmers = w.small.h[2];
    if (N > MAX_KMERS) MTG_DIE("mtg_compact_unitigs: %llu distinct k-mers; oriented k-mer ids are 32-bit", (unsigned long long)N);
    if (c.rq.counted) c.ab.distinct_kept = N;
    if (N == 0) return false;
    hu::ScanScratch<uint32_t> scan(w.n_bases);
    w.kpos.alloc(N);
    scan.scan(w.st, id_of_pos, w.n_bases, id_of_pos);
    if (c.rq.counted) w.kcount.alloc(N);
    if (c.rq.colored) w.kcolor.alloc(N);
    launch_kpos(w, kt, id_of_pos);
    if (fc.sub || fc.inter) {
        if (fc.sub) w.ksub.alloc(N);
        if (fc.inter) w.kint.alloc(N);
        kpos_filter_kernel<<<hu::grid_for(w.slots), hu::EB, 0, w.st>>>(kt.table, w.slots, id_of_pos, kt.count, c.m, fc.sub, fc.inter, w.ksub, w.kint);
        HIP_CHECK(hipGetLastError());
    }
    w.ev.mark(2, w.st);
    return true;
}

// the words of color_stats_kernel as the caller's statistics
void take_color_stats(const std::vector<unsigned long long> &h, mtg_color_stats &cs) {
    for (int i = 0; i < MAX_COLORS; i++) {
        cs.per_color[i] = h[i * MAX_COLORS + i];
        for (int j = 0; j < MAX_COLORS; j++) cs.shared[i * MAX_COLORS + j] = h[i * MAX_COLORS + j];
    }
    for (int j = 0; j <= MAX_COLORS; j++) cs.occupancy[j] = h[COLOR_OCC + j];
}
// Stage 4, nodes: the table of T's (k-1)-mer classes with their incident words, and room for succ
void build_nodes(Work &w) {
    const uint64_t slots = std::max<uint64_t>(8, 4 * w.N);
    w.nodes.table.alloc(slots);
    w.nodes.out_e.alloc(slots);
    w.nodes.in_e.alloc(slots);
    w.succ.alloc(w.n_or());
    HIP_CHECK(hipMemsetAsync(w.nodes.table, 0xFF, slots * 8, w.st));
    HIP_CHECK(hipMemsetAsync(w.nodes.out_e, 0xFF, slots * 4, w.st));
    HIP_CHECK(hipMemsetAsync(w.nodes.in_e, 0xFF, slots * 4, w.st));
    node_insert_kernel<<<hu::grid_for(w.N), hu::EB, 0, w.st>>>(w.node_args(), w.err());
}
// at most max_rounds rounds of pointer jumping over all n elements or those of `list` -> true: settled
bool jump_rounds(Work &w, uint64_t n, const uint32_t *list, int max_rounds) {
    unsigned int *d_changed = reinterpret_cast<unsigned int *>(w.small.d + 3);
    for (int i = 0; i < max_rounds; i++) {
        HIP_CHECK(hipMemsetAsync(d_changed, 0, 4, w.st));
        jump_kernel<<<hu::grid_for(n), hu::EB, 0, w.st>>>(w.pairs, n, list, d_changed);
        HIP_CHECK(hipGetLastError());
        w.c.t.rounds++;
        w.small.read(w.st, STAGE);
        if (!(w.small.h[3] & 0xFFFFFFFFull)) return true;
    }
    return false;
}
// What still moves once every chain has settled lies on closed walks: list, minimum per cycle, cut in front of it, rank like chains.
void rank_closed_walks(Work &w, bool again) {
    const uint64_t n_or = w.n_or();
    hu::DeviceArray<uint32_t> list(n_or);
    if (again) HIP_CHECK(hipMemsetAsync(w.small.d + 4, 0, 8, w.st));  // (an earlier ranking has counted its own)
    cycle_list_kernel<<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.pairs, w.succ, n_or, list, w.small.d + 4);
    HIP_CHECK(hipGetLastError());
    w.small.read(w.st, STAGE);
    const uint64_t C = w.small.h[4];
    if (C == 0 || C > n_or) MTG_DIE("unitig compaction: internal error (%llu elements on closed walks)", (unsigned long long)C);
    hu::DeviceArray<unsigned long long> buf(n_or);
    cycle_min_init_kernel<<<hu::grid_for(C), hu::EB, 0, w.st>>>(w.succ, list, C, w.pairs);
    unsigned long long *src = w.pairs, *dst = buf;
    for (int i = 0, n = log2_ceil(C); i < n; i++, w.c.t.rounds++) {
        cycle_min_kernel<<<hu::grid_for(C), hu::EB, 0, w.st>>>(src, dst, list, C);
        std::swap(src, dst);
    }
    cycle_cut_kernel<<<hu::grid_for(C), hu::EB, 0, w.st>>>(src, w.succ, list, C, w.pairs);
    HIP_CHECK(hipGetLastError());
    if (!jump_rounds(w, C, list, log2_ceil(C) + 2)) MTG_DIE("unitig compaction: internal error (a cut cycle does not settle)");
}
// Stage 5, rank: pointer jumping over succ
void rank(Work &w) {
    const bool again = w.rankings++ > 0;
    if (!w.pairs) w.pairs.alloc(w.n_or());
    rank_init_kernel<<<hu::grid_for(w.n_or()), hu::EB, 0, w.st>>>(w.succ, w.n_or(), w.pairs);
    HIP_CHECK(hipGetLastError());
    if (!jump_rounds(w, w.n_or(), nullptr, log2_ceil(w.n_or()) + 2)) rank_closed_walks(w, again);
}
// Stages 4 and 5 over T. ROUND: a cleaning round's pass -- unsplit, and the node table stays for the decision to probe; FINAL: the
// pass emit reads; SPLIT_AGAIN: succ<true> and rank once more over the node table of a round that removed nothing.
enum class Pass { ROUND, FINAL, SPLIT_AGAIN };
void pass(Work &w, Pass kind) {
    PhaseEvents<3> pe;
    pe.mark(0, w.st);
    if (kind != Pass::SPLIT_AGAIN) build_nodes(w);
    if (w.c.split && kind != Pass::ROUND) succ_kernel<true><<<hu::grid_for(w.N), hu::EB, 0, w.st>>>(w.node_args(), w.err(), w.kcolor);
    else succ_kernel<false><<<hu::grid_for(w.N), hu::EB, 0, w.st>>>(w.node_args(), w.err(), nullptr);
    HIP_CHECK(hipGetLastError());
    pe.mark(1, w.st);
    if (kind != Pass::ROUND) w.nodes = NodeTable{};  // (it goes back in front of rank; a round's decision probes it once more)
    if (kind != Pass::SPLIT_AGAIN) w.small.read(w.st, STAGE);
    rank(w);
    pe.mark(2, w.st);
    w.c.t.nodes_ms += pe.ms(0, 1);
    w.c.t.rank_ms += pe.ms(1, 2);
}

// Stage 6, one cleaning round on the snapshot of pass(ROUND): verdicts per walk end (tips and isolated walks, then the weaker arms
// of bubbles), keep flags per k-mer (keep: [N], for the move). Books the round's counters and times -> the k-mers it removes.
uint64_t clean_round(Work &w, hu::DeviceArray<uint32_t> &keep) {
    Call &c = w.c;
    const uint64_t N = w.N, n_or = w.n_or();
    PhaseEvents<2> ce;
    unsigned long long h[CLEAN_COUNTERS] = {};
    hu::DeviceArray<uint8_t> verdict(n_or);
    keep.alloc(N);
    hu::DeviceArray<unsigned long long> counters(CLEAN_COUNTERS);
    HIP_CHECK(hipMemsetAsync(verdict, 0, n_or, w.st));
    HIP_CHECK(hipMemsetAsync(counters, 0, sizeof h, w.st));
    ce.mark(0, w.st);
    clean_decide_kernel<<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.node_args(), w.pairs, n_or, c.rq.cleaned->params.tip_kmers, c.rq.cleaned->params.isolated_kmers,
                                                                verdict, counters, w.err());
    double round_bubble_ms = 0;
    if (c.popping) {  // (the same snapshot: tips and arms are disjoint, both of an arm's ends are anchored)
        PhaseEvents<2> be;
        be.mark(0, w.st);
        pop_bubbles(w.node_args(), w.pairs, w.kcount, c.rq.bubbles->params, verdict, counters + 7, w.err(), w.st);
        be.mark(1, w.st);
        clean_keep_kernel<true><<<hu::grid_for(N), hu::EB, 0, w.st>>>(w.pairs, verdict, w.kcount, N, keep, counters);
        round_bubble_ms = be.ms(0, 1);
    } else {
        clean_keep_kernel<false><<<hu::grid_for(N), hu::EB, 0, w.st>>>(w.pairs, verdict, w.kcount, N, keep, counters);
    }
    HIP_CHECK(hipGetLastError());
    ce.mark(1, w.st);
    HIP_CHECK(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, w.st));
    w.small.read(w.st, STAGE);
    c.clean_ms += ce.ms(0, 1) - round_bubble_ms;  // (nested marks on one stream)
    c.bubble_ms += round_bubble_ms;
    c.clean.rounds_run++;
    c.clean.tips += h[0];
    c.clean.isolated += h[1];
    c.clean.tip_kmers += h[2];
    c.clean.isolated_kmers += h[3];
    c.clean.removed_occurrences += h[4];
    c.popped.arm_kmers += h[5];
    c.popped.removed_occurrences += h[6];
    c.popped.arms += h[7];
    const uint64_t removed = h[2] + h[3] + h[5];
    if (removed > N) MTG_DIE("unitig compaction: internal error (%llu of %llu k-mers removed)", (unsigned long long)removed, (unsigned long long)N);
    return removed;
}
// Stage 7: the scan of the keep flags gives the survivors' new ids (creator order is kept); kpos, kcount and kcolor move there and T
// shrinks. The node table, succ and the pairs of the old ids are gone by now. booked_ms: the clock of the stage that removes.
void move_survivors(Work &w, const uint32_t *keep, uint64_t removed, double &booked_ms) {
    Call &c = w.c;
    const uint64_t N = w.N, N_left = N - removed;
    if (N_left) {
        PhaseEvents<2> me;
        hu::DeviceArray<uint32_t> new_id(N);
        hu::ScanScratch<uint32_t> scan(N);
        hu::DeviceArray<unsigned long long> kpos_to(N_left), kcolor_to;
        hu::DeviceArray<uint32_t> kcount_to;
        if (w.kcount) kcount_to.alloc(N_left);
        if (w.kcolor) kcolor_to.alloc(N_left);
        uint32_t n_left = 0;
        me.mark(0, w.st);
        scan.scan(w.st, keep, N, new_id);
        clean_move_kernel<<<hu::grid_for(N), hu::EB, 0, w.st>>>(keep, new_id, N, w.kpos, w.kcount, w.kcolor, kpos_to, kcount_to, kcolor_to);
        HIP_CHECK(hipGetLastError());
        me.mark(1, w.st);
        HIP_CHECK(hipMemcpyAsync(&n_left, scan.total(), 4, hipMemcpyDeviceToHost, w.st));
        HIP_CHECK(hipStreamSynchronize(w.st));
        booked_ms += me.ms(0, 1);
        if (n_left != N_left) MTG_DIE("unitig compaction: internal error (%llu k-mers kept, %llu counted)", (unsigned long long)n_left, (unsigned long long)N_left);
        w.kpos = std::move(kpos_to);
        w.kcount = std::move(kcount_to);
        w.kcolor = std::move(kcolor_to);
    }
    w.N = c.r.distinct_kmers = N_left;
}
// Stage 3b, select (selected calls), over the ids of S_m and in front of the first pass: the colour statistics of a
// coloured call (over S_m: they are how a carrier threshold is chosen), the keep flags of the five rules with their counters, then the
// scan and the move of a cleaning round. The filter counters go back here. false: nothing is selected.
bool select(Work &w) {
    Call &c = w.c;
    const Colored *colored = c.rq.colored;
    const mtg_selection_params &p = c.rq.selected->params;
    const uint64_t N = w.N;
    const int device_id = c.rq.device_id;
    if (colored) {
        PhaseEvents<2> ev_stats;
        std::vector<unsigned long long> h(COLOR_STATS_WORDS);
        hu::DeviceArray<unsigned long long> color_stats(COLOR_STATS_WORDS);
        HIP_CHECK(hipMemsetAsync(color_stats, 0, COLOR_STATS_WORDS * 8, w.st));
        ev_stats.mark(0, w.st);
        color_stats_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(N), 512), hu::EB, 0, w.st>>>(w.kcolor, N, (int)colored->n_colors, color_stats);
        ev_stats.mark(1, w.st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(w.st));
        hu::download_sliced(h.data(), color_stats, h.size() * 8, w.st, device_id);
        *colored->stats_ms = ev_stats.ms(0, 1);
        take_color_stats(h, *colored->stats);
        w.color_stats_done = true;
    }
    PhaseEvents<2> se;
    unsigned long long h[SELECT_WORDS] = {};
    hu::DeviceArray<uint32_t> keep(N);
    hu::DeviceArray<unsigned long long> counters(SELECT_WORDS);
    HIP_CHECK(hipMemsetAsync(counters, 0, sizeof h, w.st));
    se.mark(0, w.st);
    const SelectArgs sa{p.require, p.forbid, p.min_colors, p.max_colors, p.subtract_min_abundance, p.intersect_min_abundance};
    select_keep_kernel<<<hu::grid_for(N), hu::EB, 0, w.st>>>(w.kcolor, w.kcount, w.ksub, w.kint, sa, colored ? (int)colored->n_colors : 0, N, keep, counters);
    HIP_CHECK(hipGetLastError());
    se.mark(1, w.st);
    HIP_CHECK(hipMemcpyAsync(h, counters, sizeof h, hipMemcpyDeviceToHost, w.st));
    w.small.read(w.st, STAGE);
    c.t.select_ms = se.ms(0, 1);
    w.ksub.release();
    w.kint.release();
    mtg_selection &s = c.sel;
    s.input_kmers = N;
    s.rejected_forbid = h[0]; s.rejected_require = h[1]; s.rejected_carriers = h[2]; s.rejected_subtract = h[3]; s.rejected_intersect = h[4];
    s.selected = h[5];
    s.selected_occurrences = h[6];
    for (int b = 0; b < MAX_COLORS; b++) s.per_color_selected[b] = h[SELECT_COLOR + b];
    if (h[0] + h[1] + h[2] + h[3] + h[4] + h[5] != N)
        MTG_DIE("unitig compaction: internal error (%llu k-mers rejected and %llu selected of %llu)", h[0] + h[1] + h[2] + h[3] + h[4], h[5], (unsigned long long)N);
    if (s.selected < N) move_survivors(w, keep, N - s.selected, c.t.select_ms);
    return w.N > 0;
}
// The rounds of a cleaned call and how they end.
enum class Rounds {
    SETTLED,      // a round removed nothing: its succ and ranks are the final ones (after the extra pass where the unitigs are to be split)
    USED_UP,      // the last allowed round removed something: one more pass over the survivors follows
    NOTHING_LEFT  // everything was a tip or isolated (an arm's best stays: popping alone never gets here)
};
Rounds clean_rounds(Work &w) {
    for (;;) {
        pass(w, Pass::ROUND);
        hu::DeviceArray<uint32_t> keep;
        const uint64_t removed = clean_round(w, keep);
        if (removed == 0) {
            keep.release();
            if (w.c.split) pass(w, Pass::SPLIT_AGAIN);
            else w.nodes = NodeTable{};
            return Rounds::SETTLED;
        }
        w.nodes = NodeTable{};
        w.succ.release();
        w.pairs.release();
        move_survivors(w, keep, removed, w.c.clean_ms);
        if (w.N == 0) return Rounds::NOTHING_LEFT;
        if (w.c.clean.rounds_run == w.c.rq.cleaned->params.rounds) return Rounds::USED_UP;
    }
}
// The device arrays of the output: those of emit, the sums of a counted call, the ordered masks and statistics of a coloured one.
// They stay until the downloads are done.
struct Output {
    hu::DeviceArray<uint32_t> wmin, wlen, lead_flag, lead_chars;  // [2 N] per head, [N] per leader (lead_flag: scanned in place to the unitig number)
    hu::DeviceArray<uint64_t> char_off;                           // [N]
    hu::ScanScratch<uint32_t> scan32;                             // its total: the unitigs
    hu::ScanScratch<uint64_t> scan64;                             // its total: the characters, then the occurrences
    hu::DeviceArray<char> chars;
    hu::DeviceArray<unsigned long long> off, sums, ordered_colors, color_stats;
    hu::DeviceArray<uint32_t> ordered;  // counted calls: the abundances in unitig order
    uint64_t n_chars = 0;
    explicit Output(uint64_t N) : wmin(2 * N), wlen(2 * N), lead_flag(N), lead_chars(N), char_off(N), scan32(N), scan64(N) {}
};
// Stage 8, emit: walk, leader, the two scans, offsets, spell
Output emit(Work &w) {
    mtg_compaction &r = w.c.r;
    const uint64_t N = w.N, n_or = w.n_or(), k = w.k;
    Output o(N);
    HIP_CHECK(hipMemsetAsync(o.wmin, 0xFF, n_or * 4, w.st));
    HIP_CHECK(hipMemsetAsync(o.wlen, 0, n_or * 4, w.st));
    HIP_CHECK(hipMemsetAsync(o.lead_flag, 0, N * 4, w.st));
    HIP_CHECK(hipMemsetAsync(o.lead_chars, 0, N * 4, w.st));
    walk_kernel<<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.pairs, w.succ, n_or, o.wmin, o.wlen);
    leader_kernel<<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.pairs, w.succ, n_or, o.wmin, o.wlen, (uint32_t)k, o.lead_flag, o.lead_chars, w.small.d + 5);
    o.scan32.scan(w.st, o.lead_flag, N, o.lead_flag);
    o.scan64.scan(w.st, o.lead_chars, N, o.char_off);
    uint32_t n_unitigs = 0;
    HIP_CHECK(hipMemcpyAsync(&n_unitigs, o.scan32.total(), 4, hipMemcpyDeviceToHost, w.st));
    HIP_CHECK(hipMemcpyAsync(&o.n_chars, o.scan64.total(), 8, hipMemcpyDeviceToHost, w.st));
    w.small.read(w.st, STAGE);
    r.unitigs = n_unitigs;
    r.unitig_characters = o.n_chars;
    r.closed_walks = w.small.h[5];
    r.longest_unitig_kmers = w.small.h[6];
    if (o.n_chars != N + (k - 1) * r.unitigs) MTG_DIE("unitig compaction: internal error (%llu characters for %llu k-mers in %llu unitigs)",
                                                      (unsigned long long)o.n_chars, (unsigned long long)N, (unsigned long long)r.unitigs);
    o.chars.alloc(o.n_chars);
    o.off.alloc(r.unitigs + 1);
    offsets_kernel<<<hu::grid_for(N), hu::EB, 0, w.st>>>(o.lead_chars, o.lead_flag, o.char_off, N, o.off);
    spell_kernel<<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.seq.packed, w.kpos, w.pairs, o.wmin, o.char_off, n_or, k, o.chars);
    HIP_CHECK(hipGetLastError());
    return o;
}

// Stage 9. Counted calls: the abundances in unitig order, their 64-bit prefix sums (emit's 64-bit scratch is free again, and N is
// the same), differences at the unitig boundaries; `ordered` stays only where the call hands out the counts. Coloured calls: the
// masks in unitig order, and the statistics over kcolor (any order serves).
void sums_and_colors(Work &w, Output &o) {
    const Counted *counted = w.c.rq.counted;
    const Colored *colored = w.c.rq.colored;
    const uint64_t N = w.N, n_or = w.n_or(), unitigs = w.c.r.unitigs;
    if (counted) {
        o.ordered.alloc(N);
        hu::DeviceArray<uint64_t> prefix(N);
        o.sums.alloc(unitigs);
        order_counts_kernel<uint32_t><<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.pairs, o.wmin, o.char_off, o.lead_flag, w.kcount, n_or, w.k, o.ordered);
        o.scan64.scan(w.st, o.ordered, N, prefix);
        unitig_sums_kernel<<<hu::grid_for(unitigs), hu::EB, 0, w.st>>>(o.off, prefix, o.scan64.total(), unitigs, w.k, o.sums);
        HIP_CHECK(hipGetLastError());
        if (!counted->kmer_counts) o.ordered.release();
    }
    if (colored) {
        o.ordered_colors.alloc(N);
        order_counts_kernel<unsigned long long><<<hu::grid_for(n_or), hu::EB, 0, w.st>>>(w.pairs, o.wmin, o.char_off, o.lead_flag, w.kcolor, n_or, w.k, o.ordered_colors);
        if (!w.color_stats_done) {  // (a selected call has taken them over S_m)
            PhaseEvents<2> ev_stats;
            o.color_stats.alloc(COLOR_STATS_WORDS);
            HIP_CHECK(hipMemsetAsync(o.color_stats, 0, COLOR_STATS_WORDS * 8, w.st));
            ev_stats.mark(0, w.st);
            color_stats_kernel<<<(unsigned)std::min<uint64_t>(hu::grid_for(N), 512), hu::EB, 0, w.st>>>(w.kcolor, N, (int)colored->n_colors, o.color_stats);
            ev_stats.mark(1, w.st);
            HIP_CHECK(hipGetLastError());
            *colored->stats_ms = ev_stats.ms(0, 1);
        }
    }
}
// Stage 10: the store, and what the rungs of the call hand out
void download(Work &w, const Output &o) {
    Call &c = w.c;
    const Counted *counted = c.rq.counted;
    const Colored *colored = c.rq.colored;
    const uint64_t N = w.N, unitigs = c.r.unitigs;
    const int device_id = c.rq.device_id;
    const auto t0 = std::chrono::steady_clock::now();
    c.store->data.resize(o.n_chars);
    c.store->off.resize(unitigs + 1);
    hu::download_sliced(&c.store->data[0], o.chars, o.n_chars, w.st, device_id);
    hu::download_sliced(c.store->off.data(), o.off, unitigs * 8, w.st, device_id);
    c.store->off[unitigs] = o.n_chars;
    if (counted) {
        counted->sums->resize(unitigs);
        hu::download_sliced(counted->sums->data(), o.sums, unitigs * 8, w.st, device_id);
        if (counted->kmer_counts) {  // (`ordered` itself: unitig order is the store's window order)
            counted->kmer_counts->resize(N);
            hu::download_sliced(counted->kmer_counts->data(), o.ordered, N * 4, w.st, device_id);
        }
    }
    if (colored) {
        if (!w.color_stats_done) {
            std::vector<unsigned long long> h(COLOR_STATS_WORDS);
            hu::download_sliced(h.data(), o.color_stats, h.size() * 8, w.st, device_id);
            take_color_stats(h, *colored->stats);
        }
        colored->kmer_colors->resize(N);
        hu::download_sliced(colored->kmer_colors->data(), o.ordered_colors, N * 8, w.st, device_id);
    }
    c.t.download_ms = ms_since(t0);
}

// The stages of a call with bases, top to bottom. Every return leaves through finish(); what a stage booked by then is what the
// call reports. Device arrays go back where their owner's scope ends: the k-mer table behind ids, everything else behind the downloads.
void run(Call &c) {
    const CompactRequest &q = c.rq;
    if (c.r.characters >= POS_LIMIT) MTG_DIE("mtg_compact_unitigs: %llu bases; the limit is 2^40 - 2", (unsigned long long)c.r.characters);
    if (q.device_id < 0 || device_count() <= q.device_id) MTG_DIE("no HIP device %d for the unitig compaction (there is no CPU path)", q.device_id);
    HIP_CHECK(hipSetDevice(q.device_id));
    device_arena_reset_peak(q.device_id);
    Work w(c, nullptr);  // upload and pack
    c.t.upload_ms = w.seq.upload_ms;
    c.t.pack_ms = w.seq.pack_ms;
    if (c.r.windows == 0) return;  // nothing is as long as k
    w.ev.mark(0, w.st);
    {
        const KmerTable kt = insert(w);
        const FilterCounts fc = c.selecting && c.rq.selected->filter_n ? filter_probe(w, kt) : FilterCounts{};
        if (!ids(w, kt, fc)) return;
    }
    c.t.ids_ms = w.ev.ms(1, 2) - c.t.filter_ms;
    if (c.selecting && !select(w)) return;
    // nodes, succ and rank: once, or in a cleaned call once per round and, unless a round settled it, once more over the final set
    const Rounds rounds = c.cleaning ? clean_rounds(w) : Rounds::USED_UP;
    if (rounds == Rounds::NOTHING_LEFT) return;
    if (rounds == Rounds::USED_UP) pass(w, Pass::FINAL);
    w.ev.mark(3, w.st);
    Output o = emit(w);
    sums_and_colors(w, o);
    w.ev.mark(4, w.st);
    HIP_CHECK(hipStreamSynchronize(w.st));
    if (q.classed) color_classes(o.ordered_colors, o.off, w.N, c.r.unitigs, w.k, q.classed->split, w.st, w.small, q.device_id, q.classed->out, q.classed->times);
    download(w, o);
    c.t.emit_ms = w.ev.ms(3, 4);
    uint64_t arena[4];
    device_arena_stats(q.device_id, arena);
    c.t.peak_arena_bytes = arena[2];
    // What the kernels must move at the least: ASCII read and packed store written; per window the packed bases once (2 bits) and one
    // slot; the table filled, then read twice (mark, kpos); per base the flag word written, scanned (read + written) and read per
    // creator; per distinct k-mer its creator written and read twice with 2 (k + 15) / 16 packed words each time, two node slots
    // and two incident words written and read, two succ words; per oriented k-mer one pair per round at the least (read), succ and the
    // pair in the emit kernels, wmin / wlen; per leader flag, length and offset; and the output characters and offsets.
    const uint64_t n_bases = w.n_bases, N = w.N, n_or = w.n_or(), k = w.k;
    c.t.bytes = n_bases + w.seq.n_words * 4 + c.r.windows * 8 + w.seq.n_words * 4 + w.slots * 8 * 3 + n_bases * 4 * 3 + N * 4 +
                N * (8 * 3 + 2 * 4 * ((k + 15) / 16 + 1) + 2 * (8 + 4) * 2 + 8) + n_or * 8 * (uint64_t)std::max(c.t.rounds, 1) +
                n_or * (4 + 8 + 8 + 8 + 4) + N * (4 * 3 + 4 * 2 + 8 * 2) + o.n_chars + c.r.unitigs * 8;  // (of a cleaned call: the final pass alone)
}

}  // namespace

UnitigStore *device_compact_unitigs(const CompactRequest &rq) {
    const Counted *cn = rq.counted;
    const Colored *col = rq.colored;
    const Classed *cl = rq.classed;
    if ((cn && !cn->sums) || (col && (!cn || !cn->kmer_counts || !col->kmer_colors || !col->stats || !col->stats_ms)) ||
        (cl && (!col || !cl->out || !cl->times)))
        MTG_DIE("%s: null argument", rq.who);
    if (rq.cleaned && (!rq.cleaned->out || !rq.cleaned->clean_ms)) MTG_DIE("%s: null argument", rq.who);
    if (rq.bubbles && (!rq.bubbles->out || !rq.bubbles->bubble_ms)) MTG_DIE("%s: null argument", rq.who);
    Call c{rq};
    check_request(c);
    if (c.r.characters) run(c);
    return finish(c);
}

void device_color_classes(const uint64_t *kmer_colors, uint64_t n, const uint64_t *unitig_kmers, uint64_t n_unitigs, int device_id, ColorClasses *out,
                          ColorClassTimes *times) {
    if (!out || !times || (n && !kmer_colors) || (n_unitigs && !unitig_kmers)) MTG_DIE("mtg_color_classes_build: null argument");
    *out = ColorClasses{};
    *times = ColorClassTimes{};
    if (n > MAX_KMERS) MTG_DIE("mtg_color_classes_build: %llu k-mers; window numbers are 32-bit", (unsigned long long)n);
    std::vector<unsigned long long> off(n_unitigs + 1, 0);  // window offsets: character offsets at k = 1
    for (uint64_t u = 0; u < n_unitigs; u++) {
        if (unitig_kmers[u] == 0 || unitig_kmers[u] > n - off[u]) MTG_DIE("mtg_color_classes_build: unitig %llu has %llu k-mers of the %llu left",
                                                                         (unsigned long long)u, (unsigned long long)unitig_kmers[u], (unsigned long long)(n - off[u]));
        off[u + 1] = off[u] + unitig_kmers[u];
    }
    if (off[n_unitigs] != n) MTG_DIE("mtg_color_classes_build: the unitigs hold %llu k-mers, the masks %llu", (unsigned long long)off[n_unitigs], (unsigned long long)n);
    for (uint64_t i = 0; i < n; i++)
        if (kmer_colors[i] == 0) MTG_DIE("mtg_color_classes_build: k-mer %llu has the empty mask", (unsigned long long)i);
    if (n == 0) return;
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the colour classes (there is no CPU path)", device_id);
    HIP_CHECK(hipSetDevice(device_id));
    hipStream_t st = nullptr;
    ScalarBlock small(st);
    hu::DeviceArray<unsigned long long> d_masks(n), d_off(n_unitigs + 1);
    hu::upload_sliced(d_masks, kmer_colors, n * 8, st, device_id);
    hu::upload_sliced(d_off, off.data(), (n_unitigs + 1) * 8, st, device_id);
    color_classes(d_masks, d_off, n, n_unitigs, 1, false, st, small, device_id, out, times);
}

uint64_t device_color_class_limit(int which) { return which == 0 ? CLASS_LDS : which == 1 ? CLASS_GRID : hu::EB; }

}  // namespace mtg
