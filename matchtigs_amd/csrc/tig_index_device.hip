// tig_index_device.hip -- a k-mer dictionary the size of the tigs: the sparse minimizer index (mtg_tig_index_*)
//
// The contract is the k-mer index's (kmer_query_device.hip): the INDEX is a sequence set, its k-mers the windows of length k inside
// one record, taken by their class {x, rc(x)}; a QUERY is n records of arbitrary bytes and gets kmers / valid / found per record and
// the two bit arrays, word for word what mtg_kmer_index_query gives. What differs is what the index keeps: not a table slot per
// window but the 2-bit packed bases themselves plus one 8-byte word per ANCHOR, about 2 / (k - m + 2) of the windows.
//
// Definitions. 1 <= m <= min(k, 31), w = k - m + 1. The m-mer at a text position has the class key hash = kw::mix64(canonical 2-bit
// code), a bijection of the class. The MINIMIZER of a window is the class with the smallest hash among its w m-mers; its ANCHOR is
// the global position of the LEFTMOST m-mer of that class in the window, in the forward text. The index keeps the packed bases, the
// record offsets, entries[] = kw::tagged_pos(hash, anchor) of every position that is the anchor of at least one window, grouped by
// the top b bits of the hash and ascending by position inside a group, and dir[2^b + 1], where each group starts (2^b = the least
// power of two at or above the anchors, 8 at the least).
//
// Heavy buckets. A bucket of more than bucket_limit anchors (low-complexity minimizers: poly-A marks every position) is HEAVY: bit
// 63 of its dir word. Its anchors are dropped, and every window whose minimizer hashes into it goes into an ordinary class table
// (kw::find_slot, 2 slots per such window, the slot forms of kmer_query_device.hip) instead. Which path a k-mer takes is a function
// of its minimizer's bucket, the same for x and rc(x), in the build and in the query.
//
// Build:
//   pack       SeqStore
//   anchors    anchor_mark_kernel: a thread owns kw::RUN window starts, rolls the m-mer codes (MinimizerWalk: the minimum is kept
//              while its leftmost occurrence stays in the window, else the w candidates are rescanned) and ORs the anchor's bit
//              into a bitmap of one bit per base -- a union of bits: order independent, no duplicates at run or record borders;
//              popcount per word, hu::scan_u32, anchor_compact_kernel: the positions, ascending
//   directory  bucket_hist_kernel, bucket_light_kernel (heavy buckets count 0), hu::scan_u32, bucket_scatter_kernel (the order inside
//              a bucket is that of the atomics), bucket_sort_kernel (ascending by position: the bytes no longer depend on that order;
//              then the heavy bit)
//   heavy      heavy_kernel<.., false> counts the windows of the heavy buckets, heavy_kernel<.., true> inserts them
// Query: MaskedSeqStore, then tig_query_kernel: query_kernel's walk (64 window starts per thread, one plain store per bit-array word,
// clear_from, one atomicAdd per (thread, record) and counter) with the lookup of tig_contains.
//
// Locate (a LOCATING index only, mtg_tig_index_build_locating): device_kmer_index_locate's contract and results at the
// coordinates of the indexed sequences. Such an index also keeps heavy_where[table slots], the smallest window start of every class
// of the heavy table (atomicMin behind the inserting heavy_kernel's find_slot); nothing more where no bucket is heavy. tig_locate_kernel
// is tig_query_kernel's walk without the bit arrays; per found window hit[q] = (t << 1) | strand, t = tig_where -- the MINIMUM over all
// candidates of the bucket that pass, or heavy_where[slot] -- and strand from one forward compare at t. From the hits to the runs:
// kmer_runs_device.hpp, shared with the table index. Thread: the same, the runs left on the device and joined into
// walks there (kmer_walks_device.hpp, shared with the table index too).
//
// Payloads (mtg_tig_index_build_annotated): a locating index that also keeps win_off[records + 1] and one weight and / or
// one colour mask per window of the text, dense or as runs (tig_payload_device.hpp). t above is the position whose payload the table
// index keeps for the class, so abundance and colours are two passes: tig_locate_kernel, unchanged, then a gather over hit[].
//
// Tallies (any locating index, mtg_tig_tally_*): one 64-bit counter per window ordinal of the text, owned by a TigTally,
// not by the index. The same two passes: tig_locate_kernel, then tig_tally_add_kernel or tig_coverage_gather_kernel
// (tig_tally_device.hpp) over hit[]. t is the same for every window of a class, so the counter at its ordinal is the class's.
//
// Pseudoalignment (a COLOURED index only, mtg_pseudoaligner_*): the colour call's two passes, unchanged, once for the
// reads and, with mates, once more for the mates into per_color and counts arrays that stay on the device; pseudoalign_device.hpp
// turns every row into one mask and the masks into their dictionary.
//
// Files (mtg_tig_index_save / _load): the device arrays of the TigIndex struct below, as they are, behind a header;
// tig_index_file_device.hpp, included at the end of this file, digests them on the device, and validates what a load has uploaded
// against everything the probes here assume of the arrays. No kernel of this file knows where its index came from.
//
// Exactness. A hit is declared only after kw::same_class has compared the query's k bases with k index bases that lie inside ONE
// record, or after the heavy table's exact `same`: never a false positive, and a tag or hash collision costs a compare. No false
// negative: let the class of the query window x be the index window y at c. Both have the same set of m-mer classes, hence the same
// minimizer v and the same bucket; if that is heavy both sides use the table. Else, if y == x, the leftmost m-mer of v in y is at
// the offset j1 of the leftmost one in x, so the build marked p = c + j1 and the candidate p - j1 is c. If y == rc(x), offset j of y
// is offset w - 1 - j of x, the leftmost in y is the RIGHTMOST in x (offset jL), the build marked p = c + (w - 1 - jL), and the second
// candidate is c. Light anchors are all kept, so p is in the bucket.
//
// Limits: those of the k-mer index (fewer than 2^40 - 1 bases, k < 2^32), m <= 31, bucket_limit <= 65536 (a bucket is sorted by one
// thread). Device memory: 0.25 B per base, 8 B per record, 8 B per anchor, 8 B per bucket (at most 16 B per anchor), 16 B per heavy
// window. There is no host path.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_runs_device.hpp"
#include "kmer_walks_device.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"
#include "pseudoalign_device.hpp"
#include "tig_payload_device.hpp"
#include "tig_tally_device.hpp"

namespace mtg {

namespace {

using kr::NO_HIT;
using kr::record_of;
using kw::EMPTY_SLOT;
using kw::POS_LIMIT;
using kw::RUN;
using kw::Window;

constexpr unsigned long long HEAVY = 1ull << 63;  // in a dir word
constexpr uint64_t TAG_MASK = 0x3FFFFFull;        // kw::tagged_pos keeps these bits of a hash

// what the m-mer walk needs beside the packed bases
struct MinArgs {
    uint64_t m, w;  // w = k - m + 1 m-mers per window
    uint64_t top;   // 2 (m - 1), where a base enters the reverse-complement code
    uint64_t mask;  // the 2 m low bits
};

// the minimizer of a window: the smallest m-mer hash, the global positions of the leftmost and the rightmost m-mer of that class
struct Minimizer {
    uint64_t hash, first, last;
};

// The minimizers of windows taken in ascending order. at(q) rolls one m-mer in if q follows the window before and the leftmost
// occurrence of the minimum is still inside, else it reads the window's k bases again. Either way the result is a function of the
// window alone: min, leftmost and rightmost are kept exactly (a new m-mer below the minimum replaces all three, one equal to it moves
// `last`, and `last` >= `first` never leaves before `first` does).
struct MinimizerWalk {
    const uint32_t *packed;
    const MinArgs &a;
    kw::BaseReader rd;  // at the base behind the last m-mer read
    uint64_t fwd = 0, rc = 0, next_q = ~0ull;
    Minimizer cur{0, 0, 0};

    __device__ __forceinline__ MinimizerWalk(const uint32_t *p, const MinArgs &args) : packed(p), a(args), rd(p, 0) {}
    __device__ __forceinline__ uint64_t step() {  // one base in; the hash of the m-mer that ends with it
        const uint64_t c = rd.next();
        fwd = ((fwd << 2) | c) & a.mask;
        rc = (rc >> 2) | ((3 - c) << a.top);
        return kw::mix64(fwd < rc ? fwd : rc);
    }
    __device__ __forceinline__ void take(uint64_t h, uint64_t pos) {
        if (h < cur.hash) cur = Minimizer{h, pos, pos};
        else if (h == cur.hash) cur.last = pos;
    }
    __device__ __forceinline__ const Minimizer &at(uint64_t q) {
        if (q == next_q && cur.first >= q) {
            take(step(), q + a.w - 1);
        } else {
            rd = kw::BaseReader(packed, q);
            fwd = rc = 0;
            for (uint64_t i = 0; i + 1 < a.m; i++) (void)step();
            cur = Minimizer{step(), q, q};
            for (uint64_t j = 1; j < a.w; j++) take(step(), q + j);
        }
        next_q = q + 1;
        return cur;
    }
};

struct TigArgs : kw::WindowArgs {  // packed / off: the sequences that are walked (build: the index's, query: the query's)
    MinArgs mn;
    const uint32_t *index_packed;
    const unsigned long long *index_off;  // [index_rec + 1]
    uint64_t index_rec;
    const unsigned long long *dir;      // [2^b + 1]; bit 63: heavy
    const unsigned long long *entries;  // [anchors]
    uint32_t shift;                     // 64 - b: a hash's bucket is hash >> shift
    unsigned long long *table;          // [slots] the windows of the heavy buckets; slots == 0: there are none
    uint64_t slots;
};

// ---- build: anchors ----
// bitmap: one bit per base, zeroed; bit p & 31 of word p >> 5 is set iff p is the anchor of a window
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void anchor_mark_kernel(TigArgs a, uint64_t n_bases, uint64_t n_rec, uint32_t *bitmap) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    MinimizerWalk walk(a.packed, a.mn);
    uint64_t marked = ~0ull;  // (consecutive windows mostly share their anchor)
    kw::for_each_window<WIDE>(a, p0, p0 + RUN < n_bases ? p0 + RUN : n_bases, 0, n_rec, [&](uint64_t q, uint64_t, const Window &) {
        const uint64_t p = walk.at(q).first;
        if (p != marked) atomicOr(&bitmap[p >> 5], 1u << (p & 31));
        marked = p;
    });
}
__global__ __launch_bounds__(hu::EB) void anchor_count_kernel(const uint32_t *bitmap, uint64_t n_words, uint32_t *count) {
    const uint64_t w = hu::gid();
    if (w < n_words) count[w] = (uint32_t)__popc(bitmap[w]);
}
// pos[rank[w] ..] = the set bits of word w: all anchors, ascending
__global__ __launch_bounds__(hu::EB) void anchor_compact_kernel(const uint32_t *bitmap, uint64_t n_words, const unsigned long long *rank,
                                                                uint64_t n_anchors, unsigned long long *pos) {
    const uint64_t w = hu::gid();
    if (w >= n_words) return;
    uint64_t i = rank[w];
    for (uint32_t v = bitmap[w]; v && i < n_anchors; v &= v - 1) pos[i++] = w * 32 + (uint64_t)__builtin_ctz(v);
}

// ---- build: directory ----
__global__ __launch_bounds__(hu::EB) void bucket_hist_kernel(const uint32_t *packed, const unsigned long long *pos, uint64_t n_anchors, uint64_t m,
                                                             uint32_t shift, uint32_t *hist) {
    const uint64_t i = hu::gid();
    if (i < n_anchors) atomicAdd(&hist[kw::class_key(packed, pos[i], m).hash >> shift], 1u);
}
// light[b] = the anchors bucket b keeps: none if it is heavy; *n_heavy += heavy buckets
__global__ __launch_bounds__(hu::EB) void bucket_light_kernel(const uint32_t *hist, uint64_t buckets, uint64_t limit, uint32_t *light,
                                                              unsigned long long *n_heavy) {
    const uint64_t b = hu::gid();
    if (b >= buckets) return;
    const bool heavy = hist[b] > limit;
    light[b] = heavy ? 0u : hist[b];
    if (heavy) atomicAdd(n_heavy, 1ull);
}
// cursor: [buckets], zeroed; afterwards the anchors each bucket keeps
__global__ __launch_bounds__(hu::EB) void bucket_scatter_kernel(const uint32_t *packed, const unsigned long long *pos, uint64_t n_anchors, uint64_t m,
                                                                uint32_t shift, const uint32_t *hist, uint64_t limit, const unsigned long long *dir,
                                                                uint32_t *cursor, uint64_t n_entries, unsigned long long *entries) {
    const uint64_t i = hu::gid();
    if (i >= n_anchors) return;
    const uint64_t p = pos[i], h = kw::class_key(packed, p, m).hash, b = h >> shift;
    if (hist[b] > limit) return;
    const uint64_t at = dir[b] + atomicAdd(&cursor[b], 1u);
    if (at < n_entries) entries[at] = kw::tagged_pos(h, p);  // (the scan counted exactly these: always)
}
// one thread per bucket: its entries ascending by position (at most `limit` of them, mostly one or two), then the heavy bit
__global__ __launch_bounds__(hu::EB) void bucket_sort_kernel(const uint32_t *hist, const uint32_t *kept, uint64_t buckets, uint64_t limit,
                                                             unsigned long long *dir, unsigned long long *entries) {
    const uint64_t b = hu::gid();
    if (b >= buckets) return;
    unsigned long long *e = entries + dir[b];
    const uint32_t n = kept[b];
    for (uint32_t i = 1; i < n; i++) {
        const unsigned long long x = e[i];
        uint32_t j = i;
        for (; j > 0 && (e[j - 1] & POS_LIMIT) > (x & POS_LIMIT); j--) e[j] = e[j - 1];
        e[j] = x;
    }
    if (hist[b] > limit) dir[b] |= HEAVY;
}

// ---- the heavy table ----
// the slot of w's class; w is a window of a.packed (CLAIM: taken with w.ident if the class has none)
template <bool WIDE, bool CLAIM>
__device__ __forceinline__ kw::Found heavy_find(const TigArgs &a, const Window &w) {
    return kw::find_slot<CLAIM>(a.table, a.slots, w.hash, w.ident, [&](unsigned long long cur) {
        if (!WIDE) return cur == w.ident;
        if ((cur >> 40) != (w.ident >> 40)) return false;
        if (CLAIM) return kw::same_class(a.packed, w.ident & POS_LIMIT, cur & POS_LIMIT, a.k);
        return kw::same_class(a.packed, w.ident & POS_LIMIT, a.index_packed, cur & POS_LIMIT, a.k);
    });
}
// the windows whose minimizer's bucket is heavy: counted into *count, or (INSERT) put into the table. LOCATE (a locating index; where
// is not read otherwise): where is [a.slots], all ones before; where[slot of the class] = the smallest window start of the class -- a
// claimed slot keeps its class, and the minimum over the occurrences of a class does not depend on the order they arrive in
// (index_insert_kernel's argument). A template parameter, so that the plain build's kernel stays the one it was.
template <bool WIDE, bool INSERT, bool LOCATE = false>
__global__ __launch_bounds__(hu::EB) void heavy_kernel(TigArgs a, uint64_t n_bases, uint64_t n_rec, unsigned long long *count, unsigned int *err,
                                                       unsigned long long *where) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    MinimizerWalk walk(a.packed, a.mn);
    uint32_t n = 0;
    kw::for_each_window<WIDE>(a, p0, p0 + RUN < n_bases ? p0 + RUN : n_bases, 0, n_rec, [&](uint64_t q, uint64_t, const Window &w) {
        if (!(a.dir[walk.at(q).hash >> a.shift] & HEAVY)) return;
        if (!INSERT) n++;
        else {
            const uint64_t slot = heavy_find<WIDE, true>(a, w).slot;
            if (slot == a.slots) atomicOr(err, 1u);  // (2 slots per window: never full)
            else if (LOCATE) atomicMin(&where[slot], (unsigned long long)q);
        }
    });
    if (!INSERT && n) atomicAdd(count, (unsigned long long)n);
}

// ---- query ----
// The window at q of a.packed (w: what it is to a table, mz: its minimizer) is a k-mer of the index: the header's lookup rule.
// [lo, hi): the index record of the last anchor looked at (empty before the first). Neighbouring windows mostly hit the same record,
// and the bounds of the record that holds p are a function of p, so keeping them only saves the binary search.
template <bool WIDE>
__device__ __forceinline__ bool tig_contains(const TigArgs &a, uint64_t q, const Window &w, const Minimizer &mz, uint64_t &lo, uint64_t &hi) {
    const uint64_t b = mz.hash >> a.shift;
    const unsigned long long d = a.dir[b];
    if (d & HEAVY) return heavy_find<WIDE, false>(a, w).slot != a.slots;
    const uint64_t end = a.dir[b + 1] & ~HEAVY, tag = mz.hash & TAG_MASK;
    const uint64_t j_fwd = mz.first - q;                  // x lies forward in the text: the anchor is its leftmost occurrence
    const uint64_t j_rev = a.mn.w - 1 - (mz.last - q);    // rc(x) does: the anchor is x's rightmost one, seen from the other end
    for (uint64_t i = d; i < end; i++) {
        const unsigned long long e = a.entries[i];
        if ((e >> 40) != tag) continue;
        const uint64_t p = e & POS_LIMIT;
        if (p < lo || p >= hi) {  // a candidate counts only inside the record of p
            const uint64_t r = record_of(a.index_off, a.index_rec, p);
            lo = a.index_off[r];
            hi = a.index_off[r + 1];
        }
        if (p >= lo + j_fwd && p - j_fwd + a.k <= hi && kw::same_class(a.packed, q, a.index_packed, p - j_fwd, a.k)) return true;
        if (j_rev != j_fwd && p >= lo + j_rev && p - j_rev + a.k <= hi && kw::same_class(a.packed, q, a.index_packed, p - j_rev, a.k)) return true;
    }
    return false;
}

// tig_contains that says where: the smallest start of an index window, inside one record, of the class of the window
// at q; NO_HIT if there is none. Heavy bucket: heavy_where[slot]. Light bucket: every occurrence of the class has its anchor among
// the bucket's entries, so the candidates that pass the record bound and kw::same_class ARE the occurrences, and the answer is the
// minimum over all of them -- not the first that passes: entries ascend by anchor p, but the two candidates p - j_fwd and p - j_rev
// differ in their offsets, and an occurrence on the other strand can lie earlier in the text while its anchor lies later. A
// candidate at or above the best so far is not compared, and once a best t is known an entry with p - max(j_fwd, j_rev) >= t ends
// the scan: its candidates and those of every later entry are at or above t.
template <bool WIDE>
__device__ __forceinline__ uint64_t tig_where(const TigArgs &a, const unsigned long long *heavy_where, uint64_t q, const Window &w,
                                              const Minimizer &mz, uint64_t &lo, uint64_t &hi) {
    const uint64_t b = mz.hash >> a.shift;
    const unsigned long long d = a.dir[b];
    if (d & HEAVY) {
        const uint64_t slot = heavy_find<WIDE, false>(a, w).slot;
        return slot != a.slots ? heavy_where[slot] : NO_HIT;
    }
    const uint64_t end = a.dir[b + 1] & ~HEAVY, tag = mz.hash & TAG_MASK;
    const uint64_t j_fwd = mz.first - q, j_rev = a.mn.w - 1 - (mz.last - q), j_max = j_fwd > j_rev ? j_fwd : j_rev;
    uint64_t best = NO_HIT;
    for (uint64_t i = d; i < end; i++) {
        const unsigned long long e = a.entries[i];
        const uint64_t p = e & POS_LIMIT;
        if (best != NO_HIT && p >= best + j_max) break;
        if ((e >> 40) != tag) continue;
        if (p < lo || p >= hi) {  // a candidate counts only inside the record of p
            const uint64_t r = record_of(a.index_off, a.index_rec, p);
            lo = a.index_off[r];
            hi = a.index_off[r + 1];
        }
        if (p >= lo + j_fwd && p - j_fwd < best && p - j_fwd + a.k <= hi && kw::same_class(a.packed, q, a.index_packed, p - j_fwd, a.k))
            best = p - j_fwd;
        if (j_rev != j_fwd && p >= lo + j_rev && p - j_rev < best && p - j_rev + a.k <= hi &&
            kw::same_class(a.packed, q, a.index_packed, p - j_rev, a.k))
            best = p - j_rev;
    }
    return best;
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

// query_kernel's contract and layout (kmer_query_device.hip). counts: [2 n_rec], valid then found; valid_bits / present_bits:
// [(n_bases + 63) / 64] or null. The minimizer walk is asked for valid windows only: after an invalid stretch it reads afresh.
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void tig_query_kernel(TigArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                           unsigned long long *counts, unsigned long long *valid_bits,
                                                           unsigned long long *present_bits) {
    const uint64_t gid = hu::gid(), p0 = gid * RUN;
    if (p0 >= n_bases) return;
    unsigned long long vbits = 0, pbits = 0;
    uint64_t rec = ~0ull, next_q = ~0ull, clear_from = 0;
    uint64_t idx_lo = 1, idx_hi = 0;    // tig_contains' index record: none yet
    uint32_t n_valid = 0, n_found = 0;  // (of the current record; at most RUN)
    MinimizerWalk walk(a.packed, a.mn);
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
        if (tig_contains<WIDE>(a, q, w, walk.at(q), idx_lo, idx_hi)) {
            n_found++;
            pbits |= bit;
        }
    });
    flush();
    if (valid_bits) valid_bits[gid] = vbits;
    if (present_bits) present_bits[gid] = pbits;
}

// tig_query_kernel's walk without the bit arrays; per found window at q: hit[q] = (t << 1) | strand, t = tig_where,
// strand 0 iff the query's bases equal the index's at t one by one (kr::same_forward). hit: [n_bases], NO_HIT before; a thread is the
// only writer of its RUN positions. heavy_where: [a.slots] (null if no bucket is heavy: never read then).
template <bool WIDE>
__global__ __launch_bounds__(hu::EB) void tig_locate_kernel(TigArgs a, const unsigned long long *bad, uint64_t n_bases, uint64_t n_rec,
                                                            unsigned long long *counts, const unsigned long long *heavy_where,
                                                            unsigned long long *hit) {
    const uint64_t p0 = hu::gid() * RUN;
    if (p0 >= n_bases) return;
    uint64_t rec = ~0ull, next_q = ~0ull, clear_from = 0;
    uint64_t idx_lo = 1, idx_hi = 0;    // tig_where's index record: none yet
    uint32_t n_valid = 0, n_found = 0;  // (of the current record; at most RUN)
    MinimizerWalk walk(a.packed, a.mn);
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
        n_valid++;
        const uint64_t t = tig_where<WIDE>(a, heavy_where, q, w, walk.at(q), idx_lo, idx_hi);
        if (t == NO_HIT) return;
        n_found++;
        hit[q] = (t << 1) | (kr::same_forward(a.packed, q, a.index_packed, t, a.k) ? 0ull : 1ull);
    });
    flush();
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

struct TigIndex {
    mtg_tig_index_info info{};
    int device_id = 0;
    uint32_t shift = 61;
    hu::DeviceArray<uint32_t> packed;
    hu::DeviceArray<unsigned long long> off;      // [info.records + 1]
    hu::DeviceArray<unsigned long long> dir;      // [info.buckets + 1]
    hu::DeviceArray<unsigned long long> entries;  // [info.anchors]
    hu::DeviceArray<unsigned long long> table;    // [info.table_slots]
    bool locating = false;
    hu::DeviceArray<unsigned long long> heavy_where;  // locating, and a bucket is heavy: [info.table_slots] the smallest window start of the slot's class
    // payloads by position: none unless built annotated
    hu::DeviceArray<unsigned long long> win_off;  // [info.records + 1] the windows of the records before
    tp::Payload<uint32_t> weights;
    tp::Payload<unsigned long long> colors;
    uint64_t n_colors = 0;
};

uint64_t tig_index_default_m(uint64_t k) { return std::min<uint64_t>(19, (2 * k + 2) / 3); }

TigIndex *device_tig_index_build(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit, int device_id,
                                 TigIndexTimes *times, bool locating, const char *fn) {
    if (!fn) fn = locating ? "mtg_tig_index_build_locating" : "mtg_tig_index_build";
    if (k < 1) MTG_DIE("%s: k must be >= 1", fn);
    if (k > 0xFFFFFFFFull) MTG_DIE("%s: k too large", fn);
    if (m == 0) m = tig_index_default_m(k);
    if (m > k || m > 31) MTG_DIE("%s: the minimizer length %llu is outside 1 .. min(k, 31)", fn, (unsigned long long)m);
    if (bucket_limit == 0) bucket_limit = 64;
    if (bucket_limit > 65536) MTG_DIE("%s: bucket_limit %llu; the limit is 65536", fn, (unsigned long long)bucket_limit);
    TigIndex *ix = new TigIndex();
    mtg_tig_index_info &info = ix->info;
    info.k = k;
    info.m = m;
    info.bucket_limit = bucket_limit;
    info.records = n;
    info.occurrences = check_offsets(fn, seq, off, n, k);
    info.characters = off[n];
    if (info.characters >= POS_LIMIT) MTG_DIE("%s: %llu bases; the limit is 2^40 - 2", fn, (unsigned long long)info.characters);
    if (device_id < 0 || device_count() <= device_id) MTG_DIE("no HIP device %d for the tig index (there is no CPU path)", device_id);
    HIP_CHECK(hipSetDevice(device_id));
    ix->device_id = device_id;
    ix->locating = locating;
    hipStream_t st = nullptr;
    const bool wide = k >= 32;

    SeqStore store("indexed sequences", seq, off, n, st, device_id);
    PhaseEvents<4> ev;
    ev.mark(0, st);
    TigArgs a{};
    a.packed = a.index_packed = store.packed; a.off = a.index_off = store.off; a.index_rec = n;
    a.mn = MinArgs{m, k - m + 1, 2 * (m - 1), (1ull << (2 * m)) - 1};
    kw::window_args_set_k(a, k);
    const unsigned run_grid = hu::grid_for((store.n_bases + RUN - 1) / RUN);

    // anchors: every position that is the anchor of a window, ascending
    uint64_t all_anchors = 0;
    hu::DeviceArray<unsigned long long> pos;
    if (info.occurrences) {
        const uint64_t bit_words = (store.n_bases + 31) / 32;
        hu::DeviceArray<uint32_t> bitmap(bit_words), count(bit_words);
        hu::DeviceArray<unsigned long long> rank(bit_words);
        hu::ScanScratch<unsigned long long> scan(bit_words);
        HIP_CHECK(hipMemsetAsync(bitmap, 0, bit_words * 4, st));
        if (wide) anchor_mark_kernel<true><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, bitmap);
        else anchor_mark_kernel<false><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, bitmap);
        anchor_count_kernel<<<hu::grid_for(bit_words), hu::EB, 0, st>>>(bitmap, bit_words, count);
        HIP_CHECK(hipGetLastError());
        scan.scan(st, count, bit_words, rank);
        HIP_CHECK(hipMemcpyAsync(&all_anchors, scan.total(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        pos.alloc(all_anchors);  // (a window has an anchor: at least one)
        anchor_compact_kernel<<<hu::grid_for(bit_words), hu::EB, 0, st>>>(bitmap, bit_words, rank, all_anchors, pos);
        HIP_CHECK(hipGetLastError());
    }
    ev.mark(1, st);

    // directory: the anchors of the light buckets, grouped by bucket, ascending inside one
    uint32_t bits = 3;
    while ((1ull << bits) < all_anchors) bits++;
    const uint64_t buckets = 1ull << bits;
    ix->shift = a.shift = 64 - bits;
    info.buckets = buckets;
    ix->dir.alloc(buckets + 1);
    {
        hu::DeviceArray<uint32_t> hist(buckets), light(buckets);
        hu::ScanScratch<unsigned long long> scan(buckets);
        HIP_CHECK(hipMemsetAsync(hist, 0, buckets * 4, st));
        if (all_anchors) bucket_hist_kernel<<<hu::grid_for(all_anchors), hu::EB, 0, st>>>(store.packed, pos, all_anchors, m, a.shift, hist);
        bucket_light_kernel<<<hu::grid_for(buckets), hu::EB, 0, st>>>(hist, buckets, bucket_limit, light, store.small.d + 2);
        HIP_CHECK(hipGetLastError());
        scan.scan(st, light, buckets, ix->dir.get());
        HIP_CHECK(hipMemcpyAsync(ix->dir + buckets, scan.total(), 8, hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipMemcpyAsync(&info.anchors, scan.total(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        ix->entries.alloc(std::max<uint64_t>(info.anchors, 1));
        HIP_CHECK(hipMemsetAsync(light, 0, buckets * 4, st));  // (now the scatter's cursors)
        if (all_anchors)
            bucket_scatter_kernel<<<hu::grid_for(all_anchors), hu::EB, 0, st>>>(store.packed, pos, all_anchors, m, a.shift, hist, bucket_limit, ix->dir,
                                                                               light, info.anchors, ix->entries);
        bucket_sort_kernel<<<hu::grid_for(buckets), hu::EB, 0, st>>>(hist, light, buckets, bucket_limit, ix->dir, ix->entries);
        HIP_CHECK(hipGetLastError());
        ev.mark(2, st);
        store.small.read(st, "tig index");
        info.heavy_buckets = store.small.h[2];
    }
    pos.release();
    a.dir = ix->dir;
    a.entries = ix->entries;

    // the heavy table: every window whose minimizer's bucket is heavy
    if (info.heavy_buckets) {
        if (wide) heavy_kernel<true, false><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, store.small.d + 3, store.small.err(), nullptr);
        else heavy_kernel<false, false><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, store.small.d + 3, store.small.err(), nullptr);
        HIP_CHECK(hipGetLastError());
        store.small.read(st, "tig index");
        info.heavy_windows = store.small.h[3];
        info.table_slots = std::max<uint64_t>(8, (2 * info.heavy_windows + 7) / 8 * 8);
        a.table = ix->table.alloc(info.table_slots);
        a.slots = info.table_slots;
        HIP_CHECK(hipMemsetAsync(ix->table, 0xFF, info.table_slots * 8, st));
        if (locating) {
            ix->heavy_where.alloc(info.table_slots);
            HIP_CHECK(hipMemsetAsync(ix->heavy_where, 0xFF, info.table_slots * 8, st));
        }
        if (locating) {
            if (wide) heavy_kernel<true, true, true><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, nullptr, store.small.err(), ix->heavy_where);
            else heavy_kernel<false, true, true><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, nullptr, store.small.err(), ix->heavy_where);
        } else {
            if (wide) heavy_kernel<true, true><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, nullptr, store.small.err(), nullptr);
            else heavy_kernel<false, true><<<run_grid, hu::EB, 0, st>>>(a, store.n_bases, n, nullptr, store.small.err(), nullptr);
        }
        HIP_CHECK(hipGetLastError());
    }
    ev.mark(3, st);
    store.small.read(st, "tig index");
    if (times) {
        times->build_upload_ms = store.upload_ms;
        times->build_pack_ms = store.pack_ms;
        times->build_anchors_ms = ev.ms(0, 1);
        times->build_directory_ms = ev.ms(1, 2);
        times->build_heavy_ms = ev.ms(2, 3);
    }
    ix->packed = store.take_packed();
    ix->off = store.take_off();
    info.device_bytes = (store.n_words + 2) * 4 + (n + 1) * 8 + (buckets + 1) * 8 + std::max<uint64_t>(info.anchors, 1) * 8 + info.table_slots * 8;
    if (locating) info.device_bytes += info.table_slots * 8;  // heavy_where
    return ix;
}

void device_tig_index_info(const TigIndex *ix, mtg_tig_index_info *out) { *out = ix->info; }
bool device_tig_index_is_locating(const TigIndex *ix) { return ix->locating; }

void device_tig_index_free(TigIndex *ix) {
    if (!ix) return;
    int cur = 0;  // (an index may die on a thread whose current device is another one)
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(ix->device_id);
    delete ix;
    (void)hipSetDevice(cur);
}

void device_tig_index_query(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                            uint64_t *found, uint64_t *present_bits, uint64_t *valid_bits, TigIndexTimes *times) {
    const char *fn = "mtg_tig_index_query";
    const uint64_t k = ix->info.k;
    (void)check_offsets(fn, seq, off, n, k);
    if (n && (!kmers || !valid || !found)) MTG_DIE("%s: null argument", fn);
    if (off[n] >= POS_LIMIT) MTG_DIE("%s: %llu bases; the limit is 2^40 - 2", fn, (unsigned long long)off[n]);
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t len = off[r + 1] - off[r];
        kmers[r] = len >= k ? len - k + 1 : 0;
        valid[r] = found[r] = 0;
    }
    const uint64_t n_bases = off[n], bit_words = (n_bases + 63) / 64;
    if (times) times->query_upload_ms = times->query_pack_ms = times->query_probe_ms = 0;
    if (n_bases == 0) return;  // nothing to look at
    HIP_CHECK(hipSetDevice(ix->device_id));
    hipStream_t st = nullptr;
    MaskedSeqStore store(seq, off, n, st, ix->device_id);
    hu::DeviceArray<unsigned long long> d_counts(2 * n), d_bits;  // valid_bits, then present_bits (those asked for)
    const int n_arrays = (valid_bits != nullptr) + (present_bits != nullptr);
    if (n_arrays) d_bits.alloc(n_arrays * bit_words);
    unsigned long long *d_valid_bits = valid_bits ? d_bits.get() : nullptr;
    unsigned long long *d_present_bits = present_bits ? d_bits + (valid_bits ? bit_words : 0) : nullptr;
    TigArgs a{};
    a.packed = store.packed; a.off = store.off;
    a.index_packed = ix->packed; a.index_off = ix->off; a.index_rec = ix->info.records;
    a.dir = ix->dir; a.entries = ix->entries; a.shift = ix->shift; a.table = ix->table; a.slots = ix->info.table_slots;
    a.mn = MinArgs{ix->info.m, k - ix->info.m + 1, 2 * (ix->info.m - 1), (1ull << (2 * ix->info.m)) - 1};
    kw::window_args_set_k(a, k);
    PhaseEvents<2> ev;
    ev.mark(0, st);
    HIP_CHECK(hipMemsetAsync(d_counts, 0, 2 * n * 8, st));
    const unsigned grid = hu::grid_for(bit_words);  // (one thread per word: every word of the bit arrays is written)
    if (k >= 32) tig_query_kernel<true><<<grid, hu::EB, 0, st>>>(a, store.bad, n_bases, n, d_counts, d_valid_bits, d_present_bits);
    else tig_query_kernel<false><<<grid, hu::EB, 0, st>>>(a, store.bad, n_bases, n, d_counts, d_valid_bits, d_present_bits);
    HIP_CHECK(hipGetLastError());
    ev.mark(1, st);
    HIP_CHECK(hipMemcpyAsync(valid, d_counts, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(found, d_counts + n, n * 8, hipMemcpyDeviceToHost, st));
    if (valid_bits) HIP_CHECK(hipMemcpyAsync(valid_bits, d_valid_bits, bit_words * 8, hipMemcpyDeviceToHost, st));
    if (present_bits) HIP_CHECK(hipMemcpyAsync(present_bits, d_present_bits, bit_words * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (times) {
        times->query_upload_ms = store.upload_ms;
        times->query_pack_ms = store.pack_ms;
        times->query_probe_ms = ev.ms(0, 1);
    }
}

namespace {

// What the calls on a locating index share (locate, abundance, colors): the checks of the query, kmers[] filled, valid[] and found[]
// zeroed; returns the query's bases (missing: an out-pointer of the caller's own is null). All on the host.
uint64_t locate_windows(const char *fn, const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                        uint64_t *found, bool missing) {
    const uint64_t k = ix->info.k;
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

// ... and the first pass of a query that has bases: the query on the index's device and tig_locate_kernel between the marks 0 and 1
// of ev; d_counts: [2 n] valid then found, d_hit: [n_bases]. The caller queues its second pass and marks 2. into: the caller's own
// [2 n] counters, which the pass adds to as they are, in place of d_counts.
struct LocateProbe {
    const uint64_t n;
    const int device_id;
    hipStream_t st = nullptr;
    MaskedSeqStore store;
    hu::DeviceArray<unsigned long long> d_counts, d_hit;
    PhaseEvents<3> ev;

    LocateProbe(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, unsigned long long *into = nullptr)
        : n(n), device_id(on_device(ix->device_id)), store(seq, off, n, st, device_id), d_hit(store.n_bases) {
        const uint64_t k = ix->info.k, n_bases = store.n_bases;
        unsigned long long *counts = into ? into : d_counts.alloc(2 * n);
        TigArgs a{};
        a.packed = store.packed; a.off = store.off;
        a.index_packed = ix->packed; a.index_off = ix->off; a.index_rec = ix->info.records;
        a.dir = ix->dir; a.entries = ix->entries; a.shift = ix->shift; a.table = ix->table; a.slots = ix->info.table_slots;
        a.mn = MinArgs{ix->info.m, k - ix->info.m + 1, 2 * (ix->info.m - 1), (1ull << (2 * ix->info.m)) - 1};
        kw::window_args_set_k(a, k);
        ev.mark(0, st);
        if (!into) HIP_CHECK(hipMemsetAsync(counts, 0, 2 * n * 8, st));
        HIP_CHECK(hipMemsetAsync(d_hit, 0xFF, n_bases * 8, st));
        const unsigned grid = hu::grid_for((n_bases + RUN - 1) / RUN);
        if (k >= 32) tig_locate_kernel<true><<<grid, hu::EB, 0, st>>>(a, store.bad, n_bases, n, counts, ix->heavy_where.get(), d_hit);
        else tig_locate_kernel<false><<<grid, hu::EB, 0, st>>>(a, store.bad, n_bases, n, counts, ix->heavy_where.get(), d_hit);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
    }
    void download_counts(uint64_t *valid, uint64_t *found) {
        HIP_CHECK(hipMemcpyAsync(valid, d_counts, n * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(found, d_counts + n, n * 8, hipMemcpyDeviceToHost, st));
    }
    tp::GatherArgs gather_args(const TigIndex *ix, unsigned int *err) const {
        return tp::GatherArgs{d_hit, store.off, ix->off, ix->win_off, store.n_bases, n, ix->info.records, err};
    }
    void booked(TigPayloadTimes *t) {
        t->upload_ms = store.upload_ms;
        t->pack_ms = store.pack_ms;
        t->probe_ms = ev.ms(0, 1);
        t->gather_ms = ev.ms(1, 2);
    }
};

}  // namespace

void device_tig_index_locate(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, KmerRuns *runs, KmerLocateTimes *times) {
    const char *fn = "mtg_tig_index_locate";
    if (!ix->locating) MTG_DIE("%s: the index keeps no positions of its heavy buckets (build it with mtg_tig_index_build_locating)", fn);
    const uint64_t n_bases = locate_windows(fn, ix, seq, off, n, kmers, valid, found, !runs);
    *runs = KmerRuns();
    if (times) *times = KmerLocateTimes();
    if (n_bases == 0) return;  // nothing to look at
    LocateProbe p(ix, seq, off, n);
    const kr::RunArgs ra{p.d_hit, p.store.off, ix->off, n_bases, n, ix->info.records, ix->info.k};
    kr::runs_from_hits(ra, p.st, ix->device_id, runs, [&](hipStream_t) {
        p.ev.mark(2, p.st);
        p.download_counts(valid, found);
    });
    if (times) {
        times->upload_ms = p.store.upload_ms;
        times->pack_ms = p.store.pack_ms;
        times->probe_ms = p.ev.ms(0, 1);
        times->runs_ms = p.ev.ms(1, 2);
    }
}

// ---- thread: the same probe and run stage, then the walks from the runs where they are (kmer_walks_device.hpp) ----
void device_tig_index_thread(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t min_kmers, uint64_t *kmers,
                             uint64_t *valid, uint64_t *found, KmerWalks *walks, KmerThreadTimes *times) {
    const char *fn = "mtg_tig_index_thread";
    if (!ix->locating) MTG_DIE("%s: the index keeps no positions of its heavy buckets (build it with mtg_tig_index_build_locating)", fn);
    const uint64_t n_bases = locate_windows(fn, ix, seq, off, n, kmers, valid, found, !walks);
    *walks = KmerWalks();
    if (times) *times = KmerThreadTimes();
    if (n_bases == 0) return;  // nothing to look at
    LocateProbe p(ix, seq, off, n);
    PhaseEvents<1> walked;
    const kr::RunArgs ra{p.d_hit, p.store.off, ix->off, n_bases, n, ix->info.records, ix->info.k};
    kr::RunStage stage(n_bases);
    stage.queue(ra, p.st);
    p.ev.mark(2, p.st);
    kwk::walks_from_runs(stage, ix->off, ix->info.k, min_kmers, p.st, ix->device_id, walks, [&](hipStream_t) {
        walked.mark(0, p.st);
        p.download_counts(valid, found);
    });
    if (times) {
        times->upload_ms = p.store.upload_ms;
        times->pack_ms = p.store.pack_ms;
        times->probe_ms = p.ev.ms(0, 1);
        times->runs_ms = p.ev.ms(1, 2);
        float f = 0.f;
        HIP_CHECK(hipEventSynchronize(walked.ev[0]));
        HIP_CHECK(hipEventElapsedTime(&f, p.ev.ev[2], walked.ev[0]));
        times->walks_ms = f;
    }
}

// ---- payloads by position ----
TigIndex *device_tig_index_build_annotated(const char *seq, const uint64_t *off, uint64_t n, uint64_t k, uint64_t m, uint64_t bucket_limit,
                                           const KmerWeights *weights, const KmerColors *colors, int layout, int device_id, TigIndexTimes *times,
                                           TigPayloadTimes *payload_times) {
    const char *fn = "mtg_tig_index_build_annotated";
    if (k < 1) MTG_DIE("%s: k must be >= 1", fn);
    if (layout < 0 || layout > 2) MTG_DIE("%s: layout %d; 0 (auto), 1 (dense) and 2 (runs) are served", fn, layout);
    const uint64_t windows = check_offsets(fn, seq, off, n, k);
    if (weights && weights->n != windows) MTG_DIE("%s: %llu weights for %llu windows", fn, (unsigned long long)weights->n, (unsigned long long)windows);
    if (weights && weights->n && !weights->w) MTG_DIE("%s: null argument", fn);
    if (colors && (colors->n_colors < 1 || colors->n_colors > 64)) MTG_DIE("%s: %llu colours; 1 .. 64 are served", fn, (unsigned long long)colors->n_colors);
    if (colors && colors->n != windows) MTG_DIE("%s: %llu colour words for %llu windows", fn, (unsigned long long)colors->n, (unsigned long long)windows);
    if (colors && colors->n && !colors->c) MTG_DIE("%s: null argument", fn);
    if (colors && colors->n_colors < 64)  // (the gather adds into per_color[r C + c] for every set bit c)
        for (uint64_t i = 0; i < colors->n; i++)
            if (colors->c[i] >> colors->n_colors)
                MTG_DIE("%s: the mask of window %llu has a bit at or beyond n_colors = %llu", fn, (unsigned long long)i, (unsigned long long)colors->n_colors);
    TigIndex *ix = device_tig_index_build(seq, off, n, k, m, bucket_limit, device_id, times, true, fn);
    if (payload_times) *payload_times = TigPayloadTimes();
    if (!weights && !colors) return ix;
    hipStream_t st = nullptr;
    {
        std::vector<unsigned long long> win_off(n + 1, 0);
        for (uint64_t r = 0; r < n; r++) win_off[r + 1] = win_off[r] + (off[r + 1] - off[r] >= k ? off[r + 1] - off[r] - k + 1 : 0);
        ix->win_off.alloc(n + 1);
        hu::upload_sliced(ix->win_off, win_off.data(), (n + 1) * 8, st, device_id);
        HIP_CHECK(hipStreamSynchronize(st));  // (win_off leaves its scope)
    }
    ix->info.device_bytes += (n + 1) * 8;
    tp::PayloadBuildTimes t;
    if (weights) {
        tp::payload_build(ix->weights, weights->w, windows, 0, (uint32_t)layout, st, device_id, &t);
        ix->info.device_bytes += ix->weights.info.device_bytes;
        if (payload_times) { double *o = payload_times->weights_ms; o[0] = t.upload_ms; o[1] = t.reduce_ms; o[2] = t.flag_scan_ms; o[3] = t.store_ms; }
    }
    if (colors) {
        tp::payload_build(ix->colors, reinterpret_cast<const unsigned long long *>(colors->c), windows, colors->n_colors, (uint32_t)layout, st, device_id, &t);
        ix->n_colors = colors->n_colors;
        ix->info.device_bytes += ix->colors.info.device_bytes;
        if (payload_times) { double *o = payload_times->colors_ms; o[0] = t.upload_ms; o[1] = t.reduce_ms; o[2] = t.flag_scan_ms; o[3] = t.store_ms; }
    }
    return ix;
}

void device_tig_index_payload_info(const TigIndex *ix, mtg_tig_payload_info *out) {
    *out = mtg_tig_payload_info{};
    out->weights = ix->weights.info;
    out->colors = ix->colors.info;
    out->n_colors = ix->colors.present() ? ix->n_colors : 0;
    out->win_offset_bytes = ix->win_off ? (ix->info.records + 1) * 8 : 0;
}

namespace {
// the gather's error word, zeroed on st; check() after the stream was waited for
struct GatherErr {
    hu::DeviceArray<unsigned int> d;
    unsigned int h = 0;
    explicit GatherErr(hipStream_t st) : d(1) { HIP_CHECK(hipMemsetAsync(d, 0, 4, st)); }
    void fetch(hipStream_t st) { HIP_CHECK(hipMemcpyAsync(&h, d, 4, hipMemcpyDeviceToHost, st)); }
    void check(const char *fn) const {
        if (h) MTG_DIE("%s: internal error %u (a located window outside the payload)", fn, h);
    }
};
}  // namespace

void device_tig_index_abundance(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                                uint64_t *found, uint64_t *sum, uint32_t *min, uint32_t *max, uint32_t *per_window, TigPayloadTimes *times) {
    const char *fn = "mtg_tig_index_abundance";
    if (!ix->weights.present()) MTG_DIE("%s: the index keeps no weights (build it with mtg_tig_index_build_annotated)", fn);
    const uint64_t n_bases = locate_windows(fn, ix, seq, off, n, kmers, valid, found, n && (!sum || !min || !max));
    std::fill(sum, sum + n, 0ull);
    std::fill(min, min + n, 0u);
    std::fill(max, max + n, 0u);
    if (times) times->upload_ms = times->pack_ms = times->probe_ms = times->gather_ms = 0;
    if (n_bases == 0) return;  // nothing to look at
    LocateProbe p(ix, seq, off, n);
    hu::DeviceArray<unsigned long long> d_sum(n);
    hu::DeviceArray<uint32_t> d_minmax(2 * n), d_per_window;
    if (per_window) d_per_window.alloc(n_bases);
    GatherErr err(p.st);
    HIP_CHECK(hipMemsetAsync(d_sum, 0, n * 8, p.st));
    HIP_CHECK(hipMemsetAsync(d_minmax, 0xFF, n * 4, p.st));
    HIP_CHECK(hipMemsetAsync(d_minmax + n, 0, n * 4, p.st));
    // (one thread per run of positions: every word of per_window is written)
    tp::abundance_gather_kernel<<<hu::grid_for((n_bases + RUN - 1) / RUN), hu::EB, 0, p.st>>>(p.gather_args(ix, err.d), ix->weights.view(), d_sum, d_minmax,
                                                                                             d_per_window);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(2, p.st);
    p.download_counts(valid, found);
    err.fetch(p.st);
    HIP_CHECK(hipMemcpyAsync(sum, d_sum, n * 8, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipMemcpyAsync(min, d_minmax, n * 4, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipMemcpyAsync(max, d_minmax + n, n * 4, hipMemcpyDeviceToHost, p.st));
    HIP_CHECK(hipStreamSynchronize(p.st));
    err.check(fn);
    if (per_window) hu::download_sliced(per_window, d_per_window, n_bases * 4, p.st, p.device_id);
    for (uint64_t r = 0; r < n; r++)
        if (!found[r]) min[r] = 0;  // (nothing lowered the all-ones word)
    if (times) p.booked(times);
}

void device_tig_index_colors(const TigIndex *ix, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                             uint64_t *found, uint32_t *per_color, uint64_t *per_window, TigPayloadTimes *times) {
    const char *fn = "mtg_tig_index_colors";
    if (!ix->colors.present()) MTG_DIE("%s: the index keeps no colours (build it with mtg_tig_index_build_annotated)", fn);
    const uint64_t C = ix->n_colors;
    const uint64_t n_bases = locate_windows(fn, ix, seq, off, n, kmers, valid, found, n && !per_color);
    for (uint64_t r = 0; r < n; r++)
        if (kmers[r] >> 32) MTG_DIE("%s: record %llu has %llu windows; the per-colour counters are 32-bit", fn, (unsigned long long)r,
                                    (unsigned long long)kmers[r]);
    std::fill(per_color, per_color + n * C, 0u);
    if (times) times->upload_ms = times->pack_ms = times->probe_ms = times->gather_ms = 0;
    if (n_bases == 0) return;  // nothing to look at
    LocateProbe p(ix, seq, off, n);
    hu::DeviceArray<uint32_t> d_per_color(n * C);
    hu::DeviceArray<unsigned long long> d_per_window;
    if (per_window) d_per_window.alloc(n_bases);
    GatherErr err(p.st);
    HIP_CHECK(hipMemsetAsync(d_per_color, 0, n * C * 4, p.st));
    // (one thread per run of positions: every word of per_window is written)
    tp::color_gather_kernel<<<hu::grid_for((n_bases + RUN - 1) / RUN), hu::EB, 0, p.st>>>(p.gather_args(ix, err.d), ix->colors.view(), (uint32_t)C, d_per_color,
                                                                                         d_per_window);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(2, p.st);
    p.download_counts(valid, found);
    err.fetch(p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    err.check(fn);
    hu::download_sliced(per_color, d_per_color, n * C * 4, p.st, p.device_id);
    if (per_window) hu::download_sliced(per_window, d_per_window, n_bases * 8, p.st, p.device_id);
    if (times) p.booked(times);
}

// ---- pseudoalignment ----
uint64_t device_tig_index_n_colors(const TigIndex *ix) { return ix->colors.present() ? ix->n_colors : 0; }

// tig_locate_kernel and tp::color_gather_kernel, unchanged, once per side into one pair of arrays that stay on the device; pa::reduce
// does the rest.
void device_tig_index_pseudoalign(const TigIndex *ix, const PseudoalignRule &rule, uint64_t base, const char *seq, const uint64_t *off, uint64_t n,
                                  const char *mate_seq, const uint64_t *mate_off, uint64_t *kmers, uint64_t *valid, uint64_t *found, uint64_t *masks,
                                  PseudoalignCall *out) {
    const char *fn = "mtg_pseudoaligner_align";
    if (!ix->colors.present()) MTG_DIE("%s: the index keeps no colours (build it with mtg_tig_index_build_annotated)", fn);
    const uint64_t C = ix->n_colors;
    const bool paired = mate_off != nullptr;
    uint64_t side_bases[2] = {locate_windows(fn, ix, seq, off, n, kmers, valid, found, n && !masks), 0};
    if (paired) {
        std::vector<uint64_t> mk(n), mv(n), mf(n);
        side_bases[1] = locate_windows(fn, ix, mate_seq, mate_off, n, mk.data(), mv.data(), mf.data(), false);
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
        LocateProbe p(ix, side ? mate_seq : seq, side ? mate_off : off, n, d_counts);
        GatherErr err(p.st);
        tp::color_gather_kernel<<<hu::grid_for((n_bases + RUN - 1) / RUN), hu::EB, 0, p.st>>>(p.gather_args(ix, err.d), ix->colors.view(), (uint32_t)C, d_hits,
                                                                                             nullptr);
        HIP_CHECK(hipGetLastError());
        p.ev.mark(2, p.st);
        err.fetch(p.st);
        HIP_CHECK(hipStreamSynchronize(p.st));
        err.check(fn);
        out->upload_ms += p.store.upload_ms;
        out->pack_ms += p.store.pack_ms;
        out->probe_ms += p.ev.ms(0, 2);  // (the locate pass and the gather)
    }
    pa::reduce(fn, d_hits, d_counts, n, (uint32_t)C, rule, base, st, ix->device_id, masks, out);
    const auto t0 = std::chrono::steady_clock::now();
    HIP_CHECK(hipMemcpyAsync(valid, d_counts, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(found, d_counts + n, n * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    out->download_ms += ms_since(t0);
}

// ---- tallies by position ----
struct TigTally {
    const TigIndex *ix;  // (the caller keeps it alive for add and coverage; the rest does without it)
    int device_id;
    uint64_t windows, records;
    hu::DeviceArray<unsigned long long> count;    // [windows] the windows added on the class whose first occurrence this is
    hu::DeviceArray<unsigned long long> win_off;  // [records + 1], unless the index keeps one
    const unsigned long long *d_win_off() const { return win_off ? win_off.get() : ix->win_off.get(); }
};

TigTally *device_tig_tally_create(const TigIndex *ix) {
    const char *fn = "mtg_tig_tally_create";
    if (!ix->locating) MTG_DIE("%s: the index keeps no positions of its heavy buckets (build it with mtg_tig_index_build_locating)", fn);
    on_device(ix->device_id);
    hipStream_t st = nullptr;
    const uint64_t n = ix->info.records, k = ix->info.k;
    TigTally *t = new TigTally{ix, ix->device_id, ix->info.occurrences, n, {}, {}};
    t->count.alloc(std::max<uint64_t>(t->windows, 1));  // (an index without windows: never read)
    if (!ix->win_off) {  // the windows of the records before, from the index's own offsets
        std::vector<unsigned long long> off(n + 1, 0), win_off(n + 1, 0);
        hu::download_sliced(off.data(), ix->off.get(), (n + 1) * 8, st, ix->device_id);
        for (uint64_t r = 0; r < n; r++) win_off[r + 1] = win_off[r] + (off[r + 1] - off[r] >= k ? off[r + 1] - off[r] - k + 1 : 0);
        t->win_off.alloc(n + 1);
        hu::upload_sliced(t->win_off, win_off.data(), (n + 1) * 8, st, ix->device_id);
        HIP_CHECK(hipStreamSynchronize(st));  // (win_off leaves its scope)
    }
    device_tig_tally_reset(t);
    return t;
}

uint64_t device_tig_tally_device_bytes(const TigTally *t) { return t->windows * 8 + (t->win_off ? (t->records + 1) * 8 : 0); }
uint64_t device_tig_tally_windows(const TigTally *t) { return t->windows; }

void device_tig_tally_reset(TigTally *t) {
    on_device(t->device_id);
    if (!t->windows) return;
    HIP_CHECK(hipMemsetAsync(t->count, 0, t->windows * 8, nullptr));
    HIP_CHECK(hipStreamSynchronize(nullptr));
}

void device_tig_tally_counters(const TigTally *t, uint64_t *out) {
    if (t->windows && !out) MTG_DIE("mtg_tig_tally_counters: null argument");
    on_device(t->device_id);
    if (t->windows) hu::download_sliced(out, t->count.get(), t->windows * 8, nullptr, t->device_id);
}

void device_tig_tally_free(TigTally *t) {
    if (!t) return;
    int cur = 0;  // (as an index: it may die on a thread whose current device is another one)
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(t->device_id);
    delete t;
    (void)hipSetDevice(cur);
}

void device_tig_tally_add(TigTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid, uint64_t *found,
                          TigTallyTimes *times) {
    const char *fn = "mtg_tig_tally_add";
    const TigIndex *ix = t->ix;
    const uint64_t n_bases = locate_windows(fn, ix, seq, off, n, kmers, valid, found, false);
    if (times) *times = TigTallyTimes();
    if (n_bases == 0) return;  // nothing to look at
    LocateProbe p(ix, seq, off, n);
    GatherErr err(p.st);
    const tp::GatherArgs g{p.d_hit, p.store.off, ix->off, t->d_win_off(), n_bases, n, ix->info.records, err.d};
    tt::tig_tally_add_kernel<<<hu::grid_for((n_bases + RUN - 1) / RUN), hu::EB, 0, p.st>>>(g, t->windows, t->count);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(2, p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    const auto t0 = std::chrono::steady_clock::now();
    p.download_counts(valid, found);
    err.fetch(p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    err.check(fn);
    if (times) *times = TigTallyTimes{p.store.upload_ms, p.store.pack_ms, p.ev.ms(0, 1), p.ev.ms(1, 2), ms_since(t0)};
}

void device_tig_tally_coverage(const TigTally *t, const char *seq, const uint64_t *off, uint64_t n, uint64_t *kmers, uint64_t *valid,
                               uint64_t *found, uint64_t *covered, uint64_t *sum, uint64_t *max, uint64_t *per_window, TigTallyTimes *times) {
    const char *fn = "mtg_tig_tally_coverage";
    const TigIndex *ix = t->ix;
    const uint64_t n_bases = locate_windows(fn, ix, seq, off, n, kmers, valid, found, n && (!covered || !sum || !max));
    std::fill(covered, covered + n, 0ull);
    std::fill(sum, sum + n, 0ull);
    std::fill(max, max + n, 0ull);
    if (times) *times = TigTallyTimes();
    if (n_bases == 0) return;  // nothing to look at
    LocateProbe p(ix, seq, off, n);
    hu::DeviceArray<unsigned long long> d_out(3 * n), d_per_window;  // covered, sum, max
    if (per_window) d_per_window.alloc(n_bases);
    GatherErr err(p.st);
    HIP_CHECK(hipMemsetAsync(d_out, 0, 3 * n * 8, p.st));
    const tp::GatherArgs g{p.d_hit, p.store.off, ix->off, t->d_win_off(), n_bases, n, ix->info.records, err.d};
    // (one thread per run of positions: every word of per_window is written)
    tt::tig_coverage_gather_kernel<<<hu::grid_for((n_bases + RUN - 1) / RUN), hu::EB, 0, p.st>>>(g, t->windows, t->count, d_out, d_per_window);
    HIP_CHECK(hipGetLastError());
    p.ev.mark(2, p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    const auto t0 = std::chrono::steady_clock::now();
    p.download_counts(valid, found);
    err.fetch(p.st);
    HIP_CHECK(hipStreamSynchronize(p.st));
    err.check(fn);
    hu::download_sliced(covered, d_out.get(), n * 8, p.st, p.device_id);
    hu::download_sliced(sum, d_out + n, n * 8, p.st, p.device_id);
    hu::download_sliced(max, d_out + 2 * n, n * 8, p.st, p.device_id);
    if (per_window) hu::download_sliced(per_window, d_per_window.get(), n_bases * 8, p.st, p.device_id);
    if (times) *times = TigTallyTimes{p.store.upload_ms, p.store.pack_ms, p.ev.ms(0, 1), p.ev.ms(1, 2), ms_since(t0)};
}

}  // namespace mtg

// ---- the index as a file ----
#include "tig_index_file_device.hpp"
