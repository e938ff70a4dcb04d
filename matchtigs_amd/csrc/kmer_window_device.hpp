// kmer_window_device.hpp -- k-mer classes {x, rc(x)} over a 2-bit packed sequence store (pack_device.hpp), shared by the plain-FASTA
// join (fasta_in_device.hip), the k-mer set comparison (kmer_compare_device.hip), the unitig compaction (compact_device.hip) and the
// k-mer index (kmer_query_device.hip):
// the rolling walk over the windows of a record (for_each_window), the canonical key of the bases at one position (class_key) and the
// open-addressing table of classes (find_slot, with the exactness argument every caller relies on).
//
// The walk: a thread owns RUN consecutive window start positions. It finds the record of the first one by a binary search in the
// offsets and then cuts its run at every record end it meets (no per-base flag array). Inside a record it reads the packed words once,
// front to back, and ROLLS the window: for k <= 31 the forward and the reverse-complement 2-bit codes (2 bits in, 2 bits out), beyond
// that two polynomial hashes mod 2^64 of the forward and the reverse-complement string (one base in, one base out, whatever k is; a
// second reader k bases behind supplies the base that leaves). Identity beyond what a hash can say is decided base by base in the
// packed store (same_class: x == y or x == rc(y), 16 bases per compare), so nothing probabilistic remains.
// Everything here is a device inline or a template: each translation unit that includes the header gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pack_device.hpp"

namespace mtg {
namespace kw {

constexpr int RUN = 64;                                    // window start positions per thread
constexpr uint64_t POS_LIMIT = (1ull << 40) - 1;           // global positions are < this
constexpr uint64_t POLY_BASE = 0x9e3779b97f4a7c15ull;      // odd: invertible mod 2^64

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64's finaliser: a bijection of 64-bit words
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// what the window walk reads
struct WindowArgs {
    const uint32_t *packed;         // the bases (SeqStore::packed)
    const unsigned long long *off;  // [records + 1] global base offsets
    uint64_t k;
    uint64_t top;        // k <= 31: 2 (k - 1), where a base enters the reverse-complement code
    uint64_t kmask;      // k <= 31: the 2 k low bits
    uint64_t pow_k1;     // k >= 32: POLY_BASE^(k-1)
    uint64_t inv_base;   // k >= 32: POLY_BASE^-1
};
// the constants of the rolling walk for this k (host side)
inline void window_args_set_k(WindowArgs &a, uint64_t k) {
    a.k = k;
    if (k < 32) {
        a.top = 2 * (k - 1);
        a.kmask = (1ull << (2 * k)) - 1;
    } else {
        a.pow_k1 = 1;
        for (uint64_t i = 1; i < k; i++) a.pow_k1 *= POLY_BASE;
        a.inv_base = POLY_BASE;  // Newton's iteration doubles the correct low bits: 3 -> 6 -> ... -> 96
        for (int i = 0; i < 5; i++) a.inv_base *= 2 - POLY_BASE * a.inv_base;
    }
}

// the bases of the packed store from `pos` on, one at a time; every word is loaded once
struct BaseReader {
    const uint32_t *packed;
    uint64_t pos;
    uint32_t w;
    __device__ __forceinline__ BaseReader(const uint32_t *p, uint64_t at) : packed(p), pos(at), w(p[at >> 4] >> (2 * (at & 15))) {}
    __device__ __forceinline__ uint32_t next() {
        const uint32_t c = w & 3u;
        pos++;
        w = (pos & 15) ? w >> 2 : packed[pos >> 4];  // (the word behind the last base is padding)
        return c;
    }
};

// 16 bases from `pos` on, base pos in the lowest bits
__device__ __forceinline__ uint32_t bases16(const uint32_t *packed, uint64_t pos) {
    const uint64_t w = pos >> 4;
    const uint32_t s = 2 * (uint32_t)(pos & 15);
    const uint32_t lo = packed[w];
    return s ? (lo >> s) | (packed[w + 1] << (32 - s)) : lo;
}
// the reverse complement of 16 bases: 2-bit groups in reverse order, each complemented (3 - c)
__device__ __forceinline__ uint32_t revcomp16(uint32_t v) {
    const uint32_t r = __brev(v);
    return ~(((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1));
}
// the window x at p of the store px and the window y at q of the store py are the same k-mer class: x == y or x == rc(y)
__device__ inline bool same_class(const uint32_t *px, uint64_t p, const uint32_t *py, uint64_t q, uint64_t k) {
    bool eq = true;
    for (uint64_t i = 0; i < k && eq; i += 16) {
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        eq = ((bases16(px, p + i) ^ bases16(py, q + i)) & m) == 0;
    }
    if (eq) return true;
    for (uint64_t i = 0; i < k; i += 16) {  // x[i .. i + n) against the reverse complement of y[k - i - n .. k - i)
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        const uint32_t y = revcomp16(bases16(py, q + k - i - n) & m) >> (2 * (16 - n));
        if ((bases16(px, p + i) ^ y) & m) return false;
    }
    return true;
}
// ... where x is the window at p of px with its base j < k REPLACED: flip = old ^ new, XORed into the 16-base chunk that holds base j.
// As exact as same_class: the same two passes over the same chunks.
__device__ inline bool same_class_patched(const uint32_t *px, uint64_t p, uint64_t j, uint32_t flip, const uint32_t *py, uint64_t q, uint64_t k) {
    const uint64_t ji = j & ~15ull;                    // the chunk of base j starts at base ji of x
    const uint32_t patch = flip << (2 * (j & 15));
    bool eq = true;
    for (uint64_t i = 0; i < k && eq; i += 16) {
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        const uint32_t x = bases16(px, p + i) ^ (i == ji ? patch : 0u);
        eq = ((x ^ bases16(py, q + i)) & m) == 0;
    }
    if (eq) return true;
    for (uint64_t i = 0; i < k; i += 16) {  // x[i .. i + n) against the reverse complement of y[k - i - n .. k - i)
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        const uint32_t x = bases16(px, p + i) ^ (i == ji ? patch : 0u);
        const uint32_t y = revcomp16(bases16(py, q + k - i - n) & m) >> (2 * (16 - n));
        if ((x ^ y) & m) return false;
    }
    return true;
}
// ... both in one store
__device__ inline bool same_class(const uint32_t *packed, uint64_t p, uint64_t q, uint64_t k) {
    return p == q || same_class(packed, p, packed, q, k);
}

// the two strand hashes of a string as one hash of its class (the same for x and rc(x)), and the identity word a table keeps for
// a class too long for a code: 22 bits of that hash as a tag, then the position of one occurrence
__device__ __forceinline__ uint64_t strands_hash(uint64_t hf, uint64_t hr) { return mix64(hf) + mix64(hr); }
__device__ __forceinline__ uint64_t tagged_pos(uint64_t hash, uint64_t pos) { return ((hash & 0x3FFFFFull) << 40) | pos; }

// What a window is to a table. k <= 31: `ident` is the canonical code. k >= 32: tagged_pos.
struct Window {
    uint64_t hash, ident;
};

// Calls op(q, r, window) for every window start q in [p0, p1) of the records [rec_lo, rec_hi), whose bases are [off[rec_lo], off[rec_hi]);
// r is the record of q. q ascends; it skips whatever starts no window (the last k - 1 bases of a record, records shorter than k).
template <bool WIDE, typename Op>
__device__ __forceinline__ void for_each_window(const WindowArgs &a, uint64_t p0, uint64_t p1, uint64_t rec_lo, uint64_t rec_hi, Op op) {
    uint64_t lo = rec_lo, hi = rec_hi;  // the last record that starts at or before p0 (off[rec_lo] <= p0 < off[rec_hi])
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.off[mid] <= p0) lo = mid;
        else hi = mid;
    }
    uint64_t r = lo, p = p0;
    const uint64_t k = a.k;
    while (p < p1) {
        const uint64_t rec_end = a.off[r + 1];
        if (rec_end < p + k) {  // no window of this record starts at p or later
            if (++r >= rec_hi) break;
            p = a.off[r] > p ? (uint64_t)a.off[r] : p;
            continue;
        }
        const uint64_t last = p1 < rec_end - k + 1 ? p1 : rec_end - k + 1;
        BaseReader lead(a.packed, p);
        if (!WIDE) {
            uint64_t fwd = 0, rc = 0;  // first base in the highest bits: numeric order is lexicographic order
            for (uint64_t i = 0; i + 1 < k; i++) {
                const uint64_t c = lead.next();
                fwd = (fwd << 2) | c;
                rc = (rc >> 2) | ((3 - c) << a.top);
            }
            for (uint64_t q = p; q < last; q++) {
                const uint64_t c = lead.next();
                fwd = ((fwd << 2) | c) & a.kmask;
                rc = (rc >> 2) | ((3 - c) << a.top);
                const uint64_t canon = fwd < rc ? fwd : rc;
                op(q, r, Window{mix64(canon), canon});
            }
        } else {
            BaseReader trail(a.packed, p);
            uint64_t hf = 0, hr = 0, pw = 1;  // hf = sum (x_i + 1) B^(k-1-i), hr = sum (4 - x_i) B^i = hf of rc(x)
            for (uint64_t i = 0; i < k; i++) {
                const uint64_t c = lead.next();
                hf = hf * POLY_BASE + (c + 1);
                hr += (4 - c) * pw;
                pw *= POLY_BASE;
            }
            for (uint64_t q = p;;) {
                const uint64_t h = strands_hash(hf, hr);
                op(q, r, Window{h, tagged_pos(h, q)});
                if (++q >= last) break;
                const uint64_t o = trail.next(), c = lead.next();
                hf = (hf - (o + 1) * a.pow_k1) * POLY_BASE + (c + 1);
                hr = (hr - (4 - o)) * a.inv_base + (4 - c) * a.pow_k1;
            }
        }
        p = last;
    }
}

// The key of the class of the L bases at `pos`, not rolled (the (k-1)-mer ends of the join and of the compaction's nodes).
// flip: the canonical form (the lexicographically smaller of x and rc(x)) is rc(x); pal: x == rc(x). L <= 32: `ident` is the
// canonical code (never all ones: T...T is not canonical) and `hash` a bijection of it, so equal hashes ARE equal classes. Beyond:
// `hash` only places and pre-filters, `ident` is tagged_pos and identity is same_class.
struct ClassKey {
    uint64_t hash, ident;
    bool flip, pal;
};
__device__ __forceinline__ ClassKey class_key(const uint32_t *packed, uint64_t pos, uint64_t L) {
    ClassKey key;
    BaseReader rd(packed, pos);
    if (L <= 32) {
        uint64_t fwd = 0, rc = 0;  // first base in the highest bits: numeric order is lexicographic order
        for (uint64_t i = 0; i < L; i++) {
            const uint64_t c = rd.next();
            fwd = (fwd << 2) | c;
            rc |= (3ull - c) << (2 * i);
        }
        key.flip = rc < fwd;
        key.pal = rc == fwd;
        key.ident = key.flip ? rc : fwd;
        key.hash = mix64(key.ident);
    } else {
        int cmp = 0;
        for (uint64_t i = 0; i < L && !cmp; i++) {
            const uint32_t x = packed_base(packed, pos + i), y = 3u - packed_base(packed, pos + L - 1 - i);
            cmp = x < y ? -1 : (x > y ? 1 : 0);
        }
        key.flip = cmp > 0;
        key.pal = cmp == 0;
        uint64_t hf = 0, hr = 0, pw = 1;
        for (uint64_t i = 0; i < L; i++) {
            const uint64_t c = rd.next();
            hf = hf * POLY_BASE + (c + 1);
            hr += (4 - c) * pw;
            pw *= POLY_BASE;
        }
        key.hash = strands_hash(hf, hr);
        key.ident = tagged_pos(key.hash, pos);
    }
    return key;
}

// ---- the table of classes ----
// Open addressing in HBM: 64-bit slots, EMPTY_SLOT marks a free one (no caller's word is all ones: a canonical code is never T...T,
// and every other word holds a position or an occurrence number below its field's all-ones value), linear probing from
// umulhi(hash, slots) on a table of any size. A slot's word = what names the class (a code, or a tag plus where to find one of its
// occurrences) | the caller's payload; `same(word)` says whether an occupied slot holds the caller's class.
//
// Exactness. `same` is exact for every caller: either it compares canonical codes (hashes that are bijections of them), or a tag
// match only pre-filters and kw::same_class settles identity base by base in the packed store. A hash collision costs a compare,
// never a wrong answer.
//
// Order independence. An empty slot is claimed by CAS, and a claimed slot never changes its class (callers only lower the
// payload among occurrences of that class, or OR bits into it). A probe for class c starts at a slot that depends on c alone and
// walks on until it meets a slot that is empty or holds c. Slots only go from empty to occupied, so what a probe for c has walked
// over stays in its way: every later probe for c walks over the same slots and ends at the one that holds c.
// Hence every class owns exactly one slot. WHICH slot, and which occurrence claimed it, depends on the order the CAS land in; the
// callers take from a slot only what does not: a minimum (atomicMin), a union of bits (atomicOr), a multiset of insertions, or
// -- after the inserting kernel has finished -- the slot as the class's name.
//
// find_slot returns the slot of the class and the word found there. CLAIM: an empty slot on the way is claimed with `mine`, and
// the word returned is then EMPTY_SLOT (the caller's word is in, nothing to merge). slot == slots: the class is absent (!CLAIM) or
// the table is full (CLAIM; callers size it at 2 slots per insertion at the least, so this is an internal error).
constexpr unsigned long long EMPTY_SLOT = ~0ull;
struct Found {
    uint64_t slot;
    unsigned long long word;
};
template <bool CLAIM, typename Same>
__device__ __forceinline__ Found find_slot(unsigned long long *table, uint64_t slots, uint64_t hash, unsigned long long mine, Same same) {
    uint64_t s = __umul64hi(hash, slots);
    for (uint64_t probe = 0; probe < slots; probe++) {
        unsigned long long cur = CLAIM ? __hip_atomic_load(&table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : table[s];
        if (cur == EMPTY_SLOT) {
            if (!CLAIM) break;
            cur = atomicCAS(&table[s], EMPTY_SLOT, mine);
            if (cur == EMPTY_SLOT) return Found{s, EMPTY_SLOT};
        }
        if (same(cur)) return Found{s, cur};
        if (++s == slots) s = 0;
    }
    return Found{slots, EMPTY_SLOT};
}

}  // namespace kw
}  // namespace mtg
