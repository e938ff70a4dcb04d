// kmer_window_device.hpp -- the walk over the k-mer windows of a 2-bit packed sequence store (pack_device.hpp), shared by the k-mer
// set comparison (kmer_compare_device.hip) and the unitig compaction (compact_device.hip).
//
// A thread owns RUN consecutive window start positions. It finds the record of the first one by a binary search in the offsets and
// then cuts its run at every record end it meets (no per-base flag array). Inside a record it reads the packed words once, front to
// back, and ROLLS the window: for k <= 31 the forward and the reverse-complement 2-bit codes (2 bits in, 2 bits out), beyond that two
// polynomial hashes mod 2^64 of the forward and the reverse-complement string (one base in, one base out, whatever k is; a second
// reader k bases behind supplies the base that leaves). Identity beyond what a hash can say is decided base by base in the packed
// store (same_class: x == y or x == rc(y), 16 bases per compare), so nothing probabilistic remains.
// Everything here is a device inline or a template: each translation unit that includes the header gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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
    const uint32_t *packed;         // the bases (one word of padding behind the last)
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
// the windows at p and q are the same k-mer class: x == y or x == rc(y)
__device__ inline bool same_class(const uint32_t *packed, uint64_t p, uint64_t q, uint64_t k) {
    if (p == q) return true;
    bool eq = true;
    for (uint64_t i = 0; i < k && eq; i += 16) {
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        eq = ((bases16(packed, p + i) ^ bases16(packed, q + i)) & m) == 0;
    }
    if (eq) return true;
    for (uint64_t i = 0; i < k; i += 16) {  // x[i .. i + n) against the reverse complement of y[k - i - n .. k - i)
        const uint32_t n = (uint32_t)(k - i < 16 ? k - i : 16), m = n == 16 ? ~0u : (1u << (2 * n)) - 1;
        const uint32_t y = revcomp16(bases16(packed, q + k - i - n) & m) >> (2 * (16 - n));
        if ((bases16(packed, p + i) ^ y) & m) return false;
    }
    return true;
}

// What a window is to a table. k <= 31: `ident` is the canonical code. k >= 32: tag << 40 | position.
struct Window {
    uint64_t hash, ident;
};

// Calls op(q, window) for every window start q in [p0, p1) of the records [rec_lo, rec_hi), whose bases are [off[rec_lo], off[rec_hi]).
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
                op(q, Window{mix64(canon), canon});
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
                const uint64_t h = mix64(hf) + mix64(hr);  // the same for x and rc(x)
                op(q, Window{h, ((h & 0x3FFFFFull) << 40) | q});
                if (++q >= last) break;
                const uint64_t o = trail.next(), c = lead.next();
                hf = (hf - (o + 1) * a.pow_k1) * POLY_BASE + (c + 1);
                hr = (hr - (4 - o)) * a.inv_base + (4 - c) * a.pow_k1;
            }
        }
        p = last;
    }
}

}  // namespace kw
}  // namespace mtg
