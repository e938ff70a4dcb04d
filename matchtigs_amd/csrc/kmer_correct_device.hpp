// kmer_correct_device.hpp -- correct the substitution errors of reads against the k-mers of a table index
//
// The query pass of kmer_query_device.hip (query_kernel, unchanged) leaves two bit arrays over the global base positions of the reads:
// valid_bits (a valid window starts here) and present_bits (... and it is in the index). This header holds what turns them into
// substitutions, round by round, without downloading them.
//
// The rule (exact integers; include/mtg_engine.h states it too). For base p of a record [s, e) with e - s >= k, cover(p) = the valid
// window starts in [max(s, p - k + 1), min(p, e - k)]. p is a CANDIDATE iff cover(p) is not empty (so x[p] is good) and none of its
// windows is present. S(p, b) = the windows of cover(p) that are in the index with x[p] alone replaced by b, for the three b != x[p].
// best = max S, need = min(W, |cover(p)|): best < need -> nothing; two b at best -> AMBIGUOUS, nothing; else p becomes that b.
// Every decision of a round reads the round's input text; the substitutions are applied together afterwards.
//
//   flag      correct_flag_kernel: a thread owns 64 bases = one word of candidate bits. It finds the record of its first base by a
//             search in the offsets and walks on over the record ends; per base two bit-range tests (any_bit) on the two arrays,
//             clipped to the record. Out: the word and its popcount; hu::scan_u32 ranks the words and correct_list_kernel writes the
//             candidates' positions, ascending, into a list sized from the count.
//   evaluate  correct_eval_kernel, the hot path: one wave per candidate, grid-striding. The 3 c tasks (window w of the c <= k window
//             starts of the range, base b) are dealt over the lanes, task t = 3 w + b. A lane whose window is valid builds the
//             window's identity WITH the substitution -- k <= 31: the canonical code from two bases16 reads, the base XOR-patched
//             before the forward and the reverse-complement form are taken; k >= 32: the two strand hashes with the base's term
//             replaced -- and probes read-only (kw::find_slot<false>); for k >= 32 a tag match is settled base by base
//             (kw::same_class_patched). Per b the wave counts with __ballot and __popcll, so the decision is wave-uniform; lane 0
//             stores the new base and the accept flag and adds the record's candidates (first round) and ambiguous positions, one
//             atomic each.
//   apply     hu::scan_u32 over the accept flags, correct_accept_kernel compacts (position, base), correct_apply_kernel XORs
//             old ^ new into the packed store (atomicXor: two substitutions may share a word; a position appears once per round).
// Sums, a set of positions, XORs of disjoint bit fields: nothing depends on the launch geometry or on the order the atomics land in.
//
// No LDS beyond the scan's, no scratch. The kernels are static: every translation unit that includes this compiles its own.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device.hpp"
#include "hip_util.hpp"
#include "kmer_runs_device.hpp"
#include "kmer_window_device.hpp"
#include "pack_device.hpp"

namespace mtg {
namespace kc {

struct Args {
    const uint32_t *packed;                   // the reads' bases: the round's text
    const unsigned long long *off;            // [n_rec + 1]
    const unsigned long long *vbits, *pbits;  // [(n_bases + 63) / 64] of the round's query pass
    const uint32_t *index_packed;             // k >= 32: the bases the slots point into
    unsigned long long *table;                // [slots], read only
    uint64_t slots, n_bases, n_rec, k;
    uint64_t kmask;             // k <= 31: the 2 k low bits
    uint64_t pow_k1, inv_base;  // k >= 32: POLY_BASE^(k-1), POLY_BASE^-1
};

constexpr unsigned char NONE = 0xFF;  // a candidate's decision: no substitution

// some bit of [lo, hi] (lo <= hi, both inclusive) is set
__device__ __forceinline__ bool any_bit(const unsigned long long *bits, uint64_t lo, uint64_t hi) {
    const uint64_t w_lo = lo >> 6, w_hi = hi >> 6;
    for (uint64_t w = w_lo; w <= w_hi; w++) {
        unsigned long long m = bits[w];
        if (w == w_lo) m &= ~0ull << (lo & 63);
        if (w == w_hi) m &= ~0ull >> (63 - (hi & 63));
        if (m) return true;
    }
    return false;
}
// the window starts that cover base p of the record [s, e), e - s >= k: [lo, hi], at most k of them
__device__ __forceinline__ void cover_range(uint64_t p, uint64_t s, uint64_t e, uint64_t k, uint64_t &lo, uint64_t &hi) {
    lo = p + 1 >= s + k ? p + 1 - k : s;
    hi = p < e - k ? p : e - k;
}

// cand_bits[g] bit i: base 64 g + i is a candidate; cand_count[g] = its popcount
static __global__ __launch_bounds__(hu::EB) void correct_flag_kernel(Args a, unsigned long long *cand_bits, uint32_t *cand_count) {
    const uint64_t g = hu::gid(), p0 = g * 64;
    if (p0 >= a.n_bases) return;
    const uint64_t p1 = p0 + 64 < a.n_bases ? p0 + 64 : a.n_bases;
    uint64_t r = kr::record_of(a.off, a.n_rec, p0);
    unsigned long long m = 0;
    for (uint64_t p = p0; p < p1; p++) {
        while (a.off[r + 1] <= p) r++;  // (p < n_bases = off[n_rec]: ends at a record that holds p)
        const uint64_t s = a.off[r], e = a.off[r + 1];
        if (e - s < a.k) continue;
        uint64_t lo, hi;
        cover_range(p, s, e, a.k, lo, hi);
        if (any_bit(a.vbits, lo, hi) && !any_bit(a.pbits, lo, hi)) m |= 1ull << (p - p0);
    }
    cand_bits[g] = m;
    cand_count[g] = (uint32_t)__popcll(m);
}

// list[rank[g] ..] = the candidates of word g, ascending (rank: the exclusive scan of cand_count; cap: its total)
static __global__ __launch_bounds__(hu::EB) void correct_list_kernel(const unsigned long long *cand_bits, const unsigned long long *rank, uint64_t words,
                                                                     uint64_t cap, unsigned long long *list) {
    const uint64_t g = hu::gid();
    if (g >= words) return;
    uint64_t at = rank[g];
    for (unsigned long long m = cand_bits[g]; m && at < cap; m &= m - 1) list[at++] = g * 64 + (uint64_t)__builtin_ctzll(m);
}

// the window at i of the reads, its base j (now x) replaced by b, is in the index
template <bool WIDE>
__device__ __forceinline__ bool solid_with(const Args &a, uint64_t i, uint64_t j, uint32_t x, uint32_t b) {
    if (!WIDE) {
        uint64_t v = kw::bases16(a.packed, i);  // base t of the window at bits [2 t, 2 t + 2)
        if (a.k > 16) v |= (uint64_t)kw::bases16(a.packed, i + 16) << 32;
        v = (v ^ ((uint64_t)(x ^ b) << (2 * j))) & a.kmask;
        const uint64_t rc = ~v & a.kmask;  // the reverse complement's code: its first base in the highest bits
        uint64_t f = __brevll(v);          // the 2-bit groups in reverse order ...
        f = ((f >> 1) & 0x5555555555555555ull) | ((f & 0x5555555555555555ull) << 1);
        f >>= 64 - 2 * a.k;                // ... the first base in the highest of the 2 k bits
        const uint64_t canon = f < rc ? f : rc;
        return kw::find_slot<false>(a.table, a.slots, kw::mix64(canon), canon, [&](unsigned long long cur) { return cur == canon; }).slot != a.slots;
    }
    kw::BaseReader rd(a.packed, i);
    uint64_t hf = 0, hr = 0, pw = 1, pf = a.pow_k1, pw_j = 0, pf_j = 0;  // pw = B^t, pf = B^(k-1-t)
    for (uint64_t t = 0; t < a.k; t++) {
        const uint64_t c = rd.next();
        hf = hf * kw::POLY_BASE + (c + 1);
        hr += (4 - c) * pw;
        if (t == j) {
            pw_j = pw;
            pf_j = pf;
        }
        pw *= kw::POLY_BASE;
        pf *= a.inv_base;
    }
    hf += ((uint64_t)b - (uint64_t)x) * pf_j;  // the term (x + 1) B^(k-1-j) becomes (b + 1) B^(k-1-j), mod 2^64
    hr += ((uint64_t)x - (uint64_t)b) * pw_j;  // the term (4 - x) B^j becomes (4 - b) B^j
    const uint64_t h = kw::strands_hash(hf, hr), tag = h & 0x3FFFFFull;
    return kw::find_slot<false>(a.table, a.slots, h, 0ull, [&](unsigned long long cur) {
        return (cur >> 40) == tag && kw::same_class_patched(a.packed, i, j, x ^ b, a.index_packed, cur & kw::POS_LIMIT, a.k);
    }).slot != a.slots;
}

// list: [n_cand] ascending positions. decision[c] = the new base 0..3 or NONE, accept[c] = 1 iff a base; rec_candidates (first round
// only, else null) / rec_ambiguous: [n_rec], added to
template <bool WIDE>
static __global__ __launch_bounds__(hu::EB) void correct_eval_kernel(Args a, const unsigned long long *list, uint64_t n_cand, uint32_t min_solid,
                                                                     unsigned char *decision, uint32_t *accept, unsigned long long *rec_candidates,
                                                                     unsigned long long *rec_ambiguous) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = hu::gid() >> 6, waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t ci = wave; ci < n_cand; ci += waves) {
        const uint64_t p = list[ci];
        const uint64_t r = kr::record_of(a.off, a.n_rec, p);
        uint64_t lo, hi;
        cover_range(p, a.off[r], a.off[r + 1], a.k, lo, hi);
        const uint64_t tasks = 3 * (hi - lo + 1);
        const uint32_t x = packed_base(a.packed, p);
        uint64_t cover = 0, score[3] = {0, 0, 0};  // (wave-uniform)
        for (uint64_t t0 = 0; t0 < tasks; t0 += 64) {
            const uint64_t t = t0 + lane;
            bool valid = false, hit = false;
            uint32_t bi = 0;
            if (t < tasks) {
                const uint64_t w = t / 3, i = lo + w;
                bi = (uint32_t)(t - 3 * w);
                valid = (a.vbits[i >> 6] >> (i & 63)) & 1;
                if (valid) hit = solid_with<WIDE>(a, i, p - i, x, (x + 1 + bi) & 3u);
            }
            cover += (uint64_t)__popcll(__ballot(valid && bi == 0));
            score[0] += (uint64_t)__popcll(__ballot(hit && bi == 0));
            score[1] += (uint64_t)__popcll(__ballot(hit && bi == 1));
            score[2] += (uint64_t)__popcll(__ballot(hit && bi == 2));
        }
        const uint64_t best = score[0] > score[1] ? (score[0] > score[2] ? score[0] : score[2]) : (score[1] > score[2] ? score[1] : score[2]);
        const uint64_t need = min_solid < cover ? min_solid : cover;  // (cover >= 1: p is a candidate)
        const uint32_t winners = (score[0] == best) + (score[1] == best) + (score[2] == best);
        const bool enough = best >= need, ambiguous = enough && winners > 1;
        if (lane == 0) {
            const uint32_t bi = score[0] == best ? 0 : score[1] == best ? 1 : 2;
            const bool take = enough && !ambiguous;
            decision[ci] = take ? (unsigned char)((x + 1 + bi) & 3u) : NONE;
            accept[ci] = take;
            if (rec_candidates) atomicAdd(&rec_candidates[r], 1ull);
            if (ambiguous) atomicAdd(&rec_ambiguous[r], 1ull);
        }
    }
}

// the accepted candidates, in the list's order: pos[rank[c]], base[rank[c]]
static __global__ __launch_bounds__(hu::EB) void correct_accept_kernel(const unsigned long long *list, const unsigned char *decision, const uint32_t *accept,
                                                                       const unsigned long long *rank, uint64_t n_cand, uint64_t cap,
                                                                       unsigned long long *pos, unsigned char *base) {
    const uint64_t c = hu::gid();
    if (c >= n_cand || !accept[c]) return;
    const uint64_t at = rank[c];
    if (at >= cap) return;  // (the scan's total: never)
    pos[at] = list[c];
    base[at] = decision[c];
}

// packed: base pos[i] becomes base[i]. A position appears once in a round's list, so the two bits a thread reads are changed by no
// other thread.
static __global__ __launch_bounds__(hu::EB) void correct_apply_kernel(uint32_t *packed, const unsigned long long *pos, const unsigned char *base,
                                                                      uint64_t n_sub) {
    const uint64_t i = hu::gid();
    if (i >= n_sub) return;
    const uint64_t p = pos[i];
    const uint32_t old = packed_base(packed, p);
    atomicXor(&packed[p >> 4], (old ^ (uint32_t)base[i]) << (2 * (uint32_t)(p & 15)));
}

// The rounds on n_bases >= 1 bases whose first query pass is complete on st (a.vbits / a.pbits). query_pass() runs the next one into
// the same two arrays. d_rec: [2 n_rec] candidates, ambiguous, zeroed. *out gets the positions the rounds substituted, ascending, each
// once with the base its last substitution gave it, the rounds' counts and the phases flag / evaluate / apply.
template <typename QueryPass>
inline void rounds(const Args &a, uint32_t *packed, bool wide, uint32_t min_solid, uint32_t n_rounds, hipStream_t st, int device_id,
                   unsigned long long *d_rec, QueryPass query_pass, KmerCorrectCall *out) {
    const uint64_t words = (a.n_bases + 63) / 64;
    hu::DeviceArray<unsigned long long> d_cand_bits(words), d_word_rank(words);
    hu::DeviceArray<uint32_t> d_cand_count(words);
    hu::ScanScratch<unsigned long long> word_scan(words);
    PhaseEvents<2> ev;
    std::vector<std::pair<uint64_t, uint8_t>> subs;
    for (uint32_t round = 0; round < n_rounds; round++) {
        ev.mark(0, st);
        correct_flag_kernel<<<hu::grid_for(words), hu::EB, 0, st>>>(a, d_cand_bits, d_cand_count);
        HIP_CHECK(hipGetLastError());
        word_scan.scan(st, d_cand_count, words, d_word_rank.get());
        unsigned long long n_cand = 0;
        HIP_CHECK(hipMemcpyAsync(&n_cand, word_scan.total(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemsetAsync(d_rec + a.n_rec, 0, a.n_rec * 8, st));  // ambiguous: the last round's
        if (!n_cand) {
            ev.mark(1, st);
            out->flag_ms += ev.ms(0, 1);
            break;
        }
        hu::DeviceArray<unsigned long long> d_list(n_cand), d_rank(n_cand);
        hu::DeviceArray<unsigned char> d_decision(n_cand);
        hu::DeviceArray<uint32_t> d_accept(n_cand);
        hu::ScanScratch<unsigned long long> scan(n_cand);
        correct_list_kernel<<<hu::grid_for(words), hu::EB, 0, st>>>(d_cand_bits, d_word_rank, words, n_cand, d_list);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        out->flag_ms += ev.ms(0, 1);
        if (round == 0) out->candidates = n_cand;

        ev.mark(0, st);
        // (a wave per candidate, up to 2048 blocks of 4 waves -- the waves 256 CUs hold at once; beyond that a wave strides)
        const unsigned grid = (unsigned)std::min<uint64_t>(hu::grid_for(n_cand * 64), 2048);
        unsigned long long *rec_candidates = round == 0 ? d_rec : nullptr;
        if (wide) correct_eval_kernel<true><<<grid, hu::EB, 0, st>>>(a, d_list, n_cand, min_solid, d_decision, d_accept, rec_candidates, d_rec + a.n_rec);
        else correct_eval_kernel<false><<<grid, hu::EB, 0, st>>>(a, d_list, n_cand, min_solid, d_decision, d_accept, rec_candidates, d_rec + a.n_rec);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        out->evaluate_ms += ev.ms(0, 1);

        ev.mark(0, st);
        scan.scan(st, d_accept, n_cand, d_rank.get());
        unsigned long long n_sub = 0;
        HIP_CHECK(hipMemcpyAsync(&n_sub, scan.total(), 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (n_sub > n_cand) MTG_DIE("mtg_kmer_index_correct: internal error (%llu substitutions of %llu candidates)", n_sub, n_cand);
        out->round_corrected[round] = n_sub;
        if (n_sub) {
            hu::DeviceArray<unsigned long long> d_pos(n_sub);
            hu::DeviceArray<unsigned char> d_base(n_sub);
            correct_accept_kernel<<<hu::grid_for(n_cand), hu::EB, 0, st>>>(d_list, d_decision, d_accept, d_rank, n_cand, n_sub, d_pos, d_base);
            correct_apply_kernel<<<hu::grid_for(n_sub), hu::EB, 0, st>>>(packed, d_pos, d_base, n_sub);
            HIP_CHECK(hipGetLastError());
            ev.mark(1, st);
            out->apply_ms += ev.ms(0, 1);
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<unsigned long long> pos(n_sub);
            std::vector<unsigned char> base(n_sub);
            hu::download_sliced(pos.data(), d_pos.get(), n_sub * 8, st, device_id);
            hu::download_sliced(base.data(), d_base.get(), n_sub, st, device_id);
            for (uint64_t i = 0; i < n_sub; i++) subs.emplace_back(pos[i], "ACGT"[base[i] & 3]);
            out->download_ms += ms_since(t0);
        } else {
            ev.mark(1, st);
            out->apply_ms += ev.ms(0, 1);
            break;  // (every later round would be this one again)
        }
        query_pass();  // the next round's bits, or found_after's
    }
    // (two substitutions of one round that share a window are scored without each other and may leave that window unsolid: such a
    // position can be a candidate again, so a later round's base replaces an earlier one's)
    std::stable_sort(subs.begin(), subs.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    for (size_t i = 0; i < subs.size(); i++) {
        if (i + 1 < subs.size() && subs[i + 1].first == subs[i].first) continue;  // (a later round's follows)
        out->positions.push_back(subs[i].first);
        out->bases.push_back(subs[i].second);
    }
}

}  // namespace kc
}  // namespace mtg
