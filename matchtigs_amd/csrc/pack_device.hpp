// pack_device.hpp -- the 2-bit packed sequence store on the device and the small host-side pieces every sequence stage needs around
// it: the tig spelling (spell_device.hip), the plain-FASTA join (fasta_in_device.hip), the k-mer set comparison
// (kmer_compare_device.hip), the unitig compaction (compact_device.hip) and the k-mer index (kmer_query_device.hip). Only ACGT
// (either case) is representable, like the reference's DnaAlphabet store; the queries of the index, which may hold anything, get a
// mask of the unrepresentable bases beside the store (MaskedSeqStore).
// Layout: 16 bases per 32-bit word, base b at bits [2b, 2b+2), A C G T = 0 1 2 3 (so the complement of c is 3 - c).
// INVARIANT of the store: two zeroed words lie behind the word of the last base, so a reader may load one word past the one it
// needs (kw::bases16, kw::BaseReader in kmer_window_device.hpp) without a bounds check. SeqStore is the only place that allocates it.
// Every kernel here is `static`: each translation unit that includes the header gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>

#include "hip_util.hpp"

namespace mtg {

__device__ __forceinline__ uint32_t base_code(unsigned char c) {  // A C G T (either case) -> 0..3, anything else -> 4
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

// one thread per packed word; *bad = the smallest offset of a character outside ACGT (atomicMin; untouched when there is none)
static __global__ void pack_kernel(const char *ascii, uint64_t n_bases, uint32_t *packed, unsigned long long *bad) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b0 = w * 16;
    if (b0 >= n_bases) return;
    uint32_t v = 0;
    for (int i = 0; i < 16 && b0 + i < n_bases; i++) {
        const uint32_t c = base_code((unsigned char)ascii[b0 + i]);
        if (c > 3) { atomicMin(bad, (unsigned long long)(b0 + i)); continue; }
        v |= c << (2 * i);
    }
    packed[w] = v;
}

// pack_kernel for sequences that may hold anything (the queries of kmer_query_device.hip): a character outside ACGT is packed as
// code 0 and marked in `bad`, one bit per base (base b: bit b & 15 of bad[b >> 4], which on this little-endian machine is bit b & 63
// of the 64-bit word b >> 6). One thread per packed word; the bits behind the last base are 0.
static __global__ void pack_masked_kernel(const char *ascii, uint64_t n_bases, uint32_t *packed, unsigned short *bad) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b0 = w * 16;
    if (b0 >= n_bases) return;
    uint32_t v = 0, m = 0;
    for (int i = 0; i < 16 && b0 + i < n_bases; i++) {
        const uint32_t c = base_code((unsigned char)ascii[b0 + i]);
        if (c > 3) m |= 1u << i;
        else v |= c << (2 * i);
    }
    packed[w] = v;
    bad[w] = (unsigned short)m;
}

__device__ __forceinline__ uint32_t packed_base(const uint32_t *packed, uint64_t b) { return (packed[b >> 4] >> (2 * (b & 15))) & 3u; }

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// N HIP events on one stream: mark(i) between the phases, ms(a, b) = the time from mark a to mark b (waits for mark b)
template <int N>
struct PhaseEvents {
    hipEvent_t ev[N];
    PhaseEvents() { for (hipEvent_t &e : ev) HIP_CHECK(hipEventCreate(&e)); }
    ~PhaseEvents() { for (hipEvent_t &e : ev) (void)hipEventDestroy(e); }
    PhaseEvents(const PhaseEvents &) = delete;
    void mark(int i, hipStream_t st) { HIP_CHECK(hipEventRecord(ev[i], st)); }
    double ms(int a, int b) {
        float f = 0.f;
        HIP_CHECK(hipEventSynchronize(ev[b]));
        HIP_CHECK(hipEventElapsedTime(&f, ev[a], ev[b]));
        return f;
    }
};

// Eight 64-bit scalars on the device that the kernels of a stage report through: [0] the smallest offset of a character outside
// ACGT (all ones: none; pack_kernel), [1] error bits of the class-table kernels (low 32 bits; zero: none), [2..7] the stage's own,
// zeroed. read() brings all eight to h[] and dies on an error bit.
struct ScalarBlock {
    hu::DeviceArray<unsigned long long> d;
    unsigned long long h[8] = {};
    explicit ScalarBlock(hipStream_t st) : d(8) {
        HIP_CHECK(hipMemsetAsync(d, 0, sizeof h, st));
        HIP_CHECK(hipMemsetAsync(d, 0xFF, 8, st));
    }
    unsigned int *err() const { return reinterpret_cast<unsigned int *>(d + 1); }
    void read(hipStream_t st, const char *stage) {
        HIP_CHECK(hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (h[1] & 0xFFFFFFFFull) MTG_DIE("%s: internal error %llu (hash table)", stage, h[1] & 0xFFFFFFFFull);
    }
};

// The packed store of `n_rec` records on the device: bases [off[r], off[r + 1]) are record r, off[0] = 0. The constructor uploads the
// ASCII (`ascii`, followed by the last `tail_bases` bases from `tail` if given) and the offsets, packs, frees the ASCII and dies with
// "`what`: character at offset ..." if a character is outside ACGT. On return the stream is idle, `packed` (padded as the invariant at
// the top says) and `off` are ready, and `small` is the stage's scalar block. All three are owners.
struct SeqStore {
    hu::DeviceArray<uint32_t> packed;
    hu::DeviceArray<unsigned long long> off;  // [n_rec + 1]
    ScalarBlock small;
    uint64_t n_bases, n_words;
    double upload_ms = 0.0, pack_ms = 0.0;

    SeqStore(const char *what, const char *ascii, const uint64_t *h_off, uint64_t n_rec, hipStream_t st, int device_id,
             const char *tail = nullptr, uint64_t tail_bases = 0)
        : small(st), n_bases(h_off[n_rec]), n_words((h_off[n_rec] + 15) / 16) {
        const auto t0 = std::chrono::steady_clock::now();
        hu::DeviceArray<char> d_ascii(n_bases ? n_bases : 1);
        packed.alloc(n_words + 2);
        off.alloc(n_rec + 1);
        HIP_CHECK(hipMemsetAsync(packed + n_words, 0, 8, st));
        hu::upload_sliced(off, h_off, (n_rec + 1) * 8, st, device_id);
        hu::upload_sliced(d_ascii, ascii, n_bases - tail_bases, st, device_id);
        hu::upload_sliced(d_ascii + (n_bases - tail_bases), tail, tail_bases, st, device_id);
        upload_ms = ms_since(t0);
        PhaseEvents<2> ev;
        ev.mark(0, st);
        if (n_words) pack_kernel<<<hu::grid_for(n_words), hu::EB, 0, st>>>(d_ascii, n_bases, packed, small.d);
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        d_ascii.release();  // (synchronises: the pack is done)
        HIP_CHECK(hipMemcpyAsync(small.h, small.d, 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (small.h[0] != ~0ull) MTG_DIE("%s: character at offset %llu is not in the DNA alphabet (ACGT)", what, small.h[0]);
        pack_ms = ev.ms(0, 1);
    }
    // the packed bases and the offsets may leave the store with their ranges (the k-mer index keeps them)
    hu::DeviceArray<uint32_t> take_packed() { return std::move(packed); }
    hu::DeviceArray<unsigned long long> take_off() { return std::move(off); }
};

// SeqStore for records of arbitrary bytes: nothing aborts. A character outside ACGT is packed as A and has its bit set in `bad`
// (bit b & 63 of word b >> 6 for base b; every bit from n_bases on is 0, and one zeroed word lies behind the last).
struct MaskedSeqStore {
    hu::DeviceArray<uint32_t> packed;
    hu::DeviceArray<unsigned long long> off;  // [n_rec + 1]
    hu::DeviceArray<unsigned long long> bad;  // [(n_bases + 63) / 64 + 1]
    uint64_t n_bases, n_words;
    double upload_ms = 0.0, pack_ms = 0.0;

    MaskedSeqStore(const char *ascii, const uint64_t *h_off, uint64_t n_rec, hipStream_t st, int device_id)
        : n_bases(h_off[n_rec]), n_words((h_off[n_rec] + 15) / 16) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t bad_bytes = ((n_bases + 63) / 64 + 1) * 8;
        hu::DeviceArray<char> d_ascii(n_bases ? n_bases : 1);
        packed.alloc(n_words + 2);
        bad.alloc(bad_bytes / 8);
        off.alloc(n_rec + 1);
        HIP_CHECK(hipMemsetAsync(packed + n_words, 0, 8, st));
        HIP_CHECK(hipMemsetAsync(bad, 0, bad_bytes, st));
        hu::upload_sliced(off, h_off, (n_rec + 1) * 8, st, device_id);
        hu::upload_sliced(d_ascii, ascii, n_bases, st, device_id);
        upload_ms = ms_since(t0);
        PhaseEvents<2> ev;
        ev.mark(0, st);
        if (n_words) pack_masked_kernel<<<hu::grid_for(n_words), hu::EB, 0, st>>>(d_ascii, n_bases, packed, reinterpret_cast<unsigned short *>(bad.get()));
        HIP_CHECK(hipGetLastError());
        ev.mark(1, st);
        d_ascii.release();  // (synchronises: the pack is done)
        pack_ms = ev.ms(0, 1);
    }
};

}  // namespace mtg
