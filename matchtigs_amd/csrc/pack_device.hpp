// pack_device.hpp -- the 2-bit packed unitig store on the device, shared by the tig spelling (spell_device.hip) and the plain-FASTA
// join (fasta_in_device.hip). Only ACGT (either case) is representable, like the reference's DnaAlphabet store.
// Layout: 16 bases per 32-bit word, base b at bits [2b, 2b+2), A C G T = 0 1 2 3 (so the complement of c is 3 - c).
// Every kernel here is `static`: each translation unit that includes the header gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

__device__ __forceinline__ uint32_t packed_base(const uint32_t *packed, uint64_t b) { return (packed[b >> 4] >> (2 * (b & 15))) & 3u; }

}  // namespace mtg
