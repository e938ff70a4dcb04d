// union_find_device.hpp -- the lock-free union-find of the device stages: the trail labels of euler_device.hip and
// the components of the unitig graph (unitig_components_device.hip). One body for both translation units.
// parent[x] == x marks a root. Relaxed agent-scope atomics: no thread reads data that another published through the parent array,
// only the parent words themselves, and a stale word is an older, still valid, ancestor.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mtg {

// ---- lock-free union-find (links always point to a smaller id, so a root is the smallest id of its set) -----
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    uint32_t cur = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur != x) {
        uint32_t prev = x, next;
        while (cur > (next = __hip_atomic_load(&parent[cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            __hip_atomic_store(&parent[prev], next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
            prev = cur;
            cur = next;
        }
    }
    return cur;
}
// true iff THIS call linked two sets (the successful calls of any concurrent execution form a spanning forest)
__device__ __forceinline__ bool uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicCAS(&parent[a], a, b);  // a > b: hang root a below b
        if (old == a) return true;
        a = uf_find(parent, old);
        b = uf_find(parent, b);
    }
    return false;
}

}  // namespace mtg
