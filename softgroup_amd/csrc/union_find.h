// union_find.h -- the lock-free union-find that mask_split.hip (components of a mask) and geometry.hip (grown
// segments) share.  parent[i] <= i always: find walks strictly descending ids, a root is hooked under a smaller root
// by atomicCAS, a lost race re-finds from the value read.  Nobody waits for anybody; integer atomics only.  The
// smallest id of a component ends up as its root, whatever the order of arrival.
//
// Bounds that do not depend on the data: a find ends after P + 1 steps (ids descend strictly), a union after
// 2 P + 2 rounds (the sum of its two ids descends strictly); a bound that is hit is reported to the caller.
#pragma once
#include "common.h"

namespace sg {

__device__ __forceinline__ int32_t uf_load(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uf_store(int32_t *p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way (a store of a grandparent: any ancestor keeps parent[i] <= i and the
// component).  -1 after P + 1 steps or on a parent that does not descend.
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x, int64_t P) {
  for (int64_t step = 0; step <= P; ++step) {
    const int32_t p = uf_load(&parent[x]);
    if (p == x) return x;
    if (p < 0 || p > x) return -1;
    const int32_t g = uf_load(&parent[p]);
    if (g >= 0 && g < p) uf_store(&parent[x], g);
    x = p;
  }
  return -1;
}

// false when a bound was hit
__device__ __forceinline__ bool uf_unite(int32_t *parent, int32_t a, int32_t b, int64_t P) {
  for (int64_t round = 0; round <= 2 * P + 2; ++round) {
    a = uf_find(parent, a, P);
    b = uf_find(parent, b, P);
    if (a < 0 || b < 0) return false;
    if (a == b) return true;
    if (a < b) {
      const int32_t t = a;
      a = b, b = t;
    }
    const int32_t old = atomicCAS(&parent[a], a, b);             // the larger root under the smaller
    if (old == a) return true;
    a = old;                                                     // lost: somebody hooked a first; old < a
    if (a < 0 || a >= P) return false;
  }
  return false;
}

}  // namespace sg
