// union_find_dev.hpp -- the lock-free union-find of the radius connected-components passes
// (postprocess.hip's clusterFilt, gsphere.hip's labelled seeds): parent[] over sorted positions,
// the larger root hooked under the smaller with a CAS.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dlg {

__device__ __forceinline__ int uf_load(int32_t* parent, int x) {
  return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving (benign races: every stored value is an ancestor)
__device__ inline int uf_find(int32_t* parent, int x) {
  int p = uf_load(parent, x);
  while (p != x) {
    const int g = uf_load(parent, p);
    if (g != p)
      __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

__device__ inline void uf_unite(int32_t* parent, int a, int b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    // hook the larger root under the smaller; a failed CAS means a was hooked meanwhile
    const int old = atomicCAS(&parent[a], a, b);
    if (old == a) return;
    a = old;
  }
}

}  // namespace dlg
