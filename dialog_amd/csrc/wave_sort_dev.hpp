// wave_sort_dev.hpp -- a wave's bitonic sort of 64-bit keys held in registers (normals.hip's
// (d2, index) neighbour order, fpfh.hip's), with the lane exchanges it is built from.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dlg {

// v of lane (lane ^ S), S < 64, without LDS: DPP quad permutes (S = 1, 2), quad reversal then
// half-row mirror (4: l ^ 3 mirrored in 8 lanes is l ^ 4), row rotate by 8 (8), and gfx950's
// row / half-wave swaps (16, 32: the swap of v with itself leaves each lane's partner in one of
// the two results).  The whole wave must be active.
template <int S>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v) {
  if constexpr (S == 1) {
    return __builtin_amdgcn_update_dpp(0u, v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
  } else if constexpr (S == 2) {
    return __builtin_amdgcn_update_dpp(0u, v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
  } else if constexpr (S == 4) {
    const uint32_t r = __builtin_amdgcn_update_dpp(0u, v, 0x1B, 0xF, 0xF, false);  // [3,2,1,0]
    return __builtin_amdgcn_update_dpp(0u, r, 0x141, 0xF, 0xF, false);  // row_half_mirror
  } else if constexpr (S == 8) {
    return __builtin_amdgcn_update_dpp(0u, v, 0x128, 0xF, 0xF, false);  // row_ror:8
  } else if constexpr (S == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (threadIdx.x & 16) ? r[0] : r[1];
  } else {
    static_assert(S == 32, "xor_lane: S in 1..32");
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (threadIdx.x & 32) ? r[0] : r[1];
  }
}

template <int S>
__device__ __forceinline__ uint64_t xor_lane64(uint64_t v) {
  return (uint64_t)xor_lane<S>((uint32_t)v) | ((uint64_t)xor_lane<S>((uint32_t)(v >> 32)) << 32);
}

// one bitonic merge step at in-wave distance S over the E registers (blocks of `size` elements)
template <int E, int S>
__device__ __forceinline__ void bitonic_xstep(uint64_t (&v)[E], int size) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = lane + 64 * j;
    const bool up = (e & size) == 0;  // this element's block sorts ascending
    const bool take_min = ((lane & S) == 0) == up;  // the lower element keeps the min ascending
    const uint64_t o = xor_lane64<S>(v[j]);
    v[j] = (o < v[j]) == take_min ? o : v[j];
  }
}

// bitonic sort of 64 * E keys held E per lane (element e = lane + 64 j), ascending; the steps
// within a wave exchange through DPP / lane swaps (no LDS round trip per step)
template <int E>
__device__ __forceinline__ void wave_bitonic(uint64_t (&v)[E]) {
#pragma unroll
  for (int size = 2; size <= 64 * E; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride >= 64; stride >>= 1) {
      const int js = stride >> 6;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if ((j & js) == 0) {  // (j, j | js): both in this lane
          const bool up = ((j * 64) & size) == 0;
          uint64_t& a = v[j];
          uint64_t& b = v[j | js];
          const bool sw = up ? (a > b) : (a < b);
          if (sw) { const uint64_t t = a; a = b; b = t; }
        }
      }
    }
    if (size >= 64) bitonic_xstep<E, 32>(v, size);
    if (size >= 32) bitonic_xstep<E, 16>(v, size);
    if (size >= 16) bitonic_xstep<E, 8>(v, size);
    if (size >= 8) bitonic_xstep<E, 4>(v, size);
    if (size >= 4) bitonic_xstep<E, 2>(v, size);
    bitonic_xstep<E, 1>(v, size);
  }
}

}  // namespace dlg
