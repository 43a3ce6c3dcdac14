// voxel_model.hpp -- the grid and key arithmetic of pcl::VoxelGrid<PointXYZ>::applyFilter (PCL 1.8
// filters/impl/voxel_grid.hpp restated from memory: parity unpinned), for the host
// and the device alike: one definition, so the key a point gets on the device is the key the host
// (and tests/cpp/voxel_model_san.cpp) computes.
//
// All arithmetic is float, every product rounded on its own (build with -ffp-contract=off, like
// host_math.hpp):
//   inv[a]   = 1.0f / leaf[a]
//   d[a]     = (int64)((max_p[a] - min_p[a]) * inv[a]) + 1;  d0 * d1 * d2 > INT32_MAX: "Leaf size
//              is too small" (kVoxelTooSmall)
//   min_b[a] = (int)floorf(min_p[a] * inv[a]), max_b likewise; a floorf outside the int range is
//              undefined in PCL's cast: kVoxelOutOfInt
//   div[a]   = max_b[a] - min_b[a] + 1;  mul = (1, div0, div0 * div1)
//   ijk[a]   = (int)(floorf(p[a] * inv[a]) - (float)min_b[a])
//   key      = ijk0 * mul0 + ijk1 * mul1 + ijk2 * mul2  in unsigned 32-bit arithmetic (a wrap
//              merges voxels as PCL's int arithmetic would)
// Plain C++ without HIP too (the sanitizer program).
#pragma once

#include <cmath>
#include <cstdint>

#include "host_math.hpp"  // DLG_HD

namespace dlg {

enum { kVoxelOk = 0, kVoxelTooSmall = 1, kVoxelOutOfInt = 2 };

struct VoxelDesc {
  float inv[3];
  int32_t min_b[3];
  int32_t div[3];
  uint32_t mul[3];
};

// floorf(v * inv), the one expression both the grid origin and the keys are made of
DLG_HD inline float voxel_cell(float v, float inv) { return floorf(v * inv); }

// the grid of a cloud whose finite points span [mn, mx] (steps 1, 5, 6); g is filled as far as
// the verdict allows (inv always)
inline int voxel_make_desc(const float leaf[3], const float mn[3], const float mx[3], VoxelDesc* g) {
  for (int a = 0; a < 3; ++a) g->inv[a] = 1.0f / leaf[a];
  int64_t d[3];
  for (int a = 0; a < 3; ++a) {
    const float t = (mx[a] - mn[a]) * g->inv[a];
    // (beyond the int64 cast's range -- an infinite extent or product -- the count is over any limit)
    if (!(t < 2147483648.0f)) return kVoxelTooSmall;
    d[a] = (int64_t)t + 1;
  }
  if (d[0] * d[1] > (int64_t)INT32_MAX || d[0] * d[1] * d[2] > (int64_t)INT32_MAX)
    return kVoxelTooSmall;
  int64_t mxb[3];
  for (int a = 0; a < 3; ++a) {
    const float lo = voxel_cell(mn[a], g->inv[a]), hi = voxel_cell(mx[a], g->inv[a]);
    if (!(lo >= -2147483648.0f && lo < 2147483648.0f && hi >= -2147483648.0f && hi < 2147483648.0f))
      return kVoxelOutOfInt;
    g->min_b[a] = (int32_t)lo;
    mxb[a] = (int64_t)(int32_t)hi;
  }
  for (int a = 0; a < 3; ++a) {
    // (d bounds the float product of the extent, div the difference of two rounded products: near
    // 2^31 cells on one axis div can pass INT32_MAX where d did not -- PCL's int would overflow)
    const int64_t dv = mxb[a] - (int64_t)g->min_b[a] + 1;
    if (dv > (int64_t)INT32_MAX) return kVoxelTooSmall;
    g->div[a] = (int32_t)dv;
  }
  g->mul[0] = 1u;
  g->mul[1] = (uint32_t)g->div[0];
  g->mul[2] = (uint32_t)g->div[0] * (uint32_t)g->div[1];
  return kVoxelOk;
}

// step 7 for a finite point inside [mn, mx]: the float difference is >= 0 and < 2^32 there, so
// the unsigned conversion is defined and equals PCL's int one wherever that is
DLG_HD inline uint32_t voxel_key(const VoxelDesc& g, float x, float y, float z) {
  const uint32_t i = (uint32_t)(voxel_cell(x, g.inv[0]) - (float)g.min_b[0]);
  const uint32_t j = (uint32_t)(voxel_cell(y, g.inv[1]) - (float)g.min_b[1]);
  const uint32_t k = (uint32_t)(voxel_cell(z, g.inv[2]) - (float)g.min_b[2]);
  return i * g.mul[0] + j * g.mul[1] + k * g.mul[2];
}

// radix-sort key bits: every key is below div0 * div1 * div2 while that product stays within 2^32
// and every ijk[a] <= div[a] - 1.  The latter is exact while div[a] - 1 <= 2^24 (the float
// difference of two integers of that size is exact); on a longer axis the difference can round up
// past div[a] - 1, so such a grid sorts on all 32 bits.
inline int voxel_key_bits(const VoxelDesc& g) {
  for (int k = 0; k < 3; ++k)
    if (g.div[k] > (1 << 24)) return 32;
  const uint64_t a = (uint64_t)g.div[0] * (uint64_t)g.div[1];  // < 2^62
  if (a > 0xFFFFFFFFull || a * (uint64_t)g.div[2] > 0xFFFFFFFFull) return 32;
  const uint64_t total = a * (uint64_t)g.div[2];
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < total) ++bits;
  return bits;
}

}  // namespace dlg
