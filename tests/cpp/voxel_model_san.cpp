// voxel_model_san.cpp -- dialog_amd/csrc/voxel_model.hpp (the host side of the voxel grid's key
// arithmetic; the device calls the same functions) under ASan + UBSan, host only, no HIP.
// stdin: "lx ly lz n" then n lines "x y z" (hex floats; non-finite points are skipped, as the
// filter skips them).  stdout: "verdict V" (0 ok, 1 leaf too small, 2 outside the int range);
// with verdict 0 also "div a b c", "min_b a b c", "bits B" and one line "keys k0 k1 ..." with the
// key of every finite point in input order.  "empty" when no point is finite.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I dialog_amd/csrc voxel_model_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "voxel_model.hpp"

using namespace dlg;

int main() {
  float leaf[3];
  long n = 0;
  if (std::scanf("%a %a %a %ld", &leaf[0], &leaf[1], &leaf[2], &n) != 4 || n < 0) return 2;
  std::vector<float> p;
  p.reserve(3 * (size_t)n);
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long i = 0; i < n; ++i) {
    float q[3];
    if (std::scanf("%a %a %a", &q[0], &q[1], &q[2]) != 3) return 2;
    if (!(std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]))) continue;
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::fmin(mn[a], q[a]);
      mx[a] = std::fmax(mx[a], q[a]);
      p.push_back(q[a]);
    }
  }
  if (p.empty()) {
    std::printf("empty\n");
    return 0;
  }
  VoxelDesc g{};
  const int verdict = voxel_make_desc(leaf, mn, mx, &g);
  std::printf("verdict %d\n", verdict);
  if (verdict != kVoxelOk) return 0;
  std::printf("div %d %d %d\nmin_b %d %d %d\nbits %d\nkeys", g.div[0], g.div[1], g.div[2],
              g.min_b[0], g.min_b[1], g.min_b[2], voxel_key_bits(g));
  for (size_t i = 0; i < p.size(); i += 3)
    std::printf(" %u", voxel_key(g, p[i], p[i + 1], p[i + 2]));
  std::printf("\n");
  return 0;
}
