// voxel_host_loop.cpp -- a plain single-threaded C++ loop that downsamples a cloud on a voxel grid
// the way pcl::VoxelGrid<PointXYZ>::applyFilter does, written for tools/bench_voxel.py: the host
// time the GPU path is set against, and the bits it is checked against at the timed sizes.
// A restatement, not PCL: PCL is not linked; the order inside a voxel is list order (stable sort).
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC tools/voxel_host_loop.cpp -o tools/libvoxel_host_loop.so
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {
struct KeyIdx {
  uint32_t key;
  int32_t idx;
};
}  // namespace

// xyz: n packed points; out: up to n packed centroids; counts: up to n.  Returns the number of
// voxels, -1 when the leaf is too small (or the cells leave the int range).
extern "C" int64_t voxel_host_loop(const float* xyz, int64_t n, const float* leaf, float* out,
                                   int32_t* counts) {
  float inv[3], mn[3], mx[3];
  for (int a = 0; a < 3; ++a) {
    inv[a] = 1.0f / leaf[a];
    mn[a] = INFINITY;
    mx[a] = -INFINITY;
  }
  int64_t nf = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + 3 * i;
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
    ++nf;
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], p[a]);
      mx[a] = std::max(mx[a], p[a]);
    }
  }
  if (nf == 0) return 0;
  double cells = 1.0;
  int32_t min_b[3];
  uint32_t div[3];
  for (int a = 0; a < 3; ++a) {
    const float t = (mx[a] - mn[a]) * inv[a];
    if (!(t < 2147483648.0f)) return -1;
    cells *= (double)((int64_t)t + 1);
    const float lo = std::floor(mn[a] * inv[a]), hi = std::floor(mx[a] * inv[a]);
    if (!(std::fabs(lo) < 2147483648.0f && std::fabs(hi) < 2147483648.0f)) return -1;
    min_b[a] = (int32_t)lo;
    div[a] = (uint32_t)((int64_t)hi - (int64_t)lo + 1);
  }
  if (cells > 2147483647.0) return -1;
  const uint32_t mul[3] = {1u, div[0], div[0] * div[1]};
  std::vector<KeyIdx> kv;
  kv.reserve((size_t)nf);
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + 3 * i;
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
    uint32_t key = 0;
    for (int a = 0; a < 3; ++a)
      key += (uint32_t)(int32_t)(std::floor(p[a] * inv[a]) - (float)min_b[a]) * mul[a];
    kv.push_back(KeyIdx{key, (int32_t)i});
  }
  std::stable_sort(kv.begin(), kv.end(),
                   [](const KeyIdx& a, const KeyIdx& b) { return a.key < b.key; });
  int64_t nv = 0;
  for (size_t s = 0; s < kv.size();) {
    size_t e = s;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (; e < kv.size() && kv[e].key == kv[s].key; ++e) {
      const float* p = xyz + 3 * (int64_t)kv[e].idx;
      sx += p[0];
      sy += p[1];
      sz += p[2];
    }
    const float c = (float)(e - s);
    out[3 * nv] = sx / c;
    out[3 * nv + 1] = sy / c;
    out[3 * nv + 2] = sz / c;
    counts[nv] = (int32_t)(e - s);
    ++nv;
    s = e;
  }
  return nv;
}
