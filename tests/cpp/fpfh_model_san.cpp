// fpfh_model_san.cpp -- fpfh_model.hpp's host side over a dumped cloud, built with
// -fsanitize=address,undefined by tests/test_fpfh.py (a stand-alone program: nothing of it is
// loaded into another process).
//
// usage: fpfh_model_san IN OUT
// IN:  int32 n, int32 n_list, float radius, n x 3 float points, n x 3 float normals, n_list int32
// OUT: n x 33 int32 SPFH counts, n_list x 33 float descriptors, n_list int32 neighbour counts,
//      n_list uint8 (1: the double sums' certificate missed)
// The search is the brute-force statement of the contract: every finite point with FLANN's float d2
// below (float)((double)r * (double)r), ordered by (d2, index).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "fpfh_model.hpp"

using namespace dlg;

static float flann_d2(const float* q, const float* p) {
  const float ex = q[0] - p[0], ey = q[1] - p[1], ez = q[2] - p[2];
  return ((0.0f + ex * ex) + ey * ey) + ez * ez;
}

template <typename T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t k) {
  v.resize(k);
  return k == 0 || fread(v.data(), sizeof(T), k, f) == k;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0, n_list = 0;
  float radius = 0.0f;
  std::vector<float> xyz, nrm;
  std::vector<int32_t> lst;
  bool ok = fread(&n, 4, 1, f) == 1 && fread(&n_list, 4, 1, f) == 1 && fread(&radius, 4, 1, f) == 1 &&
            n >= 0 && n_list >= 0;
  ok = ok && read_vec(f, xyz, 3 * (size_t)n) && read_vec(f, nrm, 3 * (size_t)n) &&
       read_vec(f, lst, (size_t)n_list);
  fclose(f);
  if (!ok) return 2;
  const float r2 = (float)((double)radius * (double)radius);
  auto finite = [&](int i) { return fpfh_finite3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]); };
  // neighbours of point i, (d2, index) ascending
  auto search = [&](int i, std::vector<std::pair<float, int32_t>>& out) {
    out.clear();
    for (int j = 0; j < n; ++j) {
      if (!finite(j)) continue;
      const float d2 = flann_d2(&xyz[3 * (size_t)i], &xyz[3 * (size_t)j]);
      if (d2 < r2) out.emplace_back(d2, j);
    }
    std::sort(out.begin(), out.end());
  };
  std::vector<int32_t> counts((size_t)n * kFpfhDim, 0);
  std::vector<float> spfh((size_t)n * kFpfhDim, 0.0f);
  std::vector<std::pair<float, int32_t>> nb;
  std::vector<int32_t> ids;
  std::vector<float> d2s;
  for (int i = 0; i < n; ++i) {
    if (!finite(i)) continue;
    search(i, nb);
    ids.clear();
    for (auto& e : nb) ids.push_back(e.second);
    int32_t* c = &counts[(size_t)i * kFpfhDim];
    (void)fpfh_spfh_counts(xyz.data(), nrm.data(), i, ids.data(), (int)ids.size(), c);
    for (int b = 0; b < kFpfhDim; ++b)
      spfh[(size_t)i * kFpfhDim + b] = fpfh_bin_value((int)ids.size(), c[b]);
  }
  std::vector<float> hist((size_t)n_list * kFpfhDim);
  std::vector<int32_t> nbc((size_t)n_list);
  std::vector<uint8_t> lit((size_t)n_list, 0);
  for (int e = 0; e < n_list; ++e) {
    const int i = lst[e];
    float* h = &hist[(size_t)e * kFpfhDim];
    if (i < 0 || i >= n) return 3;
    if (!finite(i)) {
      for (int b = 0; b < kFpfhDim; ++b) h[b] = std::numeric_limits<float>::quiet_NaN();
      nbc[e] = -1;
      continue;
    }
    search(i, nb);
    ids.clear();
    d2s.clear();
    for (auto& p : nb) {
      d2s.push_back(p.first);
      ids.push_back(p.second);
    }
    lit[e] = fpfh_weight(spfh.data(), ids.data(), d2s.data(), (int)ids.size(), h) ? 0 : 1;
    nbc[e] = (int32_t)ids.size();
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  ok = (counts.empty() || fwrite(counts.data(), 4, counts.size(), f) == counts.size()) &&
       (hist.empty() || fwrite(hist.data(), 4, hist.size(), f) == hist.size()) &&
       (nbc.empty() || fwrite(nbc.data(), 4, nbc.size(), f) == nbc.size()) &&
       (lit.empty() || fwrite(lit.data(), 1, lit.size(), f) == lit.size());
  return fclose(f) == 0 && ok ? 0 : 2;
}
