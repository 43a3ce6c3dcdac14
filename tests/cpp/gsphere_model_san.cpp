// gsphere_model_san.cpp -- gsphere_model.hpp on the host: the parameter space, the vote as the
// kernel takes it (box, bound, search of all cells), the filter's ordered sum and the two host
// phases, built with -fsanitize=address,undefined by tests/test_gauss_sphere.py (a stand-alone
// program: nothing of it is loaded into another process).
//
// usage: gsphere_model_san IN OUT
// IN:  int32 n, then 10 x 4 bytes: the dlg_gs_params fields in order, then n x 3 float normals
// OUT: int32 cells, int32 n_sinks, int32 n_fallback, then cells x 3 float corners, n int32
//      cell_of_point, cells int32 raw votes, cells int32 filtered votes, cells int32 sink_init,
//      cells int32 sink, n_sinks int32 sink cells, n_sinks int64 vote_num
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/dialog_ransac.h"
#include "gsphere_model.hpp"

using namespace dlg;

template <typename T>
static bool put(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0;
  dlg_gs_params prm;
  static_assert(sizeof(prm) == 40, "ten 4-byte fields");
  bool ok = fread(&n, 4, 1, f) == 1 && fread(&prm, sizeof(prm), 1, f) == 1 && n >= 0;
  std::vector<float> nrm(3 * (size_t)(ok ? n : 0));
  ok = ok && (nrm.empty() || fread(nrm.data(), 4, nrm.size(), f) == nrm.size());
  fclose(f);
  if (!ok || !gs::valid_res(prm.num_res)) return 2;

  const gs::Space S = gs::build_space(prm.num_res);
  const int32_t cells = S.cells();
  std::vector<float> corners;
  for (int32_t c = 0; c < cells; ++c) {
    corners.push_back(S.px[(size_t)c]);
    corners.push_back(S.py[(size_t)c]);
    corners.push_back(S.pz[(size_t)c]);
  }
  std::vector<int32_t> cell_of((size_t)n), raw((size_t)cells, 0), filt((size_t)cells, 0);
  int32_t n_fallback = 0;
  for (int32_t i = 0; i < n; ++i) {
    bool fb = false;
    const int32_t c = cells ? gs::vote_cell(S, nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1],
                                            nrm[3 * (size_t)i + 2], &fb)
                            : -1;
    cell_of[(size_t)i] = c;
    if (c >= 0) ++raw[(size_t)c];
    n_fallback += fb;
  }
  std::vector<uint64_t> scratch;
  for (int32_t c = 0; c < cells; ++c)
    filt[(size_t)c] = gs::filter_cell(S, raw.data(), c, prm.std_dev_gaussian, scratch);
  std::vector<int32_t> sink_init, sink;
  const std::vector<gs::Sink> sinks = gs::gradient_field(
      S, filt.data(), raw.data(), prm.search_radius_create_gradient, prm.t_vote_num, sink_init);
  gs::rectify_sinks(S, sinks, sink_init, prm.radius_base, prm.delta_radius, prm.s_threshold,
                    prm.dev_threshold, sink);
  std::vector<int32_t> sc;
  std::vector<int64_t> sv;
  for (const gs::Sink& s : sinks) {
    sc.push_back(s.index);
    sv.push_back(s.vote_num);
  }
  const int32_t head[3] = {cells, (int32_t)sinks.size(), n_fallback};
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  ok = fwrite(head, 4, 3, f) == 3 && put(f, corners) && put(f, cell_of) && put(f, raw) &&
       put(f, filt) && put(f, sink_init) && put(f, sink) && put(f, sc) && put(f, sv);
  return fclose(f) == 0 && ok ? 0 : 2;
}
