// call_args_san.cpp -- dialog_amd/csrc/call_args.hpp under ASan + UBSan (tests/test_call_args.py).
// Feeds every check its edge rows and prints one line per row: "<name>|<status>|<text or result>".
// The point records carry a 4-float buffer at the most, so a check that read xyz, or a list past
// its end, would be a sanitizer finding.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>

#include "call_args.hpp"

namespace {

void row(const char* name, const std::function<std::string()>& f) {
  try {
    const std::string r = f();
    std::printf("%s|%d|%s\n", name, (int)DLG_OK, r.c_str());
  } catch (const dlg::DlgError& e) {
    std::printf("%s|%d|%s\n", name, (int)e.code, e.what());
  }
}

std::string points_row(const dlg_points* p, const char* what, int64_t max_n) {
  dlg::check_points(p, what, max_n);
  return "ok";
}

std::string list_row(const int32_t* idx, int64_t n_idx, int64_t n) {
  return "m=" + std::to_string(dlg::check_list(idx, n_idx, n));
}

std::string guess_row(const float* g) {
  float xf[16];
  dlg::check_guess(g, xf);
  std::string s;
  for (int k = 0; k < 16; ++k) s += (k ? " " : "") + std::to_string((int)xf[k]);
  return s;
}

}  // namespace

int main() {
  using dlg::kMaxGridPoints;
  using dlg::kMaxPoints;
  float* four = new float[4]();  // (heap: ASan guards both ends)
  // ---- point records
  row("points null", [&] { return points_row(nullptr, "points", kMaxPoints); });
  const dlg_points neg{four, -1, 12};
  row("points n=-1", [&] { return points_row(&neg, "points", kMaxPoints); });
  const dlg_points noxyz{nullptr, 4, 12};
  row("source xyz null", [&] { return points_row(&noxyz, "source", kMaxPoints); });
  const dlg_points empty{nullptr, 0, 12};
  row("points empty", [&] { return points_row(&empty, "points", kMaxPoints); });
  const dlg_points s8{four, 1, 8}, s14{four, 1, 14}, s16{four, 1, 16};
  row("points stride 8", [&] { return points_row(&s8, "points", kMaxPoints); });
  row("points stride 14", [&] { return points_row(&s14, "points", kMaxPoints); });
  row("points stride 16", [&] { return points_row(&s16, "points", kMaxPoints); });
  const dlg_points at{four, kMaxPoints, 12}, above{four, kMaxPoints + 1, 12};
  row("target n at 2^31-1", [&] { return points_row(&at, "target", kMaxPoints); });
  row("target n above 2^31-1", [&] { return points_row(&above, "target", kMaxPoints); });
  const dlg_points gat{four, kMaxGridPoints, 12}, gabove{four, kMaxGridPoints + 1, 12};
  row("points n at 2^30-1", [&] { return points_row(&gat, "points", kMaxGridPoints); });
  row("points n above 2^30-1", [&] { return points_row(&gabove, "points", kMaxGridPoints); });
  // ---- index lists over n = 5 points
  int32_t* lst = new int32_t[3]{4, 0, 2};
  row("list none", [&] { return list_row(nullptr, -7, 5); });
  row("list valid", [&] { return list_row(lst, 3, 5); });
  row("list empty", [&] { return list_row(lst, 0, 5); });
  row("list n_indices=-1", [&] { return list_row(lst, -1, 5); });
  row("list too long", [&] { return list_row(lst, kMaxPoints + 1, 5); });
  lst[1] = -1;
  row("list entry -1", [&] { return list_row(lst, 3, 5); });
  lst[1] = 5;
  row("list entry n", [&] { return list_row(lst, 3, 5); });
  // ---- the rest
  for (int64_t s : {12, 16, 20})
    row(("out stride " + std::to_string(s)).c_str(), [&] {
      dlg::check_out_stride(s);
      return std::string("ok");
    });
  float* g = new float[16];
  for (int k = 0; k < 16; ++k) g[k] = (float)(k + 1);
  row("guess null", [&] { return guess_row(nullptr); });
  row("guess given", [&] { return guess_row(g); });
  g[6] = std::numeric_limits<float>::quiet_NaN();
  row("guess NaN", [&] { return guess_row(g); });
  g[6] = 7.0f;
  g[15] = -std::numeric_limits<float>::infinity();
  row("guess inf", [&] { return guess_row(g); });
  for (int world : {1, 2})
    row(("world " + std::to_string(world)).c_str(), [&] {
      dlg::check_whole_cloud(world, "voxel grid");
      return std::string("ok");
    });
  delete[] four;
  delete[] lst;
  delete[] g;
  return 0;
}
