// axis_model_san.cpp -- dialog_amd/csrc/axis_model.hpp under ASan + UBSan (host only, no HIP):
// the axis-constrained models' validity function, the float thresholds derived from eps and the
// sample-plane arithmetic.  For each eps the thresholds' verdict must equal the formula's on the
// floats around every threshold, on a sweep of [-1.5, 1.5] and on the non-finite values; planes
// and axes of every kind (zero, denormal, huge, NaN) go through axis_valid / axis_valid_direct,
// which must agree.  Prints "ok <checksum>"; any disagreement exits 1.
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I dialog_amd/csrc axis_model_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "axis_model.hpp"

using namespace dlg;

static uint32_t float_bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

// the floats within k bit patterns of f (through zero; stops at the infinities)
static std::vector<float> around(float f, int k) {
  auto key = [](uint32_t b) -> int64_t {
    return (b & 0x80000000u) ? -(int64_t)(b & 0x7FFFFFFFu) - 1 : (int64_t)(b & 0x7FFFFFFFu);
  };
  std::vector<float> out;
  const int64_t c = key(float_bits(f));
  for (int64_t v = c - k; v <= c + k; ++v) {
    if (v > 0x7F800000ll || v < -0x7F800000ll - 1) continue;
    out.push_back(bits_float(v >= 0 ? (uint32_t)v : (0x80000000u | (uint32_t)(-v - 1))));
  }
  return out;
}

int main() {
  const double eps_list[] = {1e-3, 5.0 * M_PI / 180.0, 30.0 * M_PI / 180.0, 89.9 * M_PI / 180.0,
                             M_PI / 2, 2.0, 1e-12, 0.0, -1.0, INFINITY};
  const int models[] = {kModelPerpendicularPlane, kModelParallelPlane};
  const float unit[3] = {0.0f, 0.0f, 1.0f};
  uint64_t sum = 0;
  long bad = 0;
  for (int model : models) {
    for (double eps : eps_list) {
      const AxisTest t = make_axis_test(model, unit, eps);
      std::vector<float> fs = {INFINITY, -INFINITY, NAN, 0.0f, -0.0f, 1.0f, -1.0f, 7.0f, -7.0f};
      for (float c : {t.t_lo, t.t_hi, -t.t_hi, 0.0f, 1.0f, -1.0f})
        for (float v : around(c, 64)) fs.push_back(v);
      for (int i = -3000; i <= 3000; ++i) fs.push_back((float)i * 0.0005f);
      for (float f : fs) {
        const bool thr = t.mode == kAxisNone || axis_verdict(t, f);
        const bool direct = !(eps > 0.0) ? true
                            : model == kModelPerpendicularPlane ? perpendicular_valid_direct(f, eps)
                                                                : parallel_valid_direct(f, eps);
        if (thr != direct) {
          ++bad;
          std::fprintf(stderr, "model %d eps %.17g f %a: thresholds %d formula %d\n", model, eps,
                       (double)f, (int)thr, (int)direct);
        }
        sum = sum * 31 + (thr ? 1 : 0);
      }
    }
  }
  // planes and axes of every kind through the two entry points
  std::mt19937 g(11);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const float special[] = {0.0f, -0.0f, 1e-42f, 3e38f, -3e38f, NAN, INFINITY, 1.0f};
  for (int model : models) {
    for (int it = 0; it < 4000; ++it) {
      float axis[3], c[3];
      for (int k = 0; k < 3; ++k) {
        axis[k] = it % 7 == 0 ? special[(it / 7 + k) % 8] : u(g) * (it % 3 == 0 ? 10.0f : 1.0f);
        c[k] = it % 11 == 0 ? special[(it / 11 + 2 * k) % 8] : u(g);
      }
      const double eps = eps_list[it % 6];
      const AxisTest t = make_axis_test(model, axis, eps);
      const bool a = axis_valid(t, c[0], c[1], c[2]);
      const bool b = axis_valid_direct(model, axis, eps, c);
      float n[3];
      normalized4(c[0], c[1], c[2], n);
      if (a != b || a != axis_valid_n(t, n[0], n[1], n[2])) {
        ++bad;
        std::fprintf(stderr, "model %d eps %.17g axis %a %a %a plane %a %a %a: %d vs %d\n", model,
                     eps, (double)axis[0], (double)axis[1], (double)axis[2], (double)c[0],
                     (double)c[1], (double)c[2], (int)a, (int)b);
      }
      sum = sum * 31 + (a ? 1 : 0);
    }
  }
  // sample_plane: good, collinear, repeated and non-finite samples
  for (int it = 0; it < 2000; ++it) {
    float p[3][3];
    for (auto& q : p)
      for (float& v : q) v = it % 5 == 0 ? (float)(int)(u(g) * 2.0f) : u(g);
    if (it % 13 == 0) std::memcpy(p[2], p[1], sizeof(p[1]));
    if (it % 17 == 0) p[it % 3][it % 2] = special[it % 8];
    float c[4];
    const bool good = sample_plane(p[0], p[1], p[2], c);
    if (!good && !(c[0] != c[0] && c[3] != c[3])) ++bad;
    sum = sum * 31 + (good ? float_bits(c[0]) ^ float_bits(c[3]) : 0u);
  }
  if (bad) {
    std::fprintf(stderr, "%ld disagreements\n", bad);
    return 1;
  }
  std::printf("ok %llu\n", (unsigned long long)sum);
  return 0;
}
