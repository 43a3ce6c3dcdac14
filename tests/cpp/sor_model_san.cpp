// sor_model_san.cpp -- dialog_amd/csrc/sor_model.hpp (the host side of the statistical outlier
// filter's sums; the device calls the same functions) under ASan + UBSan, host only, no HIP.
// stdin: one list per line, "n mul t0 ... t(n-1)" (hex floats, n >= 0).  stdout, per list:
//   "cert V q units"      the certificate's verdict (1 certified), unit exponent and integer sum
//   "sums L P U"          the literal chain, a pairwise (tree) sum of the same terms and
//                         units * 2^q (L again without a certificate): with verdict 1 the three
//                         must be equal bits
//   "stats S Q M D T"     the list taken as the distances of n valid entries: sum, sq_sum, mean,
//                         stddev and threshold at multiplier mul
// (doubles as hex floats).
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I dialog_amd/csrc sor_model_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sor_model.hpp"

using namespace dlg;

static double tree_sum(const float* t, long n) {
  if (n == 0) return 0.0;
  if (n == 1) return (double)t[0];
  const long h = n / 2;
  return tree_sum(t + h, n - h) + tree_sum(t, h);
}

int main() {
  long n;
  double mul;
  while (std::scanf("%ld %la", &n, &mul) == 2) {
    if (n < 0) return 2;
    std::vector<float> t((size_t)n);
    for (long i = 0; i < n; ++i)
      if (std::scanf("%a", &t[(size_t)i]) != 1) return 2;
    int q = 0;
    uint64_t units = 0;
    const bool ok = sor_certify(t.data(), n, &q, &units);
    std::printf("cert %d %d %llu\n", ok ? 1 : 0, ok ? q : 0, ok ? (unsigned long long)units : 0ull);
    const double lit = sor_literal_sum(t.data(), n);
    std::printf("sums %a %a %a\n", lit, tree_sum(t.data(), n), ok ? sor_from_units(units, q) : lit);
    double sq = 0.0;
    for (long i = 0; i < n; ++i) sq = sor_chain(sq, sor_square(t[(size_t)i]));
    const SorThreshold th = sor_threshold(lit, sq, n, mul);
    std::printf("stats %a %a %a %a %a\n", lit, sq, th.mean, th.stddev, th.threshold);
  }
  return 0;
}
