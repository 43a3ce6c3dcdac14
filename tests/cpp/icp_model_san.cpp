// icp_model_san.cpp -- the host side of dialog_amd/csrc/icp_model.hpp as a stand-alone program
// (built without HIP, under -fsanitize=address,undefined by tests/test_icp.py).  Reads from stdin:
//   C <max_iterations> <transformation_epsilon> <euclidean_fitness_epsilon>   a new case
//   I <m> <e> <e2> <group> <reverse>     one iteration: m lines of 7 hex words follow (the float
//                                        bits of w.xyz, t.xyz, d2); the pairs are accumulated in
//                                        groups of <group> entries per flush, from the last to the
//                                        first when <reverse> is 1
// and prints per iteration the exact integers (S, T, P, D as 192-bit two's complement hex), the 16
// words of T, the bits of mse and the criteria's state.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_model.hpp"

using namespace dlg;

static void print_big(const Big& b) {
  std::printf(" ");
  for (int k = 5; k >= 0; --k) std::printf("%08x", b.w[k]);
}

int main() {
  char tag[8];
  IcpCriteria crit;
  int iterations = 0;
  while (std::scanf("%7s", tag) == 1) {
    if (tag[0] == 'C') {
      double teps, feps;
      int mi;
      if (std::scanf("%d %lf %lf", &mi, &teps, &feps) != 3) return 2;
      crit = IcpCriteria();
      crit.max_iterations = mi;
      crit.rot_thr = 1.0 - teps;
      crit.trans_thr = teps;
      crit.rel_mse = feps;
      iterations = 0;
      continue;
    }
    int m, e, e2, group, reverse;
    if (std::scanf("%d %d %d %d %d", &m, &e, &e2, &group, &reverse) != 5) return 2;
    std::vector<float> rows((size_t)m * 7);
    for (size_t i = 0; i < rows.size(); ++i) {
      uint32_t u;
      if (std::scanf("%x", &u) != 1) return 2;
      std::memcpy(&rows[i], &u, 4);
    }
    if (group < 1 || group > kIcpFlush) return 2;
    int64_t dig[kIcpDigits] = {};
    IcpAcc acc;
    icp_acc_zero(acc);
    const double sc = pow2d(kFastBits - e), sc2 = pow2d(kFastBits - e2);
    for (int k = 0; k < m; ++k) {
      const float* r = &rows[(size_t)(reverse ? m - 1 - k : k) * 7];
      const double qw[3] = {icp_q(r[0], sc), icp_q(r[1], sc), icp_q(r[2], sc)};
      const double qt[3] = {icp_q(r[3], sc), icp_q(r[4], sc), icp_q(r[5], sc)};
      icp_acc_point(acc, qw, qt, icp_q(r[6], sc2));
      if (acc.n == (double)group) icp_acc_flush(dig, acc);
    }
    icp_acc_flush(dig, acc);
    std::printf("ints %" PRId64, dig[0]);
    for (int a = 0; a < 3; ++a) print_big(big_lin(dig + 1 + 2 * a));
    for (int a = 0; a < 3; ++a) print_big(big_lin(dig + 7 + 2 * a));
    for (int k = 0; k < 9; ++k) print_big(big_prod(dig + 13 + 4 * k));
    print_big(big_lin(dig + 49));
    std::printf("\n");
    const IcpMoments mo = icp_moments(dig);
    float T[16];
    double mse;
    icp_solve(mo, e, e2, T, &mse);
    std::printf("T");
    for (int k = 0; k < 16; ++k) {
      uint32_t u;
      std::memcpy(&u, &T[k], 4);
      std::printf(" %08x", u);
    }
    uint64_t mb;
    std::memcpy(&mb, &mse, 8);
    ++iterations;
    std::printf("\nmse %016" PRIx64 "\nstate %d\n", mb, icp_criteria(crit, iterations, T, mse));
  }
  return 0;
}
