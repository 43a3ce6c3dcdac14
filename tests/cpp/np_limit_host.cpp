// Host build of the NORMAL_PLANE prefilter limit (dialog_amd/csrc/np_limit_host.hpp, what
// make_plan takes for the prune margin) for the CPU test tests/test_np_limit.py: reads lines
// "w thr" (hex doubles, or nan / inf) and prints the bit pattern of np_lim_max(w, thr).
#include <cstdio>
#include <cstring>

#include "../../dialog_amd/csrc/np_limit_host.hpp"

int main() {
  double w, thr;
  while (std::scanf("%la %la", &w, &thr) == 2) {
    const float x = dlg::np_lim_max(w, thr);
    unsigned u;
    std::memcpy(&u, &x, 4);
    std::printf("%08x\n", u);
  }
  return 0;
}
