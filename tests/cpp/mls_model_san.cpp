// mls_model_san.cpp -- dialog_amd/csrc/mls_model.hpp on the host, for the address and
// undefined-behaviour sanitizers (tests/test_mls.py builds and runs it; no GPU, no HIP).
//
// stdin, one query per line:  order polynomial_fit compute_normals sqr_gauss m qx qy qz, then the
// m neighbours' x y z (the query included), every number after the three flags in C hex-float
// notation.  stdout per query:  code x y z nx ny nz curvature (hex floats; code 3: too few
// neighbours, the values are zero).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mls_model.hpp"

namespace {

struct VecSrc {
  const std::vector<float>* p;
  int size() const { return (int)(p->size() / 3); }
  void get(int i, float o[3]) const {
    for (int k = 0; k < 3; ++k) o[k] = (*p)[(size_t)3 * i + k];
  }
};

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int order = 0, fit = 0, normals = 0;
    long m = 0;
    std::string tok;
    in >> order >> fit >> normals >> tok;
    const double sqr_gauss = std::strtod(tok.c_str(), nullptr);
    in >> m;
    float q[3];
    for (int k = 0; k < 3; ++k) {
      in >> tok;
      q[k] = std::strtof(tok.c_str(), nullptr);
    }
    std::vector<float> pts;
    pts.reserve((size_t)3 * m);
    for (long i = 0; i < 3 * m; ++i) {
      if (!(in >> tok)) return 2;
      pts.push_back(std::strtof(tok.c_str(), nullptr));
    }
    const VecSrc src{&pts};
    dlg::MlsRow r{};
    if (order == 1) dlg::mls_query<1>(src, q, fit != 0, normals != 0, sqr_gauss, &r);
    else if (order == 2) dlg::mls_query<2>(src, q, fit != 0, normals != 0, sqr_gauss, &r);
    else if (order == 3) dlg::mls_query<3>(src, q, fit != 0, normals != 0, sqr_gauss, &r);
    else return 3;
    std::printf("%d %a %a %a %a %a %a %a\n", r.code, (double)r.xyz[0], (double)r.xyz[1],
                (double)r.xyz[2], (double)r.nrm[0], (double)r.nrm[1], (double)r.nrm[2],
                (double)r.nrm[3]);
  }
  return 0;
}
