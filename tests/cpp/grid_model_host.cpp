// grid_model_host.cpp -- dialog_amd/csrc/grid_model.hpp (make_grid, cell_of and the k-NN kernels'
// distance bound) as a stand-alone host program, for tests/test_grid_model.py.  Built with the
// address and undefined-behaviour sanitizers like the other tests/cpp/*_san.cpp programs:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I dialog_amd/csrc
//       tests/cpp/grid_model_host.cpp
//
// stdin: one request per line,
//   lo0 lo1 lo2 hi0 hi1 hi2 any cell n_adj n_knn seed     (floats and cell as C hex floats)
// stdout per request: one text line
//   g0 g1 g2 ncells key_bits lo0 lo1 lo2 cell inv_cell slack
// then a uint32 record count (n_adj + n_knn; 0 when no axis spans 3 cells) and that many binary
// records of 14 words:
//   float q[3], p[3]; int32 cq[3], cp[3]; float md; int32 kind
// The map is used only to aim the samples; the caller judges them with its own arithmetic.
//   kind 0 (adjacency): q is one of the last floats of a random cell on a random wide axis, p is
//     fl(q + u * cell) with u in [0.998, 1] on that axis (the same point on the others); md = 0.
//   kind 1 (k-NN bound): q anywhere in a random cell, p in a neighbouring cell (per axis: the same
//     cell, or one of the floats nearest the shared face on the other side of it); md is the bound
//     the kernels compute for p's cell.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grid_model.hpp"

namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double uni() { return (double)(next() >> 11) * 0x1p-53; }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Rec {
  float q[3], p[3];
  int32_t cq[3], cp[3];
  float md;
  int32_t kind;
};
static_assert(sizeof(Rec) == 56, "14 words");

const dlg::GridDesc* GG;
dlg::BBox BB;

int cell(float v, int k) { return dlg::grid::cell_of(v, GG->lo[k], GG->inv_cell, GG->g[k]); }
float clampf(float v, int k) { return v < BB.lo[k] ? BB.lo[k] : v > BB.hi[k] ? BB.hi[k] : v; }

// a float of cell c on axis k near the cell's upper (up) or lower face: the map steers, by single
// floats, from the face's estimate; then `back` floats further into the cell while it stays there
float near_face(int k, int c, bool up, int back) {
  const double w = 1.0 / (double)GG->inv_cell;
  float v = clampf((float)((double)GG->lo[k] + (double)(c + (up ? 1 : 0)) * w), k);
  const float out = up ? INFINITY : -INFINITY;
  for (int it = 0; it < 64 && (up ? cell(v, k) <= c : cell(v, k) >= c); ++it) {
    const float n = clampf(std::nextafterf(v, out), k);
    if (n == v) break;
    v = n;
  }
  for (int it = 0; it < 4096 && (up ? cell(v, k) > c : cell(v, k) < c); ++it) v = std::nextafterf(v, -out);
  for (int it = 0; it < back; ++it) {
    const float n = std::nextafterf(v, -out);
    if (cell(n, k) != c) break;
    v = n;
  }
  return v;
}

int TOP[3];  // the cell of the box's upper corner (the shrink of inv_cell leaves the last cells empty)

// a random cell of axis k: half of them in the tenth of the axis farthest from lo
int random_cell(Rng& r, int k, int lo_c, int hi_c) {
  const int g = TOP[k] + 1;
  int a = lo_c, b = g - 1 - hi_c;  // c in [a, b]
  if (b < a) return -1;
  if (r.below(2)) a = b - (b - a) / 10;
  return a + r.below(b - a + 1);
}

float inside(Rng& r, int k, int c) {
  const double w = 1.0 / (double)GG->inv_cell;
  const float v = clampf((float)((double)GG->lo[k] + ((double)c + r.uni()) * w), k);
  return v;
}

}  // namespace

int main() {
  char line[1024];
  while (std::fgets(line, sizeof line, stdin)) {
    double v[8];
    int any, n_adj, n_knn;
    unsigned long long seed;
    if (std::sscanf(line, "%la %la %la %la %la %la %d %la %d %d %llu", &v[0], &v[1], &v[2], &v[3],
                    &v[4], &v[5], &any, &v[6], &n_adj, &n_knn, &seed) != 11) {
      std::fprintf(stderr, "bad request: %s", line);
      return 2;
    }
    for (int k = 0; k < 3; ++k) {
      BB.lo[k] = (float)v[k];
      BB.hi[k] = (float)v[3 + k];
    }
    BB.any = any != 0;
    const double cell_arg = v[6];
    const dlg::GridDesc G = dlg::make_grid(BB, cell_arg);
    GG = &G;
    std::printf("%d %d %d %u %d %a %a %a %a %a %a\n", G.g[0], G.g[1], G.g[2], G.ncells, G.key_bits,
                (double)G.lo[0], (double)G.lo[1], (double)G.lo[2], (double)G.cell,
                (double)G.inv_cell, (double)G.slack);
    Rng r{seed};
    std::vector<Rec> out;
    out.reserve((size_t)n_adj + (size_t)n_knn);
    int wide[3], nw = 0;
    for (int k = 0; k < 3; ++k) {
      TOP[k] = cell(BB.hi[k], k);
      if (TOP[k] >= 2) wide[nw++] = k;
    }
    for (int i = 0; i < n_adj + n_knn; ++i) {
      if (nw == 0) break;
      Rec R;
      std::memset(&R, 0, sizeof R);
      int c[3];
      for (int k = 0; k < 3; ++k) c[k] = TOP[k] >= 2 ? random_cell(r, k, 1, 1) : 0;
      if (i < n_adj) {
        R.kind = 0;
        const int a = wide[r.below(nw)];
        const bool up = r.below(2) != 0;  // the partner lies above (q at the upper face) or below
        for (int k = 0; k < 3; ++k) R.q[k] = R.p[k] = k == a ? 0.0f : inside(r, k, c[k]);
        R.q[a] = near_face(a, c[a], up, r.below(3));
        const double u = 0.998 + 0.002 * r.uni();
        R.p[a] = clampf((float)((double)R.q[a] + (up ? u : -u) * cell_arg), a);
      } else {
        R.kind = 1;
        int d[3];
        for (int k = 0; k < 3; ++k) d[k] = TOP[k] >= 2 ? r.below(3) - 1 : 0;
        // the query: anywhere in its cell, or (a quarter of them) at the face away from the
        // neighbour, where the bound is largest
        for (int k = 0; k < 3; ++k) {
          R.q[k] = inside(r, k, c[k]);
          if (d[k] != 0 && r.below(4) == 0) R.q[k] = near_face(k, c[k], d[k] < 0, r.below(3));
          R.p[k] = d[k] == 0 ? inside(r, k, c[k]) : near_face(k, c[k] + d[k], d[k] < 0, r.below(3));
        }
        int cq[3];
        float f[3];
        for (int k = 0; k < 3; ++k) {
          cq[k] = cell(R.q[k], k);
          f[k] = dlg::grid::knn_frac(R.q[k], G.lo[k], G.inv_cell, cq[k]);
        }
        const float w = dlg::grid::knn_width(G.inv_cell);
        float e[3];
        for (int k = 0; k < 3; ++k) {
          const int dd = cell(R.p[k], k) - cq[k];  // the side the kernel would visit p's cell on
          e[k] = dlg::grid::knn_side(f[k], dd < 0 ? -1 : dd > 0 ? 1 : 0, w, G.slack);
        }
        R.md = dlg::grid::knn_bound(e[0], e[1], e[2]);
      }
      for (int k = 0; k < 3; ++k) {
        R.cq[k] = cell(R.q[k], k);
        R.cp[k] = cell(R.p[k], k);
      }
      out.push_back(R);
    }
    const uint32_t cnt = (uint32_t)out.size();
    std::fwrite(&cnt, 4, 1, stdout);
    if (cnt) std::fwrite(out.data(), sizeof(Rec), cnt, stdout);
  }
  return 0;
}
