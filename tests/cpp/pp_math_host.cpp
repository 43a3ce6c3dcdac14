// pp_math_host.cpp -- dlg::segs_intersect (dialog_amd/csrc/pp_math.hpp: the reference's
// isBothLineSegsIntersect with two early outs in front of its square roots) against the oracle's
// literal statement of the same test (oracle/pcl_oracle.c, orc_segs_intersect), on the host.
//
// Built by tests/test_pp_math.py with ASan + UBSan as a program of its own; never loaded into
// Python.  usage: pp_math_host SAMPLES_PER_CELL SEED
//
// Every sample is an edge (a, b) and a ray origin c in one plane, built in double in a random
// plane basis and rounded to float; the edge record is plane_edges' (postprocess_host.cpp) and the
// ray is make_ray(c, dir), as k_pip_test builds them.  Cells = origin offset x edge length x
// class of d = nab . ncd.  Output, one line per cell:
//   cell OFFSET LENGTH D samples true false_in_band mismatches
// then `directed samples true 0 mismatches` for the directed tuples (degenerate edges, d exactly
// 0 and +-1, c on a / b / the edge, a == b == c, NaN and inf), up to 20 `bad ...` lines with the
// operands of mismatching tuples as hex floats, and `total samples true mismatches`.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "pp_math.hpp"

extern "C" int orc_segs_intersect(const float a[3], const float b[3], const float c[3],
                                  const float d[3]);

namespace {

using dlg::V3;

struct Tally {
  long n = 0, n_true = 0, n_false_band = 0, bad = 0;
};

int g_bad_printed = 0;

// one (edge, ray) pair through both statements; dir: the ray's direction as the kernel gets it
void check(V3 a, V3 b, V3 c, V3 dir, bool in_band, Tally* t) {
  // plane_edges' record
  const V3 nab = dlg::v3_normalized(dlg::v3_sub(b, a));
  const float dab = dlg::dist_p2p(a, b);
  const float a_l1 = (std::fabs(a.x) + std::fabs(a.y)) + std::fabs(a.z);
  // k_pip_test's ray
  const float c_l1 = (std::fabs(c.x) + std::fabs(c.y)) + std::fabs(c.z);
  const dlg::PipRay r = dlg::make_ray(c, dir);
  const bool got = dlg::segs_intersect(a, b, nab, dab, a_l1, c, c_l1, r);
  const float fa[3] = {a.x, a.y, a.z}, fb[3] = {b.x, b.y, b.z}, fc[3] = {c.x, c.y, c.z};
  const float fd[3] = {r.d.x, r.d.y, r.d.z};
  const bool want = orc_segs_intersect(fa, fb, fc, fd) != 0;
  ++t->n;
  t->n_true += want;
  t->n_false_band += !want && in_band;
  if (got != want) {
    ++t->bad;
    if (g_bad_printed++ < 20)
      std::printf("bad got %d want %d a %a %a %a b %a %a %a c %a %a %a dir %a %a %a\n", (int)got,
                  (int)want, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, dir.x, dir.y, dir.z);
  }
}

struct D3 {
  double x, y, z;
};
D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
D3 mul(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
D3 unit(D3 a) { return mul(1.0 / std::sqrt(dot(a, a)), a); }
V3 f32(D3 a) { return V3{(float)a.x, (float)a.y, (float)a.z}; }

const double kOffsets[] = {0, 10, 1e3, 1e4, 1e5, 1e6, 1e7};
const double kLengths[] = {1e-3, 0.05, 1, 30, 1e3, 1e4};
const double kD[] = {0.05, -0.05, 0.97, -0.97, 0.5, -0.5, 0.001, -0.001, 0.9999, -0.9999, 0.2, -0.2};

void sample_cell(std::mt19937_64& g, double offset, double len0, double d0, long n, Tally* t) {
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  for (long i = 0; i < n; ++i) {
    // a random plane basis (u, v) and an origin `offset` away from zero
    const D3 nrm = unit(D3{N(g), N(g), N(g)});
    D3 u = cross(nrm, std::fabs(nrm.x) < 0.6 ? D3{1, 0, 0} : D3{0, 1, 0});
    u = unit(u);
    const D3 v = cross(nrm, u);
    const D3 org = mul(offset, D3{2 * U(g) - 1, 2 * U(g) - 1, 2 * U(g) - 1});
    const double L = len0 * (0.5 + U(g));
    // edge direction at a random angle, ray direction at cos = d to it (either side)
    const double th = 6.283185307179586 * U(g);
    const D3 ea = add(mul(std::cos(th), u), mul(std::sin(th), v));
    const D3 eb = cross(nrm, ea);
    double d = d0 * (1.0 + 0.01 * (2 * U(g) - 1));
    d = std::fmin(1.0, std::fmax(-1.0, d));
    const double sd = std::sqrt(std::fmax(0.0, 1.0 - d * d)) * (U(g) < 0.5 ? 1.0 : -1.0);
    const D3 rd = add(mul(d, ea), mul(sd, eb));
    // where the ray's line meets the edge's line: 80 % around an end, 20 % inside
    const bool band = U(g) < 0.8;
    double s;
    if (band) {
      const double w = 2.0 * (0.0006 + 0.02 * L);
      s = (U(g) < 0.5 ? 0.0 : L) + w * (2 * U(g) - 1);
    } else {
      s = L * U(g);
    }
    const double back = (U(g) < 0.5 ? 3.0 * L : 50.0) * U(g);
    const D3 a = add(org, mul(len0 * (2 * U(g) - 1), ea));
    const D3 b = add(a, mul(L, ea));
    const D3 x = add(a, mul(s, ea));
    const D3 c = add(x, mul(-back, rd));
    check(f32(a), f32(b), f32(c), dlg::v3_normalized(f32(rd)), band, t);
  }
}

void directed(Tally* t) {
  const float inf = std::numeric_limits<float>::infinity();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const V3 axes[6] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
  std::vector<V3> dirs(axes, axes + 6);
  for (int k = 0; k < 16; ++k) {
    const float th = 0.3926990817f * (float)k + 0.01f;
    dirs.push_back(dlg::v3_normalized(V3{std::cos(th), std::sin(th), 0.0f}));
    dirs.push_back(dlg::v3_normalized(V3{0.0f, std::cos(th), std::sin(th)}));
  }
  const float steps[] = {0.0f, 1e-20f, 1e-16f, 1e-15f, 1e-7f, 1e-4f, 4.9e-4f, 5e-4f, 5.1e-4f,
                         9.9e-4f, 1e-3f, 1.1e-3f, 2e-3f, 0.25f, 0.5f, 1.0f, 1.5f, 3.0f};
  // edges of length 0, 1e-20, 1e-16 and around the 1e-15 threshold of the early outs, at the
  // origin (where such lengths are representable) and along every axis
  const float e15 = 1e-15f;
  const float lens[] = {0.0f, 1e-20f, 1e-16f, std::nextafter(e15, 0.0f), e15,
                        std::nextafter(e15, 1.0f), 2e-15f, 1e-10f};
  for (float len : lens)
    for (int ax = 0; ax < 6; ++ax) {
      const V3 a{0, 0, 0};
      const V3 b{len * axes[ax].x, len * axes[ax].y, len * axes[ax].z};
      for (const V3& dir : dirs)
        for (float st : steps)
          for (int bx = 0; bx < 6; ++bx) {
            // c back along the ray from a point `st` off a along axis bx
            for (float back : {0.0f, 1e-4f, 0.5f, 20.0f}) {
              const V3 c{st * axes[bx].x - back * dir.x, st * axes[bx].y - back * dir.y,
                         st * axes[bx].z - back * dir.z};
              check(a, b, c, dir, false, t);
            }
          }
    }
  // unit and long axis-aligned edges: d exactly 0 and exactly +-1; c exactly on a, on b, on the
  // edge, and around them
  for (float len : {1.0f, 2.0f, 4000.0f})
    for (int ax = 0; ax < 6; ++ax)
      for (float base : {0.0f, 2.0f, -4.0f, 1000.0f}) {
        const V3 a{base, base, base};
        const V3 b{a.x + len * axes[ax].x, a.y + len * axes[ax].y, a.z + len * axes[ax].z};
        for (const V3& dir : dirs)
          for (float along : {0.0f, 0.5f, 1.0f, -0.0004f, 1.0004f, -0.0006f, 1.0006f, -0.5f, 1.5f})
            for (float st : steps)
              for (float sgn : {1.0f, -1.0f}) {
                // a point of the edge's line, `st` back along the ray
                const float s = along * len;
                const V3 c{a.x + s * axes[ax].x - sgn * st * dir.x,
                           a.y + s * axes[ax].y - sgn * st * dir.y,
                           a.z + s * axes[ax].z - sgn * st * dir.z};
                check(a, b, c, dir, false, t);
              }
      }
  // a == b == c
  for (float base : {0.0f, 1.0f, -3.5f, 1e5f})
    for (const V3& dir : dirs) check(V3{base, base, base}, V3{base, base, base}, V3{base, base, base}, dir, false, t);
  // NaN and inf in each coordinate of a, b and c
  for (float bad : {nan, inf, -inf})
    for (int which = 0; which < 3; ++which)
      for (int k = 0; k < 3; ++k)
        for (const V3& dir : dirs) {
          float p[3][3] = {{0, 0, 0}, {1, 0.5f, 0}, {0.5f, -1.0f, 0}};
          p[which][k] = bad;
          check(V3{p[0][0], p[0][1], p[0][2]}, V3{p[1][0], p[1][1], p[1][2]},
                V3{p[2][0], p[2][1], p[2][2]}, dir, false, t);
        }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s SAMPLES_PER_CELL SEED\n", argv[0]);
    return 2;
  }
  const long per_cell = std::atol(argv[1]);
  std::mt19937_64 g((uint64_t)std::atoll(argv[2]));
  Tally all;
  for (double off : kOffsets)
    for (double len : kLengths)
      for (double d : kD) {
        Tally t;
        sample_cell(g, off, len, d, per_cell, &t);
        std::printf("cell %g %g %g %ld %ld %ld %ld\n", off, len, d, t.n, t.n_true, t.n_false_band,
                    t.bad);
        all.n += t.n; all.n_true += t.n_true; all.bad += t.bad;
      }
  Tally t;
  directed(&t);
  std::printf("directed %ld %ld 0 %ld\n", t.n, t.n_true, t.bad);
  all.n += t.n; all.n_true += t.n_true; all.bad += t.bad;
  std::printf("total %ld %ld %ld\n", all.n, all.n_true, all.bad);
  return 0;
}
