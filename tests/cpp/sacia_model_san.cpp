// sacia_model_san.cpp -- dialog_amd/csrc/sacia_model.hpp as a stand-alone program (built without
// HIP, under -fsanitize=address,undefined by tests/test_sac_ia.py): one whole alignment on the host,
// every draw, descriptor distance, estimate, term and adoption through the header, the searches by
// brute force.
//   sacia_model_san <in> <out>
// in:  int32 n_src, n_tgt, max_iterations, nr_samples, k, rng, seed, has_guess; float
//      min_sample_distance; double max_correspondence_distance; then float32 src xyz, src rows
//      (33 a point), tgt xyz, tgt rows, guess (16)
// out: int32 n_records, converged, best_iteration; float final[16]; uint64 hi, lo of the lowest
//      error; double error; then the records (dlg_sac_ia_hypothesis)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "dialog_ransac.h"
#include "sacia_model.hpp"

using namespace dlg;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[8];
  float msd;
  double mcd;
  if (!rd(f, hd, 8) || !rd(f, &msd, 1) || !rd(f, &mcd, 1)) return 2;
  const int n_src = hd[0], n_tgt = hd[1], max_it = hd[2], nr = hd[3], k = hd[4];
  std::vector<float> src((size_t)n_src * 3), fs((size_t)n_src * kSaciaDim), tgt((size_t)n_tgt * 3),
      ft((size_t)n_tgt * kSaciaDim);
  float fin[16];
  if (!rd(f, src.data(), src.size()) || !rd(f, fs.data(), fs.size()) ||
      !rd(f, tgt.data(), tgt.size()) || !rd(f, ft.data(), ft.size()) || !rd(f, fin, 16))
    return 2;
  std::fclose(f);
  if (!hd[7])
    for (int j = 0; j < 16; ++j) fin[j] = (j % 5 == 0) ? 1.0f : 0.0f;
  const float thr = sacia_threshold(mcd);
  std::vector<int> valid_t;
  for (int r = 0; r < n_tgt; ++r)
    if (sacia_finite(tgt[3 * (size_t)r]) && sacia_finite(tgt[3 * (size_t)r + 1]) &&
        sacia_finite(tgt[3 * (size_t)r + 2]) && sacia_row_finite(&ft[(size_t)r * kSaciaDim]))
      valid_t.push_back(r);
  if ((int)valid_t.size() < k) return 3;
  const bool score_guess = !sacia_guess_is_identity(fin);
  const int n_rec = score_guess ? std::max(max_it, 1) : max_it;
  std::vector<dlg_sac_ia_hypothesis> rec((size_t)n_rec);
  SaciaRng rng;
  rng.seed(hd[5], (uint32_t)hd[6]);
  SaciaBest best;
  for (int it = 0; it < n_rec; ++it) {
    dlg_sac_ia_hypothesis& r = rec[(size_t)it];
    std::memset(&r, 0, sizeof(r));
    for (int j = 0; j < kSaciaMaxSamples; ++j) r.sample[j] = r.match[j] = r.rank[j] = -1;
    r.valid = 1;
    if (it == 0 && score_guess) {
      std::memcpy(r.T, fin, 64);
    } else {
      sacia_select(rng, src.data(), 3, n_src, nr, msd, r.sample, &r.draws, &r.relaxations);
      for (int j = 0; j < nr; ++j) {
        r.rank[j] = rng.index(k);
        ++r.draws;
        const float* p = &src[3 * (size_t)r.sample[j]];
        if (!(sacia_finite(p[0]) && sacia_finite(p[1]) && sacia_finite(p[2]) &&
              sacia_row_finite(&fs[(size_t)r.sample[j] * kSaciaDim])))
          r.valid = 0;
      }
      if (!r.valid) continue;
      float w3[kSaciaMaxSamples][3], t3[kSaciaMaxSamples][3];
      for (int j = 0; j < nr; ++j) {
        std::vector<std::pair<float, int>> d;
        d.reserve(valid_t.size());
        for (int row : valid_t)
          d.emplace_back(sacia_feature_d2(&fs[(size_t)r.sample[j] * kSaciaDim],
                                          &ft[(size_t)row * kSaciaDim]), row);
        std::partial_sort(d.begin(), d.begin() + k, d.end());  // (d, index) order
        r.match[j] = d[(size_t)r.rank[j]].second;
        std::memcpy(w3[j], &src[3 * (size_t)r.sample[j]], 12);
        std::memcpy(t3[j], &tgt[3 * (size_t)r.match[j]], 12);
      }
      sacia_estimate(w3, t3, nr, r.T);
    }
    unsigned __int128 E = 0;
    for (int i = 0; i < n_src; ++i) {
      const float* p = &src[3 * (size_t)i];
      float q[3];
      icp_xf(r.T, p[0], p[1], p[2], q[0], q[1], q[2]);
      if (!(sacia_finite(p[0]) && sacia_finite(p[1]) && sacia_finite(p[2]) && sacia_finite(q[0]) &&
            sacia_finite(q[1]) && sacia_finite(q[2])))
        continue;
      float e = INFINITY;
      for (int row : valid_t) {
        const float* t = &tgt[3 * (size_t)row];
        const float d2 = icp_d2(q[0], q[1], q[2], t[0], t[1], t[2]);
        if (d2 < e) e = d2;
      }
      const float term = sacia_term(e, thr);
      E += sacia_quantise(term);
      r.n_far += term == 1.0f;
      ++r.n_used;
    }
    // (the two sums a device wave would add: the low 24 bits and the rest)
    uint64_t hi, lo;
    sacia_error_words((uint64_t)(E & 0xFFFFFF), (uint64_t)(E >> 24), &hi, &lo);
    r.err_hi = hi;
    r.err_lo = lo;
    if (best.offer(it, hi, lo, r.draws != 0)) std::memcpy(fin, r.T, 64);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t head[3] = {n_rec, best.best_iteration >= 0, best.best_iteration};
  const double err = best.scored ? sacia_error_double(best.hi, best.lo) : 0.0;
  std::fwrite(head, 4, 3, o);
  std::fwrite(fin, 4, 16, o);
  std::fwrite(&best.hi, 8, 1, o);
  std::fwrite(&best.lo, 8, 1, o);
  std::fwrite(&err, 8, 1, o);
  if (n_rec > 0) std::fwrite(rec.data(), sizeof(dlg_sac_ia_hypothesis), (size_t)n_rec, o);
  std::fclose(o);
  return 0;
}
