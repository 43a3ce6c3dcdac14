// sor.hpp -- device passes of the statistical outlier filter (sor.hip), driven by sor_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "normals.hpp"
#include "sor_model.hpp"

namespace dlg {

// rank[fin_pos[t]] = t for the nf finite points (rank is preset to -1 by the caller)
void launch_sor_rank(const int32_t* fin_pos, int nf, int32_t* rank, hipStream_t s);
// need[rank[idx[e]]] = 1 for every list entry whose point is finite (need preset to 0)
void launch_sor_need(const int32_t* idx, int n_list, const int32_t* rank, uint8_t* need,
                     hipStream_t s);

// One level of the (mean_k + 1)-nearest-neighbour search over the hierarchy L of the finite points,
// one wave per query: queries = the sorted positions qpos[0..nq) of level `level` (nullptr: all of
// them), skipped where need (nullable, by point) is 0.  A query with at least K = mean_k + 1
// candidates inside the level's guaranteed radius (the top level: always) writes
// dist_pt[point] = (float)(sum of sqrtf(d2[k]), k = 1..mean_k, as a double chain / mean_k); any
// other sets defer[tnext * defer_stride + point].  The chain runs as a wave reduction where
// sor_model.hpp's certificate holds, else (or always with force_literal) as the literal loop,
// counted in *n_literal.
void launch_sor_knn(const KnnLevels& L, int level, const int32_t* qpos, int nq, const uint8_t* need,
                    int mean_k, int force_literal, float* dist_pt, uint8_t* defer,
                    int64_t defer_stride, int tnext, unsigned long long* n_literal, hipStream_t s);

// dist[e] = dist_pt[rank[p]] for list entry e = point p (idx null: e), 0.0f where p is not finite
void launch_sor_entries(const int32_t* idx, int n_list, const int32_t* rank, const float* dist_pt,
                        float* dist, hipStream_t s);

// the statistics reduction over dist[0..n_list): acc[] (kSorAccWords words, zeroed here)
enum {
  kSorValid = 0,   // valid entries
  kSorQd = 1,      // min lowest-bit exponent of the distances + kSorQBias
  kSorQs = 2,      // ... of their float squares
  kSorFail = 3,    // != 0: a term is not finite or too large for its unit
  kSorDLo = 4,     // sum of (distance / unit) & 0xffffffff
  kSorDHi = 5,     // sum of (distance / unit) >> 32
  kSorSLo = 6,     // the same of the squares
  kSorSHi = 7,
  kSorLiteral = 8,  // (k_sor_knn's literal queries)
  kSorAccWords = 12
};
constexpr int kSorQBias = 1024;
void launch_sor_stats(const int32_t* idx, int n_list, const int32_t* rank, const float* dist,
                      unsigned long long* acc, hipStream_t s);

// keep[e] / rem[e] by sor_removed(dist[e], threshold, negative)
void launch_sor_classify(const float* dist, int n_list, double threshold, int negative,
                         uint8_t* keep, uint8_t* rem, hipStream_t s);
// out[j] = the index value of list position sel[j], j < *count (at most n_list)
void launch_sor_emit(const int32_t* sel, const uint32_t* count, int n_list, const int32_t* idx,
                     int32_t* out, hipStream_t s);
// gid[j] = id_base + j
void launch_sor_ids(int32_t* gid, int n, int32_t id_base, hipStream_t s);

}  // namespace dlg
