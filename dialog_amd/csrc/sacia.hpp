// sacia.hpp -- device passes of the SAC-IA initial alignment (sacia.hip), driven by sacia_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "icp.hpp"  // IcpXf, KnnLevels
#include "sacia_model.hpp"

namespace dlg {

constexpr int kSaciaSlab = 8192;  // rows of the descriptor table one wave scans

// One hypothesis's sums: lo / hi = the sums of the low 24 bits and of the rest of the per-wave
// partial sums of trunc(term 2^48) (sacia_error_words joins them), cnt = n_used 2^32 + n_far.
struct SaciaAcc {
  unsigned long long lo, hi, cnt;
};

// Device state of the scorer: the deferred pairs counted per level (zeroed before each batch) and
// the highest level a pair of the call reached.
struct SaciaState {
  uint32_t qn[kMaxLevels + 1];
  uint32_t levels;
};

// flags[r] = 1 when the descriptor row r (row_stride_f floats apart; null: not looked at) and the
// point r (px null: not looked at) are finite; *n_valid += their number
void launch_sacia_row_flags(const float* rows, int64_t row_stride_f, const float* px,
                            const float* py, const float* pz, int n, uint8_t* flags,
                            uint32_t* n_valid, hipStream_t s);

inline int sacia_slabs(int n_rows) { return (n_rows + kSaciaSlab - 1) / kSaciaSlab; }

// The k nearest flagged rows of every query (nq packed rows of 33 floats), in (d, index) order,
// d = sacia_feature_d2(query, row): one wave per (64 queries, slab of kSaciaSlab rows) keeps each
// lane's sorted list in registers and writes it to part_d / part_i (nq x slabs x k); the merge then
// writes d_out / i_out (nq x k).  A query with a non-finite value, and the ranks beyond the number
// of flagged rows, get index -1 and distance 0.  All pointers are device memory.
void launch_sacia_knn(const float* queries, int nq, const float* rows, int64_t row_stride_f,
                      int n_rows, const uint8_t* flags, int k, float* part_d, int32_t* part_i,
                      float* d_out, int32_t* i_out, hipStream_t s);

// computeErrorMetric of nb transformations at once.  Level 0: a thread takes a source point, moves
// it through each transformation (wave-uniform operands) and searches its 27 cells of the target
// hierarchy's level 0 as k_icp_level does; a pair settles when a target point lies inside the
// level's guaranteed radius, or (the `beyond` rule) when that radius squared already exceeds thr
// and nothing lies inside -- the term is then 1.0f.  Any other pair is appended to qout as
// h 2^32 + i and searched at the next level by launch_sacia_score_level, with no read-back in
// between.  Per hypothesis the quantised terms are reduced over the wave and added to acc[h] with
// one atomic per wave and word (a wave of the coarser levels that holds several hypotheses adds lane
// by lane).  thr = +inf: a pair whose squared distances cannot overflow is a
// zero term without a search.  A source point that is not finite before or after the
// transformation adds nothing.  max_blocks: as in icp.hpp.
void launch_sacia_score0(const KnnLevels& L, const float* sx, const float* sy, const float* sz, int n,
                         const IcpXf* xfs, int nb, float thr, float tmax, unsigned long long* qout,
                         SaciaState* st, SaciaAcc* acc, int num_cus, int max_blocks, hipStream_t s);
// level l >= 1 over the st->qn[l] pairs of qin (at most cap)
void launch_sacia_score_level(const KnnLevels& L, int l, const float* sx, const float* sy,
                              const float* sz, const IcpXf* xfs, float thr,
                              const unsigned long long* qin, unsigned long long* qout, uint32_t cap,
                              SaciaState* st, SaciaAcc* acc, int num_cus, int max_blocks,
                              hipStream_t s);

}  // namespace dlg
