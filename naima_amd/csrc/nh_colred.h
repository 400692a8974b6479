// nh_colred.h -- the tiling of the column reductions over a row-major device matrix x[M][ld]
// (nh_posterior.hip, nh_infocrit.hip): workgroups of 256 threads take (column tile, row chunk),
// threads are [256/cw row lanes][cw columns], a workgroup reduces its row lanes through an LDS
// tree and the per-chunk partials are summed in chunk order.  Chunks are a function of the shapes
// alone, so every floating-point sum has a fixed order.
#pragma once
#include "nh_common.h"

#include <algorithm>

namespace {

constexpr int PO_THREADS = 256;
constexpr int PO_TARGET_WG = 2048;     // workgroups a launch aims for (a few per CU)
constexpr int PO_MIN_ROWS = 1024;      // rows a chunk holds at least

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

__device__ __forceinline__ bool po_finite(double v) { return fabs(v) < INFINITY; }  // (NaN: false)

// the row chunks of a launch with `ntile` workgroups per chunk: rows per chunk (a multiple of
// `mult`) and their number, a function of the shapes only
inline void po_chunks(long long M, long long ntile, long long mult, long long* rows, long long* nch) {
  long long want = std::max<long long>(1, PO_TARGET_WG / std::max<long long>(1, ntile));
  long long n = std::min(want, cdiv(M, PO_MIN_ROWS));
  *rows = cdiv(cdiv(M, n), mult) * mult;
  *nch = cdiv(M, *rows);
}

// threads are [R = 256/cw row lanes][cw columns]; v[tid] += v[tid + s*cw] down the row lanes
template <typename T, typename F>
__device__ __forceinline__ void po_tree(T* v, int tid, int ty, int cw, F op) {
  for (int s = (PO_THREADS / cw) >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if (ty < s) v[tid] = op(v[tid], v[tid + s * cw]);
  }
  __syncthreads();
}

inline int po_pow2_at_least(int n, int cap) {
  int p = 1;
  while (p < n && p < cap) p <<= 1;
  return p;
}

}  // namespace
