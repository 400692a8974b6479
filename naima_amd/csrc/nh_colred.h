// nh_colred.h -- the column reductions over a row-major device matrix x[M][ld] with ncol <= ld
// columns in use (nh_posterior.hip, nh_infocrit.hip, nh_predictive.hip, nh_reweight.hip): the one
// statement of their tiling and of the order of their sums.
//
// A launch of colred_pass has workgroups of 256 threads on a grid (column tile, row chunk).  The
// threads are [R = 256/cw row lanes][cw columns], cw the power of two >= ncol, 64 at most; lane
// (ty, tx) of chunk k walks the rows k*rows + ty, + R, + 2 R ... of column tile*cw + tx and
// accumulates them serially, in increasing row order.  The row lanes are then merged through an
// LDS tree that halves them (lane ty takes lane ty + s for s = R/2, R/4 ... 1), one field of the
// accumulator at a time through one array, each with its own merge (+, fmin or fmax), and row lane
// 0 stores the chunk's partial of field i at out.d[(k*dstride + i*dstep)*ncol + c] (a count at
// out.n[(k*NN + i)*ncol + c]).  colred_fold then merges the partials of a column serially in
// chunk order, from the field's identity.  cw, the chunk length and the number of chunks
// (colred_plan) are functions of (M, ncol) alone, so every floating-point sum has an order fixed
// by the shapes alone and repeated calls give bit-identical results.
//
// What a row contributes is the op's: an aggregate of pointers and scalars (colred_launch<Op> takes
// its members in order) with
//   using F = colred_fields<NN, merges...>;    NN counts (long long, merged by +) and one double
//                                              per merge: '+', '<' (fmin) or '>' (fmax)
//   template <class W> __device__ void column(int c, W walk, F::acc& a) const;
// column() loads what it needs of column c, calls walk(f) -- once -- with f(t) the step of row t
// on accumulators of its own, started at the fields' identities, and ends with a = {{doubles},
// {counts}}; without a call of walk, a stays the identity.  f may have side effects (stores to
// row t, an append to a list).  Two counters are each updated by 0 or 1 in every row, not on
// exclusive branches: f is optimised on its own before it is inlined, where its accumulators are
// still behind references, and `if (p) ++m; else if (q) ++n;` becomes one update through a selected
// address there -- the counters then live in scratch memory.  Nothing but the build shows that:
// after adding an op, read its instance's ScratchSize in -Rpass-analysis=kernel-resource-usage (it
// must be 0), and add its name to the KERNELS of the module's host test, whose
// test_new_kernels_hold_no_private_memory reads the same figure from the built library.
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

// threads are [R = 256/cw row lanes][cw columns]; v[tid] = op(v[tid], v[tid + s*cw]) down the row lanes
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

// ---------------------------------------------------------------- the plan
struct colred_grid {
  long long M;
  int ncol, cw;
  long long ntile, rows, nch;
  bool ok;  // the grid is within the launch limits
  unsigned col_blocks() const { return (unsigned)cdiv(ncol, PO_THREADS); }  // one thread per column
};

inline colred_grid colred_plan(long long M, int ncol) {
  colred_grid g;
  g.M = M;
  g.ncol = ncol;
  g.cw = po_pow2_at_least(ncol, 64);
  g.ntile = cdiv(ncol, g.cw);
  po_chunks(M, g.ntile, PO_THREADS / g.cw, &g.rows, &g.nch);
  g.ok = g.nch <= 65535 && g.ntile < (1ll << 31);
  return g;
}

#define NH_REQUIRE_PLAN(g) NH_REQUIRE((g).ok, "too many columns")

// a matrix of M rows; with int_rows, their indices must fit an int (the tail lists and the sort
// store them so; the moments, the histograms and the KDE index rows in 64 bits throughout)
constexpr bool NH_ROWS_INT = true, NH_ROWS_ANY = false;
#define NH_REQUIRE_MATRIX(M, ncol, ld, int_rows)                   \
  NH_REQUIRE(M > 0, "M == 0: no samples");                         \
  NH_REQUIRE(!(int_rows) || M < (1ll << 31), "M >= 2^31 rows");    \
  NH_REQUIRE(ncol > 0, "ncol must be positive");                   \
  NH_REQUIRE(ld >= ncol, "ncol > ld")

// ---------------------------------------------------------------- fields and partials
template <int NN_, char... MERGE>
struct colred_fields {
  static constexpr int ND = sizeof...(MERGE), NN = NN_;
  struct acc {
    double d[ND];
    long long n[NN ? NN : 1];
  };
  __device__ static __forceinline__ double identity(int i) {
    constexpr char m[] = {MERGE...};
    return m[i] == '+' ? 0.0 : (m[i] == '<' ? INFINITY : -INFINITY);
  }
  __device__ static __forceinline__ double merge(int i, double a, double b) {
    constexpr char m[] = {MERGE...};
    return m[i] == '+' ? a + b : (m[i] == '<' ? fmin(a, b) : fmax(a, b));
  }
  __device__ static __forceinline__ acc identity() {
    acc a;
#pragma unroll
    for (int i = 0; i < ND; ++i) a.d[i] = identity(i);
#pragma unroll
    for (int i = 0; i < NN; ++i) a.n[i] = 0;
    return a;
  }
};

// where the partials of a pass lie: field i of chunk k at d[(k*dstride + i*dstep)*ncol + c],
// count i at n[(k*NN + i)*ncol + c]
struct colred_out {
  double* d;
  long long* n;
  int dstride, dstep;
};

// the fields side by side: d [nch][ND][ncol], n [nch][NN][ncol]
template <class Op>
inline colred_out colred_dense(double* d, long long* n = nullptr) {
  colred_out o = {d, n, Op::F::ND, 1};
  return o;
}

// ---------------------------------------------------------------- the chunk pass
// the rows of one lane: f(t) in increasing t
struct colred_rows {
  long long first, end;
  int step;
  template <class Fn>
  __device__ __forceinline__ void operator()(Fn f) const {
    for (long long t = first; t < end; t += step) f(t);
  }
};

// (Four waves per SIMD at least: the 128 VGPRs of the widest row step, k_pit_sum's erf and erfc.
// Every argument is a scalar or a pointer, the op arriving as its members: the compiler preloads
// kernel arguments into SGPRs only up to the first struct.)
template <class Op, class... A>
__global__ __launch_bounds__(PO_THREADS, 4) void colred_pass(long long M, int ncol, int cw,
                                                             long long rows,
                                                             double* __restrict__ od,
                                                             long long* __restrict__ on, int dstride,
                                                             int dstep, A... members) {
  using F = typename Op::F;
  __shared__ double r[PO_THREADS];
  const Op op = {members...};
  const int tid = threadIdx.x, tx = tid % cw, ty = tid / cw, R = PO_THREADS / cw;
  const int c = blockIdx.x * cw + tx;
  const long long k = blockIdx.y;
  const long long t0 = k * rows, t1 = min(M, t0 + rows);
  typename F::acc a = F::identity();
  if (c < ncol) op.column(c, colred_rows{t0 + ty, t1, R}, a);
#pragma unroll
  for (int i = 0; i < F::ND; ++i) {
    r[tid] = a.d[i];
    po_tree(r, tid, ty, cw, [i](double p, double q) { return F::merge(i, p, q); });
    if (ty == 0 && c < ncol) od[(k * dstride + i * dstep) * ncol + c] = r[tid];
  }
#pragma unroll
  for (int i = 0; i < F::NN; ++i) {  // (a count travels through the array as its bits)
    r[tid] = __longlong_as_double(a.n[i]);
    po_tree(r, tid, ty, cw, [](double p, double q) {
      return __longlong_as_double(__double_as_longlong(p) + __double_as_longlong(q));
    });
    if (ty == 0 && c < ncol) on[(k * F::NN + i) * ncol + c] = __double_as_longlong(r[tid]);
  }
}

// one pass of Op{members...} over the plan's grid
template <class Op, class... A>
int colred_launch(hipStream_t s, const colred_grid& g, const colred_out& out, A... members) {
  hipLaunchKernelGGL((colred_pass<Op, A...>), dim3((unsigned)g.ntile, (unsigned)g.nch),
                     dim3(PO_THREADS), 0, s, g.M, g.ncol, g.cw, g.rows, out.d, out.n, out.dstride,
                     out.dstep, members...);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

// ---------------------------------------------------------------- the fold
// the partials of column c merged in chunk order.  One thread walks all chunks, so the loop is as
// slow as its loads are serial: the pointers step by additions alone, and the loop is unrolled so
// that the loads of four chunks are in flight while the merges stay in chunk order.
template <class Op>
__device__ __forceinline__ typename Op::F::acc colred_fold(const colred_out& out, long long nch,
                                                           int ncol, int c) {
  using F = typename Op::F;
  typename F::acc a = F::identity();
  const long long dchunk = (long long)out.dstride * ncol, dfield = (long long)out.dstep * ncol;
  const double* pd = out.d + c;
  const long long* pn = F::NN ? out.n + c : nullptr;
#pragma unroll 4
  for (long long k = 0; k < nch; ++k, pd += dchunk, pn += (long long)F::NN * ncol) {
#pragma unroll
    for (int i = 0; i < F::ND; ++i) a.d[i] = F::merge(i, a.d[i], pd[i * dfield]);
#pragma unroll
    for (int i = 0; i < F::NN; ++i) a.n[i] += pn[(long long)i * ncol];
  }
  return a;
}

}  // namespace
