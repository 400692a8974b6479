// nh_posterior.hip -- column reductions over a chain in HBM for the posterior figures: what
// np.histogram, np.histogram2d and scipy.stats.gaussian_kde compute on the host for naima's
// plot_chain / plot_distribution panels and for a corner plot, without bringing the samples back.
// Every entry point reads a row-major device matrix x[M][ld] with ncol <= ld columns in use (the
// layout of get_chain(flat=True) and of stored scalar blobs).
//
//   nh_column_moments  per column: the counts of finite values and of NaNs, min, max, mean and the
//                      unbiased variance of the finite values.  Two chunk passes of nh_colred.h
//                      (the mean, then the sum of (x - mean)^2), each folded in chunk order.
//   nh_hist_columns    1-D counts of every column and 2-D counts of a list of column pairs on
//                      per-column edges.  A thread reads a row, bins every column once (an
//                      arithmetic estimate corrected against the edges, as NumPy does), keeps the
//                      indices in LDS and feeds the 1-D and every pair histogram from them:
//                      32-bit counts in LDS (integer LDS atomics), merged into the 64-bit global
//                      bins with agent-scope integer atomics.  Histograms that do not fit one
//                      workgroup's LDS together are spread over several launches (groups of
//                      columns and pairs); counts are integers, so the grouping cannot show.
//   nh_kde_columns     the Gaussian kernel density of every column at G points.  A workgroup takes
//                      (point tile, row chunk, column), stages the chunk's values in LDS (a
//                      broadcast read per row) and writes one partial per point; a second launch
//                      sums the partials in chunk order and normalises.
//   nh_group_moments   the chain [rows][walker][parameter] of k ensembles of n walkers, its rows cut
//                      into nsplit parts: per (part, ensemble, parameter) the count, mean and
//                      unbiased variance of the finite values over all the ensemble's walkers (the
//                      sequences of a Gelman-Rubin R-hat).  Two passes as above; a workgroup takes
//                      (row chunk, ensemble, part) and walks the ensemble's n*ndim contiguous
//                      values of its rows with a stride that is a multiple of ndim, so a thread
//                      keeps one parameter; the threads of a parameter are summed in thread order,
//                      the chunks in chunk order.
//
// No floating-point atomics: every floating-point sum has an order fixed by the shapes alone, so
// repeated calls give bit-identical results.  Row indices are 64-bit.  Every launch is on the
// context's stream; nothing synchronises with the host.
#include "nh_colred.h"

namespace {

constexpr int PO_CTR_BUDGET = 11264;   // 32-bit LDS counters per histogram workgroup (44 KiB)
constexpr int PO_KDE_STAGE = 1024;     // values of a column per LDS stage of the KDE kernel
constexpr unsigned short PO_DROPPED = 0xffffu;

// ---------------------------------------------------------------- moments
// (the chunk pass, its partials and the fold in chunk order: nh_colred.h)
// sum, min, max of the finite values | their number, that of the NaNs
struct k_po_sum {
  using F = colred_fields<2, '+', '<', '>'>;
  const double* __restrict__ x;
  long long ld;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    long long n = 0, nn = 0;
    walk([&](long long t) {
      double v = x[t * ld + c];
      if (po_finite(v)) {
        s += v;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
        ++n;
      }
      nn += v != v ? 1 : 0;  // (beside the branch: a counter moves in every row, nh_colred.h)
    });
    a = {{s, lo, hi}, {n, nn}};
  }
};

// counts[0|1][c] = n, NaNs; stats[0|1|2][c] = min, max, mean (NaN without a finite value; the
// value itself for a column whose finite values are all equal)
__global__ void k_po_mean(long long nch, int ncol, long long* __restrict__ counts,
                          double* __restrict__ stats, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const auto a = colred_fold<k_po_sum>(part, nch, ncol, c);
  const double s = a.d[0], lo = a.d[1], hi = a.d[2];
  const long long n = a.n[0];
  counts[c] = n;
  counts[ncol + c] = a.n[1];
  stats[c] = n ? lo : nh_nan();
  stats[ncol + c] = n ? hi : nh_nan();
  stats[2 * ncol + c] = n ? (lo == hi ? lo : s / (double)n) : nh_nan();
}

// the sum of (x - mean)^2 over the finite values
struct k_po_sq {
  using F = colred_fields<0, '+'>;
  const double* __restrict__ x;
  long long ld;
  const double* __restrict__ stats;
  int ncol;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    const double mean = stats[2 * ncol + c];
    double q = 0.0;
    walk([&](long long t) {
      double v = x[t * ld + c];
      if (po_finite(v)) {
        double d = v - mean;
        q = fma(d, d, q);
      }
    });
    a = {{q}};
  }
};

// stats[3][c] = sum / (n - 1): exactly 0 for equal values, NaN for fewer than two
__global__ void k_po_var(long long nch, int ncol, const long long* __restrict__ counts,
                         double* __restrict__ stats, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double q = colred_fold<k_po_sq>(part, nch, ncol, c).d[0];
  long long n = counts[c];
  double var = nh_nan();
  if (n > 1) var = stats[c] == stats[ncol + c] ? 0.0 : q / (double)(n - 1);
  stats[3 * ncol + c] = var;
}

// ---------------------------------------------------------------- group moments
// rows [first + p*L, first + (p+1)*L) are part p; a part has nch chunks of `rows` rows
struct po_groups {
  long long first, L, rows, nch, ld;
  int k, n, ndim;
};

// the values of (part, ensemble, chunk) that thread `tid` of T = (256/ndim)*ndim visits: the flat
// index tid + j*T over [row][n*ndim]; n*ndim and T are multiples of ndim, so the parameter of
// every one of them is tid % ndim.  f(v) per value.
template <typename F>
__device__ __forceinline__ void po_group_walk(const double* __restrict__ x, const po_groups& g,
                                              int tid, int T, F f) {
  const long long E = (long long)g.n * g.ndim;
  const long long t0 = g.first + blockIdx.z * g.L + blockIdx.x * g.rows;
  const long long t1 = min(g.first + (blockIdx.z + 1) * g.L, t0 + g.rows);
  const double* base = x + (long long)blockIdx.y * E;
  const long long qT = T / E, rT = T % E;
  long long row = t0 + tid / E, e = tid % E;
  while (row < t1) {
    f(base[row * g.ld + e]);
    e += rT;
    row += qT;
    if (e >= E) { e -= E; ++row; }
  }
}

// per (part p, ensemble r, chunk c, parameter d), i = ((p*k + r)*nch + c)*ndim + d:
// pd[3 i + 0|1|2] = sum, min, max of the finite values, pc[i] their number
__global__ __launch_bounds__(PO_THREADS) void k_po_gsum(const double* __restrict__ x, po_groups g,
                                                        double* __restrict__ pd,
                                                        long long* __restrict__ pc) {
  __shared__ double rs[PO_THREADS], rlo[PO_THREADS], rhi[PO_THREADS];
  __shared__ long long rn[PO_THREADS];
  const int tid = threadIdx.x, T = (PO_THREADS / g.ndim) * g.ndim;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  long long n = 0;
  if (tid < T)
    po_group_walk(x, g, tid, T, [&](double v) {
      if (po_finite(v)) {
        s += v;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
        ++n;
      }
    });
  rs[tid] = s; rlo[tid] = lo; rhi[tid] = hi; rn[tid] = n;
  __syncthreads();
  if (tid < g.ndim) {
    for (int j = tid + g.ndim; j < T; j += g.ndim) {
      s += rs[j];
      lo = fmin(lo, rlo[j]);
      hi = fmax(hi, rhi[j]);
      n += rn[j];
    }
    long long i = (((long long)blockIdx.z * g.k + blockIdx.y) * g.nch + blockIdx.x) * g.ndim + tid;
    pd[3 * i] = s; pd[3 * i + 1] = lo; pd[3 * i + 2] = hi;
    pc[i] = n;
  }
}

// per group q = (p*k + r)*ndim + d of nq: counts[q] = n, stats[q] = mean (NaN without a finite
// value; the value itself when all are equal), lohi[2 q + 0|1] = min, max
__global__ void k_po_gmean(const double* __restrict__ pd, const long long* __restrict__ pc,
                           long long nch, int ndim, long long nq, long long* __restrict__ counts,
                           double* __restrict__ stats, double* __restrict__ lohi) {
  long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const long long i0 = (q / ndim) * nch * ndim + q % ndim;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  long long n = 0;
  for (long long c = 0; c < nch; ++c) {
    long long i = i0 + c * ndim;
    s += pd[3 * i];
    lo = fmin(lo, pd[3 * i + 1]);
    hi = fmax(hi, pd[3 * i + 2]);
    n += pc[i];
  }
  counts[q] = n;
  stats[q] = n ? (lo == hi ? lo : s / (double)n) : nh_nan();
  lohi[2 * q] = lo;
  lohi[2 * q + 1] = hi;
}

// pq[i] = the chunk's sum of (x - mean)^2 over the finite values (i as in k_po_gsum)
__global__ __launch_bounds__(PO_THREADS) void k_po_gsq(const double* __restrict__ x, po_groups g,
                                                       const double* __restrict__ stats,
                                                       double* __restrict__ pq) {
  __shared__ double rq[PO_THREADS];
  const int tid = threadIdx.x, T = (PO_THREADS / g.ndim) * g.ndim;
  const long long grp = (long long)blockIdx.z * g.k + blockIdx.y;
  double q = 0.0;
  if (tid < T) {
    const double mean = stats[grp * g.ndim + tid % g.ndim];
    po_group_walk(x, g, tid, T, [&](double v) {
      if (po_finite(v)) {
        double d = v - mean;
        q = fma(d, d, q);
      }
    });
  }
  rq[tid] = q;
  __syncthreads();
  if (tid < g.ndim) {
    for (int j = tid + g.ndim; j < T; j += g.ndim) q += rq[j];
    pq[(grp * g.nch + blockIdx.x) * g.ndim + tid] = q;
  }
}

// stats[nq + q] = sum / (n - 1): exactly 0 for equal values, NaN for fewer than two
__global__ void k_po_gvar(const double* __restrict__ pq, long long nch, int ndim, long long nq,
                          const long long* __restrict__ counts,
                          const double* __restrict__ lohi, double* __restrict__ stats) {
  long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const long long i0 = (q / ndim) * nch * ndim + q % ndim;
  double sq = 0.0;
  for (long long c = 0; c < nch; ++c) sq += pq[i0 + c * ndim];
  long long n = counts[q];
  double var = nh_nan();
  if (n > 1) var = lohi[2 * q] == lohi[2 * q + 1] ? 0.0 : sq / (double)(n - 1);
  stats[nq + q] = var;
}

// ---------------------------------------------------------------- histograms
struct po_pairs { unsigned char i[NH_HIST_MAX_PAIRS], j[NH_HIST_MAX_PAIRS]; };

// the bin of v on the edges e[0..nb]: k with e[k] <= v < e[k+1], the last bin closed on the right;
// PO_DROPPED outside [e[0], e[nb]] and for NaN and +-inf
__device__ __forceinline__ unsigned short po_bin(double v, const double* __restrict__ e, int nb) {
  const double lo = e[0], hi = e[nb];
  if (!po_finite(v) || !(v >= lo && v <= hi)) return PO_DROPPED;
  int k = (int)((v - lo) / (hi - lo) * (double)nb);
  k = min(max(k, 0), nb - 1);
  while (k > 0 && v < e[k]) --k;
  while (k < nb - 1 && v >= e[k + 1]) ++k;
  return (unsigned short)k;
}

// the 1-D histograms of columns [c0, c1) and the 2-D ones of pairs [p0, p1) over the rows of
// this workgroup.  LDS: [(c1-c0)*nb | (p1-p0)*nb*nb] 32-bit counters, then the bin of every
// column of the thread's row, idx[c][thread] (thread-private: no barrier in the row loop)
__global__ __launch_bounds__(PO_THREADS) void k_po_hist(const double* __restrict__ x, long long M,
                                                        int ncol, long long ld,
                                                        const double* __restrict__ edges, int nb,
                                                        long long rpb, int c0, int c1, int p0,
                                                        int p1, po_pairs pr,
                                                        unsigned long long* __restrict__ h1,
                                                        unsigned long long* __restrict__ h2) {
  extern __shared__ unsigned po_lds[];
  const int n1 = (c1 - c0) * nb, n2 = (p1 - p0) * nb * nb;
  unsigned* ctr2 = po_lds + n1;
  unsigned short* idx = (unsigned short*)(po_lds + n1 + n2);
  int tid = threadIdx.x;
  for (int i = tid; i < n1 + n2; i += PO_THREADS) po_lds[i] = 0u;
  __syncthreads();
  long long row0 = (long long)blockIdx.x * rpb, row1 = min(M, row0 + rpb);
  for (long long row = row0 + tid; row < row1; row += PO_THREADS) {
    const double* xr = x + row * ld;
    for (int c = 0; c < ncol; ++c)
      idx[c * PO_THREADS + tid] = po_bin(xr[c], edges + (long long)c * (nb + 1), nb);
    for (int c = c0; c < c1; ++c) {
      unsigned k = idx[c * PO_THREADS + tid];
      if (k != PO_DROPPED)
        __hip_atomic_fetch_add(po_lds + (c - c0) * nb + k, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    for (int p = p0; p < p1; ++p) {
      unsigned a = idx[pr.i[p] * PO_THREADS + tid], b = idx[pr.j[p] * PO_THREADS + tid];
      if (a != PO_DROPPED && b != PO_DROPPED)
        __hip_atomic_fetch_add(ctr2 + ((p - p0) * nb + a) * nb + b, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();
  for (int i = tid; i < n1; i += PO_THREADS) {
    unsigned v = po_lds[i];
    if (v) __hip_atomic_fetch_add(h1 + (long long)c0 * nb + i, (unsigned long long)v,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int i = tid; i < n2; i += PO_THREADS) {
    unsigned v = ctr2[i];
    if (v) __hip_atomic_fetch_add(h2 + (long long)p0 * nb * nb + i, (unsigned long long)v,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- KDE
// threads are [RS = 256/gp row lanes][gp points]; part[(c*nch + k)*G + g] = the sum over the
// finite values of chunk k of exp(-((p[c][g] - x)/h_c)^2 / 2), pn[c*nch + k] their number
__global__ __launch_bounds__(PO_THREADS) void k_po_kde(const double* __restrict__ x, long long M,
                                                       long long ld,
                                                       const double* __restrict__ pts, int G,
                                                       const double* __restrict__ bw, int gp,
                                                       long long rows, long long nch,
                                                       double* __restrict__ part,
                                                       long long* __restrict__ pn) {
  __shared__ double xs[PO_KDE_STAGE];
  __shared__ double red[PO_THREADS];
  __shared__ unsigned nfin;
  int tid = threadIdx.x, tg = tid % gp, rl = tid / gp, RS = PO_THREADS / gp;
  int g = blockIdx.x * gp + tg;
  long long k = blockIdx.y;
  int c = blockIdx.z;
  const double inv = 1.0 / bw[c];
  const double p = g < G ? pts[(long long)c * G + g] : 0.0;
  long long t0 = k * rows, t1 = min(M, t0 + rows);
  if (tid == 0) nfin = 0u;
  __syncthreads();
  double acc = 0.0;
  unsigned nf = 0u;
  for (long long tb = t0; tb < t1; tb += PO_KDE_STAGE) {
    int len = (int)min((long long)PO_KDE_STAGE, t1 - tb);
    __syncthreads();  // (the stage before has been read)
    for (int i = tid; i < len; i += PO_THREADS) {
      double v = x[(tb + i) * ld + c];
      bool f = po_finite(v);
      xs[i] = f ? v : INFINITY;  // (p - inf)^2 = inf: the term is exp(-inf) = 0
      nf += f;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = rl; i < len; i += RS) {
      double u = (p - xs[i]) * inv;
      acc += exp(-0.5 * u * u);
    }
  }
  red[tid] = acc;
  if (nf) __hip_atomic_fetch_add(&nfin, nf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  for (int s = RS >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if (rl < s) red[tid] += red[tid + s * gp];
  }
  __syncthreads();
  if (rl == 0 && g < G) part[((long long)c * nch + k) * G + g] = red[tid];
  if (tid == 0 && blockIdx.x == 0) pn[(long long)c * nch + k] = (long long)nfin;
}

// out[c][g] = sum_k part / (n_c h_c sqrt(2 pi)), the chunks in order
__global__ void k_po_kde_reduce(const double* __restrict__ part, const long long* __restrict__ pn,
                                long long nch, int G, const double* __restrict__ bw,
                                double* __restrict__ out) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  int c = blockIdx.y;
  if (g >= G) return;
  double s = 0.0;
  long long n = 0;
  for (long long k = 0; k < nch; ++k) {
    s += part[((long long)c * nch + k) * G + g];
    n += pn[(long long)c * nch + k];
  }
  out[(long long)c * G + g] = s / ((double)n * bw[c] * 2.5066282746310002);
}

}  // namespace

extern "C" int nh_column_moments(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                                 long long* counts, double* stats) {
  NH_REQUIRE(ctx && x && counts && stats, "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_ANY);
  const colred_grid g = colred_plan(M, ncol);
  NH_REQUIRE_PLAN(g);
  const long long nch = g.nch;
  // scratch: pd [nch][3][ncol] | pq [nch][ncol] | pc [nch][2][ncol]
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)nch * ncol * 6 * 8, &base);
  if (rc) return rc;
  double* pd = (double*)base;
  double* pq = pd + (size_t)nch * 3 * ncol;
  long long* pc = (long long*)(pq + (size_t)nch * ncol);
  const colred_out sums = colred_dense<k_po_sum>(pd, pc), sq = colred_dense<k_po_sq>(pq);
  hipStream_t s = ctx->stream;
  if ((rc = colred_launch<k_po_sum>(s, g, sums, x, ld))) return rc;
  hipLaunchKernelGGL(k_po_mean, dim3(g.col_blocks()), dim3(PO_THREADS), 0, s, nch, ncol, counts, stats,
                     sums);
  NH_CHECK_HIP(hipGetLastError());
  if ((rc = colred_launch<k_po_sq>(s, g, sq, x, ld, stats, ncol))) return rc;
  hipLaunchKernelGGL(k_po_var, dim3(g.col_blocks()), dim3(PO_THREADS), 0, s, nch, ncol, counts, stats,
                     sq);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_hist_columns(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                               const double* edges, int nb, const int* pairs, int npairs,
                               long long* h1, long long* h2) {
  NH_REQUIRE(ctx && x && edges && h1, "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_ANY);
  NH_REQUIRE(ncol <= NH_HIST_MAX_COLS, "ncol > NH_HIST_MAX_COLS");
  NH_REQUIRE(nb >= 1, "nb must be positive");
  NH_REQUIRE(nb <= NH_HIST_MAX_BINS_1D, "nb > NH_HIST_MAX_BINS_1D");
  NH_REQUIRE(npairs >= 0 && npairs <= NH_HIST_MAX_PAIRS, "npairs outside [0, NH_HIST_MAX_PAIRS]");
  NH_REQUIRE(npairs == 0 || (pairs && h2), "null argument");
  NH_REQUIRE(npairs == 0 || nb <= NH_HIST_MAX_BINS_2D, "nb > NH_HIST_MAX_BINS_2D with pairs");
  po_pairs pr = {};
  for (int p = 0; p < npairs; ++p) {
    int i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || i >= ncol || j < 0 || j >= ncol)
      return nh_set_error(NH_EINVAL, "nh_hist_columns: pair %d is (%d, %d), outside [0, %d)", p, i,
                          j, ncol);
    pr.i[p] = (unsigned char)i;
    pr.j[p] = (unsigned char)j;
  }
  hipStream_t s = ctx->stream;
  NH_CHECK_HIP(hipMemsetAsync(h1, 0, (size_t)ncol * nb * 8, s));
  if (npairs) NH_CHECK_HIP(hipMemsetAsync(h2, 0, (size_t)npairs * nb * nb * 8, s));
  long long rpb = std::max<long long>(4 * PO_MIN_ROWS, cdiv(M, PO_TARGET_WG / 2));
  rpb = cdiv(rpb, PO_THREADS) * PO_THREADS;
  unsigned nrb = (unsigned)cdiv(M, rpb);
  // groups: the columns in order, then the pairs in order, as many as fit the counter budget
  const int per_c = nb, per_p = nb * nb;
  int c = 0, p = 0;
  while (c < ncol || p < npairs) {
    int used = 0, c0 = c, p0 = p;
    while (c < ncol && used + per_c <= PO_CTR_BUDGET) { used += per_c; ++c; }
    if (c == ncol)
      while (p < npairs && used + per_p <= PO_CTR_BUDGET) { used += per_p; ++p; }
    size_t lds = (size_t)used * 4 + (size_t)ncol * PO_THREADS * 2;
    hipLaunchKernelGGL(k_po_hist, dim3(nrb), dim3(PO_THREADS), lds, s, x, M, ncol, ld, edges, nb,
                       rpb, c0, c, p0, p, pr, (unsigned long long*)h1, (unsigned long long*)h2);
    NH_CHECK_HIP(hipGetLastError());
  }
  return NH_OK;
}

extern "C" int nh_kde_columns(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                              const double* points, int G, const double* bw, double* out) {
  NH_REQUIRE(ctx && x && points && bw && out, "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_ANY);
  NH_REQUIRE(ncol <= 65535, "ncol > 65535");
  NH_REQUIRE(G > 0, "G must be positive");
  int gp = po_pow2_at_least(G, PO_THREADS);
  long long npt = cdiv(G, gp), rows, nch;
  po_chunks(M, npt * ncol, 1, &rows, &nch);
  // scratch: part [ncol][nch][G] | pn [ncol][nch]
  void* base = nullptr;
  int rc = nh_scratch(ctx, ((size_t)ncol * nch * G + (size_t)ncol * nch) * 8, &base);
  if (rc) return rc;
  double* part = (double*)base;
  long long* pn = (long long*)(part + (size_t)ncol * nch * G);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_po_kde, dim3((unsigned)npt, (unsigned)nch, (unsigned)ncol),
                     dim3(PO_THREADS), 0, s, x, M, ld, points, G, bw, gp, rows, nch, part, pn);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_po_kde_reduce, dim3((unsigned)cdiv(G, PO_THREADS), (unsigned)ncol),
                     dim3(PO_THREADS), 0, s, part, pn, nch, G, bw, out);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_group_moments(nh_ctx* ctx, const double* x, long long row0, long long nrows,
                                long long ld, int k, int n, int ndim, int nsplit,
                                long long* counts, double* stats) {
  NH_REQUIRE(ctx && x && counts && stats, "null argument");
  NH_REQUIRE(k >= 1 && k <= 65535, "k outside [1, 65535]");
  NH_REQUIRE(n >= 1, "n must be positive");
  NH_REQUIRE(ndim >= 1 && ndim <= PO_THREADS, "ndim outside [1, 256]");
  NH_REQUIRE(nsplit >= 1 && nsplit <= 65535, "nsplit outside [1, 65535]");
  NH_REQUIRE(row0 >= 0, "row0 is negative");
  NH_REQUIRE(nrows >= nsplit, "fewer rows than parts");
  const long long E = (long long)n * ndim;
  NH_REQUIRE(E <= (1ll << 40) / k && ld >= (long long)k * E, "k * n * ndim > ld");
  po_groups g;
  g.L = nrows / nsplit;
  g.first = row0 + (nrows - g.L * nsplit);  // (the remainder is dropped from the front)
  g.ld = ld; g.k = k; g.n = n; g.ndim = ndim;
  // chunks of a part: a workgroup reads 16 values per thread at least, the launch aims at
  // PO_TARGET_WG workgroups -- a function of the shapes only
  long long want = std::max<long long>(1, PO_TARGET_WG / ((long long)k * nsplit));
  long long nch = std::min(
      want, std::max<long long>(1, (long long)((double)g.L * (double)E / (16.0 * PO_THREADS))));
  g.rows = cdiv(g.L, nch);
  g.nch = cdiv(g.L, g.rows);
  const long long nq = (long long)nsplit * k * ndim, ni = nq * g.nch;
  // scratch: pd [ni][3] | pq [ni] | lohi [nq][2] | pc [ni]
  void* base = nullptr;
  int rc = nh_scratch(ctx, ((size_t)ni * 5 + (size_t)nq * 2) * 8, &base);
  if (rc) return rc;
  double* pd = (double*)base;
  double* pq = pd + (size_t)ni * 3;
  double* lohi = pq + (size_t)ni;
  long long* pc = (long long*)(lohi + (size_t)nq * 2);
  hipStream_t s = ctx->stream;
  dim3 grid((unsigned)g.nch, (unsigned)k, (unsigned)nsplit);
  unsigned qb = (unsigned)cdiv(nq, PO_THREADS);
  hipLaunchKernelGGL(k_po_gsum, grid, dim3(PO_THREADS), 0, s, x, g, pd, pc);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_po_gmean, dim3(qb), dim3(PO_THREADS), 0, s, pd, pc, g.nch, ndim, nq, counts,
                     stats, lohi);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_po_gsq, grid, dim3(PO_THREADS), 0, s, x, g, stats, pq);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_po_gvar, dim3(qb), dim3(PO_THREADS), 0, s, pq, g.nch, ndim, nq, counts, lohi,
                     stats);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
