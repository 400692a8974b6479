// nh_infocrit.hip -- model comparison from a chain's stored spectra: the pointwise log-likelihood
// matrix L[sample][data point] and the column reductions WAIC and PSIS-LOO need, without bringing
// the samples back.  Matrices are row-major device matrices [M][ld] with ncol <= ld columns in
// use, as in nh_posterior.hip.
//
//   nh_pointwise_lnl     L[s][k] = the term of data point k in core.lnprobmodel (core.py:64-94) of
//                        spectrum s: one wave per row, as the likelihood kernel (nh_lnprob.h) --
//                        a first walk over the row counts the violated upper limits (the
//                        reference indexes cl by that count, core.py:89-92), a second one writes
//                        the terms; optionally the row totals; the number of non-finite terms in
//                        a device int64 (an integer atomic per wave that met one).
//   nh_lnl_column_stats  per column of L: max, mean, unbiased variance, lse = max + log sum
//                        exp(L - max), min.  Two passes over L in the tiling of nh_colred.h, the
//                        per-chunk partials summed in chunk order.
//   nh_psis_columns      Pareto-smoothed importance sampling per column (Vehtari, Simpson, Gelman,
//                        Yao, Gabry; the generalised-Pareto fit of Zhang & Stephens 2009 with the
//                        weak priors of the loo package).  With x = min(L) - L (the negated column,
//                        its maximum subtracted) and the cutoff from the order statistic of rank
//                        Mt of L (nh_column_select), one chunked pass over L sums exp(x) and
//                        exp(x + L - min) over the rows with x <= cut per chunk, and appends the
//                        tail rows (x > cut: at most Mt of them) to a per-column list through an
//                        integer atomic counter -- the pass reads L coalesced, which a workgroup
//                        walking one column could not.  Then one workgroup per column loads its
//                        list into LDS, sorts it by (value, row index) (a bitonic network), fits
//                        the generalised Pareto distribution (a wave per candidate b_j, lanes over
//                        the tail, butterfly sums), replaces the tail by the fitted quantiles and
//                        adds the tail's share of the two sums; no [M][ncol] weight matrix exists.
//
// Two facts that follow from the definitions.  The list's order after the atomic gather is
// arbitrary, the sort by (value, row) removes it; rows whose values tie can then only be told
// apart by their index, and swapping two tied rows of L changes nothing in elpd_loo because tied
// rows have equal L: the same smoothed values meet the same L.  pareto_k is a function of the
// sorted tail VALUES alone, so it does not depend on the order of the rows at all.
//
// No floating-point atomics: every floating-point sum has an order fixed by the shapes alone (and,
// in the tail, by the sorted values), so repeated calls give bit-identical results.  Row indices
// are 64-bit, M < 2^31.  Every launch is on the context's stream; nothing synchronises with the
// host.
#include "nh_gpd.h"

namespace {

// ---------------------------------------------------------------- pointwise terms
__global__ __launch_bounds__(PO_THREADS) void k_crit_pointwise(
    const double* __restrict__ x, long long M, int nE, long long ld,
    const double* __restrict__ conv, const double* __restrict__ flux,
    const double* __restrict__ elo, const double* __restrict__ ehi, const int* __restrict__ ul,
    const double* __restrict__ cl, double* __restrict__ L, long long ldL,
    double* __restrict__ total, unsigned long long* __restrict__ nbad) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * (PO_THREADS / 64);
  for (long long s = (long long)blockIdx.x * (PO_THREADS / 64) + (threadIdx.x >> 6); s < M;
       s += stride) {  // (s is the wave's: every loop bound below is wave-uniform)
    const double* xr = x + s * ld;
    int nviol = 0;
    for (int k = lane; k < nE; k += 64)
      if (ul[k]) nviol += (xr[k] * conv[k] > flux[k]) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nviol += __shfl_xor(nviol, off, 64);
    // quirk kept from core.py:89-92: cl is indexed by the row's violation count (cl has nE + 1
    // entries); every violated limit of the row carries log(1 - cl[nviol])
    const double pen = nviol > 0 ? log(1.0 - cl[nviol]) : 0.0;
    double acc = 0.0;
    int bad = 0;
    for (int k = lane; k < nE; k += 64) {
      const double mc = xr[k] * conv[k];
      const double f = flux[k];
      double t;
      if (ul[k]) {
        t = (mc > f) ? pen : 0.0;
      } else {
        const double d = mc - f;
        const double sg = (d > 0.0) ? ehi[k] : elo[k];
        t = -(d * d) / (2.0 * (sg * sg));
      }
      L[s * ldL + k] = t;
      acc += t;
      bad += po_finite(t) ? 0 : 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      acc += __shfl_down(acc, off, 64);
      bad += __shfl_down(bad, off, 64);
    }
    if (lane == 0) {
      if (total) total[s] = acc;
      if (bad)
        __hip_atomic_fetch_add(nbad, (unsigned long long)bad, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------- column statistics
// per (row chunk k, column c): pd[(k*3 + 0|1|2)*ncol + c] = sum, min, max
__global__ __launch_bounds__(PO_THREADS) void k_crit_sum(const double* __restrict__ x, long long M,
                                                       int ncol, long long ld, int cw,
                                                       long long rows, double* __restrict__ pd) {
  __shared__ double rs[PO_THREADS], rlo[PO_THREADS], rhi[PO_THREADS];
  int tid = threadIdx.x, tx = tid % cw, ty = tid / cw, R = PO_THREADS / cw;
  int c = blockIdx.x * cw + tx;
  long long k = blockIdx.y;
  long long t0 = k * rows, t1 = min(M, t0 + rows);
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  if (c < ncol) {
    for (long long t = t0 + ty; t < t1; t += R) {
      double v = x[t * ld + c];
      s += v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
  }
  rs[tid] = s; rlo[tid] = lo; rhi[tid] = hi;
  po_tree(rs, tid, ty, cw, [](double a, double b) { return a + b; });
  po_tree(rlo, tid, ty, cw, [](double a, double b) { return fmin(a, b); });
  po_tree(rhi, tid, ty, cw, [](double a, double b) { return fmax(a, b); });
  if (ty == 0 && c < ncol) {
    pd[(k * 3 + 0) * ncol + c] = rs[tid];
    pd[(k * 3 + 1) * ncol + c] = rlo[tid];
    pd[(k * 3 + 2) * ncol + c] = rhi[tid];
  }
}

// stats[0|1|4][c] = max, mean (the value itself for a column of equal values), min
__global__ void k_crit_mean(const double* __restrict__ pd, long long nch, int ncol, long long M,
                          double* __restrict__ stats) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  for (long long k = 0; k < nch; ++k) {
    s += pd[(k * 3 + 0) * ncol + c];
    lo = fmin(lo, pd[(k * 3 + 1) * ncol + c]);
    hi = fmax(hi, pd[(k * 3 + 2) * ncol + c]);
  }
  stats[c] = hi;
  stats[ncol + c] = lo == hi ? lo : s / (double)M;
  stats[4 * ncol + c] = lo;
}

// pq[(k*2 + 0|1)*ncol + c] = the chunk's sums of (x - mean)^2 and of exp(x - max)
__global__ __launch_bounds__(PO_THREADS) void k_crit_sq(const double* __restrict__ x, long long M,
                                                      int ncol, long long ld, int cw,
                                                      long long rows,
                                                      const double* __restrict__ stats,
                                                      double* __restrict__ pq) {
  __shared__ double rq[PO_THREADS], re[PO_THREADS];
  int tid = threadIdx.x, tx = tid % cw, ty = tid / cw, R = PO_THREADS / cw;
  int c = blockIdx.x * cw + tx;
  long long k = blockIdx.y;
  long long t0 = k * rows, t1 = min(M, t0 + rows);
  double q = 0.0, e = 0.0;
  if (c < ncol) {
    const double hi = stats[c], mean = stats[ncol + c];
    for (long long t = t0 + ty; t < t1; t += R) {
      double v = x[t * ld + c];
      double d = v - mean;
      q = fma(d, d, q);
      e += exp(v - hi);
    }
  }
  rq[tid] = q; re[tid] = e;
  po_tree(rq, tid, ty, cw, [](double a, double b) { return a + b; });
  po_tree(re, tid, ty, cw, [](double a, double b) { return a + b; });
  if (ty == 0 && c < ncol) {
    pq[(k * 2 + 0) * ncol + c] = rq[tid];
    pq[(k * 2 + 1) * ncol + c] = re[tid];
  }
}

// stats[2][c] = sum / (M - 1): exactly 0 for equal values, NaN for M == 1;
// stats[3][c] = max + log(sum of exp(x - max))
__global__ void k_crit_fin(const double* __restrict__ pq, long long nch, int ncol, long long M,
                         double* __restrict__ stats) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  double q = 0.0, e = 0.0;
  for (long long k = 0; k < nch; ++k) {
    q += pq[(k * 2 + 0) * ncol + c];
    e += pq[(k * 2 + 1) * ncol + c];
  }
  const double hi = stats[c], lo = stats[4 * ncol + c];
  stats[2 * ncol + c] = M > 1 ? (lo == hi ? 0.0 : q / (double)(M - 1)) : crit_nan();
  stats[3 * ncol + c] = hi + log(e);
}

// ---------------------------------------------------------------- PSIS
// the cutoff of column c on x = min - L: the order statistic of rank Mt of L is that of rank
// M - Mt - 1 of x (the map is monotone), floored at log(DBL_MIN)
__device__ __forceinline__ double crit_cut(double lmin, double lsel) {
  return fmax(lmin - lsel, CRIT_LOG_TINY);
}

// per (row chunk k, column c) over the rows with x <= cut: part[(k*2 + 0|1)*ncol + c] = the sums
// of exp(x) and of exp((x + L) - min); the rows with x > cut go to the column's list
// tx / trow [c*cap ..], their number to cnt[c] (zeroed before the launch)
__global__ __launch_bounds__(PO_THREADS) void k_crit_split(
    const double* __restrict__ L, long long M, int ncol, long long ld, int cw, long long rows,
    const double* __restrict__ stats, const double* __restrict__ lsel, int cap,
    double* __restrict__ part, double* __restrict__ tx, int* __restrict__ trow,
    unsigned* __restrict__ cnt) {
  __shared__ double ra[PO_THREADS], rb[PO_THREADS];
  int tid = threadIdx.x, txc = tid % cw, ty = tid / cw, R = PO_THREADS / cw;
  int c = blockIdx.x * cw + txc;
  long long k = blockIdx.y;
  long long t0 = k * rows, t1 = min(M, t0 + rows);
  double a = 0.0, b = 0.0;
  if (c < ncol) {
    const double lmin = stats[4 * ncol + c];
    const double cut = crit_cut(lmin, lsel[c]);
    for (long long t = t0 + ty; t < t1; t += R) {
      const double v = L[t * ld + c];
      const double xv = lmin - v;
      if (xv > cut) {
        unsigned slot = __hip_atomic_fetch_add(cnt + c, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
        if (slot < (unsigned)cap) {  // (always: at most Mt values lie above the rank-Mt statistic)
          tx[(long long)c * cap + slot] = xv;
          trow[(long long)c * cap + slot] = (int)t;
        }
      } else {
        a += exp(xv);
        b += exp((xv + v) - lmin);
      }
    }
  }
  ra[tid] = a; rb[tid] = b;
  po_tree(ra, tid, ty, cw, [](double p, double q) { return p + q; });
  po_tree(rb, tid, ty, cw, [](double p, double q) { return p + q; });
  if (ty == 0 && c < ncol) {
    part[(k * 2 + 0) * ncol + c] = ra[tid];
    part[(k * 2 + 1) * ncol + c] = rb[tid];
  }
}

// one workgroup per column: sort the tail, fit, smooth, finish the two log-sum-exps
__global__ __launch_bounds__(PO_THREADS) void k_crit_tail(
    const double* __restrict__ L, int ncol, long long ld, long long nch, int cap,
    const double* __restrict__ stats, const double* __restrict__ lsel,
    const double* __restrict__ part, const double* __restrict__ tx, const int* __restrict__ trow,
    const unsigned* __restrict__ cnt, double* __restrict__ pareto_k, long long* __restrict__ n_tail,
    double* __restrict__ elpd) {
  CRIT_TAIL_LDS(s);
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  const int n = (int)min(cnt[c], (unsigned)min(cap, CRIT_TAIL_MAX));
  const double lmin = stats[4 * ncol + c];
  const double cut = crit_cut(lmin, lsel[c]);
  const double ecut = exp(cut);
  // ---- the tail sorted by (value, row), fitted and smoothed (nh_gpd.h)
  const double kpar = crit_tail_fit(s, tx + (long long)c * cap, trow + (long long)c * cap, n, ecut, tid);
  double* xs = reinterpret_cast<double*>(s.key);
  double* tt = s.tt;
  double* red = s.red;
  const int* row = s.row;

  // ---- lw = x - logsumexp(x), elpd = logsumexp(lw + L): the tail's share of both sums, the
  // second one shifted by the tail's largest exponent (smoothing may lift x + L above min)
  double a = 0.0, emax = 0.0;
  __syncthreads();
  for (int i = tid; i < n; i += PO_THREADS) {
    const double xv = xs[i];
    a += exp(xv);
    const double e = (xv + L[(long long)row[i] * ld + c]) - lmin;
    tt[i] = e;  // (t is no longer needed)
    emax = fmax(emax, e);
  }
  a = crit_block_reduce(a, red, tid, [](double p, double q) { return p + q; });
  emax = crit_block_reduce(emax, red, tid, [](double p, double q) { return fmax(p, q); });
  double b = 0.0;
  for (int i = tid; i < n; i += PO_THREADS) b += exp(tt[i] - emax);
  b = crit_block_reduce(b, red, tid, [](double p, double q) { return p + q; });
  if (tid == 0) {
    double an = 0.0, bn = 0.0;
    for (long long k = 0; k < nch; ++k) {
      an += part[(k * 2 + 0) * ncol + c];
      bn += part[(k * 2 + 1) * ncol + c];
    }
    pareto_k[c] = kpar;
    n_tail[c] = n;
    elpd[c] = (lmin + emax) + (log(bn * exp(-emax) + b) - log(an + a));
  }
}

}  // namespace

#define CRIT_REQUIRE_MATRIX(M, ncol, ld)                             \
  NH_REQUIRE(M > 0, "M == 0: no samples");                         \
  NH_REQUIRE(M < (1ll << 31), "M >= 2^31 rows");                   \
  NH_REQUIRE(ncol > 0, "ncol must be positive");                   \
  NH_REQUIRE(ld >= ncol, "ncol > ld")

extern "C" int nh_pointwise_lnl(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                                const double* conv, const double* flux, const double* elo,
                                const double* ehi, const int* ul, const double* cl, double* L,
                                long long ldL, double* total, long long* nbad) {
  NH_REQUIRE(ctx && x && conv && flux && elo && ehi && ul && cl && L && nbad, "null argument");
  CRIT_REQUIRE_MATRIX(M, nE, ld);
  NH_REQUIRE(ldL >= nE, "nE > ldL");
  hipStream_t s = ctx->stream;
  NH_CHECK_HIP(hipMemsetAsync(nbad, 0, 8, s));
  unsigned nb = (unsigned)std::min<long long>(cdiv(M, PO_THREADS / 64), 8192);
  hipLaunchKernelGGL(k_crit_pointwise, dim3(nb), dim3(PO_THREADS), 0, s, x, M, nE, ld, conv, flux,
                     elo, ehi, ul, cl, L, ldL, total, (unsigned long long*)nbad);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_lnl_column_stats(nh_ctx* ctx, const double* L, long long M, int ncol,
                                   long long ld, double* stats) {
  NH_REQUIRE(ctx && L && stats, "null argument");
  CRIT_REQUIRE_MATRIX(M, ncol, ld);
  int cw = po_pow2_at_least(ncol, 64);
  long long ntile = cdiv(ncol, cw), rows, nch;
  po_chunks(M, ntile, PO_THREADS / cw, &rows, &nch);
  NH_REQUIRE(nch <= 65535 && ntile < (1ll << 31), "too many columns");
  // scratch: pd [nch][3][ncol] | pq [nch][2][ncol]
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)nch * ncol * 5 * 8, &base);
  if (rc) return rc;
  double* pd = (double*)base;
  double* pq = pd + (size_t)nch * 3 * ncol;
  hipStream_t s = ctx->stream;
  dim3 grid((unsigned)ntile, (unsigned)nch);
  unsigned cb = (unsigned)cdiv(ncol, PO_THREADS);
  hipLaunchKernelGGL(k_crit_sum, grid, dim3(PO_THREADS), 0, s, L, M, ncol, ld, cw, rows, pd);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_crit_mean, dim3(cb), dim3(PO_THREADS), 0, s, pd, nch, ncol, M, stats);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_crit_sq, grid, dim3(PO_THREADS), 0, s, L, M, ncol, ld, cw, rows, stats, pq);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_crit_fin, dim3(cb), dim3(PO_THREADS), 0, s, pq, nch, ncol, M, stats);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_psis_columns(nh_ctx* ctx, const double* L, long long M, int ncol, long long ld,
                               int Mt, const double* stats, const double* lsel, double* pareto_k,
                               long long* n_tail, double* elpd) {
  NH_REQUIRE(ctx && L && stats && lsel && pareto_k && n_tail && elpd, "null argument");
  CRIT_REQUIRE_MATRIX(M, ncol, ld);
  NH_REQUIRE(Mt >= 0 && Mt < M, "Mt outside [0, M)");
  NH_REQUIRE(Mt <= NH_PSIS_MAX_TAIL, "Mt > NH_PSIS_MAX_TAIL: thin the chain");
  const int cap = std::max(Mt, 1);
  int cw = po_pow2_at_least(ncol, 64);
  long long ntile = cdiv(ncol, cw), rows, nch;
  po_chunks(M, ntile, PO_THREADS / cw, &rows, &nch);
  NH_REQUIRE(nch <= 65535, "too many columns");
  // scratch: part [nch][2][ncol] | tx [ncol][cap] | trow [ncol][cap] | cnt [ncol]
  const size_t npart = (size_t)nch * 2 * ncol, nlist = (size_t)ncol * cap;
  void* base = nullptr;
  int rc = nh_scratch(ctx, (npart + nlist) * 8 + nlist * 4 + (size_t)ncol * 4, &base);
  if (rc) return rc;
  double* part = (double*)base;
  double* tx = part + npart;
  int* trow = (int*)(tx + nlist);
  unsigned* cnt = (unsigned*)(trow + nlist);
  hipStream_t s = ctx->stream;
  NH_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)ncol * 4, s));
  hipLaunchKernelGGL(k_crit_split, dim3((unsigned)ntile, (unsigned)nch), dim3(PO_THREADS), 0, s, L, M,
                     ncol, ld, cw, rows, stats, lsel, cap, part, tx, trow, cnt);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_crit_tail, dim3((unsigned)ncol), dim3(PO_THREADS), 0, s, L, ncol, ld, nch, cap,
                     stats, lsel, part, tx, trow, cnt, pareto_k, n_tail, elpd);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
