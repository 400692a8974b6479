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
//                        exp(L - max), min.  Two chunk passes over L (nh_colred.h).
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
// (the chunk pass, its partials and the fold in chunk order: nh_colred.h)
// sum, min, max
struct k_crit_sum {
  using F = colred_fields<0, '+', '<', '>'>;
  const double* __restrict__ x;
  long long ld;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    walk([&](long long t) {
      double v = x[t * ld + c];
      s += v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    });
    a = {{s, lo, hi}};
  }
};

// stats[0|1|4][c] = max, mean (the value itself for a column of equal values), min
__global__ void k_crit_mean(long long nch, int ncol, long long M, double* __restrict__ stats,
                            colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const auto a = colred_fold<k_crit_sum>(part, nch, ncol, c);
  const double s = a.d[0], lo = a.d[1], hi = a.d[2];
  stats[c] = hi;
  stats[ncol + c] = lo == hi ? lo : s / (double)M;
  stats[4 * ncol + c] = lo;
}

// the sums of (x - mean)^2 and of exp(x - max)
struct k_crit_sq {
  using F = colred_fields<0, '+', '+'>;
  const double* __restrict__ x;
  long long ld;
  const double* __restrict__ stats;
  int ncol;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    const double hi = stats[c], mean = stats[ncol + c];
    double q = 0.0, e = 0.0;
    walk([&](long long t) {
      double v = x[t * ld + c];
      double d = v - mean;
      q = fma(d, d, q);
      e += exp(v - hi);
    });
    a = {{q, e}};
  }
};

// stats[2][c] = sum / (M - 1): exactly 0 for equal values, NaN for M == 1;
// stats[3][c] = max + log(sum of exp(x - max))
__global__ void k_crit_fin(long long nch, int ncol, long long M, double* __restrict__ stats,
                           colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const auto a = colred_fold<k_crit_sq>(part, nch, ncol, c);
  const double q = a.d[0], e = a.d[1];
  const double hi = stats[c], lo = stats[4 * ncol + c];
  stats[2 * ncol + c] = M > 1 ? (lo == hi ? 0.0 : q / (double)(M - 1)) : nh_nan();
  stats[3 * ncol + c] = hi + log(e);
}

// ---------------------------------------------------------------- PSIS
// the cutoff of column c on x = min - L: the order statistic of rank Mt of L is that of rank
// M - Mt - 1 of x (the map is monotone), floored at log(DBL_MIN)
__device__ __forceinline__ double crit_cut(double lmin, double lsel) {
  return fmax(lmin - lsel, CRIT_LOG_TINY);
}

// over the rows with x <= cut: the sums of exp(x) and of exp((x + L) - min); the rows with x > cut
// go to the column's list tx / trow [c*cap ..], their number to cnt[c] (zeroed before the launch)
struct k_crit_split {
  using F = colred_fields<0, '+', '+'>;
  const double* __restrict__ L;
  long long ld;
  const double* __restrict__ stats;
  const double* __restrict__ lsel;
  int ncol, cap;
  double* __restrict__ tx;
  int* __restrict__ trow;
  unsigned* __restrict__ cnt;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    const double lmin = stats[4 * ncol + c];
    const double cut = crit_cut(lmin, lsel[c]);
    double sa = 0.0, sb = 0.0;
    walk([&](long long t) {
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
        sa += exp(xv);
        sb += exp((xv + v) - lmin);
      }
    });
    a = {{sa, sb}};
  }
};

// one workgroup per column: sort the tail, fit, smooth, finish the two log-sum-exps
__global__ __launch_bounds__(PO_THREADS) void k_crit_tail(
    const double* __restrict__ L, int ncol, long long ld, long long nch, int cap,
    const double* __restrict__ stats, const double* __restrict__ lsel,
    colred_out part, const double* __restrict__ tx, const int* __restrict__ trow,
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
    const auto below = colred_fold<k_crit_split>(part, nch, ncol, c);
    const double an = below.d[0], bn = below.d[1];
    pareto_k[c] = kpar;
    n_tail[c] = n;
    elpd[c] = (lmin + emax) + (log(bn * exp(-emax) + b) - log(an + a));
  }
}

}  // namespace

extern "C" int nh_pointwise_lnl(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                                const double* conv, const double* flux, const double* elo,
                                const double* ehi, const int* ul, const double* cl, double* L,
                                long long ldL, double* total, long long* nbad) {
  NH_REQUIRE(ctx && x && conv && flux && elo && ehi && ul && cl && L && nbad, "null argument");
  NH_REQUIRE_MATRIX(M, nE, ld, NH_ROWS_INT);
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
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_INT);
  const colred_grid g = colred_plan(M, ncol);
  NH_REQUIRE_PLAN(g);
  const long long nch = g.nch;
  // scratch: pd [nch][3][ncol] | pq [nch][2][ncol]
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)nch * ncol * 5 * 8, &base);
  if (rc) return rc;
  double* pd = (double*)base;
  double* pq = pd + (size_t)nch * 3 * ncol;
  const colred_out sums = colred_dense<k_crit_sum>(pd), sq = colred_dense<k_crit_sq>(pq);
  hipStream_t s = ctx->stream;
  if ((rc = colred_launch<k_crit_sum>(s, g, sums, L, ld))) return rc;
  hipLaunchKernelGGL(k_crit_mean, dim3(g.col_blocks()), dim3(PO_THREADS), 0, s, nch, ncol, M, stats,
                     sums);
  NH_CHECK_HIP(hipGetLastError());
  if ((rc = colred_launch<k_crit_sq>(s, g, sq, L, ld, stats, ncol))) return rc;
  hipLaunchKernelGGL(k_crit_fin, dim3(g.col_blocks()), dim3(PO_THREADS), 0, s, nch, ncol, M, stats, sq);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_psis_columns(nh_ctx* ctx, const double* L, long long M, int ncol, long long ld,
                               int Mt, const double* stats, const double* lsel, double* pareto_k,
                               long long* n_tail, double* elpd) {
  NH_REQUIRE(ctx && L && stats && lsel && pareto_k && n_tail && elpd, "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_INT);
  NH_REQUIRE(Mt >= 0 && Mt < M, "Mt outside [0, M)");
  NH_REQUIRE(Mt <= NH_PSIS_MAX_TAIL, "Mt > NH_PSIS_MAX_TAIL: thin the chain");
  const int cap = std::max(Mt, 1);
  const colred_grid g = colred_plan(M, ncol);
  NH_REQUIRE_PLAN(g);
  const long long nch = g.nch;
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
  const colred_out below = colred_dense<k_crit_split>(part);
  if ((rc = colred_launch<k_crit_split>(s, g, below, L, ld, stats, lsel, ncol, cap, tx, trow, cnt)))
    return rc;
  hipLaunchKernelGGL(k_crit_tail, dim3((unsigned)ncol), dim3(PO_THREADS), 0, s, L, ncol, ld, nch, cap,
                     stats, lsel, below, tx, trow, cnt, pareto_k, n_tail, elpd);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
