// nh_evidence.hip -- what the bridge-sampling estimate of the marginal likelihood (Meng & Wong
// 1996; the "normal" method of Gronau et al. 2017) reads from a chain where it lies in HBM: the
// mean and covariance of its pooled rows, draws from the normal proposal fitted to them, that
// proposal's log-density at every pooled row, and the two sums of one iteration of the estimator.
// Pooled rows are nh_rank.hip's: row e = t * npool + j of a chain block is the d values
// x[(row0 + t) * ld + j * cstride + 0..d-1]; a plain matrix is npool = 1.  d <= NH_EVID_MAX_DIM.
//
//   nh_chain_cov     two passes in the tiling of nh_colred.h.  k_cov_sum: per (row chunk, column)
//                    the sum and whether a value is not finite; k_cov_mean adds the chunks in
//                    order.  k_cov_prod: a workgroup walks its row chunk in tiles of EV_TR centred
//                    rows in LDS; a thread owns up to EV_PPT of the d (d + 1) / 2 pairs (a >= b)
//                    and adds their products row by row; k_cov_fin adds the chunks in order,
//                    divides by S - 1 and mirrors.  A column with a non-finite value has a NaN
//                    mean, which makes its row and column of the covariance NaN; S = 1 gives 0/0.
//   nh_mvn_draw      threads are [256 / cw rows][cw columns], cw the power of two >= d.  Thread
//                    (row, c) takes Philox4x32-10 of counter (lo32(row), hi32(row), c >> 1,
//                    NH_PHILOX_MVN) under key (lo32(seed), hi32(seed)), row the GLOBAL row:
//                    U = nh_u52(r0, r1), V = nh_u52(r2, r3), z = sqrt(-2 log U) * (c odd ?
//                    sin : cos)(2 pi V) -- Box-Muller, one call serving columns 2 m and 2 m + 1;
//                    z goes to LDS, then out[row][c] = mean[c] + sum_{k <= c} L[c][k] z[k] in k
//                    order and z2[row] = sum_k z[k]^2 in k order.
//   nh_mvn_logpdf    one pooled row per thread, L in LDS (every lane reads the same word: a
//                    broadcast), forward substitution y = L^-1 (theta - mean) with the thread's
//                    y in a column of LDS of its own (no runtime-indexed registers):
//                    log N = -d/2 log 2 pi - sum log L_ii - |y|^2 / 2.
//   nh_bridge_l2     l2 = lp + z2 / 2 + d/2 log 2 pi + sum log L_ii: the log-probability over the
//                    proposal's density at a draw, from the draw's own |z|^2.
//   nh_bridge_sums   workgroups take row chunks of l2 (numerator) and of l1 (denominator), reduce
//                    through an LDS tree and write one partial each; k_bridge_fin adds each side's
//                    partials in chunk order.
//
// FP64 throughout.  No atomics: every floating-point sum has an order fixed by the shapes alone,
// so repeated calls give bit-identical results.  Every launch is on the context's stream; nothing
// synchronises with the host.
#include "nh_colred.h"
#include "nh_philox.h"

namespace {

constexpr int EV_TR = 64;  // centred rows per LDS tile of k_cov_prod
constexpr int EV_PPT = 3;  // pairs per thread: 32 * 33 / 2 = 528 <= 3 * 256
constexpr int EV_D = NH_EVID_MAX_DIM;
constexpr int EV_LP_THREADS = 128;  // nh_mvn_logpdf: d * 128 * 8 bytes of LDS hold the y of a workgroup
static_assert(EV_D * (EV_D + 1) / 2 <= EV_PPT * PO_THREADS, "pairs per thread");
static_assert(EV_D <= 64, "k_cov_mean is one wave");

__device__ __forceinline__ long long ev_src(long long e, long long row0, long long ld,
                                            long long cstride, int npool) {
  const long long t = e / npool, j = e - t * npool;
  return (row0 + t) * ld + j * cstride;
}

// -d/2 log 2 pi - sum_i log L_ii, the diagonal in order
__device__ __forceinline__ double ev_lognorm(const double* __restrict__ L, int d) {
  double s = 0.0;
  for (int i = 0; i < d; ++i) s += log(L[i * d + i]);
  return -0.5 * (double)d * 1.8378770664093453 - s;
}

// ---------------------------------------------------------------- mean and covariance
__global__ __launch_bounds__(PO_THREADS) void k_cov_sum(
    const double* __restrict__ x, long long row0, long long ld, long long cstride, int npool, int d,
    long long S, int cw, long long rows, double* __restrict__ part, int* __restrict__ bad) {
  __shared__ double rs[PO_THREADS];
  __shared__ int rb[PO_THREADS];
  const int tid = threadIdx.x, tx = tid % cw, ty = tid / cw, R = PO_THREADS / cw;
  const long long k = blockIdx.x;
  const long long e0 = k * rows, e1 = min(S, e0 + rows);
  double s = 0.0;
  int nb = 0;
  if (tx < d)
    for (long long e = e0 + ty; e < e1; e += R) {
      const double v = x[ev_src(e, row0, ld, cstride, npool) + tx];
      s += v;
      nb |= !po_finite(v);
    }
  rs[tid] = s;
  rb[tid] = nb;
  po_tree(rs, tid, ty, cw, [](double a, double b) { return a + b; });
  po_tree(rb, tid, ty, cw, [](int a, int b) { return a | b; });
  if (ty == 0 && tx < d) {
    part[k * d + tx] = rs[tid];
    bad[k * d + tx] = rb[tid];
  }
}

__global__ void k_cov_mean(const double* __restrict__ part, const int* __restrict__ bad,
                           long long nch, int d, long long S, double* __restrict__ mean) {
  const int c = threadIdx.x;
  if (c >= d) return;
  double s = 0.0;
  int nb = 0;
  for (long long k = 0; k < nch; ++k) {
    s += part[k * d + c];
    nb |= bad[k * d + c];
  }
  mean[c] = nb ? nh_nan() : s / (double)S;
}

// part[k * np + p] = the sum over the rows of chunk k of the centred product of pair p = (a, b),
// p = a (a + 1) / 2 + b, b <= a
__global__ __launch_bounds__(PO_THREADS) void k_cov_prod(
    const double* __restrict__ x, long long row0, long long ld, long long cstride, int npool, int d,
    long long S, long long rows, const double* __restrict__ mean, double* __restrict__ part) {
  __shared__ double tile[EV_TR][EV_D + 1];
  __shared__ double mu[EV_D];
  const int tid = threadIdx.x, np = d * (d + 1) / 2;
  int pa[EV_PPT], pb[EV_PPT];
  double acc[EV_PPT];
#pragma unroll
  for (int q = 0; q < EV_PPT; ++q) {
    const int p = tid + q * PO_THREADS;
    int a = 0;
    if (p < np)
      while ((a + 1) * (a + 2) / 2 <= p) ++a;
    pa[q] = a;
    pb[q] = p < np ? p - a * (a + 1) / 2 : 0;
    acc[q] = 0.0;
  }
  if (tid < d) mu[tid] = mean[tid];
  const long long k = blockIdx.x;
  const long long e0 = k * rows, e1 = min(S, e0 + rows);
  for (long long t0 = e0; t0 < e1; t0 += EV_TR) {  // (uniform over the workgroup)
    const int nr = (int)min((long long)EV_TR, e1 - t0);
    __syncthreads();  // mu is written; the tile of the trip before is read
    for (int i = tid; i < nr * d; i += PO_THREADS) {
      const int r = i / d, c = i - r * d;
      tile[r][c] = x[ev_src(t0 + r, row0, ld, cstride, npool) + c] - mu[c];
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
#pragma unroll
      for (int q = 0; q < EV_PPT; ++q) acc[q] = fma(tile[r][pa[q]], tile[r][pb[q]], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < EV_PPT; ++q) {
    const int p = tid + q * PO_THREADS;
    if (p < np) part[k * np + p] = acc[q];
  }
}

__global__ void k_cov_fin(const double* __restrict__ part, long long nch, int d, long long S,
                          double* __restrict__ cov) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d * d) return;
  const int r = i / d, c = i - r * d;
  const int a = max(r, c), b = min(r, c), np = d * (d + 1) / 2, p = a * (a + 1) / 2 + b;
  double s = 0.0;
  for (long long k = 0; k < nch; ++k) s += part[k * np + p];
  cov[i] = s / (double)(S - 1);
}

// ---------------------------------------------------------------- proposal draws
__global__ __launch_bounds__(PO_THREADS) void k_mvn_draw(
    const double* __restrict__ mean, const double* __restrict__ L, int d, int cw,
    unsigned long long seed, long long row0, long long n, double* __restrict__ out, long long ld,
    double* __restrict__ z2) {
  __shared__ double Ls[EV_D * EV_D];
  __shared__ double mu[EV_D];
  __shared__ double zs[PO_THREADS];
  const int tid = threadIdx.x, tx = tid % cw, ty = tid / cw, R = PO_THREADS / cw;
  for (int i = tid; i < d * d; i += PO_THREADS) Ls[i] = L[i];
  if (tid < d) mu[tid] = mean[tid];
  for (long long base = (long long)blockIdx.x * R; base < n; base += (long long)gridDim.x * R) {
    const long long r = base + ty;  // (base is the workgroup's: the barriers below are uniform)
    const bool live = r < n && tx < d;
    __syncthreads();  // Ls and mu are written; zs of the trip before is read
    double z = 0.0;
    if (live) {
      const unsigned long long row = (unsigned long long)(row0 + r);
      const nh_u4 w = nh_philox((unsigned)(row & 0xffffffffull), (unsigned)(row >> 32),
                                (unsigned)(tx >> 1), NH_PHILOX_MVN,
                                (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32));
      const double rad = sqrt(-2.0 * log(nh_u52(w.x, w.y)));
      double sn, cs;
      sincos(6.283185307179586 * nh_u52(w.z, w.w), &sn, &cs);
      z = rad * ((tx & 1) ? sn : cs);
    }
    zs[tid] = z;
    __syncthreads();
    if (live) {
      const double* zr = zs + ty * cw;
      double acc = mu[tx];
      for (int k = 0; k <= tx; ++k) acc = fma(Ls[tx * d + k], zr[k], acc);
      out[r * ld + tx] = acc;
      if (tx == 0) {
        double q = 0.0;
        for (int k = 0; k < d; ++k) q = fma(zr[k], zr[k], q);
        z2[r] = q;
      }
    }
  }
}

// ---------------------------------------------------------------- the proposal's log-density
// dynamic LDS (doubles): y [d][EV_LP_THREADS] (a thread's y is a column: consecutive lanes,
// consecutive words) | L [d][d] | mean [d] | the normalisation
__global__ __launch_bounds__(EV_LP_THREADS) void k_mvn_logpdf(
    const double* __restrict__ x, long long row0, long long ld, long long cstride, int npool, int d,
    long long S, const double* __restrict__ mean, const double* __restrict__ L,
    const double* __restrict__ lp, double* __restrict__ out) {
  extern __shared__ double ev_lds[];
  double* ys = ev_lds;
  double* Ls = ys + d * EV_LP_THREADS;
  double* mu = Ls + d * d;
  double* lognorm = mu + d;
  const int tid = threadIdx.x;
  for (int i = tid; i < d * d; i += EV_LP_THREADS) Ls[i] = L[i];
  if (tid < d) mu[tid] = mean[tid];
  if (tid == 0) *lognorm = ev_lognorm(L, d);
  __syncthreads();
  double* y = ys + tid;
  for (long long e = (long long)blockIdx.x * EV_LP_THREADS + tid; e < S;
       e += (long long)gridDim.x * EV_LP_THREADS) {
    const double* xr = x + ev_src(e, row0, ld, cstride, npool);
    double q = 0.0;
    bool bad = false;
    for (int i = 0; i < d; ++i) {
      const double v = xr[i];
      bad |= !po_finite(v);
      double acc = v - mu[i];
      for (int k = 0; k < i; ++k) acc = fma(-Ls[i * d + k], y[k * EV_LP_THREADS], acc);
      const double yi = acc / Ls[i * d + i];
      y[i * EV_LP_THREADS] = yi;
      q = fma(yi, yi, q);
    }
    const double lg = *lognorm - 0.5 * q;
    out[e] = bad ? nh_nan() : (lp ? lp[e] - lg : lg);
  }
}

__global__ __launch_bounds__(PO_THREADS) void k_bridge_l2(const double* __restrict__ lp,
                                                          const double* __restrict__ z2, long long n,
                                                          const double* __restrict__ L, int d,
                                                          double* __restrict__ out) {
  __shared__ double lognorm;
  if (threadIdx.x == 0) lognorm = ev_lognorm(L, d);
  __syncthreads();
  for (long long i = (long long)blockIdx.x * PO_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * PO_THREADS)
    out[i] = lp[i] - (lognorm - 0.5 * z2[i]);
}

// ---------------------------------------------------------------- one iteration's sums
// with x = l - lstar: f(x) = e^x / (s1 e^x + s2 r) over l2 (workgroups [0, nch2)) and
// g(x) = 1 / (s1 e^x + s2 r) over l1 (the workgroups behind them); for x > 0 both through e^-x,
// so nothing overflows; x = -inf gives f = 0 exactly
__global__ __launch_bounds__(PO_THREADS) void k_bridge_part(
    const double* __restrict__ l1, long long N1, const double* __restrict__ l2, long long N2,
    double lstar, double s1, double s2r, long long rows1, long long rows2, long long nch2,
    double* __restrict__ part, double* __restrict__ f1, double* __restrict__ f2) {
  __shared__ double rs[PO_THREADS];
  const int tid = threadIdx.x;
  const bool num = (long long)blockIdx.x < nch2;
  const long long k = num ? (long long)blockIdx.x : (long long)blockIdx.x - nch2;
  const double* l = num ? l2 : l1;
  double* dst = num ? f1 : f2;
  const long long N = num ? N2 : N1, rows = num ? rows2 : rows1;
  const long long i0 = k * rows, i1 = min(N, i0 + rows);
  double s = 0.0;
  for (long long i = i0 + tid; i < i1; i += PO_THREADS) {
    const double xv = l[i] - lstar;
    double v;
    if (xv > 0.0) {
      const double em = exp(-xv), den = s1 + s2r * em;
      v = num ? 1.0 / den : em / den;
    } else {  // (a NaN comes here and stays one)
      const double ex = exp(xv), den = s1 * ex + s2r;
      v = num ? ex / den : 1.0 / den;
    }
    if (dst) dst[i] = v;
    s += v;
  }
  rs[tid] = s;
  po_tree(rs, tid, tid, 1, [](double a, double b) { return a + b; });
  if (tid == 0) part[blockIdx.x] = rs[0];
}

__global__ void k_bridge_fin(const double* __restrict__ part, long long nch1, long long nch2,
                             double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t > 1) return;
  const long long k0 = t == 0 ? 0 : nch2, k1 = t == 0 ? nch2 : nch2 + nch1;
  double s = 0.0;
  for (long long k = k0; k < k1; ++k) s += part[k];
  out[t] = s;
}

int ev_check_pool(const char* fn, long long row0, long long nrows, long long ld, long long cstride,
                  int npool, int d) {
  if (row0 < 0 || nrows < 1 || npool < 1 || d < 1)
    return nh_set_error(NH_EINVAL, "%s: row0 < 0, or nrows, npool or d not positive", fn);
  if (d > NH_EVID_MAX_DIM)
    return nh_set_error(NH_EINVAL, "%s: d > NH_EVID_MAX_DIM", fn);
  if (npool > 1 && cstride < d)
    return nh_set_error(NH_EINVAL, "%s: cstride < d: pooled rows would overlap", fn);
  if (cstride < 0 || (long long)(npool - 1) * cstride + d > ld)
    return nh_set_error(NH_EINVAL, "%s: (npool - 1) * cstride + d > ld", fn);
  if (nrows >= (1ll << 31) / npool)
    return nh_set_error(NH_EINVAL, "%s: nrows * npool >= 2^31 pooled rows", fn);
  return NH_OK;
}

unsigned ev_grid(long long n, long long per) {
  return (unsigned)std::min<long long>(cdiv(n, per), PO_TARGET_WG);
}

}  // namespace

extern "C" int nh_chain_cov(nh_ctx* ctx, const double* x, long long row0, long long nrows,
                            long long ld, long long cstride, int npool, int d, double* mean,
                            double* cov) {
  NH_REQUIRE(ctx && x && mean && cov, "null argument");
  int rc = ev_check_pool(__func__, row0, nrows, ld, cstride, npool, d);
  if (rc) return rc;
  const long long S = nrows * npool;
  const int cw = po_pow2_at_least(d, EV_D), np = d * (d + 1) / 2;
  long long rows1, nch1, rows2, nch2;
  po_chunks(S, 1, PO_THREADS / cw, &rows1, &nch1);
  po_chunks(S, 1, EV_TR, &rows2, &nch2);
  // scratch: part1 [nch1][d] | part2 [nch2][np] | bad (int) [nch1][d]
  void* base = nullptr;
  rc = nh_scratch(ctx, ((size_t)nch1 * d + (size_t)nch2 * np) * 8 + (size_t)nch1 * d * 4, &base);
  if (rc) return rc;
  double* part1 = (double*)base;
  double* part2 = part1 + nch1 * d;
  int* bad = (int*)(part2 + nch2 * np);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_cov_sum, dim3((unsigned)nch1), dim3(PO_THREADS), 0, s, x, row0, ld, cstride,
                     npool, d, S, cw, rows1, part1, bad);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cov_mean, dim3(1), dim3(64), 0, s, part1, bad, nch1, d, S, mean);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cov_prod, dim3((unsigned)nch2), dim3(PO_THREADS), 0, s, x, row0, ld, cstride,
                     npool, d, S, rows2, mean, part2);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cov_fin, dim3((unsigned)cdiv(d * d, PO_THREADS)), dim3(PO_THREADS), 0, s,
                     part2, nch2, d, S, cov);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_mvn_draw(nh_ctx* ctx, const double* mean, const double* L, int d,
                           unsigned long long seed, long long row0, long long n, double* out,
                           long long ld, double* z2) {
  NH_REQUIRE(ctx && mean && L && out && z2, "null argument");
  NH_REQUIRE(d >= 1 && d <= NH_EVID_MAX_DIM, "d outside [1, NH_EVID_MAX_DIM]");
  NH_REQUIRE(n > 0 && n < (1ll << 31), "n outside [1, 2^31)");
  NH_REQUIRE(row0 >= 0, "row0 < 0");
  NH_REQUIRE(ld >= d, "d > ld");
  const int cw = po_pow2_at_least(d, EV_D);
  hipLaunchKernelGGL(k_mvn_draw, dim3(ev_grid(n, PO_THREADS / cw)), dim3(PO_THREADS), 0,
                     ctx->stream, mean, L, d, cw, seed, row0, n, out, ld, z2);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_mvn_logpdf(nh_ctx* ctx, const double* x, long long row0, long long nrows,
                             long long ld, long long cstride, int npool, int d, const double* mean,
                             const double* L, const double* lp, double* out) {
  NH_REQUIRE(ctx && x && mean && L && out, "null argument");
  int rc = ev_check_pool(__func__, row0, nrows, ld, cstride, npool, d);
  if (rc) return rc;
  const long long S = nrows * npool;
  const size_t lds = ((size_t)d * EV_LP_THREADS + (size_t)d * d + d + 1) * 8;  // <= 40 KiB
  hipLaunchKernelGGL(k_mvn_logpdf, dim3(ev_grid(S, EV_LP_THREADS)), dim3(EV_LP_THREADS), lds,
                     ctx->stream, x, row0, ld, cstride, npool, d, S, mean, L, lp, out);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_bridge_l2(nh_ctx* ctx, const double* lp, const double* z2, long long n,
                            const double* L, int d, double* out) {
  NH_REQUIRE(ctx && lp && z2 && L && out, "null argument");
  NH_REQUIRE(d >= 1 && d <= NH_EVID_MAX_DIM, "d outside [1, NH_EVID_MAX_DIM]");
  NH_REQUIRE(n > 0 && n < (1ll << 31), "n outside [1, 2^31)");
  hipLaunchKernelGGL(k_bridge_l2, dim3(ev_grid(n, PO_THREADS)), dim3(PO_THREADS), 0, ctx->stream,
                     lp, z2, n, L, d, out);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_bridge_sums(nh_ctx* ctx, const double* l1, long long N1, const double* l2,
                              long long N2, double lstar, double s1, double s2, double r,
                              double* out, double* f1, double* f2) {
  NH_REQUIRE(ctx && l1 && l2 && out, "null argument");
  NH_REQUIRE(N1 > 0 && N1 < (1ll << 31) && N2 > 0 && N2 < (1ll << 31), "N1 or N2 outside [1, 2^31)");
  long long rows1, nch1, rows2, nch2;
  po_chunks(N1, 2, PO_THREADS, &rows1, &nch1);
  po_chunks(N2, 2, PO_THREADS, &rows2, &nch2);
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)(nch1 + nch2) * 8, &base);
  if (rc) return rc;
  double* part = (double*)base;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_bridge_part, dim3((unsigned)(nch1 + nch2)), dim3(PO_THREADS), 0, s, l1, N1,
                     l2, N2, lstar, s1, s2 * r, rows1, rows2, nch2, part, f1, f2);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_bridge_fin, dim3(1), dim3(64), 0, s, part, nch1, nch2, out);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
