// nh_autocorr.hip -- the walker-averaged normalised autocorrelation function of one dimension of a
// chain: what emcee.autocorr.integrated_time computes per dimension (function_1d of every walker's
// series, averaged over walkers) before its window search, which stays on the host.
//
//   nh_autocorr_prep  centres walker w's series of dimension d, z[w][t] = x[t][w*n_d+d] - mean_t,
//                     into a device matrix contiguous in t, and writes s2[w] = sum_t z[w][t]^2.
//                     Three launches: per (walker tile, row chunk) sums and extremes; the centred
//                     tile written through an LDS transpose with its partial sums of squares; the
//                     sums of squares reduced.  A series whose values are all equal gets z = 0 and
//                     s2 = 0 exactly, so that the host sees it as emcee's 0/0.
//   nh_autocorr_lags  f[k] = (1/n_w) sum_w (sum_{t < n_t-tau} z[w][t] z[w][t+tau]) / s2[w] for
//                     tau = lag0 + k.  A workgroup takes 256 consecutive lags (one per lane), a
//                     group of walkers and a chunk of t; it stages z[t0 .. t0+512) and
//                     z[t0+tau0 .. t0+tau0+768) in LDS, so that z[t] is a broadcast and z[t+tau] is
//                     lane-consecutive, and writes one partial per lag.  A second launch sums the
//                     partials in a fixed order.
//
//   nh_acf_accumulate, nh_acf_finalize  the same function of a chain block that GROWS in HBM, from
//                     running lag sums (see "the running accumulator" below): a check every few
//                     steps of a run costs the new rows only, and nothing leaves the device.
//
// No floating-point atomics: every sum has an order fixed by the shapes alone (not by the device),
// so repeated calls, and ranks that hold the same chain, give bit-identical results.  Indices into
// the chain and the series are 64-bit.  Every launch is on the context's stream.
#include "nh_common.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int AC_THREADS = 256;
constexpr int AC_W = 64;                      // walkers per prep workgroup (one per lane)
constexpr int AC_R = AC_THREADS / AC_W;       // rows handled at once by a prep workgroup
constexpr int AC_LAGS = 256;                  // lags per lag workgroup (one per lane)
constexpr int AC_TT = 512;                    // values of t per LDS stage of the lag kernel
constexpr int AC_TARGET_WG = 2048;            // workgroups a launch aims for (a few per CU)

// per (row chunk c, walker w): part[(c*3 + 0|1|2)*n_w + w] = sum, min, max of x over the chunk
__global__ __launch_bounds__(AC_THREADS) void k_ac_sum(const double* __restrict__ x, long long n_t,
                                                       int n_w, int n_d, int d, long long rows,
                                                       double* __restrict__ part) {
  __shared__ double red[3][AC_R][AC_W];
  int tx = threadIdx.x % AC_W, ty = threadIdx.x / AC_W;
  int w = blockIdx.x * AC_W + tx;
  int c = blockIdx.y;
  long long ld = (long long)n_w * n_d;
  long long t0 = c * rows, t1 = min(n_t, t0 + rows);
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  if (w < n_w) {
    const double* col = x + (long long)w * n_d + d;
    for (long long t = t0 + ty; t < t1; t += AC_R) {
      double v = col[t * ld];
      s += v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
  }
  red[0][ty][tx] = s;
  red[1][ty][tx] = lo;
  red[2][ty][tx] = hi;
  __syncthreads();
  if (ty == 0 && w < n_w) {
    part[(c * 3 + 0) * (long long)n_w + w] = (red[0][0][tx] + red[0][1][tx]) +
                                             (red[0][2][tx] + red[0][3][tx]);
    part[(c * 3 + 1) * (long long)n_w + w] = fmin(fmin(red[1][0][tx], red[1][1][tx]),
                                                  fmin(red[1][2][tx], red[1][3][tx]));
    part[(c * 3 + 2) * (long long)n_w + w] = fmax(fmax(red[2][0][tx], red[2][1][tx]),
                                                  fmax(red[2][2][tx], red[2][3][tx]));
  }
}

// z[w][t] = x[t][w*n_d+d] - mean_w over the chunk's rows (0 for a series whose values are all
// equal), through a 64 x 64 LDS transpose; q[c*n_w + w] = the chunk's sum of z^2
__global__ __launch_bounds__(AC_THREADS) void k_ac_center(const double* __restrict__ x, long long n_t,
                                                          int n_w, int n_d, int d, long long rows,
                                                          int nch, const double* __restrict__ part,
                                                          double* __restrict__ z,
                                                          double* __restrict__ q) {
  __shared__ double tile[AC_W][AC_W + 1];  // [t][w], padded: the column reads are conflict-free
  __shared__ double mean[AC_W];
  __shared__ int flat[AC_W];
  __shared__ double red[AC_R][AC_W];
  int tx = threadIdx.x % AC_W, ty = threadIdx.x / AC_W;
  int w0 = blockIdx.x * AC_W;
  int w = w0 + tx;
  int c = blockIdx.y;
  long long ld = (long long)n_w * n_d;
  if (ty == 0 && w < n_w) {
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < nch; ++k) {  // (the chunks in order: every workgroup gets the same mean)
      s += part[(k * 3 + 0) * (long long)n_w + w];
      lo = fmin(lo, part[(k * 3 + 1) * (long long)n_w + w]);
      hi = fmax(hi, part[(k * 3 + 2) * (long long)n_w + w]);
    }
    flat[tx] = lo == hi;
    mean[tx] = s / (double)n_t;
  }
  __syncthreads();
  long long t0 = c * rows, t1 = min(n_t, t0 + rows);
  double acc = 0.0;
  const double* col = x + (long long)(w < n_w ? w : 0) * n_d + d;
  for (long long tb = t0; tb < t1; tb += AC_W) {
    for (int i = ty; i < AC_W; i += AC_R) {
      long long t = tb + i;
      double y = 0.0;
      if (w < n_w && t < t1) {
        y = flat[tx] ? 0.0 : col[t * ld] - mean[tx];
        acc += y * y;
      }
      tile[i][tx] = y;
    }
    __syncthreads();
    for (int j = ty; j < AC_W; j += AC_R) {
      long long t = tb + tx;
      if (w0 + j < n_w && t < t1) z[(long long)(w0 + j) * n_t + t] = tile[tx][j];
    }
    __syncthreads();
  }
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && w < n_w)
    q[(long long)c * n_w + w] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

__global__ void k_ac_s2(const double* __restrict__ q, int nch, int n_w, double* __restrict__ s2) {
  int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_w) return;
  double s = 0.0;
  for (int k = 0; k < nch; ++k) s += q[(long long)k * n_w + w];
  s2[w] = s;
}

// part[p][b*256 + k] = sum over the walkers of group g and the t of chunk c (p = g*nch + c) of
// z[w][t] z[w][t+tau] / s2[w], tau = lag0 + b*256 + k
__global__ __launch_bounds__(AC_THREADS) void k_ac_lags(const double* __restrict__ z,
                                                        const double* __restrict__ s2, long long n_t,
                                                        int n_w, long long lag0, int nlags, int wpg,
                                                        long long tlen, int nch,
                                                        double* __restrict__ part, long long ldp) {
  __shared__ double A[AC_TT];            // z[t0 + i]           (0 past the chunk)
  __shared__ double B[AC_TT + AC_LAGS];  // z[t0 + tau0 + j]    (0 past the series)
  int k = threadIdx.x;
  int b = blockIdx.x;
  int p = blockIdx.y;
  int g = p / nch, c = p % nch;
  long long tau0 = lag0 + (long long)b * AC_LAGS;
  long long t_begin = (long long)c * tlen, t_end = min(n_t, t_begin + tlen);
  long long t_stop = min(t_end, n_t - tau0);  // no later t meets a partner inside the series
  int w_begin = g * wpg, w_end = min(n_w, w_begin + wpg);
  double total = 0.0;
  for (int w = w_begin; w < w_end; ++w) {
    const double* zw = z + (long long)w * n_t;
    double acc = 0.0;
    for (long long t0 = t_begin; t0 < t_stop; t0 += AC_TT) {
      for (int i = k; i < AC_TT; i += AC_THREADS) {
        long long t = t0 + i;
        A[i] = t < t_end ? zw[t] : 0.0;
      }
      for (int j = k; j < AC_TT + AC_LAGS; j += AC_THREADS) {
        long long t = t0 + tau0 + j;
        B[j] = t < n_t ? zw[t] : 0.0;
      }
      __syncthreads();
      // four chains of FMAs (latency), summed in a fixed order
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
      for (int i = 0; i < AC_TT; i += 4) {
        a0 = fma(A[i + 0], B[i + 0 + k], a0);
        a1 = fma(A[i + 1], B[i + 1 + k], a1);
        a2 = fma(A[i + 2], B[i + 2 + k], a2);
        a3 = fma(A[i + 3], B[i + 3 + k], a3);
      }
      acc += (a0 + a1) + (a2 + a3);
      __syncthreads();
    }
    total += acc / s2[w];
  }
  int kk = b * AC_LAGS + k;
  if (kk < nlags) part[(long long)p * ldp + kk] = total;
}

__global__ void k_ac_reduce(const double* __restrict__ part, int nparts, long long ldp, int nlags,
                            int n_w, double* __restrict__ f) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nlags) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += part[(long long)p * ldp + k];
  f[k] = s / (double)n_w;
}

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// ---- the running accumulator -------------------------------------------------------------------
// Over the rows [row_start, n) of a chain block x[row][col] (col = w*n_d + d: a row is contiguous
// over the series), with y = x - pivot[col], pivot = the series' first value, the state holds
//   S[col][k] = sum_{t >= row_start + k} y[t] y[t-k], k < L     T[col] = sum y[t]     min, max of y
// Every one of these is ONE accumulator chain in the order of t, so the state after rows [a, b) is
// the same bit for bit however [a, b) was cut into calls (padding terms are fma(0, y, acc) or
// fma(y, 0, acc) on a finite y: they leave acc as it is).  A workgroup takes ACF_CT adjacent
// series and 256 lags (one per lane): it stages the ACF_TT new rows and the 255 + ACF_TT rows
// behind them, 64 contiguous bytes per row, into LDS transposed to [series][t]; y[t] is then a
// broadcast and y[t-k] lane-consecutive, and a lane carries ACF_CT independent chains.
constexpr int ACF_CT = 8;                       // adjacent series per workgroup (64 B of a row)
constexpr int ACF_TT = 128;                     // new rows per LDS stage
constexpr int ACF_AS = ACF_TT + 2;              // row strides = 2 mod 16 doubles: the transposed
constexpr int ACF_BT = ACF_TT + AC_LAGS;        //   stores of 16 lanes fall on 16 banks
constexpr int ACF_BS = ACF_BT + 2;
constexpr int ACF_HS = AC_LAGS + 2;
static_assert(AC_THREADS == AC_LAGS && AC_THREADS % ACF_CT == 0, "a thread loads one series");

__global__ void k_acf_pivot(const double* __restrict__ x, long long ld, long long row_start,
                            double* __restrict__ pivot) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < ld) pivot[c] = x[row_start * ld + c];
}

// adds rows [n0, n1) to S and stats = {T, min, max}[ld]; n0 == row_start: the state starts here
// (nothing of it is read).  grid (series tiles, lag blocks)
__global__ __launch_bounds__(AC_THREADS) void k_acf_accumulate(
    const double* __restrict__ x, long long ld, long long row_start, long long n0, long long n1,
    int L, const double* __restrict__ pivot, double* __restrict__ S, double* __restrict__ stats) {
  __shared__ double As[ACF_CT][ACF_AS];  // y[t0 + i]                  (0 from n1 on)
  __shared__ double Bs[ACF_CT][ACF_BS];  // y[t0 - k0 - 255 + j]       (0 before row_start)
  const int kl = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * ACF_CT;
  const long long k0 = (long long)blockIdx.y * AC_LAGS;
  const long long k = k0 + kl;
  const bool fresh = n0 == row_start;
  // no earlier t has a partner t - k >= row_start for any lag of this workgroup
  const long long tb = max(n0, row_start + k0);
  if (tb >= n1 && !fresh) return;
  double acc[ACF_CT];
#pragma unroll
  for (int c = 0; c < ACF_CT; ++c)
    acc[c] = (!fresh && k < L && c0 + c < ld) ? S[(c0 + c) * L + k] : 0.0;
  const int lc = kl % ACF_CT;  // the series this thread loads
  const bool col_ok = c0 + lc < ld;
  const double* xc = x + c0 + lc;
  const double pv = col_ok ? pivot[c0 + lc] : 0.0;
  const bool stat = blockIdx.y == 0 && kl < ACF_CT && col_ok;  // (kl == lc there)
  double T = 0.0, lo = INFINITY, hi = -INFINITY;
  if (stat && !fresh) {
    T = stats[c0 + kl];
    lo = stats[ld + c0 + kl];
    hi = stats[2 * ld + c0 + kl];
  }
  for (long long t0 = tb; t0 < n1; t0 += ACF_TT) {
    for (int idx = kl; idx < ACF_TT * ACF_CT; idx += AC_THREADS) {
      int i = idx / ACF_CT;
      long long t = t0 + i;
      As[lc][i] = (col_ok && t < n1) ? xc[t * ld] - pv : 0.0;
    }
    for (int idx = kl; idx < ACF_BT * ACF_CT; idx += AC_THREADS) {
      int j = idx / ACF_CT;
      long long t = t0 - k0 - (AC_LAGS - 1) + j;
      Bs[lc][j] = (col_ok && t >= row_start && t < n1) ? xc[t * ld] - pv : 0.0;
    }
    __syncthreads();
    if (stat) {
      int m = (int)min((long long)ACF_TT, n1 - t0);
      for (int i = 0; i < m; ++i) {
        double v = As[kl][i];
        T += v;
        lo = fmin(lo, v);
        hi = fmax(hi, v);
      }
    }
    const double* b = &Bs[0][AC_LAGS - 1 - kl];
#pragma unroll 4
    for (int i = 0; i < ACF_TT; ++i) {
#pragma unroll
      for (int c = 0; c < ACF_CT; ++c) acc[c] = fma(As[c][i], b[c * ACF_BS + i], acc[c]);
    }
    __syncthreads();
  }
  if (k < L) {
#pragma unroll
    for (int c = 0; c < ACF_CT; ++c)
      if (c0 + c < ld) S[(c0 + c) * L + k] = acc[c];
  }
  if (stat) {
    stats[c0 + kl] = T;
    stats[ld + c0 + kl] = lo;
    stats[2 * ld + c0 + kl] = hi;
  }
}

// c_k = sum_{t >= k} (y[t] - m)(y[t-k] - m) = S_k - m ((T - P_k) + (T - Q_k)) + (n - k) m^2, with
// P_k / Q_k the sums of the first / last k values of y (one sequence of operations for every k,
// so that c_k / c_0 is exactly 1 at k = 0)
__device__ inline double acf_ck(double S, double T, double m, double P, double Q, double nk) {
  double u = (T - P) + (T - Q);
  return fma(nk * m, m, fma(-m, u, S));
}

// R[col][k] = c_k / c_0 of series col for k < Lc (NaN throughout for a series that is constant or
// holds a non-finite value); nn = n - row_start values per series.  grid (series tiles)
__global__ __launch_bounds__(AC_THREADS) void k_acf_ratio(
    const double* __restrict__ x, long long ld, long long row_start, long long nn, int L, int Lc,
    const double* __restrict__ pivot, const double* __restrict__ S,
    const double* __restrict__ stats, double* __restrict__ R) {
  __shared__ double Ps[ACF_CT][ACF_HS];  // the first values of y, then their exclusive prefix sums
  __shared__ double Qs[ACF_CT][ACF_HS];  // the last values, backwards, likewise
  __shared__ double sT[ACF_CT], sm[ACF_CT], sc0[ACF_CT];
  const int tid = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * ACF_CT;
  const int lc = tid % ACF_CT;
  const bool col_ok = c0 + lc < ld;
  const double* xc = x + c0 + lc;
  const double pv = col_ok ? pivot[c0 + lc] : 0.0;
  if (tid < ACF_CT) {
    double T = 0.0, m = 0.0, c0v = NAN;
    if (col_ok) {  // (tid == lc)
      T = stats[c0 + tid];
      double lo = stats[ld + c0 + tid], hi = stats[2 * ld + c0 + tid];
      m = T / (double)nn;
      double v = acf_ck(S[(c0 + tid) * L], T, m, 0.0, 0.0, (double)nn);
      if (isfinite(T) && lo < hi && isfinite(v) && v > 0.0) c0v = v;
    }
    sT[tid] = T;
    sm[tid] = m;
    sc0[tid] = c0v;
  }
  double carry = 0.0;  // of the scan this thread makes (tid < 2 * ACF_CT)
  for (long long kt = 0; kt < Lc; kt += AC_LAGS) {
    for (int idx = tid; idx < AC_LAGS * ACF_CT; idx += AC_THREADS) {
      int j = idx / ACF_CT;
      long long kk = kt + j;
      bool ok = col_ok && kk < nn;
      Ps[lc][j] = ok ? xc[(row_start + kk) * ld] - pv : 0.0;
      Qs[lc][j] = ok ? xc[(row_start + nn - 1 - kk) * ld] - pv : 0.0;
    }
    __syncthreads();
    if (tid < 2 * ACF_CT) {
      double* a = tid < ACF_CT ? Ps[tid] : Qs[tid - ACF_CT];
      for (int j = 0; j < AC_LAGS; ++j) {
        double v = a[j];
        a[j] = carry;
        carry += v;
      }
    }
    __syncthreads();
    long long kk = kt + tid;
    if (kk < Lc) {
      for (int c = 0; c < ACF_CT; ++c) {
        if (c0 + c >= ld) break;
        double ck = acf_ck(S[(c0 + c) * L + kk], sT[c], sm[c], Ps[c][tid], Qs[c][tid],
                           (double)(nn - kk));
        R[(c0 + c) * L + kk] = ck / sc0[c];
      }
    }
    __syncthreads();
  }
}

// f[d][k] = the mean over the walkers, in their order, of R[w*n_d + d][k]; NaN for k >= Lc
__global__ void k_acf_mean(const double* __restrict__ R, int n_w, int n_d, int L, int Lc,
                           double* __restrict__ f) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  int d = blockIdx.y;
  if (k >= L) return;
  double s = NAN;
  if (k < Lc) {
    s = 0.0;
    for (int w = 0; w < n_w; ++w) s += R[((long long)w * n_d + d) * L + k];
    s /= (double)n_w;
  }
  f[(long long)d * L + k] = s;
}

}  // namespace

extern "C" int nh_autocorr_prep(nh_ctx* ctx, const double* x, long long n_t, int n_w, int n_d,
                                int d, double* z, double* s2) {
  NH_REQUIRE(ctx && x && z && s2, "null argument");
  NH_REQUIRE(n_t > 0, "n_t == 0: an empty chain");
  NH_REQUIRE(n_w > 0, "n_w must be positive");
  NH_REQUIRE(n_d > 0, "n_d must be positive");
  NH_REQUIRE(d >= 0 && d < n_d, "d outside [0, n_d)");
  // row chunks: enough workgroups to fill the chip, >= 256 rows each (a multiple of the tile)
  long long ntile = cdiv(n_w, AC_W);
  long long want = std::max<long long>(1, AC_TARGET_WG / ntile);
  long long nch = std::min(want, cdiv(n_t, 256));
  long long rows = cdiv(cdiv(n_t, nch), AC_W) * AC_W;
  nch = cdiv(n_t, rows);
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)nch * n_w * 4 * sizeof(double), &base);
  if (rc) return rc;
  double* part = (double*)base;                 // [nch][3][n_w]
  double* q = part + (size_t)nch * 3 * n_w;     // [nch][n_w]
  hipStream_t s = ctx->stream;
  dim3 grid((unsigned)ntile, (unsigned)nch);
  hipLaunchKernelGGL(k_ac_sum, grid, dim3(AC_THREADS), 0, s, x, n_t, n_w, n_d, d, rows, part);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_ac_center, grid, dim3(AC_THREADS), 0, s, x, n_t, n_w, n_d, d, rows,
                     (int)nch, part, z, q);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_ac_s2, dim3((unsigned)cdiv(n_w, AC_THREADS)), dim3(AC_THREADS), 0, s, q,
                     (int)nch, n_w, s2);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_autocorr_lags(nh_ctx* ctx, const double* z, const double* s2, long long n_t,
                                int n_w, long long lag0, int nlags, double* f) {
  NH_REQUIRE(ctx && z && s2 && f, "null argument");
  NH_REQUIRE(n_t > 0, "n_t == 0: an empty chain");
  NH_REQUIRE(n_w > 0, "n_w must be positive");
  NH_REQUIRE(nlags > 0, "nlags must be positive");
  NH_REQUIRE(lag0 >= 0 && lag0 + nlags <= n_t, "lags outside [0, n_t)");
  // lag blocks x parts (walker groups x t chunks): about AC_TARGET_WG workgroups, a function of
  // the shapes only so that the order of every sum is too
  long long nlb = cdiv(nlags, AC_LAGS);
  long long want = std::max<long long>(1, cdiv(AC_TARGET_WG, nlb));
  long long ngroups = std::min<long long>(n_w, want);
  long long wpg = cdiv(n_w, ngroups);
  ngroups = cdiv(n_w, wpg);
  long long nch = std::min(std::max<long long>(1, want / ngroups), cdiv(n_t, AC_TT));
  long long tlen = cdiv(cdiv(n_t, nch), AC_TT) * AC_TT;
  nch = cdiv(n_t, tlen);
  long long nparts = ngroups * nch;
  long long ldp = nlb * AC_LAGS;
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)(nparts * ldp) * sizeof(double), &base);
  if (rc) return rc;
  double* part = (double*)base;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_ac_lags, dim3((unsigned)nlb, (unsigned)nparts), dim3(AC_THREADS), 0, s, z,
                     s2, n_t, n_w, lag0, nlags, (int)wpg, tlen, (int)nch, part, ldp);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_ac_reduce, dim3((unsigned)cdiv(nlags, AC_THREADS)), dim3(AC_THREADS), 0, s,
                     part, (int)nparts, ldp, nlags, n_w, f);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_acf_accumulate(nh_ctx* ctx, const double* x, long long rows, int n_w, int n_d,
                                 long long row_start, long long n0, long long n1, int L,
                                 double* pivot, double* S, double* stats) {
  NH_REQUIRE(ctx && x && pivot && S && stats, "null argument");
  NH_REQUIRE(n_w > 0, "n_w must be positive");
  NH_REQUIRE(n_d > 0, "n_d must be positive");
  NH_REQUIRE(L > 0, "L must be positive");
  NH_REQUIRE(0 <= row_start && row_start <= n0 && n0 <= n1 && n1 <= rows,
             "need 0 <= row_start <= n0 <= n1 <= rows");
  long long ld = (long long)n_w * n_d;
  long long tiles = cdiv(ld, ACF_CT), lagb = cdiv(L, AC_LAGS);
  NH_REQUIRE(tiles < (1ll << 31) && lagb <= 65535, "too many series or lags for one launch");
  if (n0 == n1) return NH_OK;
  hipStream_t s = ctx->stream;
  if (n0 == row_start) {
    hipLaunchKernelGGL(k_acf_pivot, dim3((unsigned)cdiv(ld, AC_THREADS)), dim3(AC_THREADS), 0, s, x,
                       ld, row_start, pivot);
    NH_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(k_acf_accumulate, dim3((unsigned)tiles, (unsigned)lagb), dim3(AC_THREADS), 0,
                     s, x, ld, row_start, n0, n1, L, pivot, S, stats);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_acf_finalize(nh_ctx* ctx, const double* x, long long rows, int n_w, int n_d,
                               long long row_start, long long n, int L, const double* pivot,
                               const double* S, const double* stats, double* f) {
  NH_REQUIRE(ctx && x && pivot && S && stats && f, "null argument");
  NH_REQUIRE(n_w > 0, "n_w must be positive");
  NH_REQUIRE(n_d > 0 && n_d <= 65535, "n_d outside [1, 65535]");
  NH_REQUIRE(L > 0, "L must be positive");
  NH_REQUIRE(0 <= row_start && row_start < n && n <= rows, "need 0 <= row_start < n <= rows");
  long long ld = (long long)n_w * n_d;
  long long tiles = cdiv(ld, ACF_CT);
  NH_REQUIRE(tiles < (1ll << 31), "too many series for one launch");
  long long nn = n - row_start;
  int Lc = (int)std::min<long long>(L, nn);
  void* base = nullptr;
  int rc = nh_scratch(ctx, (size_t)ld * L * sizeof(double), &base);
  if (rc) return rc;
  double* R = (double*)base;  // [ld][L]
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_acf_ratio, dim3((unsigned)tiles), dim3(AC_THREADS), 0, s, x, ld, row_start,
                     nn, L, Lc, pivot, S, stats, R);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_acf_mean, dim3((unsigned)cdiv(L, AC_THREADS), (unsigned)n_d),
                     dim3(AC_THREADS), 0, s, R, n_w, n_d, L, Lc, f);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
