// nh_gpd.h -- the tail step of Pareto-smoothed importance sampling that nh_infocrit.hip
// (nh_psis_columns) and nh_reweight.hip (nh_psis_weights) share: one workgroup of PO_THREADS
// threads loads a column's list of tail rows into LDS, sorts it by (value, row index) (a bitonic
// network), fits the generalised Pareto distribution of Zhang & Stephens 2009 with the loo
// package's weak priors (a wave per candidate b_j, lanes over the tail, butterfly sums) and
// replaces the tail by the fitted quantiles.  Every sum has an order fixed by the sorted values.
#pragma once
#include "nh_colred.h"

#include <cfloat>

namespace {

constexpr int CRIT_TAIL_MAX = NH_PSIS_MAX_TAIL;      // tail entries a workgroup's LDS is sized for
constexpr int CRIT_MAX_CAND = 96;                    // 30 + floor(sqrt(4096)) = 94 candidates b_j
constexpr double CRIT_LOG_TINY = -708.3964185322641; // log(DBL_MIN)

__device__ __forceinline__ double crit_wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// an order-preserving 64-bit key of a double that is not NaN, and back (nh_select.hip)
__device__ __forceinline__ unsigned long long crit_key(double v) {
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double crit_value(unsigned long long k) {
  unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// the sum / the maximum of one value per thread, the same in every thread (a fixed tree)
template <typename F>
__device__ __forceinline__ double crit_block_reduce(double v, double* red, int tid, F op) {
  __syncthreads();  // (red may still be read from the reduction before)
  red[tid] = v;
  for (int s = PO_THREADS >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) red[tid] = op(red[tid], red[tid + s]);
  }
  __syncthreads();
  return red[0];
}

// the LDS of a tail workgroup
struct crit_tail_lds {
  unsigned long long* key;  // [CRIT_TAIL_MAX] the sort's keys, then the tail's x
  double* tt;               // [CRIT_TAIL_MAX] t_i = exp(x_i) - exp(cut)
  int* row;                 // [CRIT_TAIL_MAX]
  double *bj, *lj, *wj;     // [CRIT_MAX_CAND]
  double* red;              // [PO_THREADS]
  double* bpost;            // [1]
};

#define CRIT_TAIL_LDS(name)                                                                 \
  __shared__ unsigned long long name##_key[CRIT_TAIL_MAX];                                  \
  __shared__ double name##_tt[CRIT_TAIL_MAX];                                               \
  __shared__ int name##_row[CRIT_TAIL_MAX];                                                 \
  __shared__ double name##_bj[CRIT_MAX_CAND], name##_lj[CRIT_MAX_CAND], name##_wj[CRIT_MAX_CAND]; \
  __shared__ double name##_red[PO_THREADS];                                                 \
  __shared__ double name##_bpost;                                                           \
  const crit_tail_lds name = {name##_key, name##_tt, name##_row, name##_bj,                 \
                              name##_lj,  name##_wj, name##_red, &name##_bpost}

// The n tail entries (tx[i], trow[i]) of a column, all threads of the workgroup calling: on
// return s.row holds the rows sorted ascending by (value, row index) and the doubles that overlay
// s.key their values -- the fitted quantiles where a fit was made (n > 4) and its k is finite,
// the sorted values as they were otherwise.  Returns pareto_k (+inf without a fit).  A barrier
// separates nothing from the caller's first read: the caller synchronises.
__device__ __forceinline__ double crit_tail_fit(const crit_tail_lds& s, const double* __restrict__ tx,
                                                const int* __restrict__ trow, int n, double ecut,
                                                int tid) {
  unsigned long long* key = s.key;
  double* tt = s.tt;
  int* row = s.row;
  double *bj = s.bj, *lj = s.lj, *wj = s.wj;
  double* xs = reinterpret_cast<double*>(key);
  const int lane = tid & 63, wave = tid >> 6;

  // ---- the list, padded to a power of two with keys behind every value, sorted by (value, row)
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = tid; i < P; i += PO_THREADS) {
    key[i] = i < n ? crit_key(tx[i]) : ~0ull;
    row[i] = i < n ? trow[i] : 0x7fffffff;
  }
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < P; i += PO_THREADS) {
        const int o = i ^ j;
        if (o > i) {  // (each pair belongs to one thread)
          const unsigned long long ka = key[i], kb = key[o];
          const int ra = row[i], rb = row[o];
          const bool gt = ka > kb || (ka == kb && ra > rb);
          if (gt == ((i & k) == 0)) {
            key[i] = kb; key[o] = ka;
            row[i] = rb; row[o] = ra;
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += PO_THREADS) {
    const double xv = crit_value(key[i]);
    xs[i] = xv;  // (in place: the same eight bytes, this thread's own)
    tt[i] = exp(xv) - ecut;
  }
  __syncthreads();

  // ---- Zhang & Stephens' fit on the sorted t
  double kpar = INFINITY, sigma = 0.0;
  if (n > 4) {  // (n is the workgroup's: every barrier below is met by all threads)
    const double dn = (double)n;
    const int m = 30 + (int)floor(sqrt(dn));
    if (tid < m) {
      double b = 1.0 - sqrt((double)m / ((double)(tid + 1) - 0.5));
      b /= 3.0 * tt[(int)(dn / 4.0 + 0.5) - 1];
      b += 1.0 / tt[n - 1];
      bj[tid] = b;
    }
    __syncthreads();
    for (int j = wave; j < m; j += PO_THREADS / 64) {  // a wave per candidate
      const double b = bj[j];
      double sum = 0.0;
      for (int i = lane; i < n; i += 64) sum += log1p(-b * tt[i]);
      sum = crit_wave_allsum(sum);
      if (lane == 0) {
        const double kk = sum / dn;
        lj[j] = dn * (log(-(b / kk)) - kk - 1.0);
      }
    }
    __syncthreads();
    if (tid < m) {
      double sum = 0.0;
      for (int i = 0; i < m; ++i) sum += exp(lj[i] - lj[tid]);
      const double w = 1.0 / sum;
      wj[tid] = (w >= 10.0 * DBL_EPSILON) ? w : 0.0;  // (dropped; a NaN weight too)
    }
    __syncthreads();
    if (tid == 0) {
      double sw = 0.0, b = 0.0;
      for (int j = 0; j < m; ++j) sw += wj[j];
      for (int j = 0; j < m; ++j) b += bj[j] * (wj[j] / sw);
      *s.bpost = b;
    }
    __syncthreads();
    const double b = *s.bpost;
    double sum = 0.0;
    for (int i = tid; i < n; i += PO_THREADS) sum += log1p(-b * tt[i]);
    sum = crit_block_reduce(sum, s.red, tid, [](double p, double q) { return p + q; });
    const double kp = sum / dn;
    sigma = -kp / b;
    kpar = (dn * kp + 5.0) / (dn + 10.0);
    if (po_finite(kpar)) {  // the tail becomes the fitted distribution's quantiles
      for (int i = tid; i < n; i += PO_THREADS) {
        const double lp = log1p(-((double)i + 0.5) / dn);
        const double g = fabs(kpar) < DBL_EPSILON ? -lp : expm1(-kpar * lp) / kpar;
        const double v = log(g * sigma + ecut);
        xs[i] = v > 0.0 ? 0.0 : v;  // (a NaN stays one)
      }
    }
  }
  return kpar;
}

}  // namespace
