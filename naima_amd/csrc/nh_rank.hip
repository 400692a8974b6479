// nh_rank.hip -- the rank transform of whole pooled columns of a device matrix, and what the
// rank-normalised convergence statistics of Vehtari et al. 2021 build on it:
//   nh_rank_columns        scipy.stats.rankdata(col, method="average") of every pooled column;
//   nh_rank_normal_scores  z = Phi^-1((r - 3/8) / (S + 1/4)) (Blom), pooled or in the chain's layout;
//   nh_rank_transform      |x - m| (folding) and x <= q (tail indicators), thresholds per column.
//
// A pooled column p holds S = nrows * npool values: element e = t * npool + j is
// x[(row0 + t) * ld + j * cstride + p] -- for a chain [rows][walker][parameter] (cstride = ndim,
// npool = walkers) the order of chain[row0:, :, p].ravel(); for a plain matrix npool = 1.  Nothing
// is copied into a pooled matrix, on the host or on the device.
//
// Ranking, per group of columns that fits the scratch budget (columns are independent):
//   k_rank_keys     order-preserving 64-bit keys, column-major [column][e] in library scratch
//                   (-0.0 is made +0.0 first: the two tie); counts the column's non-finite values
//                   into status (one integer atomic per wave);
//   eight passes of a least-significant-digit radix sort of the row INDEX (8-bit digits; the key
//   is read through the index, so an element costs 16 bytes of scratch: key, and the index twice):
//   k_rank_hist, k_rank_scan and k_rank_scatter of nh_radix.h, which nh_reweight.hip shares;
//   k_rank_ties     position i of the sorted run finds the first and last position of its key (a
//                     few neighbours, then a binary search) and writes (first + last) / 2 + 1
//                     through the index; a column with a non-finite value is written NaN throughout.
// Every launch is on the context's stream; nothing synchronises with the host.
#include "nh_radix.h"

namespace {

constexpr int RK_NEAR = 4;                        // neighbours looked at before the binary search

__device__ __forceinline__ long long rk_src(long long e, long long row0, long long ld,
                                            long long cstride, int npool, int p) {
  long long t = e / npool, j = e - t * npool;
  return (row0 + t) * ld + j * cstride + p;
}

__global__ __launch_bounds__(RK_THREADS) void k_rank_keys(const double* __restrict__ x, long long row0,
                                                          long long ld, long long cstride, int npool,
                                                          long long S, int c0,
                                                          unsigned long long* __restrict__ keys,
                                                          int* __restrict__ status) {
  long long e = (long long)blockIdx.x * RK_THREADS + threadIdx.x;
  int p = c0 + blockIdx.y;
  bool bad = false;
  if (e < S) {
    double v = x[rk_src(e, row0, ld, cstride, npool, p)];
    bad = !(fabs(v) <= 1.7976931348623157e308);  // NaN, +-inf
    keys[(long long)blockIdx.y * S + e] = rk_key(v);
  }
  unsigned long long m = __builtin_amdgcn_ballot_w64(bad);
  if (m && (threadIdx.x & 63) == 0)
    __hip_atomic_fetch_add(status + p, (int)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// r[idx[i]] = the mean of the 1-based positions the key of sorted position i occupies
__global__ __launch_bounds__(RK_THREADS) void k_rank_ties(const unsigned long long* __restrict__ keys,
                                                          const unsigned* __restrict__ idx, long long S,
                                                          int c0, int ncolp,
                                                          const int* __restrict__ status,
                                                          double* __restrict__ r) {
  long long i = (long long)blockIdx.x * RK_THREADS + threadIdx.x;
  if (i >= S) return;
  const unsigned long long* kc = keys + (long long)blockIdx.y * S;
  const unsigned* ic = idx + (long long)blockIdx.y * S;
  int p = c0 + blockIdx.y;
  unsigned me = ic[i];
  double* dst = r + (long long)me * ncolp + p;
  if (status[p] != 0) { *dst = nh_nan(); return; }
  unsigned long long k = kc[me];
  long long first = i, last = i;
  for (int n = 0; n < RK_NEAR && first > 0 && kc[ic[first - 1]] == k; ++n) --first;
  if (first > 0 && kc[ic[first - 1]] == k) {  // the run starts further down: keys ascend
    long long lo = 0, hi = first - 1;
    while (lo < hi) {
      long long mid = (lo + hi) >> 1;
      if (kc[ic[mid]] < k) lo = mid + 1; else hi = mid;
    }
    first = lo;
  }
  for (int n = 0; n < RK_NEAR && last < S - 1 && kc[ic[last + 1]] == k; ++n) ++last;
  if (last < S - 1 && kc[ic[last + 1]] == k) {
    long long lo = last + 1, hi = S - 1;
    while (lo < hi) {
      long long mid = (lo + hi + 1) >> 1;
      if (kc[ic[mid]] > k) hi = mid - 1; else lo = mid;
    }
    last = lo;
  }
  *dst = 0.5 * (double)(first + last) + 1.0;
}

// Wichura's algorithm AS 241, PPND16: the normal deviate of the lower tail area p, about 1e-16
// relative.  Central rational in q = p - 1/2 for |q| <= 0.425; the tails in
// r = sqrt(-log(min(p, 1 - p))), two ranges split at r = 5 (p = 1.4e-11).
__device__ double rk_ppnd16(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    double num = 2.5090809287301226727e3;
    num = fma(num, r, 3.3430575583588128105e4);
    num = fma(num, r, 6.7265770927008700853e4);
    num = fma(num, r, 4.5921953931549871457e4);
    num = fma(num, r, 1.3731693765509461125e4);
    num = fma(num, r, 1.9715909503065514427e3);
    num = fma(num, r, 1.3314166789178437745e2);
    num = fma(num, r, 3.3871328727963666080e0);
    double den = 5.2264952788528545610e3;
    den = fma(den, r, 2.8729085735721942674e4);
    den = fma(den, r, 3.9307895800092710610e4);
    den = fma(den, r, 2.1213794301586595867e4);
    den = fma(den, r, 5.3941960214247511077e3);
    den = fma(den, r, 6.8718700749205790830e2);
    den = fma(den, r, 4.2313330701600911252e1);
    den = fma(den, r, 1.0);
    return q * num / den;
  }
  double r = q < 0.0 ? p : 1.0 - p;  // (1 - p is exact for p >= 1/2)
  if (!(r > 0.0)) return r == 0.0 ? (q < 0.0 ? -INFINITY : INFINITY) : nh_nan();
  r = sqrt(-log(r));
  double num, den;
  if (r <= 5.0) {
    r -= 1.6;
    num = 7.74545014278341407640e-4;
    num = fma(num, r, 2.27238449892691845833e-2);
    num = fma(num, r, 2.41780725177450611770e-1);
    num = fma(num, r, 1.27045825245236838258e0);
    num = fma(num, r, 3.64784832476320460504e0);
    num = fma(num, r, 5.76949722146069140550e0);
    num = fma(num, r, 4.63033784615654529590e0);
    num = fma(num, r, 1.42343711074968357734e0);
    den = 1.05075007164441684324e-9;
    den = fma(den, r, 5.47593808499534494600e-4);
    den = fma(den, r, 1.51986665636164571966e-2);
    den = fma(den, r, 1.48103976427480074590e-1);
    den = fma(den, r, 6.89767334985100004550e-1);
    den = fma(den, r, 1.67638483018380384940e0);
    den = fma(den, r, 2.05319162663775882187e0);
    den = fma(den, r, 1.0);
  } else {
    r -= 5.0;
    num = 2.01033439929228813265e-7;
    num = fma(num, r, 2.71155556874348757815e-5);
    num = fma(num, r, 1.24266094738807843860e-3);
    num = fma(num, r, 2.65321895265761230930e-2);
    num = fma(num, r, 2.96560571828504891230e-1);
    num = fma(num, r, 1.78482653991729133580e0);
    num = fma(num, r, 5.46378491116411436990e0);
    num = fma(num, r, 6.65790464350110377720e0);
    den = 2.04426310338993978564e-15;
    den = fma(den, r, 1.42151175831644588870e-7);
    den = fma(den, r, 1.84631831751005468180e-5);
    den = fma(den, r, 7.86869131145613259100e-4);
    den = fma(den, r, 1.48753612908506148525e-2);
    den = fma(den, r, 1.36929880922735805310e-1);
    den = fma(den, r, 5.99832206555887937690e-1);
    den = fma(den, r, 1.0);
  }
  const double v = num / den;
  return q < 0.0 ? -v : v;
}

// where element e of pooled column p lies in a chain-layout matrix whose rows start at 0
__device__ __forceinline__ long long rk_chain_at(long long e, int p, int npool, long long ldz,
                                                 long long cstride) {
  long long t = e / npool, j = e - t * npool;
  return t * ldz + j * cstride + p;
}

__global__ __launch_bounds__(RK_THREADS) void k_rank_scores(const double* __restrict__ r, long long S,
                                                            int npool, int ncolp, int layout,
                                                            long long ldz, long long cstride,
                                                            double* __restrict__ z) {
  long long n = S * ncolp;
  const double denom = (double)S + 0.25;
  for (long long i = (long long)blockIdx.x * RK_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * RK_THREADS) {
    long long e = i / ncolp;
    int p = (int)(i - e * ncolp);
    double v = r[i];
    double s = v != v ? nh_nan() : rk_ppnd16((v - 0.375) / denom);
    z[layout == NH_RANK_CHAIN ? rk_chain_at(e, p, npool, ldz, cstride) : i] = s;
  }
}

__global__ __launch_bounds__(RK_THREADS) void k_rank_transform(const double* __restrict__ x,
                                                               long long row0, long long ld,
                                                               long long cstride, int npool, int ncolp,
                                                               long long S,
                                                               const double* __restrict__ thr, int mode,
                                                               double* __restrict__ out, long long ldo) {
  long long n = S * ncolp;
  for (long long i = (long long)blockIdx.x * RK_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * RK_THREADS) {
    long long e = i / ncolp;
    int p = (int)(i - e * ncolp);
    double v = x[rk_src(e, row0, ld, cstride, npool, p)], q = thr[p];
    double o;
    if (mode == NH_RANK_FOLD) o = fabs(v - q);
    else o = (v != v || q != q) ? nh_nan() : (v <= q ? 1.0 : 0.0);
    out[rk_chain_at(e, p, npool, ldo, cstride)] = o;
  }
}

int rk_check_pool(const char* fn, long long row0, long long nrows, long long ld, long long cstride,
                  int npool, int ncolp) {
  if (row0 < 0 || nrows < 1 || npool < 1 || ncolp < 1)
    return nh_set_error(NH_EINVAL, "%s: row0 < 0, or nrows, npool or ncolp not positive", fn);
  if (npool > 1 && cstride < ncolp)
    return nh_set_error(NH_EINVAL, "%s: cstride < ncolp: pooled columns would overlap", fn);
  if (cstride < 0 || (long long)(npool - 1) * cstride + ncolp > ld)
    return nh_set_error(NH_EINVAL, "%s: (npool - 1) * cstride + ncolp > ld", fn);
  if (nrows >= (1ll << 31) / npool)
    return nh_set_error(NH_EINVAL, "%s: nrows * npool >= 2^31 values in a pooled column", fn);
  return NH_OK;
}

unsigned rk_grid(long long n) {
  return (unsigned)std::min<long long>((n + RK_THREADS - 1) / RK_THREADS, 1 << 16);
}

}  // namespace

extern "C" int nh_rank_columns(nh_ctx* ctx, const double* x, long long row0, long long nrows,
                               long long ld, long long cstride, int npool, int ncolp, double* r,
                               int* status) {
  NH_REQUIRE(ctx && x && r && status, "null argument");
  int rc = rk_check_pool(__func__, row0, nrows, ld, cstride, npool, ncolp);
  if (rc) return rc;
  const long long S = nrows * npool;
  const int G = rk_group(S, ncolp, 0);
  void* base = nullptr;
  rc = nh_scratch(ctx, rk_bytes_per_column(S) * G, &base);
  if (rc) return rc;
  const rk_buffers b(base, S, G);
  hipStream_t s = ctx->stream;
  NH_CHECK_HIP(hipMemsetAsync(status, 0, (size_t)ncolp * sizeof(int), s));
  const unsigned eb = (unsigned)((S + RK_THREADS - 1) / RK_THREADS);
  for (int c0 = 0; c0 < ncolp; c0 += G) {
    const int g = std::min(G, ncolp - c0);
    hipLaunchKernelGGL(k_rank_keys, dim3(eb, g), dim3(RK_THREADS), 0, s, x, row0, ld, cstride, npool,
                       S, c0, b.keys, status);
    NH_CHECK_HIP(hipGetLastError());
    const unsigned* in = nullptr;
    rc = rk_sort(s, b, S, g, &in);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rank_ties, dim3(eb, g), dim3(RK_THREADS), 0, s, b.keys, in, S, c0, ncolp,
                       status, r);
    NH_CHECK_HIP(hipGetLastError());
  }
  return NH_OK;
}

extern "C" int nh_rank_normal_scores(nh_ctx* ctx, const double* r, long long nrows, int npool,
                                     int ncolp, int layout, long long ldz, long long cstride,
                                     double* z) {
  NH_REQUIRE(ctx && r && z, "null argument");
  NH_REQUIRE(layout == NH_RANK_POOLED || layout == NH_RANK_CHAIN, "layout must be NH_RANK_POOLED or NH_RANK_CHAIN");
  int rc = rk_check_pool(__func__, 0, nrows, layout == NH_RANK_CHAIN ? ldz : (1ll << 62),
                         layout == NH_RANK_CHAIN ? cstride : (npool > 1 ? ncolp : 0), npool, ncolp);
  if (rc) return rc;
  const long long S = nrows * npool;
  hipLaunchKernelGGL(k_rank_scores, dim3(rk_grid(S * ncolp)), dim3(RK_THREADS), 0, ctx->stream, r, S,
                     npool, ncolp, layout, ldz, cstride, z);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_rank_transform(nh_ctx* ctx, const double* x, long long row0, long long nrows,
                                 long long ld, long long cstride, int npool, int ncolp,
                                 const double* thr, int mode, double* out, long long ldo) {
  NH_REQUIRE(ctx && x && thr && out, "null argument");
  NH_REQUIRE(mode == NH_RANK_FOLD || mode == NH_RANK_LE, "mode must be NH_RANK_FOLD or NH_RANK_LE");
  int rc = rk_check_pool(__func__, row0, nrows, ld, cstride, npool, ncolp);
  if (rc) return rc;
  NH_REQUIRE((long long)(npool - 1) * cstride + ncolp <= ldo, "(npool - 1) * cstride + ncolp > ldo");
  const long long S = nrows * npool;
  hipLaunchKernelGGL(k_rank_transform, dim3(rk_grid(S * ncolp)), dim3(RK_THREADS), 0, ctx->stream, x,
                     row0, ld, cstride, npool, ncolp, S, thr, mode, out, ldo);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
