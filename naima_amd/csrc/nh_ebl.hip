// nh_ebl.hip -- EBL absorption (models.py:470-552 of the reference) with the redshift a
// per-walker parameter.
//
// The reference takes the nearest of the 399 tabulated redshift columns (no interpolation in z),
// so at a fixed set of photon energies the transmission is a walker-independent table
// T[row][k] with 400 rows: row 0 is the z < 0.01 case (tau = 10**0, a spline identically 0),
// row c + 1 is column c.  Per walker the only work is one row index and a gathered row.
//
//   nh_ebl_table  builds T (and/or the TableModel values 10**S of __call__) once per set of
//                 energies from the host-prepared cubic B-spline of log10(tau) in log10(E):
//                 one knot vector and one coefficient column per tabulated redshift
//                 (scipy's make_interp_spline(k=3), what interp1d(kind="cubic") evaluates).
//   nh_ebl_apply  out[w][k] = Tab[row(z_w)][k] * colfac[k] * sum_j s_j buf_j[w*ld_j + k] for a
//                 lazy per-walker redshift z_w; with no terms it gathers rows of Tab.
//
// Deterministic, no atomics, no scratch, on the context's stream.
#include "nh_common.h"

#include <cmath>

namespace {

constexpr int EBL_K = 3;                 // cubic
constexpr int EBL_THREADS = 256;
constexpr int EBL_WAVES = EBL_THREADS / 64;

// value at x of the cubic B-spline (t[nt], c[(nt-4)][ldc] column col), x in [t[3], t[nt-4]];
// the basis by the recurrence scipy's _deBoor_D uses, in the same order, without contraction
__device__ double ebl_spline(const double* __restrict__ t, int nt, const double* __restrict__ c,
                             int ldc, int col, double x) {
#pragma clang fp contract(off)
  const int n = nt - EBL_K - 1;
  // the interval l in [k, n-1] with t[l] <= x < t[l+1] (l = n-1 at the right end)
  int lo = EBL_K, hi = n - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= x) lo = mid; else hi = mid - 1;
  }
  const int l = lo;
  double h[EBL_K + 1], hh[EBL_K];
  h[0] = 1.0;
  for (int j = 1; j <= EBL_K; ++j) {
    for (int i = 0; i < j; ++i) hh[i] = h[i];
    h[0] = 0.0;
    for (int i = 1; i <= j; ++i) {
      const double xb = t[l + i], xa = t[l + i - j];
      if (xb == xa) {
        h[i] = 0.0;
        continue;
      }
      const double w = hh[i - 1] / (xb - xa);
      h[i - 1] += w * (xb - x);
      h[i] = w * (x - xa);
    }
  }
  double s = 0.0;
  for (int a = 0; a <= EBL_K; ++a) s = s + c[(long long)(l + a - EBL_K) * ldc + col] * h[a];
  return s;
}

// one thread per (row, energy)
__global__ __launch_bounds__(EBL_THREADS) void k_ebl_table(
    const double* __restrict__ t, int nt, const double* __restrict__ c, int ncol,
    const double* __restrict__ x, const int* __restrict__ code, int nE, double t_hi,
    double* __restrict__ T, double* __restrict__ P) {
#pragma clang fp contract(off)
  long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)(ncol + 1) * nE) return;
  const int row = (int)(idx / nE), k = (int)(idx % nE);
  const int cd = code[k];
  const double xv = x[k];
  double S;
  if (cd & NH_EBL_OUTSIDE) S = -INFINITY;  // interp1d's fill value outside the table
  else if (xv != xv) S = xv;
  else if (row == 0) S = 0.0;              // z < 0.01: log10(10**0) everywhere
  else S = ebl_spline(t, nt, c, ncol, row - 1, xv);
  const double v = exp10(S);               // TableModel.__call__: 10**interp
  if (P) P[idx] = v;
  if (T) {
    const int br = cd & 3;
    // transmission: exp(-log10(__call__)) between 1 GeV and 100 TeV, as the scalar path
    T[idx] = br == NH_EBL_ONE ? 1.0 : br == NH_EBL_HIGH ? t_hi : exp(-log10(v));
  }
}

// the row of Tab for redshift z: -1 (a NaN row) for z < 0, NaN or +-inf; 0 for z < 0.01;
// else 1 + argmin_i |zl[i] - z| with the first index winning a tie (np.argmin)
__device__ int ebl_row(const double* __restrict__ zl, int nzl, double z) {
  if (!(z >= 0.0) || isinf(z)) return -1;  // (-0.0 >= 0.0: valid, as the reference's value < 0)
  if (!(z >= 0.01)) return 0;
  // zl[i] ~ 0.01 (i + 1): the nearest lies within [c - 1, c + 2], c = floor(100 z) - 1
  const int c = (int)floor(fmin(z * 100.0, 1e6)) - 1;
  const int lo = max(0, min(c - 1, nzl - 1)), hi = min(nzl - 1, max(c + 2, 0));
  int best = lo;
  double bd = INFINITY;
  for (int i = lo; i <= hi; ++i) {
    const double d = fabs(zl[i] - z);
    if (d < bd) {
      bd = d;
      best = i;
    }
  }
  return best + 1;
}

struct ebl_comps { nh_comp c[NH_MAX_COMP]; int n; };

// one wave per walker row: the row index is wave-uniform
__global__ __launch_bounds__(EBL_THREADS) void k_ebl_apply(
    const double* __restrict__ tab, int ldt, const double* __restrict__ zl, int nzl, nh_lazy z,
    ebl_comps P, const double* __restrict__ colfac, int N, int m, double* __restrict__ out,
    int ldo) {
  const int w = blockIdx.x * EBL_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= N) return;
  const int row = __builtin_amdgcn_readfirstlane(ebl_row(zl, nzl, nh_lazy_eval(z, w)));
  double* o = out + (long long)w * ldo;
  if (row < 0) {
    for (int k = lane; k < m; k += 64) o[k] = NAN;
    return;
  }
  const double* tr = tab + (long long)row * ldt;
  for (int k = lane; k < m; k += 64) {
    double s = 1.0;
    if (P.n > 0) {
      s = 0.0;
      for (int j = 0; j < P.n; ++j) s += P.c[j].scale * P.c[j].ptr[(long long)w * P.c[j].ld + k];
    }
    if (colfac) s *= colfac[k];
    o[k] = tr[k] * s;
  }
}

}  // namespace

extern "C" int nh_ebl_table(nh_ctx* c, const double* knots, int nt, const double* coef, int ncol,
                            const double* x, const int* code, int nE, double t_hi, double* T,
                            double* P) {
  NH_REQUIRE(c && knots && coef && x && code && (T || P), "null argument");
  NH_REQUIRE(nt >= 2 * (EBL_K + 1) && ncol >= 1 && nE >= 1, "bad table shape");
  nh_prof_scope ps(c, NH_K_GLUE);
  long long tot = (long long)(ncol + 1) * nE;
  hipLaunchKernelGGL(k_ebl_table, dim3((unsigned)((tot + EBL_THREADS - 1) / EBL_THREADS)),
                     dim3(EBL_THREADS), 0, c->stream, knots, nt, coef, ncol, x, code, nE, t_hi, T,
                     P);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_ebl_apply(nh_ctx* c, const double* tab, int ldt, int nrows, const double* zl,
                            int nzl, const nh_lazy* z, const nh_comp* comps, int ncomp,
                            const double* colfac, int N, int m, double* out, int ldo) {
  NH_REQUIRE(c && tab && zl && z && out, "null argument");
  NH_REQUIRE(nzl >= 1 && nrows == nzl + 1, "the table must have one row per redshift column + 1");
  NH_REQUIRE(ncomp >= 0 && ncomp <= NH_MAX_COMP && (ncomp == 0 || comps), "ncomp must be 0..8");
  NH_REQUIRE(N >= 0 && m >= 1 && m <= ldt && ldo >= m, "bad shape");
  if (N == 0) return NH_OK;
  ebl_comps P;
  P.n = ncomp;
  for (int j = 0; j < ncomp; ++j) P.c[j] = comps[j];
  nh_prof_scope ps(c, NH_K_GLUE);
  hipLaunchKernelGGL(k_ebl_apply, dim3((unsigned)((N + EBL_WAVES - 1) / EBL_WAVES)),
                     dim3(EBL_THREADS), 0, c->stream, tab, ldt, zl, nzl, *z, P, colfac, N, m, out,
                     ldo);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
