// nh_pairabs.hip -- gamma-gamma pair-production absorption on photon fields (Breit-Wheeler
// cross section; Gould & Schreder 1967), per walker.
//
// With m = m_e c^2 and s = E eps (1 - cos theta) / (2 m^2) the cross section is, for s > 1,
//   sigma(s) = (3 sigma_T / 16)(1 - b^2) [ (3 - b^4) ln((1+b)/(1-b)) - 2 b (2 - b^2) ],
//   b = sqrt(1 - 1/s),
// and the opacity per unit length of a field of differential density n(eps) is
//   isotropic:       int n(eps) sbar(E eps / m^2) deps,  sbar(s0) = (2/s0^2) int_1^s0 s sigma ds
//   at an angle:     mu int n(eps) sigma(E eps mu / (2 m^2)) deps,  mu = 1 - cos theta.
//
//   nh_pairabs_rows   kappa[row][k]: the opacity per unit length and per unit of field density
//                     of ONE field at photon energy k -- per dilution factor w = u / (a T^4) of
//                     a thermal field, per photon of a monochromatic one, and the opacity
//                     itself of a tabulated one.  One wave per (row, energy).
//   nh_pairabs_apply  out[w][k] = exp(-sum_f L_f(w) a_f(w) kappa_f[row_f(w)][k]) * colfac[k]
//                     * sum_j s_j buf_j[w*ld_j + k]; one wave per walker row.
//
// The integration variable is t with s = cosh^2 t: then b = tanh t, ln((1+b)/(1-b)) = 2t and
// sigma is an analytic function of t through the threshold t = 0 (in s it starts like
// sqrt(s - 1)), while for large s, t = ln(4s)/2 is logarithmic.  The integrals
//   thermal, isotropic:  (2/eta^2) int_1^inf s sigma(s) (-ln(1 - exp(-s/eta))) ds, eta = E kT/m^2
//     (the double integral over the Planck spectrum and sbar with the order exchanged)
//   thermal, at an angle: eta'^-3 int_1^inf s^2 sigma(s) / (exp(s/eta') - 1) ds, eta' = eta mu/2
//   monochromatic:       (2/s0^2) int_1^s0 s sigma(s) ds
// are taken with a fixed composite 8-point Gauss-Legendre rule on at most PA_PANELS panels
// between t = 0 (the threshold: the range STARTS at the kink) and, for the thermal fields, the t
// at which s - 1 = PA_TAIL eta: the integrand has fallen by exp(-PA_TAIL) there.  On the Wien
// side (eta << 1) that range is ~ sqrt(PA_TAIL eta) wide and the panels follow the Gaussian
// exp(-sinh^2 t / eta); on the Rayleigh-Jeans side (eta >> 1) a panel ends at s = eta, where
// -ln(1 - exp(-s/eta)) ~ ln(eta/s) hands over to the Planck tail exp(-s/eta).  No pow in the
// node loop.  A value that underflows is 0.
//
// FP64, deterministic, no atomics, no scratch, on the context's stream.  Measured errors
// against mpmath: profiles/NOTES_pairabs.md, tests/test_gpu_pairabs.py.
#include "nh_common.h"

#include <cmath>

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_WAVES = PA_THREADS / 64;
constexpr int PA_PANELS = 64;        // 512 nodes: eight per lane
constexpr double PA_TAIL = 50.0;     // exp(-50) = 2e-22 of the integrand is left out
constexpr double PA_AR_CGS = 7.565733250280007e-15;  // radiation constant, constants.py
constexpr double PA_SIGMA_T = 8.0 * NH_PI / 3.0 * NH_R0_CM * NH_R0_CM;
constexpr double PA_LAMBDA_C = NH_HBAR_CGS / (NH_M_E_G * NH_C_CGS);  // hbar c / (m_e c^2), cm

__constant__ double PA_GLX[8] = {-0.9602898564975363, -0.7966664774136267, -0.5255324099163290,
                                 -0.1834346424956498, 0.1834346424956498,  0.5255324099163290,
                                 0.7966664774136267,  0.9602898564975363};
__constant__ double PA_GLW[8] = {0.1012285362903763, 0.2223810344533745, 0.3137066458778873,
                                 0.3626837833783620, 0.3626837833783620, 0.3137066458778873,
                                 0.2223810344533745, 0.1012285362903763};

__device__ __forceinline__ double pa_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

// sigma / sigma_T at s = cosh^2 t (ch = cosh t), t >= 0
__device__ __forceinline__ double pa_sigma(double t, double ch) {
  const double b = tanh(t), b2 = b * b;
  return (3.0 / 16.0) / (ch * ch) * ((3.0 - b2 * b2) * (2.0 * t) - 2.0 * b * (2.0 - b2));
}

// -ln(1 - exp(-x)), x > 0: each branch keeps the relative accuracy of its small quantity
__device__ __forceinline__ double pa_planck_log(double x) {
  return x > 0.6931471805599453 ? -log1p(-exp(-x)) : -log(-expm1(-x));
}

enum { PA_ISO = 0, PA_ANGLE = 1, PA_MONO = 2 };

// int_0^tend f(t) dt with s = cosh^2 t, f = ds/dt times
//   PA_ISO:   s sigma(s) (-ln(1 - exp(-s/eta)))
//   PA_ANGLE: s^2 sigma(s) / (exp(s/eta) - 1)
//   PA_MONO:  s sigma(s)
// in units of sigma_T; a panel ends at tkink when 0 < tkink < tend
__device__ double pa_integral(int mode, double eta, double tend, double tkink, int lane) {
  if (!(tend > 0.0)) return tend == 0.0 ? 0.0 : tend + __builtin_nan("");
  // two stretches of equal panels, PA_PANELS at most together
  const double h = tend / (PA_PANELS - 2);
  int n1 = 0;
  double w1 = 0.0, a2 = 0.0;
  if (tkink > 0.0 && tkink < tend) {
    n1 = (int)ceil(tkink / h);
    w1 = tkink / n1;
    a2 = tkink;
  }
  const int n2 = (int)ceil((tend - a2) / h);
  const double w2 = (tend - a2) / n2;
  const int np = n1 + n2;
  const double inv_eta = mode == PA_MONO ? 0.0 : 1.0 / eta;
  double acc = 0.0;
  for (int n = lane; n < np * 8; n += 64) {
    const int pan = n >> 3, q = n & 7;
    const bool first = pan < n1;
    const double w = first ? w1 : w2;
    const double t = (first ? 0.0 : a2) + ((first ? pan : pan - n1) + 0.5 * (1.0 + PA_GLX[q])) * w;
    const double ch = cosh(t), sh = sinh(t), s = ch * ch;
    double f = s * pa_sigma(t, ch) * (2.0 * ch * sh);
    if (mode == PA_ISO) {
      f *= pa_planck_log(s * inv_eta);
    } else if (mode == PA_ANGLE) {
      const double e = expm1(s * inv_eta);  // (inf: the term is gone)
      f = isinf(e) ? 0.0 : f * s / e;
    }
    if (!(f == f) || isinf(f)) f = 0.0;  // an overflowed tail contributes nothing
    acc += PA_GLW[q] * w * f;
  }
  return pa_wave_sum(acc) * 0.5;
}

// one segment of trapz_loglog as the reference writes it (utils.py:336-348)
__device__ double pa_trapz_seg(double x1, double x2, double y1, double y2) {
  if (y1 == 0.0 || y2 == 0.0) return 0.0;
  const double b = log10(y2 / y1) / log10(x2 / x1);
  if (fabs(b + 1.0) > 1e-10) return y1 * (x2 * pow(x2 / x1, b) - x1) / (b + 1.0);
  return x1 * y1 * log(x2 / x1);
}

struct pa_rows_args {
  int kind, iso;
  double k_to_mec2;
  nh_lazy T, theta;
  const double* se;  // [ns] eV
  const double* sn;  // [ns] 1/(eV cm3), a tabulated field
  int ns;
  const double* x;   // [nE] E / (m_e c^2)
  int nE, nrows;
  double* out;
  int ldo;
};

// one wave per (row, energy)
__global__ __launch_bounds__(PA_THREADS) void k_pairabs_rows(pa_rows_args A) {
  const long long task = (long long)blockIdx.x * PA_WAVES + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (task >= (long long)A.nrows * A.nE) return;
  const int row = (int)(task / A.nE), k = (int)(task % A.nE);
  const double x = A.x[k];
  double mu = 2.0;
  if (!A.iso) mu = 1.0 - cos(fabs(nh_lazy_eval(A.theta, row)));
  // every case is the ONE call of pa_integral below (a closed form at an angle): a thermal or
  // monochromatic field in one trip, a tabulated one in a trip per node of its table
  const int trips = A.kind == NH_PAIR_TABLE ? A.ns : 1;
  double v = 0.0, yp = 0.0, ep = 0.0;
  for (int i = 0; i < trips; ++i) {
    int mode = PA_MONO;
    double eta = 0.0, tend = 0.0, tkink = 0.0, pre = 0.0, fixed = 0.0, e = 0.0;
    bool quad = false;
    if (A.kind == NH_PAIR_THERMAL) {
      const double T = nh_lazy_eval(A.T, row);
      const double th = T * A.k_to_mec2;  // kT / (m_e c^2)
      eta = A.iso ? x * th : x * th * (0.5 * mu);
      if (!(T > 0.0) || isinf(T) || !(eta == eta) || isinf(eta)) {
        fixed = __builtin_nan("");
      } else if (eta > 0.0) {  // (else theta = 0 or E = 0: nothing is above the threshold)
        quad = true;
        mode = A.iso ? PA_ISO : PA_ANGLE;
        tend = asinh(sqrt(PA_TAIL * eta));
        tkink = eta > 1.0 ? asinh(sqrt(eta - 1.0)) : 0.0;
        const double lam = th / PA_LAMBDA_C;
        pre = PA_SIGMA_T * (lam * lam * lam) / (NH_PI * NH_PI);
        pre = A.iso ? pre * (2.0 / (eta * eta)) : pre * mu / (eta * eta * eta);
      }
    } else {
      // sbar(s0), or with an angle mu sigma(s0 mu / 2)
      e = A.se[i];
      const double s0 = x * (e / NH_MEC2_EV);
      const double s = A.iso ? s0 : s0 * (0.5 * mu);
      if (!(s == s)) {
        fixed = s;
      } else if (s > 1.0) {
        const double t0 = asinh(sqrt(s - 1.0));  // (s - 1 is exact next to the threshold)
        if (A.iso) {
          quad = true;
          tend = t0;
          pre = PA_SIGMA_T * (2.0 / (s0 * s0));
        } else {
          fixed = PA_SIGMA_T * mu * pa_sigma(t0, cosh(t0));
        }
      }
    }
    const double y = quad ? pre * pa_integral(mode, eta, tend, tkink, lane) : fixed;
    if (A.kind != NH_PAIR_TABLE) {
      v = y;
    } else {
      // naima's rule for a tabulated field: trapz_loglog over the table's own nodes
      const double yn = A.sn[i] * y;
      if (i > 0) v += pa_trapz_seg(ep, e, yp, yn);
      yp = yn;
      ep = e;
    }
  }
  if (lane == 0) A.out[(long long)row * A.ldo + k] = v;
}

struct pa_apply_args {
  nh_pair_field f[NH_MAX_COMP];
  int nf;
  nh_comp c[NH_MAX_COMP];
  int nc;
};

// one wave per walker row: the fields' scalars are wave-uniform
__global__ __launch_bounds__(PA_THREADS) void k_pairabs_apply(
    pa_apply_args P, const double* __restrict__ colfac, int write_tau, int N, int m,
    double* __restrict__ out, int ldo) {
#pragma clang fp contract(off)
  const int w = blockIdx.x * PA_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= N) return;
  double coef[NH_MAX_COMP];
  bool bad = false;
#pragma unroll
  for (int f = 0; f < NH_MAX_COMP; ++f) {
    coef[f] = 0.0;
    if (f < P.nf) {
      const double L = nh_lazy_eval(P.f[f].L_cm, w);
      double a = nh_lazy_eval(P.f[f].dens, w);
      bad = bad || !(L >= 0.0) || isinf(L) || !(a >= 0.0) || isinf(a);
      if (P.f[f].thermal) {
        const double T = nh_lazy_eval(P.f[f].T_K, w);
        bad = bad || !(T > 0.0) || isinf(T);
        const double T2 = T * T;
        a = a / (PA_AR_CGS * (T2 * T2));  // the dilution factor u / (a T^4)
      }
      coef[f] = L * a;
    }
  }
  double* o = out + (long long)w * ldo;
  if (bad) {
    for (int k = lane; k < m; k += 64) o[k] = __builtin_nan("");
    return;
  }
  for (int k = lane; k < m; k += 64) {
    double tau = 0.0;
#pragma unroll
    for (int f = 0; f < NH_MAX_COMP; ++f)
      if (f < P.nf) tau = tau + coef[f] * P.f[f].kappa[(long long)w * P.f[f].ld + k];
    if (write_tau) {
      o[k] = tau;
      continue;
    }
    double s = 1.0;
    if (P.nc > 0) {
      s = 0.0;
      for (int j = 0; j < P.nc; ++j) s += P.c[j].scale * P.c[j].ptr[(long long)w * P.c[j].ld + k];
    }
    if (colfac) s *= colfac[k];
    o[k] = exp(-tau) * s;
  }
}

}  // namespace

extern "C" int nh_pairabs_rows(nh_ctx* c, int kind, double k_to_mec2, const nh_lazy* T_K,
                               const nh_lazy* theta, const double* seed_E_eV,
                               const double* seed_dens, int ns, const double* x, int nE, int nrows,
                               double* out, int ldo) {
  NH_REQUIRE(c && x && out, "null argument");
  NH_REQUIRE(kind >= NH_PAIR_THERMAL && kind <= NH_PAIR_TABLE, "unknown field kind");
  NH_REQUIRE(nE >= 1 && nrows >= 0 && ldo >= nE, "bad shape");
  pa_rows_args A;
  memset(&A, 0, sizeof A);
  A.kind = kind;
  A.iso = theta == nullptr;
  A.k_to_mec2 = k_to_mec2;
  if (theta) A.theta = *theta;
  if (kind == NH_PAIR_THERMAL) {
    NH_REQUIRE(T_K && k_to_mec2 > 0.0, "a thermal field needs its temperature");
    A.T = *T_K;
  } else {
    NH_REQUIRE(seed_E_eV && ns >= 1, "a monochromatic or tabulated field needs its energies");
    NH_REQUIRE(kind == NH_PAIR_MONO ? ns == 1 : (seed_dens && ns >= 2),
               "one energy (monochromatic), or two and more with their densities (tabulated)");
    NH_REQUIRE(nrows <= 1 || (theta && theta->base), "these fields have one row");
  }
  if (nrows == 0) return NH_OK;
  A.se = seed_E_eV;
  A.sn = seed_dens;
  A.ns = ns;
  A.x = x;
  A.nE = nE;
  A.nrows = nrows;
  A.out = out;
  A.ldo = ldo;
  const long long tasks = (long long)nrows * nE;
  NH_REQUIRE(tasks <= 0x7fffffffLL, "too many (row, energy) pairs");
  nh_prof_scope ps(c, NH_K_TABLES);
  hipLaunchKernelGGL(k_pairabs_rows, dim3((unsigned)((tasks + PA_WAVES - 1) / PA_WAVES)),
                     dim3(PA_THREADS), 0, c->stream, A);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_pairabs_apply(nh_ctx* c, const nh_pair_field* fields, int nfields,
                                const nh_comp* comps, int ncomp, const double* colfac,
                                int write_tau, int N, int m, double* out, int ldo) {
  NH_REQUIRE(c && out, "null argument");
  NH_REQUIRE(nfields >= 0 && nfields <= NH_MAX_COMP && (nfields == 0 || fields),
             "nfields must be 0..8");
  NH_REQUIRE(ncomp >= 0 && ncomp <= NH_MAX_COMP && (ncomp == 0 || comps), "ncomp must be 0..8");
  NH_REQUIRE(!write_tau || (ncomp == 0 && !colfac), "the opacity takes no terms");
  NH_REQUIRE(N >= 0 && m >= 1 && ldo >= m, "bad shape");
  if (N == 0) return NH_OK;
  pa_apply_args P;
  memset(&P, 0, sizeof P);
  P.nf = nfields;
  for (int f = 0; f < nfields; ++f) {
    NH_REQUIRE(fields[f].kappa && (fields[f].ld == 0 || fields[f].ld >= m), "bad field rows");
    P.f[f] = fields[f];
  }
  P.nc = ncomp;
  for (int j = 0; j < ncomp; ++j) P.c[j] = comps[j];
  nh_prof_scope ps(c, NH_K_GLUE);
  hipLaunchKernelGGL(k_pairabs_apply, dim3((unsigned)((N + PA_WAVES - 1) / PA_WAVES)),
                     dim3(PA_THREADS), 0, c->stream, P, colfac, write_tau, N, m, out, ldo);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
