// nh_kelner_leptons.hip -- SecondaryLeptonsKelner06._spectrum: the electrons and neutrinos of
// pp -> pi+- -> mu nu -> e nu nu with the parametrisation of Kelner, Aharonian & Bugayov 2006
// (KAB06), the paper nh_kelner.hip takes the gamma rays from.  No reference counterpart.
//
// Three components -- e (e+ + e-, which is also the muon neutrino of the muon decay), nu_e,
// and numu1 (the muon neutrino of the pion decay) -- are integrals over x = E / Ep (full
// calculation, E >= Etrans) or x = E / E_pi (delta-functional approximation, below) of the
// same sigma_inel J as the gamma rays, times one more kernel function each:
//   full  (Eq. 62-69):  c int_0^1 sigma(Ep) J(Ep) F(x, Ep) dx/x,            Ep = E / x
//   delta (section IV): 2 (c / K_pi) int_0^1 f(x) sigma(Ep0) J(Ep0) dx/x,   Ep0 = m_p + E / (x K_pi)
//                       restricted to E_pi = E / x >= m_pi
// With x = exp(-t), dx/x = dt, both are integrals over t of smooth, exponentially decaying
// functions between kinks, and one wave forms every component a task needs on ONE set of panels:
// sigma J once per node.  The panels are those of k06_integral (nh_kelner.hip): stretches that end
// at the kinks -- e_break, 0.1 TeV, the threshold, a steep cut-off's 40 e-foldings -- and the
// h-grid behind the last.  The kinks these integrands add:
//   t_lambda = ln(1/0.427): where numu1 starts in both branches (a node takes part in it when
//       its stretch starts at or behind t_lambda -- an exact comparison of two copies of one number)
//   t_r = ln(1/0.573): where the decay distributions of the delta branch change form
//   full branch, Ep = 36.3 GeV: below it Eq. 64's beta_e does not exist (the fourth root of a
//       negative number).  beta_e -> inf from above and F_e -> 0 with all its derivatives, so
//       F_e = 0 below is its continuation; the fit is used from there although KAB06 give it for
//       Ep >= 0.1 TeV.  Behind that onset F_e is smooth but not analytic: up to the next kink,
//       0.1 TeV, the panels are h/16 (h/8 reaches 1e-9 of the integral, h misses by 6e-8).
// The delta branch starts at ln(m_pi / E) for E < m_pi.
//
// Results are the converged integrals to 1e-8 (tests/test_gpu_kelner_leptons.py, against
// tests/kelner_leptons_np.py, which mpmath certifies; figures in profiles/NOTES_kelner_leptons.md).
#include "nh_kelner.h"

namespace {

constexpr double K06L_R = 0.573;     // 1 - lambda
constexpr double K06L_LAM = 0.427;   // 1 - (m_mu / m_pi)^2
constexpr int K06L_KINKS = 6;        // k06_integral's four, t_lambda, and t_r or F_e's onset
constexpr double K06L_FE_ONSET_TEV = 0.03628163947348171;  // 0.201 + 0.062 L + 0.00042 L^2 = 0
constexpr double K06L_ONSET_SUB = 16.0;
enum { K06L_E = 1, K06L_NUE = 2, K06L_NUMU1 = 4, K06L_ALL = 7 };

// KAB06 Eq. 62-65 at x = exp(-t):
//   B (1 + k t^2)^3 t^5 exp((1 - beta) t) / (exp(-beta t) + 0.3)   (regular at t -> 0, no overflow)
__device__ __forceinline__ double k06l_Fe(double t, double Ep) {
  const double L = log(Ep);
  const double base = 0.201 + 0.062 * L + 0.00042 * L * L;
  if (!(base > 0.0)) return 0.0;
  const double B = 1.0 / (69.5 + 2.65 * L + 0.3 * L * L);
  const double beta = 1.0 / sqrt(sqrt(base));
  const double k = (0.279 + 0.141 * L + 0.0172 * L * L) / (0.3 + (2.3 + L) * (2.3 + L));
  const double t2 = t * t, p = 1.0 + k * t2;
  return B * (p * p * p) * (t2 * t2 * t) * exp((1.0 - beta) * t) / (exp(-beta * t) + 0.3);
}

// KAB06 Eq. 66-69 at y = x / lambda = exp(-s): F_gamma's form in y, so k06_Fgamma's
// rearrangement with the primed coefficients
__device__ __forceinline__ double k06l_Fnumu1(double s, double Ep) {
  const double L = log(Ep);
  const double B = 1.75 + 0.204 * L + 0.010 * L * L;
  const double beta = 1.0 / (1.67 + 0.111 * L + 0.0038 * L * L);
  const double k = 1.07 - 0.086 * L + 0.002 * L * L;
  const double xb = exp(-beta * s);
  const double omx = -expm1(-beta * s);
  const double D = 1.0 + k * xb * omx;
  const double G = omx / D;
  return B * exp(s) * (G * G * G) * (G + (4.0 * beta * s * xb / D) * (1.0 + k * (1.0 - 2.0 * xb) * G));
}

// the decay distributions of a relativistic pion at x = exp(-t); ``low``: x < r
__device__ __forceinline__ double k06l_fe(double x, double t, bool low) {
  constexpr double r = K06L_R;
  constexpr double c = (3.0 - 2.0 * r) / (9.0 * (1.0 - r) * (1.0 - r));
  if (!low) return c * (9.0 * x * x + 6.0 * t - 4.0 * x * x * x - 5.0);
  const double h1 = c * (9.0 * r * r - 6.0 * log(r) - 4.0 * r * r * r - 5.0);
  return h1 + (1.0 + 2.0 * r) * (r - x) / (9.0 * r * r) *
                  (9.0 * (r + x) - 4.0 * (r * r + r * x + x * x));
}
__device__ __forceinline__ double k06l_fnue(double x, double t, bool low) {
  constexpr double r = K06L_R;
  constexpr double c = 2.0 / (3.0 * (1.0 - r) * (1.0 - r));
  if (!low)
    return c * ((1.0 - x) * (6.0 * (1.0 - x) * (1.0 - x) + r * (5.0 + 5.0 * x - 4.0 * x * x)) -
                6.0 * r * t);
  const double he1 =
      c * ((1.0 - r) * (6.0 - 7.0 * r + 11.0 * r * r - 4.0 * r * r * r) + 6.0 * r * log(r));
  return he1 + 2.0 * (r - x) / (3.0 * r * r) *
                   (7.0 * r * r - 4.0 * r * r * r + 7.0 * x * r - 4.0 * x * r * r - 2.0 * x * x -
                    4.0 * x * x * r);
}

__device__ __forceinline__ double k06l_finite(double f) {
  return (!(f == f) || isinf(f)) ? 0.0 : f;  // overflowed tails contribute nothing
}

// The components in ``mask`` at E [TeV], 1/(s TeV) per unit n_H, by the full calculation (v[1],
// nu_e, is then v[0]: F_nue ~= F_e) or by the delta-functional one with nhat = 1.
__device__ void k06l_integral(bool full, int mask, int kind, const pd_par& p, double E, int lane,
                              double v[3]) {
  const double t_lam = -log(K06L_LAM), t_r = -log(K06L_R);
  // E_pi = E exp(t) >= m_pi
  const double t0 = full ? 0.0 : fmax(log(K06_MPI_TEV / E), 0.0);
  const double Estart = full ? E : K06_MP_TEV + E * exp(t0) / K06_KPI;
  const double tend = t0 + K06_PANELS * K06_H;
  // proton energy [TeV] -> t (one the range never reaches: below its start, -inf or NaN)
  auto t_of = [&](double Ep) { return full ? log(Ep / E) : log((Ep - K06_MP_TEV) * K06_KPI / E); };

  // the kinks inside (t0, tend); one that is absent is NaN and never chosen
  double tk[K06L_KINKS];
  tk[0] = pd_has_break(kind) ? t_of(p.eb * 1e-12) : __builtin_nan("");
  tk[1] = t_of(K06_SIGMA_SWITCH_TEV);
  tk[2] = t_of(K06_ETH_TEV);
  tk[3] = __builtin_nan("");
  tk[4] = t_lam;
  tk[5] = full ? t_of(K06L_FE_ONSET_TEV) : t_r;
  // a steep cut-off, as in k06_integral (d ln Ep / dt <= 1 in both branches)
  double h_cut = K06_H;
  if (pd_has_cutoff(kind)) {
    const double x0 = pow(Estart / (p.ec * 1e-12), p.be);
    if (p.be * x0 > 2.0) {
      tk[3] = t_of(Estart * pow(1.0 + K06_CUT_EFOLDS / x0, 1.0 / p.be));
      h_cut = 1.0 / (p.be * x0);
    }
  }
  // stretch s ends at the s-th kink in ascending order; the last one is the plain h-grid
  double sa[K06L_KINKS + 1], sw[K06L_KINKS + 1];
  int sp[K06L_KINKS + 1];  // a stretch's first panel
  double cur = t0;
  int np = 0;
#pragma unroll
  for (int s = 0; s < K06L_KINKS; ++s) {
    double nx = tend;
#pragma unroll
    for (int c = 0; c < K06L_KINKS; ++c)
      if (tk[c] > cur && tk[c] < nx) nx = tk[c];
    sa[s] = cur;
    sw[s] = K06_H;
    sp[s] = np;
    if (nx < tend) {
      double hs = cur < tk[3] ? h_cut : K06_H;
      if (full && cur < tk[1]) hs = fmin(hs, K06_H / K06L_ONSET_SUB);  // F_e behind its onset
      const double cnt = fmin(fmax(ceil((nx - cur) / hs), 1.0), K06_SEG_PANELS_MAX);
      sw[s] = (nx - cur) / cnt;
      np += (int)cnt;
      cur = nx;
    }
  }
  sa[K06L_KINKS] = cur;
  sw[K06L_KINKS] = K06_H;
  sp[K06L_KINKS] = np;
  np += K06_PANELS;

  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int n = lane; n < np * 8; n += 64) {
    const int pan = n >> 3, q = n & 7;
    double a = sa[0], w = sw[0];
    int first = 0;
#pragma unroll
    for (int s = 1; s <= K06L_KINKS; ++s)
      if (pan >= sp[s]) a = sa[s], w = sw[s], first = sp[s];
    const double t = a + (pan - first + 0.5 * (1.0 + GLX[q])) * w;
    const bool mu_on = (mask & K06L_NUMU1) && a >= t_lam;  // the stretch starts behind t_lambda
    const double gw = GLW[q] * w;
    if (full) {
      const double Ep = E * exp(t);
      const double sj = k06_sigma_inel(Ep) * k06_J(kind, p, Ep);
      if (mask & (K06L_E | K06L_NUE)) a0 += gw * k06l_finite(sj * k06l_Fe(t, Ep));
      if (mu_on) a2 += gw * k06l_finite(sj * k06l_Fnumu1(t - t_lam, Ep));
    } else {
      const double Ep0 = K06_MP_TEV + E * exp(t) / K06_KPI;
      const double sj = k06_sigma_inel(Ep0) * k06_J(kind, p, Ep0);
      const double x = exp(-t);
      const bool low = a >= t_r;
      if (mask & K06L_E) a0 += gw * k06l_finite(sj * k06l_fe(x, t, low));
      if (mask & K06L_NUE) a1 += gw * k06l_finite(sj * k06l_fnue(x, t, low));
      if (mu_on) a2 += gw * k06l_finite(sj * (1.0 / K06L_LAM));
    }
  }
  const double sc = 0.5 * (full ? NH_C_CGS : 2.0 * NH_C_CGS / K06_KPI);
  v[0] = k06_wave_sum(a0) * sc;
  v[1] = full ? v[0] : k06_wave_sum(a1) * sc;
  v[2] = k06_wave_sum(a2) * sc;
}

// the components of product 0..3 (electron, nu_e, nu_mu, nu_all) on either side of Etrans
__device__ __forceinline__ int k06l_mask(int product, bool full) {
  const int m = product == 0 ? K06L_E
              : product == 1 ? K06L_NUE
              : product == 2 ? (K06L_E | K06L_NUMU1) : K06L_ALL;
  return full && (m & K06L_NUE) ? (m | K06L_E) : m;
}

__global__ __launch_bounds__(256) void k_pp_leptons_kelner06(
    int kind, const double* __restrict__ params, int N, const double* __restrict__ E_eV, int nE,
    double Etrans_TeV, int match, int product, double* __restrict__ out, int ldo,
    double* __restrict__ nhat_out) {
  extern __shared__ double res[];  // [nE + 2][3]: spectra | full(Etrans) | delta(Etrans)
  const int wi = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double* pr = params + (long long)wi * NH_PD_NPAR;
  const pd_par p = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6]};
  for (int task = wv; task < nE + 2; task += 4) {
    double v[3] = {0.0, 0.0, 0.0};
    if (task < nE) {
      const double E = E_eV[task] * 1e-12;
      const bool full = E >= Etrans_TeV;
      k06l_integral(full, k06l_mask(product, full), kind, p, E, lane, v);
    } else if (match) {
      k06l_integral(task == nE, K06L_ALL, kind, p, Etrans_TeV, lane, v);
    }
    if (lane == 0) {
      res[3 * task] = v[0];
      res[3 * task + 1] = v[1];
      res[3 * task + 2] = v[2];
    }
  }
  __syncthreads();
  // each component's delta branch meets its full one at Etrans (nu_e meets F_e)
  const double* fu = res + 3 * nE;
  const double* de = fu + 3;
  const double nh_e = match ? fu[0] / de[0] : 1.0;
  const double nh_ne = match ? fu[1] / de[1] : 1.0;
  const double nh_m = match ? fu[2] / de[2] : 1.0;
  for (int k = threadIdx.x; k < nE; k += blockDim.x) {
    const bool hi = E_eV[k] * 1e-12 >= Etrans_TeV;
    const double e = hi ? res[3 * k] : res[3 * k] * nh_e;
    const double ne = hi ? res[3 * k + 1] : res[3 * k + 1] * nh_ne;
    const double m = hi ? res[3 * k + 2] : res[3 * k + 2] * nh_m;
    const double s = product == 0 ? e : product == 1 ? ne : product == 2 ? e + m : e + ne + m;
    out[(long long)wi * ldo + k] = s * 1e-12;  // 1/(s TeV) -> 1/(s eV)
  }
  if (threadIdx.x == 0 && nhat_out) {
    nhat_out[3 * (long long)wi] = nh_e;
    nhat_out[3 * (long long)wi + 1] = nh_ne;
    nhat_out[3 * (long long)wi + 2] = nh_m;
  }
}

}  // namespace

extern "C" int nh_pp_leptons_kelner06(nh_ctx* c, int kind, const double* params, int N,
                                      const double* E_eV, int nE, double Etrans_eV, int match,
                                      int product, double* out, int ldo, double* nhat_out) {
  NH_REQUIRE(c && params && E_eV && out, "NULL pointer");
  NH_REQUIRE(kind >= NH_PD_POWERLAW && kind <= NH_PD_LOGPARABOLA, "unknown particle distribution kind");
  NH_REQUIRE(product >= 0 && product <= 3, "product outside 0..3 (electron, nu_e, nu_mu, nu_all)");
  NH_REQUIRE(N >= 0 && nE >= 1 && ldo >= nE && Etrans_eV > 0.0, "bad sizes");
  NH_REQUIRE(((size_t)nE + 2) * 3 * sizeof(double) <= 60 * 1024, "too many energies per call");
  if (N == 0) return NH_OK;
  nh_prof_scope ps(c, NH_K_TABLES);
  hipLaunchKernelGGL(k_pp_leptons_kelner06, dim3((unsigned)N), dim3(256),
                     (nE + 2) * 3 * sizeof(double), c->stream, kind, params, N, E_eV, nE,
                     Etrans_eV * 1e-12, match != 0, product, out, ldo, nhat_out);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
