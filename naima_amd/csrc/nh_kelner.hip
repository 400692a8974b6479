// nh_kelner.hip -- PionDecayKelner06._spectrum (radiative.py:1543-1767): Kelner, Aharonian
// & Bugayov 2006 parametrisation of pp -> pi0 -> gamma gamma.
//
// The reference integrates with adaptive QUADPACK (scipy.integrate.quad, epsrel = 1e-3)
// one photon energy at a time.  Here every (walker, photon energy) pair is one wave that
// evaluates the same integrals with a fixed composite Gauss-Legendre rule after a change
// of variable that makes the integrands smooth and exponentially decaying:
//   E_gamma >= Etrans (Eq. 71/72, :1665-1684):  int_0^1 sigma J F dx/x,   x = exp(-t)
//       -> int_0^T sigma(Ep) J(Ep) F(x, Ep) dt,  Ep = E_gamma exp(t)
//   E_gamma <  Etrans (delta-functional, :1693-1714):
//       2 int_{Epimin}^inf q_pi / sqrt(Epi^2 - m_pi^2) dEpi,  Epi = m_pi cosh(s)
//       -> 2 int_{s_min}^{s_min+T} q_pi(m_pi cosh s) ds      (the root singularity is gone)
// T = 64 (the integrands fall like exp(-(alpha-1) t)), panels of h = 0.5 x 8 points.
//
// A fixed rule converges spectrally only where the integrand is smooth inside every panel, so
// no panel straddles a kink: the break energy of the broken power laws (a jump of the slope)
// and the two of k06_sigma_inel (0.1 TeV, where it changes form with a relative jump of
// 4.4e-8, and the 1.22e-3 TeV threshold).  Each is mapped to the integration variable; the
// stretch up to it is cut into ceil(length / h) equal panels and the h-grid starts again
// behind it.  Without this a broken power law was 1e-4 off, with a sign and size that changed
// as e_break moved across panel edges.  A cut-off that is already steep where the range
// starts -- beta (E/e_cutoff)^beta > 2, a photon energy beyond the cut-off -- is resolved in
// the same way: the 40 e-foldings in which it kills the integrand get panels of its own
// e-folding length in t.
//
// The result is the CONVERGED integral to 1e-8 (tests/test_gpu_kelner.py: every kind, against
// a reference certified by mpmath; measured figures in profiles/NOTES_kelner.md): it differs
// from the reference's number by the reference's own quadrature error (measured 4e-5, bound
// 1e-3); tests/test_oracle.py pins both.
#include "nh_kelner.h"

namespace {

// proton energy [TeV] -> integration variable: the inverse of the node maps in k06_integral
// (an energy the variable never reaches gives a value at or below the range's start, or NaN)
__device__ __forceinline__ double k06_t_of(int mode, double Ep, double Eg) {
  if (mode == 0) return log(Ep / Eg);
  if (mode == 1) return acosh(fmax((Ep - K06_MP_TEV) * K06_KPI / K06_MPI_TEV, 1.0));
  return log(Ep / K06_ETH_TEV);
}

// mode 0: full calculation at E_gamma; mode 1: delta-functional (nhat = 1); mode 2: Wp
__device__ double k06_integral(int mode, int kind, const pd_par& p, double Eg, int lane) {
  double t0 = 0.0, Estart = mode == 0 ? Eg : K06_ETH_TEV;
  if (mode == 1) {
    const double Epimin = Eg + K06_MPI_TEV * K06_MPI_TEV / (4.0 * Eg);
    t0 = acosh(fmax(Epimin / K06_MPI_TEV, 1.0));
    Estart = K06_MP_TEV + Epimin / K06_KPI;
  }
  // Wp's integrand falls only like exp(-(alpha-2) t): eight times the range
  const int panels = mode == 2 ? 8 * K06_PANELS : K06_PANELS;
  const double tend = t0 + panels * K06_H;

  // the kinks inside (t0, tend); one that is absent is NaN and never chosen
  double tk[K06_KINKS];
  tk[0] = pd_has_break(kind) ? k06_t_of(mode, p.eb * 1e-12, Eg) : __builtin_nan("");
  tk[1] = k06_t_of(mode, K06_SIGMA_SWITCH_TEV, Eg);
  tk[2] = k06_t_of(mode, K06_ETH_TEV, Eg);
  tk[3] = __builtin_nan("");
  // a steep cut-off: up to tk[3], where it has fallen by K06_CUT_EFOLDS, panels of width h_cut
  // (d ln E / dt <= 1 in every mode, so 1 / (beta x0) is at most its e-folding length in t)
  double h_cut = K06_H;
  if (pd_has_cutoff(kind)) {
    const double x0 = pow(Estart / (p.ec * 1e-12), p.be);
    if (p.be * x0 > 2.0) {
      tk[3] = k06_t_of(mode, Estart * pow(1.0 + K06_CUT_EFOLDS / x0, 1.0 / p.be), Eg);
      h_cut = 1.0 / (p.be * x0);
    }
  }
  // stretch s = 0..K06_KINKS-1 ends at the s-th kink in ascending order (empty when there
  // are fewer); the last one is the plain h-grid behind the last kink
  double sa[K06_KINKS + 1], sw[K06_KINKS + 1];
  int sp[K06_KINKS + 1];  // a stretch's first panel
  double cur = t0;
  int np = 0;
#pragma unroll
  for (int s = 0; s < K06_KINKS; ++s) {
    double nx = tend;
#pragma unroll
    for (int c = 0; c < K06_KINKS; ++c)
      if (tk[c] > cur && tk[c] < nx) nx = tk[c];
    sa[s] = cur;
    sw[s] = K06_H;
    sp[s] = np;
    if (nx < tend) {
      const double hs = cur < tk[3] ? h_cut : K06_H;
      const double cnt = fmin(fmax(ceil((nx - cur) / hs), 1.0), K06_SEG_PANELS_MAX);
      sw[s] = (nx - cur) / cnt;
      np += (int)cnt;
      cur = nx;
    }
  }
  sa[K06_KINKS] = cur;
  sw[K06_KINKS] = K06_H;
  sp[K06_KINKS] = np;
  np += panels;

  double acc = 0.0;
  for (int n = lane; n < np * 8; n += 64) {
    const int pan = n >> 3, q = n & 7;
    double a = sa[0], w = sw[0];
    int first = 0;
#pragma unroll
    for (int s = 1; s <= K06_KINKS; ++s)
      if (pan >= sp[s]) a = sa[s], w = sw[s], first = sp[s];
    const double t = a + (pan - first + 0.5 * (1.0 + GLX[q])) * w;
    double f;
    if (mode == 0) {
      const double Ep = Eg * exp(t);
      f = k06_sigma_inel(Ep) * k06_J(kind, p, Ep) * k06_Fgamma(t, Ep);
    } else if (mode == 1) {
      const double Ep0 = K06_MP_TEV + K06_MPI_TEV * cosh(t) / K06_KPI;
      f = k06_sigma_inel(Ep0) * k06_J(kind, p, Ep0);
    } else {
      const double E = K06_ETH_TEV * exp(t);  // int E J dE = int E^2 J dt
      f = E * E * k06_J(kind, p, E);
    }
    if (!(f == f) || isinf(f)) f = 0.0;  // overflowed tails contribute nothing
    acc += GLW[q] * w * f;
  }
  acc = k06_wave_sum(acc) * 0.5;
  if (mode == 0) return NH_C_CGS * acc;
  if (mode == 1) return 2.0 * NH_C_CGS / K06_KPI * acc;
  return acc;
}

__global__ __launch_bounds__(256) void k_pion_kelner06(int kind, const double* __restrict__ params,
                                                        int N, const double* __restrict__ E_eV,
                                                        int nE, double Etrans_TeV, int mixed,
                                                        double* __restrict__ out, int ldo,
                                                        double* __restrict__ nhat_out,
                                                        double* __restrict__ wp_out) {
  extern __shared__ double res[];  // [nE + 3]: spectra | full(Etrans) | delta(Etrans) | Wp
  const int wi = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double* pr = params + (long long)wi * NH_PD_NPAR;
  const pd_par p = {pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6]};
  for (int task = wv; task < nE + 3; task += 4) {
    double v = 0.0;
    if (task < nE) {
      const double Eg = E_eV[task] * 1e-12;
      v = k06_integral(Eg >= Etrans_TeV ? 0 : 1, kind, p, Eg, lane);
    } else if (task == nE) {
      if (mixed) v = k06_integral(0, kind, p, Etrans_TeV, lane);
    } else if (task == nE + 1) {
      if (mixed) v = k06_integral(1, kind, p, Etrans_TeV, lane);
    } else if (wp_out) {
      v = k06_integral(2, kind, p, 0.0, lane);
    }
    if (lane == 0) res[task] = v;
  }
  __syncthreads();
  // nhat makes the delta-functional branch meet the full one at Etrans (:1743-1748)
  const double nhat = mixed ? res[nE] / res[nE + 1] : 1.0;
  for (int k = threadIdx.x; k < nE; k += blockDim.x) {
    const bool hi = E_eV[k] * 1e-12 >= Etrans_TeV;
    out[(long long)wi * ldo + k] = (hi ? res[k] : res[k] * nhat) * 1e-12;  // 1/(s TeV) -> 1/(s eV)
  }
  if (threadIdx.x == 0) {
    if (nhat_out) nhat_out[wi] = nhat;
    if (wp_out) wp_out[wi] = res[nE + 2];
  }
}

}  // namespace

extern "C" int nh_pion_kelner06(nh_ctx* c, int kind, const double* params, int N,
                                const double* E_eV, int nE, double Etrans_eV, int mixed,
                                double* out, int ldo, double* nhat_out, double* wp_TeV_out) {
  NH_REQUIRE(c && params && E_eV && out, "NULL pointer");
  NH_REQUIRE(kind >= NH_PD_POWERLAW && kind <= NH_PD_LOGPARABOLA, "unknown particle distribution kind");
  NH_REQUIRE(N >= 0 && nE >= 1 && ldo >= nE && Etrans_eV > 0.0, "bad sizes");
  NH_REQUIRE((size_t)(nE + 3) * sizeof(double) <= 60 * 1024, "too many photon energies per call");
  if (N == 0) return NH_OK;
  nh_prof_scope ps(c, NH_K_TABLES);
  hipLaunchKernelGGL(k_pion_kelner06, dim3((unsigned)N), dim3(256), (nE + 3) * sizeof(double),
                     c->stream, kind, params, N, E_eV, nE, Etrans_eV * 1e-12, mixed, out, ldo,
                     nhat_out, wp_TeV_out);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
