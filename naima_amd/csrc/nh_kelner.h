// nh_kelner.h -- what the Kelner, Aharonian & Bugayov 2006 kernels share: the constants, the
// Gauss-Legendre nodes, the inelastic cross section, the proton spectrum at a node, the gamma-ray
// kernel function and the wave reduction (nh_kelner.hip: pi0 -> gamma gamma;
// nh_kelner_leptons.hip: pi+- -> mu nu -> e nu nu)
#pragma once
#include "nh_pdist.h"

namespace {

constexpr double K06_KPI = 0.17;                       // radiative.py:1689
constexpr double K06_MP_TEV = NH_M_P_GEV * 1e-3;       // :1690
constexpr double K06_MPI_TEV = 1.349766e-4;            // :1691
constexpr double K06_ETH_TEV = 1.22e-3;                // :1643
constexpr int K06_PANELS = 128;
constexpr double K06_H = 0.5;
constexpr int K06_KINKS = 4;                           // e_break, 0.1 TeV, threshold, steep cut-off
constexpr double K06_SEG_PANELS_MAX = 8.0 * K06_PANELS;  // per stretch between two kinks
constexpr double K06_SIGMA_SWITCH_TEV = 0.1;           // :1640
constexpr double K06_CUT_EFOLDS = 40.0;                // exp(-40): nothing left of the integrand

__constant__ double GLX[8] = {-0.9602898564975363, -0.7966664774136267, -0.5255324099163290,
                              -0.1834346424956498, 0.1834346424956498,  0.5255324099163290,
                              0.7966664774136267,  0.9602898564975363};
__constant__ double GLW[8] = {0.1012285362903763, 0.2223810344533745, 0.3137066458778873,
                              0.3626837833783620, 0.3626837833783620, 0.3137066458778873,
                              0.2223810344533745, 0.1012285362903763};

// KAB06 Eq. 73, 79 (radiative.py:1625-1647), cm^2
__device__ __forceinline__ double k06_sigma_inel(double Ep) {
  const double L = log(Ep);
  double s = 34.3 + 1.88 * L + 0.25 * L * L;
  if (Ep <= K06_SIGMA_SWITCH_TEV) {
    const double r = K06_ETH_TEV / Ep, r2 = r * r;
    const double f = 1.0 - r2 * r2;
    s *= f * f * nh_heaviside(Ep - K06_ETH_TEV);
  }
  return s * 1e-27;
}

// particles per TeV at Ep [TeV]
__device__ __forceinline__ double k06_J(int kind, const pd_par& p, double Ep_TeV) {
  const double E = Ep_TeV * 1e12;
  double n, dsh;
  pd_node(kind, p, E, E, 0.0, n, dsh);
  return n * 1e12;
}

// KAB06 Eq. 58-61 (radiative.py:1597-1623) at x = exp(-t): F1*F2 rearranged so that the
// 1/ln(x) and 1/(1 - x^beta) factors cancel analytically (regular as t -> 0):
//   F = (B/x) G^3 [ G + (4 beta t xb / D)(1 + k (1 - 2 xb) G) ],
//   xb = x^beta, D = 1 + k xb (1 - xb), G = (1 - xb)/D
__device__ __forceinline__ double k06_Fgamma(double t, double Ep) {
  const double L = log(Ep);
  const double B = 1.30 + 0.14 * L + 0.011 * L * L;
  const double beta = 1.0 / (1.79 + 0.11 * L + 0.008 * L * L);
  const double k = 1.0 / (0.801 + 0.049 * L + 0.014 * L * L);
  const double xb = exp(-beta * t);
  const double omx = -expm1(-beta * t);
  const double D = 1.0 + k * xb * omx;
  const double G = omx / D;
  return B * exp(t) * (G * G * G) * (G + (4.0 * beta * t * xb / D) * (1.0 + k * (1.0 - 2.0 * xb) * G));
}

__device__ __forceinline__ double k06_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

}  // namespace
