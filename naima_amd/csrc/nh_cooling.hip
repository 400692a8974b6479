// nh_cooling.hip -- cooled electron populations, per walker.
//
// An injection rate Q(E) [1/(eV s)] that has been switched on for a time `age` under the energy
// loss rate b(E) = -dE/dt [eV/s] leaves the population (Kardashev 1962; GAMERA's constant-loss
// case)
//   n(E) = [S(E) - S(E*)] / b(E),  S(E) = int_E^Emax Q dE',  T(E) = int_E^Emax dE'/b,
// where E* is the energy an electron now at E was injected with at the start: T(E*) = T(E) - age,
// and E* = Emax (S = 0) when T(E) <= age, which includes age = inf, the steady state.  Injection
// above Emax is ignored.
//   b(E) = (4/3) sigma_T c (B^2 / 8 pi) gamma^2 + sum_f u_f loss_f(E)
// with loss_f the inverse-Compton loss per unit energy density of field f (Klein-Nishina
// included; models.CooledElectrons builds it from the project's own IC emissivity).
//
// Everything is the power-law-per-segment picture of trapz_loglog (utils.py:336-348) on the
// model's own grid: Q and 1/b are power laws inside a segment, S and T are suffix sums of the
// segment terms (log branch for |slope + 1| <= 1e-10, a zero node ends a segment), and inside
// the segment that holds E* both E* and the partial integral of Q are closed forms.  The
// integral of Q over [E_i, E*] is summed as (whole segments i .. j-1, a difference of the suffix
// sums AT NODES) + (the partial segment j); when E* lies in E_i's own segment it is that
// segment's closed form alone, so that n -> Q age for age far below the cooling time instead of
// the difference of two nearly equal numbers.
//
//   nh_cooled_electrons   one workgroup of 256 threads per walker; ln E, Q, 1/b, S and T in LDS
//                         (40 B per node, 80 KiB at the cap of 2048 nodes).  The scans run in a
//                         fixed order: every thread sums a run of nodes, a wave-level scan of the
//                         runs' totals, a carry across the four waves -- the same bits at every
//                         call, no atomics on data.
//   nh_cooled_weights     the solution resampled onto a radiative class's particle grid by
//                         log-log linear interpolation: w = xg unit_scale n and dlw, with
//                         NH_DL_ZERO wherever a neighbour is zero (what _weights_table writes).
//   nh_cooled_ic_rows     the isotropic IC kernel of every electron on its own row of outgoing
//                         photon energies, from which models.CooledElectrons reduces loss_f.
//
// FP64, deterministic, on the context's stream.  Measured differences against the NumPy
// restatement: profiles/NOTES_cooling.md, tests/test_gpu_cooling.py.
#include "nh_common.h"

#include <cmath>

#include "nh_ic.h"

namespace {

constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / 64;
constexpr int CE_MAX_NODES = 2048;
constexpr double CE_SIGMA_T = 8.0 * NH_PI / 3.0 * NH_R0_CM * NH_R0_CM;
// b_syn [eV/s] = CE_SYN B^2 E^2 (B in gauss, E in eV)
constexpr double CE_SYN = (4.0 / 3.0) * CE_SIGMA_T * NH_C_CGS / (8.0 * NH_PI) * NH_ERG_TO_EV_ /
                          (NH_MEC2_EV * NH_MEC2_EV);

struct ce_args {
  const double* Q;
  long long ldq;
  int N, nC, nf;
  const double* e;
  nh_lazy B, age;
  const double* loss;
  nh_lazy u[NH_MAX_COMP];
  double* out;
  int* status;
};

// one segment of trapz_loglog (utils.py:336-348) from its nodes and lx = ln(x2/x1)
__device__ __forceinline__ double ce_seg(double x1, double x2, double y1, double y2, double lx) {
#pragma clang fp contract(off)
  if (y1 == 0.0 || y2 == 0.0) return 0.0;
  const double s1 = log(y2 / y1) / lx + 1.0;
  if (fabs(s1) > 1e-10) return (x2 * y2 - x1 * y1) / s1;
  return x1 * y1 * lx;
}

// int of the segment's power law through (x1, y1) with slope + 1 = s1, over z = ln(x / x1)
__device__ __forceinline__ double ce_part(double x1, double y1, double s1, double z) {
#pragma clang fp contract(off)
  if (fabs(s1) > 1e-10) return x1 * y1 * expm1(s1 * z) / s1;
  return x1 * y1 * z;
}

__global__ __launch_bounds__(CE_THREADS) void k_cooled_electrons(ce_args A) {
#pragma clang fp contract(off)
  extern __shared__ double ce_smem[];
  const int nC = A.nC;
  double* L = ce_smem;          // ln E
  double* Qs = L + nC;          // Q
  double* R = Qs + nC;          // 1 / b
  double* S = R + nC;           // int_E^Emax Q
  double* T = S + nC;           // int_E^Emax 1/b
  double* carry = T + nC;       // [CE_WAVES][2]
  __shared__ int ce_bad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long w = blockIdx.x;
  double* o = A.out + w * (long long)nC;

  // ---- the walker's scalars and its domain ------------------------------------------------
  const double B = nh_lazy_eval(A.B, w), age = nh_lazy_eval(A.age, w);
  bool bad = !(age > 0.0) || !(B == B) || isinf(B);
  bool anyu = false;
  double uf[NH_MAX_COMP];
#pragma unroll
  for (int f = 0; f < NH_MAX_COMP; ++f) {
    uf[f] = 0.0;
    if (f < A.nf) {
      uf[f] = nh_lazy_eval(A.u[f], w);
      bad = bad || !(uf[f] >= 0.0) || isinf(uf[f]);
      anyu = anyu || uf[f] > 0.0;
    }
  }
  bad = bad || (!(B > 0.0) && !anyu);
  if (t == 0) ce_bad = 0;
  __syncthreads();

  // ---- nodes: ln E, Q, 1/b ------------------------------------------------------------------
  if (!bad) {
    const double cs = CE_SYN * (B * B);
    const double* q = A.Q + w * A.ldq;
    for (int i = t; i < nC; i += CE_THREADS) {
      const double E = A.e[i];
      double b = cs * (E * E);
#pragma unroll
      for (int f = 0; f < NH_MAX_COMP; ++f)
        if (f < A.nf) b = b + uf[f] * A.loss[(long long)f * nC + i];
      if (!(b > 0.0) || isinf(b)) ce_bad = 1;  // (b has to be positive everywhere)
      L[i] = log(E);
      Qs[i] = q[i];
      R[i] = 1.0 / b;
    }
  }
  __syncthreads();
  if (bad || ce_bad) {
    for (int i = t; i < nC; i += CE_THREADS) o[i] = __builtin_nan("");
    if (t == 0) atomicAdd(A.status, 1);
    return;
  }

  // ---- segment terms of S and T (node i holds segment (i, i+1); the last node holds 0) ------
  for (int i = t; i < nC; i += CE_THREADS) {
    double ts = 0.0, tt = 0.0;
    if (i + 1 < nC) {
      const double x1 = A.e[i], x2 = A.e[i + 1], lx = L[i + 1] - L[i];
      ts = ce_seg(x1, x2, Qs[i], Qs[i + 1], lx);
      tt = ce_seg(x1, x2, R[i], R[i + 1], lx);
    }
    S[i] = ts;
    T[i] = tt;
  }
  __syncthreads();

  // ---- suffix sums, in a fixed order: thread t owns the nodes nC-1 - (t ch + c), c < ch ------
  {
    const int ch = (nC + CE_THREADS - 1) / CE_THREADS;
    double sS = 0.0, sT = 0.0;
    for (int c = 0; c < ch; ++c) {
      const int k = t * ch + c;
      if (k < nC) {
        const int i = nC - 1 - k;
        sS = sS + S[i];
        S[i] = sS;
        sT = sT + T[i];
        T[i] = sT;
      }
    }
    double aS = sS, aT = sT;  // inclusive scan of the runs' totals over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double vS = __shfl_up(aS, off, 64), vT = __shfl_up(aT, off, 64);
      if (lane >= off) {
        aS = aS + vS;
        aT = aT + vT;
      }
    }
    if (lane == 63) {
      carry[2 * wave] = aS;
      carry[2 * wave + 1] = aT;
    }
    double eS = __shfl_up(aS, 1, 64), eT = __shfl_up(aT, 1, 64);  // the runs before this one
    if (lane == 0) eS = eT = 0.0;
    __syncthreads();
    double cS = 0.0, cT = 0.0;  // the waves before this one
    for (int v = 0; v < wave; ++v) {
      cS = cS + carry[2 * v];
      cT = cT + carry[2 * v + 1];
    }
    eS = cS + eS;
    eT = cT + eT;
    for (int c = 0; c < ch; ++c) {
      const int k = t * ch + c;
      if (k < nC) {
        const int i = nC - 1 - k;
        S[i] = eS + S[i];
        T[i] = eT + T[i];
      }
    }
  }
  __syncthreads();

  // ---- the solution at every node -----------------------------------------------------------
  for (int i = t; i < nC; i += CE_THREADS) {
    const double Ti = T[i];
    double I;  // int_{E_i}^{E*} Q dE
    if (Ti <= age) {
      I = S[i];  // E* = Emax
    } else {
      // j: the last node the electron passed on its way down, T_i - T_j <= age < T_i - T_{j+1}
      int lo = i, hi = nC - 1;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (Ti - T[mid] <= age) lo = mid; else hi = mid;
      }
      const int j = lo;
      const double rem = j == i ? age : age - (Ti - T[j]);  // the time spent inside segment j
      const double lx = L[j + 1] - L[j];
      const double xj = A.e[j], rj = R[j];
      // E* = xj exp(z): rj xj (exp(p1 z) - 1) / p1 = rem with 1/b ~ E^(p1 - 1) in the segment
      const double p1 = log(R[j + 1] / rj) / lx + 1.0;
      double z = fabs(p1) > 1e-10 ? log1p(rem * p1 / (rj * xj)) / p1 : rem / (rj * xj);
      z = fmin(fmax(z, 0.0), lx);
      const double qj = Qs[j], qn = Qs[j + 1];
      double part = 0.0;
      if (qj != 0.0 && qn != 0.0) part = ce_part(xj, qj, log(qn / qj) / lx + 1.0, z);
      I = j == i ? part : (S[i] - S[j]) + part;
    }
    o[i] = I * R[i];
  }
}

// one workgroup per walker: the solve grid's logarithms in LDS, the target nodes by thread
__global__ __launch_bounds__(CE_THREADS) void k_cooled_weights(
    const double* __restrict__ n, const double* __restrict__ ec, int nC, int N,
    const double* __restrict__ e, const double* __restrict__ xg, int nG, double unit_scale,
    double* __restrict__ wout, double* __restrict__ dlw) {
#pragma clang fp contract(off)
  const long long w = blockIdx.x;
  const double* nr = n + w * (long long)nC;
  double* wr = wout + w * (long long)nG;
  double* dr = dlw + w * (long long)nG;
  const double e0 = ec[0], e1 = ec[nC - 1];
  for (int g = threadIdx.x; g < nG; g += CE_THREADS) {
    const double E = e[g];
    double v = 0.0;
    if (E >= e0 && E <= e1) {
      int lo = 0, hi = nC - 1;  // ec[lo] <= E <= ec[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ec[mid] <= E) lo = mid; else hi = mid;
      }
      const double x1 = ec[lo], x2 = ec[hi], y1 = nr[lo], y2 = nr[hi];
      if (E == x1) {
        v = y1;
      } else if (E == x2) {
        v = y2;
      } else if (y1 == 0.0 || y2 == 0.0) {
        v = (y1 == y1 && y2 == y2) ? 0.0 : __builtin_nan("");
      } else {
        v = y1 * exp(log(y2 / y1) / log(x2 / x1) * log(E / x1));
      }
    } else if (!(E == E)) {
      v = E;
    }
    wr[g] = xg[g] * unit_scale * v;
  }
  __syncthreads();  // (the row this workgroup has just written)
  for (int g = threadIdx.x; g < nG; g += CE_THREADS) {
    double d = 0.0;
    if (g + 1 < nG) {
      const double a = wr[g], b = wr[g + 1];
      d = log(fabs(b / a));
      if (a == 0.0 || b == 0.0 || !(d == d) || isinf(d)) d = NH_DL_ZERO;
    }
    dr[g] = d;
  }
}

// Kt[i][k]: the isotropic Khangulyan kernel (nh_ic.h, what nh_table_ic_planck tabulates) of the
// electron gam[i] at the outgoing photon energy gam[i] z[k] -- every electron on its own photon
// grid, a fixed grid in the fraction z of its energy
__global__ __launch_bounds__(256) void k_cooled_ic_rows(const double* __restrict__ gam, int nC,
                                                         const double* __restrict__ z, int nE,
                                                         double Tp, double* __restrict__ Kt, int ld) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)nC * nE) return;
  const int i = (int)(idx / nE), k = (int)(idx % nE);
  const double g = gam[i];
  Kt[(long long)i * ld + k] = ic_planck_K(g, g * z[k], Tp, 0.0, true);
}

}  // namespace

extern "C" int nh_cooled_ic_rows(nh_ctx* c, const double* gam, int nC, const double* z, int nE,
                                 double T_K, double* Kt, int ld) {
  NH_REQUIRE(c && gam && z && Kt, "null argument");
  NH_REQUIRE(nC >= 1 && nE >= 1 && ld >= nE, "bad shape");
  NH_REQUIRE(T_K > 0.0, "the field's temperature must be positive");
  nh_prof_scope ps(c, NH_K_TABLES);
  const long long tot = (long long)nC * nE;
  NH_REQUIRE(tot <= 0x7fffffffLL * 256, "too many (electron, photon) pairs");
  hipLaunchKernelGGL(k_cooled_ic_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                     gam, nC, z, nE, T_K * NH_K_TO_MEC2, Kt, ld);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_cooled_electrons(nh_ctx* c, const double* Q, long long ldq, int N,
                                   const double* e_eV, int nC, const nh_lazy* B_G,
                                   const double* loss, int nf, const nh_lazy* u,
                                   const nh_lazy* age_s, double* n_out, int* status) {
  NH_REQUIRE(c && Q && e_eV && B_G && age_s && n_out && status, "null argument");
  NH_REQUIRE(nC >= 2 && nC <= CE_MAX_NODES, "the solve grid has 2 .. 2048 nodes");
  NH_REQUIRE(nf >= 0 && nf <= NH_MAX_COMP && (nf == 0 || (loss && u)), "nf must be 0..8");
  NH_REQUIRE(N >= 0 && (ldq == 0 || ldq >= nC), "bad shape");
  if (N == 0) return NH_OK;
  ce_args A;
  memset(&A, 0, sizeof A);
  A.Q = Q;
  A.ldq = ldq;
  A.N = N;
  A.nC = nC;
  A.nf = nf;
  A.e = e_eV;
  A.B = *B_G;
  A.age = *age_s;
  A.loss = loss;
  for (int f = 0; f < nf; ++f) A.u[f] = u[f];
  A.out = n_out;
  A.status = status;
  const size_t shm = (size_t)(5 * nC + 2 * CE_WAVES) * sizeof(double);
  if (shm > 64 * 1024)
    NH_CHECK_HIP(hipFuncSetAttribute((const void*)k_cooled_electrons,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  nh_prof_scope ps(c, NH_K_COOLING);
  hipLaunchKernelGGL(k_cooled_electrons, dim3((unsigned)N), dim3(CE_THREADS), shm, c->stream, A);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_cooled_weights(nh_ctx* c, const double* n, const double* e_c, int nC, int N,
                                 const double* e_eV, const double* xg, int nG, double unit_scale,
                                 double* w, double* dlw) {
  NH_REQUIRE(c && n && e_c && e_eV && xg && w && dlw, "null argument");
  NH_REQUIRE(nC >= 2 && nG >= 1 && N >= 0, "bad shape");
  if (N == 0) return NH_OK;
  nh_prof_scope ps(c, NH_K_COOLING);
  hipLaunchKernelGGL(k_cooled_weights, dim3((unsigned)N), dim3(CE_THREADS), 0, c->stream, n, e_c,
                     nC, N, e_eV, xg, nG, unit_scale, w, dlw);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
