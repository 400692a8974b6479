// nh_ssa.hip -- synchrotron self-absorption of a homogeneous one-zone source, per walker.
//
// For an isotropic population N(gamma) [per unit Lorentz factor] in a volume V the absorption
// coefficient, integrated by parts so that it holds no derivative of N (the edge terms of a
// truncated distribution are in it, and every node is non-negative), is
//   alpha(E) V = kappa(E) = pi^2 hbar^3 CS1(E) / (m_e E) * trapz_loglog((N/gamma) H(x), gamma)
//   H(x) = 2 Gtilde(x) (1 - D(x)),  D = dln Gtilde / dln x,  x = E / Ec(gamma, B)
// with CS1, Ec and Gtilde = P(x) exp(-x) those of the emission (nh_synchrotron.hip; AKP10 Eq.
// D7).  With c = cbrt(x), D = Dp(c) - x and
//   3 Dp = 1/(1 + 3.4 c^2) + (4.42 c^2 + 1.388 c^4)/gt2 - (2.706 c^2 + 0.868 c^4)/gt3,
// so H = 2 Q(x) exp(-x) with Q = P (1 + x - Dp) rational in c (but for P's square root): the
// node and the segment's log-ratio have the emission kernel's form with Q in the place of P,
//   u_i = (w_i / gamma_i) Q(x_i) exp(-x_i),   ln(u2/u1) = dlw_i - lx_i + ln(Q2/Q1) - (x2 - x1).
// Dp <= 1/3, so Q > 0.
//
//   nh_syn_absorption  kappa[w][k], cm^2: a kernel of its own with the mapping of k_synchrotron
//                      (one workgroup per walker and tile of <= 64 energies, live-energy
//                      compaction, chunks over the live range, the same LDS tables); no
//                      likelihood epilogue.  The launch shape is nh_synchrotron_plan's.
//   nh_ssa_apply       out[w][k] = f(tau_w[k]) colfac[k] sum_j comps[j]: the escape fraction of
//                      a homogeneous sphere (tau = 2 alpha R along a diameter, Gould 1979) or of
//                      a face-on slab; one wave per walker row.
//
// FP64, deterministic, no atomics, no scratch, on the context's stream.
#include "nh_syn.h"

namespace {

constexpr int SSA_MAXCH = 64;  // chunks per energy (LDS: part[SSA_MAXCH][64]), as SYN_MAXCH

// Q = P (1 + x - Dp) from cb = cbrt(x) and x: syn_P1's polynomials, one more reciprocal for
// the three denominators of Dp together.  Bn t34 gt3 and Cn t34 gt2 cancel to a few eps of
// 4 den at large c: 1e-15 absolute on Dp, next to the 3e-14 / 3 of the reciprocal.
__device__ __forceinline__ double ssa_Q1(double cb, double x) {
  const double cb2 = cb * cb;
  const double cb4 = cb2 * cb2;
  const double t34 = fma(3.4, cb2, 1.0);
  const double gt2 = fma(0.347, cb4, fma(2.210, cb2, 1.0));
  const double gt3 = fma(0.217, cb4, fma(1.353, cb2, 1.0));
  const double P = ((1.808 * cb) * gt2) * nh_rsqrt1((gt3 * gt3) * t34);
  const double Bn = fma(1.388, cb4, 4.42 * cb2);
  const double Cn = fma(0.868, cb4, 2.706 * cb2);
  const double g23 = gt2 * gt3;
  const double num = fma(t34, fma(Bn, gt3, -(Cn * gt2)), g23);
  const double Dp3 = num * nh_rcp1f(g23 * t34);
  return P * fma(Dp3, -1.0 / 3.0, 1.0 + x);
}

// k_synchrotron (nh_synchrotron.hip) without its epilogue and with the absorption's node
template <int C>
__global__ __launch_bounds__(64 * C) void k_syn_absorption(
    const double* __restrict__ w, const double* __restrict__ dlw, const double* __restrict__ B,
    int ldB, int N, const double* __restrict__ gam, const double* __restrict__ lx, int nG,
    const double* __restrict__ E_eV, int nE, double* __restrict__ out, int ldo, int tw) {
  extern __shared__ double smem[];  // ig2[nG] | dig2[nG] | ig23[nG] | part[SSA_MAXCH][64]
  double* ig2 = smem;
  double* dig2 = smem + nG;
  double* ig23 = smem + 2 * nG;
  double* part = smem + 3 * nG;
  __shared__ int amap[64];   // compacted live energy -> energy index
  __shared__ int ai0[64];    //                       -> its first segment that can contribute
  __shared__ int s_nA;
  __shared__ double T64[64];  // 2^(j/64): the table of nh_exp_tab
  constexpr int T = 64 * C;
  const int tid = threadIdx.x;
  for (int i = tid; i < nG; i += T) {
    const double g = gam[i];
    const double v = 1.0 / (g * g);
    ig2[i] = v;
    ig23[i] = cbrt(v);
    double d = 0.0;
    if (i + 1 < nG) {
      const double r = g / gam[i + 1];  // 1/g2^2 - 1/g1^2 without cancellation
      d = v * (r * r - 1.0);
    }
    dig2[i] = d;
  }
  if (tid == 0) s_nA = 0;
  if (tid >= T - 64) T64[tid - (T - 64)] = exp2((double)(tid - (T - 64)) * 0.015625);
  __syncthreads();

  // tiles of tw (<= 64) photon energies, interleaved over the ktiles tiles of a walker
  const int ktiles = (nE + tw - 1) / tw;
  const int tile = blockIdx.x % ktiles, wi = blockIdx.x / ktiles;
  if (wi >= N) return;  // (the grid is ktiles * N workgroups exactly)
  const double Bw = B[(long long)wi * ldB];
  const bool badB = !(Bw > 0.0) || isinf(Bw);  // such a walker's energies all read NaN
  const double qfac = NH_ERG_PER_EV * (2.0 * (NH_M_E_G * NH_C_CGS)) /
                      (3.0 * NH_E_GAUSS * NH_HBAR_CGS * Bw);

  // ---- 1. liveness of the tile's energies (first wave) ----------------------
  if (tid < 64) {
    const int k = tid < tw ? tid * ktiles + tile : nE;
    int i0 = nG;
    if (k < nE && !badB) {
      const double q = E_eV[k] * qfac;
      int lo = 0, hi = nG;  // first i with q*ig2[i] <= 746 (ig2 decreases with i)
      while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (q * ig2[mid] <= 746.0) hi = mid; else lo = mid + 1;
      }
      i0 = lo;
    }
    const bool live = i0 < nG;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
    if (live) {
      const int pos = __popcll(m & ((1ull << tid) - 1ull));
      amap[pos] = k;
      ai0[pos] = i0;
    }
    if (tid == 0) s_nA = __popcll(m);
    if (k < nE && !live) out[(long long)wi * ldo + k] = badB ? nh_nan() : 0.0;
  }
  __syncthreads();
  const int nA = s_nA;
  if (nA == 0) return;
  const int nseg = nG - 1;

  // ---- 2. (live energy, chunk) per thread ------------------------------------
  const int Cd = min(T / nA, SSA_MAXCH);
  const int a = tid % nA, ch = tid / nA;
  if (ch < Cd) {
    double acc = 0.0;
    const int sbeg = ai0[a];
    const int per = (nseg - sbeg + Cd - 1) / Cd;
    const int s0 = sbeg + ch * per;
    const int s1 = min(nseg, s0 + per);
    const int k = amap[a];
    const double E_erg = E_eV[k] * NH_ERG_PER_EV;
    // CS1 = sqrt(3) e^3 B / (2 pi m_e c^2 hbar E), the emission's
    const double cs1 = (1.7320508075688772 * (NH_E_GAUSS * NH_E_GAUSS * NH_E_GAUSS) * Bw) /
                       (2.0 * NH_PI * NH_M_E_G * (NH_C_CGS * NH_C_CGS) * NH_HBAR_CGS * E_erg);
    // 2 pi^2 hbar^3 / m_e: H = 2 Q exp(-x)
    const double pref = (2.0 * (NH_PI * NH_PI) * (NH_HBAR_CGS * NH_HBAR_CGS * NH_HBAR_CGS) /
                         NH_M_E_G) * (cs1 / E_erg);
    const double q = E_eV[k] * qfac;
    const double cbq = cbrt(q);
    const double* wr = w + (long long)wi * nG;
    const double* dwr = dlw + (long long)wi * nG;
    if (s0 < s1) {
      // a range starts at its first live node, so no node of it is dead; a zero weight gives
      // u = 0 by itself and its segments carry |dlw| = 1e300, whose reciprocal is 0
      auto node = [&](int sn, double& u, double& Q) {
        const double x = q * ig2[sn];
        const double wn = wr[sn] * (ig2[sn] * gam[sn]);  // w / gamma
        const double Qv = ssa_Q1(cbq * ig23[sn], x);
        const double ev = nh_exp_tab(-x, T64);
        u = wn * (Qv * ev);
        Q = Qv;
      };
      double u1, Q1;
      node(s0, u1, Q1);
      int s = s0;
      for (; s + 2 <= s1; s += 2) {
        double uA, QA, uB, QB;
        node(s + 1, uA, QA);
        node(s + 2, uB, QB);
        const double lA = lx[s], lB = lx[s + 1];
        const double dlA = (dwr[s] - lA) + syn_dlnP1(Q1, QA) - q * dig2[s];
        const double dlB = (dwr[s + 1] - lB) + syn_dlnP1(QA, QB) - q * dig2[s + 1];
        acc += nh_seg_pos<false>(u1, uA, dlA, lA);
        acc += nh_seg_pos<false>(uA, uB, dlB, lB);
        u1 = uB;
        Q1 = QB;
      }
      if (s < s1) {
        double uA, QA;
        node(s + 1, uA, QA);
        const double lA = lx[s];
        const double dlA = (dwr[s] - lA) + syn_dlnP1(Q1, QA) - q * dig2[s];
        acc += nh_seg_pos<false>(u1, uA, dlA, lA);
      }
    }
    part[ch * 64 + a] = acc * pref;  // the terms are linear in u: the prefactor once per thread
  }
  __syncthreads();
  // ---- 3. per-energy reduction -------------------------------------------------
  if (tid < nA) {
    double sum = 0.0;
    for (int j = 0; j < Cd; ++j) sum += part[j * 64 + tid];
    out[(long long)wi * ldo + amap[tid]] = sum;
  }
}

// ---- the escape fraction ------------------------------------------------------------------------
// sphere: f = 3 u / tau, u = 1/2 + exp(-tau)/tau - (1 - exp(-tau))/tau^2 (Gould 1979), whose
// terms cancel to tau/3 of 1/tau^2 at small tau (3 eps / tau^3 relative).  Below SSA_TAU_X = 1
// the series f = sum_{n>=2} (-1)^n 3 n tau^(n-2) / (n+1)!, n = 2..21: the first term left out is
// 66/23! = 2.6e-21, and Horner's roundings are at most 20 eps sum |a_n| tau^(n-2) <= 30 eps of
// f >= f(1) = 0.707: 42 eps.  Above it the closed form's roundings come to 5 eps of 0.64 on
// u(1) = 0.236, less beyond: 25 eps.  f(0) = 1 exactly (the leading coefficient).
// slab: f = -expm1(-tau)/tau, 1 at tau = 0.
constexpr double SSA_TAU_X = 1.0;
constexpr int SSA_NTERMS = 20;
struct ssa_series { double a[SSA_NTERMS]; };
// a[j] = (-1)^n 3 n / (n+1)!, n = j + 2 (the factorials up to 22! are exact doubles: one rounding)
constexpr ssa_series ssa_make_series() {
  ssa_series s = {};
  double fact = 2.0;  // (n+1)! as n goes up
  for (int n = 2; n < SSA_NTERMS + 2; ++n) {
    fact *= (double)(n + 1);
    s.a[n - 2] = (n % 2 ? -3.0 : 3.0) * (double)n / fact;
  }
  return s;
}
__constant__ ssa_series SSA_SER = ssa_make_series();

__device__ __forceinline__ double ssa_escape(double tau, int geometry) {
  if (geometry == NH_SSA_SLAB) return tau == 0.0 ? 1.0 : -expm1(-tau) / tau;
  if (tau < SSA_TAU_X) {
    double p = SSA_SER.a[SSA_NTERMS - 1];
#pragma unroll
    for (int n = SSA_NTERMS - 2; n >= 0; --n) p = fma(p, tau, SSA_SER.a[n]);
    return p;
  }
  const double e = exp(-tau), r = 1.0 / tau;
  const double u = 0.5 + r * (e - (1.0 - e) * r);
  return (3.0 * u) * r;
}

constexpr int SSA_THREADS = 256;
constexpr int SSA_WAVES = SSA_THREADS / 64;

struct ssa_apply_args {
  nh_lazy R;
  nh_comp c[NH_MAX_COMP];
  int nc;
};

// one wave per walker row: R is wave-uniform
__global__ __launch_bounds__(SSA_THREADS) void k_ssa_apply(
    ssa_apply_args P, const double* __restrict__ kappa, long long ldk, int geometry,
    const double* __restrict__ colfac, int write_tau, int N, int m, double* __restrict__ out,
    int ldo) {
#pragma clang fp contract(off)
  const int w = blockIdx.x * SSA_WAVES + (int)(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= N) return;
  const double R = nh_lazy_eval(P.R, w);
  double* o = out + (long long)w * ldo;
  if (!(R > 0.0) || isinf(R)) {
    for (int k = lane; k < m; k += 64) o[k] = nh_nan();
    return;
  }
  // tau = 3 kappa / (2 pi R^2) along a sphere's diameter, kappa / (pi R^2) through a slab
  const double area = (geometry == NH_SSA_SLAB ? NH_PI : 2.0 * NH_PI / 3.0) * (R * R);
  for (int k = lane; k < m; k += 64) {
    const double tau = kappa[(long long)w * ldk + k] / area;
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
    o[k] = ssa_escape(tau, geometry) * s;
  }
}

}  // namespace

extern "C" int nh_syn_absorption_plan(int N, int nG, int nE, int* C, int* tw, int* ktiles,
                                      int* lds_bytes) {
  return nh_synchrotron_plan(N, nG, nE, 0, C, tw, ktiles, lds_bytes);
}

extern "C" int nh_syn_absorption(nh_ctx* c, const double* w, const double* dlw, const double* B_G,
                                 int ldB, int N, const double* gam, const double* lx, int nG,
                                 const double* E_eV, int nE, double* out, int ldo) {
  NH_REQUIRE(c && w && dlw && B_G && gam && lx && E_eV && out, "NULL pointer");
  NH_REQUIRE(N >= 0 && nG >= 2 && nE >= 1 && ldo >= nE && ldB >= 1, "bad sizes");
  int C = 0, tw = 0, ktiles = 0, lds = 0;
  if (const int rc = nh_synchrotron_plan(N, nG, nE, 0, &C, &tw, &ktiles, &lds)) return rc;
  if (N == 0) return NH_OK;
  const size_t shm = ((size_t)3 * nG + SSA_MAXCH * 64) * sizeof(double);
  NH_REQUIRE((size_t)lds == shm && tw >= 1 && tw <= 64 && (long long)ktiles * tw >= nE,
             "the plan does not fit this kernel's LDS layout");
  nh_prof_scope ps(c, NH_K_SYNCHROTRON);
  const unsigned blocks = (unsigned)(ktiles * N);
#define NH_LAUNCH_SSA(CC)                                                                      \
  do {                                                                                         \
    if (shm > 64 * 1024)                                                                       \
      NH_CHECK_HIP(hipFuncSetAttribute((const void*)k_syn_absorption<CC>,                      \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)); \
    hipLaunchKernelGGL((k_syn_absorption<CC>), dim3(blocks), dim3(64 * CC), shm, c->stream, w, \
                       dlw, B_G, ldB, N, gam, lx, nG, E_eV, nE, out, ldo, tw);                 \
  } while (0)
  switch (C) {
    case 16: NH_LAUNCH_SSA(16); break;
    case 8: NH_LAUNCH_SSA(8); break;
    default: NH_LAUNCH_SSA(4); break;
  }
#undef NH_LAUNCH_SSA
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_ssa_apply(nh_ctx* c, const double* kappa, long long ldk, const nh_lazy* R_cm,
                            int geometry, const nh_comp* comps, int ncomp, const double* colfac,
                            int write_tau, int N, int m, double* out, int ldo) {
  NH_REQUIRE(c && kappa && R_cm && out, "null argument");
  NH_REQUIRE(geometry == NH_SSA_SPHERE || geometry == NH_SSA_SLAB, "unknown geometry");
  NH_REQUIRE(ncomp >= 0 && ncomp <= NH_MAX_COMP && (ncomp == 0 || comps), "ncomp must be 0..8");
  NH_REQUIRE(!write_tau || (ncomp == 0 && !colfac), "the opacity takes no terms");
  NH_REQUIRE(N >= 0 && m >= 1 && ldo >= m && (ldk == 0 || ldk >= m), "bad shape");
  ssa_apply_args P;
  memset(&P, 0, sizeof P);
  P.R = *R_cm;
  P.nc = ncomp;
  for (int j = 0; j < ncomp; ++j) {
    NH_REQUIRE(comps[j].ptr && (comps[j].ld == 0 || comps[j].ld >= m), "bad component");
    P.c[j] = comps[j];
  }
  if (N == 0) return NH_OK;
  nh_prof_scope ps(c, NH_K_GLUE);
  hipLaunchKernelGGL(k_ssa_apply, dim3((unsigned)((N + SSA_WAVES - 1) / SSA_WAVES)),
                     dim3(SSA_THREADS), 0, c->stream, P, kappa, ldk, geometry, colfac, write_tau,
                     N, m, out, ldo);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
