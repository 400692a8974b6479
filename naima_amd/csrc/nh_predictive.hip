// nh_predictive.hip -- posterior predictive checks from a chain's stored spectra: replicated data
// drawn from the likelihood's own sampling distribution, discrepancy statistics of the observed
// and the replicated data per posterior sample, their comparison counts, and the probability
// integral transform of every data point.  Matrices are row-major device matrices [M][ld] with
// ncol <= ld columns in use, as in nh_infocrit.hip; the data columns are nh_pointwise_lnl's.
//
//   nh_ppc_rows      one wave per row s (global index row = row0 + s).  With mc = x*conv, for a
//                    point k that is not an upper limit: the observed residual
//                    r_obs = -(mc - flux)/sg, sg = mc > flux ? ehi : elo (data minus model in
//                    units of the error the likelihood uses), and a replicate from the split
//                    normal that likelihood implies: Philox4x32-10 of counter (lo32(row),
//                    hi32(row), k, 0) under key (lo32(seed), hi32(seed)) gives r0..r3,
//                    U = ((r0 << 20 | r1 >> 12) + 0.5) 2^-52, V = (r2 + 0.5) 2^-32, W = r3 2^-32,
//                    a = sqrt(-2 log U) |cos(2 pi V)| (half-normal), below = W (elo + ehi) < ehi,
//                    y_rep = below ? mc - ehi a : mc + elo a, r_rep = below ? -a : +a.  A value
//                    depends on (seed, row, k) alone: not on the grid, not on how a chain is cut
//                    into calls.  Y[s][k] = y_rep (mc at an upper limit); T[s][0..5] = chi2_obs,
//                    chi2_rep, maxabs_obs, maxabs_rep, runs_obs, runs_rep over the points that
//                    are not upper limits, in column order: chi2 = sum r^2 (lane order, then a
//                    butterfly), maxabs = max |r| (a NaN stays), runs = 1 + the sign changes
//                    between consecutive such points (r >= 0 is positive; 0 without a point),
//                    taken from wave ballots.
//   nh_ppc_counts    counts[0..3] over the rows of T whose six values are finite: chi2_rep >=
//                    chi2_obs, maxabs_rep >= maxabs_obs, runs_rep <= runs_obs; and the number of
//                    the other rows.  An integer atomic per wave.
//   nh_pit_columns   per column: the mean over the rows of the split-normal CDF of the datum
//                    given the row's model (an upper limit: the fraction of rows above it): one
//                    chunk pass (nh_colred.h).
//
// No floating-point atomics: every floating-point sum has an order fixed by the shapes alone, so
// repeated calls give bit-identical results.  Row indices are 64-bit, M < 2^31.  Every launch is
// on the context's stream; nothing synchronises with the host.
#include "nh_colred.h"
#include "nh_philox.h"

namespace {

// ---------------------------------------------------------------- the random stream
// (Philox4x32-10: nh_philox.h; counter word 3 = 0 is this stream's)
// the half-normal a and the side of the replicate of (row, k)
__host__ __device__ __forceinline__ double ppc_draw(unsigned long long seed, long long row, int k,
                                                    double elo, double ehi, bool* below) {
  const nh_u4 r = nh_philox((unsigned)((unsigned long long)row & 0xffffffffull),
                            (unsigned)((unsigned long long)row >> 32), (unsigned)k, 0u,
                            (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32));
  const double U =
      ((double)(((unsigned long long)r.x << 20) | (unsigned long long)(r.y >> 12)) + 0.5) *
      0x1p-52;
  const double V = ((double)r.z + 0.5) * 0x1p-32;
  const double W = (double)r.w * 0x1p-32;
  *below = W * (elo + ehi) < ehi;
  return sqrt(-2.0 * log(U)) * fabs(cos(6.283185307179586 * V));
}

// the sign changes of `pos` between consecutive set bits of `valid` (a 64-column tile, one bit
// per lane), the last point before the tile having sign `carry` (if `has`): this lane's share
__device__ __forceinline__ int ppc_change(unsigned long long valid, unsigned long long pos,
                                          int lane, bool has, bool carry) {
  if (!((valid >> lane) & 1ull)) return 0;
  const bool mine = (pos >> lane) & 1ull;
  const unsigned long long before = valid & ((1ull << lane) - 1ull);
  if (before) return mine != (bool)((pos >> (63 - __clzll((long long)before))) & 1ull);
  return has && mine != carry;
}

// the larger of two values, a NaN winning over any number
__device__ __forceinline__ double ppc_max(double m, double v) { return (v > m || v != v) ? v : m; }

// ---------------------------------------------------------------- replicates and row statistics
__global__ __launch_bounds__(PO_THREADS) void k_ppc_rows(
    const double* __restrict__ x, long long M, int nE, long long ld,
    const double* __restrict__ conv, const double* __restrict__ flux,
    const double* __restrict__ elo, const double* __restrict__ ehi, const int* __restrict__ ul,
    unsigned long long seed, long long row0, double* __restrict__ Y, long long ldY,
    double* __restrict__ T) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * (PO_THREADS / 64);
  for (long long s = (long long)blockIdx.x * (PO_THREADS / 64) + (threadIdx.x >> 6); s < M;
       s += stride) {  // (s is the wave's: every loop bound below is wave-uniform)
    const double* xr = x + s * ld;
    double co = 0.0, cr = 0.0, mo = 0.0, mr = 0.0;
    int no = 0, nr = 0;
    bool has = false, lo = false, lr = false;  // the last point before the tile: any, its signs
    for (int k0 = 0; k0 < nE; k0 += 64) {  // (whole tiles: the ballots below need every lane)
      const int k = k0 + lane;
      bool valid = false, po = false, pr = false;
      if (k < nE) {
        const double mc = xr[k] * conv[k];
        double y = mc;
        if (!ul[k]) {
          const double el = elo[k], eh = ehi[k];
          const double d = mc - flux[k];
          const double ro = -d / (d > 0.0 ? eh : el);
          bool below;
          const double a = ppc_draw(seed, row0 + s, k, el, eh, &below);
          y = below ? mc - eh * a : mc + el * a;
          valid = true;
          po = ro >= 0.0;
          pr = !below;
          co += ro * ro;
          cr += a * a;
          mo = ppc_max(mo, fabs(ro));
          mr = ppc_max(mr, a);
        }
        if (Y) Y[s * ldY + k] = y;
      }
      const unsigned long long bv = __ballot(valid), bo = __ballot(po), br = __ballot(pr);
      no += ppc_change(bv, bo, lane, has, lo);
      nr += ppc_change(bv, br, lane, has, lr);
      if (bv) {
        const int last = 63 - __clzll((long long)bv);
        has = true;
        lo = (bo >> last) & 1ull;
        lr = (br >> last) & 1ull;
      }
    }
    if (!T) continue;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      co += __shfl_down(co, off, 64);
      cr += __shfl_down(cr, off, 64);
      mo = ppc_max(mo, __shfl_down(mo, off, 64));
      mr = ppc_max(mr, __shfl_down(mr, off, 64));
      no += __shfl_down(no, off, 64);
      nr += __shfl_down(nr, off, 64);
    }
    if (lane == 0) {
      double* t = T + s * 6;
      t[0] = co;
      t[1] = cr;
      t[2] = mo;
      t[3] = mr;
      t[4] = has ? (double)(1 + no) : 0.0;
      t[5] = has ? (double)(1 + nr) : 0.0;
    }
  }
}

// ---------------------------------------------------------------- comparison counts
__global__ __launch_bounds__(PO_THREADS) void k_ppc_counts(const double* __restrict__ T, long long M,
                                                         unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * PO_THREADS;
  const long long base = (long long)blockIdx.x * PO_THREADS + (threadIdx.x & ~63);
  for (long long w = base; w < M; w += stride) {  // (w is the wave's first row: wave-uniform)
    const long long s = w + lane;
    bool c0 = false, c1 = false, c2 = false, bad = false;
    if (s < M) {
      const double* t = T + s * 6;
      const double a0 = t[0], a1 = t[1], a2 = t[2], a3 = t[3], a4 = t[4], a5 = t[5];
      bad = !(po_finite(a0) && po_finite(a1) && po_finite(a2) && po_finite(a3) && po_finite(a4) &&
              po_finite(a5));
      c0 = !bad && a1 >= a0;
      c1 = !bad && a3 >= a2;
      c2 = !bad && a5 <= a4;
    }
    const unsigned long long n0 = __popcll(__ballot(c0)), n1 = __popcll(__ballot(c1)),
                             n2 = __popcll(__ballot(c2)), n3 = __popcll(__ballot(bad));
    if (lane < 4) {
      const unsigned long long n = lane == 0 ? n0 : lane == 1 ? n1 : lane == 2 ? n2 : n3;
      if (n)
        __hip_atomic_fetch_add(counts + lane, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------- PIT
// the split-normal CDF of the datum y given the model m: scale ehi below the model, elo above;
// the lower tail through erfc, which keeps a far point's probability positive
__device__ __forceinline__ double ppc_cdf(double y, double m, double el, double eh) {
  const double z = y - m, w = el + eh;
  if (z <= 0.0) return (2.0 * eh / w) * (0.5 * erfc(-(z / eh) * 0.7071067811865476));
  return eh / w + (2.0 * el / w) * (0.5 * erf((z / el) * 0.7071067811865476));
}

// the sum of the CDF (of the rows above the limit, for an upper limit)
struct k_pit_sum {
  using F = colred_fields<0, '+'>;
  const double* __restrict__ x;
  long long ld;
  const double* __restrict__ conv;
  const double* __restrict__ flux;
  const double* __restrict__ elo;
  const double* __restrict__ ehi;
  const int* __restrict__ ul;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    const double cv = conv[c], f = flux[c], el = elo[c], eh = ehi[c];
    const bool lim = ul[c] != 0;
    double s = 0.0;
    walk([&](long long t) {
      const double mc = x[t * ld + c] * cv;
      s += lim ? (mc > f ? 1.0 : 0.0) : ppc_cdf(f, mc, el, eh);
    });
    a = {{s}};
  }
};

// out[0][c] = pit, out[1][c] = ul_violation: the chunks in order, NaN where the other applies
__global__ void k_pit_fin(long long nch, int ncol, long long M, const int* __restrict__ ul,
                          double* __restrict__ out, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double v = colred_fold<k_pit_sum>(part, nch, ncol, c).d[0] / (double)M;
  const bool lim = ul[c] != 0;
  out[c] = lim ? nh_nan() : v;
  out[ncol + c] = lim ? v : nh_nan();
}

}  // namespace

extern "C" int nh_ppc_rows(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                           const double* conv, const double* flux, const double* elo,
                           const double* ehi, const int* ul, unsigned long long seed,
                           long long row0, double* Y, long long ldY, double* T) {
  NH_REQUIRE(ctx && x && conv && flux && elo && ehi && ul, "null argument");
  NH_REQUIRE(Y || T, "Y and T both NULL: nothing to write");
  NH_REQUIRE_MATRIX(M, nE, ld, NH_ROWS_INT);
  NH_REQUIRE(!Y || ldY >= nE, "nE > ldY");
  NH_REQUIRE(row0 >= 0, "row0 < 0");
  unsigned nb = (unsigned)std::min<long long>(cdiv(M, PO_THREADS / 64), 8192);
  hipLaunchKernelGGL(k_ppc_rows, dim3(nb), dim3(PO_THREADS), 0, ctx->stream, x, M, nE, ld, conv,
                     flux, elo, ehi, ul, seed, row0, Y, ldY, T);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_ppc_counts(nh_ctx* ctx, const double* T, long long M, long long* counts) {
  NH_REQUIRE(ctx && T && counts, "null argument");
  NH_REQUIRE(M > 0, "M == 0: no samples");
  NH_REQUIRE(M < (1ll << 31), "M >= 2^31 rows");
  hipStream_t s = ctx->stream;
  NH_CHECK_HIP(hipMemsetAsync(counts, 0, 4 * 8, s));
  unsigned nb = (unsigned)std::min<long long>(cdiv(M, PO_THREADS), 2048);
  hipLaunchKernelGGL(k_ppc_counts, dim3(nb), dim3(PO_THREADS), 0, s, T, M,
                     (unsigned long long*)counts);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_pit_columns(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                              const double* conv, const double* flux, const double* elo,
                              const double* ehi, const int* ul, double* out) {
  NH_REQUIRE(ctx && x && conv && flux && elo && ehi && ul && out, "null argument");
  NH_REQUIRE_MATRIX(M, nE, ld, NH_ROWS_INT);
  const colred_grid g = colred_plan(M, nE);
  NH_REQUIRE_PLAN(g);
  void* base = nullptr;  // scratch: part [nch][nE]
  int rc = nh_scratch(ctx, (size_t)g.nch * nE * 8, &base);
  if (rc) return rc;
  const colred_out part = colred_dense<k_pit_sum>((double*)base);
  hipStream_t s = ctx->stream;
  if ((rc = colred_launch<k_pit_sum>(s, g, part, x, ld, conv, flux, elo, ehi, ul))) return rc;
  hipLaunchKernelGGL(k_pit_fin, dim3(g.col_blocks()), dim3(PO_THREADS), 0, s, g.nch, nE, M, ul, out,
                     part);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
