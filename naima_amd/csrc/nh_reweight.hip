// nh_reweight.hip -- importance reweighting of a finished fit: what turns the log-ratios of a new
// target to the fitted one into Pareto-smoothed, self-normalised log-weights, and the weighted
// reductions over the samples in HBM.  Matrices are row-major device matrices [M][ld] with
// ncol <= ld columns in use, as in nh_posterior.hip and nh_infocrit.hip.  A WEIGHT COLUMN is a
// pointer to lw[0] and a row stride ldw, holding normalised log-weights; a row with lw = -inf has
// weight zero and is left out of every reduction, whatever its value (a NaN included).
//
//   nh_row_sums_select      out[s] = sign * sum_j L[s][cols[j]] in the order of cols: the
//                           log-ratio of leaving data points out (sign -1) or adding them (+1).
//   nh_psis_weights         per column of log-ratios: x = lr - max; the chunked pass of
//                           nh_psis_columns sums exp(x) below the cutoff and over all rows and lists
//                           the tail rows (an integer atomic counter); one workgroup per column
//                           sorts, fits and smooths the tail (nh_gpd.h) and writes the tail's
//                           log-weights; a last pass writes the others and sums exp(2 lw).
//   nh_weighted_moments     count, weighted mean and weighted variance per column: two chunk
//                           passes (nh_colred.h).
//   nh_weighted_select      weighted order statistics: the radix sort of (key, row index) of
//                           nh_radix.h per column, zero-weight rows keyed behind everything; then
//                           the running sum of the weights in sorted order (below) picks the rows.
//   nh_resample_systematic  the running sum in row order, stored; output j searches it.
//   nh_gather_rows          out[j] = x[idx[j]].
//
// The running sum c_i of n weights is a function of n alone and never decreases: tiles of
// RW_TILE elements, a thread adds RW_PER consecutive weights in order (r), thread 0 of the tile
// adds the threads' totals in order (off), one thread per column adds the tiles' totals in order
// (boff), and c_i = boff + (off + r_i).  Each level starts where the one before ended in the same
// rounded value, so c_i >= c_(i-1) holds in floating point and "the first i with c_i >= t" is a
// lower bound.
//
// No floating-point atomics: every floating-point sum has an order fixed by the shapes alone (and,
// in the tail and the sorted columns, by the sorted values), so repeated calls give bit-identical
// results.  Row indices are 64-bit, M < 2^31.  Every launch is on the context's stream; nothing
// synchronises with the host.
#include "nh_gpd.h"
#include "nh_radix.h"

namespace {

constexpr int RW_COLS = 64;                    // columns one launch of k_rw_row_sums adds
constexpr int RW_PER = 8;                      // consecutive weights a thread adds
constexpr int RW_TILE = PO_THREADS * RW_PER;   // weights per workgroup of the running sum
constexpr int RW_MAX_Q = 16;

struct rw_cols { int c[RW_COLS]; };
struct rw_q { double q[RW_MAX_Q]; };

// w = exp(lw); exactly 0 for lw = -inf
__device__ __forceinline__ double rw_weight(double lw) { return lw == -INFINITY ? 0.0 : exp(lw); }

// ---------------------------------------------------------------- row sums of chosen columns
__global__ __launch_bounds__(PO_THREADS) void k_rw_row_sums(const double* __restrict__ L, long long M,
                                                           long long ld, rw_cols cols, int n,
                                                           double sign, int first,
                                                           double* __restrict__ out, long long ldo) {
  for (long long s = (long long)blockIdx.x * PO_THREADS + threadIdx.x; s < M;
       s += (long long)gridDim.x * PO_THREADS) {
    double acc = first ? 0.0 : out[s * ldo];
    for (int j = 0; j < n; ++j) acc += sign * L[s * ld + cols.c[j]];
    out[s * ldo] = acc;
  }
}

// ---------------------------------------------------------------- PSIS weights
// (the chunk passes, their partials and the fold in chunk order: nh_colred.h)
// the maximum (NaNs passed over) | the number of NaN or +inf entries, of finite ones
struct k_rw_max {
  using F = colred_fields<2, '>'>;
  const double* __restrict__ x;
  long long ld;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    double hi = -INFINITY;
    long long bad = 0, fin = 0;
    walk([&](long long t) {
      double v = x[t * ld + c];
      hi = fmax(hi, v);
      const bool f = po_finite(v);  // (each counter moves in every row: nh_colred.h)
      fin += f ? 1 : 0;
      bad += (f || v == -INFINITY) ? 0 : 1;
    });
    a = {{hi}, {bad, fin}};
  }
};

// cst[0][c] = the column's maximum; status[c] = its NaN and +inf entries, M for a column without
// a finite entry (every one of its -inf entries offends), 0 for a column that gets weights
__global__ void k_rw_max_fin(long long nch, int ncol, long long M, double* __restrict__ cst,
                             int* __restrict__ status, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const auto a = colred_fold<k_rw_max>(part, nch, ncol, c);
  const long long bad = a.n[0], fin = a.n[1];
  cst[c] = a.d[0];
  status[c] = (int)(bad ? bad : (fin ? 0 : M));
}

// the cutoff of column c on x = lr - max: the order statistic of rank M - Mt - 1 of lr is that of
// x (the map is monotone), floored at log(DBL_MIN)
__device__ __forceinline__ double rw_cut(double hi, double lsel) {
  return fmax(lsel - hi, CRIT_LOG_TINY);
}

// the sums of exp(x) over the rows with x <= cut and over all rows (slots 0 and 2 of part
// [nch][3][ncol]; slot 1 is k_rw_write's); the rows with x > cut go to the column's list
// tx / trow [c*cap ..], their number to cnt[c] (zeroed before the launch)
struct k_rw_split {
  using F = colred_fields<0, '+', '+'>;
  const double* __restrict__ lr;
  long long ld;
  const double* __restrict__ cst;
  const int* __restrict__ status;
  const double* __restrict__ lsel;
  int cap;
  double* __restrict__ tx;
  int* __restrict__ trow;
  unsigned* __restrict__ cnt;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    if (status[c] != 0) return;
    const double hi = cst[c];
    const double cut = rw_cut(hi, lsel[c]);
    double sa = 0.0, r = 0.0;
    walk([&](long long t) {
      const double xv = lr[t * ld + c] - hi;
      const double e = exp(xv);
      r += e;
      if (xv > cut) {
        unsigned slot = __hip_atomic_fetch_add(cnt + c, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
        if (slot < (unsigned)cap) {  // (always: at most Mt values lie above that order statistic)
          tx[(long long)c * cap + slot] = xv;
          trow[(long long)c * cap + slot] = (int)t;
        }
      } else {
        sa += e;
      }
    });
    a = {{sa, r}};
  }
};

// one workgroup per column: sort the tail, fit, smooth; the normaliser and the mean ratio; the
// tail rows' log-weights.  cst[1][c] = logsumexp(x) for k_rw_write, cst[2][c] = the tail's sum of
// exp(2 lw) for k_rw_ess (taken on lw, not on x: exp(2 x) underflows long before exp(2 lw) does
// where one ratio towers over the rest).
__global__ __launch_bounds__(PO_THREADS) void k_rw_tail(
    int ncol, long long M, long long nch, int cap, double* __restrict__ cst,
    const int* __restrict__ status, const double* __restrict__ lsel, colred_out part,
    const double* __restrict__ tx, const int* __restrict__ trow, const unsigned* __restrict__ cnt,
    double* __restrict__ lw, long long ldw, double* __restrict__ pareto_k,
    long long* __restrict__ n_tail, double* __restrict__ lmean) {
  CRIT_TAIL_LDS(s);
  const int tid = threadIdx.x;
  const int c = blockIdx.x;
  if (status[c] != 0) {  // (the workgroup's: no barrier is skipped by a part of it)
    if (tid == 0) {
      pareto_k[c] = lmean[c] = cst[ncol + c] = cst[2 * ncol + c] = nh_nan();
      n_tail[c] = 0;
    }
    return;
  }
  const int n = (int)min(cnt[c], (unsigned)min(cap, CRIT_TAIL_MAX));
  const double hi = cst[c];
  const double ecut = exp(rw_cut(hi, lsel[c]));
  const double kpar = crit_tail_fit(s, tx + (long long)c * cap, trow + (long long)c * cap, n, ecut, tid);
  const double* xs = reinterpret_cast<const double*>(s.key);

  double a = 0.0;
  __syncthreads();
  for (int i = tid; i < n; i += PO_THREADS) a += exp(xs[i]);
  a = crit_block_reduce(a, s.red, tid, [](double p, double q) { return p + q; });
  if (tid == 0) {
    const auto sums = colred_fold<k_rw_split>(part, nch, ncol, c);
    const double an = sums.d[0], rn = sums.d[1];
    const double lz = log(an + a);
    pareto_k[c] = kpar;
    n_tail[c] = n;
    lmean[c] = hi + (log(rn) - log((double)M));
    cst[ncol + c] = lz;
    *s.bpost = lz;
  }
  __syncthreads();
  const double lz = *s.bpost;
  double b = 0.0;
  for (int i = tid; i < n; i += PO_THREADS) {
    const double l = xs[i] - lz;
    lw[(long long)s.row[i] * ldw + c] = l;
    b += exp(2.0 * l);
  }
  b = crit_block_reduce(b, s.red, tid, [](double p, double q) { return p + q; });
  if (tid == 0) cst[2 * ncol + c] = b;
}

// lw = x - logsumexp(x) of the rows below the cutoff, and the sum of exp(2 lw) over them (slot 1
// of part); NaN in every row of a column without weights
struct k_rw_write {
  using F = colred_fields<0, '+'>;
  const double* __restrict__ lr;
  long long ld;
  const double* __restrict__ cst;
  const int* __restrict__ status;
  const double* __restrict__ lsel;
  int ncol;
  double* __restrict__ lw;
  long long ldw;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    if (status[c] != 0) {
      walk([&](long long t) { lw[t * ldw + c] = nh_nan(); });
      return;
    }
    const double hi = cst[c], lz = cst[ncol + c];
    const double cut = rw_cut(hi, lsel[c]);
    double b = 0.0;
    walk([&](long long t) {
      const double xv = lr[t * ld + c] - hi;
      if (!(xv > cut)) {
        const double l = xv - lz;
        lw[t * ldw + c] = l;
        b += exp(2.0 * l);
      }
    });
    a = {{b}};
  }
};

// ess[c] = 1 / sum_s exp(2 lw): the chunks in chunk order, then the tail; NaN without weights
__global__ void k_rw_ess(long long nch, int ncol, const double* __restrict__ cst,
                         const int* __restrict__ status, double* __restrict__ ess, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double b = colred_fold<k_rw_write>(part, nch, ncol, c).d[0];
  ess[c] = status[c] != 0 ? nh_nan() : 1.0 / (b + cst[2 * ncol + c]);
}

// ---------------------------------------------------------------- weighted moments
// over the rows with lw > -inf: the sums of w and of w x, min and max of x | their number, that
// of non-finite x
struct k_rw_wsum {
  using F = colred_fields<2, '+', '+', '<', '>'>;
  const double* __restrict__ x;
  long long ld;
  const double* __restrict__ lw;
  long long ldw;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    double sw = 0.0, s = 0.0, lo = INFINITY, hi = -INFINITY;
    long long n = 0, bad = 0;
    walk([&](long long t) {
      const double l = lw[t * ldw];
      if (l == -INFINITY) return;
      const double w = exp(l), v = x[t * ld + c];
      sw += w;
      s += w * v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
      ++n;
      bad += po_finite(v) ? 0 : 1;
    });
    a = {{sw, s, lo, hi}, {n, bad}};
  }
};

// out[0|1][c] = the number of rows with positive weight, the weighted mean (the value itself
// where all are equal; NaN with a non-finite value or without a row); mst[0|1][c] = the sum of
// the weights, 1 where the variance is exactly 0 / 0 where it is a quotient / -1 where it is NaN
__global__ void k_rw_wmean(long long nch, int ncol, double* __restrict__ out,
                           double* __restrict__ mst, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const auto a = colred_fold<k_rw_wsum>(part, nch, ncol, c);
  const double sw = a.d[0], s = a.d[1], lo = a.d[2], hi = a.d[3];
  const long long n = a.n[0], bad = a.n[1];
  const bool none = bad || n == 0;
  out[c] = (double)n;
  out[ncol + c] = none ? nh_nan() : (lo == hi ? lo : s / sw);
  mst[c] = sw;
  mst[ncol + c] = none ? -1.0 : (lo == hi ? 1.0 : 0.0);
}

// the sum of w (x - mean)^2 over the rows with lw > -inf
struct k_rw_wsq {
  using F = colred_fields<0, '+'>;
  const double* __restrict__ x;
  long long ld;
  const double* __restrict__ lw;
  long long ldw;
  const double* __restrict__ out;
  int ncol;
  template <class W>
  __device__ __forceinline__ void column(int c, W walk, F::acc& a) const {
    const double mean = out[ncol + c];
    double q = 0.0;
    walk([&](long long t) {
      const double l = lw[t * ldw];
      if (l == -INFINITY) return;
      const double d = x[t * ld + c] - mean;
      q += exp(l) * (d * d);
    });
    a = {{q}};
  }
};

__global__ void k_rw_wvar(long long nch, int ncol, const double* __restrict__ mst,
                          double* __restrict__ out, colred_out part) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double q = colred_fold<k_rw_wsq>(part, nch, ncol, c).d[0];
  const double kind = mst[ncol + c];
  out[2 * ncol + c] = kind < 0.0 ? nh_nan() : (kind > 0.0 ? 0.0 : q / mst[c]);
}

// ---------------------------------------------------------------- the running sum of weights
// element i of column blockIdx.y is row idx[i] (row i without idx); its weight
__device__ __forceinline__ double rw_elem_weight(const double* __restrict__ lw, long long ldw,
                                                 const unsigned* __restrict__ ic, long long i) {
  return rw_weight(lw[(ic ? (long long)ic[i] : i) * ldw]);
}

// a thread's total of its RW_PER consecutive weights, then off[t] = the totals of the threads
// before t added in order by thread 0; off[PO_THREADS] = the tile's total.  All threads call.
__device__ __forceinline__ void rw_tile_offsets(const double* __restrict__ lw, long long ldw,
                                                const unsigned* __restrict__ ic, long long S,
                                                double* off) {
  const int t = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * RW_TILE + (long long)t * RW_PER;
  double r = 0.0;
  for (int e = 0; e < RW_PER; ++e)
    if (i0 + e < S) r = r + rw_elem_weight(lw, ldw, ic, i0 + e);
  off[t + 1] = r;
  __syncthreads();
  if (t == 0) {
    double run = 0.0;
    for (int q = 0; q < PO_THREADS; ++q) {
      const double tot = off[q + 1];
      off[q] = run;
      run = run + tot;
    }
    off[PO_THREADS] = run;
  }
  __syncthreads();
}

// bsum[col][tile] = the tile's total
__global__ __launch_bounds__(PO_THREADS) void k_rw_tile_sums(const double* __restrict__ lw,
                                                            long long ldw,
                                                            const unsigned* __restrict__ idx,
                                                            long long S, unsigned nblk,
                                                            double* __restrict__ bsum) {
  __shared__ double off[PO_THREADS + 1];
  const unsigned* ic = idx ? idx + (long long)blockIdx.y * S : nullptr;
  rw_tile_offsets(lw, ldw, ic, S, off);
  if (threadIdx.x == 0) bsum[(long long)blockIdx.y * nblk + blockIdx.x] = off[PO_THREADS];
}

// one thread per column: boff[col][tile] = the totals of the tiles before it added in order,
// total[col] = C.  With `out` (the selection): a column with a NaN under positive weight
// (nanflag) or without a positive sum gets NaN in all nq rows here, and k_rw_pick leaves it alone.
__global__ void k_rw_tile_scan(const double* __restrict__ bsum, unsigned nblk, int g,
                               double* __restrict__ boff, double* __restrict__ total,
                               const int* __restrict__ nanflag, int c0, int ncol, int nq,
                               double* __restrict__ out) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= g) return;
  double run = 0.0;
  for (unsigned b = 0; b < nblk; ++b) {
    boff[(long long)j * nblk + b] = run;
    run = run + bsum[(long long)j * nblk + b];
  }
  if (out && (nanflag[j] != 0 || !(run > 0.0))) {
    for (int r = 0; r < nq; ++r) out[(long long)r * ncol + c0 + j] = nh_nan();
    run = nh_nan();
  }
  total[j] = run;
}

__device__ __forceinline__ bool rw_reached(double c, double thr) { return c >= thr && c > 0.0; }

// the selection: element i of the sorted column is the answer of q_j when its running sum is the
// first to reach q_j C; the running sum of the element before it is known without a neighbour
__global__ __launch_bounds__(PO_THREADS) void k_rw_pick(const double* __restrict__ x, long long ld,
                                                       const double* __restrict__ lw, long long ldw,
                                                       const unsigned* __restrict__ idx, long long S,
                                                       unsigned nblk, const double* __restrict__ boff,
                                                       const double* __restrict__ total, int c0,
                                                       int ncol, rw_q q, int nq,
                                                       double* __restrict__ out) {
  __shared__ double off[PO_THREADS + 1];
  const unsigned* ic = idx + (long long)blockIdx.y * S;
  rw_tile_offsets(lw, ldw, ic, S, off);
  const double C = total[blockIdx.y];
  if (!(C > 0.0)) return;  // (the column's: NaN was written by k_rw_tile_scan)
  const double b0 = boff[(long long)blockIdx.y * nblk + blockIdx.x];
  const double o = off[threadIdx.x];
  const long long i0 = (long long)blockIdx.x * RW_TILE + (long long)threadIdx.x * RW_PER;
  double r = 0.0, prev = b0 + o;
  for (int e = 0; e < RW_PER && i0 + e < S; ++e) {
    r = r + rw_elem_weight(lw, ldw, ic, i0 + e);
    const double c = b0 + (o + r);
    if (c > prev) {
      for (int j = 0; j < nq; ++j) {
        const double thr = q.q[j] * C;
        if (rw_reached(c, thr) && !rw_reached(prev, thr))
          out[(long long)j * ncol + c0 + blockIdx.y] = x[(long long)ic[i0 + e] * ld + c0 + blockIdx.y];
      }
    }
    prev = c;
  }
}

// keys[col][row]: rk_key of the value; ~0, behind everything, for a row of weight zero and for a
// NaN; nanflag[col] counts the NaNs under positive weight (one integer atomic per wave)
__global__ __launch_bounds__(PO_THREADS) void k_rw_keys(const double* __restrict__ x, long long M,
                                                       long long ld, const double* __restrict__ lw,
                                                       long long ldw, int c0,
                                                       unsigned long long* __restrict__ keys,
                                                       int* __restrict__ nanflag) {
  long long e = (long long)blockIdx.x * PO_THREADS + threadIdx.x;
  bool bad = false;
  if (e < M) {
    const double v = x[e * ld + c0 + blockIdx.y];
    const bool live = !(lw[e * ldw] == -INFINITY);
    bad = live && v != v;
    keys[(long long)blockIdx.y * M + e] = (live && v == v) ? rk_key(v) : ~0ull;
  }
  unsigned long long m = __builtin_amdgcn_ballot_w64(bad);
  if (m && (threadIdx.x & 63) == 0)
    __hip_atomic_fetch_add(nanflag + blockIdx.y, (int)__popcll(m), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- systematic resampling
// cs[i] = the running sum of the weights in row order
__global__ __launch_bounds__(PO_THREADS) void k_rw_cumsum(const double* __restrict__ lw, long long ldw,
                                                         long long S, const double* __restrict__ boff,
                                                         double* __restrict__ cs) {
  __shared__ double off[PO_THREADS + 1];
  rw_tile_offsets(lw, ldw, nullptr, S, off);
  const double b0 = boff[blockIdx.x];
  const double o = off[threadIdx.x];
  const long long i0 = (long long)blockIdx.x * RW_TILE + (long long)threadIdx.x * RW_PER;
  double r = 0.0;
  for (int e = 0; e < RW_PER && i0 + e < S; ++e) {
    r = r + rw_elem_weight(lw, ldw, nullptr, i0 + e);
    cs[i0 + e] = b0 + (o + r);
  }
}

// idx[j] = the first i with cs[i] >= ((u0 + j) / n_out) C and cs[i] > 0: cs never decreases, so
// that row's own weight is positive; -1 throughout when no weight is
__global__ __launch_bounds__(PO_THREADS) void k_rw_draw(const double* __restrict__ cs, long long S,
                                                       const double* __restrict__ total, double u0,
                                                       long long n_out, long long* __restrict__ idx) {
  const double C = total[0];
  for (long long j = (long long)blockIdx.x * PO_THREADS + threadIdx.x; j < n_out;
       j += (long long)gridDim.x * PO_THREADS) {
    if (!(C > 0.0)) { idx[j] = -1; continue; }
    const double thr = ((u0 + (double)j) / (double)n_out) * C;
    long long lo = 0, hi = S - 1;  // (cs[S - 1] = C reaches every threshold)
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (rw_reached(cs[mid], thr)) hi = mid; else lo = mid + 1;
    }
    idx[j] = lo;
  }
}

__global__ __launch_bounds__(PO_THREADS) void k_rw_gather(const double* __restrict__ x, long long ld,
                                                         const long long* __restrict__ idx,
                                                         long long n_out, int ncol,
                                                         double* __restrict__ out, long long ldo) {
  const long long n = n_out * ncol;
  for (long long i = (long long)blockIdx.x * PO_THREADS + threadIdx.x; i < n;
       i += (long long)gridDim.x * PO_THREADS) {
    const long long j = i / ncol;
    const int c = (int)(i - j * ncol);
    out[j * ldo + c] = x[idx[j] * ld + c];
  }
}

unsigned rw_grid(long long n) {
  return (unsigned)std::min<long long>(std::max<long long>(cdiv(n, PO_THREADS), 1), 1 << 16);
}

}  // namespace

extern "C" int nh_row_sums_select(nh_ctx* ctx, const double* L, long long M, int ncol, long long ld,
                                  const int* cols, int n, int sign, double* out, long long ldo) {
  NH_REQUIRE(ctx && L && out && (cols || n == 0), "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_INT);
  NH_REQUIRE(n >= 0, "n must not be negative");
  NH_REQUIRE(sign == 1 || sign == -1, "sign must be +1 or -1");
  NH_REQUIRE(ldo >= 1, "ldo must be positive");
  for (int j = 0; j < n; ++j)
    if (cols[j] < 0 || cols[j] >= ncol)
      return nh_set_error(NH_EINVAL, "nh_row_sums_select: column %d is %d, outside [0, %d)", j,
                          cols[j], ncol);
  hipStream_t s = ctx->stream;
  for (int a = 0; a == 0 || a < n; a += RW_COLS) {  // (n == 0: one launch writes the zeros)
    rw_cols c = {};
    const int m = std::min(RW_COLS, n - a);
    for (int j = 0; j < m; ++j) c.c[j] = cols[a + j];
    hipLaunchKernelGGL(k_rw_row_sums, dim3(rw_grid(M)), dim3(PO_THREADS), 0, s, L, M, ld, c, m,
                       (double)sign, a == 0 ? 1 : 0, out, ldo);
    NH_CHECK_HIP(hipGetLastError());
  }
  return NH_OK;
}

extern "C" int nh_psis_weights(nh_ctx* ctx, const double* lr, long long M, int ncol, long long ld,
                               int Mt, const double* lsel, double* lw, long long ldw,
                               double* pareto_k, long long* n_tail, double* ess, double* lmean,
                               int* status) {
  NH_REQUIRE(ctx && lr && lsel && lw && pareto_k && n_tail && ess && lmean && status,
             "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_INT);
  NH_REQUIRE(ldw >= ncol, "ncol > ldw");
  NH_REQUIRE(Mt >= 0 && Mt < M, "Mt outside [0, M)");
  NH_REQUIRE(Mt <= NH_PSIS_MAX_TAIL, "Mt > NH_PSIS_MAX_TAIL: thin the chain");
  const int cap = std::max(Mt, 1);
  const colred_grid g = colred_plan(M, ncol);
  NH_REQUIRE_PLAN(g);
  const long long nch = g.nch;
  // scratch: part [nch][3][ncol] (its first third is k_rw_max's pm before) | pc [nch][2][ncol] |
  // cst [3][ncol] | tx [ncol][cap] | trow [ncol][cap] | cnt [ncol]
  const size_t npart = (size_t)nch * 3 * ncol, npc = (size_t)nch * 2 * ncol;
  const size_t nlist = (size_t)ncol * cap;
  void* base = nullptr;
  int rc = nh_scratch(ctx, (npart + npc + 3 * (size_t)ncol + nlist) * 8 + nlist * 4 + (size_t)ncol * 4,
                      &base);
  if (rc) return rc;
  double* part = (double*)base;
  long long* pc = (long long*)(part + npart);
  double* cst = (double*)(pc + npc);
  double* tx = cst + 3 * (size_t)ncol;
  int* trow = (int*)(tx + nlist);
  unsigned* cnt = (unsigned*)(trow + nlist);
  hipStream_t s = ctx->stream;
  const unsigned cb = g.col_blocks();
  const colred_out maxes = colred_dense<k_rw_max>(part, pc);
  const colred_out sums = {part, nullptr, 3, 2}, sq = {part + ncol, nullptr, 3, 1};  // slots 0, 2 | 1
  NH_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)ncol * 4, s));
  if ((rc = colred_launch<k_rw_max>(s, g, maxes, lr, ld))) return rc;
  hipLaunchKernelGGL(k_rw_max_fin, dim3(cb), dim3(PO_THREADS), 0, s, nch, ncol, M, cst, status, maxes);
  NH_CHECK_HIP(hipGetLastError());
  if ((rc = colred_launch<k_rw_split>(s, g, sums, lr, ld, cst, status, lsel, cap, tx, trow, cnt)))
    return rc;
  hipLaunchKernelGGL(k_rw_tail, dim3((unsigned)ncol), dim3(PO_THREADS), 0, s, ncol, M, nch, cap, cst,
                     status, lsel, sums, tx, trow, cnt, lw, ldw, pareto_k, n_tail, lmean);
  NH_CHECK_HIP(hipGetLastError());
  if ((rc = colred_launch<k_rw_write>(s, g, sq, lr, ld, cst, status, lsel, ncol, lw, ldw))) return rc;
  hipLaunchKernelGGL(k_rw_ess, dim3(cb), dim3(PO_THREADS), 0, s, nch, ncol, cst, status, ess, sq);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_weighted_moments(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                                   const double* lw, long long ldw, double* out) {
  NH_REQUIRE(ctx && x && lw && out, "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_INT);
  NH_REQUIRE(ldw >= 1, "ldw must be positive");
  const colred_grid g = colred_plan(M, ncol);
  NH_REQUIRE_PLAN(g);
  const long long nch = g.nch;
  // scratch: pd [nch][4][ncol] | pc [nch][2][ncol] | pq [nch][ncol] | mst [2][ncol]
  const size_t nc = (size_t)nch * ncol;
  void* base = nullptr;
  int rc = nh_scratch(ctx, (nc * 7 + 2 * (size_t)ncol) * 8, &base);
  if (rc) return rc;
  double* pd = (double*)base;
  long long* pc = (long long*)(pd + nc * 4);
  double* pq = (double*)(pc + nc * 2);
  double* mst = pq + nc;
  hipStream_t s = ctx->stream;
  const unsigned cb = g.col_blocks();
  const colred_out sums = colred_dense<k_rw_wsum>(pd, pc), sq = colred_dense<k_rw_wsq>(pq);
  if ((rc = colred_launch<k_rw_wsum>(s, g, sums, x, ld, lw, ldw))) return rc;
  hipLaunchKernelGGL(k_rw_wmean, dim3(cb), dim3(PO_THREADS), 0, s, nch, ncol, out, mst, sums);
  NH_CHECK_HIP(hipGetLastError());
  if ((rc = colred_launch<k_rw_wsq>(s, g, sq, x, ld, lw, ldw, out, ncol))) return rc;
  hipLaunchKernelGGL(k_rw_wvar, dim3(cb), dim3(PO_THREADS), 0, s, nch, ncol, mst, out, sq);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_weighted_select(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                                  const double* lw, long long ldw, const double* q, int nq,
                                  double* out) {
  NH_REQUIRE(ctx && x && lw && q && out, "null argument");
  NH_REQUIRE_MATRIX(M, ncol, ld, NH_ROWS_INT);
  NH_REQUIRE(ldw >= 1, "ldw must be positive");
  NH_REQUIRE(nq >= 1 && nq <= RW_MAX_Q, "nq must be in [1, 16]");
  rw_q qs = {};
  for (int j = 0; j < nq; ++j) {
    if (!(q[j] >= 0.0 && q[j] <= 1.0))
      return nh_set_error(NH_EINVAL, "nh_weighted_select: q[%d] is %g, outside [0, 1]", j, q[j]);
    qs.q[j] = q[j];
  }
  const unsigned nblk = (unsigned)cdiv(M, RW_TILE);
  // per column, behind the sort's buffers: bsum [nblk] | boff [nblk] | total | nanflag (8 bytes)
  const size_t extra = (size_t)nblk * 16 + 16;
  const int G = rk_group(M, ncol, extra);
  void* base = nullptr;
  int rc = nh_scratch(ctx, (rk_bytes_per_column(M) + extra) * G, &base);
  if (rc) return rc;
  const rk_buffers b(base, M, G);
  double* bsum = (double*)((char*)base + rk_bytes_per_column(M) * G);
  double* boff = bsum + (size_t)G * nblk;
  double* total = boff + (size_t)G * nblk;
  int* nanflag = (int*)(total + G);
  hipStream_t s = ctx->stream;
  const unsigned eb = (unsigned)cdiv(M, PO_THREADS);
  for (int c0 = 0; c0 < ncol; c0 += G) {
    const int g = std::min(G, ncol - c0);
    NH_CHECK_HIP(hipMemsetAsync(nanflag, 0, (size_t)g * 4, s));
    hipLaunchKernelGGL(k_rw_keys, dim3(eb, g), dim3(PO_THREADS), 0, s, x, M, ld, lw, ldw, c0, b.keys,
                       nanflag);
    NH_CHECK_HIP(hipGetLastError());
    const unsigned* in = nullptr;
    rc = rk_sort(s, b, M, g, &in);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rw_tile_sums, dim3(nblk, g), dim3(PO_THREADS), 0, s, lw, ldw, in, M, nblk,
                       bsum);
    NH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rw_tile_scan, dim3((unsigned)cdiv(g, PO_THREADS)), dim3(PO_THREADS), 0, s,
                       bsum, nblk, g, boff, total, nanflag, c0, ncol, nq, out);
    NH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rw_pick, dim3(nblk, g), dim3(PO_THREADS), 0, s, x, ld, lw, ldw, in, M, nblk,
                       boff, total, c0, ncol, qs, nq, out);
    NH_CHECK_HIP(hipGetLastError());
  }
  return NH_OK;
}

extern "C" int nh_resample_systematic(nh_ctx* ctx, const double* lw, long long ldw, long long M,
                                      double u0, long long n_out, long long* idx) {
  NH_REQUIRE(ctx && lw && idx, "null argument");
  NH_REQUIRE(M > 0, "M == 0: no samples");
  NH_REQUIRE(M < (1ll << 31), "M >= 2^31 rows");
  NH_REQUIRE(ldw >= 1, "ldw must be positive");
  NH_REQUIRE(u0 >= 0.0 && u0 < 1.0, "u0 outside [0, 1)");
  NH_REQUIRE(n_out >= 1 && n_out < (1ll << 31), "n_out outside [1, 2^31)");
  const unsigned nblk = (unsigned)cdiv(M, RW_TILE);
  // scratch: bsum [nblk] | boff [nblk] | total | cs [M]
  void* base = nullptr;
  int rc = nh_scratch(ctx, ((size_t)nblk * 2 + 1 + (size_t)M) * 8, &base);
  if (rc) return rc;
  double* bsum = (double*)base;
  double* boff = bsum + nblk;
  double* total = boff + nblk;
  double* cs = total + 1;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(k_rw_tile_sums, dim3(nblk, 1), dim3(PO_THREADS), 0, s, lw, ldw,
                     (const unsigned*)nullptr, M, nblk, bsum);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_rw_tile_scan, dim3(1), dim3(PO_THREADS), 0, s, bsum, nblk, 1, boff, total,
                     (const int*)nullptr, 0, 0, 0, (double*)nullptr);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_rw_cumsum, dim3(nblk), dim3(PO_THREADS), 0, s, lw, ldw, M, boff, cs);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_rw_draw, dim3(rw_grid(n_out)), dim3(PO_THREADS), 0, s, cs, M, total, u0, n_out,
                     idx);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_gather_rows(nh_ctx* ctx, const double* x, long long ld, const long long* idx,
                              long long n_out, int ncol, double* out, long long ldo) {
  NH_REQUIRE(ctx && x && idx && out, "null argument");
  NH_REQUIRE(n_out >= 1 && n_out < (1ll << 31), "n_out outside [1, 2^31)");
  NH_REQUIRE(ncol > 0, "ncol must be positive");
  NH_REQUIRE(ld >= ncol && ldo >= ncol, "ncol > ld or ncol > ldo");
  hipLaunchKernelGGL(k_rw_gather, dim3(rw_grid(n_out * ncol)), dim3(PO_THREADS), 0, ctx->stream, x, ld,
                     idx, n_out, ncol, out, ldo);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
