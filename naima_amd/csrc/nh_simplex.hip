// nh_simplex.hip -- the bookkeeping of S independent Nelder-Mead searches that advance in
// lock-step (naima_amd/optimize.py): the simplexes live in HBM, their candidate points are written
// straight into a parameter block qT[ndim][columns] (the layout of DPars) and the function values
// are read where the likelihood left them.  The model evaluation between propose and update is
// the caller's; per iteration the host reads two integers (nh_simplex_counts) and nothing else.
//
// The algorithm is naima_amd/neldermead.py's minimize_batched, decision for decision, for every
// simplex on the reduced function of its FREE coordinates (a frozen coordinate holds its pinned
// value in every point, is never perturbed and enters no tolerance test).  Two rules are fixed
// where NumPy leaves them open: a function value that is NaN counts as +inf, and the sort is
// stable -- ties keep their previous order, the replaced point sitting last before the sort.
//
// State (one block of nh_simplex_bytes(S, ndim, nmax) bytes, P = nmax + 1 points), structure of
// arrays over the simplex index s so that consecutive lanes touch consecutive words:
//   sim  [P][ndim][S] double   the points, by STORAGE slot
//   fsim [P][S]       double   their function values
//   order[P][S]       int      order[r] = the slot of the point of rank r (0 best, nfree worst)
//   fidx [ndim][S]    int      the free coordinates, ascending (nfree of them)
//   nfree, nit, nfev, status, shrink, maxit, maxfev, list [S] int; counts [2] int
// The order is a permutation in HBM: nothing here is a per-lane array, so nothing goes to
// scratch.  One lane per simplex; tail lanes of the last workgroup do nothing.  S is tens to a
// few thousand and the model evaluation dominates an iteration by orders of magnitude.
//
// Arithmetic is the host code's, operation for operation (the centroid is the rank-by-rank sum
// of the N best points, then / N; candidates are (1 + rho) xbar - rho worst and so on), with FP
// contraction off for the whole file, so a simplex follows the host algorithm bit for bit.
// counts = { simplexes still active, simplexes that want a shrink } and the ordered list of the
// latter come from a one-workgroup scan in index order: no atomics, nothing depends on timing.
#include "nh_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SX_THREADS = 64;
constexpr int SX_SCAN = 256;
constexpr int SX_ACTIVE = -1;
constexpr int SX_INVALID = 3;

struct sx_state {
  double* sim;
  double* fsim;
  int* order;
  int* fidx;
  int* nfree;
  int* nit;
  int* nfev;
  int* status;
  int* shrink;
  int* maxit;
  int* maxfev;
  int* list;
  int* counts;
  int S, D, P;
};

size_t sx_bytes(long long S, long long D, long long P) {
  const long long dbl = P * D * S + P * S, ints = P * S + D * S + 8 * S + 2;
  return (size_t)(8 * dbl + 4 * ((ints + 1) / 2 * 2));
}

sx_state sx_layout(void* base, int S, int D, int nmax) {
  sx_state st;
  const long long P = nmax + 1, s = S, d = D;
  st.S = S, st.D = D, st.P = (int)P;
  st.sim = (double*)base;
  st.fsim = st.sim + P * d * s;
  st.order = (int*)(st.fsim + P * s);
  st.fidx = st.order + P * s;
  st.nfree = st.fidx + d * s;
  st.nit = st.nfree + s;
  st.nfev = st.nit + s;
  st.status = st.nfev + s;
  st.shrink = st.status + s;
  st.maxit = st.shrink + s;
  st.maxfev = st.maxit + s;
  st.list = st.maxfev + s;
  st.counts = st.list + s;
  return st;
}

__device__ __forceinline__ double sx_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

__device__ __forceinline__ long long sx_at(const sx_state& st, int slot, int d, int s) {
  return ((long long)slot * st.D + d) * st.S + s;
}

// the function value of column col: negated where f is a log-probability, NaN -> +inf
__device__ __forceinline__ double sx_val(const double* __restrict__ f, long long stride,
                                         long long col, int negate) {
  double v = f[col * stride];
  if (negate) v = -v;
  return v != v ? sx_inf() : v;
}

// stable insertion sort of the ranks 0..N by function value, from the order they have
__device__ void sx_sort(const sx_state& st, int s, int N) {
  const long long S = st.S;
  for (int r = 1; r <= N; ++r) {
    const int slot = st.order[r * S + s];
    const double kf = st.fsim[slot * S + s];
    int j = r - 1;
    while (j >= 0) {
      const int oj = st.order[j * S + s];
      if (!(st.fsim[oj * S + s] > kf)) break;
      st.order[(j + 1) * S + s] = oj;
      --j;
    }
    st.order[(j + 1) * S + s] = slot;
  }
}

// neldermead.py:36-38 and :75 once nit and nfev are what the iteration left: the limits first,
// then the relative tolerances on the free coordinates (a NaN in either test: not converged)
__device__ void sx_check(const sx_state& st, int s, int N, int nit, int nfev, double xtol,
                         double ftol) {
  const long long S = st.S;
  if (nfev >= st.maxfev[s]) {
    st.status[s] = 1;
    return;
  }
  if (nit >= st.maxit[s]) {
    st.status[s] = 2;
    return;
  }
  const int o0 = st.order[s];
  const double f0 = st.fsim[o0 * S + s];
  double xm = 0.0, fm = 0.0;
  bool bad = false;
  for (int j = 1; j <= N; ++j) {
    const int oj = st.order[j * S + s];
    const double v = fabs((f0 - st.fsim[oj * S + s]) / f0);
    if (v != v) bad = true;
    else if (v > fm) fm = v;
    for (int k = 0; k < N; ++k) {
      const int d = st.fidx[k * S + s];
      const double a = st.sim[sx_at(st, o0, d, s)];
      const double u = fabs((st.sim[sx_at(st, oj, d, s)] - a) / a);
      if (u != u) bad = true;
      else if (u > xm) xm = u;
    }
  }
  if (!bad && xm <= xtol && fm <= ftol) st.status[s] = 0;
}

// ---------------------------------------------------------------- initial simplex
__global__ __launch_bounds__(SX_THREADS) void k_sx_init(
    sx_state st, const double* __restrict__ x0, const int* __restrict__ frozen,
    const double* __restrict__ value, int maxiter, int maxfev, double* __restrict__ qT) {
  const int s = blockIdx.x * SX_THREADS + threadIdx.x;
  if (s >= st.S) return;
  const long long S = st.S;
  const int D = st.D, P = st.P;
  int n = 0;
  bool over = false;
  for (int d = 0; d < D; ++d)
    if (!(frozen && frozen[(long long)s * D + d])) {
      if (n < P - 1) st.fidx[n++ * S + s] = d;
      else over = true;
    }
  const bool valid = n >= 1 && !over;
  if (!valid) n = 0;
  st.nfree[s] = n;
  st.nit[s] = 0;
  st.nfev[s] = 0;
  st.shrink[s] = 0;
  st.status[s] = valid ? SX_ACTIVE : SX_INVALID;
  st.maxit[s] = maxiter >= 0 ? maxiter : 200 * n;
  st.maxfev[s] = maxfev >= 0 ? maxfev : 200 * n;
  for (int p = 0; p < P; ++p) {
    st.order[p * S + s] = p;
    st.fsim[p * S + s] = sx_inf();
    const int moved = p >= 1 && p <= n ? st.fidx[(p - 1) * S + s] : -1;
    for (int d = 0; d < D; ++d) {
      const long long e = (long long)s * D + d;
      double v = frozen && frozen[e] ? value[e] : x0[e];
      if (d == moved) v = v != 0.0 ? 1.05 * v : 0.00025;
      st.sim[sx_at(st, p, d, s)] = v;
      qT[(long long)d * P * S + p * S + s] = v;
    }
  }
}

__global__ __launch_bounds__(SX_THREADS) void k_sx_adopt(sx_state st, const double* __restrict__ f,
                                                         long long stride, int negate, double xtol,
                                                         double ftol) {
  const int s = blockIdx.x * SX_THREADS + threadIdx.x;
  if (s >= st.S || st.status[s] != SX_ACTIVE) return;
  const long long S = st.S;
  const int N = st.nfree[s];
  for (int p = 0; p <= N; ++p) st.fsim[p * S + s] = sx_val(f, stride, p * S + s, negate);
  sx_sort(st, s, N);
  st.nfev[s] = N + 1;
  st.nit[s] = 1;
  sx_check(st, s, N, 1, N + 1, xtol, ftol);
}

// ---------------------------------------------------------------- one iteration
__global__ __launch_bounds__(SX_THREADS) void k_sx_propose(sx_state st, double* __restrict__ qT) {
  const int s = blockIdx.x * SX_THREADS + threadIdx.x;
  if (s >= st.S) return;
  const long long S = st.S;
  const int D = st.D, N = st.nfree[s];
  const bool active = st.status[s] == SX_ACTIVE;
  // a finished simplex proposes its best point four times; an active one its worst point's
  // frozen coordinates, which are every point's
  const int src = st.order[(active ? N : 0) * S + s];
  for (int d = 0; d < D; ++d) {
    const double v = st.sim[sx_at(st, src, d, s)];
    double* q = qT + (long long)d * 4 * S + s;
    q[0] = v, q[S] = v, q[2 * S] = v, q[3 * S] = v;
  }
  if (!active) return;
  for (int k = 0; k < N; ++k) {
    const int d = st.fidx[k * S + s];
    double acc = st.sim[sx_at(st, st.order[s], d, s)];
    for (int r = 1; r < N; ++r) acc = acc + st.sim[sx_at(st, st.order[r * S + s], d, s)];
    const double xbar = acc / (double)N;
    const double w = st.sim[sx_at(st, src, d, s)];
    double* q = qT + (long long)d * 4 * S + s;
    q[0] = 2.0 * xbar - 1.0 * w;      // reflection          (1 + rho) xbar - rho worst
    q[S] = 3.0 * xbar - 2.0 * w;      // expansion           (1 + rho chi) xbar - rho chi worst
    q[2 * S] = 1.5 * xbar - 0.5 * w;  // outside contraction (1 + psi rho) xbar - psi rho worst
    q[3 * S] = 0.5 * xbar + 0.5 * w;  // inside contraction  (1 - psi) xbar + psi worst
  }
}

__global__ __launch_bounds__(SX_THREADS) void k_sx_update(
    sx_state st, const double* __restrict__ qT, const double* __restrict__ f, long long stride,
    int negate, double xtol, double ftol) {
  const int s = blockIdx.x * SX_THREADS + threadIdx.x;
  if (s >= st.S || st.status[s] != SX_ACTIVE || st.shrink[s]) return;
  const long long S = st.S;
  const int N = st.nfree[s];
  const double fxr = sx_val(f, stride, s, negate), fxe = sx_val(f, stride, S + s, negate);
  const double fxc = sx_val(f, stride, 2 * S + s, negate);
  const double fxcc = sx_val(f, stride, 3 * S + s, negate);
  const int ow = st.order[N * S + s];
  const double f0 = st.fsim[st.order[s] * S + s];
  const double fs = st.fsim[st.order[(N - 1) * S + s] * S + s];  // fsim[-2]
  const double fw = st.fsim[ow * S + s];
  int nfev = st.nfev[s] + 1, pick;  // neldermead.py:47-67
  if (fxr < f0) {
    nfev += 1;
    pick = fxe < fxr ? 1 : 0;
  } else if (fxr < fs) {
    pick = 0;
  } else {
    nfev += 1;
    if (fxr < fw) pick = fxc <= fxr ? 2 : -1;
    else pick = fxcc < fw ? 3 : -1;
  }
  st.nfev[s] = nfev;
  if (pick < 0) {
    st.shrink[s] = 1;  // nh_simplex_shrink_adopt finishes the iteration
    return;
  }
  const double fv = pick == 0 ? fxr : pick == 1 ? fxe : pick == 2 ? fxc : fxcc;
  for (int k = 0; k < N; ++k) {
    const int d = st.fidx[k * S + s];
    st.sim[sx_at(st, ow, d, s)] = qT[(long long)d * 4 * S + pick * S + s];
  }
  st.fsim[ow * S + s] = fv;
  // the stable sort of a sorted prefix and the new value behind it: the new point goes
  // behind every point that is not worse
  int j = N - 1;
  while (j >= 0) {
    const int oj = st.order[j * S + s];
    if (!(st.fsim[oj * S + s] > fv)) break;
    st.order[(j + 1) * S + s] = oj;
    --j;
  }
  st.order[(j + 1) * S + s] = ow;
  const int nit = st.nit[s] + 1;
  st.nit[s] = nit;
  sx_check(st, s, N, nit, nfev, xtol, ftol);
}

// counts[0] = simplexes still active, counts[1] = those that want a shrink, list = the latter in
// index order.  One workgroup: thread t takes the simplexes [t * per, (t + 1) * per).
__global__ __launch_bounds__(SX_SCAN) void k_sx_scan(sx_state st) {
  __shared__ int na[SX_SCAN], ns[SX_SCAN];
  const int t = threadIdx.x, per = (st.S + SX_SCAN - 1) / SX_SCAN;
  const int a = min(st.S, t * per), b = min(st.S, a + per);
  int ca = 0, cs = 0;
  for (int s = a; s < b; ++s) {
    ca += st.status[s] == SX_ACTIVE;
    cs += st.shrink[s] != 0;
  }
  na[t] = ca;
  ns[t] = cs;
  __syncthreads();
  int before = 0;
  for (int u = 0; u < t; ++u) before += ns[u];
  for (int s = a; s < b; ++s)
    if (st.shrink[s]) st.list[before++] = s;
  if (t == 0) {
    int ta = 0, ts = 0;
    for (int u = 0; u < SX_SCAN; ++u) ta += na[u], ts += ns[u];
    st.counts[0] = ta;
    st.counts[1] = ts;
  }
}

// ---------------------------------------------------------------- shrink
// entry k of the list: the points of rank 1..nmax move half way to the best one (:69); column
// (j - 1) * nshrink + k is the point of rank j (the best point where the simplex has fewer)
__global__ __launch_bounds__(SX_THREADS) void k_sx_shrink_points(sx_state st, int nshrink,
                                                                 double* __restrict__ qT) {
  const int k = blockIdx.x * SX_THREADS + threadIdx.x;
  if (k >= nshrink) return;
  const int s = st.list[k];
  if (s < 0 || s >= st.S || !st.shrink[s]) return;  // (nshrink is not what the last scan counted)
  const long long S = st.S, ldq = (long long)(st.P - 1) * nshrink;
  const int D = st.D, N = st.nfree[s], o0 = st.order[s];
  for (int j = 1; j < st.P; ++j) {
    const int slot = j <= N ? st.order[j * S + s] : o0;
    double* q = qT + (long long)(j - 1) * nshrink + k;
    for (int d = 0; d < D; ++d) q[d * ldq] = st.sim[sx_at(st, slot, d, s)];
    if (j > N) continue;
    for (int c = 0; c < N; ++c) {
      const int d = st.fidx[c * S + s];
      const double b = st.sim[sx_at(st, o0, d, s)];
      const double v = b + 0.5 * (st.sim[sx_at(st, slot, d, s)] - b);
      st.sim[sx_at(st, slot, d, s)] = v;
      q[d * ldq] = v;
    }
  }
}

__global__ __launch_bounds__(SX_THREADS) void k_sx_shrink_adopt(
    sx_state st, int nshrink, const double* __restrict__ f, long long stride, int negate,
    double xtol, double ftol) {
  const int k = blockIdx.x * SX_THREADS + threadIdx.x;
  if (k >= nshrink) return;
  const int s = st.list[k];
  if (s < 0 || s >= st.S || !st.shrink[s]) return;
  const long long S = st.S;
  const int N = st.nfree[s];
  for (int j = 1; j <= N; ++j)
    st.fsim[st.order[j * S + s] * S + s] = sx_val(f, stride, (long long)(j - 1) * nshrink + k, negate);
  sx_sort(st, s, N);
  const int nfev = st.nfev[s] + N, nit = st.nit[s] + 1;
  st.nfev[s] = nfev;
  st.nit[s] = nit;
  st.shrink[s] = 0;
  sx_check(st, s, N, nit, nfev, xtol, ftol);
}

// ---------------------------------------------------------------- result
__global__ __launch_bounds__(SX_THREADS) void k_sx_result(sx_state st, double* __restrict__ x,
                                                          double* __restrict__ fun,
                                                          int* __restrict__ ints) {
  const int s = blockIdx.x * SX_THREADS + threadIdx.x;
  if (s >= st.S) return;
  const long long S = st.S;
  const int o0 = st.order[s];
  for (int d = 0; d < st.D; ++d) x[(long long)s * st.D + d] = st.sim[sx_at(st, o0, d, s)];
  fun[s] = st.fsim[o0 * S + s];
  ints[s] = st.nfev[s];
  ints[S + s] = st.nit[s];
  ints[2 * S + s] = st.status[s];
  ints[3 * S + s] = st.nfree[s];
}

int sx_check_dims(const char* fn, int S, int ndim, int nmax) {
  if (S < 1 || ndim < 1 || ndim > NH_SIMPLEX_MAX_DIM || nmax < 1 || nmax > ndim)
    return nh_set_error(NH_EINVAL, "%s: S < 1, ndim outside [1, NH_SIMPLEX_MAX_DIM] or nmax outside [1, ndim]", fn);
  if ((long long)S * (nmax + 1) * ndim >= (1ll << 31))
    return nh_set_error(NH_EINVAL, "%s: S * (nmax + 1) * ndim >= 2^31", fn);
  return NH_OK;
}

unsigned sx_grid(int n) { return (unsigned)((n + SX_THREADS - 1) / SX_THREADS); }

}  // namespace

extern "C" long long nh_simplex_bytes(int S, int ndim, int nmax) {
  if (S < 1 || ndim < 1 || ndim > NH_SIMPLEX_MAX_DIM || nmax < 1 || nmax > ndim) return 0;
  if ((long long)S * (nmax + 1) * ndim >= (1ll << 31)) return 0;
  return (long long)sx_bytes(S, ndim, nmax + 1);
}

extern "C" int nh_simplex_init_points(nh_ctx* ctx, void* state, int S, int ndim, int nmax,
                                      const double* x0, const int* frozen, const double* value,
                                      int maxiter, int maxfev, double* qT) {
  NH_REQUIRE(ctx && state && x0 && qT, "null argument");
  NH_REQUIRE(!frozen == !value, "frozen and value come together");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sx_init, dim3(sx_grid(S)), dim3(SX_THREADS), 0, ctx->stream,
                     sx_layout(state, S, ndim, nmax), x0, frozen, value, maxiter, maxfev, qT);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_simplex_adopt(nh_ctx* ctx, void* state, int S, int ndim, int nmax,
                                const double* f, long long fstride, int is_logp, double xtol,
                                double ftol) {
  NH_REQUIRE(ctx && state && f && fstride >= 1, "null argument or fstride < 1");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  const sx_state st = sx_layout(state, S, ndim, nmax);
  hipLaunchKernelGGL(k_sx_adopt, dim3(sx_grid(S)), dim3(SX_THREADS), 0, ctx->stream, st, f,
                     fstride, is_logp != 0, xtol, ftol);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_sx_scan, dim3(1), dim3(SX_SCAN), 0, ctx->stream, st);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_simplex_propose(nh_ctx* ctx, void* state, int S, int ndim, int nmax,
                                  double* qT) {
  NH_REQUIRE(ctx && state && qT, "null argument");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sx_propose, dim3(sx_grid(S)), dim3(SX_THREADS), 0, ctx->stream,
                     sx_layout(state, S, ndim, nmax), qT);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_simplex_update(nh_ctx* ctx, void* state, int S, int ndim, int nmax,
                                 const double* qT, const double* f, long long fstride,
                                 int is_logp, double xtol, double ftol) {
  NH_REQUIRE(ctx && state && qT && f && fstride >= 1, "null argument or fstride < 1");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  const sx_state st = sx_layout(state, S, ndim, nmax);
  hipLaunchKernelGGL(k_sx_update, dim3(sx_grid(S)), dim3(SX_THREADS), 0, ctx->stream, st, qT, f,
                     fstride, is_logp != 0, xtol, ftol);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_sx_scan, dim3(1), dim3(SX_SCAN), 0, ctx->stream, st);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_simplex_counts(nh_ctx* ctx, const void* state, int S, int ndim, int nmax,
                                 int* counts) {
  NH_REQUIRE(ctx && state && counts, "null argument");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  const sx_state st = sx_layout(const_cast<void*>(state), S, ndim, nmax);
  NH_CHECK_HIP(hipMemcpyAsync(counts, st.counts, 2 * sizeof(int), hipMemcpyDeviceToHost,
                              ctx->stream));
  NH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return NH_OK;
}

extern "C" int nh_simplex_shrink_points(nh_ctx* ctx, void* state, int S, int ndim, int nmax,
                                        int nshrink, double* qT) {
  NH_REQUIRE(ctx && state && qT, "null argument");
  NH_REQUIRE(nshrink >= 1 && nshrink <= S, "nshrink outside [1, S]");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sx_shrink_points, dim3(sx_grid(nshrink)), dim3(SX_THREADS), 0, ctx->stream,
                     sx_layout(state, S, ndim, nmax), nshrink, qT);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_simplex_shrink_adopt(nh_ctx* ctx, void* state, int S, int ndim, int nmax,
                                       int nshrink, const double* f, long long fstride,
                                       int is_logp, double xtol, double ftol) {
  NH_REQUIRE(ctx && state && f && fstride >= 1, "null argument or fstride < 1");
  NH_REQUIRE(nshrink >= 1 && nshrink <= S, "nshrink outside [1, S]");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  const sx_state st = sx_layout(state, S, ndim, nmax);
  hipLaunchKernelGGL(k_sx_shrink_adopt, dim3(sx_grid(nshrink)), dim3(SX_THREADS), 0, ctx->stream,
                     st, nshrink, f, fstride, is_logp != 0, xtol, ftol);
  NH_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_sx_scan, dim3(1), dim3(SX_SCAN), 0, ctx->stream, st);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}

extern "C" int nh_simplex_result(nh_ctx* ctx, const void* state, int S, int ndim, int nmax,
                                 double* x, double* fun, int* ints) {
  NH_REQUIRE(ctx && state && x && fun && ints, "null argument");
  int rc = sx_check_dims(__func__, S, ndim, nmax);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sx_result, dim3(sx_grid(S)), dim3(SX_THREADS), 0, ctx->stream,
                     sx_layout(const_cast<void*>(state), S, ndim, nmax), x, fun, ints);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
