// nh_select.hip -- exact per-column order statistics of a device matrix (nh_column_select):
// the confidence bands of naima's plots, np.sort(model[:, i])[nf] for every energy i
// (plot.py:438-501), without sorting and without bringing the samples to the host.
//
// Every double is mapped to an order-preserving 64-bit key (negatives: all bits flipped; the
// rest: the sign bit flipped; every NaN: ~0, after +inf as NumPy sorts).  The first kernel
// writes the keys of the ncol columns COLUMN-MAJOR into library scratch (one read of x through
// an LDS tile transpose), so that the eight radix passes after it read each column as one
// contiguous, coalesced run of rows.  Each pass resolves one 8-bit digit of every
// (column, rank)'s answer, most significant first:
//   k_sel_hist  a histogram in LDS (32-bit integer LDS atomics) of the digit of the keys that
//               still match the prefix resolved so far, merged into global bins with agent-scope
//               integer atomics (order-independent: the result is bit-reproducible);
//   k_sel_pick  one workgroup per column: a scan of the bins finds the digit the remaining rank
//               falls in, narrows prefix and rank, and clears the column's bins.
// Ranks whose prefixes agree (all of them in the first pass) share one histogram.  Every launch
// is on the context's stream; nothing synchronises with the host.
#include "nh_common.h"

#include <algorithm>

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_TILE = 64;          // rows x columns of the transpose tile
constexpr int SEL_LDS_HISTS = 32;     // (column, rank) histograms per workgroup: 32 KiB of LDS

struct sel_ranks { int r[NH_SELECT_MAX_RANKS]; };

__device__ __forceinline__ unsigned long long sel_key(double v) {
  if (v != v) return ~0ull;  // every NaN, whatever its sign and payload
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double sel_value(unsigned long long k) {
  if (k == ~0ull) return nh_nan();
  unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// state of the selection: prefix[ncol*R], rem[ncol*R] (rank still to find among the keys that
// match the prefix), alias[ncol*R] (the first rank of the column with the same prefix: whose
// histogram this rank reads), bins[ncol*R*256]
__global__ void k_sel_init(unsigned long long* prefix, unsigned* rem, int* alias, unsigned* bins,
                           int ncol, int R, sel_ranks ranks) {
  long long nstate = (long long)ncol * R;
  long long nbins = nstate * 256;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nbins;
       i += (long long)gridDim.x * blockDim.x) {
    bins[i] = 0u;
    if (i < nstate) {
      int r = (int)(i % R);
      prefix[i] = 0ull;
      rem[i] = (unsigned)ranks.r[r];
      alias[i] = 0;  // no digit resolved yet: one histogram per column
    }
  }
}

// keys[c][row] = sel_key(x[row][c]) for c < ncol, row < M
__global__ __launch_bounds__(SEL_THREADS) void k_sel_keys(const double* __restrict__ x, long long M,
                                                          int ncol, long long ld,
                                                          unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long tile[SEL_TILE][SEL_TILE + 1];
  long long r0 = (long long)blockIdx.x * SEL_TILE;
  int c0 = blockIdx.y * SEL_TILE;
  int tx = threadIdx.x % SEL_TILE, ty = threadIdx.x / SEL_TILE;
  for (int i = ty; i < SEL_TILE; i += SEL_THREADS / SEL_TILE) {
    long long row = r0 + i;
    int c = c0 + tx;
    if (row < M && c < ncol) tile[i][tx] = sel_key(x[row * ld + c]);
  }
  __syncthreads();
  for (int j = ty; j < SEL_TILE; j += SEL_THREADS / SEL_TILE) {
    long long row = r0 + tx;
    int c = c0 + j;
    if (row < M && c < ncol) keys[(long long)c * M + row] = tile[tx][j];
  }
}

// one pass: histogram of digit (key >> shift) & 255 over the keys of columns [c0, c0+ct) and
// rows [row0, row1) that match the resolved prefix of each histogram-owning rank
__global__ __launch_bounds__(SEL_THREADS) void k_sel_hist(const unsigned long long* __restrict__ keys,
                                                          long long M, int ncol, int R, int ct,
                                                          long long rows_per_block, int shift,
                                                          const unsigned long long* __restrict__ prefix,
                                                          const int* __restrict__ alias,
                                                          unsigned* __restrict__ bins) {
  extern __shared__ unsigned hist[];  // [ct][R][256]
  __shared__ unsigned long long pre[SEL_LDS_HISTS];
  __shared__ int own[SEL_LDS_HISTS];
  int c0 = blockIdx.x * ct;
  int nct = min(ct, ncol - c0);
  int nh = nct * R;
  for (int i = threadIdx.x; i < nh * 256; i += SEL_THREADS) hist[i] = 0u;
  if (threadIdx.x < nh) {
    int s = (c0 + threadIdx.x / R) * R + threadIdx.x % R;
    pre[threadIdx.x] = prefix[s];
    own[threadIdx.x] = alias[s] == threadIdx.x % R;
  }
  __syncthreads();
  // the bits above this pass's digit are resolved (none in the first pass)
  const unsigned long long hi = shift >= 56 ? 0ull : (~0ull << (shift + 8));
  long long row0 = (long long)blockIdx.y * rows_per_block;
  long long row1 = min(M, row0 + rows_per_block);
  for (int j = 0; j < nct; ++j) {
    const unsigned long long* col = keys + (long long)(c0 + j) * M;
    unsigned* hj = hist + j * R * 256;
    for (long long row = row0 + threadIdx.x; row < row1; row += SEL_THREADS) {
      unsigned long long k = col[row];
      unsigned d = (unsigned)(k >> shift) & 255u;
      for (int r = 0; r < R; ++r) {
        if (own[j * R + r] && ((k ^ pre[j * R + r]) & hi) == 0ull)
          __hip_atomic_fetch_add(hj + r * 256 + d, 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nh * 256; i += SEL_THREADS) {
    unsigned v = hist[i];
    if (v) __hip_atomic_fetch_add(bins + (long long)c0 * R * 256 + i, v, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
  }
}

// one workgroup per column: pick each rank's digit, narrow its prefix and rank, re-alias the
// ranks by prefix and clear the column's bins; after the last digit write the values
__global__ __launch_bounds__(SEL_THREADS) void k_sel_pick(int ncol, int R, int shift,
                                                          unsigned long long* prefix, unsigned* rem,
                                                          int* alias, unsigned* bins,
                                                          double* __restrict__ out) {
  __shared__ unsigned scan[SEL_THREADS];
  int c = blockIdx.x;
  int t = threadIdx.x;
  unsigned* cb = bins + (long long)c * R * 256;
  for (int r = 0; r < R; ++r) {
    int s = c * R + r;
    unsigned h = cb[alias[s] * 256 + t];
    scan[t] = h;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele scan of 256 bins
      unsigned v = t >= off ? scan[t - off] : 0u;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    unsigned incl = scan[t], excl = incl - h;
    unsigned k = rem[s];
    __syncthreads();  // every lane has read rem[s] before its owner moves it
    if (excl <= k && k < incl) {  // exactly one digit holds the k-th key
      prefix[s] |= (unsigned long long)t << shift;
      rem[s] = k - excl;
    }
    __syncthreads();
  }
  if (t == 0) {
    for (int r = 0; r < R; ++r) {
      int a = r;
      for (int q = 0; q < r; ++q)
        if (prefix[c * R + q] == prefix[c * R + r]) { a = q; break; }
      alias[c * R + r] = a;
    }
  }
  for (int i = t; i < R * 256; i += SEL_THREADS) cb[i] = 0u;
  if (shift == 0 && t < R) out[(long long)t * ncol + c] = sel_value(prefix[c * R + t]);
}

}  // namespace

extern "C" int nh_column_select(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                                const int* ranks, int R, double* out) {
  NH_REQUIRE(ctx && x && out && ranks, "null argument");
  NH_REQUIRE(M > 0, "M == 0: no samples to select from");
  NH_REQUIRE(M < (1ll << 31), "M >= 2^31 rows");
  NH_REQUIRE(ncol > 0, "ncol must be positive");
  NH_REQUIRE(ld >= ncol, "ncol > ld");
  NH_REQUIRE(R >= 1 && R <= NH_SELECT_MAX_RANKS, "R must be in [1, 16]");
  sel_ranks rk = {};
  for (int r = 0; r < R; ++r) {
    if (ranks[r] < 0 || ranks[r] >= M)
      return nh_set_error(NH_EINVAL, "nh_column_select: rank %d is %d, outside [0, %lld)", r,
                          ranks[r], M);
    rk.r[r] = ranks[r];
  }
  // scratch: keys [ncol][M] | bins [ncol][R][256] | prefix [ncol][R] | rem | alias
  size_t nstate = (size_t)ncol * R;
  size_t kbytes = (size_t)M * ncol * 8;
  size_t bbytes = nstate * 256 * 4;
  size_t total = kbytes + bbytes + nstate * 8 + nstate * 4 + nstate * 4;
  void* base = nullptr;
  int rc = nh_scratch(ctx, total, &base);
  if (rc) return rc;
  char* p = (char*)base;
  auto* keys = (unsigned long long*)p;
  auto* prefix = (unsigned long long*)(p + kbytes);
  auto* bins = (unsigned*)(p + kbytes + nstate * 8);
  auto* rem = (unsigned*)(p + kbytes + nstate * 8 + bbytes);
  auto* alias = (int*)(p + kbytes + nstate * 8 + bbytes + nstate * 4);
  hipStream_t s = ctx->stream;

  int ib = (int)std::min<size_t>((nstate * 256 + SEL_THREADS - 1) / SEL_THREADS, 1024);
  hipLaunchKernelGGL(k_sel_init, dim3(ib), dim3(SEL_THREADS), 0, s, prefix, rem, alias, bins, ncol,
                     R, rk);
  NH_CHECK_HIP(hipGetLastError());
  dim3 tg((unsigned)((M + SEL_TILE - 1) / SEL_TILE), (unsigned)((ncol + SEL_TILE - 1) / SEL_TILE));
  hipLaunchKernelGGL(k_sel_keys, tg, dim3(SEL_THREADS), 0, s, x, M, ncol, ld, keys);
  NH_CHECK_HIP(hipGetLastError());

  // column tile: as many columns as keep R histograms each within SEL_LDS_HISTS KiB of LDS;
  // row blocks: enough workgroups to fill the chip several times over, >= 1024 rows each
  int ct = std::max(1, SEL_LDS_HISTS / R);
  ct = std::min(ct, ncol);
  int ntile = (ncol + ct - 1) / ct;
  long long want = std::max(1, 2048 / ntile);
  long long rpb = std::max<long long>(1024, (M + want - 1) / want);
  rpb = (rpb + SEL_THREADS - 1) / SEL_THREADS * SEL_THREADS;
  unsigned nrb = (unsigned)((M + rpb - 1) / rpb);
  size_t lds = (size_t)ct * R * 256 * 4;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(k_sel_hist, dim3(ntile, nrb), dim3(SEL_THREADS), lds, s, keys, M, ncol, R, ct,
                       rpb, shift, prefix, alias, bins);
    NH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sel_pick, dim3(ncol), dim3(SEL_THREADS), 0, s, ncol, R, shift, prefix, rem,
                       alias, bins, out);
    NH_CHECK_HIP(hipGetLastError());
  }
  return NH_OK;
}
