// nh_radix.h -- the stable least-significant-digit radix sort of (64-bit key, row index) per column
// that nh_rank.hip and nh_reweight.hip share.  The keys of a group of g columns lie column-major
// [column][S] in library scratch; eight passes over 8-bit digits sort the row INDEX (the key is
// read through the index, so an element costs 16 bytes of scratch: key, and the index twice):
//   k_rank_hist     per-workgroup digit histogram in LDS (integer LDS atomics) -> counts
//                   [column][digit][workgroup];
//   k_rank_scan     one workgroup per column: exclusive scan in (digit, workgroup) order;
//   k_rank_scatter  stable scatter: a tile is walked in chunks of 256 in order; within a chunk a
//                   lane's offset is the number of lower lanes of its wave with the same digit
//                   (eight ballots) plus the counts of the lower waves -- no atomics, so equal
//                   digits keep their order and every pass is reproducible bit for bit.
// Equal keys therefore end in ascending row order: the sort is by (key, row index).
#pragma once
#include "nh_common.h"

#include <algorithm>

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_CHUNKS = 16;                     // chunks of RK_THREADS elements per tile
constexpr int RK_TILE = RK_THREADS * RK_CHUNKS;   // elements of a column per workgroup
constexpr size_t RK_BUDGET = (size_t)256 << 20;   // scratch per group of columns

// finite doubles (and +-inf) in their order, -0.0 == +0.0
__device__ __forceinline__ unsigned long long rk_key(double v) {
  if (v == 0.0) v = 0.0;  // -0.0 -> +0.0
  unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ unsigned rk_digit(const unsigned long long* __restrict__ keys,
                                             const unsigned* __restrict__ idx, long long i, int shift) {
  unsigned long long k = keys[idx ? (long long)idx[i] : i];
  return (unsigned)(k >> shift) & 255u;
}

// counts[(g * 256 + d) * nblk + b] = keys of column g's tile b with digit d
__global__ __launch_bounds__(RK_THREADS) void k_rank_hist(const unsigned long long* __restrict__ keys,
                                                          const unsigned* __restrict__ idx_in,
                                                          long long S, int shift, unsigned nblk,
                                                          unsigned* __restrict__ counts) {
  __shared__ unsigned hist[256];
  const unsigned long long* kc = keys + (long long)blockIdx.y * S;
  const unsigned* ic = idx_in ? idx_in + (long long)blockIdx.y * S : nullptr;
  hist[threadIdx.x] = 0u;
  __syncthreads();
  long long i0 = (long long)blockIdx.x * RK_TILE;
  for (int c = 0; c < RK_CHUNKS; ++c) {
    long long i = i0 + c * RK_THREADS + threadIdx.x;
    if (i < S)
      __hip_atomic_fetch_add(hist + rk_digit(kc, ic, i, shift), 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  counts[((long long)blockIdx.y * 256 + threadIdx.x) * nblk + blockIdx.x] = hist[threadIdx.x];
}

// one workgroup per column: counts -> where each (digit, tile) starts in the sorted column
__global__ __launch_bounds__(256) void k_rank_scan(unsigned* __restrict__ counts, unsigned nblk) {
  __shared__ unsigned scan[256];
  int t = threadIdx.x;
  unsigned* cd = counts + ((long long)blockIdx.x * 256 + t) * nblk;
  unsigned tot = 0u;
  for (unsigned b = 0; b < nblk; ++b) tot += cd[b];
  scan[t] = tot;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive Hillis-Steele scan of the 256 digits
    unsigned v = t >= off ? scan[t - off] : 0u;
    __syncthreads();
    scan[t] += v;
    __syncthreads();
  }
  unsigned run = scan[t] - tot;
  for (unsigned b = 0; b < nblk; ++b) {
    unsigned n = cd[b];
    cd[b] = run;
    run += n;
  }
}

__global__ __launch_bounds__(RK_THREADS) void k_rank_scatter(const unsigned long long* __restrict__ keys,
                                                             const unsigned* __restrict__ idx_in,
                                                             unsigned* __restrict__ idx_out,
                                                             long long S, int shift, unsigned nblk,
                                                             const unsigned* __restrict__ counts) {
  __shared__ unsigned base[256];             // where the next key of each digit goes
  __shared__ unsigned wcnt[RK_WAVES][256];   // this chunk's keys per (wave, digit)
  const unsigned long long* kc = keys + (long long)blockIdx.y * S;
  const unsigned* ic = idx_in ? idx_in + (long long)blockIdx.y * S : nullptr;
  unsigned* oc = idx_out + (long long)blockIdx.y * S;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  base[t] = counts[((long long)blockIdx.y * 256 + t) * nblk + blockIdx.x];
  for (int q = 0; q < RK_WAVES; ++q) wcnt[q][t] = 0u;
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  long long i0 = (long long)blockIdx.x * RK_TILE;
  for (int c = 0; c < RK_CHUNKS; ++c) {
    long long i = i0 + c * RK_THREADS + t;
    if (i0 + c * RK_THREADS >= S) break;  // (uniform over the workgroup)
    bool live = i < S;
    unsigned src = 0u, d = 0u;
    if (live) {
      src = ic ? ic[i] : (unsigned)i;
      d = (unsigned)(kc[src] >> shift) & 255u;
    }
    // the live lanes of this wave with this lane's digit
    unsigned long long same = __builtin_amdgcn_ballot_w64(live);
    for (int b = 0; b < 8; ++b) {
      unsigned long long m = __builtin_amdgcn_ballot_w64((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? m : ~m;
    }
    unsigned before = (unsigned)__popcll(same & below);
    if (live && before == 0u) wcnt[w][d] = (unsigned)__popcll(same);  // one writer per (wave, digit)
    __syncthreads();
    if (live) {
      unsigned pos = base[d] + before;
      for (int q = 0; q < w; ++q) pos += wcnt[q][d];
      oc[pos] = src;
    }
    __syncthreads();
    unsigned n = 0u;
    for (int q = 0; q < RK_WAVES; ++q) { n += wcnt[q][t]; wcnt[q][t] = 0u; }
    base[t] += n;
    __syncthreads();
  }
}

// tiles of a column of S keys, and the scratch a column needs: keys 8 S | two index buffers 4 S
// each | counts 256 nblk words
inline unsigned rk_tiles(long long S) { return (unsigned)((S + RK_TILE - 1) / RK_TILE); }
inline size_t rk_bytes_per_column(long long S) {
  return (size_t)S * 16 + (size_t)rk_tiles(S) * 256 * 4;
}

// columns per group under the scratch budget (NAIMA_AMD_RANK_SCRATCH_KIB, read at every call, sets
// another one), `extra` further bytes per column being the caller's own
inline int rk_group(long long S, int ncol, size_t extra) {
  size_t budget = RK_BUDGET;
  if (const char* e = getenv("NAIMA_AMD_RANK_SCRATCH_KIB")) budget = (size_t)std::max(1, atoi(e)) << 10;
  int G = (int)std::min<size_t>(std::max<size_t>(budget / (rk_bytes_per_column(S) + extra), 1), 65535);
  return std::min(G, ncol);
}

// where a group of G columns' buffers lie in scratch that starts at `base`
struct rk_buffers {
  unsigned long long* keys;
  unsigned *ia, *ib, *counts;
  rk_buffers(void* base, long long S, int G) {
    char* b = (char*)base;
    keys = (unsigned long long*)b;
    ia = (unsigned*)(b + (size_t)G * S * 8);
    ib = (unsigned*)(b + (size_t)G * S * 12);
    counts = (unsigned*)(b + (size_t)G * S * 16);
  }
};

// sort the g columns whose keys are in b.keys: *sorted (b.ia or b.ib) holds the row indices in
// ascending order of (key, row index)
inline int rk_sort(hipStream_t s, const rk_buffers& b, long long S, int g, const unsigned** sorted) {
  const unsigned nblk = rk_tiles(S);
  const unsigned* in = nullptr;
  unsigned* out = b.ia;
  for (int shift = 0; shift < 64; shift += 8) {
    hipLaunchKernelGGL(k_rank_hist, dim3(nblk, g), dim3(RK_THREADS), 0, s, b.keys, in, S, shift, nblk,
                       b.counts);
    NH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rank_scan, dim3(g), dim3(256), 0, s, b.counts, nblk);
    NH_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rank_scatter, dim3(nblk, g), dim3(RK_THREADS), 0, s, b.keys, in, out, S, shift,
                       nblk, b.counts);
    NH_CHECK_HIP(hipGetLastError());
    in = out;
    out = out == b.ia ? b.ib : b.ia;
  }
  *sorted = in;
  return NH_OK;
}

}  // namespace
