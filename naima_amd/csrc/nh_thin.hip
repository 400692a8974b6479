// nh_thin.hip -- every stride-th row of up to eight row-major matrices, copied into the next rows
// of as many compact ones (emcee's thin_by: the device loop writes every step's row into a staging
// block and keeps every t-th; naima_amd/device_sampler.py).
//
// One launch for all segments (chain, log-probability, every blob history of a chunk).  Pure
// copy: no LDS, nothing to reduce.  The work is cut into tiles of TH_THREADS x TH_UNROLL units of
// one destination row (a unit: 16 bytes where the segment's width is even and both bases are
// 16-byte aligned, else 8), the tiles of all segments numbered in one sequence; workgroups stride
// over that sequence.  Segment and row of a tile are found once per tile, uniformly for the
// workgroup (one 64-bit division per 16 KiB copied); a thread's TH_UNROLL loads are independent and
// issued before its stores, so that each wave keeps 4 KiB of reads in flight.  At most
// TH_MAX_WG workgroups (8 per CU of the 256): enough waves on every CU to cover HBM latency.
#include <algorithm>

#include "nh_common.h"

namespace {

constexpr int TH_THREADS = 256;
constexpr int TH_UNROLL = 4;
constexpr int TH_MAX_WG = 2048;
constexpr int TH_MAX_SEGS = 8;

struct th_seg {
  const char* src;     // first source row to copy
  char* dst;           // first destination row to write
  long long upr;       // units per row
  long long tpr;       // tiles per row
  long long tile0;     // first tile of this segment in the launch's sequence
  int vec;             // 1: 16-byte units, 0: 8-byte units
};

struct th_args {
  th_seg seg[TH_MAX_SEGS];
  int nsegs;
  long long ntiles;
  long long stride;    // source rows between two copied rows
};

template <typename T>
__device__ __forceinline__ void th_copy_tile(const T* __restrict__ s, T* __restrict__ d,
                                             long long col0, long long upr) {
  T v[TH_UNROLL];
#pragma unroll
  for (int j = 0; j < TH_UNROLL; ++j) {
    long long c = col0 + (long long)j * TH_THREADS + threadIdx.x;
    if (c < upr) v[j] = s[c];
  }
#pragma unroll
  for (int j = 0; j < TH_UNROLL; ++j) {
    long long c = col0 + (long long)j * TH_THREADS + threadIdx.x;
    if (c < upr) d[c] = v[j];
  }
}

__global__ void __launch_bounds__(TH_THREADS) k_hist_thin(const th_args a) {
  for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int g = 0;
    for (int i = 1; i < a.nsegs; ++i) g += (tile >= a.seg[i].tile0) ? 1 : 0;
    // (indexed by a loop-computed g: select instead of a dynamic index into the kernel arguments)
    th_seg sg = a.seg[0];
#pragma unroll
    for (int i = 1; i < TH_MAX_SEGS; ++i)
      if (i == g) sg = a.seg[i];
    long long t = tile - sg.tile0;
    long long row = t / sg.tpr;
    long long col0 = (t - row * sg.tpr) * (TH_THREADS * TH_UNROLL);
    long long ub = sg.vec ? 16 : 8;
    const char* s = sg.src + row * a.stride * sg.upr * ub;
    char* d = sg.dst + row * sg.upr * ub;
    if (sg.vec)
      th_copy_tile<double2>((const double2*)s, (double2*)d, col0, sg.upr);
    else
      th_copy_tile<double>((const double*)s, (double*)d, col0, sg.upr);
  }
}

}  // namespace

extern "C" int nh_hist_thin(nh_ctx* ctx, const nh_thin_seg* segs, int nsegs, long long first,
                            long long stride, long long nrows, long long dst_row0) {
  NH_REQUIRE(ctx && segs, "null argument");
  NH_REQUIRE(nsegs >= 1 && nsegs <= TH_MAX_SEGS, "nsegs outside [1, 8]");
  NH_REQUIRE(stride >= 1, "stride must be at least 1");
  NH_REQUIRE(first >= 0, "first must not be negative");
  NH_REQUIRE(nrows >= 0 && dst_row0 >= 0, "nrows and dst_row0 must not be negative");
  for (int i = 0; i < nsegs; ++i) {
    NH_REQUIRE(segs[i].src && segs[i].dst, "null segment");
    NH_REQUIRE(segs[i].width >= 1, "a segment's width must be positive");
    NH_REQUIRE(((uintptr_t)segs[i].src | (uintptr_t)segs[i].dst) % 8 == 0,
               "segments must be 8-byte aligned");
  }
  if (nrows == 0) return NH_OK;
  // rows are copied in parallel: no byte read by the launch may be one it writes
  for (int i = 0; i < nsegs; ++i) {
    uintptr_t w0 = (uintptr_t)segs[i].dst + (uintptr_t)(dst_row0 * segs[i].width) * 8;
    uintptr_t w1 = w0 + (uintptr_t)(nrows * segs[i].width) * 8;
    for (int j = 0; j < nsegs; ++j) {
      uintptr_t r0 = (uintptr_t)segs[j].src + (uintptr_t)(first * segs[j].width) * 8;
      uintptr_t r1 = r0 + (uintptr_t)(((nrows - 1) * stride + 1) * segs[j].width) * 8;
      NH_REQUIRE(w1 <= r0 || r1 <= w0, "source and destination rows overlap");
      if (j != i) {
        uintptr_t v0 = (uintptr_t)segs[j].dst + (uintptr_t)(dst_row0 * segs[j].width) * 8;
        uintptr_t v1 = v0 + (uintptr_t)(nrows * segs[j].width) * 8;
        NH_REQUIRE(w1 <= v0 || v1 <= w0, "two segments' destination rows overlap");
      }
    }
  }
  th_args a;
  memset(&a, 0, sizeof(a));
  a.nsegs = nsegs;
  a.stride = stride;
  long long tiles = 0;
  for (int i = 0; i < nsegs; ++i) {
    long long w = segs[i].width;
    th_seg& g = a.seg[i];
    g.src = (const char*)(segs[i].src + first * w);
    g.dst = (char*)(segs[i].dst + dst_row0 * w);
    // (width even: every row of a 16-byte aligned matrix is 16-byte aligned too)
    g.vec = (w % 2 == 0 && ((uintptr_t)segs[i].src | (uintptr_t)segs[i].dst) % 16 == 0) ? 1 : 0;
    g.upr = g.vec ? w / 2 : w;
    g.tpr = (g.upr + TH_THREADS * TH_UNROLL - 1) / (TH_THREADS * TH_UNROLL);
    g.tile0 = tiles;
    tiles += g.tpr * nrows;
  }
  a.ntiles = tiles;
  unsigned grid = (unsigned)std::min<long long>(tiles, TH_MAX_WG);
  hipLaunchKernelGGL(k_hist_thin, dim3(grid), dim3(TH_THREADS), 0, ctx->stream, a);
  NH_CHECK_HIP(hipGetLastError());
  return NH_OK;
}
