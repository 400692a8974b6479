// nh_philox.h -- the counter-based random stream of the posterior analyses (nh_predictive.hip,
// nh_evidence.hip): Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011), ten rounds of two
// 32 x 32 -> 64 bit products, the key bumped by the Weyl constants between rounds.  A value is a
// function of (counter, key) alone.  The streams are kept apart by counter word 3: 0 is the
// replicates of nh_ppc_rows, NH_PHILOX_MVN the proposal draws of nh_mvn_draw.
#pragma once
#include "nh_common.h"

namespace {

constexpr unsigned NH_PHILOX_MVN = 0x4D564E31u;  // "MVN1"

struct nh_u4 {
  unsigned x, y, z, w;
};

__host__ __device__ __forceinline__ nh_u4 nh_philox(unsigned c0, unsigned c1, unsigned c2,
                                                    unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return nh_u4{c0, c1, c2, c3};
}

// a uniform in (0, 1) from 52 bits of two words: ((hi << 20 | lo >> 12) + 0.5) 2^-52
__host__ __device__ __forceinline__ double nh_u52(unsigned hi, unsigned lo) {
  return ((double)(((unsigned long long)hi << 20) | (unsigned long long)(lo >> 12)) + 0.5) *
         0x1p-52;
}

}  // namespace
