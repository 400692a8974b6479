// item_lanes_host.cpp -- how the resident loop's log-domain synchrotron items share their lanes
// among a slice's live energies (naima_amd/csrc/nh_syn2.h: hs_s2_spread, hs_s2_lane_of,
// hs_s2_chunk_nodes -- the functions the kernel calls) as a stand-alone host program: no GPU, no HIP
// runtime call.  tests/test_item_lanes_host.py builds it (host-only, under the address and
// undefined-behaviour sanitizers) and checks what it prints.
//
// stdin, whitespace-separated:  lm nG syn_nodes cdmax n, then n times  i0 Z  (a live energy's first
// live node and the comb index of the grid's node 0, in the compacted order).
// stdout: "plan nA=.. Cd=.. nS=.. cd=.. nx=.." as the items phase derives them, then per lane of the
// nS items "lane vt a ch cda kb n" (a = -1: idle; kb: the chunk's first node on the comb, n: its
// nodes, 0 where the chunk starts past the grid's end).
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "../naima_amd/csrc/nh_hs_plan.h"  // (nh_syn2.h behind what it needs)

int nh_set_error(int code, const char*, ...) { return code; }

static int rd_i() { int v = 0; if (scanf("%d", &v) != 1) { fprintf(stderr, "bad input\n"); exit(2); } return v; }

int main() {
  const int lm = rd_i(), nG = rd_i(), syn_nodes = rd_i(), cdmax = rd_i(), nA = rd_i();
  std::vector<int> i0((size_t)nA), Z((size_t)nA);
  int live = 0;
  for (int a = 0; a < nA; ++a) {
    i0[a] = rd_i();
    Z[a] = rd_i();
    live += nG - 1 - i0[a];
  }
  // (k_half_step_run behind barrier 2: one chunk count from the mean range, the items it fills)
  int Cd = 1, nS = 0;
  if (nA > 0) {
    Cd = (live / nA + syn_nodes - 1) / syn_nodes;
    Cd = Cd < 1 ? 1 : (Cd > cdmax ? cdmax : Cd);
    nS = (nA * Cd + 63) >> 6;
  }
  const hs_s2_lanes L = hs_s2_spread(nA, Cd, nS, cdmax);
  printf("plan nA=%d Cd=%d nS=%d cd=%d nx=%d\n", nA, Cd, nS, L.cd, L.nx);
  for (int vt = 0; vt < 64 * nS; ++vt) {
    int a = -1, ch = 0, cda = 0;
    if (!hs_s2_lane_of(L, nA, vt, a, ch, cda)) {
      printf("lane %d -1 0 0 0 0\n", vt);
      continue;
    }
    if (cda != hs_s2_chunks_of(L, a)) { fprintf(stderr, "the sum phase counts other chunks\n"); return 3; }
    const int k0 = ((Z[a] + i0[a]) >> lm) << lm, kend = Z[a] + nG - 1;
    const int per = hs_s2_chunk_nodes(k0, kend, cda, lm);
    const int kb = k0 + ch * per;
    const int n = kb <= kend ? (per < kend - kb + 1 ? per : kend - kb + 1) : 0;
    printf("lane %d %d %d %d %d %d\n", vt, a, ch, cda, kb, n);
  }
  return 0;
}
