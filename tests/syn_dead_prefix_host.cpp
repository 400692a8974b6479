// syn_dead_prefix_host.cpp -- where the resident loop's log-domain synchrotron items may start a
// live range (naima_amd/csrc/nh_syn2.h: hs_s2_prepare's constants, hs_s2_cut_node, hs_s2_cut_ok) as
// a stand-alone host program: no GPU, no HIP runtime call.  tests/test_syn_dead_prefix_host.py
// builds it (host-only, under the address and undefined-behaviour sanitizers) and holds what it
// prints against a NumPy transcription and against the oracle's synchrotron integral.
//
// stdin, whitespace-separated:  nG gam_first gam_last scale n, then n times
//   kind alpha beta alpha_2 ln_e0 ln_ecutoff ln_q
// (the grid is rebuilt log-uniform from its end points; ln_q: q = E / (Ec / gamma^2), x = q / gamma^2).
// stdout: one "cut ..." line with the constants, then per draw "r ic ok" (r with 17 digits).
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "../naima_amd/csrc/nh_hs_plan.h"  // (nh_syn2.h behind what it needs)

int nh_set_error(int code, const char*, ...) { return code; }

static double rd_d() { double v = 0; if (scanf("%lf", &v) != 1) { fprintf(stderr, "bad input\n"); exit(2); } return v; }
static int rd_i() { return (int)rd_d(); }

int main() {
  const int nG = rd_i();
  const double g0 = rd_d(), g1 = rd_d(), scale = rd_d();
  const int n = rd_i();
  std::vector<double> gam((size_t)nG);
  for (int i = 0; i < nG; ++i) gam[i] = exp(log(g0) + (log(g1) - log(g0)) * i / (nG - 1));
  hs_s2_host S;
  if (!hs_s2_prepare(gam.data(), nG, scale, 8, S)) { printf("refused\n"); return 0; }
  const hs_s2_cut& C = S.cut;
  printf("cut rcut=%.17g span=%.17g lx=%.17g lne0m=%.17g margin=%.17g lntcap=%.17g dref=%d on=%d invd=%.17g r746=%.17g m=%d\n",
         C.rcut, C.span, C.lx, C.lne0m, C.margin, C.lntcap, C.dref, C.on, S.invd, S.r746, 1 << S.par.lm);
  for (int k = 0; k < n; ++k) {
    const int kind = rd_i();
    const double al = rd_d(), be = rd_d(), a2 = rd_d(), lg0 = rd_d(), lg1 = rd_d(), lnq = rd_d();
    const double r = fma(lnq, S.invd, S.r746);  // (as the kernel forms it)
    const int ic = hs_s2_cut_node(C, r, nG);
    printf("%.17g %d %d\n", r, ic, hs_s2_cut_ok(C, kind, r, ic, nG, al, be, a2, lg0, lg1) ? 1 : 0);
  }
  return 0;
}
