// plan_shape_host.cpp -- the half-step planner (naima_amd/csrc/nh_hs_plan.h) as a stand-alone host
// program: no GPU, no HIP runtime call.  tests/test_plan_shape_host.py builds it (host-only, under
// the address and undefined-behaviour sanitizers) and feeds it the sizes recorded in
// tests/golden/plan_shapes.json, or synthetic ones.
//
// stdin, whitespace-separated:  ncu run_rt want_resident nplans, then per plan
//   ns ndim lo nloc kind do_accept write_weights send_width has_lp nE nterms
//   ngrids { nG unit_scale }  nmoms { grid }  ntab { grid nK ldo nonnegative r0 }
//   syn_grid [ nE n1 ldo ldo2 two_outputs bcol x_first x_last ]
//   ncomp { table at }  nblobs { kind m mom }
// The synchrotron grid is rebuilt log-uniform from its end points.  The resident loop is planned on
// top of the LAST plan.  stdout: one "plan ..." line per plan, one "run ..." line.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../naima_amd/csrc/nh_hs_plan.h"

static char g_err[512];
int nh_set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// pointers of a descriptor are never followed by the planner, only compared: they point into one
// arena so that every comparison and difference is defined
static double g_arena[1 << 22];
static size_t g_used = 8;
static double* arena(size_t n) {
  double* p = g_arena + g_used;
  g_used += n;
  if (g_used > sizeof(g_arena) / sizeof(double)) { fprintf(stderr, "arena exhausted\n"); exit(2); }
  return p;
}

static int rd_i() { long long v = 0; if (scanf("%lld", &v) != 1) { fprintf(stderr, "bad input\n"); exit(2); } return (int)v; }
static double rd_d() { double v = 0; if (scanf("%lf", &v) != 1) { fprintf(stderr, "bad input\n"); exit(2); } return v; }

static bool inside(int o, int n, size_t lds) { return o < 0 || (size_t)(o + n) * 8 <= lds; }

int main() {
  const int ncu = rd_i(), run_rt = rd_i(), want_resident = rd_i(), nplans = rd_i();
  hs_knobs k = hs_knobs_default();
  k.run_rt = run_rt;
  static nh_halfstep_plan P;  // (the last plan: what the resident loop builds on)
  std::vector<double> xg;
  bool last_ok = false;
  for (int ip = 0; ip < nplans; ++ip) {
    g_used = 8;
    static nh_hs_desc d;
    memset(&d, 0, sizeof(d));
    d.ns = rd_i(); d.ndim = rd_i(); d.lo = rd_i(); d.nloc = rd_i(); d.kind = rd_i();
    d.do_accept = rd_i(); d.write_weights = rd_i(); d.send_width = rd_i();
    const int has_lp = rd_i();
    d.nE = rd_i(); d.nterms = rd_i();
    d.coords = arena(1); d.logp = arena(1); d.blk = arena(1); d.cursor = (int*)arena(1);
    d.qT = arena((size_t)d.ndim * d.nloc); d.factors = arena(1); d.total = arena(1);
    d.accepted = (int*)arena(1); d.naccepted = (int*)arena(1);
    d.params = arena(1);
    d.conv = arena(1); d.flux = arena(1); d.err_lo = arena(1); d.err_hi = arena(1);
    d.ul = (int*)arena(1); d.cl = arena(1);
    d.lp = has_lp ? arena(1) : nullptr;
    d.npacks = 1;  // (the packs decide no shape: one pack of constants that writes the particle rows)
    d.packs[0].ncols = 7; d.packs[0].ld = 8; d.packs[0].out = const_cast<double*>(d.params);
    d.ngrids = rd_i();
    for (int g = 0; g < d.ngrids && g < NH_MAX_GRIDS; ++g) {
      nh_grid& gr = d.grids[g];
      gr.nG = rd_i(); gr.unit_scale = rd_d();
      gr.e_eV = arena(1); gr.xg = arena(1); gr.ln_e = arena(1); gr.lx = arena(1);
      gr.w = arena(1); gr.dlw = arena(1);
    }
    d.nmoms = rd_i();
    for (int m = 0; m < d.nmoms && m < NH_MAX_MOMENT; ++m) {
      d.moms[m].grid = rd_i();
      d.moms[m].Kt = arena(1); d.moms[m].dlnKt = arena(1); d.moms[m].out = arena(1);
    }
    hs_facts f;
    f.ncu = ncu;
    f.syn_xg = nullptr;
    d.ntab = rd_i();
    for (int t = 0; t < d.ntab && t < NH_HS_MAX_TAB; ++t) {
      nh_hs_table& tb = d.tab[t];
      tb.grid = rd_i(); tb.nK = rd_i(); tb.ldo = rd_i(); tb.nonnegative = rd_i();
      f.r0[t] = rd_i();
      tb.KD = arena(1); tb.out = arena((size_t)tb.ldo + 1);
    }
    d.syn.grid = rd_i();
    if (d.syn.grid >= 0) {
      nh_hs_syn& s = d.syn;
      s.nE = rd_i(); s.n1 = rd_i(); s.ldo = rd_i(); s.ldo2 = rd_i();
      const int two = rd_i();
      s.bcol = rd_i();
      const double x0 = rd_d(), x1 = rd_d();
      s.ldB = 1; s.B = arena(1); s.E_eV = arena(1);
      s.out = arena((size_t)d.nloc * s.ldo + (size_t)d.nloc * s.ldo2 + 1);
      s.out2 = two ? s.out + (long long)d.nloc * s.ldo : nullptr;
      const int nG = d.grids[s.grid].nG;
      xg.assign((size_t)nG, 0.0);
      for (int i = 0; i < nG; ++i)  // (np.logspace: ln gamma_i = ln gamma_0 + i lx)
        xg[i] = i == 0 ? x0 : (i == nG - 1 ? x1 : (double)expl(logl((long double)x0) + i * (logl((long double)x1) - logl((long double)x0)) / (nG - 1)));
      f.syn_xg = xg.data();
    }
    d.ncomp = rd_i();
    for (int q = 0; q < d.ncomp && q < NH_MAX_COMP; ++q) {
      const int tab = rd_i(), at = rd_i();
      nh_comp& cp = d.comps[q];
      cp.scale = 1.0;
      if (tab >= 0) { cp.ptr = d.tab[tab].out + at; cp.ld = d.tab[tab].ldo; }
      else if (tab == -1) { cp.ptr = d.syn.out + at; cp.ld = d.syn.ldo; }
      else { cp.ptr = arena((size_t)d.nE); cp.ld = d.nE; }
    }
    d.nblobs = rd_i();
    for (int b = 0; b < d.nblobs && b < NH_HS_MAX_BLOB; ++b) {
      d.blobs[b].kind = rd_i(); d.blobs[b].m = rd_i(); d.blobs[b].mom = rd_i();
      d.blobs[b].cur = arena(1);
    }
    hs_shape S;
    const int rc = hs_plan(&d, k, f, P.hot, S);
    last_ok = rc == NH_OK;
    if (!last_ok) {
      printf("plan rc=%d error=%s\n", rc, g_err);
      continue;
    }
    const hs_hot& H = P.hot;
    P.lds_bytes = S.lds_bytes; P.lds_core = S.lds_core; P.threads = S.threads; P.blocks = d.nloc;
    P.split = S.split; P.rowsplit = S.rowsplit; P.rt = S.rt;
    {  // (what hs_create publishes of hs_first and the resident planner reads)
      P.hot.F.broken = ((d.kind == NH_PD_BROKENPL || d.kind == NH_PD_ECBPL) ? 1 : 0) |
                       ((d.kind == NH_PD_ECPL || d.kind == NH_PD_ECBPL) ? 2 : 0);
    }
    // every block of the layout inside the LDS the plan asks for
    bool in = true;
    const size_t core = S.lds_core, lds = S.lds_bytes;
    for (int g = 0; g < H.ngrids; ++g) {
      in = in && inside(H.o_w[g], H.nG[g], core) && inside(H.o_d[g], H.nG[g], core) && inside(H.o_lx[g], H.nG[g], core) &&
           inside(H.o_dp[g], H.nG[g], core) && inside(H.o_th[g], H.nG[g], core);
    }
    if (H.syn_grid >= 0) {
      const int nG = H.nG[H.syn_grid];
      in = in && inside(H.o_ig2, nG, core) && inside(H.o_dig2, nG, core) && inside(H.o_ig23, nG, core) &&
           inside(H.o_sq, 3 * H.syn_nE, core) && inside(H.o_amap, H.syn_nE + 1, core) &&
           inside(H.o_part_s, H.C.syn_cdmax * H.syn_nE, core);
      if (H.o_s2) in = in && H.o_s2 * 8 >= (long long)core && inside(H.o_s2, 1, lds);
    }
    in = in && inside(H.o_part_t, H.C.nT * 64, core) && inside(H.o_spec, H.C.nspec, core) &&
         inside(H.o_lik, 5 * H.nE, core) && inside(H.o_scale, H.C.nspec, core) && inside(H.o_synE, H.syn_nE, core) &&
         inside(H.o_pri, (int)(sizeof(nh_prior_pack) / 8) + 1, core) && inside(H.C.o_mrow, H.nE + NH_MAX_MOMENT, core) &&
         core <= lds;
    printf("plan rc=0 threads=%d blocks=%d split=%d lds_bytes=%zu syn_form=%d rowsplit=%d rt=%d segscale=%d "
           "lds_core=%zu nT=%d nT_cap=%d seg=%d syn_nodes=%d offsets_inside=%d\n",
           S.threads, d.nloc, S.split, S.lds_bytes, H.syn_grid < 0 ? 0 : (H.o_s2 ? 2 : 1), (int)S.rowsplit, (int)S.rt,
           S.segscale, S.lds_core, H.C.nT, S.split > 1 ? 160 : 96, H.C.seg, H.C.syn_nodes, (int)in);
  }
  if (!want_resident || !last_ok) return 0;
  static hs_run R;
  hs_run_shape RS;
  const int rc = hs_run_plan(&P, false, 0, 1, k, P.hot.syn_grid >= 0 ? xg.data() : nullptr, R, RS);
  if (rc != NH_OK) {
    printf("run rc=%d error=%s\n", rc, g_err);
    return 0;
  }
  const hs_hot& H = P.hot;
  const size_t lds = RS.lds_bytes;
  bool in = true;
  for (int g = 0; g < H.ngrids; ++g)
    in = in && inside(R.o_gx[g], H.nG[g], lds) && inside(R.o_lne[g], H.nG[g], lds) &&
         inside(R.o_ge[g], (H.F.broken & 1) ? H.nG[g] : 0, lds) && inside(R.o_il[g], H.nG[g], lds);
  in = in && inside(R.o_ut, 1, lds) && inside(R.o_sum, R.sum_cols, lds) && inside(R.o_cmp, 2 * NH_MAX_COMP + 2, lds) &&
       inside(R.o_pci, (NH_MAX_PRIOR + 1) / 2, lds) && inside(R.o_synce, H.syn_nE, lds) && inside(R.o_mt, 4 * NH_MAX_MOMENT, lds) &&
       inside(R.o_rs, 1, lds) && inside(R.o_it, 1, lds) && inside(R.o_pk, NH_MAX_PACK * NH_MAX_LAZY * HS_RUN_PKW, lds) &&
       inside(R.o_small1, HS_O_T64, lds) && inside(R.o_olds, 128, lds) && inside(R.o_lcl, H.nE + 1, lds) &&
       inside(R.o_trail, 1, lds);
  if (R.syn2) {  // (where the block did not fit, its offsets are left as tried and nobody reads them)
    const int nG = H.nG[H.syn_grid];
    in = in && inside(R.o_lnt, 256, lds) && inside(R.o_s2tab, (R.s2.P + 1) * HS_S2_STRIDE, lds) && inside(R.o_s2lw, nG, lds) && inside(R.o_s2ig, nG, lds) &&
         inside(R.o_s2lg, nG, lds) && inside(R.o_s2q, 4 * H.syn_nE, lds) && inside(R.o_s2z, (H.syn_nE + 1) / 2, lds) &&
         inside(R.o_s2t, HS_S2_TN, lds);
  }
  printf("run rc=0 threads=%d lds_bytes=%zu syn_log_domain=%d syn_nodes_per_piece=%d syn_pieces=%d "
         "tables_in_registers=%d workgroups_per_walker=%d rows_split=%d s2_own=%d tcompact=%d syn_nodes=%d "
         "offsets_inside=%d\n",
         P.threads, lds, R.syn2, R.syn2 ? 1 << R.s2.lm : 0, R.syn2 ? R.s2.P + 1 : 0, (int)RS.rt, P.split,
         R.rowsplit, R.syn2 ? R.s2_own : 0, R.tcompact, R.syn_nodes, (int)in);
  return 0;
}
