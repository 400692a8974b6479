// nh_hs_plan.h -- every decision and the LDS layout of the two half-step loops, as plain functions:
// no HIP runtime call and no environment read in here.  What a decision needs from the device
// comes in by value (hs_facts: the CU count, a host copy of the synchrotron grid, per table the
// first row that holds a non-zero); every environment override comes in one struct (hs_knobs),
// filled by whoever creates a plan.  A host-only program can therefore ask what the planner does
// for a given model without a GPU (tests/test_plan_shape_host.py).
//
//   hs_plan       nh_half_step_create's plan: validation, workgroup size, workgroups per walker,
//                 work items, LDS layout, the retry with fewer / coarser items when LDS overflows
//   hs_run_plan   the resident loop on top of that plan: what stays in LDS, where
//   hs_run_grid   the resident launch's grid from the occupancy the runtime reports
#pragma once
#include "nh_hs.h"
#include "nh_syn2.h"

// ---- the resident loop's by-value descriptor (k_half_step_run reads it, hs_run_plan fills it) ----
#define HS_RUN_MAX_STEPS 32  // steps per launch (one block of moves); ring rows = this + 1
#define HS_RUN_ERR_TIMEOUT 1
#define HS_RUN_ERR_PEER 2
#define HS_RUN_ERR_LAST_ROW 3  // (epilogue of a shared ensemble: a rank's last records never came)
#define HS_RUN_MAX_RANKS 8     // GPUs of one node that may share an ensemble
#define HS_RUN_HEAD 512        // granules ahead of the rings in a shared allocation (probe slots)
#define HS_O_HX 56           // two ints of the small block: HX_PRE, HX_SPECRD (two walkers in flight)
enum { HX_PRE = 0, HX_SPECRD = 1 };
#define HS_O_LNA 48          // in the small per-walker block (proposal coordinates: <= 15 of its first 64 doubles)
#define HS_O_S2CUT 32        // seven doubles of the FIRST small block: hs_s2_cut (nh_syn2.h), written when the launch begins
#define HS_RUN_TRAIL 16        // ints of first-row entries per table in LDS (>= tiles of any table)
#define HS_RUN_PKW 8           // doubles per parameter-pack column in LDS

// the weights' unit table (hs_run.o_ut): ints per unit
enum { HSU_FL = 0, HSU_NL, HSU_G, HSU_W, HSU_D, HSU_DP, HSU_IL, HSU_TH, HSU_LX, HSU_LNE, HSU_GX, HSU_GE,
       HSU_S2LW, HSU_S2LG, HSU_SC_LO, HSU_SC_HI, HSU_N };
// HSU_FL: bits 0-1 = 0 plain | 1 the log-domain synchrotron items read ln w of this grid too | 2 and
// nothing else of it; bit 2: the non-negative table items' pre-divided log-ratios are kept; bit 3:
// ... with 1 / lx and the thresholds in LDS since the launch began; bit 4: the unit is its grid's last
static_assert(HSU_N == 16, "a unit's descriptor is four 16-byte reads");

// the table items' descriptors (hs_run.o_it): HS_MAX_TAB x 16 ints per TABLE (HST_*), then 4 ints
// per ITEM { table | tile << 4, first row, end row, the same two ignoring the leading zero rows (16
// bits each) }
enum { HST_KD_LO = 0, HST_KD_HI, HST_NK, HST_NG, HST_AW, HST_AD, HST_AL, HST_FLAGS, HST_SUB, HST_NKP,
       HST_N = 16 };
#define HSI_N 4

struct hs_run {
  unsigned long long* ring;  // [HS_RUN_MAX_STEPS + 1][N][gr] granules
  int* status;               // device word: 0, or HS_RUN_ERR_* of the first workgroup that gave up
  int* accw;                 // [HS_RUN_MAX_STEPS][N]: 1 where the step's proposal was accepted
  double* hcoords; double* hlogp;  // chain history of this call (or NULL) ...
  double* hblob[NH_HS_MAX_BLOB];   // ... and the blobs' (or NULL)
  long long hrow0, hcap;     // history row of the launch's first step; rows the history holds
  long long* dbg;            // NH_HS_DEBUG: [256][64][8] wall-clock stamps, or NULL
  // gridDim.y = K > 1 workgroups share a walker (a half-step of fewer walkers than CUs, as in
  // k_half_step): what workgroups 1 .. K - 1 hand over per (slice, walker) at xspec, tagged granules
  // -- per slice, because nothing stops one of a walker's workgroups from running slices ahead of
  // another.  (tick: unused, always NULL; it keeps its place because the kernels' argument offsets
  // follow this layout)
  double* xspec; int* tick;
  int slice0, nslices;       // slices [slice0, slice0 + nslices) of the block of moves; slice0 even
  unsigned seq;              // launch sequence number (tags)
  int gr, N;                 // granules per record (a multiple of 16: one record = whole lines)
  int o_gx[NH_MAX_GRIDS], o_lne[NH_MAX_GRIDS], o_ge[NH_MAX_GRIDS];  // LDS: grid nodes, ln E, E
  int o_pk, o_small1, o_olds;  // LDS: pack descriptors, the second small block, old coordinates
  int o_lcl;                   // LDS: ln(1 - cl[n]), n <= nE
  int o_trail;                 // LDS: the tables' trailers (ints)
  // the loop's own copies of the plan's tables with their columns sorted (nh_hs.h; NULL: the
  // plan's table as it is)
  const double* kds[HS_MAX_TAB];
  int spin_limit;
  // synchrotron nodes per thread and work item.  The plan's 10 suit a launch per half-step and
  // workgroups that share a walker; one resident workgroup per walker runs fastest on items
  // three times that long (cfg3, us per 40 half-steps: 1 015 at 10, 981 at 16, 975 at 24, 959
  // at 30 and at 40; two workgroups per walker -- cfg2 -- 901 at 5, 885 at 10, 914 at 16)
  int syn_nodes;
  int rebalance;  // a tile's chunks divide the rows above its first non-zero one (table-only models)
  // what the host learns about a launch without a round trip of its own: k_run_epilogue stores
  // { status, NaN proposals, forbidden proposals, launch number } (the number last) into one of
  // two slots of page-locked host memory (nh_half_step_run_report)
  int* report;
  int report_launch;
  // NaN / forbidden proposals THIS launch has met (two device ints, a pair per launch parity):
  // k_run_epilogue adds them to the plan's counters only when the launch ended well, so that a
  // launch that gave up part of the way leaves the counters as it found them whoever of its
  // workgroups had already counted (what a replay of its block of moves starts from)
  int* lcnt;
  int o_il[NH_MAX_GRIDS];  // LDS: 1 / lx per node of a grid a non-negative table is reduced over (-1: none)
  // LDS: the weights' units -- 64 consecutive nodes of one grid each -- as 16 ints per unit
  // (HSU_*: grid, first node, node count, where the node's inputs and outputs sit in LDS, the
  // grid's scale), built once per launch; -1: the grids' nodes are not in LDS (small workgroups)
  int o_ut;
  // LDS: the table work items -- which table, column tile and rows, where the walker's arrays
  // sit -- as 16 ints per item (HSI_*), built once per launch: a work item read its table's
  // descriptor out of the kernel-argument segment field by field (dependent vector loads: the
  // table index is not a constant) and re-derived its rows -- ~300 vector instructions before its
  // first segment, as many as the segments of a 32-row item cost; -1: not used
  int o_it;
  // LDS: per column of the tables' (sorted) spectra 4 ints { first partial sum | stride | chunks |
  // where it goes in spec } + its scale's index rides with `where`; and the model's components as
  // NH_MAX_COMP x { offset in spec (int, as a double's low word) | scale }: the phases behind
  // barrier 3 -- one or a few waves, everybody else waiting -- took these out of the
  // kernel-argument segment one dependent scalar load at a time (four round trips per component)
  int o_sum, o_cmp;
  int o_pci;  // LDS: per prior term the proposed coordinate it reads, or -1 (ints)
  int o_mt;     // LDS: per single-row reduction { w, dlw, lx, K | dlnK (LDS byte addresses), nG, first row, last row } (ints)
  int o_lnt;    // LDS: 128 x { 1 / c_j, ln c_j }, c_j the centres of [1/2, 1)'s 128 bins (hsr_ln_tab; log-domain instances)
  int o_synce;  // LDS: CS1 / B per photon energy (walker-independent: a division per live energy and slice otherwise)
  // K workgroups of a table-only walker split the grid's ROWS (hs_plan's rowsplit): workgroup
  // `part` owns the nodes [b_part, b_part+1] -- the boundaries sit between
  // two of the table's chunks -- forms the weights there, reduces its chunks and its part of the
  // single-row reductions, and hands its partial sums to workgroup 0 of the walker
  int rowsplit;
  int tcompact;  // K > 1: a table item's partial sums in the slot of its group (hs_run_plan)
  int o_rs;   // LDS: this workgroup's nodes per grid and its units (rowsplit)
  int nxmax;  // doubles a workgroup hands over at most (spectrum + single-row reductions)
  int sum_cols;  // columns of all the tables together (the sum phase's loop bound)
  // ---- an ensemble shared by several GPUs (nrank > 1; see "The ensemble across GPUs" in
  // nh_persist.hip): `ring` is this launch's ring in THIS rank's memory, peer[p] the same ring in
  // rank p's (peer[rank] == ring); a mover stores its walker's record into every one of them
  int nrank, rank;
  unsigned long long* peer[HS_RUN_MAX_RANKS];
  int* nacc_own;   // acceptance counters of the moves THIS rank made (the plan's are replicated)
  int* hacc;       // with a history: [hcap][N] -1 | 0 | 1 = not moved by this rank | rejected | accepted
  int* curstamp;   // with blobs: [N] stamp of the last move this rank accepted for the walker
  int stamp0;         // stamp of the launch's first step (counts the steps of all launches)
  // NH_RUN_PUBLISH_DELAY (100 MHz ticks; experiments): a mover waits this long before it stores a
  // record -- every hand-off of the shared loop then pays what a slower link would add
  int publish_delay;
  // ---- the synchrotron items in the log domain, on the grid's comb (nh_syn2.h; syn2 != 0) ----
  int syn2, s2_own;  // s2_own: nobody else reads the synchrotron grid's w / dlw (its LDS is reused)
  int o_s2tab, o_s2lw, o_s2ig, o_s2lg, o_s2q, o_s2z, o_s2t;  // LDS: table | Lambda ln w (guards either side) |
                                                      // 1/gamma^2 (guards) | Lambda (ln gamma / 3 +
                                                      // ln scale) | per live energy 4 doubles | comb index | 2^(j/128)
  const double* s2_dev;  // device: the table's (P + 1) x 6 doubles, then the grid's nG values of the above
  hs_syn2_par s2;
  double s2_z0, s2_invd;  // z = s2_z0 - ln(q) s2_invd: where node 0 sits on the comb below T_top
  double s2_r746;         // (T_top - ln 746) s2_invd - s2_z0: the first live node is ceil(ln(q) s2_invd + this)
  double s2_lnw0;         // ln |n| + ln(E / eV) above this: the weight gamma n scale is not 0 in double
  hs_s2_cut s2_cut;       // a live range whose head is nothing of the integral starts at x <= 128 (nh_syn2.h: hs_s2_cut_ok)
  int pipeline;           // two walkers in flight (a workgroup with several walkers of a slice): NH_RUN_PIPELINE
  long long* clk;         // the context's span clock (nh_common.h): this launch opens a span, k_run_epilogue closes it
};

static_assert(sizeof(hs_hot) + sizeof(hs_run) <= 4000, "both argument blocks fit the kernarg segment");

// ---- the knobs: every environment override of the two creates (tuning experiments, test hooks) --
struct hs_opt {  // an override that may be absent
  bool set;
  int v;
  int or_else(int dflt) const { return set ? v : dflt; }
};
struct hs_knobs {
  // nh_half_step_create (NH_HS_*)
  bool test_reject;             // NH_HS_TEST_REJECT set: the plan is turned down (test hook)
  int kmax;                     // NH_HS_SPLIT: workgroups per walker at most (8)
  int part_kb;                  // NH_HS_PART_KB: LDS for the synchrotron items' partial sums (40)
  hs_opt threads;               // NH_HS_THREADS
  int split_min_work;           // NH_HS_SPLIT_MIN_WORK (1 << 20)
  int rowsplit, rt, syn2;       // NH_HS_ROWSPLIT, NH_HS_RT, NH_HS_SYN2 (1: allowed)
  bool rt_debug;                // NH_HS_RT_DEBUG set: the decisions on stderr
  hs_opt seg, syn_nodes;        // NH_HS_SEG (ignored below 4), NH_HS_SYN_NODES (ignored below 1)
  bool debug;                   // NH_HS_DEBUG != 0: the kernels' wall-clock stamps
  // the resident loop (NH_RUN_*)
  int run_rt, run_grids_in_lds, run_ut, run_rowsplit, run_syn2, run_il;  // (1: allowed)
  hs_opt run_rebalance;         // NH_RUN_REBALANCE (table-only models: 1)
  int run_tcompact_min;         // NH_RUN_TCOMPACT_MIN (4)
  hs_opt run_syn_nodes;         // NH_RUN_SYN_NODES
  int run_pipeline;             // NH_RUN_PIPELINE (1)
  int run_syn_cut;              // NH_RUN_SYN_CUT (1): the log-domain items leave a range's faint head out
  int run_fail_at;              // NH_RUN_FAIL_AT: the launch whose first wait times out (tests; 0)
  hs_opt run_grid;              // NH_RUN_GRID (ignored below 1)
  hs_opt run_max_per_wg;        // NH_RUN_MAX_PER_WG
  int run_shared_alloc;         // NH_RUN_SHARED_ALLOC (1)
  hs_opt run_spin_limit;        // NH_RUN_SPIN_LIMIT (ignored below 1)
  int run_publish_delay;        // NH_RUN_PUBLISH_DELAY (0)
};
// what the library does when nothing is set
static inline hs_knobs hs_knobs_default() {
  hs_knobs k;
  memset(&k, 0, sizeof(k));
  k.kmax = 8; k.part_kb = 40; k.split_min_work = 1 << 20;
  k.rowsplit = k.rt = k.syn2 = 1;
  k.run_rt = k.run_grids_in_lds = k.run_ut = k.run_rowsplit = k.run_syn2 = k.run_il = 1;
  k.run_tcompact_min = 4; k.run_pipeline = 1; k.run_shared_alloc = 1; k.run_syn_cut = 1;
  return k;
}

// ---- what the planner has to be told about the device -------------------------------------------
struct hs_facts {
  int ncu;               // the device's CUs, NAIMA_AMD_CU_SHARE applied
  const double* syn_xg;  // host copy of the synchrotron grid's nodes; NULL: could not be read
  int r0[HS_MAX_TAB];    // per table the first row that holds a non-zero; -1: not read (too large
                         // for a lane's registers anyway, or the read failed: "does not fit")
};
// can hs_plan ask for r0 at all?  (the one-time read of every table is made only then)
static inline bool hs_plan_reads_rows(const nh_hs_desc* d, const hs_knobs& k, int ncu) {
  return d->syn.grid < 0 && d->ntab > 0 && d->ntab <= NH_HS_MAX_TAB && d->nloc <= ncu && k.rt != 0;
}

// (errors carry the name of the create that asked: `who` of the function at hand)
#define HSP_REQUIRE(cond, msg)                                               \
  do {                                                                       \
    if (!(cond)) return nh_set_error(NH_EINVAL, "%s: %s", who, msg);         \
  } while (0)
#define HS_S2_HDR 16  // doubles ahead of the log-domain block in LDS (k_half_step<true, true>)

// ---- nh_half_step_create's plan -----------------------------------------------------------------
struct hs_shape {
  int threads, split, segscale;
  bool rowsplit, rt;
  size_t lds_core, lds_bytes;  // lds_core: without k_half_step's own log-domain block (the last thing in it)
  hs_s2_host s2;               // the log-domain table (valid where H.o_s2 != 0)
  nh_pack packs[NH_MAX_PACK];  // the parameter packs, for their device copy
};
// what does not depend on (kmax, segscale)
struct hs_plan_front {
  int off, nspec, syn_nE, threads;
  long long work;
  bool s2_ok;
};

static inline int hs_plan_checked(const nh_hs_desc* d, const hs_knobs& k, const hs_facts& f, hs_hot& H,
                                  hs_shape& S, hs_plan_front& A) {
  static const char* who = "hs_create";
  HSP_REQUIRE(d->coords && d->logp && d->blk && d->cursor && d->qT && d->factors && d->params &&
                  d->total, "NULL pointer in the descriptor");
  HSP_REQUIRE(d->ns >= 1 && d->ndim >= 1 && d->ndim <= 64 && d->lo >= 0 && d->nloc >= 1 &&
                  d->lo + d->nloc <= d->ns, "bad proposal block");
  HSP_REQUIRE(!d->do_accept || (d->lo == 0 && d->nloc == d->ns && d->accepted),
              "the in-kernel accept needs every walker of the slice in this launch");
  HSP_REQUIRE(d->npacks >= 1 && d->npacks <= NH_MAX_PACK, "bad pack plan");
  HSP_REQUIRE(d->kind >= NH_PD_POWERLAW && d->kind <= NH_PD_LOGPARABOLA, "unknown particle distribution kind");
  HSP_REQUIRE(d->ngrids >= 1 && d->ngrids <= NH_MAX_GRIDS, "bad grid count");
  HSP_REQUIRE(d->nmoms >= 0 && d->nmoms <= NH_MAX_MOMENT, "bad reductions");
  HSP_REQUIRE(d->ntab >= 0 && d->ntab <= NH_HS_MAX_TAB && (d->ntab > 0 || d->syn.grid >= 0),
              "a half-step needs at least one emission component");
  HSP_REQUIRE(d->ncomp >= 1 && d->ncomp <= NH_MAX_COMP && d->nE >= 1, "bad likelihood components");
  HSP_REQUIRE(d->conv && d->flux && d->err_lo && d->err_hi && d->ul && d->cl, "NULL data column");
  HSP_REQUIRE(d->nterms >= 0 && d->nterms <= NH_MAX_PRIOR, "bad prior terms");
  static_assert(NH_HS_MAX_TAB == HS_MAX_TAB, "table count");
  static_assert(sizeof(hs_hot) <= 3800, "the by-value kernel argument must fit the 4 KB segment");
  memset(&H, 0, sizeof(H));
  hs_dev& C = H.C;
  memset(S.packs, 0, sizeof(S.packs));
  H.coords = d->coords; H.logp = d->logp; H.blk = d->blk; H.cursor = d->cursor;
  H.qT = d->qT; H.factors = d->factors; H.hist = d->hist;
  H.ns = d->ns; H.ndim = d->ndim; H.lo = d->lo; H.nloc = d->nloc;
  C.npk = d->npacks; C.kind = d->kind; C.params = d->params;
  bool have_params = false;
  for (int q = 0; q < d->npacks; ++q) {
    const nh_pack& pk = d->packs[q];
    HSP_REQUIRE(pk.out && pk.ncols >= 1 && pk.ncols <= NH_MAX_LAZY && pk.ld >= pk.ncols,
                "bad pack request");
    for (int c = 0; c < pk.ncols; ++c) {
      const double* b = pk.cols[c].base;
      HSP_REQUIRE(b == nullptr || (b >= d->qT && b < d->qT + (long long)d->ndim * d->nloc &&
                                   (b - d->qT) % d->nloc == 0 && pk.cols[c].stride == 1),
                  "a pack column must read one proposal coordinate (or be a constant)");
    }
    if (pk.out == d->params) {
      HSP_REQUIRE(pk.ncols >= 7, "the particle rows need 7 columns");
      have_params = true;
    }
    S.packs[q] = pk;
  }
  HSP_REQUIRE(have_params, "params must be the output of one of the packs");
  HSP_REQUIRE(d->ndim < 255, "at most 254 fit parameters");
  for (int t = 0; t < d->ntab; ++t) {  // (checked before anything indexes grids[] with it)
    const nh_hs_table& tb = d->tab[t];
    HSP_REQUIRE(tb.grid >= 0 && tb.grid < d->ngrids && tb.KD && tb.out && tb.nK >= 1 &&
                    tb.ldo >= tb.nK, "bad table reduction");
  }
  if (k.test_reject)  // (test hook: a plan this function turns down)
    return nh_set_error(NH_EINVAL, "half-step plan rejected (NH_HS_TEST_REJECT)");
  H.ngrids = d->ngrids;
  int off = HS_O_FREE;
  for (int g = 0; g < d->ngrids; ++g) {
    const nh_grid& gr = d->grids[g];
    HSP_REQUIRE(gr.e_eV && gr.xg && gr.nG >= 2 && (!d->write_weights || (gr.w && gr.dlw)),
                "bad grid descriptor");
    HSP_REQUIRE(gr.ln_e && gr.lx, "the half-step kernel needs the grids' ln_e and lx arrays");
    H.e[g] = gr.e_eV; H.xg[g] = gr.xg; H.lne[g] = gr.ln_e; H.lx[g] = gr.lx;
    H.scale[g] = gr.unit_scale; H.nG[g] = gr.nG;
    C.w[g] = gr.w; C.dlw[g] = gr.dlw;
    H.o_w[g] = off; off += gr.nG;
    H.o_d[g] = off; off += gr.nG;
    H.o_lx[g] = off; off += gr.nG;
    H.o_dp[g] = H.o_th[g] = -1;
    for (int t = 0; t < d->ntab; ++t)
      if (d->tab[t].grid == g && d->tab[t].nonnegative) {
        H.o_dp[g] = off; off += gr.nG;
        H.o_th[g] = off; off += gr.nG;
        break;
      }
  }
  H.o_mkt = off;
  H.nmom = d->nmoms;
  for (int m = 0; m < d->nmoms; ++m) {
    HSP_REQUIRE(d->moms[m].grid >= 0 && d->moms[m].grid < d->ngrids && d->moms[m].Kt &&
                    d->moms[m].dlnKt && d->moms[m].out, "bad reduction");
    H.mKt[m] = d->moms[m].Kt; H.mdK[m] = d->moms[m].dlnKt; H.mgrid[m] = d->moms[m].grid;
    C.mom_out[m] = d->moms[m].out;
    off += 2 * d->grids[d->moms[m].grid].nG;
  }
  C.accepted = d->accepted; C.naccepted = d->naccepted; C.sel = d->sel;
  C.do_accept = d->do_accept; C.write_weights = d->write_weights;
  // ---- synchrotron ----
  H.syn_grid = -1;
  int nspec = 0;
  int syn_nE = 0;
  if (d->syn.grid >= 0) {
    const nh_hs_syn& s = d->syn;
    HSP_REQUIRE(s.grid < d->ngrids && s.E_eV && s.out && s.nE >= 1 && s.ldo >= (s.out2 ? s.n1 : s.nE) &&
                    (s.bcol >= 0 ? s.bcol < NH_PD_NPAR : (s.B != nullptr && s.ldB >= 1)),
                "bad synchrotron component");
    const int nG = d->grids[s.grid].nG;
    HSP_REQUIRE(s.nE <= 512, "at most 512 photon energies for the synchrotron component");
    H.syn_grid = s.grid; H.syn_E = s.E_eV; H.syn_nE = syn_nE = s.nE;
    C.synB = s.B; C.syn_out = s.out; C.syn_ldo = s.ldo; C.syn_bcol = s.bcol; C.syn_ldB = s.ldB;
    HSP_REQUIRE(s.out2 == nullptr || (s.n1 >= 1 && s.n1 < s.nE && s.ldo >= s.n1 && s.ldo2 >= s.nE - s.n1),
                "bad split of the synchrotron component's output");
    HSP_REQUIRE(s.out2 == nullptr || (s.out2 == s.out + (long long)d->nloc * s.ldo && s.ldo2 == s.nE - s.n1 &&
                                      s.ldo < (1 << 20) && s.n1 < (1 << 11)),
                "the synchrotron component's second array must follow its first (out + nloc * ldo), rows of nE - n1");
    if (s.out2) C.syn_ldo = s.ldo | (s.n1 << 20);
    H.o_ig2 = off; off += nG;
    H.o_dig2 = off; off += nG;
    H.o_ig23 = off; off += nG;
    H.o_sq = off; off += 3 * s.nE;
    H.o_amap = off; off += s.nE + 1;  // 2 nE ints
    int cdmax = (int)(((size_t)k.part_kb * 1024) / ((size_t)s.nE * 8));  // (partial sums: 40 KB of LDS at most)
    cdmax = cdmax > 32 ? 32 : (cdmax < 1 ? 1 : cdmax);
    C.syn_cdmax = cdmax;
    H.o_part_s = off; off += cdmax * s.nE;
    H.syn_spec_off = nspec;
    nspec += s.nE;
  }
  // workgroup size: small reductions are bound by the dependent round trips, not by lanes
  int maxnG = 0;
  for (int g = 0; g < d->ngrids; ++g) maxnG = d->grids[g].nG > maxnG ? d->grids[g].nG : maxnG;
  long long work = 0;
  for (int t = 0; t < d->ntab; ++t)
    work += (long long)((d->tab[t].nK + 63) / 64) * 64 * d->grids[d->tab[t].grid].nG * 12;
  if (d->syn.grid >= 0) work += (long long)d->syn.nE * d->grids[d->syn.grid].nG * 110 / 3;
  int threads = work >= (1 << 20) ? 1024 : (work >= (1 << 18) ? 512 : 256);
  if (threads < 1024 && maxnG > threads) threads = maxnG > 512 ? 1024 : 512;
  // A table-only model's launch is half prologue and tail (dependent round trips, single-wave
  // phases: 9 of cfg5's 16 us) with the CU's other waves idle.  When a launch holds more
  // walkers than the chip has CUs, smaller workgroups put several walkers on a CU at once and
  // one walker's prologue runs beside another's items: cfg5 at 1024 walkers per launch 66.8 us
  // (1024 threads, four rounds) -> 51.6 (512) -> 37.0 (256 threads, four workgroups per CU).
  // Launches of at most one walker per CU keep the large workgroup (256 walkers: 15.6 us at
  // 1024 threads, 16.7 at 512, 24.5 at 256).
  if (d->syn.grid < 0)
    while (threads > 256 && (long long)d->nloc * threads > 1024LL * f.ncu) threads >>= 1;
  if (k.threads.set) threads = k.threads.v;
  HSP_REQUIRE(threads >= 128 && threads <= 1024 && threads % 64 == 0, "bad workgroup size");
  if (d->syn.grid >= 0 && threads / 64 < (d->syn.nE + 63) / 64 + 2) threads = 1024;
  while (threads < 1024 && threads / 64 <= d->nmoms + 1) threads <<= 1;  // (a wave per single-row reduction)
  HSP_REQUIRE(threads / 64 > d->nmoms + 1, "more single-row reductions than waves");
  // ---- the synchrotron items in the log domain (nh_syn2.h), as the resident loop runs them: a
  // log-uniform grid (np.logspace, radiative.py:147-154), its table and node constants behind the
  // grid's three arrays in syn_c, their block in LDS behind o_s2 (k_half_step<true, true>)
  A.s2_ok = d->syn.grid >= 0 && k.syn2 != 0 && f.syn_xg != nullptr &&
            hs_s2_prepare(f.syn_xg, d->grids[d->syn.grid].nG, d->grids[d->syn.grid].unit_scale,
                          2 * HS_S2_GUARD, S.s2);
  A.off = off; A.nspec = nspec; A.syn_nE = syn_nE; A.threads = threads; A.work = work;
  return NH_OK;
}

// one shape: at most kmax workgroups per walker, table items of segscale times the usual length.
// *lds_overflow: the shape was turned down because its partial sums do not fit LDS (a smaller
// kmax or a larger segscale may)
static inline int hs_plan_shape(const nh_hs_desc* d, const hs_knobs& k, const hs_facts& f,
                                const hs_plan_front& A, int kmax, int segscale, hs_hot& H, hs_shape& S,
                                bool* lds_overflow) {
  static const char* who = "hs_create";
  hs_dev& C = H.C;
  const int ncu = f.ncu;
  const long long work = A.work;
  int off = A.off, nspec = A.nspec, threads = A.threads;
  // ---- a launch of fewer walkers than the chip has CUs: K workgroups per walker ----
  // (each repeats the prologue -- on CUs that would otherwise idle -- and takes every K-th
  // work item; the items are cut finer so that every wave of every workgroup still gets some)
  int split = 1;
  {
    // (worth it where the work items are most of a launch: measured on cfg2 / cfg3 at 128
    // walkers per launch 42.3 -> 32.7 us and 33.8 -> 28.0 us; the hand-off costs ~3.5 us, which
    // the table-only models cfg1 / cfg5 -- 7 us of items in a 17 us launch -- do not get back)
    if (work >= k.split_min_work)
      while (split * 2 <= kmax && (long long)d->nloc * split * 2 <= ncu) split *= 2;
  }
  // ---- a table-only model with ONE table, at most half as many walkers per launch as
  // CUs (BASELINE's PionDecay fit at one GPU's share of its 2048 walkers): two workgroups per
  // walker that split the grid's ROWS -- each forms the weights of its half, reduces its half of
  // the table (from registers: half the rows fit a lane's) and of the single-row reductions, and
  // the second hands its partial spectrum to the first (the resident loop: hs_run.rowsplit; the
  // per-launch kernel runs the same plan with its items interleaved, as any split launch)
  bool rowsplit = false;
  if (split == 1 && d->syn.grid < 0 && d->ntab == 1 && kmax >= 2 &&
      (long long)d->nloc * 2 <= ncu && k.rowsplit != 0) {
    split = 2;
    rowsplit = true;
  }
  // ---- a table-only model whose items' rows fit a lane's registers: workgroups of 512 threads
  // (256 vector registers per lane), for the resident loop's register-resident items (nh_hs.h:
  // hs_rt_item; k_half_step_run<false, ., false, RT>).  The rows an item walks start at the first
  // one in which a column is non-zero (the resident loop's sorted copies: at least that far up).
  bool rt_plan = false;
  // (launches of at most one workgroup per CU: a workgroup of this instance has a CU to itself)
  if (d->syn.grid < 0 && d->ntab > 0 && threads >= 256 && (long long)d->nloc * split <= ncu &&
      k.rt != 0) {
    bool fits = true;
    int tiles = 0;
    for (int t = 0; t < d->ntab; ++t) {
      tiles += (d->tab[t].nK + 63) / 64;
    }
    const int t_rt = threads > 512 ? 512 : threads;
    const int free_waves = (t_rt / 64 - d->nmoms) * split;
    fits = fits && free_waves >= 1 && tiles <= free_waves;
    const int per_tile = fits ? free_waves / tiles : 1;
    for (int t = 0; t < d->ntab && fits; ++t) {
      const nh_hs_table& tb = d->tab[t];
      const int nG = d->grids[tb.grid].nG, nK = tb.nK;
      const int r0 = f.r0[t];
      if (r0 < 0) {  // (nothing of that size fits a lane's registers, or the table could not be read)
        fits = false;
        break;
      }
      const int sub = nK <= 32 ? (nK <= 16 ? (nK <= 8 ? (nK <= 4 ? (nK <= 2 ? (nK <= 1 ? 64 : 32) : 16) : 8) : 4) : 2) : 1;
      const int per = (nG - 1 - r0 + per_tile - 1) / per_tile;
      fits = (per + sub - 1) / sub + 1 <= HS_RT_NODES;
      if (k.rt_debug)
        fprintf(stderr, "RT: table %d nG %d nK %d r0 %d per_tile %d per %d sub %d nodes %d fits %d\n", t, nG, nK, r0,
                per_tile, per, sub, (per + sub - 1) / sub + 1, (int)fits);
    }
    if (k.rt_debug) fprintf(stderr, "RT: fits %d threads %d nmoms %d split %d\n", (int)fits, threads, d->nmoms, split);
    if (fits) {
      threads = t_rt;
      rt_plan = true;
    }
  }
  // ---- table reductions: work items of `seg` segments x 64 columns ----
  // With a synchrotron component the items interleave with its (issue-bound) items and 32
  // segments keep the waves evenly loaded; without one, ONE round of equal items over the
  // waves that are free from the start (not on a single-row reduction) ends soonest.
  C.ntab = d->ntab;
  // (48 segments per item where a walker has one workgroup: with the synchrotron items in the log
  // domain -- half the instructions they were -- the table items are the larger share of the
  // resident loop's work, and a third fewer of them means a third less set-up: cfg3 10.6 -> 11.0 M
  // walker-steps/s together with 48-node synchrotron items; 64: 10.9, 96: 10.7, 128: 10.3.  The
  // per-launch kernel loses 2 % to it.)
  int seg = split >= 4 ? 8 : (split == 2 ? 16 : (d->syn.grid >= 0 ? 48 : 32));
  if (split > 1) seg *= segscale;  // (coarser items: fewer partial sums in LDS)
  C.syn_nodes = HS_SYN_NODES / split > 3 ? HS_SYN_NODES / split : 3;
  if (k.seg.set) seg = k.seg.v >= 4 ? k.seg.v : seg;  // (tuning experiments)
  if (k.syn_nodes.set) C.syn_nodes = k.syn_nodes.v >= 1 ? k.syn_nodes.v : C.syn_nodes;
  if (d->syn.grid < 0 && d->ntab > 0) {
    int tiles = 0, maxseg = 0;
    for (int t = 0; t < d->ntab; ++t) {
      tiles += (d->tab[t].nK + 63) / 64;
      const int nseg = d->grids[d->tab[t].grid].nG - 1;
      maxseg = nseg > maxseg ? nseg : maxseg;
    }
    const int free_waves = (threads / 64 - d->nmoms) * split;
    int per_tile = free_waves / tiles > 1 ? free_waves / tiles : 1;
    seg = (maxseg + per_tile - 1) / per_tile;
    if (seg < 8) seg = 8;
  }
  auto chunking = [&](int nseg) { return (nseg + seg - 1) / seg; };
  for (;;) {
    int nT = 0;
    for (int t = 0; t < d->ntab; ++t) {
      const int tiles = (d->tab[t].nK + 63) / 64;
      nT += tiles * chunking(d->grids[d->tab[t].grid].nG - 1);
    }
    if (nT <= (split > 1 ? 160 : 96)) break;
    seg *= 2;
  }
  C.seg = seg;
  int nT = 0;
  for (int t = 0; t < d->ntab; ++t) {
    const nh_hs_table& tb = d->tab[t];
    const int nG = d->grids[tb.grid].nG;
    HSP_REQUIRE((long long)nG * tb.nK < (1LL << 27), "table too large for 32-bit offsets");
    hs_tab& o = C.tab[t];
    o.KD = tb.KD; o.scale = tb.scale;
    H.tscale[t] = tb.scale; H.tnK[t] = tb.nK; o.out = tb.out; o.grid = tb.grid;
    o.nK = tb.nK; o.ldo = tb.ldo; o.nonneg = tb.nonnegative;
    o.tiles = (tb.nK + 63) / 64;
    o.nKp = 64;
    o.sub = 1;
    if (tb.nK <= 32) {
      o.nKp = 32;
      while (o.nKp / 2 >= tb.nK && o.nKp > 1) o.nKp /= 2;
      o.sub = 64 / o.nKp;
    }
    const int nchunks = chunking(nG - 1);
    HSP_REQUIRE(nchunks < 256 && seg < 32768, "table cut into too many chunks");
    o.chunks = nchunks | (nchunks << 8) | (seg << 16);  // (chunks | chunks of length seg | seg)
    o.item0 = nT;
    nT += o.tiles * nchunks;
    o.spec_off = nspec;
    H.tspec[t] = nspec;
    nspec += tb.nK;
  }
  C.nT = nT;
  H.o_part_t = off; off += nT * 64;
  H.o_spec = off; off += nspec;
  C.nspec = nspec;
  H.o_lik = off; off += 5 * d->nE;
  H.o_scale = off; off += nspec;
  H.o_synE = off; off += A.syn_nE;
  H.o_pri = off; off += (int)(sizeof(nh_prior_pack) / sizeof(double)) + 1;
  H.ntab = d->ntab;
  HSP_REQUIRE(d->nblobs >= 0 && d->nblobs <= NH_HS_MAX_BLOB, "bad blob count");
  C.nblob = d->nblobs;
  C.sendw = d->do_accept ? 0 : d->send_width;
  if (C.sendw > 0) {
    int wsum = 1;
    for (int b = 0; b < d->nblobs; ++b) wsum += d->blobs[b].m;
    HSP_REQUIRE(C.sendw >= wsum, "send_width smaller than 1 + the blobs' lengths");
  }
  C.o_mrow = off; off += d->nE + NH_MAX_MOMENT;
  for (int b = 0; b < d->nblobs; ++b) {
    const nh_hs_blob& bl = d->blobs[b];
    HSP_REQUIRE(d->do_accept || d->send_width > 0,
                "blobs in the launch need the in-launch accept or an exchange row");
    HSP_REQUIRE(bl.cur && ((bl.kind == 0 && bl.m == d->nE) ||
                           (bl.kind == 1 && bl.m == 1 && bl.mom >= 0 && bl.mom < d->nmoms)),
                "bad blob");
    C.blob[b] = bl;
  }
  // ---- likelihood: where does each component of the model live? ----
  C.ncomp = d->ncomp; H.nE = d->nE;
  for (int q = 0; q < d->ncomp; ++q) {
    const nh_comp& cp = d->comps[q];
    HSP_REQUIRE(cp.ptr && cp.ld >= d->nE, "bad component");
    hs_comp& o = C.comp[q];
    o.ptr = cp.ptr; o.ld = cp.ld; o.scale = cp.scale; o.off = -1;
    for (int t = 0; t < d->ntab && o.off < 0; ++t) {
      const long long dd = cp.ptr - d->tab[t].out;
      if (dd >= 0 && dd + d->nE <= d->tab[t].nK && cp.ld == d->tab[t].ldo)
        o.off = C.tab[t].spec_off + (int)dd;
    }
    if (o.off < 0 && d->syn.grid >= 0) {
      const long long dd = cp.ptr - d->syn.out;
      if (dd >= 0 && dd + d->nE <= A.syn_nE && cp.ld == d->syn.ldo) o.off = H.syn_spec_off + (int)dd;
    }
  }
  H.conv = d->conv; H.flux = d->flux; H.elo = d->err_lo; H.ehi = d->err_hi; H.ul = d->ul;
  H.cl = d->cl;
  C.lp = d->lp; C.model_out = d->model_out; C.total = d->total;
  C.pri.n = d->nterms;
  for (int t = 0; t < d->nterms; ++t) C.pri.t[t] = d->terms[t];
  // ---- the log-domain block behind everything else, where it fits
  H.o_s2 = 0;
  const size_t lds_core = (size_t)off * sizeof(double);  // (what the resident loop builds on: it has a block of its own)
  if (d->syn.grid >= 0 && k.syn2 != 0) {
    const int sg = d->syn.grid, nGs = d->grids[sg].nG;
    if (k.rt_debug)
      fprintf(stderr, "S2: grid %d nG %d nE %d log-uniform %d off %d (%.1f KB) split %d\n", sg, nGs, d->syn.nE, (int)A.s2_ok, off,
              off * 8.0 / 1024, split);
    if (A.s2_ok) {
      const int o = off + (off & 1);  // (the pieces are read as ds_read_b128)
      const int need = HS_S2_HDR + (S.s2.par.P + 1) * HS_S2_STRIDE + HS_S2_TN + nGs + (nGs + 2 * HS_S2_GUARD) +
                       4 * d->syn.nE + (d->syn.nE + 1) / 2 + 1;
      if ((size_t)(o + need) * sizeof(double) <= 160 * 1024) {  // (a CU's LDS; the plan's own layout keeps to 150 KB)
        H.o_s2 = o;
        off = o + need;
        // (items that start on a piece boundary with a node and six coefficients of their own:
        // short ones pay for that -- the resident loop's lengths)
        // (cfg3 / 512, one launch per half-step: 30.6 us at 16 or 24 nodes per item, 31.1 at 32,
        // 33.9 at 48, 32.7 in the direct form)
        if (!k.syn_nodes.set) C.syn_nodes = split == 1 ? 24 : (C.syn_nodes < 16 ? 16 : C.syn_nodes);
      }
    }
  }
  const size_t lds = (size_t)off * sizeof(double);
  if (lds_core > 150 * 1024) *lds_overflow = true;
  HSP_REQUIRE(lds_core <= 150 * 1024, "the model's grids and tables do not fit in LDS");
  S.threads = threads; S.split = split; S.segscale = segscale;
  S.rowsplit = rowsplit; S.rt = rt_plan;
  S.lds_core = lds_core; S.lds_bytes = lds;
  return NH_OK;
}

// the plan of nh_half_step_create: H (all but the pointers to the plan's own device memory and the
// first trip's block, which hs_create publishes) and S.
// (a split launch cuts the work items finer and needs more LDS for their partial sums: where
// that does not fit, coarser items before fewer workgroups per walker)
static inline int hs_plan(const nh_hs_desc* d, const hs_knobs& k, const hs_facts& f, hs_hot& H, hs_shape& S) {
  hs_plan_front A;
  int rc = hs_plan_checked(d, k, f, H, S, A);
  if (rc != NH_OK) return rc;
  for (int kmax = k.kmax;; kmax >>= 1)
    for (int segscale = 1; segscale <= 4; segscale *= 2) {
      bool lds_overflow = false;
      rc = hs_plan_shape(d, k, f, A, kmax, segscale, H, S, &lds_overflow);
      if (rc == NH_OK || !lds_overflow || kmax <= 1) return rc;
    }
}

// ---- the resident loop on top of a plan ---------------------------------------------------------
struct hs_run_shape {
  bool rt;           // the instance whose table items stay in registers
  size_t lds_bytes;
  hs_s2_host s2;     // the log-domain table (valid where R.syn2 != 0)
};

// syn_xg: host copy of the synchrotron grid's nodes (read only where the log-domain form is allowed)
static inline int hs_run_plan(const nh_halfstep_plan* P, bool shared, int rank, int nrank, const hs_knobs& k,
                              const double* syn_xg, hs_run& R, hs_run_shape& S) {
  static const char* who = "hs_run_create";
  const hs_hot& H = P->hot;
  HSP_REQUIRE(shared || H.C.do_accept, "the resident loop needs the in-launch accept");
  HSP_REQUIRE(H.ndim <= 15, "at most 15 fit parameters in a record (32 granules per wave half)");
  HSP_REQUIRE(shared || (H.lo == 0 && H.nloc == H.ns), "the resident loop moves whole half-ensembles");
  HSP_REQUIRE(!shared || (nrank <= HS_RUN_MAX_RANKS && rank >= 0 && rank < nrank && H.nloc >= 1 &&
                          H.lo >= 0 && H.lo + H.nloc <= H.ns),
              "a shared ensemble: at most 8 ranks, each with at least one walker of every half-step");
  HSP_REQUIRE(H.C.lp == nullptr, "a prior evaluated by a launch of its own cannot ride in the resident loop");
  for (int b = 0; b < H.C.nblob; ++b)
    HSP_REQUIRE(2LL * H.ns * H.C.blob[b].m < (1LL << 31), "a blob's rows of one step: too large for 32-bit element offsets");
  for (int q = 0; q < H.C.ncomp; ++q)
    HSP_REQUIRE(H.C.comp[q].off >= 0, "every component of the model must be produced inside the launch");
  memset(&R, 0, sizeof(R));
  R.N = 2 * H.ns;
  R.gr = ((2 * (H.ndim + 1) + 15) / 16) * 16;
  // LDS: the plan's layout, then what stays resident on top of it
  int off = (int)(P->lds_core / sizeof(double));
  // Workgroups of 1024 threads own their CU: the grids' nodes, ln E (and E where the particle
  // distribution has a break) stay in LDS for the whole launch.  Smaller workgroups (a half-step
  // of more walkers than CUs, k_half_step item 14) share a CU, and LDS decides how many fit:
  // they read the nodes from L2 every slice, as k_half_step does, while a neighbour computes.
  // RT: a table-only model in workgroups of <= 512 threads (256 vector registers per lane) keeps
  // its table items' rows in registers (nh_hs.h: hs_rt_item); a workgroup owns its CU then, too
  bool rt = P->rt != 0 && H.syn_grid < 0 && H.ntab > 0 && P->threads <= 512 && k.run_rt != 0;
  rt = rt && H.C.nT <= (P->threads / 64) * P->split;  // (one item per wave)
  const bool grids_in_lds = (P->threads >= 1024 || rt) && k.run_grids_in_lds != 0;
  for (int g = 0; g < NH_MAX_GRIDS; ++g) R.o_gx[g] = R.o_lne[g] = R.o_ge[g] = -1;
  for (int g = 0; g < H.ngrids && grids_in_lds; ++g) {
    R.o_gx[g] = off; off += H.nG[g];
    R.o_lne[g] = off; off += H.nG[g];
    R.o_ge[g] = off;
    if (H.F.broken & 1) off += H.nG[g];
  }
  // ---- the table grids' 1 / lx in LDS, and the weights' units (below)
  for (int g = 0; g < NH_MAX_GRIDS; ++g) R.o_il[g] = -1;
  R.rebalance = k.run_rebalance.or_else(H.syn_grid < 0 ? 1 : 0);
  const bool units_tab = grids_in_lds && k.run_ut != 0;
  // (the plan chose two workgroups per walker for a table-only model with one table: they halve
  // the grids' rows when the units' table is there -- the grids' nodes in LDS -- the chunks divide
  // the walked rows and come in a whole number per workgroup; else they interleave the items)
  R.rowsplit = (P->rowsplit && P->split >= 2 && units_tab && R.rebalance && H.ntab == 1 &&
                HS_CHUNKS(H.C.tab[0].chunks) % P->split == 0 && H.C.nT % P->split == 0 &&
                k.run_rowsplit != 0) ? 1 : 0;
  // K > 1 workgroups per walker: a workgroup computes one work item of every K, and keeps its
  // table items' partial sums in the slot of the GROUP (its n-th item: slot n) -- a K-th of the
  // plan's block of them, which k_half_step fills in full; what that frees (54 KB at four
  // workgroups per walker) is the first place the loop's own arrays go
  // (from four workgroups per walker on: with two, clearing the whole block every slice and
  // summing it blindly measured faster than deciding per chunk whose it is -- cfg5 / 256 10.9
  // against 10.3 M walker-steps/s, cfg3 / 256 7.12 against 6.94; cfg3 / 128, four per walker: 3.95
  // against 4.07 the other way, and its log-domain synchrotron table fits LDS again)
  R.tcompact = P->split >= k.run_tcompact_min ? 1 : 0;
  int hole_lo = 0, hole_hi = 0;
  if (R.tcompact) {
    int nsmax = 0;  // synchrotron items of a slice at most
    if (H.syn_grid >= 0) nsmax = (H.syn_nE * H.C.syn_cdmax + 63) / 64;
    const int nslots = R.rowsplit ? H.C.nT / P->split : (H.C.nT + nsmax) / P->split + 2;
    if (nslots < H.C.nT) {
      hole_lo = H.o_part_t + nslots * 64;
      hole_hi = H.o_part_t + H.C.nT * 64;
    } else {
      R.tcompact = 0;
    }
  }
  auto take = [&](int n, bool align16) {
    if (align16) hole_lo += hole_lo & 1;
    if (hole_lo + n <= hole_hi) {
      const int at = hole_lo;
      hole_lo += n;
      return at;
    }
    if (align16) off += off & 1;
    const int at = off;
    off += n;
    return at;
  };
  R.o_ut = -1;
  if (units_tab) {
    int nunits = 0;
    for (int g = 0; g < H.ngrids; ++g) nunits += (H.nG[g] + 63) / 64;
    R.o_ut = take(nunits * (HSU_N / 2), true);  // (a unit's descriptor is read as four ds_read_b128)
  }
  {
    int ncols = 0;
    for (int t = 0; t < H.ntab; ++t) ncols += H.C.tab[t].nK;
    R.sum_cols = ncols;
    R.o_sum = take(ncols, false);
    R.o_cmp = take(2 * NH_MAX_COMP + 2, false);
    R.o_pci = take((NH_MAX_PRIOR + 1) / 2, false);
    R.o_synce = H.syn_grid >= 0 ? take(H.syn_nE, false) : -1;
    R.o_lnt = -1;  // (allotted with the log-domain block, below)
    R.o_mt = take(4 * NH_MAX_MOMENT, true);
    {
      int nun = 0;
      for (int g = 0; g < H.ngrids; ++g) nun += (H.nG[g] + 63) / 64;
      R.o_rs = take((9 + nun + 2 * NH_MAX_GRIDS + 1) / 2, false);
    }
    R.nxmax = H.C.nspec + NH_MAX_MOMENT;
  }
  for (int t = 0; t < H.ntab; ++t)
    HSP_REQUIRE(H.nG[H.C.tab[t].grid] < 65536, "a table's grid has too many nodes for the items' descriptors");
  R.o_it = -1;
  if (!rt && H.C.nT > 0)  // (the register-resident instance keeps its rows per wave: no table)
    R.o_it = take((HS_MAX_TAB * HST_N + H.C.nT * HSI_N + 1) / 2, true);
  R.o_pk = take(NH_MAX_PACK * NH_MAX_LAZY * HS_RUN_PKW, false);
  R.o_small1 = take(HS_O_T64, false);
  R.o_olds = take(128, false);
  R.o_lcl = take(H.nE + 1, false);
  R.o_trail = take((HS_RUN_TRAIL * HS_MAX_TAB + H.C.nspec + 1) / 2, false);
  for (int t = 0; t < H.ntab; ++t)
    HSP_REQUIRE(H.C.tab[t].tiles <= HS_RUN_TRAIL, "a table of more column tiles than the resident loop stages");
  // ---- the synchrotron items in the log domain (nh_syn2.h): a log-uniform grid only -------------
  // (the resident loop takes grids from 8 nodes on: its guards need not lie in the plan's arrays)
  R.syn2 = 0;
  R.s2_dev = nullptr;
  if (H.syn_grid >= 0 && k.run_syn2 != 0 && syn_xg != nullptr &&
      hs_s2_prepare(syn_xg, H.nG[H.syn_grid], H.scale[H.syn_grid], 8, S.s2)) {
    const int nG = H.nG[H.syn_grid], Pn = S.s2.par.P;
    R.s2 = S.s2.par;
    R.s2_invd = S.s2.invd; R.s2_lnw0 = S.s2.lnw0; R.s2_z0 = S.s2.z0; R.s2_r746 = S.s2.r746;
    R.s2_cut = S.s2.cut;
    R.s2_cut.on = k.run_syn_cut != 0 ? 1 : 0;
    const int off_was = off, hole_was = hole_lo;  // (tentative: undone if it does not fit)
    R.o_s2tab = take((Pn + 1) * HS_S2_STRIDE, true);  // (16-byte aligned: the pieces are read as ds_read_b128)
    // the plan's LDS holds w | dlw of the synchrotron grid and 1/g^2 | its differences | its
    // cube roots, none of which these items read: when no table and no single-row reduction
    // shares the grid, the new arrays take their place (cfg3 with four workgroups per walker
    // has 142 KB of partial sums and arrays before this table)
    const int sg = H.syn_grid;
    bool own = nG >= 2 * HS_S2_GUARD && H.o_d[sg] == H.o_w[sg] + nG && H.o_ig23 == H.o_dig2 + nG;
    for (int t = 0; t < H.ntab; ++t) own = own && H.C.tab[t].grid != sg;
    for (int q = 0; q < H.nmom; ++q) own = own && H.mgrid[q] != sg;
    R.s2_own = own ? 1 : 0;
    if (own) {
      R.o_s2lw = H.o_w[sg];   // (w, dlw: 2 nG doubles in a row)
      R.o_s2ig = H.o_dig2;    // (dig2, ig23: 2 nG doubles in a row)
    } else {
      R.o_s2lw = take(nG + 2 * HS_S2_GUARD, false);
      R.o_s2ig = take(nG + 2 * HS_S2_GUARD, false);
    }
    if (own && grids_in_lds) {
      R.o_s2lg = R.o_gx[sg];  // (gamma itself: only the weights w = gamma n read it)
    } else {
      R.o_s2lg = take(nG, false);
    }
    R.o_s2q = take(4 * H.syn_nE, false);
    R.o_s2z = take((H.syn_nE + 1) / 2, false);
    R.o_s2t = take(HS_S2_TN, false);
    R.o_lnt = take(256, true);
    if ((size_t)off * sizeof(double) <= 160 * 1024) {
      R.syn2 = 1;
    } else {
      off = off_was;
      hole_lo = hole_was;
    }
  }
  // (1 / lx of the table grids: optional -- where LDS has room behind everything else)
  if (k.run_il != 0)
    for (int g = 0; g < H.ngrids; ++g)
      if (H.o_dp[g] >= 0 && (hole_lo + H.nG[g] <= hole_hi || (size_t)(off + H.nG[g]) * sizeof(double) <= 158 * 1024))
        R.o_il[g] = take(H.nG[g], false);
  R.syn_nodes = H.C.syn_nodes;
  if (P->split == 1 && R.syn_nodes < 32) R.syn_nodes = R.syn2 ? 48 : 32;
  if (P->split == 2 && R.syn_nodes < 10) R.syn_nodes = 10;  // (cfg2: 901 -> 885 us; 914 at 16)
  // (the log-domain items start on a piece boundary with a node and six coefficients of their
  // own: short items pay for that -- cfg3 / 128, four workgroups per walker, us per half-step:
  // 18.4 at the plan's 4 nodes, 16.9 at 16, 17.7 at 24, direct form 17.2; cfg3 / 256, two per
  // walker: 20.8 at 10, 20.8 at 16, 20.0 at 24; cfg2 / 256: 17.7 at 10 and at 16, 18.3 at 24)
  if (R.syn2 && P->split >= 2 && R.syn_nodes < 16) R.syn_nodes = 16;
  R.syn_nodes = k.run_syn_nodes.or_else(R.syn_nodes);
  R.pipeline = k.run_pipeline;
  if (k.run_fail_at > 0)
    fprintf(stderr, "libnaima_hip: NH_RUN_FAIL_AT=%d -- that launch of the resident loop is made to time "
                    "out (fault injection of the tests)\n", k.run_fail_at);
  HSP_REQUIRE(R.syn_nodes >= 1, "NH_RUN_SYN_NODES must be positive");
  const size_t lds = (size_t)off * sizeof(double);
  HSP_REQUIRE(lds <= 160 * 1024, "the resident loop's working set does not fit in LDS");
  S.rt = rt;
  S.lds_bytes = lds;
  return NH_OK;
}

// The resident launch's grid from what the runtime reports: per_cu resident workgroups of the
// instance per CU, ncu CUs (the share applied).  Every workgroup of the launch has to be resident
// (they wait for each other's records).
// (MI355X_MICROARCH.md: the query can be one block per CU high where the SGPR file is what
// limits residency -- 6 waves per SIMD at this kernel's ~110 SGPRs; its 128 VGPRs allow 4,
// so registers or LDS bind first and the query is exact.  The bounded waits are the net.)
// *deep_candidate: the instance with two walkers in flight is worth asking the runtime about
static inline int hs_run_grid(const nh_halfstep_plan* P, bool shared, bool rt, const hs_run& R, const hs_knobs& k,
                              int per_cu, int ncu, int* grid, bool* deep_candidate) {
  static const char* who = "hs_run_create";
  const hs_hot& H = P->hot;
  HSP_REQUIRE(per_cu >= 1 && ncu >= 1, "the resident kernel does not fit a compute unit");
  long long cap = (long long)per_cu * ncu;
  if (k.run_grid.set) cap = k.run_grid.v > 0 ? k.run_grid.v : cap;
  // More walkers per half-step than resident workgroups: a workgroup takes several of a slice,
  // one after the other (dependencies still point backwards in (slice, walker) order).  Pays for
  // workgroups that own their CU -- cfg3 at 1024 / 2048 walkers: 7.8 / 8.1 M walker-steps/s
  // launched per half-step, 10.9 / 11.2 M resident -- not for the small workgroups of a
  // table-only model (cfg5 at 1024 walkers per half-step ran 19.6 M walker-steps/s with two
  // walkers per workgroup and slice, two 256-thread workgroups per CU, against 24.2 M launched
  // per half-step, four).  NH_RUN_MAX_PER_WG overrides (1: never).
  const long long per_wg = k.run_max_per_wg.or_else(P->threads >= 1024 ? 8 : 1);
  HSP_REQUIRE((long long)H.nloc * P->split <= cap * (per_wg > 1 ? per_wg : 1),
              "more walkers per half-step than resident workgroups");
  *grid = (int)(H.nloc < cap / P->split ? H.nloc : cap / P->split);
  // two walkers in flight (the DEEP instance): one GPU's loop whose workgroups own their CU, have
  // the walker to themselves and take more than one of a slice -- a model with a synchrotron
  // component (the 1024-thread instances; a table-only model's ensembles of that size run in small
  // workgroups that share a CU, where the hardware overlaps them).  NH_RUN_PIPELINE=0: never.
  // (With phase A alone made ahead cfg2 -- synchrotron items only, twenty of them for sixteen waves --
  // measured 1 % slower and models without table items were left out; with the priors made ahead as
  // well it gains like cfg3: cfg2 / 1024 13.61 -> 14.01 M, / 2048 14.01 -> 14.73 M.)
  // (taken where it is as resident as the instance the grid was sized for: per_cu_deep >= per_cu)
  *deep_candidate = !shared && !rt && H.syn_grid >= 0 && P->split == 1 && P->threads >= 1024 &&
                    H.nloc > *grid && R.pipeline != 0;
  return NH_OK;
}

// ---- not the planner's: what fills its inputs (nh_halfstep.hip) -----------------------------------
hs_knobs hs_knobs_read();  // every environment override, read once per create
bool hs_read_grid(const double* xg, int nG, std::vector<double>& out);  // host copy of a grid's nodes (after a sync)
