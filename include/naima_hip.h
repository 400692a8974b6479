/* naima_hip.h -- C ABI of libnaima_hip.so: the MI355X (gfx950) implementation of
 * naima's radiative-likelihood hot path.
 *
 * The reference (zblz/naima) has NO FFI: the path sits behind Python callables
 * (SURVEY.md 8b).  This header is the boundary this build introduces; every
 * entry point names the reference function(s) it replaces (paths relative to
 * /root/reference/src/naima/).  INTEGRATION.md shows the ctypes stub a naima
 * maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a
 *     negative NH_E* code, and nh_last_error() returns a thread-local message;
 *   - all numeric data are float64, C-contiguous;
 *   - compute entry points take DEVICE pointers obtained from nh_alloc() and are
 *     asynchronous on the context's HIP stream (stream-ordered, single host
 *     thread per context, no callbacks).  nh_upload/nh_download/nh_sync move
 *     data and synchronise;
 *   - "N" is the number of walkers in the batch (emcee evaluates lnprob once
 *     per walker, core.py:450-457; here a half-ensemble is ONE call);
 *   - particle spectra travel between kernels as the per-walker weight arrays
 *       w[N][nG]  = x_i * n_w(E_i)      dlw[N][nG]: dlw[i] = ln|w[i+1]/w[i]|
 *     with x the integration variable (Lorentz factor for electrons, total
 *     energy in GeV for protons) and n the particles per unit x; the log-ratios
 *     of ADJACENT nodes (last entry unused) are what utils.py:336 needs and are
 *     assembled from small, separately accurate pieces;
 *   - emission kernels travel as TRANSPOSED tables Kt[nG][nK] with
 *     dlnKt[i][k] = ln|Kt[i+1][k]/Kt[i][k]| (last row unused); the
 *     table builders write an [nG][nE] block with row stride ld >= nE, so several
 *     seeds can sit side by side in one [nG][S*nE] table (Kt + j*nE, ld = S*nE);
 *   - spectra are returned in 1/(s eV) (intrinsic luminosity per unit energy),
 *     exactly what <Class>._spectrum() returns in the reference.
 */
#ifndef NAIMA_HIP_H
#define NAIMA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nh_ctx nh_ctx;

enum {
  NH_OK = 0,
  NH_EINVAL = -1,  /* bad argument */
  NH_EHIP = -2,    /* HIP runtime error (message has the hipError string) */
  NH_ENOMEM = -3,
  NH_ECOMM = -4    /* RCCL error */
};

/* particle distribution kinds, models.py:49-422 */
enum {
  NH_PD_POWERLAW = 0,            /* models.py:88-92   */
  NH_PD_ECPL = 1,                /* models.py:157-161 */
  NH_PD_BROKENPL = 2,            /* models.py:234-238 */
  NH_PD_ECBPL = 3,               /* models.py:330-335 */
  NH_PD_LOGPARABOLA = 4          /* models.py:402-407 */
};
/* parameter row of a particle distribution (energies in eV):
 *   [0] amplitude (1/eV)   [1] e_0      [2] alpha | alpha_1
 *   [3] e_cutoff           [4] beta     [5] e_break   [6] alpha_2   [7] unused
 * LogParabola uses [2]=alpha, [4]=beta. */
#define NH_PD_NPAR 8

/* hadronic high-energy models, radiative.py:1179-1209 */
enum { NH_PP_GEANT4 = 0, NH_PP_PYTHIA8 = 1, NH_PP_SIBYLL = 2, NH_PP_QGSJET = 3 };

/* ---- context, memory, stream ------------------------------------------- */
const char* nh_last_error(void);
int nh_version(void);
int nh_create(int device, nh_ctx** out);
int nh_destroy(nh_ctx* ctx);
/* HIP devices visible to this process (no context needed).  The reference's parallel mode asks
 * for `threads` worker processes and takes what the host gives (core.py:446-448: Pool(threads));
 * a launcher of one rank per GPU checks this first and refuses a run the node cannot hold. */
int nh_device_count(int* count);
int nh_device_info(nh_ctx* ctx, char* name, int name_len, int* compute_units,
                   double* hbm_bytes, int* clock_khz);
/* PCI bus id of the context's GPU, e.g. "0000:c1:00.0" (len >= 16): one worker per GPU is the
 * reference's Pool(threads) with GPUs for workers (core.py:446-457) -- a launcher checks that the
 * ranks' ids are distinct */
int nh_device_pci_bus_id(nh_ctx* ctx, char* out, int len);
int nh_alloc(nh_ctx* ctx, long long bytes, void** dev_out);
int nh_free(nh_ctx* ctx, void* dev);
int nh_upload(nh_ctx* ctx, void* dev_dst, const void* host_src, long long bytes);
/* host -> device on a copy stream of its own: not ordered behind the main stream's work and not
 * waited for by nh_sync (the NEXT block of stretch-move random numbers goes up while the current
 * block's launch runs; emcee draws them inside the step, StretchMove.get_proposal).  `marker` is
 * recorded behind the copy; nh_stream_wait_marker orders the main stream behind it.  `after`
 * orders the copy itself behind a point of the main stream: the destination may still be read
 * by launches queued before that point (a ring of blocks that wraps). */
int nh_upload_ahead(nh_ctx* ctx, void* dev_dst, const void* host_src, long long bytes,
                    void* marker, void* after /* marker on the main stream the copy waits for, or NULL */);
int nh_stream_wait_marker(nh_ctx* ctx, void* marker);
int nh_download(nh_ctx* ctx, void* host_dst, const void* dev_src, long long bytes);
int nh_memset(nh_ctx* ctx, void* dev, int byte, long long bytes);
/* dev[0..n) := values[0..n), n <= 8 64-bit words carried as kernel arguments: stream-ordered
 * like nh_upload, without the staging copy an upload from pageable memory costs (the
 * descriptors a run of the sampler re-points: where its chain history goes) */
int nh_set_words(nh_ctx* ctx, void* dev, const long long* values /*host*/, int n);
int nh_sync(nh_ctx* ctx);
/* pinned host staging + markers: nh_upload from a pinned buffer is truly asynchronous, so
 * the host can prepare half-step h+1 while the device runs h; a marker recorded after the
 * upload tells the host when the pinned buffer may be overwritten */
int nh_host_alloc(nh_ctx* ctx, long long bytes, void** host_out);
int nh_host_free(nh_ctx* ctx, void* host);
int nh_marker_create(nh_ctx* ctx, void** marker_out);
int nh_marker_record(nh_ctx* ctx, void* marker);
int nh_marker_wait(nh_ctx* ctx, void* marker);
int nh_marker_destroy(nh_ctx* ctx, void* marker);
/* HIP-event timing on the context's stream (used by bench.py for the roofline) */
int nh_timer_start(nh_ctx* ctx);
int nh_timer_stop(nh_ctx* ctx, double* elapsed_ms);
/* per-kernel accumulated HIP-event time since the last reset; kernel ids NH_K_* */
enum { NH_K_PDIST = 0, NH_K_INTEGRATE = 1, NH_K_SYNCHROTRON = 2, NH_K_TABLES = 3,
       NH_K_LNPROB = 4, NH_K_SSC = 5, NH_K_GLUE = 6 /* pack, move, scatter, lincomb */,
       NH_K_ROWS = 7 /* k_integrate_rows (We/Wp) */,
       NH_K_HALFSTEP = 8 /* k_half_step: the whole half-step in one launch */,
       NH_K_COOLING = 9 /* nh_cooled_electrons, nh_cooled_weights */, NH_K_COUNT = 10 };
int nh_profile_enable(nh_ctx* ctx, int on);
/* HIP-event time of an empty kernel: the fixed cost an event pair adds per launch */
int nh_profile_calibrate(nh_ctx* ctx, int reps, double* overhead_us);
int nh_profile_read(nh_ctx* ctx, double* ms_per_kernel /*[NH_K_COUNT]*/,
                    long long* launches /*[NH_K_COUNT]*/, int reset);

/* ---- row 1: utils.py:285-355 trapz_loglog ------------------------------ */
/* out[r] = trapz_loglog(y[r][0:n], x[0:n]) for r < nrows (axis=-1 semantics:
 * zero nodes, NaN/sign-change -> log branch, |b+1| <= 1e-10 -> log branch). */
int nh_trapz_loglog(nh_ctx* ctx, const double* y, const double* x, int nrows, int n,
                    double* out);
/* the same with intervals=True (utils.py:350-351): out[row*(n-1) + i] = the term of
 * segment (x_i, x_{i+1}) */
int nh_trapz_loglog_intervals(nh_ctx* ctx, const double* y, const double* x, int nrows, int n,
                              double* out);

/* ---- rows 2,3: models.py eval statics + radiative.py:147-160,1002-1015 -- */
/* w[N][nG] = xg_i * unit_scale * f_kind(e_eV_i; params_w), dlw[i] = ln|w[i+1]/w[i]|.
 * unit_scale = mec2[eV] for electrons (1/eV -> 1/mec2, radiative.py:160) or 1e9
 * for protons (1/eV -> 1/GeV, radiative.py:1015).  n_out (optional, may be NULL)
 * receives the bare n = w/xg (what _nelec/_J return). */
int nh_particle_weights(nh_ctx* ctx, int kind, const double* params /*[N][NH_PD_NPAR]*/,
                        int N, const double* e_eV /*[nG]*/, const double* xg /*[nG]*/,
                        int nG, double unit_scale, double* w, double* dlw, double* n_out);

/* the same walkers on up to NH_MAX_GRIDS grids in ONE launch (the components of a model
 * evaluation use different particle grids) */
typedef struct { const double* e_eV; const double* xg; double* w; double* dlw;
                 double unit_scale; int nG; int pad;
                 const double* ln_e; /* ln e_eV[i], or NULL: taken per node */
                 const double* lx;   /* ln(xg[i+1]/xg[i]) (nh_grid_logratio), or NULL */
               } nh_grid;
#define NH_MAX_GRIDS 4
int nh_particle_weights_multi(nh_ctx* ctx, int kind, const double* params, int N,
                              const nh_grid* grids /*host [ngrids]*/, int ngrids);

/* lx[i] = ln(xg[i+1]/xg[i]), i < nG-1 (the abscissa ratios of utils.py:336) */
int nh_grid_logratio(nh_ctx* ctx, const double* xg, int nG, double* lx);

/* ---- the generic per-walker reduction (rows 1+6..10) --------------------- */
/* out[w*ldo + k] = scale[k] * trapz_loglog(n_w * K_k, xg)  for k < nK,
 * (summed over the nsplit planes, see below)
 * evaluated as sum_i  lx_i * (u2-u1)/ln(u2/u1),  u = w_i*Kt[i][k],
 * ln(u2/u1) = dlw[i] + dlnKt[i][k].
 * scale may be NULL (=1).  nonnegative != 0 promises Kt >= 0, w of one sign, and dlnKt
 * finite with dlnKt[i][k] >= 1e300 wherever Kt[i][k] or Kt[i+1][k] is zero (what every
 * nh_table_* builder writes; true for all emission tables except the FITPACK look-up
 * table, which rings below zero, and the Baring+99 fits): sign-change and zero-node
 * handling are then compiled out of the inner loop.  Replaces the trapz_loglog(nelec*gamint, gam) calls of
 * radiative.py:684 (IC), 949-953/966-970 (bremsstrahlung), 1530 (pion decay),
 * 165/193/1020/1053 (We, Wp). */
int nh_integrate_tables(nh_ctx* ctx, const double* w, const double* dlw, int N, int nG,
                        const double* lx, const double* Kt, const double* dlnKt, int nK,
                        const double* scale, double* out, int ldo, int nonnegative,
                        int nsplit);
/* nsplit > 1 cuts the abscissa into nsplit ranges handled by different workgroups, each
 * writing its partial sums to its own plane out + h*N*ldo (h < nsplit): the result is the
 * sum of the planes, which the consumer forms (nh_lnprob / nh_lincomb take the planes as
 * components).  It evens out the work per CU when (tiles x walkers) does not fill the
 * 256 CUs evenly; nh_integrate_tables_nsplit gives the recommended value. */
int nh_integrate_tables_nsplit(int N, int nG, int nK);
/* Which kernel nh_integrate_tables launches for a shape (host arithmetic only; the launcher
 * asks the same function): *rows_kernel = 1 the one-wave-per-(walker, k) kernel of small
 * batches (N*nK < 1024; the other outputs are 0), else the table kernel with *C = 1/2/4/8/16
 * waves splitting the abscissa of a plane, *W = 1/2/4 walkers per thread and *staged = 1 when
 * the workgroup copies its walkers' w and dlw rows to LDS first.  *fused = 1 when, asked through
 * nh_integrate_tables_lnprob (want_epilogue != 0), that launch also carries the likelihood;
 * 0 when the entry point launches it separately.  N = 0 launches nothing: all outputs 0.
 * Sizes that nh_integrate_tables refuses are refused here. */
int nh_integrate_tables_plan(int N, int nG, int nK, int nsplit, int want_epilogue,
                             int* rows_kernel, int* C, int* W, int* staged, int* fused);

/* ---- row 5: radiative.py:282-342 Synchrotron._spectrum ------------------- */
/* out[w*ldo+k] = spectrum 1/(s eV) at photon energy E_eV[k] for field B_G[w*ldB]
 * (Gauss; ldB = 1 for a plain vector, NH_PD_NPAR when B rides in slot 7 of the packed
 * parameter rows); walker-dependent through both w/dlw and B. */
int nh_synchrotron(nh_ctx* ctx, const double* w, const double* dlw, const double* B_G, int ldB,
                   int N, const double* gam, const double* lx, int nG,
                   const double* E_eV, int nE, double* out, int ldo);
/* Which kernel nh_synchrotron launches for a shape (host arithmetic only; the launcher asks the
 * same function): a workgroup of *C = 4/8/16 waves per (walker, tile), *tw <= 64 photon energies
 * per tile, *ktiles = ceil(nE / *tw) tiles per walker (energy k sits in tile k % *ktiles) and
 * *lds_bytes of dynamic LDS, 24 nG + 32768 (above 64 KB the launcher raises the kernel's limit
 * first).  want_epilogue != 0 asks as nh_synchrotron_lnprob does: one tile of 64, the instance
 * that goes on to the likelihood.  N = 0 launches nothing: all outputs 0.  Sizes that
 * nh_synchrotron refuses are refused here: nG < 2, nE < 1, N < 0, the epilogue with nE > 64,
 * more than 150 KB of LDS (nG > 5034). */
int nh_synchrotron_plan(int N, int nG, int nE, int want_epilogue, int* C, int* tw, int* ktiles,
                        int* lds_bytes);

/* ---- rows 6,7: radiative.py:547-607 + G12/G34 345-367 -------------------- */
/* Kt[i][k] (1/s per unit ... as _iso/_ani_ic_on_planck return) for temperature
 * T_K; isotropic != 0 selects the isotropic Eq.14 (theta_rad is not read), otherwise Eq.11
 * with 1 - cos(theta_rad) as the reference forms it (radiative.py:597) for an angle of ANY sign:
 * theta and -theta give the same table, theta = 0 a table of NaN.  T_K = 0 passes (the
 * reference's "positive" admits it) and gives NaN as well.
 * scale[k] = uf*Eph_k/E_eV_k so that integrate_tables gives radiative.py:684-687 */
int nh_table_ic_planck(nh_ctx* ctx, const double* gam, int nG, const double* E_eV, int nE,
                       double T_K, double theta_rad, int isotropic, double* Kt, double* dlnKt,
                       int ld);

/* ---- row 8: radiative.py:609-655 _iso_ic_on_monochromatic ---------------- */
/* seed_E_eV[ns]; ns == 1: seed_dens = energy density eV/cm3 (monochromatic);
 * ns > 1: differential photon density 1/(eV cm3), integrated with trapz_loglog
 * over the seed energies (radiative.py:638-640). */
int nh_table_ic_seed(nh_ctx* ctx, const double* gam, int nG, const double* E_eV, int nE,
                     const double* seed_E_eV, const double* seed_dens, int ns,
                     double* Kt, double* dlnKt, int ld);
/* walker-dependent seed density (SSC: examples/CrabNebula_SynSSC.py:29-31):
 * seed_dens[N][ns]; fused outer+inner reduction, out as nh_integrate_tables. */
int nh_ic_seed_walkers(nh_ctx* ctx, const double* w, const double* dlw, int N,
                       const double* gam, const double* lx, int nG,
                       const double* E_eV, int nE, const double* seed_E_eV,
                       const double* seed_dens /*[N][ns]*/, int ns, double* out, int ldo);

/* The same with the Aharonian-Atoyan kernel of radiative.py:620-637 tabulated: it depends on
 * (seed energy, gamma, photon energy) only, so a sampler builds it once -- nh_ssc_table fills
 * `table` (nh_ssc_table_bytes bytes of device memory: cfg4's grids 374 MB) -- and every step
 * runs the walkers' part alone.  Same result as nh_ic_seed_walkers. */
long long nh_ssc_table_bytes(int nG, int nE, int ns);
int nh_ssc_table(nh_ctx* ctx, const double* gam, int nG, const double* E_eV, int nE,
                 const double* seed_E_eV, int ns, void* table);
int nh_ic_seed_walkers_tab(nh_ctx* ctx, const double* w, const double* dlw, int N,
                           const double* gam, const double* lx, int nG,
                           const double* E_eV, int nE, const double* seed_E_eV,
                           const double* seed_dens /*[N][ns]*/, int ns, const void* table,
                           double* out, int ldo);

/* ---- row 10: radiative.py:838-989 Bremsstrahlung ------------------------- */
/* two tables: sigma_ee (rel/non-rel, 873-928) and sigma_ep = sigma_1 (838-849),
 * both in cm2/eV. */
int nh_table_brems(nh_ctx* ctx, const double* gam, int nG, const double* E_eV, int nE,
                   double* Kt_ee, double* dlnKt_ee, double* Kt_ep, double* dlnKt_ep, int ld);

/* ---- row 9: radiative.py:1215-1482 Kafexhiu+14, 1770-1797 LookupTable ---- */
/* Kt[i][k] = dsigma/dEgamma(Ep_i, Egamma_k) in cm2/GeV */
int nh_table_pion_analytic(nh_ctx* ctx, const double* Ep_GeV, int nG, const double* E_eV,
                           int nE, int hiE_model, int nuclear_enhancement,
                           double* Kt, double* dlnKt, int ld);
/* bicubic tensor-product B-spline (FITPACK bispev) with knots tx[ntx], ty[nty]
 * and coefficients c[(ntx-4)*(nty-4)], evaluated at (log10 Ep, log10 Egamma) */
int nh_table_pion_lut(nh_ctx* ctx, const double* Ep_GeV, int nG, const double* E_eV, int nE,
                      const double* tx, int ntx, const double* ty, int nty, const double* c,
                      double* Kt, double* dlnKt, int ld);

/* ---- row 11: core.py:64-94 lnprobmodel ----------------------------------- */
/* PionDecayKelner06._spectrum (radiative.py:1716-1767; Kelner, Aharonian & Bugayov 2006):
 * out[w*ldo + k] = differential luminosity 1/(s eV) for nh = 1 cm^-3 at photon energies
 * E_eV[k]: full calculation (Eq. 71, :1665-1684) at E >= Etrans_eV, delta-functional
 * approximation (:1693-1714) below, joined at Etrans by nhat (:1743-1748) when `mixed`
 * (the host sets it when energies lie on both sides).  params: the [N][8] particle rows of
 * nh_particle_weights (eV).  The reference's adaptive quad (epsrel 1e-3) is replaced by a
 * fixed Gauss-Legendre rule whose panels end at the integrand's kinks: within 1e-8 of the
 * converged integral for every kind.  nhat_out[N], wp_TeV_out[N] (the `Wp` property,
 * :1716-1728, in TeV) may be NULL.  EINVAL: a kind outside the enum, nE < 1, ldo < nE,
 * Etrans_eV <= 0, nE + 3 doubles beyond 60 KiB of LDS.  N = 0 is no error. */
int nh_pion_kelner06(nh_ctx* ctx, int kind, const double* params, int N, const double* E_eV,
                     int nE, double Etrans_eV, int mixed, double* out, int ldo,
                     double* nhat_out, double* wp_TeV_out);
/* SecondaryLeptonsKelner06._spectrum (no reference counterpart): the secondary electrons and
 * neutrinos of the same collisions, pp -> pi+- -> mu nu -> e nu nu, KAB06 Eq. 62-69 at
 * E >= Etrans_eV and the delta-functional approximation of its section IV below.
 * out[w*ldo + k] = differential luminosity 1/(s eV) for nh = 1 cm^-3 at E_eV[k] of
 * product 0: electrons (e+ + e-), 1: nu_e, 2: nu_mu (= electrons + the pion decay's muon
 * neutrino), 3: all flavours; neutrinos and antineutrinos together, at the source.
 * `match` (the host sets it when an energy lies below Etrans): each of the three components
 * (e, nu_e, numu1) of the delta branch is scaled to meet its full calculation at Etrans
 * (nu_e meets F_e); nhat_out[N][3], in that order, may be NULL (match = 0: all 1).
 * params: the [N][8] particle rows of nh_particle_weights (eV).  Fixed Gauss-Legendre rule
 * on nh_pion_kelner06's panels, within 1e-8 of the converged integrals.  EINVAL: a kind
 * outside the enum, product outside 0..3, nE < 1, ldo < nE, Etrans_eV <= 0, 3 (nE + 2)
 * doubles beyond 60 KiB of LDS.  N = 0 is no error. */
int nh_pp_leptons_kelner06(nh_ctx* ctx, int kind, const double* params, int N,
                           const double* E_eV, int nE, double Etrans_eV, int match, int product,
                           double* out, int ldo, double* nhat_out);

/* model[w][k] = sum_j cscale[j] * comp_j[w*ldc + k]        (1/(s cm2 eV))
 * m' = model*conv[k] (SED<->differential factor, utils.py:219-282)
 * lnl[w] = -sum_{!ul} (m'-flux)^2/(2 sigma^2), sigma = err_hi if m'>flux else err_lo,
 *          + nviol*ln(1-cl[nviol]), nviol = #{ul : m' > flux}   (cl indexed by count).
 * model_out may be NULL.  ncomp <= 4. */
int nh_lnprobmodel(nh_ctx* ctx, const double* const* comps /*host array of dev ptrs*/,
                   const double* cscale /*host [ncomp]*/, int ncomp, int ldc, int N, int nE,
                   const double* conv, const double* flux, const double* err_lo,
                   const double* err_hi, const int* ul, const double* cl,
                   double* model_out, double* lnl);

/* ---- device-resident step loop ------------------------------------------- */
/* A lazy per-walker scalar: value[w] = a * tf(b * base[w*stride] + c); base NULL
 * means the constant a.  It lets the parameter transforms a naima model function
 * writes (10**pars[0] / u.eV, pars[3] * u.uG ...) be folded into the kernel that
 * consumes them, with pars living in HBM. */
enum { NH_TF_ID = 0, NH_TF_POW10 = 1, NH_TF_EXP = 2, NH_TF_LOG = 3, NH_TF_LOG10 = 4,
       NH_TF_SQRT = 5, NH_TF_SQUARE = 6, NH_TF_RECIP = 7 };
typedef struct { const double* base; long long stride; double a, b, c; int tf; int pad; } nh_lazy;
#define NH_MAX_LAZY 8
/* out[w*ld + j] = value_j[w], j < ncols <= NH_MAX_LAZY: builds the [N][NH_PD_NPAR]
 * parameter rows of nh_particle_weights (and B[N]) on the device */
int nh_pack_rows(nh_ctx* ctx, const nh_lazy* cols /*host [ncols]*/, int ncols, int N,
                 double* out, int ld);
enum { NH_OP_ADD = 0, NH_OP_SUB, NH_OP_MUL, NH_OP_DIV, NH_OP_POW, NH_OP_MAX, NH_OP_MIN,
       NH_OP_LT, NH_OP_LE, NH_OP_GT, NH_OP_GE };
int nh_ew_binary(nh_ctx* ctx, int op, const nh_lazy* x, const nh_lazy* y, int N, double* out);

/* a spectrum component: ptr[w*ld + k] * scale */
typedef struct { const double* ptr; long long ld; double scale; } nh_comp;
#define NH_MAX_COMP 8
/* out[w*ldo + k] = rowfac[w] * colfac[k] * sum_j comps[j]   (colfac, rowfac may be NULL):
 * rowfac carries a per-walker physical factor (target density n0 / nh, seed energy
 * density) that the reference applies as a scalar, radiative.py:684-687, 949-987, 1534 */
int nh_lincomb(nh_ctx* ctx, const nh_comp* comps /*host*/, int ncomp, const double* colfac,
               const nh_lazy* rowfac /*host*/, int N, int m, double* out, int ldo);

/* ---- utils.py:285-355 trapz_loglog of a lazy matrix: a band-integrated flux or luminosity
 * per walker, trapz_loglog(spectrum * E, E) (docs/radiative.rst "luminosity by setting distance
 * to 0", tests/test_models.py's known-answer luminosities), without writing the matrix.
 *   y[w][k] = rowfac[w] * colfac[k] * sum_j comps[j]     (as nh_lincomb forms it)
 *   out[w*ldo] = trapz_loglog(y[w][0:n], x[0:n])  for w < N
 * with nh_trapz_loglog's segment term and edge rules (a zero node or x1 == x2 -> 0,
 * |b+1| <= 1e-10 or NaN b -> log branch, n == 1 -> 0) and its order of summation: the result
 * is what nh_trapz_loglog gives for nh_lincomb's output, and the same bits at every call.
 * colfac, rowfac may be NULL; comps[j].ld >= n. */
int nh_trapz_loglog_comps(nh_ctx* ctx, const nh_comp* comps /*host*/, int ncomp,
                          const double* colfac, const nh_lazy* rowfac /*host*/, const double* x,
                          int N, int n, double* out, int ldo);
/* the same with intervals=True (utils.py:350-351): out[w*ldo + i] = the term of segment
 * (x_i, x_{i+1}), i < n-1; n >= 2, ldo >= n-1 */
int nh_trapz_loglog_comps_intervals(nh_ctx* ctx, const nh_comp* comps /*host*/, int ncomp,
                                    const double* colfac, const nh_lazy* rowfac /*host*/,
                                    const double* x, int N, int n, double* out, int ldo);

/* priors of core.py:34-58 on lazy scalars; lp[w] = sum of the terms */
enum { NH_PRIOR_UNIFORM = 0, NH_PRIOR_NORMAL = 1, NH_PRIOR_LOGUNIFORM = 2, NH_PRIOR_VALUE = 3 };
typedef struct { nh_lazy x; double p0, p1; int kind; int pad; } nh_prior;
#define NH_MAX_PRIOR 16
int nh_priors(nh_ctx* ctx, const nh_prior* terms /*host*/, int nterms, int N, double* lp);

/* core.py:97-121 in one launch: model = sum comps; lnl as nh_lnprobmodel;
 * p = lp[w] (NULL = 0) + sum of the prior terms (nterms may be 0);
 * total[w] = isinf(p) ? p : lnl + p. */
int nh_lnprob(nh_ctx* ctx, const nh_comp* comps /*host*/, int ncomp, int N, int nE,
              const double* conv, const double* flux, const double* err_lo,
              const double* err_hi, const int* ul, const double* cl, const double* lp,
              const nh_prior* terms /*host*/, int nterms,
              double* model_out /*[N][nE] or NULL*/, double* total);

/* stretch move on a device-resident ensemble coords[N][ndim], logp[N].  The host ships the
 * random numbers of many half-steps as one block, slice h (stride 3*ns doubles) =
 * { z[ns] | lnU'[ns] (float64) | S[ns] | partner[ns] (int32) }: S = active walkers,
 * partner = each one's partner in the complementary half.  cursor[0] (device int) selects
 * the slice; accept advances it (advance != 0), so a captured graph replays unchanged.
 * propose writes the block [lo, lo+nloc) of the proposals TRANSPOSED (qT[d][j]: pars[d] is
 * a contiguous vector over walkers); accept needs all ns new log-probabilities and
 * optionally leaves the slice's S in sel[ns] for nh_scatter_rows. */
int nh_move_propose(nh_ctx* ctx, const double* coords, const double* blk, const int* cursor,
                    int ns, int ndim, int lo, int nloc, double* qT, double* factors);
int nh_move_accept(nh_ctx* ctx, double* coords, double* logp, const double* blk, int* cursor,
                   const double* newlp, int ns, int ndim, int* accepted, int* naccepted,
                   int* sel, int advance);

/* nh_move_accept on gathered ROWS { lnprob | blob 0 | blob 1 ... } (width doubles each, row j
 * = proposal j of the slice): the blobs of an accepted proposal go to cur[b][walker] (m[b]
 * values each, consecutive in the row).  advance as nh_move_accept. */
int nh_move_accept_rows(nh_ctx* ctx, double* coords, double* logp, const double* blk, int* cursor,
                        const double* rows, int width, int ns, int ndim, int* accepted,
                        int* naccepted, int* sel, int advance, int nblobs,
                        double* const* cur /*host [nblobs]*/, const int* m /*host [nblobs]*/);

/* ---- the two launches that bracket a model evaluation in the device step loop ------
 * Slice protocol of these two: cursor[0] = index of the slice whose proposals are being
 * evaluated (-1 right after a block upload).
 *
 * nh_step_front (one block per proposed walker): proposes block [lo, lo+nloc) of slice
 * cursor[0]+1 into qT/factors, evaluates `packs` (the nh_pack_rows requests the model
 * made on its first evaluation; their lazy columns read qT or are constants) for the
 * proposed walkers, then the particle weights of nh_particle_weights_multi(kind, params,
 * nloc, grids) -- params must be one of the pack outputs -- and `moms`: single-row
 * reductions (We, Wp: nh_integrate_tables with nK = 1) over one of those grids.  When the
 * slice just accepted closed an ensemble step (cursor odd) the chain history row is
 * appended first.  The last block to finish advances the cursor.  `done` is a zeroed
 * device int the launch uses to find that block. */
typedef struct { nh_lazy cols[NH_MAX_LAZY]; int ncols; int ld; double* out; } nh_pack;
#define NH_MAX_PACK 4
/* chain history, DEVICE-resident (the host rewrites it between runs): row n receives
 * coords[N][ndim] and logp[N], n is incremented, while n < cap.  coords == NULL: off. */
typedef struct { double* coords; double* logp; long long n; long long cap; } nh_hist;
typedef struct { int grid; int pad; const double* Kt; const double* dlnKt; double* out; } nh_moment;
#define NH_MAX_MOMENT 4
int nh_step_front(nh_ctx* ctx, const double* coords, const double* logp, const double* blk,
                  int* cursor, int* done, int ns, int ndim, int lo, int nloc, double* qT,
                  double* factors, const nh_pack* packs /*host*/, int npacks, int kind,
                  const double* params, const nh_grid* grids /*host*/, int ngrids,
                  const nh_moment* moms /*host*/, int nmoms, nh_hist* hist /*device or NULL*/);

/* nh_lnprob followed, in the same launch, by the accept of nh_move_accept for walkers
 * [lo, lo+N) of slice cursor[0] (single-rank loop: every walker's new log-probability is
 * the one this launch just computed).  The cursor is not advanced (nh_step_front does). */
typedef struct { double* coords; double* logp; const double* blk; const int* cursor; int ns;
                 int ndim; int lo; int pad; int* accepted; int* naccepted; int* sel; } nh_accept;
int nh_lnprob_accept(nh_ctx* ctx, const nh_comp* comps /*host*/, int ncomp, int N, int nE,
                     const double* conv, const double* flux, const double* err_lo,
                     const double* err_hi, const int* ul, const double* cl, const double* lp,
                     const nh_prior* terms /*host*/, int nterms, double* model_out,
                     double* total, const nh_accept* mv /*host*/);

/* nh_synchrotron whose workgroups go on to evaluate nh_lnprob (+ nh_lnprob_accept's move
 * when mv != NULL) for their own walker: for models where the synchrotron spectrum is the
 * last component the likelihood waits for, the step loop saves a launch.  comps[syn_comp]
 * must be this launch's output (it is taken from LDS); nE <= 64. */
int nh_synchrotron_lnprob(nh_ctx* ctx, const double* w, const double* dlw, const double* B_G,
                          int ldB, int N, const double* gam, const double* lx, int nG,
                          const double* E_eV, int nE, double* out, int ldo,
                          const nh_comp* comps /*host*/, int ncomp, int syn_comp,
                          const double* conv, const double* flux, const double* err_lo,
                          const double* err_hi, const int* ul, const double* cl,
                          const double* lp, const nh_prior* terms /*host*/, int nterms,
                          double* total, const nh_accept* mv /*host or NULL*/);

/* the same for a table reduction that is the last producer (pi0 decay, a single-seed IC
 * model): nh_integrate_tables (one plane) whose workgroups finish their walkers' nh_lnprob
 * (+ accept when mv != NULL).  The spectrum has nK energies; comps[loc_comp] must be this
 * launch's output.  Shapes that cannot carry the epilogue (more than 64 columns, ...) are
 * run as the two launches. */
int nh_integrate_tables_lnprob(nh_ctx* ctx, const double* w, const double* dlw, int N, int nG,
                               const double* lx, const double* Kt, const double* dlnKt, int nK,
                               const double* scale, double* out, int ldo, int nonnegative,
                               const nh_comp* comps /*host*/, int ncomp, int loc_comp,
                               const double* conv, const double* flux, const double* err_lo,
                               const double* err_hi, const int* ul, const double* cl,
                               const double* lp, const nh_prior* terms /*host*/, int nterms,
                               double* total, const nh_accept* mv /*host or NULL*/);
/* dst[idx[lo+j]][0:m] = src[j][0:m] where accepted[lo+j] (accepted NULL = all) */
int nh_scatter_rows(nh_ctx* ctx, double* dst, int ldd, const double* src, int lds,
                    const int* idx, const int* accepted, int lo, int nloc, int m);
int nh_copy(nh_ctx* ctx, void* dev_dst, const void* dev_src, long long bytes);

/* ---- the general electron path: a particle grid PER WALKER --------------------------------
 * Eemin / Eemax as per-walker values (fit parameters; the reference takes any keyword as
 * per-call state, radiative.py:280, 430): walker w integrates over
 *   gamma = logspace(log10(Eemin_w/mec2), log10(Eemax_w/mec2), max(10, int(nEed * decades)))
 * (radiative.py:147-154), built with its weights in the workgroup's LDS; the emission kernel is
 * evaluated at every (node, photon energy) -- no walker-independent table exists.
 *   what = 0: Synchrotron._spectrum (radiative.py:282-342) with B_G per walker,
 *             out[w*ldo + k] in 1/(s eV)
 *   what = 1: InverseCompton on nseed thermal seed fields (radiative.py:547-607), seed s at
 *             out[w*ldo + s*nE + k] = trapz_loglog(nelec sigma_s, gamma); the caller applies
 *             uf * Eph / E (radiative.py:684-687); bit s of seed_iso_mask set: seed s is
 *             isotropic and seed_theta[s] is not read.  An anisotropic seed's angle may have any
 *             sign -- the reference forms 1 - cos(theta), radiative.py:597: theta and -theta give
 *             the same spectrum, theta = 0 NaN.  T and theta are lazy scalars: a seed temperature
 *             / angle may itself be a fit parameter (a walker with T <= 0 gets the NaN the
 *             reference's arithmetic gives)
 *   what = 2: We = trapz_loglog(gamma nelec, gamma mec2) over the walker's grid, erg
 *             (radiative.py:162-195: We, compute_We with per-walker limits); out[w*ldo]
 *   what = 3: Bremsstrahlung (radiative.py:838-989): out[w*ldo + k] = trapz_loglog(nelec
 *             sigma_ee, gamma), out[w*ldo + nE + k] the same with sigma_1 (electron-ion), per
 *             eV; the caller applies n0 c and the abundance weights (radiative.py:949-987)
 * The limits arrive in the unit the caller's Quantity carries, with that unit's value in erg
 * beside them: the kernel forms gamma_min = (Eemin / mec2[erg]) * unit_erg exactly as the host
 * path does (what astropy reduces Eemin / mec2 to), so both paths take log10 of the same double.
 * nEed is a lazy scalar too (nodes per decade per walker), of any sign: a count below 10 is 10.
 * A walker whose nEed * decades is not finite -- a limit that is negative (NaN) or 0 (+-inf),
 * where the reference's int() raises ValueError / OverflowError -- gets NaN and leaves status
 * alone; so does a synchrotron walker with B <= 0, where the reference's arithmetic gives NaN.
 * nmax: grid nodes the workgroup's LDS is sized for (4 nmax doubles); a walker that needs more
 * gets NaN and status[0] (device ints, zeroed by the caller) receives the largest count asked
 * for.  status[1] counts evaluations whose nEed * decades lay within 1e-9 of an integer: there
 * int() may differ between this log10 and numpy's in the last place -- reported, not silent. */
int nh_general_electron(nh_ctx* ctx, int kind, const double* rows /*[N][NH_PD_NPAR]*/, int N,
                        const nh_lazy* Eemin /*host*/, double Eemin_unit_erg,
                        const nh_lazy* Eemax /*host*/, double Eemax_unit_erg,
                        const nh_lazy* nEed /*host*/, int what, const nh_lazy* B_G /*host, what = 0*/,
                        const nh_lazy* seed_T_K /*host*/, const nh_lazy* seed_theta /*host*/,
                        int seed_iso_mask, int nseed, const double* E_eV, int nE, double* out, int ldo, int nmax,
                        int* status /*device, 2 ints*/);
/* the same over every walker's own grid for ONE monochromatic (ns = 1: seed_dens its energy
 * density, eV/cm3) or tabulated (seed_dens in 1/(eV cm3) at the ns energies seed_E, eV) isotropic
 * seed field that all walkers share -- InverseCompton._calc_specic's inner trapz_loglog over the
 * seed's energies (radiative.py:609-655) at every (node, photon energy):
 * out[w*ldo + k] = trapz_loglog(nelec sigma_seed, gamma); the caller applies Eph / E
 * (radiative.py:684-687) */
int nh_general_electron_seed(nh_ctx* ctx, int kind, const double* rows /*[N][NH_PD_NPAR]*/, int N,
                             const nh_lazy* Eemin /*host*/, double Eemin_unit_erg,
                             const nh_lazy* Eemax /*host*/, double Eemax_unit_erg,
                             const nh_lazy* nEed /*host*/, const double* seed_E /*device*/,
                             const double* seed_dens /*device*/, int ns,
                             const double* E_eV /*device*/, int nE, double* out, int ldo, int nmax,
                             int* status);
/* The same with a photon density PER WALKER, seed_dens[w * seed_ld + s] (seed_ld >= ns): a
 * synchrotron-self-Compton seed -- each walker's own synchrotron photons,
 * examples/CrabNebula_SynSSC.py:29-45 -- combined with Eemin / Eemax / nEed per walker
 * (InverseCompton takes any keyword per call, radiative.py:430; inner integral :609-655). */
int nh_general_electron_seed_rows(nh_ctx* ctx, int kind, const double* rows, int N,
                                  const nh_lazy* Eemin, double Eemin_unit_erg, const nh_lazy* Eemax,
                                  double Eemax_unit_erg, const nh_lazy* nEed, const double* seed_E,
                                  const double* seed_dens, long long seed_ld, int ns,
                                  const double* E_eV, int nE, double* out, int ldo, int nmax,
                                  int* status);

/* The same for protons: Epmin / Epmax / nEpd per walker (radiative.py:1002-1055, 1495-1536).
 * Walker w integrates over Ep = logspace(log10 Epmin_w, log10 Epmax_w, max(10, int(nEpd_w *
 * decades))) GeV, decades = log10(Epmax / Epmin) (count_mode 0: the spectrum's grid,
 * radiative.py:1002-1009) or log10 Epmax - log10 Epmin (count_mode 1: compute_Wp's,
 * :1047-1053); the limits arrive in the caller's unit with that unit in GeV beside them.
 *   what = 0: out[w*ldo + k] = trapz_loglog(dsigma/dE(Ep, E_k) J, Ep), the Kafexhiu+14 cross
 *             section evaluated at every (node, energy) (hiE: NH_PP_*, nuc: nuclear enhancement);
 *             the caller applies nh c (radiative.py:1530-1536)
 *   what = 1: the same with the look-up table's FITPACK spline (tx, ty, cf as for
 *             nh_table_pion_lut) evaluated at every (node, energy)
 *   what = 2: out[w*ldo] = Wp = trapz_loglog(Ep J, Ep), GeV
 * nmax / status as for nh_general_electron. */
int nh_general_proton(nh_ctx* ctx, int kind, const double* rows /*[N][NH_PD_NPAR]*/, int N,
                      const nh_lazy* Epmin /*host*/, double Epmin_unit_GeV,
                      const nh_lazy* Epmax /*host*/, double Epmax_unit_GeV,
                      const nh_lazy* nEpd /*host*/, int count_mode, int what, int hiE, int nuc,
                      const double* tx, int ntx, const double* ty, int nty, const double* cf,
                      const double* E_eV, int nE, double* out, int ldo, int nmax,
                      int* status /*device, 2 ints*/);

/* ---- ONE launch per half-step ---------------------------------------------------------
 * nh_step_front + every table reduction of the model + its synchrotron component +
 * nh_lnprob (+ the accept of nh_lnprob_accept when do_accept) for the proposed walkers
 * [lo, lo+nloc) of slice cursor[0]+1, one workgroup per walker: emcee's
 * StretchMove.get_proposal / RedBlueMove.propose around core.py:97-121 around
 * radiative.py:282-342, 657-710, 1495-1536.  The particle weights stay in LDS (they are
 * also written to grids[].w/.dlw when write_weights), every spectrum is written to its
 * `out` as the separate entry points would.
 * Slices: nh_half_step_begin_block tells the plan that a new block of moves sits in `blk`;
 * the k-th launch after it proposes, evaluates and (do_accept) accepts slice first_slice + k -- the plan
 * counts its own launches on the device, nothing has to be advanced by the caller.  The
 * history row of a closed ensemble step (row steps_before + k/2 - 1 of hist, hist->n is not
 * used) is written by the NEXT launch of the same block of moves; after the last half-step
 * of a block, and whenever the chain may be read, the caller writes it with nh_hist_append
 * (writing a row twice is harmless).  The descriptor is copied once (nh_half_step_create);
 * a launch takes no other argument, so it can be captured into a hipGraph and replayed. */
/* KD: the emission table of nh_integrate_tables in the interleaved layout the kernel streams,
 * KD[(i*nK + k)*2 + {0,1}] = {Kt[i][k], dlnKt[i][k]} (nh_table_interleave).  Where column k
 * changes sign between nodes i and i+1 the second entry is NaN: that segment takes the
 * reference's log branch (NaN exponent b, utils.py:336-345) -- decided once per table, the
 * sign pattern does not depend on the walker.  A table declared `nonnegative` to the half-step
 * plan is built WITH lx = ln(x[i+1]/x[i]) of its grid: its second entries are dlnKt / lx (the
 * kernel then integrates a segment as (u2 - u1) / (dl / lx), utils.py:336-339 without the
 * multiplication); other tables with lx = NULL. */
typedef struct { int grid; int nK; int ldo; int nonnegative;
                 const double* KD; const double* reserved; const double* scale /*[nK] or NULL*/;
                 double* out /*[nloc][ldo]*/; } nh_hs_table;
int nh_table_interleave(nh_ctx* ctx, const double* Kt, const double* dlnKt,
                        const double* lx /*[nG-1] device, or NULL*/, int nG, int nK,
                        double* KD);
typedef struct { int grid /* -1: no synchrotron component */; int nE; int ldo;
                 int bcol /* column of the particle rows that carries B [G], or -1 */; int ldB;
                 int n1 /* 0, or: energies [n1, nE) go to out2 -- two Synchrotron.flux calls of one
                           model evaluation (CrabNebula_SynSSC.py:29, 45) as ONE component */;
                 const double* E_eV; const double* B /* [nloc*ldB] when bcol < 0 */;
                 double* out /*[nloc][ldo]*/; double* out2 /*[nloc][ldo2] == out + nloc * ldo, or NULL*/; int ldo2; int pad2;
               } nh_hs_syn;
#define NH_HS_MAX_TAB 4
/* a blob the model function returns besides its flux (core.py:103-113; emcee keeps the blobs
 * of the ACCEPTED position of every walker): kind 0 = the model spectrum itself (the sum of
 * `comps`, nE values), kind 1 = lazy(result of single-row reduction `mom`) (We, Wp).  On
 * accept the launch writes the row into cur[walker]; with the coordinates it appends the
 * ensemble's rows to the history at *hist (a device word holding the history's base, 0: off). */
typedef struct { int kind; int mom; int m; int pad; nh_lazy lazy;
                 double* cur /*[N][m]*/; double* const* hist /*device*/; } nh_hs_blob;
#define NH_HS_MAX_BLOB 4
typedef struct {
  double* coords; double* logp; const double* blk;
  int* cursor; /* out: the slice of the launch, for nh_move_accept(advance = 0) after it */
  int* reserved;
  int ns, ndim, lo, nloc;
  double* qT; double* factors; nh_hist* hist /* device, or NULL */;
  int* accepted; int* naccepted; int* sel;
  int do_accept;      /* 1: single rank, the launch accepts; 0: total[] only (sharded loop) */
  int write_weights;  /* also store w / dlw in grids[].w / .dlw */
  nh_pack packs[NH_MAX_PACK]; int npacks;
  int kind; const double* params;
  nh_grid grids[NH_MAX_GRIDS]; int ngrids;
  nh_moment moms[NH_MAX_MOMENT]; int nmoms;
  nh_hs_table tab[NH_HS_MAX_TAB]; int ntab;
  nh_hs_syn syn;
  nh_comp comps[NH_MAX_COMP]; int ncomp; int nE;
  const double* conv; const double* flux; const double* err_lo; const double* err_hi;
  const int* ul; const double* cl; const double* lp /* [nloc] or NULL */;
  nh_prior terms[NH_MAX_PRIOR]; int nterms;
  double* model_out /* [nloc][nE] or NULL */; double* total /* [nloc] */;
  nh_hs_blob blobs[NH_HS_MAX_BLOB]; int nblobs;
  /* do_accept = 0 (sharded loop) with blobs: total[] is an exchange buffer of rows of
   * send_width doubles, row j = { lnprob | blob 0 | blob 1 ... } of walker j: ONE all-gather
   * per half-step carries the log-probabilities and the blobs; nh_move_accept_rows takes the
   * gathered rows.  0: total[] holds the log-probabilities only. */
  int send_width;
} nh_hs_desc;
typedef struct nh_halfstep_plan nh_halfstep_plan;
int nh_half_step_create(nh_ctx* ctx, const nh_hs_desc* desc /*host*/, nh_halfstep_plan** out);
int nh_half_step_begin_block(nh_ctx* ctx, nh_halfstep_plan* plan, int first_slice,
                             int steps_before);
/* slice >= 0: the launch works on that slice of the block of moves (a captured graph replays
 * it for the same slice); slice < 0: the slice the plan's own launch counter says is next */
int nh_half_step_launch(nh_ctx* ctx, nh_halfstep_plan* plan, int slice);
/* Which launches of a half-step open and close a span of the context's device clock
 * (nh_clock_read).  Default: every launch of the plan is a span by itself.  A half-step of
 * several launches -- a model that asks for its synchrotron spectrum twice with the SSC seed
 * integral in between, examples/CrabNebula_SynSSC.py:29-45 -- opens with its first launch
 * (1, 0) and closes with its last (0, 1). */
int nh_half_step_span(nh_halfstep_plan* plan, int open, int close);
int nh_half_step_info(const nh_halfstep_plan* plan, int* threads, int* blocks,
                      long long* lds_bytes);
/* workgroups per walker of the plan's launches: 1, or K = 2, 4, 8 where a launch holds fewer
 * walkers than the device has compute units and the model's work items are most of a launch
 * (each of the K workgroups repeats the prologue and takes every K-th work item; the last to
 * arrive sums the partial spectra in index order and evaluates the likelihood: the results do
 * not depend on arrival order).  NH_HS_SPLIT=<K> in the environment caps K (1: never split). */
int nh_half_step_split(const nh_halfstep_plan* plan, int* split);
/* How the plan's launches integrate the synchrotron component (radiative.py:282-342): *form = 0 no
 * such component, 1 the direct form (nh_syn.h), 2 the log-domain form on the grid's comb
 * (nh_syn2.h: a log-uniform particle grid whose table fits in LDS beside the model's). */
int nh_half_step_syn_form(const nh_halfstep_plan* plan, int* form);
/* NaN log-probabilities the accepts of the separate kernels (nh_lnprob / ..._lnprob with a move,
 * nh_move_accept, nh_move_accept_rows) have met since the last reset: emcee raises
 * ValueError("Probability function returned NaN") at the first one (EnsembleSampler.
 * compute_log_prob; reference call site core.py:128); a launch rejects the proposal -- NaN
 * compares false -- and counts.  The one-launch kernels count per plan (below). */
int nh_nan_count(nh_ctx* ctx, int reset, int* count);
/* ... and the proposals the same accepts found forbidden by the prior (their log-probability is
 * the prior's -inf), counted the same way. */
int nh_forbidden_count(nh_ctx* ctx, int reset, int* count);
/* The device span clock: what the step loop's launches -- the kernels that replace emcee's
 * EnsembleSampler.sample loop around core.py:97-121 (reference call sites core.py:128, 450-457)
 * -- have spent ON the device since the last reset, measured on those launches themselves: the
 * first workgroup of a span's first kernel stamps the GPU's constant-rate wall clock, the last
 * workgroup out of the span's last kernel adds the difference (a span = one launch of the
 * resident loop with its epilogue, or the launches of one half-step of the per-launch loop).
 * out[3] = { ticks inside closed spans, closed spans, ticks per millisecond }.  Spans lie inside
 * the host interval around their launch calls and do not overlap, so (host time of a region) -
 * (span time) >= 0 by construction: bench.py's region_overhead_us.  Synchronises the stream;
 * reading adds nothing to any launch. */
int nh_clock_read(nh_ctx* ctx, int reset, long long* out);
/* proposals whose log-probability was NaN since the plan was created (or the last reset):
 * emcee raises ValueError("Probability function returned NaN") on the first one
 * (EnsembleSampler.compute_log_prob; reference call site core.py:128), a launch rejects the
 * proposal and counts it here for the caller to act on.  Synchronises the stream. */
int nh_half_step_nan_count(nh_ctx* ctx, nh_halfstep_plan* plan, int reset, int* count);
/* The same with, beside it, the proposals the prior forbade (core.py:99-101, 115-119: the
 * launch evaluates none of their integrals; the reference evaluates the model and discards the
 * result).  A negative *nan / *forbidden on entry SETS that counter to -value - 1 first (a
 * replayed block of moves must not count its proposals twice). */
int nh_half_step_counts(nh_ctx* ctx, nh_halfstep_plan* plan, int reset, int* nan, int* forbidden);
int nh_half_step_destroy(nh_ctx* ctx, nh_halfstep_plan* plan);

/* ---- a whole block of moves in ONE launch: the half-step kernel with resident workgroups ----
 * Replaces the sequence of nh_half_step_launch calls for slices [slice0, slice0 + nslices) of
 * the block of moves in `blk` (whole ensemble steps: slice0 and nslices even, at most 32 steps)
 * -- emcee's EnsembleSampler.sample loop over StretchMove / RedBlueMove.propose around
 * core.py:97-121 (reference call sites core.py:128, 450-457).  The workgroups stay resident
 * for the whole launch; the ensemble-wide barrier between half-steps becomes a per-walker
 * hand-off: a walker of slice h + 1 waits only for its own and its partner's record of the
 * previous slices (data-tagged 8-byte granules written write-through by the workgroup that
 * moved the walker; see nh_persist.hip).  Everything walker-independent (grid nodes, table
 * of exponentials, data columns, priors) is loaded into LDS once per launch.
 * Needs a plan with do_accept = 1, one workgroup per walker, lo = 0, nloc = ns, ndim <= 15, no
 * separately evaluated prior (lp == NULL) and every likelihood component produced inside the
 * launch; nh_half_step_run_create says no otherwise (the caller keeps launching per half-step).
 * The launch reads coords / logp as they are and leaves them at the state after the last
 * slice; naccepted is advanced; the spectra / weights / parameter-row outputs of the plan's
 * descriptor are NOT written.  Chain history: hist_coords [cap][N][ndim], hist_logp [cap][N]
 * and hist_blobs[b] [cap][N][m_b] (device; hist_coords NULL: none kept) receive rows hist_row0,
 * hist_row0 + 1, ... for the steps of the launch; the blobs' current values (blobs[].cur) end at
 * the last step's.  A launch whose workgroups cannot all be resident would wait for ever: the
 * grid is sized by the occupancy query, every wait is bounded, and a time-out aborts the
 * launch and latches an error that nh_half_step_run_status reports (0 = every launch so far
 * found its records). */
typedef struct nh_halfstep_run nh_halfstep_run;
int nh_half_step_run_create(nh_ctx* ctx, nh_halfstep_plan* plan, nh_halfstep_run** out);
int nh_half_step_run(nh_ctx* ctx, nh_halfstep_plan* plan, nh_halfstep_run* run, int slice0,
                     int nslices, double* hist_coords, double* hist_logp,
                     double* const* hist_blobs /*host array of device pointers, or NULL*/,
                     long long hist_row0, long long hist_cap);
int nh_half_step_run_status(nh_ctx* ctx, nh_halfstep_run* run, int* status);
/* What launch number `launch` of the loop (1, 2, ...) left behind, read from page-locked host
 * memory its epilogue wrote -- no stream operation, no synchronisation: *done = 0 while it has not
 * ended (wait != 0: sleeps until it has), else its status (0 = it found every record; -1 = the
 * report has been overwritten: only the last two launches have one) and the plan's counters of
 * NaN log-probabilities and of proposals the prior forbids (core.py:99-119) as they stood behind
 * it.  The sampler queues launch n + 1 only once launch n - 1 is known to have ended well, so a
 * launch that gave up costs the replay of two blocks of moves at most.  One-GPU loops only. */
int nh_half_step_run_report(nh_ctx* ctx, nh_halfstep_run* run, int launch, int wait, int* done,
                            int* status, int* nan_count, int* forbidden,
                            int* before /*[2]: the two counters as the launch found them, or NULL*/);
/* The resident loop's own copies of the plan's emission tables with their columns SORTED by the
 * first grid row in which they are non-zero (an inverse-Compton or pi0 table is zero below the
 * kinematic threshold gamma = E / mec2, Ep = E ...: rows that contribute exact zeros to
 * trapz_loglog, utils.py:347-348).  kds[t] (device): the interleaved table [nG][nK][2] of plan
 * table t with permuted columns (nh_table_interleave of the permuted Kt / dlnKt), followed by a
 * trailer of ints { row0[8] | perm[nK] }: row0[tile] = first row in which any of the tile's 64
 * columns is non-zero (segments below it are not walked), perm[p] = the column of the spectrum
 * that position p holds.  NULL keeps the plan's table.  The caller keeps the buffers alive.  The
 * trailers are read back and checked (rows in range, the column order a permutation). */
int nh_half_step_run_tables(nh_ctx* ctx, nh_halfstep_plan* plan, nh_halfstep_run* run,
                            const double* const* kds /*host*/, int ntab);
/* ---- the resident loop over an ensemble SHARED by the GPUs of a node (2 .. 8 ranks, one process
 * per GPU).  Replaces, for walkers sharded as in the per-launch loop (rank r proposes positions
 * [lo, lo + nloc) of every half-step; the reference's analogue is Pool(threads) over a fixed
 * ensemble, core.py:446-457), the all-gather between the launches of a half-step: a mover stores
 * its walker's record into EVERY rank's ring (system-scope stores; xGMI for the others), consumers
 * poll their local ring as on one GPU.  No collective and no launch per half-step.
 *   create_shared: plan with lo / nloc = this rank's block (do_accept not needed), rings in
 *                  fine-grained device memory;
 *   export / attach: the 64-byte hipIpc handle of a rank's rings, to be carried to every other
 *                  rank by the caller's control plane and attached there (all before the first run);
 *   probe:         `rounds` tagged exchanges with every peer inside ONE launch -- status 0 only if
 *                  stores another GPU makes while the kernel runs reach its polling loads (call on
 *                  every rank at the same time; bounded like every wait of the loop);
 *   hist_flags:    where nh_half_step_run keeps who-moved-what of the following launches,
 *                  [hist_cap][N] ints, rows hist_row0 ... of every launch: -1 = another rank
 *                  moved the walker in that step, 0 / 1 = this rank did and rejected / accepted
 *                  (history rows and blobs are written by the mover only, on its own GPU; blob
 *                  rows of rejected moves are NOT filled);
 *   counters:      nacc_own[N] (moves this rank accepted; the plan's naccepted is not touched) and
 *                  curstamp[N] (-1, or the step count at which this rank last accepted a move of
 *                  the walker: whoever holds the largest stamp holds the walker's current blobs in
 *                  its blobs[].cur); reset bit 0 / 1 clears the first / second afterwards.
 * After a shared launch coords / logp hold the whole ensemble on every rank. */
int nh_half_step_run_create_shared(nh_ctx* ctx, nh_halfstep_plan* plan, int rank, int nrank,
                                   nh_halfstep_run** out);
int nh_half_step_run_export(nh_ctx* ctx, nh_halfstep_run* run, void* handle64);
int nh_half_step_run_attach(nh_ctx* ctx, nh_halfstep_run* run, int peer, const void* handle64);
int nh_half_step_run_probe(nh_ctx* ctx, nh_halfstep_run* run, int rounds, int* status,
                           double* us_per_round);
int nh_half_step_run_hist_flags(nh_halfstep_run* run, int* flags);
int nh_half_step_run_counters(nh_ctx* ctx, nh_halfstep_run* run, int* nacc_own, int* curstamp,
                              int reset);
int nh_half_step_run_info(const nh_halfstep_run* run, int* grid, int* threads,
                          long long* lds_bytes);
/* How the loop evaluates Synchrotron._spectrum's integrand (radiative.py:300-340): mode 1 = in
 * the log domain on the grid's comb (csrc/nh_syn2.h: one exponent per node, ln Gtilde from a
 * table of `pieces` degree-5 pieces of `nodes_per_piece` grid steps; taken when the particle
 * grid is log-uniform, as radiative.py:147-154 makes it), 0 = the direct form (any grid; no
 * synchrotron component). */
int nh_half_step_run_syn_info(const nh_halfstep_run* run, int* mode, int* nodes_per_piece, int* pieces);
/* Where the loop's table work items (the trapz_loglog over the particle grid of radiative.py:684,
 * 1534-1536) read their rows: in_registers = 1 when the loop runs the instance of a table-only
 * model whose items keep their rows of {K, dlnK} in vector registers for the whole launch
 * (workgroups of 512 threads; an emission table does not depend on the walker), `nodes_max` the
 * rows per lane that instance can hold; 0 = streamed from the L2s every half-step. */
/* workgroups per walker of the resident loop's launches (the plan's split) and whether they
 * divide the grid's ROWS between them (table-only models: core.py:450-457's one evaluation per
 * walker on two compute units, each with half of radiative.py:1495-1536's proton grid) */
int nh_half_step_run_split_info(const nh_halfstep_run* run, int* split, int* rows);
/* *deep = 1 when the loop's launches keep TWO walkers of a workgroup in flight (ensembles of more
 * walkers per half-step than resident workgroups: a workgroup's next walker has its records,
 * proposal and parameter packs made while the current one's work items run, and its weights
 * start while the current one's likelihood -- core.py:64-121 -- is still being summed) */
int nh_half_step_run_pipeline_info(const nh_halfstep_run* run, int* deep);
int nh_half_step_run_table_info(const nh_halfstep_run* run, int* in_registers, int* nodes_max);
/* NH_HS_DEBUG=1: out[256][64][8] wall-clock stamps (100 MHz) of the last launch, per
 * (workgroup, slice handled): start | records in | packs done | weights done | own items
 * done | all items done | spectra summed | record published; then [64][4][16]: for workgroup
 * 0, per slice handled, when each of its waves reached barrier 1 | 2 | 3 (| unused) */
int nh_half_step_run_stamps(nh_ctx* ctx, const nh_halfstep_run* run, long long* out);
int nh_half_step_run_destroy(nh_ctx* ctx, nh_halfstep_run* run);
/* diagnostics (plans created under NH_HS_DEBUG=1): per-phase 100 MHz wall-clock stamps of the
 * first 8 workgroups of the last launch, out[8][16], followed by 4 x 16 per-wave figures of
 * workgroup 0, then start[1024] and end[1024] stamps of every workgroup (2304 values in all);
 * all zero otherwise */
int nh_half_step_stamps(nh_ctx* ctx, const nh_halfstep_plan* plan, long long* out);
/* row `row` (-1: hist->n - 1) of the device-resident history := coords[N][ndim] / logp[N] */
int nh_hist_append(nh_ctx* ctx, const double* coords, const double* logp, long long N, int ndim,
                   const nh_hist* hist /*device*/, long long row);
/* the same for the blobs a half-step plan keeps: row `row` of every blob history := cur */
int nh_half_step_append_blobs(nh_ctx* ctx, const nh_halfstep_plan* plan, long long row);

/* host-side generator of the move's random numbers: a worker thread fills a ring of
 * (page-locked) blocks ahead of the consumer, in exactly the slice layout above.  The
 * stream (xoshiro256** from `seed`; per step: permutation, z, partners, ln U') does not
 * depend on how many steps are taken at once, nor on the rank. */
typedef struct nh_moves nh_moves;
int nh_moves_create(unsigned long long seed, int N, double a, int ksteps_per_block, int depth,
                    int pinned, nh_moves** out);
/* k independent ensembles of n walkers each as ONE stream of N = k*n walkers (ns = k*n/2): k
 * generator states, state r seeded as nh_moves_create(seeds[r], n, ...) seeds its own.  Per
 * ensemble step every ensemble r runs the recipe above on its own state with N = n and writes its
 * n/2 entries at [r*n/2, (r+1)*n/2) of z, ln U', S and partner of both slices, r*n added to S and
 * partner.  Ensemble r's sub-stream is therefore bit for bit the stream of
 * nh_moves_create(seeds[r], n, a, ...) apart from that offset; walkers [r*n, (r+1)*n) form
 * ensemble r, and every partner lies in the inactive half of its own ensemble.  k == 1 is
 * nh_moves_create's stream.  seeds is a HOST array of k values, read during the call only.
 * NH_EINVAL: k < 1, n odd or < 2, k*n beyond an int, a null seeds or out, a <= 1, depth < 3. */
int nh_moves_create_ensembles(const unsigned long long* seeds /*host*/, int k, int n, double a,
                              int ksteps_per_block, int depth, int pinned, nh_moves** out);
/* both kinds of stream: up to `want` consecutive steps, contiguous in host memory (2*got slices); depth >= 3.
 * A used-up block goes back to the producer one block late: an asynchronous copy out of
 * the MOST RECENT take may still be pending at the next take, all earlier ones must be done. */
int nh_moves_take(nh_moves* m, int want, const void** host_ptr, int* got);
int nh_moves_destroy(nh_moves* m);

/* capture everything launched on the context's stream into a hipGraph, replay it */
int nh_graph_begin(nh_ctx* ctx);
int nh_graph_end(nh_ctx* ctx, void** graph_exec_out);
int nh_graph_launch(nh_ctx* ctx, void* graph_exec);
int nh_graph_destroy(nh_ctx* ctx, void* graph_exec);

/* ---- multi-GPU: one all-gather per half-step -------------- */
#define NH_UNIQUE_ID_BYTES 128
/* NH_OK when librccl could be loaded and every entry point resolved (no communicator is made).
 * Every rank asks this first and the answers are min-reduced over the control plane, so that no
 * rank enters the blocking ncclCommInitRank while another one never will. */
int nh_comm_available(void);
int nh_comm_unique_id(char* id_out /*[NH_UNIQUE_ID_BYTES]*/);
int nh_comm_init(nh_ctx* ctx, int rank, int nranks, const char* id);
int nh_comm_destroy(nh_ctx* ctx);
/* what the live communicator says of itself (ncclCommCount, ncclCommUserRank, ncclCommCuDevice):
 * the workers the reference's Pool(threads) would report, core.py:446-457 */
int nh_comm_info(nh_ctx* ctx, int* nranks, int* rank, int* device);
/* recv[r*count .. (r+1)*count) = send of rank r (device buffers, float64 count) */
int nh_comm_allgather(nh_ctx* ctx, const double* send, double* recv, long long count);

/* ---- posterior bands: exact per-column order statistics (plot.py:438-501) -------------------
 * out[r][c] = np.sort(x[0:M, c])[ranks[r]] for c < ncol, r < R: the confidence bands of naima's
 * _calc_CI (np.sort(model[:, i])[nf] per energy i) over the samples of a chain's blobs or of model
 * evaluations at drawn parameters.  x is a row-major DEVICE matrix [M][ld] (samples x energies,
 * the layout of stored blobs and of a dense model output), ranks a HOST array of R <= 16 ranks in
 * [0, M), out a device [R][ncol].  Exact (an MSD radix select on order-preserving 64-bit keys,
 * integer atomics only); NaNs rank after +inf as in NumPy, -0.0 and +0.0 as equals.  Stream-ordered
 * on the context's stream, no host synchronisation; library scratch of 8*M*ncol bytes + a little.
 * NH_EINVAL: M == 0, M >= 2^31, ncol > ld, R outside [1, 16] or a rank outside [0, M). */
#define NH_SELECT_MAX_RANKS 16
int nh_column_select(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                     const int* ranks /*host*/, int R, double* out);

/* ---- integrated autocorrelation time (emcee.autocorr.integrated_time) ----------------------
 * The walker-averaged normalised autocorrelation function of one dimension of a chain, emcee's
 * function_1d of every walker's series averaged over the walkers; the window search and the
 * tolerance check stay on the host.  Deterministic (no floating-point atomics: the order of every
 * sum is fixed by the shapes), 64-bit indices, stream-ordered on the context's stream, no host
 * synchronisation; library scratch of a few MiB at most.
 * nh_autocorr_prep: x is a row-major DEVICE matrix [n_t][n_w*n_d] (get_chain's layout: column
 *   w*n_d + d is walker w's series of dimension d).  Writes the centred series of dimension d,
 *   z[w][t] = x[t][w*n_d+d] - mean_t, into the device matrix z [n_w][n_t] (contiguous in t) and
 *   s2[w] = sum_t z[w][t]^2 into the device array s2 [n_w].  A series whose values are all equal
 *   gets z = 0 and s2 = 0 exactly; a non-finite value makes its s2 non-finite.
 *   NH_EINVAL: n_t, n_w or n_d not positive, d outside [0, n_d).
 * nh_autocorr_lags: f[k] = (1/n_w) sum_w (sum_{t < n_t-tau} z[w][t] z[w][t+tau]) / s2[w] for
 *   tau = lag0 + k, k < nlags, from nh_autocorr_prep's z and s2 (every s2[w] positive and finite:
 *   the host leaves a dimension with a zero or non-finite one out, as NaN); f is a device [nlags].
 *   NH_EINVAL: n_t, n_w or nlags not positive, lags outside [0, n_t). */
int nh_autocorr_prep(nh_ctx* ctx, const double* x, long long n_t, int n_w, int n_d, int d,
                     double* z, double* s2);
int nh_autocorr_lags(nh_ctx* ctx, const double* z, const double* s2, long long n_t, int n_w,
                     long long lag0, int nlags, double* f);

/* ---- the same function of a chain that is still growing: running lag sums --------------------
 * x is a row-major DEVICE block [rows][n_w*n_d] whose rows [row_start, n) hold a chain so far (a
 * history block of the device loop).  With y = x - pivot (a series' value in row row_start) the
 * state holds S[col][k] = sum_{t >= row_start + k} y[t] y[t-k] for k < L (DEVICE [n_w*n_d][L]),
 * stats = {sum of y, min y, max y} (DEVICE [3][n_w*n_d]) and pivot (DEVICE [n_w*n_d]); the caller
 * owns the three arrays and need not initialise them.  Same conventions as above (no floating-
 * point atomics, 64-bit indices, the context's stream, no host synchronisation).
 * nh_acf_accumulate: adds rows [n0, n1) to the state; n0 == row_start starts it (nothing of it is
 *   read); otherwise the state must hold rows [row_start, n0).  Reads at most 255 + L rows before
 *   n0, copies nothing.  Every sum is one chain in the order of the rows: the state after rows
 *   [a, b) is bit-identical however [a, b) was cut into calls.  n0 == n1: nothing is launched.
 *   NH_EINVAL: n_w, n_d or L not positive, not 0 <= row_start <= n0 <= n1 <= rows.
 * nh_acf_finalize: f (DEVICE [n_d][L]) from the state of rows [row_start, n): f[d][k] = the mean
 *   over walkers of c_k / c_0 for k < min(L, n - row_start), NaN behind that, with
 *   c_k = S_k - m ((T - P_k) + (T - Q_k)) + (n - row_start - k) m^2, m = T / (n - row_start), and
 *   P_k / Q_k the sums of the first / last k values of y, read from the block: emcee's function_1d
 *   per walker, averaged, as nh_autocorr_lags gives it.  A walker whose series is constant or
 *   holds a non-finite value makes its dimension NaN.  Library scratch of 8*n_w*n_d*L bytes.
 *   NH_EINVAL: n_w, n_d or L not positive, not 0 <= row_start < n <= rows. */
int nh_acf_accumulate(nh_ctx* ctx, const double* x, long long rows, int n_w, int n_d,
                      long long row_start, long long n0, long long n1, int L, double* pivot,
                      double* S, double* stats);
int nh_acf_finalize(nh_ctx* ctx, const double* x, long long rows, int n_w, int n_d,
                    long long row_start, long long n, int L, const double* pivot, const double* S,
                    const double* stats, double* f);

/* ---- EBL absorption with a per-walker redshift (models.py:470-552) ------------------------
 * The reference picks the nearest of the tabulated redshifts zl = arange(0.01, 4, 0.01)
 * (models.py:520-528, no interpolation in z), clips log tau at 150 (models.py:529-531) and
 * interpolates log10(tau) in log10(E) with interp1d(kind="cubic") (models.py:445-466).  At fixed energies
 * the transmission is therefore a walker-independent table Tab[ncol+1][nE]: row 0 is z < 0.01
 * (models.py:532-536), row c+1 is column c.  Deterministic, no atomics, no scratch.
 * nh_ebl_table: knots[nt] and coef[nt-4][ncol] (DEVICE) are the cubic B-spline of every column
 *   (scipy make_interp_spline, k = 3); x[nE] = log10(E/eV) and code[nE] (DEVICE) the host's
 *   per-energy decisions: code & 3 = NH_EBL_ONE below 1 GeV (transmission 1), NH_EBL_HIGH
 *   above 100 TeV (transmission t_hi = exp(-log10(6000))), models.py:542-552;
 *   code & NH_EBL_OUTSIDE: outside the table (interp1d's fill value -inf).  Writes
 *   P[r][k] = 10**S_r(x_k) (TableModel.__call__) and T[r][k] = exp(-log10(P[r][k])) or the
 *   branch value (transmission); either may be NULL, not both.
 * nh_ebl_apply: out[w*ldo+k] = Tab[row(z_w)][k] * colfac[k] * sum_j comps[j] (ncomp 0..8; no
 *   terms: the row itself; colfac may be NULL), z a lazy per-walker redshift, zl[nzl] (DEVICE)
 *   the tabulated redshifts, nrows = nzl + 1.  row(z) = 0 for 0 <= z < 0.01, else
 *   1 + argmin_i |zl[i] - z| (first index on a tie); z < 0, NaN or +-inf gives a NaN row. */
enum { NH_EBL_ONE = 1, NH_EBL_HIGH = 2, NH_EBL_OUTSIDE = 4 };
int nh_ebl_table(nh_ctx* ctx, const double* knots, int nt, const double* coef, int ncol,
                 const double* x, const int* code, int nE, double t_hi, double* T, double* P);
int nh_ebl_apply(nh_ctx* ctx, const double* tab, int ldt, int nrows, const double* zl, int nzl,
                 const nh_lazy* z /*host*/, const nh_comp* comps /*host*/, int ncomp,
                 const double* colfac, int N, int m, double* out, int ldo);

/* ---- gamma-gamma pair-production absorption on photon fields, per walker ---------------------
 * (new: the reference has none.)  Breit-Wheeler cross section on the seed-photon-field grammar of
 * InverseCompton; tau(E) = sum over fields of L_f * a_f * kappa_f(E).  FP64, deterministic, no
 * atomics, no scratch.
 * nh_pairabs_rows: out[r*ldo+k] = kappa of ONE field at x[k] = E_k / (m_e c^2) (DEVICE), one
 *   wave per (row, energy), a fixed composite Gauss-Legendre rule in t, s = cosh^2 t:
 *   NH_PAIR_THERMAL  per dilution factor w = u / (a T^4), 1/cm: T_K (and theta, rad; NULL =
 *                    isotropic) are lazy values evaluated at the ROW index, so nrows = 1 with
 *                    constants is the row all walkers share and nrows = N one row per walker;
 *                    k_to_mec2 = k_B / (m_e c^2) per kelvin.  T <= 0, NaN or inf: a NaN row.
 *   NH_PAIR_MONO     per photon, cm^2: seed_E_eV[1] (DEVICE), sbar(E E0 / m^2)
 *   NH_PAIR_TABLE    the opacity itself, 1/cm: trapz_loglog over the ns >= 2 nodes seed_E_eV[ns]
 *                    (eV), seed_dens[ns] (1/(eV cm3)) (DEVICE) of dens_i * sbar(E E_i / m^2)
 *   With theta the field comes from one direction: (1 - cos theta) sigma(E eps (1 - cos theta) /
 *   (2 m^2)) replaces sbar; theta = 0 gives 0 and -theta the bits of theta.
 * nh_pairabs_apply: out[w*ldo+k] = exp(-tau_w[k]) * colfac[k] * sum_j comps[j] (ncomp 0..8; no
 *   terms: the transmission itself; write_tau: tau itself, which takes no terms and no colfac),
 *   tau_w[k] = sum_f L_f(w) a_f(w) kappa_f[w*ld_f + k] added in the order given (ld_f = 0: the
 *   shared row).  a_f = dens (photons/cm3, or 1), or for a thermal field dens / (a_rad T_K^4) with
 *   dens in erg/cm3.  A walker with L or dens negative, NaN or +-inf, or a thermal field's T <= 0,
 *   NaN or inf, gets a NaN row; L = 0 or dens = 0 gives exactly 1. */
enum { NH_PAIR_THERMAL = 0, NH_PAIR_MONO = 1, NH_PAIR_TABLE = 2 };
typedef struct { const double* kappa; long long ld; nh_lazy L_cm; nh_lazy dens; nh_lazy T_K;
                 int thermal; int pad; } nh_pair_field;
int nh_pairabs_rows(nh_ctx* ctx, int kind, double k_to_mec2, const nh_lazy* T_K /*host*/,
                    const nh_lazy* theta /*host or NULL*/, const double* seed_E_eV,
                    const double* seed_dens, int ns, const double* x, int nE, int nrows,
                    double* out, int ldo);
int nh_pairabs_apply(nh_ctx* ctx, const nh_pair_field* fields /*host*/, int nfields /* <= 8 */,
                     const nh_comp* comps /*host*/, int ncomp, const double* colfac, int write_tau,
                     int N, int m, double* out, int ldo);

/* ---- synchrotron self-absorption of a homogeneous one-zone source, per walker ----------------
 * (new: the reference has none.)  For N(gamma) particles per unit Lorentz factor in a volume V,
 *   alpha(E) V = kappa(E) = pi^2 hbar^3 CS1(E) / (m_e E) trapz_loglog((N/gamma) H(x), gamma)
 *   H = 2 Gtilde(x) (1 - dln Gtilde / dln x),  x = E / Ec(gamma, B)
 * (the form integrated by parts: no derivative of N, non-negative node by node) with CS1, Ec and
 * Gtilde those of nh_synchrotron.  FP64, deterministic, no atomics, no scratch.
 * nh_syn_absorption: out[w*ldo+k] = kappa_w(E_eV[k]) in cm^2.  The arguments, the refusals and
 *   the rules of nh_synchrotron: a zero node kills its segments, a NaN weight in an energy's live
 *   range makes it NaN, a node with x > 746 is dead, B <= 0, NaN or +-inf gives a NaN row.  A
 *   kernel of its own at the launch shape nh_synchrotron_plan gives without the epilogue, which
 *   nh_syn_absorption_plan reports.
 * nh_ssa_apply: out[w*ldo+k] = f(tau_w[k]) * colfac[k] * sum_j comps[j] (ncomp 0..8; no terms:
 *   the escape fraction itself; write_tau: tau itself, which takes no terms and no colfac) from
 *   kappa[w*ldk + k] (ldk = 0: one shared row) and the lazy radius R_cm(w):
 *   NH_SSA_SPHERE  tau = 3 kappa / (2 pi R^2) along a diameter, f = 3 u / tau,
 *                  u = 1/2 + exp(-tau)/tau - (1 - exp(-tau))/tau^2 (Gould 1979); below tau = 1 the
 *                  series 1 - 3 tau/8 + tau^2/10 - ... (20 terms)
 *   NH_SSA_SLAB    a face-on cylinder of face radius R: tau = kappa / (pi R^2), f = -expm1(-tau)/tau
 *   kappa = 0 gives exactly 1, a NaN kappa NaN; a walker with R <= 0, NaN or +-inf a NaN row. */
enum { NH_SSA_SPHERE = 0, NH_SSA_SLAB = 1 };
int nh_syn_absorption(nh_ctx* ctx, const double* w, const double* dlw, const double* B_G, int ldB,
                      int N, const double* gam, const double* lx, int nG,
                      const double* E_eV, int nE, double* out, int ldo);
int nh_syn_absorption_plan(int N, int nG, int nE, int* C, int* tw, int* ktiles, int* lds_bytes);
int nh_ssa_apply(nh_ctx* ctx, const double* kappa, long long ldk, const nh_lazy* R_cm /*host*/,
                 int geometry, const nh_comp* comps /*host*/, int ncomp, const double* colfac,
                 int write_tau, int N, int m, double* out, int ldo);

/* ---- cooled electron populations, per walker -------------------------------------------------
 * (new: the reference has none.)  An injection rate Q(E) [1/(eV s)] switched on for age_s under
 * the loss rate b(E) = (4/3) sigma_T c (B^2/8 pi) gamma^2 + sum_f u_f loss_f(E) [eV/s] leaves
 *   n(E_i) = int_{E_i}^{E*} Q dE / b(E_i),  int_{E_i}^{E*} dE / b = age  (E* = E_max if never),
 * in the power-law-per-segment picture of trapz_loglog on the grid e_eV[nC] (DEVICE, ascending):
 * suffix sums of the segment terms, E* and the partial integral of Q by the segment's closed
 * forms (log branch for |slope + 1| <= 1e-10, a zero node ends a segment).  Injection above
 * e_eV[nC-1] is ignored.  FP64, the same bits at every call.
 * nh_cooled_electrons: n_out[w*nC + i], one workgroup per walker.  Q[w*ldq + i] (DEVICE), ldq = 0:
 *   one row for all walkers.  B_G (gauss), age_s (s; +inf: the steady state) and u[nf] (erg/cm3)
 *   are lazy per-walker values (host structs).  loss[f*nC + i] (DEVICE): eV/s per erg/cm3 of
 *   field f at node i; nf <= 8.  A walker with age <= 0 or NaN, B NaN or +-inf, a u that is
 *   negative, NaN or inf, B <= 0 and no positive u, or b not positive and finite at every node
 *   gets a NaN row and adds 1 to status[0] (DEVICE int).  Q == 0 gives exact zeros.
 *   EINVAL: nC outside 2..2048 (40 B of LDS per node), nf outside 0..8, 0 < ldq < nC.
 *   N = 0 is no error.
 * nh_cooled_weights: the rows n[N][nC] on the grid e_c[nC] resampled at e_eV[nG] by log-log
 *   linear interpolation: w[w*nG + g] = xg[g] * unit_scale * n(e_eV[g]) and dlw[g] =
 *   ln|w[g+1]/w[g]| (dlw[nG-1] = 0), the inputs of nh_integrate_tables and nh_synchrotron.
 *   Exactly 0 outside [e_c[0], e_c[nC-1]] and inside a segment with a zero node; a target node
 *   that IS a grid node takes its value unchanged; dlw = 1e300 where w[g] or w[g+1] is zero or the
 *   ratio is not finite.
 * nh_cooled_ic_rows: Kt[i*ld + k] = the isotropic Khangulyan+14 kernel (Eq. 14, what
 *   nh_table_ic_planck tabulates) of the electron gam[i] on a Planck field of T_K at the outgoing
 *   photon energy gam[i] * z[k] (in m_e c^2; z[nE], gam[nC] DEVICE): every electron on its own
 *   photon grid, one launch.  trapz_loglog of z K over z, times gam^2 m_e c^2 [eV] / (a_rad T^4),
 *   is the loss rate per unit energy density that nh_cooled_electrons takes as `loss`.
 *   EINVAL: T_K <= 0, ld < nE. */
int nh_cooled_ic_rows(nh_ctx* ctx, const double* gam, int nC, const double* z, int nE, double T_K,
                      double* Kt, int ld);
int nh_cooled_electrons(nh_ctx* ctx, const double* Q, long long ldq, int N, const double* e_eV,
                        int nC, const nh_lazy* B_G /*host*/, const double* loss, int nf,
                        const nh_lazy* u /*host [nf]*/, const nh_lazy* age_s /*host*/,
                        double* n_out, int* status);
int nh_cooled_weights(nh_ctx* ctx, const double* n, const double* e_c, int nC, int N,
                      const double* e_eV, const double* xg, int nG, double unit_scale, double* w,
                      double* dlw);

/* ---- thinning a chain history on the device (emcee's thin_by) -------------------------------
 * For every segment (row-major DEVICE matrices of doubles, `width` columns each):
 *   dst row (dst_row0 + k) := src row (first + k*stride),  k < nrows.
 * One launch for all segments: the chain, the log-probability and every blob history of a chunk
 * of steps.  A plain copy (16-byte accesses where a segment's width is even and both its bases
 * are 16-byte aligned, else 8-byte ones), stream-ordered on the context's stream, no host
 * synchronisation, no scratch.  Rows are copied in parallel, so the bytes read and the bytes
 * written must not overlap (an in-place compaction would race).  nrows == 0: nothing is launched.
 * NH_EINVAL: nsegs outside [1, 8], stride < 1, first, nrows or dst_row0 negative, a null or
 *   misaligned segment, a width < 1, source and destination rows that overlap. */
typedef struct { const double* src; double* dst; long long width; } nh_thin_seg;
int nh_hist_thin(nh_ctx* ctx, const nh_thin_seg* segs /*host*/, int nsegs /* <= 8 */,
                 long long first, long long stride, long long nrows, long long dst_row0);

/* ---- posterior panels and a corner plot: column reductions over a chain ----------------------
 * What np.histogram, np.histogram2d and scipy.stats.gaussian_kde compute on the host for naima's
 * posterior panels (plot_chain, plot_distribution) and for a corner figure.  x is a row-major DEVICE matrix
 * [M][ld] with ncol <= ld columns in use (get_chain(flat=True), stored scalar blobs).  Stream-
 * ordered on the context's stream, no host synchronisation, library scratch, 64-bit row indices.
 * Deterministic: integer atomics only; every floating-point sum has an order fixed by the shapes.
 * Every entry point: NH_EINVAL for M == 0, ncol < 1, ncol > ld or a null argument.
 * nh_column_moments: counts (DEVICE int64 [2][ncol]) = the number of finite values, of NaNs;
 *   stats (DEVICE [4][ncol]) = min, max, mean and unbiased variance (ddof = 1) of the finite
 *   values, two passes (the mean, then sum (x - mean)^2).  Non-finite values are counted and
 *   otherwise left out.  A column whose finite values are all equal has that value as its mean
 *   and variance exactly 0; without a finite value min, max and mean are NaN, with fewer than two
 *   the variance is.
 * nh_hist_columns: edges is a DEVICE [ncol][nb+1] of increasing edges per column, evenly spaced
 *   to within rounding (np.linspace); pairs a HOST [npairs][2] of column pairs (i, j), NULL when
 *   npairs == 0.  h1 (DEVICE int64 [ncol][nb]) = the counts of every column, h2 (DEVICE int64
 *   [npairs][nb][nb], NULL when npairs == 0) = h2[p][a][b] with a the bin of column i.  A value v
 *   is in bin k iff edges[k] <= v < edges[k+1]; v == edges[nb] counts in bin nb-1; values outside
 *   [edges[0], edges[nb]], NaN and +-inf are dropped, a pair entry if either coordinate is (the
 *   rule of np.histogram(range=) and of np.histogram2d(bins=[e_i, e_j])).  The bin is estimated
 *   arithmetically and corrected against the edges.
 *   NH_EINVAL also: ncol > NH_HIST_MAX_COLS, nb < 1, nb > NH_HIST_MAX_BINS_1D, nb >
 *   NH_HIST_MAX_BINS_2D with pairs, npairs outside [0, NH_HIST_MAX_PAIRS], a pair index outside
 *   [0, ncol).
 * nh_kde_columns: out[c][g] = 1/(n_c h_c sqrt(2 pi)) sum_m exp(-((p[c][g] - x[m][c])/h_c)^2 / 2)
 *   over the n_c finite values of column c; points p and out are DEVICE [ncol][G], bw = h a
 *   DEVICE [ncol] of positive bandwidths (scipy.stats.gaussian_kde in one dimension with
 *   h = factor * std).  NH_EINVAL also: G < 1, ncol > 65535. */
#define NH_HIST_MAX_COLS 32
#define NH_HIST_MAX_PAIRS 496
#define NH_HIST_MAX_BINS_1D 4096
#define NH_HIST_MAX_BINS_2D 100
int nh_column_moments(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                      long long* counts, double* stats);
int nh_hist_columns(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                    const double* edges, int nb, const int* pairs /*host*/, int npairs,
                    long long* h1, long long* h2);
int nh_kde_columns(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                   const double* points, int G, const double* bw, double* out);

/* ---- the sequences of a Gelman-Rubin R-hat over k independent ensembles -----------------------
 * x is the DEVICE chain [rows][ld] of k ensembles of n walkers (nh_moves_create_ensembles), a row
 * laid out [walker][parameter] with k*n*ndim <= ld values in use: walkers [r*n, (r+1)*n) are
 * ensemble r (a history block of the device loop; an uploaded get_chain()).  Rows
 * [row0, row0 + nrows) are cut into nsplit equal parts of nrows / nsplit rows, a remainder being
 * dropped from the FRONT.  With q = (part*k + r)*ndim + d, all walkers of the ensemble pooled:
 *   counts (DEVICE int64 [nsplit*k*ndim]): counts[q] = the number of finite values;
 *   stats  (DEVICE [2][nsplit*k*ndim]): stats[0][q] = their mean, stats[1][q] = their unbiased
 *     variance (ddof = 1).
 * Two passes (the mean, then sum (x - mean)^2), as nh_column_moments: non-finite values are left
 * out of both; equal values have that value as their mean and variance exactly 0; the mean is NaN
 * without a finite value, the variance with fewer than two.  Stream-ordered on the context's
 * stream, no host synchronisation, library scratch, 64-bit row indices.  Deterministic: no
 * floating-point atomics, every sum in an order fixed by the shapes alone.
 * NH_EINVAL: a null argument, k or nsplit outside [1, 65535], n < 1, ndim outside [1, 256],
 *   row0 < 0, nrows < nsplit, k*n*ndim > ld. */
int nh_group_moments(nh_ctx* ctx, const double* x, long long row0, long long nrows, long long ld,
                     int k, int n, int ndim, int nsplit, long long* counts, double* stats);

/* ---- model comparison: pointwise log-likelihood, WAIC and PSIS-LOO ----------------------------
 * The matrix L[sample][data point] of a chain's stored spectra and the column reductions the
 * widely applicable information criterion and Pareto-smoothed importance-sampling leave-one-out
 * cross-validation (Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry) need.
 * Every matrix is a row-major DEVICE matrix [M][ld] with ncol <= ld columns in use; every other
 * array is a DEVICE array unless marked host; results stay on the device.  Stream-ordered on the
 * context's stream, no host synchronisation, library scratch, 64-bit row indices.  Deterministic:
 * integer atomics only; every floating-point sum has an order fixed by the shapes alone.
 * Every entry point: NH_EINVAL for M == 0, M >= 2^31, ncol < 1, ncol > ld or a null argument.
 * nh_pointwise_lnl: x [M][ld] holds M spectra at the table's nE energies in the model's unit;
 *   conv, flux, elo, ehi [nE], ul (int32 [nE]) and cl [nE + 1] are the data columns of the
 *   likelihood (nh_lnprob).  Writes L [M][ldL]: for a point that is not an upper limit
 *   -(d*d)/(2*sg*sg) with d = x*conv - flux and sg = d > 0 ? ehi : elo; for an upper limit
 *   log(1 - cl[nviol]) if x*conv > flux, else 0, nviol being the number of violated limits of the
 *   ROW (the reference's quirk, core.py:89-92) -- the columns of a row sum to nh_lnprob's
 *   likelihood of that spectrum.  total [M] (or NULL) receives the row sums (lane order, then a
 *   butterfly), nbad (int64 [1]) the number of non-finite values written to L.  One wave per row.
 *   NH_EINVAL also: nE > ldL.
 * nh_lnl_column_stats: stats [5][ncol] = per column of L its max, mean, unbiased variance
 *   (ddof = 1; exactly 0 for equal values, NaN for M == 1), lse = max + log sum_s exp(L - max),
 *   and min.  Two passes in chunk order.  L must be finite (a non-finite value spreads).
 * nh_psis_columns: per column k, with x_s = min_k - L[s][k] (the negated column, its maximum
 *   subtracted), Mt the tail length (host: min(M / 5, ceil(3 sqrt(M / reff)))), stats the output
 *   of nh_lnl_column_stats and lsel [ncol] the order statistic of rank Mt of every column of L
 *   (nh_column_select): cut = max(min_k - lsel[k], log(DBL_MIN)); the tail is the n <= Mt rows
 *   with x > cut, sorted by (value, row index).  n <= 4 (always for Mt == 0): pareto_k = +inf and
 *   nothing is smoothed.  Otherwise the generalised Pareto distribution is fitted to
 *   t = exp(x) - exp(cut) (Zhang & Stephens 2009 with m = 30 + floor(sqrt(n)) candidates, the
 *   loo package's weak priors: k = (n k' + 5) / (n + 10)) and, k being finite, tail value i
 *   becomes min(0, log(sigma expm1(-k log1p(-p_i)) / k + exp(cut))), p_i = (i + 0.5) / n
 *   (-sigma log1p(-p_i) for |k| < DBL_EPSILON).  With lw = x - logsumexp(x):
 *   pareto_k [ncol], n_tail (int64 [ncol]) = n, elpd [ncol] = logsumexp_s(lw_s + L[s][k]).
 *   No weight matrix is written: the rows below the cutoff enter both sums in one chunked pass.
 *   NH_EINVAL also: Mt outside [0, M), Mt > NH_PSIS_MAX_TAIL (the tail lives in one workgroup's
 *   LDS: thin the chain). */
#define NH_PSIS_MAX_TAIL 4096
int nh_pointwise_lnl(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                     const double* conv, const double* flux, const double* elo, const double* ehi,
                     const int* ul, const double* cl, double* L, long long ldL, double* total,
                     long long* nbad);
int nh_lnl_column_stats(nh_ctx* ctx, const double* L, long long M, int ncol, long long ld,
                        double* stats);
int nh_psis_columns(nh_ctx* ctx, const double* L, long long M, int ncol, long long ld, int Mt,
                    const double* stats, const double* lsel, double* pareto_k, long long* n_tail,
                    double* elpd);

/* ---- rank-normalised convergence statistics: the rank transform of whole pooled columns ------
 * What scipy.stats.rankdata(method="average"), scipy.special.ndtri on Blom's plotting positions
 * and two elementwise NumPy expressions compute on the host for the rank-normalised, folded
 * split-R-hat and the bulk / tail effective sample sizes of Vehtari, Gelman, Simpson, Carpenter &
 * Buerkner 2021.  x is a row-major DEVICE matrix [rows][ld].  A POOLED column p < ncolp holds
 * S = nrows * npool values, element e = t * npool + j being x[(row0 + t) * ld + j * cstride + p]:
 * a plain matrix [M][ncol] is row0 = 0, nrows = M, npool = 1, ncolp = ncol; a chain
 * [rows][walker][parameter] behind `discard` rows, every walker's values of a parameter pooled
 * (chain[discard:, :, p].ravel()), is row0 = discard, cstride = ndim, npool = walkers,
 * ncolp = ndim.  No pooled copy is made.  Stream-ordered on the context's stream, no host
 * synchronisation, 64-bit indices.  Deterministic and bit-reproducible from call to call: integer
 * atomics only (digit histograms in LDS, the status count), the scatter of the sort takes its
 * offsets from wave ballots.
 * Every entry point: NH_EINVAL for a null argument, row0 < 0, nrows, npool or ncolp < 1,
 *   cstride < ncolp with npool > 1, (npool - 1) * cstride + ncolp > ld (or ldz, ldo),
 *   nrows * npool >= 2^31.
 * nh_rank_columns: r (DEVICE [S][ncolp], the pooled layout) = the 1-based average ranks within
 *   each pooled column: equal values share the mean of the positions they occupy; -0.0 and +0.0
 *   are equal.  A pooled column that holds any NaN or +-inf is NaN in every row, and status
 *   (DEVICE int32 [ncolp]) counts its non-finite values (0 for a ranked column): no partial
 *   ranking.  A least-significant-digit radix sort of (64-bit key, row index), eight 8-bit
 *   passes.  Library scratch of 16 * S bytes per pooled column + a little; above 256 MiB the
 *   pooled columns are ranked in groups (NAIMA_AMD_RANK_SCRATCH_KIB, read at every call, sets
 *   another budget).
 * nh_rank_normal_scores: z = Phi^-1((r - 3/8) / (S + 1/4)) for every rank of r (DEVICE
 *   [S][ncolp], nh_rank_columns' output), S = nrows * npool; NaN in, NaN out.  layout =
 *   NH_RANK_POOLED: z is [S][ncolp] (ldz, cstride unused); NH_RANK_CHAIN: element e = t * npool + j
 *   of column p goes to z[t * ldz + j * cstride + p], the chain's layout with its rows starting
 *   at 0 -- what nh_group_moments and nh_autocorr_prep take.  Phi^-1 is Wichura's AS 241 PPND16
 *   in FP64 (a rational in the centre, two tail branches in sqrt(-log p)), applied to the
 *   correctly rounded quotient; accurate for the arguments ranks give, S <= 2^24.
 * nh_rank_transform: out[t * ldo + j * cstride + p] (the chain's layout, rows from 0) =
 *   |x - thr[p]| for mode NH_RANK_FOLD, (x <= thr[p] ? 1 : 0) for NH_RANK_LE, thr a DEVICE
 *   [ncolp]; NaN where x (or, for NH_RANK_LE, thr[p]) is NaN.  NH_EINVAL also: another mode. */
enum { NH_RANK_POOLED = 0, NH_RANK_CHAIN = 1 };
enum { NH_RANK_FOLD = 0, NH_RANK_LE = 1 };
int nh_rank_columns(nh_ctx* ctx, const double* x, long long row0, long long nrows, long long ld,
                    long long cstride, int npool, int ncolp, double* r, int* status);
int nh_rank_normal_scores(nh_ctx* ctx, const double* r, long long nrows, int npool, int ncolp,
                          int layout, long long ldz, long long cstride, double* z);
int nh_rank_transform(nh_ctx* ctx, const double* x, long long row0, long long nrows, long long ld,
                      long long cstride, int npool, int ncolp, const double* thr, int mode,
                      double* out, long long ldo);

/* ---- posterior predictive checks: replicated data, discrepancy statistics, PIT ----------------
 * Goodness of fit from a chain's stored spectra.  x [M][ld] holds M spectra at the table's nE
 * energies in the model's unit; conv, flux, elo, ehi [nE] and ul (int32 [nE]) are the data columns
 * of the likelihood (nh_pointwise_lnl), mc[s][k] = x[s][k]*conv[k] the model in the data's unit.
 * Upper limits take no part in a discrepancy statistic; P is the set of the other points.  Every
 * matrix is a row-major DEVICE matrix with ncol <= ld columns in use; every array is a DEVICE
 * array; results stay on the device.  Stream-ordered on the context's stream, no host
 * synchronisation, 64-bit row indices.  Deterministic: integer atomics only; every floating-point
 * sum has an order fixed by the shapes alone.
 * Every entry point: NH_EINVAL for M == 0, M >= 2^31, nE < 1, nE > ld or a null argument.
 * nh_ppc_rows: the sampling distribution is the one the likelihood implies (core.py:76-85): a
 *   datum y given the model m is split normal, scale ehi on the side y < m (weight
 *   ehi/(elo+ehi)) and elo on the side y > m.  For k in P and the global row index row = row0 + s,
 *   Philox4x32-10 (Salmon et al. 2011: multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants
 *   0x9E3779B9, 0xBB67AE85) of counter (lo32(row), hi32(row), k, 0) under key (lo32(seed),
 *   hi32(seed)) gives r0..r3;
 *     U = (((uint64)r0 << 20 | r1 >> 12) + 0.5) 2^-52,  V = (r2 + 0.5) 2^-32,  W = r3 2^-32,
 *     a = sqrt(-2 log U) |cos(2 pi V)|  (half-normal),  below = W (elo + ehi) < ehi,
 *     y_rep = below ? mc - ehi a : mc + elo a,  r_rep = below ? -a : +a,
 *   and the observed residual is r_obs = -d/sg with d = mc - flux, sg = d > 0 ? ehi : elo.  A
 *   value depends on (seed, row, k) alone: neither on the launch shape nor on how the rows are
 *   cut into calls.  Y [M][ldY] (or NULL) receives y_rep, mc itself at an upper limit; T [M][6]
 *   (or NULL) = chi2_obs, chi2_rep, maxabs_obs, maxabs_rep, runs_obs, runs_rep over P in column
 *   order: chi2 = sum r^2 (lane order, then a butterfly), maxabs = max |r| (NaN if an r is),
 *   runs = 1 + the sign changes between consecutive points of P, r >= 0 counting as positive
 *   (0 for an empty P), stored as doubles -- a matrix nh_column_moments, nh_hist_columns and
 *   nh_column_select take as it is.  One wave per row.
 *   NH_EINVAL also: Y and T both NULL, nE > ldY, row0 < 0.
 * nh_ppc_counts: counts (int64 [4]) over the rows of T [M][6] whose six values are all finite:
 *   [0] chi2_rep >= chi2_obs, [1] maxabs_rep >= maxabs_obs, [2] runs_rep <= runs_obs; [3] the
 *   number of the other rows.
 * nh_pit_columns: out [2][nE].  out[0][k], k in P: the mean over the rows of the split-normal CDF
 *   F(flux[k] | mc[s][k]), F = 2 ehi/(elo+ehi) Phi(z/ehi) for z = y - m <= 0 (Phi through erfc:
 *   a far point stays positive), ehi/(elo+ehi) + 2 elo/(elo+ehi) (Phi(z/elo) - 1/2) above.
 *   out[1][k], k an upper limit: the fraction of rows with mc > flux.  NaN where the other
 *   applies.  Column sums in the tiling of nh_column_moments, per-chunk partials added in chunk
 *   order: repeated calls are bit-identical. */
int nh_ppc_rows(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                const double* conv, const double* flux, const double* elo, const double* ehi,
                const int* ul, unsigned long long seed, long long row0, double* Y, long long ldY,
                double* T);
int nh_ppc_counts(nh_ctx* ctx, const double* T, long long M, long long* counts);
int nh_pit_columns(nh_ctx* ctx, const double* x, long long M, int nE, long long ld,
                   const double* conv, const double* flux, const double* elo, const double* ehi,
                   const int* ul, double* out);

/* ---- marginal likelihood by bridge sampling: covariance, normal proposal, iteration sums ------
 * What the bridge-sampling estimate of Z = int exp(lnprob) (Meng & Wong 1996; the "normal" method
 * of Gronau et al. 2017) reads from a chain in HBM.  Pooled rows are addressed as the pooled
 * columns of nh_rank_columns are: pooled row e = t * npool + j holds the d values
 * x[(row0 + t) * ld + j * cstride + 0 .. d - 1]; S = nrows * npool of them.  A chain
 * [rows][walker][parameter] behind `discard` rows is row0 = discard, cstride = d, npool = walkers;
 * a plain matrix [M][ld] is npool = 1.  mean is [d], L the LOWER Cholesky factor of the
 * covariance, row-major [d][d] (the upper triangle is not read); every array is a DEVICE array and
 * results stay on the device.  FP64; stream-ordered on the context's stream, no host
 * synchronisation; no atomics: every floating-point sum has an order fixed by the shapes alone
 * (per-chunk partials added in chunk order, the tiling of nh_column_moments), so repeated calls
 * are bit-identical.
 * nh_chain_cov, nh_mvn_logpdf: NH_EINVAL for a null argument, row0 < 0, nrows, npool or d < 1,
 *   d > NH_EVID_MAX_DIM, cstride < d with npool > 1, (npool - 1) * cstride + d > ld,
 *   nrows * npool >= 2^31.
 * nh_chain_cov: mean [d] and cov [d][d], the unbiased (ddof = 1) covariance of the S pooled rows,
 *   exactly symmetric.  Two passes: the mean, then the centred products.  A column that holds a
 *   NaN or +-inf has a NaN mean, and its row and column of cov are NaN.  S = 1: cov is NaN (0/0).
 * nh_mvn_draw: out[r][0..d-1] = mean + L z_r for r < n, out a matrix [n][ld]; columns d..ld-1 are
 *   not written.  z_r[c] is standard normal: Philox4x32-10 (nh_ppc_rows' generator) of counter
 *   (lo32(row), hi32(row), c >> 1, 0x4D564E31) under key (lo32(seed), hi32(seed)), row = row0 + r,
 *   gives r0..r3; U = (((uint64)r0 << 20 | r1 >> 12) + 0.5) 2^-52, V the same of (r2, r3),
 *   z = sqrt(-2 log U) cos(2 pi V) for an even c and ... sin(2 pi V) for an odd one (Box-Muller).
 *   Counter word 3 keeps the stream apart from nh_ppc_rows' (word 3 = 0) under the same seed.  A
 *   value depends on (seed, row, c) alone: neither on the launch shape nor on how the rows are
 *   cut into calls.  z2[r] = sum_c z_r[c]^2 in column order.
 *   NH_EINVAL: a null argument, d outside [1, NH_EVID_MAX_DIM], n outside [1, 2^31), row0 < 0,
 *   d > ld.
 * nh_mvn_logpdf: out[e] = log N(theta_e; mean, L L^T) = -d/2 log 2 pi - sum_i log L_ii - |y|^2/2,
 *   y = L^-1 (theta_e - mean) by forward substitution, for every pooled row; with lp [S] given
 *   (else NULL), out[e] = lp[e] - log N(...): the chain's stored log-probability over the
 *   proposal's density.  A row with a NaN or +-inf entry gives NaN.
 * nh_bridge_l2: out[i] = lp[i] + z2[i]/2 + d/2 log 2 pi + sum_i log L_ii for i < n: the same
 *   ratio at draw i of nh_mvn_draw, whose density follows from its own |z|^2.  lp = -inf (a draw
 *   the prior forbids) stays -inf.
 * nh_bridge_sums: one iteration of the estimator.  out [2] = { sum_j f(l2[j] - lstar),
 *   sum_i g(l1[i] - lstar) } with f(x) = e^x / (s1 e^x + s2 r), g(x) = 1 / (s1 e^x + s2 r); for
 *   x > 0 both are evaluated through e^-x, so nothing overflows, and x = -inf gives f = 0
 *   exactly.  f1 [N2] and f2 [N1] (or NULL) receive the terms themselves.  Two launches.
 *   NH_EINVAL: a null l1, l2 or out, N1 or N2 outside [1, 2^31). */
#define NH_EVID_MAX_DIM 32
int nh_chain_cov(nh_ctx* ctx, const double* x, long long row0, long long nrows, long long ld,
                 long long cstride, int npool, int d, double* mean, double* cov);
int nh_mvn_draw(nh_ctx* ctx, const double* mean, const double* L, int d, unsigned long long seed,
                long long row0, long long n, double* out, long long ld, double* z2);
int nh_mvn_logpdf(nh_ctx* ctx, const double* x, long long row0, long long nrows, long long ld,
                  long long cstride, int npool, int d, const double* mean, const double* L,
                  const double* lp, double* out);
int nh_bridge_l2(nh_ctx* ctx, const double* lp, const double* z2, long long n, const double* L,
                 int d, double* out);
int nh_bridge_sums(nh_ctx* ctx, const double* l1, long long N1, const double* l2, long long N2,
                   double lstar, double s1, double s2, double r, double* out, double* f1,
                   double* f2);

/* ---- reweighting a finished fit: PSIS weights and weighted reductions -------------------------
 * What importance reweighting of the samples already held needs: the log-ratio of a new target
 * from columns of the pointwise matrix, Pareto-smoothed self-normalised log-weights (Vehtari,
 * Simpson, Gelman, Yao & Gabry), weighted moments and order statistics, and an equal-weight
 * sample by systematic resampling.  FP64; every matrix is a row-major DEVICE matrix [M][ld] with
 * ncol <= ld columns in use; every other array is a DEVICE array unless marked host; results stay
 * on the device.  Stream-ordered on the context's stream, no host synchronisation, library
 * scratch, 64-bit row indices.  Deterministic: integer atomics only; every floating-point sum has
 * an order fixed by the shapes alone (in a sorted column, by the sorted values), so repeated calls
 * are bit-identical.
 * Every entry point that takes a matrix: NH_EINVAL for a null argument, M == 0, M >= 2^31,
 *   ncol < 1, ncol > ld.
 * A WEIGHT COLUMN is a pointer lw to its first entry and a row stride ldw >= 1 (NH_EINVAL
 *   otherwise), holding NORMALISED log-weights (a column of nh_psis_weights' lw).  A row with
 *   lw = -inf has weight zero: it is left out of every reduction below whatever its value, a NaN
 *   included.  Every other row counts as a row of positive weight, w = exp(lw).
 * nh_row_sums_select: out[s * ldo] = sign * sum_j L[s][cols[j]] for s < M, added in the order of
 *   cols (host int [n]; a column may repeat); n == 0 writes zeros (cols may be NULL then).
 *   NH_EINVAL also: n < 0, a column outside [0, ncol), sign other than +1 or -1, ldo < 1.
 * nh_psis_weights: per column k of the log-ratios lr, with x_s = lr[s][k] - max_s lr[s][k], Mt the
 *   tail length and lsel [ncol] the order statistic of rank M - Mt - 1 of every column of lr
 *   (nh_column_select): cut = max(lsel[k] - max_k, log(DBL_MIN)); the tail is the n <= Mt rows
 *   with x > cut, sorted by (value, row index); the fit and the smoothing are nh_psis_columns'
 *   (n <= 4, always for Mt == 0: pareto_k = +inf and nothing is smoothed -- plain self-normalised
 *   weights).  Writes lw[s * ldw + k] = x_s - logsumexp_s(x) (columns ncol..ldw-1 are not
 *   touched), pareto_k [ncol], n_tail (int64 [ncol]) = n, ess [ncol] = 1 / sum_s exp(2 lw) (Kish)
 *   and lmean [ncol] = logsumexp_s(lr) - log M of the RAW ratios, the estimate of
 *   log(Z_new / Z_old).  An entry -inf is legal: weight zero, never a tail row.  A column that
 *   holds a NaN or a +inf, or no finite entry, gets NaN in every row of lw and in pareto_k, ess and
 *   lmean, and n_tail = 0: no partial result; status (int32 [ncol]) counts its NaN and +inf
 *   entries (M for a column of -inf alone), 0 for a column that got weights.
 *   NH_EINVAL also: ncol > ldw, Mt outside [0, M), Mt > NH_PSIS_MAX_TAIL.
 * nh_weighted_moments: out [3][ncol] = per column the number of rows of positive weight (as a
 *   double), the weighted mean sum w x / sum w and the weighted variance sum w (x - mean)^2 /
 *   sum w.  Two passes, per-chunk partials added in chunk order (the tiling of
 *   nh_column_moments).  Equal values have that value as their mean and variance exactly 0; a
 *   non-finite value in a row of positive weight, or no such row, makes mean and variance NaN.
 * nh_weighted_select: the rows of positive weight of a column sorted ascending by (value, row
 *   index), -0.0 == +0.0; c_i the inclusive running sum of w in that order, C the last one.
 *   out[j][col] ([nq][ncol]) = the value of the first i with c_i >= q[j] * C and c_i > 0.  A NaN
 *   value under positive weight, or C not positive, gives NaN in the column's nq entries.  The
 *   sort is nh_rank_columns' (its scratch rule too: columns in groups above the budget); the
 *   running sum's order depends on M alone and it never decreases.
 *   NH_EINVAL also: q[j] (host double [nq]) outside [0, 1], nq outside [1, 16].
 * nh_resample_systematic: with c_i the inclusive running sum of w over the M rows IN ROW ORDER and
 *   C the last one, idx[j] (int64 [n_out]) = the first i with c_i >= ((u0 + j) / n_out) * C and
 *   w_i > 0: row i is drawn floor(n_out w_i / C) or one more times, the indices never decrease.
 *   Without a positive C every idx[j] is -1.  NH_EINVAL: a null argument, M == 0, M >= 2^31,
 *   ldw < 1, u0 outside [0, 1), n_out outside [1, 2^31).
 * nh_gather_rows: out[j * ldo + c] = x[idx[j] * ld + c] for j < n_out, c < ncol; idx (int64
 *   [n_out]) must hold rows of x.  NH_EINVAL: a null argument, n_out outside [1, 2^31), ncol < 1,
 *   ncol > ld, ncol > ldo. */
int nh_row_sums_select(nh_ctx* ctx, const double* L, long long M, int ncol, long long ld,
                       const int* cols /*host*/, int n, int sign, double* out, long long ldo);
int nh_psis_weights(nh_ctx* ctx, const double* lr, long long M, int ncol, long long ld, int Mt,
                    const double* lsel, double* lw, long long ldw, double* pareto_k,
                    long long* n_tail, double* ess, double* lmean, int* status);
int nh_weighted_moments(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                        const double* lw, long long ldw, double* out);
int nh_weighted_select(nh_ctx* ctx, const double* x, long long M, int ncol, long long ld,
                       const double* lw, long long ldw, const double* q /*host*/, int nq,
                       double* out);
int nh_resample_systematic(nh_ctx* ctx, const double* lw, long long ldw, long long M, double u0,
                           long long n_out, long long* idx);
int nh_gather_rows(nh_ctx* ctx, const double* x, long long ld, const long long* idx,
                   long long n_out, int ncol, double* out, long long ldo);

/* ---- S Nelder-Mead searches in lock-step (nh_simplex.hip; naima_amd/optimize.py) -------------
 * The bookkeeping of S independent simplexes in HBM; the function evaluation between the calls
 * is the caller's.  Simplex s minimises over its FREE coordinates -- those d with
 * frozen[s * ndim + d] == 0, n_free(s) of them, 1 <= n_free(s) <= nmax <= ndim -- with the others
 * pinned at value[s * ndim + d] (frozen == value == NULL: every coordinate is free), and follows
 * naima's prefit algorithm (relative xtol / ftol; rho = 1, chi = 2, psi = sigma = 1/2; initial
 * simplex x 1.05, or 0.00025 where the coordinate is 0) on that reduced function decision for
 * decision and bit for bit, with two rules fixed: a function value that is NaN counts as +inf,
 * and the sort is stable (ties keep their order; the replaced point is last before the sort).
 * `state` is device memory of nh_simplex_bytes(S, ndim, nmax) bytes (0: sizes out of range) that
 * the caller owns; every call takes the same (S, ndim, nmax).  ndim <= NH_SIMPLEX_MAX_DIM, the
 * step kernels' own limit, and S * (nmax + 1) * ndim < 2^31.  A parameter block qT[ndim][n] is
 * n columns of ndim coordinates, column c at qT[d * n + c] (the layout of the step loop's qT).
 * A FUNCTION COLUMN is a pointer f and a stride fstride >= 1: the value of column c is
 * f[c * fstride], negated first where is_logp != 0 (f is a log-probability to MAXIMISE).
 *   nh_simplex_init_points  x0 [S][ndim]; maxiter, maxfev < 0: 200 * n_free(s).  Writes the state
 *       and the initial points qT[ndim][(nmax + 1) * S], point p of simplex s in column p * S + s
 *       (p > n_free(s): the start itself).  A simplex with n_free outside [1, nmax] gets status 3
 *       and is never touched again.
 *   nh_simplex_adopt        takes those columns' values: sort, nfev = n_free + 1, nit = 1.
 *   nh_simplex_propose      qT[ndim][4 * S]: reflection, expansion, outside and inside contraction
 *       of simplex s in columns s, S + s, 2 S + s, 3 S + s; a finished simplex writes its best
 *       point four times and its state is not touched again.
 *   nh_simplex_update       takes those columns' values (qT as propose wrote it): accepts one of
 *       the four and re-sorts, or flags the simplex for a shrink; nfev counts what the sequential
 *       algorithm would have evaluated; then the stopping rules: status 0 converged, 1 maxfev,
 *       2 maxiter, -1 still active.
 *   nh_simplex_counts       (host int [2]) = { simplexes still active, simplexes flagged for a
 *       shrink } as the last adopt / update / shrink_adopt left them: an 8-byte download.  Both
 *       come from a scan in index order, not from atomics.
 *   nh_simplex_shrink_points  for the nshrink = counts[1] flagged simplexes, k-th in index order:
 *       moves the points of rank j >= 1 half way to the best and writes them to
 *       qT[ndim][nmax * nshrink], column (j - 1) * nshrink + k (j > n_free: the best point).
 *   nh_simplex_shrink_adopt   takes those columns' values, nfev += n_free, sorts, clears the flag
 *       and applies the stopping rules.
 *   nh_simplex_result       x [S][ndim] the best point, fun [S] its value (of the MINIMISED
 *       function), ints (int32 [4][S]) = nfev, nit, status, n_free.
 * Every launch is on the context's stream; only nh_simplex_counts synchronises. */
#define NH_SIMPLEX_MAX_DIM 64
long long nh_simplex_bytes(int S, int ndim, int nmax);
int nh_simplex_init_points(nh_ctx* ctx, void* state, int S, int ndim, int nmax, const double* x0,
                           const int* frozen, const double* value, int maxiter, int maxfev,
                           double* qT);
int nh_simplex_adopt(nh_ctx* ctx, void* state, int S, int ndim, int nmax, const double* f,
                     long long fstride, int is_logp, double xtol, double ftol);
int nh_simplex_propose(nh_ctx* ctx, void* state, int S, int ndim, int nmax, double* qT);
int nh_simplex_update(nh_ctx* ctx, void* state, int S, int ndim, int nmax, const double* qT,
                      const double* f, long long fstride, int is_logp, double xtol, double ftol);
int nh_simplex_counts(nh_ctx* ctx, const void* state, int S, int ndim, int nmax,
                      int* counts /*host*/);
int nh_simplex_shrink_points(nh_ctx* ctx, void* state, int S, int ndim, int nmax, int nshrink,
                             double* qT);
int nh_simplex_shrink_adopt(nh_ctx* ctx, void* state, int S, int ndim, int nmax, int nshrink,
                            const double* f, long long fstride, int is_logp, double xtol,
                            double ftol);
int nh_simplex_result(nh_ctx* ctx, const void* state, int S, int ndim, int nmax, double* x,
                      double* fun, int* ints);

#ifdef __cplusplus
}
#endif
#endif /* NAIMA_HIP_H */
