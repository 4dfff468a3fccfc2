/*
 * msom.h -- C ABI of libmsomhip: the MI355X-native multi-layer quasi-geostrophic
 * timestepper that replaces the PV-advection + streamfunction-inversion hot path of
 * bderembl/msom (msqg/qg.h, msqg/poisson_layer.h, msqg/layer.h, driver msqg/qg.c).
 *
 * Every entry point names the reference interface it replaces (file:line relative to the
 * reference tree).  Plain pointers and sizes only.  All field arrays are fp64, numpy
 * C-order [layer][y][x], interior points only (msqg/qg.h:1164-1188); every `double*`
 * field argument may be a host pointer or a HIP device pointer (the library copies with
 * hipMemcpyDefault).  The caller owns every buffer it passes.
 *
 * Error convention: the reference prints to stdout and calls exit(0) on bad input
 * (msqg/qg.h:735-738,990-1012).  The library never exits: functions return MSOM_OK (0) or
 * a negative code and msom_last_error() holds the message.  Multigrid non-convergence is
 * not an error (reference: stderr warning, mspg/elliptic.h:215-219); it is reported in
 * msom_mgstats.
 */
#ifndef MSOM_H
#define MSOM_H

#ifdef __cplusplus
extern "C" {
#endif

#define MSOM_OK 0
#define MSOM_ERR_ARG (-1)      /* bad argument / unknown key / unknown field          */
#define MSOM_ERR_IO (-2)       /* file not found or short read                         */
#define MSOM_ERR_CONFIG (-3)   /* dh == 0, Rom <= 0, N not a power of two, nl too big  */
#define MSOM_ERR_HIP (-4)      /* HIP runtime error (no device, out of memory, ...)    */
#define MSOM_ERR_COMM (-5)     /* RCCL error                                           */
#define MSOM_ERR_STATE (-6)    /* call order violated (e.g. step before set_const)     */

#define MSOM_MAXNL 16          /* layers supported (msqg/poisson_layer.h:77 sizes its column arrays by nl) */
#define MSOM_FASTNL 8          /* up to here: the register-resident kernels (chained smoother, one-launch coarse levels, fused
                                  tendency pass); 9 .. MSOM_MAXNL: one kernel per reference loop, same arithmetic */

/* field ids, mirroring the reference's global layer lists (msqg/qg.h:22-57) */
enum {
  MSOM_PSI = 0,    /* pol    stream function                 */
  MSOM_Q = 1,      /* qol    potential vorticity (evolving)  */
  MSOM_ZETA = 2,   /* zetal  relative vorticity              */
  MSOM_PSIPG = 3,  /* ppl    large-scale stream function     */
  MSOM_ZETAPG = 4, /* zetapl large-scale relative vorticity  */
  MSOM_QFORC = 5,  /* q_forcl 3-D PV forcing                 */
  MSOM_TMP = 6,    /* tmpl                                   */
  MSOM_FR = 7,     /* Frl    Froude number, nl-1 layers      */
  MSOM_S = 8,      /* strl   (Fr/Ro)^2, nl-1 layers          */
  MSOM_DQ = 9,     /* updates                                */
  MSOM_RO = 10,    /* Ro, 1 layer                            */
  MSOM_TOPO = 11,  /* topo, 1 layer                          */
  MSOM_QPRED = 12, /* predictor                              */
  MSOM_NOISE = 13, /* n_stochl (msqg/qg_stochastic.h:13)     */
  MSOM_SIGMA = 14, /* s_stochl (msqg/qg_stochastic.h:14)     */
  /* passive tracers (nptr > 0): nl*nptr layers, index l*nptr + nt (msqg/qg.h:100-101) */
  MSOM_PTR = 15,       /* ptracersl                          */
  MSOM_PTR_RELAX = 16, /* ptr_relaxl                         */
  MSOM_DPTR = 17,      /* tracer part of `updates`           */
  MSOM_PTR_PRED = 18,  /* tracer part of the predictor       */
  MSOM_RD = 19,        /* Rd, deformation radius of the filter scale, 1 layer (msqg/qg.h:47,913,963-968) */
  MSOM_QOF = 20,       /* qofl, filter mean (msqg/qg.h:27,549); allocated on first use           */
  /* energy / PV budgets (msqg/qg_energy.h:7-15), nl layers each, allocated on first use */
  MSOM_DE_BF = 21, MSOM_DE_VD = 22, MSOM_DE_J1 = 23, MSOM_DE_J2 = 24, MSOM_DE_J3 = 25, MSOM_DE_FT = 26,
  MSOM_TMP2 = 27, MSOM_PO_MFT = 28,
  /* back-and-forth nudging on the device (msom_bfn_*): the arrays of the loop of msqg/qg_bfn.py:47-73, nl layers each, allocated on first use */
  MSOM_BFN_F1 = 29,   /* F1  newest AB3 history slot: the nudged tendency of the step being taken (msqg/qg_bfn.py:49,65-68) */
  MSOM_BFN_F2 = 30,   /* F2  second AB3 history slot (:50,73) */
  MSOM_BFN_F3 = 31,   /* F3  oldest AB3 history slot (:51,72) */
  MSOM_BFN_OBS = 32,  /* observed PV, the target of the nudging term ("BFN nudging goes here", :67-68) */
  MSOM_BFN_GAIN = 33, /* nudging gain per cell-layer, zero where nothing is observed; never set: 1 everywhere */
  MSOM_NFIELDS = 34
};

/* mgstats of Basilisk (text: mspg/elliptic.h:118-123), kept by the reference in `mgpsi`
 * (msqg/qg.h:61) */
typedef struct {
  int i;             /* number of multigrid cycles                */
  double resb, resa; /* max |residual| before and after           */
  double sum;        /* sum of the right-hand side                */
  int nrelax;        /* relaxations per level at exit             */
} msom_mgstats;

typedef struct msom msom_t;

const char *msom_last_error(void);
const char *msom_version(void);

/* ---- lifecycle: read_params -> init_grid -> set_vars   (msqg/qg.c:34-47, qg.h:689-761,837-925)
 * msom_create parses a params.in file; msom_create_str parses the same text from memory.
 * Extension keys (ignored by the reference parser, qg.h:698-731): Ny (non-square domain),
 * TOLERANCE, NITERMAX, NITERMIN.  Returns NULL on error. */
msom_t *msom_create(const char *params_path);
msom_t *msom_create_str(const char *params_text);
/* trash_vars, msqg/qg.h:1130-1154 */
int msom_destroy(msom_t *m);

/* run-time counterparts of the reference's compile-time flags and Basilisk globals:
 * "TOLERANCE" "NITERMAX" "NITERMIN" (mspg/elliptic.h:111-112, qg.h:159), "DT", "quiet",
 * "stochastic" (-D_STOCHASTIC), "seed", "noise_mode" (0: the reference's serial rand() stream generated on
 * the host, 1: counter-based Philox on the device), "flag_topo", "uniform_S" (0 forces the general
 * S-field kernels), "mode_pv_invert" [0] (MODE_PV_INVERT, msqg/qg.h:116: the inversion goes through the vertical modes, one tile only;
 * see msom_modes_mgstats), "profile" (HIP-event timing of the finest-level launches: 1 every kernel, 2 only the chained smoother passes;
 * an event pair costs ~10 us of stream time).
 * Implementation switches, all result-preserving in the strict build (defaults in brackets):
 * "fused" [1] one-pass tendency kernel, "adv_fused" [1] advance folded into it, "stoch_fused" [1] (product build only) the
 * stochastic variant rides in that kernel too: -q/tau and the noise are read in its finalisation next to q_in, "rhs_variant" [6: one layer per
 * wavefront with register windows; 1: LDS tiles],
 * "rhs_resid" [-1: from the size at which it wins] first residual of the next inversion as its by-product (msom_get_param("rhs_resid"):
 * whether this handle's passes emit it -- the option resolved and one tile with walls, "mg_fused", more than one level, "rhs_variant" 6, or 1 in
 * the strict build, whose by-products have the residual pass's bits), "mg_fused" [1] fused
 * residual/restriction and correction/residual passes, "prolong_fused" [1], "mg_coarse" [4] coarse levels
 * in one launch (1: their arrays in global memory, 2: resident in LDS, 3: as 2 with the LDS pool pre-filled with NaN -- test aid; round 3,
 * default 4: the lean LDS form k_mg_coarse_lean where it applies -- uniform S or one layer, walls or doubly periodic -- else as 2),
 * "resmax_rows" [0 = 32] rows per chunk of the marching max-only residual pass (-1: the LDS-tiled kernel), "march" [1] chained half-sweep smoother on HBM-bound single-GPU levels (2: on every level that is
 * wide enough), "march_k" [4] half-sweeps per pass, "march_rows" [0 = auto] chunk height, "march_min" [23] log2 of the cell-layers a level needs, "march_prolong" [1] prolongation folded
 * into the first pass, "march_dma" [2] memory side of the pass (0: register-window loads, 1: LDS-DMA prefetch with one strip per
 * workgroup, 2: four strips per workgroup marching in step), "graph" [0] replay the launches of a multigrid cycle from a captured hipGraph on the launch-bound grids
 * (measured neutral), "march_partial" [1], "march_correct" [1] correction folded into the last pass, "march_xcd" [1] XCD-contiguous block numbering, "march_flip" [1] odd chunks march downwards, "block_sweeps" [0] LDS-tiled blocked smoother (2 sweeps per launch, every level), "restrict2" [1] the pre-cycle residual pass restricts two levels down, "restrict_pyr" [1] the rest of the restriction chain in launches of up to five levels, "step_sync" [-1] (see msom_sync), "block8" [1] / "block8_max" [1024] round 3: prolongation + up to 8 half-sweeps of a
 * visit of a launch-bound level (64 .. block8_max cells a side, not marched; one GPU, walls or doubly periodic, nl <= 8; uniform or general S) in one launch of that kernel with a halo of 8, "agglomerate" [1] / "agg_size" [256]
 * gathered coarse levels of tiled runs, "mg_global_sum" [0]; "march_visit_rows" [0 = 28] / "march_visit_pairs" [2] chunk height /
 * wave pairs per workgroup of the fused finest-level visit; "march_dbg", "rhs_dbg", "lpw_dbg", "block_variant": timing experiments of
 * tools/.  Every option, these tuning keys included, is a setting of the handle it is set on and reaches no other handle. */
int msom_set_option(msom_t *m, const char *key, double value);
/* parsed / derived parameters: N nx ny nl L0 DT iRe iRe4 CFL Rom tend dtout beta tau0 Ekb Eks
 * sbc idh0_<l> idh1_<l> Fr_<l> dh_<l> nlevels; the handle's kernel options march_rows march_xcd march_flip march_dbg
 * march_lean march_dma march_visit_rows march_visit_pairs march_visit_ring march_visit_split resmax_rows block_variant rhs_dbg lpw_dbg.
 * The paths the solve takes (after msom_set_const), each from the same function the dispatch calls: relax_path_<k> (level k's sweeps:
 * 0 per-colour launches, 1 block2 -- two sweeps per LDS-tiled launch, an odd last sweep per colour, 2 block8 -- up to 8 half-sweeps
 * per launch, 3 chained half-sweeps k_relax_march, 4 inside the one-launch coarse group k_mg_coarse; 8 + one of 0..3 for a level
 * on the gathered global grid of a tiled run), march_levels (how many levels report 3), march_kmax (half-sweeps per chained pass),
 * march_lean_fine (level 0 is chained with its interior chunks in the lean body), march_visit (1: the first action of level 0's
 * visit in a cycle of 4 relaxations, asked the way the solve asks it, is the fused visit k_relax_visit) and march_visit_ring (how
 * that visit runs its wall-ring chunks, 0 / 1 / 2; -1 where march_visit is 0, which overrides the option of the same name) */
double msom_get_param(msom_t *m, const char *key);

/* pyset_field / pyget_field, msqg/qg.h:1164-1188 (array [layer][y][x]; BC applied after set) */
int msom_set_field(msom_t *m, int field, const double *a);
int msom_get_field(msom_t *m, int field, double *a);
int msom_field_layers(msom_t *m, int field);
/* mean removal of the initial condition, msqg/qg.c:65-70 */
int msom_remove_mean(msom_t *m, int field);
/* set_const, msqg/qg.h:931-1116: layer metrics, Ro, S = (Fr/Ro)^2, q = comp_q(psi), BCs.
 * Input files (psipg_, frpg_, topo, qforc_, p0.bas ...) are read by msom_read_inputs. */
int msom_set_const(msom_t *m);
/* optional input-file discovery in `dir` (msqg/qg.h:940-984, msqg/qg.c:55-59) */
int msom_read_inputs(msom_t *m, const char *dir);

/* ---- the two hooks Basilisk's run() calls (installed at msqg/qg.h:922-923) */
/* update_qg, msqg/qg.h:609-650: dq/dt = F(q); returns the CFL-limited dtmax (< 0 on error) */
double msom_update(msom_t *m, const double *q, double *dqdt, double dtmax);
/* advance_qg, msqg/qg.h:594-606 (stochastic: msqg/qg_stochastic.h:128-149) */
int msom_advance(msom_t *m, double *qout, const double *qin, const double *dqdt, double dt);

/* ---- elliptic plug-in (poisson_layer -> mg_solve(relax_layer, residual_layer),
 * msqg/poisson_layer.h:263-306; invertq msqg/qg.h:114-163).  psi is warm start and result. */
int msom_invertq(msom_t *m, const double *q, double *psi, msom_mgstats *st);
/* comp_q, msqg/qg.h:397-403 */
int msom_comp_q(msom_t *m, const double *psi, double *q);

/* ---- the array-level operator API of the reference's Python module, same argument order
 * (msqg/qg_bfn.h:21-103; SWIG typemaps msqg/qg_bfn.i) */
int pystep_bfn(msom_t *m, double *varin_py, int len1, int len2, int len3, double *tend_py, int len4, int len5,
               int len6, double direction, int vartype);
int pyq2p(msom_t *m, double *po_py, int len7, int len8, int len9, double *qo_py, int len10, int len11, int len12);
int pyp2q(msom_t *m, double *po_py, int len13, int len14, int len15, double *qo_py, int len16, int len17, int len18);
/* ---- the time loop around pystep_bfn, msqg/qg_bfn.py:47-73 (Adams-Bashforth 3 in numpy on the caller's side, "BFN nudging goes
 * here" :67-68), run on the library's stream with the state in device memory.  The evolving variable is the handle's MSOM_Q
 * (msom_set_field), the observations and the gain are MSOM_BFN_OBS / MSOM_BFN_GAIN, the history is MSOM_BFN_F1..F3; all five take
 * msom_set_field / msom_get_field (observation input, restart of the history).
 * msom_bfn_begin: F1 = F2 = F3 = 0 (:49-51; the AB3 weights apply from the first step on, as there).
 * msom_bfn_steps, nsteps times: F1 = tendency of q exactly as pystep_bfn(vartype = 1, direction) computes it (:65; the sign flips of
 * iRe, iRe4, Eks, Ekb persist in the handle, the warm start psi and the dt limiter end up where nsteps pystep_bfn calls leave them);
 *   F1 = F1 + (k * gain) * (obs - q)                      (k == 0: the term is skipped, obs and gain are not read)
 *   q  = q + (dt / 12) * ((23 * F1 - 16 * F2) + 5 * F3)   (:71; this expression order is the contract of the strict build)
 * boundary(q), then the slots rotate F1 -> F2 -> F3 -> F1 (:72-73 without the copies): on return F2 holds the newest nudged tendency,
 * F3 the one before it and F1 the oldest, which the next step overwrites.  dt is the caller's, signed: backward integration passes
 * dt < 0, direction = -1 and the sign of k it wants.  Time and iteration count of the handle do not change (pystep_bfn leaves them
 * alone).  nsteps == 0: no-op; nsteps < 0: MSOM_ERR_ARG; no msom_bfn_begin since msom_set_const, or k != 0 with MSOM_BFN_OBS never
 * set: MSOM_ERR_STATE.  Returns at the first error; the stream is synchronised on return.
 * msom_bfn_misfit: sqrt(sum gain (obs - q)^2 / sum gain) over every cell-layer of the domain (all tiles; collective there), by the
 * deterministic two-stage sums; MSOM_ERR_STATE without observations. */
int msom_bfn_begin(msom_t *m);
int msom_bfn_steps(msom_t *m, int nsteps, double dt, double direction, double k);
int msom_bfn_misfit(msom_t *m, double *misfit);

/* ---- running time means and eddy statistics on the device, and time_filter (msqg/qg.h:491-507).  The accumulators are no field ids:
 * they have this enum and the accessors below.  Ids 0 .. MSOM_ST_NACC - 1 are weighted sums kept in device memory, one [nl][ny][nx]
 * fp64 array each, only those a handle asked for; the ids from 16 on are formed from them on request and never stored. */
enum { MSOM_ST_PSI = 0,  /* sum w psi            */   MSOM_ST_Q = 1,   /* sum w q   */
       MSOM_ST_PSI2 = 2, /* sum w psi^2          */   MSOM_ST_Q2 = 3,  /* sum w q^2 */
       MSOM_ST_KE = 4,   /* sum w (u^2 + v^2)/2  */
       MSOM_ST_UQ = 5,   /* sum w u q            */   MSOM_ST_VQ = 6,  /* sum w v q */
       MSOM_ST_NACC = 7,
       /* derived on the device from the accumulators, never stored */
       MSOM_ST_EKE = 16,      /* mean KE - KE of the mean psi             */
       MSOM_ST_UQ_EDDY = 17,  /* mean(uq) - u(mean psi) * mean(q)         */
       MSOM_ST_VQ_EDDY = 18,
       MSOM_ST_QME = 32 };    /* qo_me of time_filter, msqg/qg.h:499-503  */
/* A sample reads the handle's MSOM_PSI (with the ghost values boundary() left in it, the ones the Jacobian reads; on tiles the exchanged
 * ones) and MSOM_Q, and adds to every selected accumulator, cell by cell,
 *   acc = acc + w * x,   x = psi, q, psi*psi, q*q, 0.5 * (u*u + v*v), u*q, v*q
 *   u = (psi[j-1][i] - psi[j+1][i]) / (2 Delta),   v = (psi[j][i+1] - psi[j][i-1]) / (2 Delta)     (2 Delta formed once on the host)
 * and W = W + w.  This expression order is the contract of the strict build (true divisions); the product build multiplies by
 * 1 / (2 Delta) and may contract.  No atomics and no reductions: the result is the same on every run.
 * msom_stats_begin: bit k of mask selects accumulator k; allocates the selected ones, zeroes them and W, restarts the count of
 *   "stats_every".  May be called again (another mask: the arrays are reallocated).  msom_set_const drops the statistics.
 * msom_stats_accumulate: one sample of weight w from the psi and q the handle holds now; queued on the library's stream, not synchronised.
 * msom_stats_weight: W.  msom_stats_get: `which` < MSOM_ST_NACC: S / W (a true division in both builds); MSOM_ST_EKE (needs PSI and KE)
 *   = S_KE / W - 0.5 * (um*um + vm*vm), MSOM_ST_UQ_EDDY (PSI, Q, UQ) = S_UQ / W - um * (S_Q / W), MSOM_ST_VQ_EDDY (PSI, Q, VQ) likewise
 *   with vm, where um, vm are the differences above of the mean psi after boundary() on a copy of it in a scratch field (difference
 *   operator and boundary conditions are linear, so these are the mean velocities); MSOM_ST_QME: qo_me.  out: [nl][ny][nx], host or
 *   device pointer, the local tile as with msom_get_field; the derived ids are collective on tiles (halo exchange of the mean psi).
 *   Both calls synchronise the stream.
 * Option "stats" [0] = 1: every msom_step takes one sample of (q_n, psi_n) with weight dt_n -- q_n the state the step starts from,
 *   psi_n what the step's first inversion leaves in MSOM_PSI (the pair the output event of msqg/qg.c:115 sees), dt_n the step the
 *   limiter chose -- before the second stage overwrites psi, with no host synchronisation (a lazy step stays lazy: the weight is read
 *   from the device scalar the step keeps it in).  "stats_every" [1] = n: only every n-th step since msom_stats_begin, with that
 *   step's dt.  msom_bfn_steps, msom_update and the pystep_* calls never sample; the option changes nothing in psi, q, dt or mgstats.
 * msom_time_filter: qo_me = (1 - a) * qo_me + a * q with a = dt / tau_f (option "tau_f" [20]) on the handle's MSOM_Q; qo_me is
 *   allocated and zeroed by the first call after msom_set_const (the reference's freshly created field) and needs no msom_stats_begin.
 * Errors: null handle, mask 0 or a bit >= MSOM_ST_NACC, w or dt not finite, `which` unknown or its accumulators not in the mask:
 *   MSOM_ERR_ARG; msom_stats_begin / msom_time_filter before msom_set_const, any other stats call (or option "stats" = 1, or a
 *   msom_step with it) with no msom_stats_begin since msom_set_const, msom_stats_get with W == 0 or of MSOM_ST_QME with no
 *   msom_time_filter since msom_set_const: MSOM_ERR_STATE.
 * msom_get_param "stats_mask" / "stats_bytes": the mask, and 8 nl ny nx bytes per array held (accumulators, qo_me; the allocations
 *   carry the pads of a field on top); both 0 on a handle that never called msom_stats_begin or msom_time_filter;
 *   "stats_dev_samples": automatic samples since msom_stats_begin that read their weight from the device scalar. */
int msom_stats_begin(msom_t *m, unsigned mask);     /* bit k = accumulator k; allocates those, zeroes them and W */
int msom_stats_accumulate(msom_t *m, double w);     /* one sample of the handle's MSOM_PSI / MSOM_Q, weight w */
int msom_stats_weight(msom_t *m, double *W);        /* sum of the weights so far */
int msom_stats_get(msom_t *m, int which, double *out); /* [nl][ny][nx], host or device pointer: S / W, or a derived quantity */
int msom_time_filter(msom_t *m, double dt);         /* qo_me = (1 - a) * qo_me + a * q, a = dt / tau_f; option "tau_f" [20] */

/* ---- vertical normal modes of the stretching operator on the device: eigmod of msqg/eigmode.h (compiled out in the reference by
 * MODE_PV_INVERT 0) and the layer <-> mode products of msqg/qg.h:117-131,143-157.  The mode arrays are no field ids: they have this enum
 * and the accessors below.  Only M2L and IBU are stored; L2M and RD are formed from them on request. */
enum { MSOM_MD_IBU = 0,  /* iBu_m = -lambda_m, iBu_0 = 0 exactly (eigmode.h:256-266); nl arrays [ny][nx]          */
       MSOM_MD_RD  = 1,  /* sqrt(-1 / iBu_m), 0 for m = 0 (eigmode.h:284); nl arrays                               */
       MSOM_MD_M2L = 2,  /* cm2l: array k*nl+m = vr[k][m], layer k from mode m (eigmode.h:246-248); nl*nl arrays   */
       MSOM_MD_L2M = 3,  /* cl2m: array m*nl+k, mode m from layer k (eigmode.h:245-247); nl*nl arrays              */
       MSOM_MD_N   = 4 };
/* msom_modes_compute (after msom_set_const): per column, from the handle's MSOM_S and the layer thicknesses, the eigenproblem of the
 *   tridiagonal amat of eigmode.h:86-109 (amat[l][l+1] = -S_l / (dhc_l dhf_l), amat[l][l-1] = -S_l-1 / (dhc_l-1 dhf_l), diagonal = minus
 *   the row's off-diagonals; nl = 1: the 1 x 1 zero matrix), solved as the symmetric tridiagonal D^1/2 amat D^-1/2, D = diag(dhf), by
 *   cyclic Jacobi rotations with a fixed cap of sweeps.  Modes in ascending order of the eigenvalue, mode 0 the barotropic one; right
 *   vectors with Flierl's normalisation sum_k dhf_k vr_km^2 = htotal (= 1, eigmode.h:70) and positive at the surface (sign(x) = x > 0 ?
 *   1 : -1); iBu_m = -lambda_m with iBu_0 = 0; left vectors l2m[m][k] = dhf[k] * m2l[k][m] (that product, htotal = 1 dropped), which is
 *   what the normalisation of eigmode.h:223-231 gives; Rd_m = sqrt(-1. / iBu_m).
 *   Storage: a stratification that is the same in every column (no MSOM_FR / MSOM_RO / MSOM_S set, no varRo) is solved once, by the same
 *   kernel on cell (0, 0), and kept as nl*nl + nl doubles in the handle; otherwise nl*nl + nl arrays of one layer each are allocated on
 *   the first compute and freed by msom_destroy.  Option "modes_compact" [-1: automatic; 0: always per column].
 *   An interface whose S is not positive and finite (the spectrum is degenerate, the vectors are not unique), an iteration that hits
 *   the cap, or a column too weakly stratified: MSOM_ERR_CONFIG, no modes; the handle stays usable.  msom_set_const drops the modes.
 *   Too weakly stratified: with lambda_0 <= lambda_1 <= ... <= lambda_max the computed eigenvalues of a column, nl >= 2 and
 *   lambda_1 <= 8 nl 2^-52 lambda_max.  8 nl eps lambda_max is the eigenvalue error of the method; below it fp64 cannot separate the first
 *   baroclinic mode from the barotropic one: the sign of lambda_1 (so Rd_1, and the sign of the mode's Helmholtz term) and which of the
 *   two near-null vectors is mode 0 would be arbitrary.  An MSOM_FR of 1e-9 of its neighbours' does this; msom_last_error names the cause.
 *   The surface entry vr[0][m] of a mode may be zero (never negative).
 * msom_modes_layers: arrays of `which` (nl or nl*nl).  msom_modes_get: those arrays, [layers][ny][nx], the local tile; the compact
 *   form is broadcast.
 * msom_modes_project: to_modes != 0: out_m = sum_k l2m[m][k] * in_k, else out_k = sum_m m2l[k][m] * in_m, accumulated as acc = 0;
 *   acc = acc + c * x with the inner index ascending (the contract of the strict build; the product build fuses each step).  Pointwise,
 *   so it works on tiles; in == out is allowed.
 * msom_modes_energy: from the handle's MSOM_PSI with the ghost values boundary() left there and u, v as the msom_stats_* block defines
 *   them: x_m = sum_k l2m[m][k] x_k for u, v, psi; ke[m] = sum_cells 0.5 * (u_m^2 + v_m^2) * Delta^2, pe[m] = sum_cells 0.5 * (-iBu_m) *
 *   psi_m^2 * Delta^2, one pass over psi, deterministic two-stage sums; over all tiles (collective there, like msom_bfn_misfit).
 *   Pointwise sum_m u_m^2 = sum_k dhf_k u_k^2 and sum_m (-iBu_m) psi_m^2 = sum_l S_l (psi_l - psi_l+1)^2 / dhc_l.
 * msom_modes_set_rd: MSOM_RD = MSOM_MD_RD of `mode` with the boundary condition of msom_set_field(MSOM_RD); the next msom_wavelet_filter
 *   builds sig_filt = min(afilt * Rd, Lfmax) from it.  mode = 1 is the reference's MODE_PV_INVERT branch, msqg/qg.h:1055-1057.
 * Errors: null handle, `which` out of range, null in / out (msom_modes_energy: both null), mode outside 1 .. nl-1: MSOM_ERR_ARG; any call
 *   but msom_modes_compute with no successful msom_modes_compute since msom_set_const: MSOM_ERR_STATE.  The stream is synchronised on
 *   return of every call except msom_modes_project with two device pointers.
 * msom_get_param "modes_ready", "modes_compact" (the form held, or that the next compute will take), "modes_bytes" (8 ny nx per stored
 *   array, 0 in the compact form).  msom_bench_kernel names "modes_project" and "modes_energy". */
int msom_modes_compute(msom_t *m);
int msom_modes_layers(msom_t *m, int which);                       /* nl or nl*nl */
int msom_modes_get(msom_t *m, int which, double *out);             /* [layers][ny][nx], host or device pointer, local tile */
int msom_modes_project(msom_t *m, int to_modes, const double *in, double *out);  /* [nl][ny][nx] each, host or device */
int msom_modes_energy(msom_t *m, double *ke, double *pe);          /* [nl] each, host pointers; either may be NULL */
int msom_modes_set_rd(msom_t *m, int mode);                        /* MSOM_RD = MSOM_MD_RD of `mode` */

/* ---- modal PV inversion: the MODE_PV_INVERT 1 body of invertq, msqg/qg.h:116-157, as a run-time option.
 * msom_set_option("mode_pv_invert", 1) [0]: the one place that inverts (msom_invertq, pyq2p, msom_update, msom_step, msom_run,
 *   pystep_bfn, msom_bfn_steps, pystep_de) computes the modes if they are not ready (as msom_modes_compute does, its errors pass
 *   through), projects q_m = sum_k l2m[m][k] q_k, solves the nl independent problems  lap(p_m) + iBu_m p_m = q_m  by the multigrid cycle
 *   of mspg/elliptic.h (minlevel = 1, red-black Jacobi half-sweeps starting with the colour (i + j) even, mean-of-4 restriction, bilinear
 *   prolongation), then psi_k = sum_m m2l[k][m] p_m into MSOM_PSI with its boundary fill.  The warm start is the persistent mode-space
 *   field p_m (the reference's pom), zero after msom_set_const; MSOM_PSI is not read.  msom_comp_q / pyp2q stay layered (:397-403).
 *   Every mode has its own mgstats: i, nrelax (4 at the start, +1 where resb / resa < 1.2, -1 where > 10, as mg_solve), resb, resa,
 *   sum.  All modes of a level share a launch; the host reads the nl maxima once per cycle.  Freeze rule: a mode that has met TOLERANCE
 *   after NITERMIN cycles (or has done NITERMAX) is frozen -- it takes no more sweeps, its correction is zero on every level and its p_m
 *   keeps its bits -- while the others go on, each with its own nrelax (a launch runs max nrelax sweeps, a mode stops at its count).
 *   msom_last_mgstats / the mgstats of msom_invertq are the LAST mode's (the reference overwrites mgpsi per poisson() call);
 *   msom_modes_mgstats gives any mode's: MSOM_ERR_STATE before the first modal solve since msom_set_const, MSOM_ERR_ARG for a mode
 *   outside 0 .. nl-1.  With the option on, msom_set_const also computes the modes and sets MSOM_RD from mode 1 (msom_modes_set_rd(m, 1),
 *   msqg/qg.h:1055-1057; skipped for nl = 1).  The fused paths of the layered solver (rhs_resid, residual2, the speculative tendency
 *   launch, the marched and fused visits) are off in modal mode; max|u| of the dt limiter comes from its own pass over psi.
 *   Scope: one tile, walls or sbc = -1.  A handle of msom_create_tiled with more than one rank answers the option with MSOM_ERR_CONFIG.
 *   Doubly periodic: the barotropic mode (iBu_0 = 0) is singular as the layered problem's barotropic part is: zero-mean q needed.
 * Expression order (the contract of the strict build; E, W, N, S the four neighbours, D = Delta):
 *   relax:    n = -(D*D) * b;  n = n + (a[E] + a[W]);  n = n + (a[N] + a[S]);  d = (-(iBu * (D*D)) + 2) + 2;  a = n / d
 *             product build: n = fma(-(D*D), b, a[E] + a[W]);  n = n + (a[N] + a[S]);  a = n * (1 / fma(-iBu, D*D, 4))
 *   residual: r = b - iBu * a;  r = r + ((a - a[W]) / D - (a[E] - a) / D) / D;  r = r + ((a - a[S]) / D - (a[N] - a) / D) / D
 *             product build: r = fma(-iBu, a, b) and multiplications by 1 / D for the divisions
 *   A stratification that varies from column to column reads iBu per cell; on the coarse levels it is the mean of the 4 children, level
 *   by level (poisson()'s restriction({alpha, lambda})), built by the first modal solve after a msom_modes_compute (a handle
 *   that only decomposes does not hold it; "modes_bytes" does not count it: 4/3 * 8 nl ny nx more) and dropped with the modes. */
int msom_modes_mgstats(msom_t *m, int mode, msom_mgstats *st);

/* ---- isotropic wavenumber spectra and spectral fluxes on the device: get_spec_2D, radial_average / get_spec_1D and get_flux of
 * msqg/scripts/fftlib.py, as msqg/scripts/spectra.py:113-142 (KE / PE spectra) and energy_offline.py:119-124 (fluxes of the budget terms)
 * use them on .bas files.  The contract is fftlib.py in exact arithmetic, restated with integers so that it does not depend on how fftfreq
 * rounds.  D = Delta, nmax = max(nx, ny), sx = nmax / nx, sy = nmax / ny; signed wavenumber indices i = -nx/2 .. nx/2 - 1,
 * j = -ny/2 .. ny/2 - 1; R2(i, j) = (i sx)^2 + (j sy)^2.
 *   spec_2D(i, j) = Re(A(i, j) conj B(i, j)) D^4 with A = fft2(a), unnormalised (fftlib.py:44-47)
 *   nbins = nmax / 2 - 2, dk = 1 / (nmax D), kr[r] = (r + 1) dk, r = 0 .. nbins - 1 (:20-33)
 *   bin r holds the points with r^2 <= R2 <= (r + 1)^2, both ends inclusive as :13 (a point on a circle of integer radius counts in two
 *     bins); count[r] is their number
 *   spec[l][r] = 2 pi kr[r] (sum over bin r of spec_2D) / count[r]                                  (:15-16)
 *   flux[l][r] = (sum over (r + 1)^2 <= R2 of spec_2D) dkx dky, dkx = 1 / (nx D), dky = 1 / (ny D)    (:71-74; dk^2 on the square)
 *   On the square this is the reference; the rule for nx != ny is this library's extension, like the key Ny.  With L0 = 1 the reference's
 *   floating-point membership test agrees with the integer rule in every cell for N = 8 .. 256; with other L0 the reference itself moves
 *   points across bin edges by rounding.
 * Arrays: a, b [layers][ny][nx] fp64, host or device pointers, a == b allowed; out [layers][ny][nx], host or device; spec, flux, ke, pe, kr
 *   host pointers; either of spec / flux and either of ke / pe may be NULL.
 * msom_spec_layout: host code only, no handle and no GPU: nbins and (count != NULL) count[nbins].  A side that is no power of two, below 8
 *   or above 32768: MSOM_ERR_CONFIG.
 * msom_spec_bins: nbins of the handle's grid.  msom_spec_kr: kr[nbins].
 * msom_spec_2d: spec_2D, fftshift-ed: index 0 is the most negative wavenumber on both axes.  The one call that stores the plane.
 * msom_spec_cross: spec and / or flux, [layers][nbins].
 * msom_spec_fields: msom_spec_cross on two of the handle's fields, which must have the same layer count; MSOM_PSI with MSOM_DE_* gives the
 *   budget fluxes of energy_offline.py (the sign of -p is the caller's: the result is linear in each argument).  Nothing leaves the device
 *   but [layers][nbins] numbers.
 * msom_spec_energy: from the handle's MSOM_PSI with the ghost values boundary() left there, u, v as the msom_stats_* block defines them,
 *   dhc_l = 0.5 (dh_l + dh_l+1):  ke[l][r] = 0.5 (spec(u_l, u_l) + spec(v_l, v_l))[r] dh_l, [nl][nbins];
 *   pe[l][r] = 0.5 spec(g_l, g_l)[r] dhc_l with g_l = sqrt(S_l) (psi_l+1 - psi_l) / dhc_l and S = MSOM_S, [nl - 1][nbins] (spectra.py:113-139;
 *   b Fr there is g because S = (Fr / Ro)^2).  nl = 1: pe is not touched.
 * Arithmetic: a pair of real fields goes through one complex transform (Z = fft2(a + i b): Re(A conj B)(k) = Im(Z(k) Z(-k)) / 2 and
 *   |A|^2 + |B|^2 = (|Z(k)|^2 + |Z(-k)|^2) / 2; a == b and the auto-spectra take a + 0 i).  Twiddle factors come from a table computed on
 *   the host in long double and rounded once.  The transform's own arithmetic is free in both builds (the results are not bit-comparable
 *   with another FFT); bin and flux sums are two-stage sums in a fixed order, no atomics: two calls on the same data return the same bits.
 * Scope: an msqg operator on one tile: a handle of msom_create_tiled with more than one rank answers MSOM_ERR_CONFIG.  Sides: powers of
 *   two, 8 .. 4096 in any combination (a line of the transform lives in LDS); anything else MSOM_ERR_CONFIG.
 * Errors: null handle, null a / b / out / kr, layers < 1, both results NULL, an unknown field id or two fields of different layer counts:
 *   MSOM_ERR_ARG; before msom_set_const: MSOM_ERR_STATE.
 * Memory: the work arrays (two complex copies of a batch of layers, spec_2D of the half plane, the sums; a batch is as many layers as fit
 *   1 GiB, at least one) are allocated by the first call, dropped by msom_set_const and freed by msom_destroy; msom_get_param "spec_bytes"
 *   reports them (0 on a handle that has not called a spectrum function since msom_set_const), "spec_batch" the layers of a batch.
 *   Every call synchronises the stream and changes nothing in psi, q, dt, mgstats or any field.
 * msom_bench_kernel names "spec_rows", "spec_transpose", "spec_cols", "spec_shells": the passes on one batch of layers of u + i v. */
int msom_spec_layout(int nx, int ny, int *nbins, long *count);   /* host only: no handle, no GPU */
int msom_spec_bins(msom_t *m);                                    /* nbins, or an error code < 0 */
int msom_spec_kr(msom_t *m, double *kr);                          /* [nbins] host */
int msom_spec_2d(msom_t *m, const double *a, const double *b, int layers, double *out);
int msom_spec_cross(msom_t *m, const double *a, const double *b, int layers, double *spec, double *flux);
int msom_spec_fields(msom_t *m, int field_a, int field_b, double *spec, double *flux);
int msom_spec_energy(msom_t *m, double *ke, double *pe);

/* ---- time loop of Basilisk predictor-corrector run() as driven by msqg/qg.c
 * msom_step: one RK2 step on the internal state (update, dtnext, advance dt/2, update,
 * advance dt).  msom_set_tnext gives the time of the next t-scheduled event (output). */
int msom_step(msom_t *m, double *dt_used);
int msom_set_tnext(msom_t *m, double tnext);
double msom_time(msom_t *m);
int msom_iter(msom_t *m);
/* kinetic-energy diagnostic of the per-step stdout line, msqg/qg.c:101-109 */
double msom_ke(msom_t *m);
int msom_last_mgstats(msom_t *m, msom_mgstats *st);
/* msom_run: whole main() loop of msqg/qg.c:34-173 (stdout line, po/qo .bas every dtout,
 * outdir_%04d creation, params.in backup).  nsteps_max < 0: run to tend. */
int msom_run(msom_t *m, const char *workdir, long nsteps_max);
/* lossless fp64 checkpoint and bit-exact restart of a msom_t, and the options "ckpt_steps" / "resume" of this loop: msom_state.h */

/* ---- .bas IO, msqg/auxiliar_input.h:24-59 (input_matrixl), :101-167 (output_matrixl, write_field) */
/* tiled models: msom_write_* / msom_read_* / msom_read_inputs / msom_run are collective (every rank calls them): the
 * global field is gathered and rank 0 writes; every rank reads the shared file and keeps its tile */
int msom_write_bas(msom_t *m, int field, const char *path);
int msom_read_bas(msom_t *m, int field, const char *path);

/* ---- NetCDF-3 classic output / restart (libnetcdf-free): create_nc + write_nc + read_nc of
 * newqg/netcdf_bas.h:42-244 and qg-node/netcdf_vertex_bas.h:315-424.  msom_write_nc appends one
 * record (time = t; variables "psi" and "q", all levels, float) to `path`, creating the file
 * with dims level,y,x,time(UNLIMITED) and coordinate variables time,y,x when it does not exist.
 * msom_read_nc loads record `record` (-1 = last) of variable `varname` into `field`
 * (restart: "psi" -> MSOM_PSI, then msom_set_const). */
int msom_write_nc(msom_t *m, const char *path);
int msom_read_nc(msom_t *m, int field, const char *path, const char *varname, int record);

/* ---- wavelet scale filter, the "multiple scale" part of msom (msqg/qg.h:509-560; event filter :655-658;
 * coefficients sig_lev from sig_filt = min(afilt * Rd, Lfmax), :1059-1090).  Saves q in tmp, inverts
 * q -> psi, removes from every layer of psi the wavelet details selected by sig_lev, recomputes q and
 * sets qof = (q_before - q_after) / dtflt; dtflt < 0 (energy diagnostics, qg_energy.h:213) restores q.
 * Single tile or tiles (the pyramid levels above those that hold a cell of every tile are gathered on every rank). */
int msom_wavelet_filter(msom_t *m, double dtflt);
/* ---- energy / PV budgets, msqg/qg_energy.h (params key ediag: -1 off, 0: terms x (-psi), 1: PV terms).
 * msom_energy_tend = energy_tend (:227-241, event comp_diag :289-291): accumulates de_j1/j2/j3, de_vd,
 * de_bf from the current psi with weight dt and updates the running mean po_mft; msom_filter_de =
 * filter_de (:208-225) with po_mft = field `pm_field`; msom_reset_de zeroes the six budgets
 * (msqg/qg.c:153-159); pystep_de = the Python entry point (:296-349, msqg/qg_energy.i:31), same
 * argument order (+ handle).  msom_run drives the events and writes de_*%09d.bas (qg.c:131-160). */
int msom_energy_tend(msom_t *m, double dt);
int msom_filter_de(msom_t *m, int pm_field, double dtflt);
int msom_reset_de(msom_t *m);
int pystep_de(msom_t *m, const double *po_py, int len1, int len2, int len3, double *de_bf_py, int len4, int len5, int len6,
              double *de_vd_py, int len7, int len8, int len9, double *de_j1_py, int len10, int len11, int len12,
              double *de_j2_py, int len13, int len14, int len15, double *de_j3_py, int len16, int len17, int len18,
              double *de_ft_py, int len19, int len20, int len21, int onlyKE);

/* pieces for the parity tests: number of pyramid levels (level 0 = finest ... 1 x 1 cell), sig_lev of
 * one level [ny>>level][nx>>level], and the bare transform-scale-inverse applied to a field */
int msom_dbg_wavelet_levels(msom_t *m);
int msom_dbg_siglev(msom_t *m, int level, double *out);
int msom_dbg_wavelet_apply(msom_t *m, int field);

/* ---- the newqg dialect: the cell-centred, dimensional one-layer model of newqg/qg.h with the optional Helmholtz ("1.5-layer")
 * inversion, on a msom_t.  msom_create_newqg parses a params.in of that model, msom_create_newqg_str the same text from memory; NULL on
 * error.  One tile, one layer.
 * Keys (newqg/extra.h:42-58): N nl L0 DT CFL TOLERANCE f0 beta hEkb tau0 nu gp_low sbc tend dtout dh; extension keys Ny NITERMAX NITERMIN
 *   as in msom_create.  Defaults newqg/qg.h:85-94 and the Basilisk globals: f0 = 1, dh = [1], tend = dtout = 1, N = 64, L0 = 1, DT = 1e10,
 *   CFL = 0.5, TOLERANCE = 1e-3, everything else 0.  Line rules as msom_create.  Derived: nu != 0: DT = 0.5 * min(DT, sq(L0/N) / nu / 4)
 *   (extra.h:71); bc_fac = sbc / ((0.5*sbc + 1) * sq(L0/N)) (qg.h:295); iRd2_low = gp_low != 0 ? -(f0*f0) / (gp_low * dh[0]) : 0
 *   (qg.h:348-354, a uniform field there).  nl != 1 ("to be updated for multi layer", qg.h:347), N or Ny not a power of two >= 2,
 *   dh[0] == 0, sbc < 0 other than -1 (the reference installs its wall conditions for sbc >= 0 only, qg.h:303): MSOM_ERR_CONFIG (NULL,
 *   message in msom_last_error).  tau0 is parsed and reported only: the reference uses it in the
 *   driver's sample forcing alone (newqg/qg.c:69-75).
 * msom_get_param: model (1 on such a handle, 0 on every other), N nx ny nl L0 DT CFL TOLERANCE tend dtout f0 beta nu hEkb tau0 gp_low sbc
 *   bc_fac iRd2_low dh_0 nlevels, and the options nq_fused nq_adv_fused nq_rows (nq_rows: the chunk height a launch takes).
 * Fields: MSOM_PSI, MSOM_Q, MSOM_ZETA, MSOM_DQ, MSOM_QPRED, MSOM_QFORC, one layer each; every other id: MSOM_ERR_ARG from
 *   msom_set_field / msom_get_field, 0 from msom_field_layers.
 * Boundary conditions (qg.h:303-319; sbc = -1: periodic(right), periodic(top), newqg/qg.c:33-36): psi dirichlet(0), ghost = -interior,
 *   corners by the y rule over the x-ghost column; zeta and q ghosts bc_fac * (psi[interior] - psi[ghost]) -- 0 with sbc = 0 -- and a
 *   corner ghost is that y rule on the x-ghost column, bc_fac * (psi[x-ghost, interior row] - psi[corner ghost]); sbc = -1: wrapped copies.
 * Calls:
 *   msom_set_const (qg.h:345-358): q = comp_q(psi), boundary fill; time = 0, iteration = 0, the limiter's previous = 0 (the static of
 *     qg.h:203 at the start of a run).  Every call below needs it first: MSOM_ERR_STATE otherwise (msom_update: that code as its value).
 *   msom_comp_q (:184-189): q = lap(psi); gp_low != 0: q = q + iRd2_low * psi.
 *   msom_invertq (:148-157): poisson(psi, q, lambda = iRd2_low): the multigrid of the modal inversion above with ONE problem,
 *     iBu := iRd2_low, a = MSOM_PSI in place (warm start and result; there is no mode-space field), b = q, no projections, psi's boundary
 *     fill after the last correction; relax / residual expression orders as documented there (Basilisk's poisson() relax and residual,
 *     text mspg/elliptic.h:262-350).  mgstats of the one problem: i, nrelax from 4 by the 1.2 / 10 rule, resb, resa, sum.  gp_low = 0 is
 *     plain Poisson; doubly periodic with gp_low = 0 needs zero-mean q.
 *   msom_update (:264-284): solve, tendency into MSOM_ZETA (always stored: update_qg leaves lap(psi) there) and MSOM_DQ, and the
 *     limiter of advection_pv :202-219, applied ONCE per update with one `previous` (max|u| over the faces from a pass over psi:
 *     D / max|u| is the minimum over the faces of D / |u| exactly).  Returns the new dtmax.
 *   msom_advance (:249-261): qo = qi + dq * dt.
 *   msom_step, msom_set_tnext, msom_time, msom_iter: one iteration of the predictor-corrector run() as msom_step above (dtnext, update,
 *     advance dt/2, update, advance dt); `previous` moves in the second update too; synchronous.
 *   msom_ke: sum -0.5 * psi * lap(psi) * Delta^2 (newqg/qg.c:89-91), deterministic two-stage sums.
 *   msom_last_mgstats, msom_write_nc / msom_read_nc (the format is newqg/netcdf_bas.h), msom_profile_read ("rhs", "helm_relax",
 *     "helm_residual", "helm_coarse") / msom_profile_reset, msom_sync, msom_dbg_nlevels / msom_dbg_level_dims, msom_destroy;
 *     msom_bench_kernel: "nq_rhs" (tendency + advance), "nq_rhs_dq", "helm_sweep", "helm_residual"; a measurement, not an operator: it
 *     overwrites MSOM_ZETA, MSOM_DQ and MSOM_QPRED of the handle and the solver's work arrays (psi and q stay).
 *   Forcing: surface_forcing is a prototype the driver fills in (:246); here it is the handle's MSOM_QFORC: once set, dq = dq + qforc as
 *     the last term.  The driver's time-dependent sample expression and its noise() start are the caller's.
 * Options: TOLERANCE NITERMAX NITERMIN DT quiet profile; nq_fused [1] (0: the tendency as one launch per reference loop, the validation
 *   chain; same bits in the strict build), nq_adv_fused [1] (the advance folded into the tendency pass, dq then not stored by
 *   msom_step), nq_rows [0 = automatic] chunk height of the fused kernel.  Any other key: MSOM_ERR_ARG.
 * Every other entry point of this header that takes a msom_t * (msom_run, pystep_*, pyq2p / pyp2q, msom_bfn_*, msom_stats_*,
 *   msom_time_filter, msom_modes_*, msom_spec_* with a handle, msom_wavelet_filter, the energy budgets, .bas IO, msom_read_inputs, msom_remove_mean, msom_tile_info,
 *   msom_dbg_relax / _residual / _helm_* / _restrict / _prolong / _op / _wavelet_* / _siglev) is an msqg operator and answers such a handle
 *   with MSOM_ERR_CONFIG, a message naming the call, and no change to its fields.  msom_create_tiled has no newqg form.
 * Expression order of the tendency (the contract of the strict build: true divisions, no contraction; it is how the C of
 *   newqg/qg.h:125-141,164,200,229,240,258 parses; E / W = x +- 1, N / S = y +- 1, D = Delta):
 *   z    = ((((pE + pW) + pN) + pS) - 4*p) / (D*D)                       (the 0*zeta_old of comp_del2(.., 0., 1.) is dropped)
 *   J    = ((pE-pW)*(zN-zS) + (pS-pN)*(zE-zW) + pE*(zNE-zSE) - pW*(zNW-zSW) - pN*(zNE-zNW) + pS*(zSE-zSW)
 *           + zN*(pNE-pNW) - zS*(pSE-pSW) - zE*(pNE-pSE) + zW*(pNW-pSW)) / ((12.*D)*D)      summed left to right
 *   dq   = 0 + ((-J) - (beta*(pE - pW)) / (2*D))                         (the += on the zeroed updates, :267-270,200)
 *   dq   = dq + nu * (((((zE + zW) + zN) + zS) - 4*z) / (D*D))
 *   dq   = dq - ((hEkb*f0) / (2*dh0)) * z                                (coefficient formed once on the host)
 *   dq   = dq + qforc                                                    (only if MSOM_QFORC was set)
 *   qout = qin + dq*dt
 *   Product build: reciprocals of D*D, (12 D) D and 2 D formed once on the host; the Jacobian one chain of fused multiply-adds in the
 *   order above, z and lap(z) as fma(-4, c, sum) * (1 / (D*D)), and dq = fma(nu, lap z, dq), fma(-cek, z, dq), qout = fma(dq, dt, qin). */
msom_t *msom_create_newqg(const char *params_path);
msom_t *msom_create_newqg_str(const char *params_text);

/* select the HIP device of the calling thread before msom_create* (one process per GPU:
 * device = LOCAL_RANK) */
int msom_set_device(int device);

/* ---- multi-GPU tiling (replaces Basilisk's MPI layer: boundary() halo exchange and
 * foreach(reduction)).  One process per GPU; the 2-D domain is a px x py grid of
 * equal tiles; rank r owns tile (r % px, r / px).  id128 is the 128-byte ncclUniqueId made by
 * msom_comm_unique_id on rank 0 and distributed by the caller (e.g. torch.distributed). */
int msom_comm_unique_id(void *id128);
msom_t *msom_create_tiled(const char *params_text, int px, int py, int rank, const void *id128);
int msom_tile_info(msom_t *m, int *px, int *py, int *ix, int *iy, int *nx_local, int *ny_local);

/* ---- debug / test hooks (used by tests/ to compare single kernels with the oracle) */
int msom_dbg_nlevels(msom_t *m);
int msom_dbg_level_dims(msom_t *m, int lev, int *nx, int *ny);
int msom_dbg_relax(msom_t *m, int lev, double *da, const double *res, int nsweeps);
int msom_dbg_residual(msom_t *m, const double *a, const double *b, double *res, double *maxres);
/* QPRED = Q + dt dq in one tendency pass, then the first residual of its inversion on levels 0 and 1 (raw split arrays of
   msom_get_param("split_ls_0") / ("split_ls_1") doubles per layer, "split_rp_<k>" per row of two half rows, each with "split_pad" pad
   doubles on either side; NaN where nothing was written), max|res| and the sum of QPRED:
   fused != 0: out of the pass itself (option rhs_resid), 0: from the solver's residual pass */
int msom_dbg_rhs_resid(msom_t *m, int fused, double dt, double *res0, double *res1, double *maxres, double *bsum);
/* the modal solver's kernels (need the modes: computed if not ready).  da, res: [mode][y][x] of level `lev`; nhalf half-sweeps starting
 * with colour 0 (half-sweep h is sweep h / 2); count_per_mode[m] = sweeps mode m takes (NULL: every mode takes all), a mode whose
 * count is used up keeps its da.  a, b, res: [mode][ny][nx]; maxres_per_mode: nl maxima of |res_m| */
int msom_dbg_helm_relax(msom_t *m, int lev, double *da, const double *res, int nhalf, const int *count_per_mode);
int msom_dbg_helm_residual(msom_t *m, const double *a, const double *b, double *res, double *maxres_per_mode);
int msom_dbg_restrict(msom_t *m, int lev_fine, const double *fine, double *coarse);
int msom_dbg_prolong(msom_t *m, int lev_coarse, const double *coarse, double *fine);
int msom_dbg_op(msom_t *m, const char *op, int f_in, int f_out, double add, double fac);

/* ---- measurement: average HIP-event duration (events recorded on the library's own stream while the option
 * "profile" is on, i.e. inside the timed steps) of the finest-level launches named
 *   "sweep" (red + black half-sweep pair), "march2" / "march3" / "march4" (passes of K chained half-sweeps),
 *   "march_pl" (first pass of a level visit: prolongation + K half-sweeps), "march_corr" (last pass of the cycle: K half-sweeps
 *   + correction), "resid_max" (max|res|, max|u| of the corrected psi),
 *   "red_prolong" (first red half-sweep + prolongation), "resid_restrict" (pre-cycle residual + restriction),
 *   "resid_correct" (correction + residual + max|u|), "residual" (both of the former), "rhs" (fused PV tendency
 *   [+ advance] pass), "block2";
 * and a back-to-back kernel microbenchmark outside any step */
int msom_profile_read(msom_t *m, const char *kernel, double *avg_ms, long *launches);
int msom_profile_reset(msom_t *m);
/* waits for everything the handle has queued on its stream.  With option "step_sync" = 0 (default -1: on grids below 2^23 cell-layers;
 * 1: never) and "async_solve", msom_step returns while its last tendency pass is still running; every call that returns device data
 * to the host synchronises by itself, so this is for timing and for callers that share the fields' device pointers with their own streams.
 * Where option "rhs_close" resolves to 2 (msom_get_param) the second stage's tendency pass also produces the residual that decides the
 * step, msom_step waits for it and "step_sync" = 0 leaves no pass running. */
int msom_sync(msom_t *m);
int msom_bench_kernel(msom_t *m, const char *kernel, int reps, double *avg_ms);
/* one-rank RCCL communicator on the current device: grouped send/recv to self, all-reduce and
 * all-gather through the library's transport code (wiring check on a single GPU) */
int msom_dbg_rccl_selftest(void);

/* ======================================================================================
 * Vertex-grid (masked-domain) variant: qg-node/qg.h + qg_baroclinic_ms.h (nl >= 2) /
 * qg_barotropic.h (nl = 1) + nodal-poisson.h + my_vertex.h, driver qg-node/qg.c.
 * Unknowns on the (N+1)^2 vertices; field arrays are fp64 [layer][N+1][N+1]
 * (qg-node/netcdf_vertex_bas.h:253), host or device pointers.  Single GPU.
 * ====================================================================================== */
enum {
  MSOMN_PSI = 0,   /* psi       stream function                           qg-node/qg.h:130 */
  MSOMN_Q = 1,     /* q         potential vorticity (evolving)            qg.h:131         */
  MSOMN_ZETA = 2,  /* zeta      relative vorticity                qg_baroclinic_ms.h:32   */
  MSOMN_TMP = 3,   /* tmp                                                                  */
  MSOMN_PSIPG = 4, /* psi_pg    large-scale stream function                                */
  MSOMN_S2 = 5,    /* S2        N^2 before, f^2/N^2 after set_const; nl-1 layers           */
  MSOMN_TOPO = 6,  /* topo      1 layer                                                    */
  MSOMN_QFORC = 7, /* q_forcing 1 layer                                   qg.h:133         */
  MSOMN_MASK = 8,  /* mask      1 inside / 0 land and boundary, 1 layer   qg.h:134         */
  MSOMN_DQ = 9,    /* updates                                                              */
  MSOMN_QPRED = 10,/* predictor                                                            */
  MSOMN_QFORC3D = 11, /* q_forcing_3d (-DFORCING_3D, qg_baroclinic_ms.h:25,179-185): added to every layer once set */
  /* surface-QG variant (params key sqg = 1): the finished parts of qg-node/sqg_baroclinic_ms.h -- comp_stretch with the
   * surface buoyancy :77-98, idh0[0] = 1/dh[0] :502, S2 of the surface = f/N2[0] :545, tmp boundary rule :64-67,
   * laplacian(bs) in both dissipation operators :160-201.  That file stops at "TODO: STOPPED HERE" (:222) and does not
   * compile; bs is therefore a prescribed field (its tendency rhs_bs is unfinished there), comp_q / invert_q are completed
   * consistently with comp_stretch */
  MSOMN_BS = 12,   /* bs        surface buoyancy, 1 layer                                  */
  MSOMN_S2S = 13,  /* S2 of the surface: N2[0] before, f/N2[0] after set_const, 1 layer    */
  MSOMN_PSIF = 14, /* psi_f     running mean of the part the wavelet filter removes (qg_baroclinic_ms.h:30,384) */
  MSOMN_NFIELDS = 15
};
typedef struct msomn msomn_t;

/* read_params (qg-node/extra.h:83-116, key list qg.c:72-107) + init_grid + set_bc/set_vars
 * (qg.h:404-459, qg_baroclinic_ms.h:400-447): mask = 1 inside and 0 on the boundary
 * vertices, S2 = N2[l], everything else 0.  Extension: none.  NULL on error. */
msomn_t *msomn_create(const char *params_path);
msomn_t *msomn_create_str(const char *params_text);
/* Vertex model on tiles.  The global grid of N x N cells is covered by px x py tiles (powers of two, px != py allowed), rank r = tile
 * (r % px, r / px) as msom_create_tiled; id128 from msom_comm_unique_id (in-process transport if it starts with "MSOMLOCL", RCCL
 * otherwise).  A tile of Tx = N / px by Ty = N / py cells HOLDS (Tx + 1) x (Ty + 1) vertices, the ones on its interior edges too: a
 * vertex on a shared edge exists on both tiles (on all four at a cross point) and every holder computes it.  The result equals the
 * single tile's of the same global grid bit for bit (dt, t, iter, mgstats identical on all ranks; msomn_ke and msomn_diag1d differ in
 * their summation order only).  msomn_set_field / msomn_get_field take and return the tile's [layers][Ty + 1][Tx + 1]; the caller
 * gives shared vertices the same values on every holder (not checked).  msomn_set_field, msomn_set_const and every call that
 * computes are COLLECTIVE: all ranks call them, in the same order.  Everything that depends on x or y uses the global vertex index.
 * px = py = 1 gives the plain handle.  NULL with msom_last_error set for px / py not a power of two, N not divisible, a tile side
 * below 2 cells, a bad rank, bc_fac = -1.  sqg = 1 runs on tiles as on one (S2S takes f at the global row; laplacian(bs) copies at walls
 * of the domain only and reads the halo of bs on an interior edge).
 * On more than one tile the multigrid levels down to the gather level (msomn_get_param "agg_level": the first level of at most
 * max(mg_coarse, px, py) cells a side, at least level 1) live on the tiles, the coarser ones are gathered and solved on every rank;
 * set option mg_coarse before msomn_set_const.  The fused passes resolve to off (options node_pfused, node_tile_s, node_march_s,
 * node_march, tiled_relax, node_corr_fused, node_rhs_fused read 0 and stay 0); msomn_get_param "exchanges" counts halo exchanges.
 * msomn_dbg_relax / _residual / _restrict / _prolong / _level_mask work on the tiled levels with tile-sized arrays (a gathered
 * level: MSOM_ERR_ARG).  Refused with MSOM_ERR_CONFIG and a message naming the call, the handle unchanged: msomn_dbg_del2_zeta; unless
 * the option io_tiles is 1: msomn_run, msomn_write_nc, msomn_read_nc, msomn_state_save / _load; and, unless the option wavelet_tiles is
 * 1: option stochastic, msomn_noise_draw, msomn_dbg_noise, msomn_dbg_csig, msomn_wavelet_filter, msomn_dbg_wv_get / _apply.
 * Option io_tiles [0] (0 or 1, else MSOM_ERR_ARG; on one tile accepted, no effect): with 1 those five calls are COLLECTIVE.  A tile
 * OWNS its local columns 0 .. Tx - 1, and column Tx too iff it is the last tile of its row of tiles, rows likewise: every global
 * vertex is owned once.  Save and write_nc gather the owned windows and rank 0 writes the global arrays -- the files equal the single
 * tile's byte for byte; load and read_nc: every rank reads the shared file and takes its window, shared vertices and halos included; a
 * state file of any tiling loads on any other (include/msomn_state.h).  What one rank alone can see (rank 0's write, a short read)
 * ends in one all-reduce: every rank returns the same code, the rank that saw the cause carries the message, the handle stays as it
 * was.  msomn_run: rank 0 alone makes the output directory, prints and writes; it needs msomn_set_const or a state.msom to resume
 * from (MSOM_ERR_STATE otherwise: the driver's cold start draws from the process-wide rand()), and wavelet_tiles = 1 when dtflt > 0.
 * Option wavelet_tiles [0] (0 or 1, else MSOM_ERR_ARG; on one tile accepted, no effect): with 1 those calls, and msomn_step /
 * msomn_advance with the stochastic forcing, run on the tiles as COLLECTIVE calls with the single tile's bits.  The cell pyramids
 * then hold the tile's window of (Tx >> k) x (Ty >> k) cells on the levels k < agg_level and the global level of (N >> k)^2 cells on
 * every rank from agg_level on: msomn_dbg_noise and msomn_dbg_wv_apply take and give the tile's window [Ty][Tx] of cells,
 * msomn_dbg_csig and msomn_dbg_wv_get the window below agg_level and the whole level from it on.  A transform posts 2 agg_level - 1
 * halo exchanges and one all-gather.  noise_mode = 0 stays refused on more than one tile wherever a draw would be taken (the host's
 * rand() stream is one state per process and cannot be shared by tiles): set noise_mode = 1. */
msomn_t *msomn_create_tiled(const char *params_text, int px, int py, int rank, const void *id128);
/* msomn_create_tiled of the params text in a state file (include/msomn_state.h), io_tiles = 1, wavelet_tiles = 1 if the file is
 * stochastic or holds psi_f, the options the file records, msomn_state_load.  Collective; NULL on the errors of either call. */
msomn_t *msomn_create_tiled_from_state(const char *path, int px, int py, int rank, const void *id128);
int msomn_tile_info(msomn_t *m, int *px, int *py, int *ix, int *iy, int *nx_local, int *ny_local);  /* vertices: Tx + 1, Ty + 1 */
void msomn_destroy(msomn_t *m);                                 /* trash_vars qg.h:537-544 */
/* keys: TOLERANCE NITERMAX NITERMIN (nodal-poisson.h:19-23) DT quiet wavelet_tiles [0] io_tiles [0] (both: msomn_create_tiled above) stochastic seed (kept in the handle, and srand) noise_mode [0] (0: the
 * noise is drawn from the serial rand() stream on the host, 1: on the device by k_n_noise; other values: MSOM_ERR_ARG); implementation switches (result-preserving in
 * the strict build): node_split [65] levels of >= that many vertices a side keep correction / residual / mask / S2 copies in the
 * x-parity split layout (0: off), s2_rows [1] row tables for an S2 that does not depend on x, node_pfused [1] prolongation folded into the first colour pass of the split levels, mg_coarse [32] levels of at most that
 * many cells a side in one launch, tiled_relax [0], node_march [0] (measured slower, kept for the tests), node_march_rows [0 = automatic] chunk height of the marching passes; round 3: node_march_s [2049] split
 * levels of >= that many vertices a side chain up to 4 colour half-sweeps per pass (node_march_tail1 [1]: 9 half-sweeps as 4 + 4 + a colour
 * launch, 0: 4 + 3 + 2), node_tile_s [65] / node_tile_max [513] / node_tile_k [8]
 * the split levels between those sizes run up to node_tile_k colour half-sweeps per LDS-tiled launch (nl <= 4), node_rhs_fused [1] the
 * baroclinic tendency in three passes instead of the twelve loops of the reference, node_corr_fused [2] the correction of a cycle applied
 * inside the residual pass of the next (2: rows marched, 1: one thread per vertex, 0: separate passes), profile [0] */
int msomn_set_option(msomn_t *m, const char *key, double value);
/* keys: N nl L0 DT tend dtout nlevels iRd2_low bc_fac idh0_<l> idh1_<l>, the options node_march_s node_march_rows noise_mode seed,
 * noise_draw (number of the next draw of the device generator; msomn_set_const: 0); NaN if unknown.
 * The paths the solve takes (after msomn_set_const), each from the same function the dispatch calls: sqg, s2_xuniform (S2 does not
 * depend on x: row tables), split_<k> (level k in the x-parity split layout), node_march_kmax (K cap of the chained split pass
 * k_n_relax_march_s: 4 for nl <= 4, 3 for nl 5-6, 0 where it cannot run: nl > 6 or no row tables), relax_path_<k> (level k's sweeps:
 * 0 natural colour passes, 1 split colour passes, 2 LDS-tiled split passes k_n_relax_tile_s (taken for 2 sweeps or more), 3 chained
 * split passes, 4 inside the one-launch coarse group k_n_mg_coarse, 5 option node_march, 6 option tiled_relax), corr_march (1: the
 * correction rides in the next residual pass as rows marched by k_n_correct_residual_m) */
double msomn_get_param(msomn_t *m, const char *key);
int msomn_field_layers(msomn_t *m, int field);
int msomn_set_field(msomn_t *m, int field, const double *a);   /* a: [layers][N+1][N+1] */
int msomn_get_field(msomn_t *m, int field, double *a);
/* init events: layer metrics + S2 = f^2/N^2 + topo scaling (qg_baroclinic_ms.h:449-510),
 * iRd2_low (qg_barotropic.h:115-118), mask and S2 on every multigrid level, DT limits and
 * q = comp_q(psi) (set_const, qg.h:465-524).  psi, S2 (= N^2), mask, topo, psi_pg must be
 * set before; restart / input files are the driver's business (msomn_run). */
int msomn_set_const(msomn_t *m);
/* update_qg (qg.h:334-354): invert_q + rhs_pv + adjust_dt; *dt_out = new time step */
int msomn_update(msomn_t *m, int qfield, int dqfield, double dtmax, double *dt_out);
int msomn_advance(msomn_t *m, int out, int in, int dq, double dt);        /* advance_qg qg.h:291-302 */
int msomn_invert_q(msomn_t *m, int qfield, msom_mgstats *stats);           /* qg_baroclinic_ms.h:217-225 */
int msomn_comp_q(msomn_t *m, int psifield, int qfield);                    /* :199-211 / qg_barotropic.h:32-39 */
int msomn_rhs_pv(msomn_t *m, int qfield, int dqfield);                     /* :104-196 / qg_barotropic.h:16-29 */
int msomn_forcing(msomn_t *m);                                             /* event forcing, qg.c:136-145 */
/* events of iteration i (forcing if with_forcing_event), then one predictor-corrector step of run() */
int msomn_step(msomn_t *m, int with_forcing_event);
int msomn_set_tnext(msomn_t *m, double tnext);
double msomn_time(msomn_t *m);
double msomn_dt(msomn_t *m);
int msomn_iter(msomn_t *m);
int msomn_ke(msomn_t *m, double *ke);                                      /* event writestdout qg.c:171-178 */
int msomn_last_mgstats(msomn_t *m, msom_mgstats *stats);
/* Running time means and eddy statistics of the vertex model on the device: the twin of msom_stats_* above, with its ids (MSOM_ST_*,
 * no second enum): the accumulators MSOM_ST_PSI .. MSOM_ST_VQ (bit k of the mask = accumulator k) and the derived MSOM_ST_EKE,
 * MSOM_ST_UQ_EDDY, MSOM_ST_VQ_EDDY.  MSOM_ST_QME is not offered (MSOM_ERR_ARG): the vertex model's running mean is psi_f.
 * One sample reads MSOMN_PSI, MSOMN_Q and MSOMN_MASK as the handle holds them; for every held vertex and layer, in this expression
 *   order (the strict build's contract; the product build multiplies by 1 / (2 Delta) and contracts): acc = acc + w * x with x = psi,
 *   q, psi*psi, q*q, 0.5 * (u*u + v*v), u*q, v*q, where u = ((psi[j-1][i] - psi[j+1][i]) / (2 Delta)) * mask[j][i] and
 *   v = ((psi[j][i+1] - psi[j][i-1]) / (2 Delta)) * mask[j][i]; on a vertex of the DOMAIN boundary (global i or j equal to 0 or N)
 *   u = v = 0 and the neighbour beyond the wall is not read; on a tile's interior edge the neighbour is the halo.  W = W + w.
 *   No atomics, no reductions: the same bits on every run, and every holder of a shared vertex accumulates the same bits.
 * msomn_stats_begin allocates the selected arrays only, zeroes them and W, restarts the counts, and may be called again;
 *   msomn_set_const drops everything; a handle that never calls it allocates nothing.
 * msomn_stats_accumulate: one sample by hand; on tiles it exchanges the halo of psi first (collective).
 * msomn_stats_get: `which` < MSOM_ST_NACC: S / W (a true division in both builds).  Derived ids: the mean psi goes into the scratch
 *   field MSOMN_TMP, its sides get the boundary rule of psi, on tiles its halo is exchanged (collective), um and vm are the same masked
 *   differences, and EKE = S_KE/W - 0.5 * (um*um + vm*vm), UQ_EDDY = S_UQ/W - um * (S_Q/W), VQ_EDDY = S_VQ/W - vm * (S_Q/W); nothing
 *   derived is stored.  out: the tile's [nl][Ty+1][Tx+1] as msomn_get_field, host or device pointer.
 * Option "stats" [0] = 1: msomn_step (and so msomn_run) queues one sample right after stage 1's update, before the first advance: q is
 *   q_n, psi what stage 1 inverted from it (masked, sides set, on tiles already exchanged by the tendency: no further exchange), the
 *   weight the dt the step then uses.  "stats_every" [1] = n: only every n-th step since msomn_stats_begin.  msomn_update,
 *   msomn_advance and msomn_invert_q on their own never sample; psi, q, dt, t, mgstats and noise_draw of a run do not depend on the option.
 * Errors: null handle, mask 0 or a bit >= MSOM_ST_NACC, w not finite, stats_every < 1, `which` unknown or its accumulators not in the
 *   mask: MSOM_ERR_ARG; any of these calls before msomn_set_const, any but msomn_stats_begin (or option "stats" = 1, or a msomn_step
 *   with it) with no msomn_stats_begin since msomn_set_const, msomn_stats_get with W == 0: MSOM_ERR_STATE.
 * msomn_get_param "stats_mask", "stats_bytes" (8 nl (Ty+1) (Tx+1) per accumulator held), "stats_samples" (samples since
 *   msomn_stats_begin, automatic and by hand).  The state file carries the accumulators (msomn_state.h). */
int msomn_stats_begin(msomn_t *m, unsigned mask);
int msomn_stats_accumulate(msomn_t *m, double w);
int msomn_stats_weight(msomn_t *m, double *W);
int msomn_stats_get(msomn_t *m, int which, double *out);   /* [nl][Ty+1][Tx+1], host or device pointer */
/* measurement only (option "profile" = 1): HIP-event timing of the finest-level launches; slots "relax_fine", "relax_prolong_fine",
 * "residual", "correct", "rhs" (the whole rhs_pv chain), "coarse" (the one-launch coarse levels) */
int msomn_profile_read(msomn_t *m, const char *slot, double *avg_ms, long *launches);
int msomn_profile_reset(msomn_t *m);
int msomn_diag1d(msomn_t *m, double *out3);                                /* event write_1d_diag qg.h:361-399: ke, dissipation, forcing */
/* NetCDF-3 output / restart of vertex fields (qg-node/netcdf_vertex_bas.h:95-424): one record of
 * "psi" and "q" appended to `path`; msomn_read_nc loads variable `varname` into `field` */
int msomn_write_nc(msomn_t *m, const char *path);
int msomn_read_nc(msomn_t *m, int field, const char *path, const char *varname, int record);
/* main() + events of qg-node/qg.c: psi = noise_init (noise + sin(2 pi y / L0)) (qg.h:475-479),
 * restart.nc and input_vars_<nl>l_N<N>.nc when present in the working directory, vars.nc in
 * <workdir>/outdir_%04d/, one stdout line per iteration; nsteps_max < 0: run to tend.
 * Returns the iteration count or < 0. */
/* lossless fp64 checkpoint and bit-exact restart of a msomn_t, and the options "ckpt_steps" / "resume" of this loop: msomn_state.h */
int msomn_run(msomn_t *m, const char *workdir, long nsteps_max);
/* wavelet_filter of the vertex model, qg_baroclinic_ms.h:346-400 (event filter :405-408, driven by msomn_run when dtflt > 0):
 * invert q, masked wavelet transform (qg-node/wavelet_vertex.h:10-46) of the cell average of psi scaled by sig_lev
 * (:525-552; keys Lfmax, Lfmin, fac_filt_Rd), psi_f running mean, psi -= filtered part, q = comp_q(psi) */
int msomn_wavelet_filter(msomn_t *m, double dtflt);
int msomn_dbg_wv_get(msomn_t *m, int what /* 0 sig_lev, 1 mask_c */, int level, double *out /* [n][n], n = N >> level; tiles: msomn_create_tiled */);
int msomn_dbg_wv_apply(msomn_t *m, const double *in, double *out /* cell fields [nl][N][N]; tiles: the window [nl][Ty][Tx] */);
/* multigrid pieces on level arrays [layer][n_k+1][n_k+1] (level 0 = finest), for the parity tests */
int msomn_dbg_relax(msomn_t *m, int level, double *da, const double *res, int nsweeps);
int msomn_dbg_residual(msomn_t *m, const double *a, const double *b, double *res, double *maxres);
int msomn_dbg_restrict(msomn_t *m, int level_fine, const double *fine, double *coarse);
int msomn_dbg_prolong(msomn_t *m, int level_coarse, const double *coarse, double *fine);
int msomn_dbg_level_mask(msomn_t *m, int level, double *out);
int msomn_dbg_del2_zeta(msomn_t *m);
/* stochastic forcing of the vertex model (-D_STOCHASTIC: qg-node/qg_stochastic.h, qg-node/qg.h:306-320; params keys
 * amp_stoch, L_filt; option "stochastic" before msomn_set_const, option "seed" = srand).  The noise is a CELL
 * scalar (N x N), wavelet-filtered with the coefficients of the uniform length L_filt.  msomn_dbg_noise: optionally
 * set n_stoch, optionally filter it, optionally read it back; msomn_dbg_csig: sig_lev of one level.
 * Option "noise_mode" = 1 draws on the device instead (k_n_noise): Philox-4x32-10 with the counter (cell j * N + i, 0, draw, "msom")
 * and the key (seed, "MI35"), the layout of the cell-centred model's generator; the draw counter belongs to the handle, so handles
 * with the same seed give the same sequence whatever else the process does.  msomn_noise_draw: the next draw into n_stoch (mode 1:
 * device generator, advances the draw counter; mode 0: host stream), wavelet-filtered if filter != 0; MSOM_ERR_STATE when
 * stochastic forcing is off. */
int msomn_dbg_noise(msomn_t *m, const double *set, int filter, double *get);
int msomn_noise_draw(msomn_t *m, int filter);
int msomn_dbg_csig(msomn_t *m, int level, double *out);

#ifdef __cplusplus
}
#endif
#endif
