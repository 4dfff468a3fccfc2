// msom_host.h -- private to the host side of the layered model: struct msom, the error macros, the device scalar slots and the host
// functions that one msom_*.hip unit calls in another.  Included by msom_api.hip, msom_helm.hip, msom_diag.hip, msom_newqg.hip,
// msom_wavelet.hip, msom_io.hip, msom_state.hip, msom_hooks.hip and msom_floats.hip, and by nothing else (no kernel file, not comm.hip, not
// msom_node.hip, not the floats' host engine floats_host.hip, whose header this one includes for fh::Opts).
#ifndef MSOM_HOST_H
#define MSOM_HOST_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <time.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <map>
#include <vector>

#include "comm.h"
#include "floats_host.h"
#include "kernels.h"
#include "prof_slot.h"
#include "spec_inl.h"
#include "helm_inl.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e__ = (x);                                                                  \
    if (e__ != hipSuccess) {                                                               \
      msom_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e__), __FILE__, __LINE__, #x); \
      return MSOM_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)
#define STICKY(m, call)                                  \
  do {                                                   \
    int r__ = (call);                                    \
    if (r__ && !(m)->sticky) (m)->sticky = r__;          \
  } while (0)

// device scalar slots
// RES0, RES1 and UMAX[nl] are contiguous: one max all-reduce / one copy brings them to the host
enum { SC_BSUM = 2, SC_KE = 3, SC_SCRATCH = 4, SC_RES0 = 6, SC_RES1 = 7, SC_UMAX = 8 /* MAXNL */, SC_RESF = 8 + MSOM_MAXNL /* max|res| from the fused tendency pass */, SC_LSUM = 32 /* MAXNL */, SC_SPEC = 48 /* k_step_dt: dt limit, dt, tnext, dt / 2 */, SC_COUNT = 64 };
static_assert(SC_RESF < SC_LSUM && SC_LSUM + MSOM_MAXNL <= SC_SPEC && SC_SPEC + 4 <= SC_COUNT, "scalar slots overlap");

struct msom {
  Params p;
  std::string params_text;  // raw params.in text (backup copy in the output directory)
  // decomposition (single tile unless created with msom_create_tiled)
  int px = 1, py = 1, ix = 0, iy = 0, rank = 0, nranks = 1;
  int gnx = 0, gny = 0;  // global cells
  int nx = 0, ny = 0;    // local cells
  int walls = WALL_ALL;
  Comm *comm = nullptr;
  int sticky = MSOM_OK;  // first error of a void helper (exchange inside fill_bc / mg_cycle)
  int comm_hold = 0;     // see comm_begin
  int dbg_nosync = 0;    // option dbg_nosync (timing experiment)
  KernelOpts opt;        // options that pick kernel variants and launch shapes (kernels.h)
  int async_solve = 1;               // option: msom_step queues its tendency passes speculatively (struct SpecPass below)
  int step_sync = -1;                // option: 0 = msom_step returns without waiting for its last tendency pass (async_solve only; with rhs_close = 2
                                     // that pass carries the solve's closing residual and the host has waited for it anyway), 1 = it waits,
                                     // -1 (default) = it waits on grids of >= 2^23 cell-layers.  Measured (same process): 128^2 x 1 0.203 -> 0.185 ms per
                                     // step, 512^2 x 3 0.374 -> 0.352, 2048^2 x 3 1.238 -> 1.226, 4096^2 x 6 6.15 -> 6.20 (worse)
  double *h_pub = nullptr, *d_pub = nullptr;   // coherent pinned host block the device publishes the scalars into (+ a sequence word), and its device address
  long pub_seq = 0;
  double *q_alt = nullptr;           // stage 2 writes q + dt dq here
  int nb[8];  // neighbour ranks by direction (DIR_*), -1 = none
  int nl = 1, nlm = 1;
  int bc = BC_DIRICHLET0;
  // layer metrics (msqg/qg.h:1017-1027)
  double dhf[MSOM_MAXARR], dhc[MSOM_MAXARR];
  LayerCoef lc;
  // natural fields
  NatGeom g;
  double *f[MSOM_NFIELDS];
  int flayers[MSOM_NFIELDS];
  int fbc[MSOM_NFIELDS];
  // multigrid hierarchy (level 0 = finest)
  int nlev = 0;
  std::vector<SplitGeom> sg;
  std::vector<double *> da, da_alt, res, S;
  // chained smoother on tiles: the MARCH_HALO nearest rows of the S / N neighbour tiles (correction, residual), per level
  std::vector<double *> mh_da_s, mh_da_n, mh_res_s, mh_res_n;
  std::vector<RelaxCoef> rc;
  size_t max_split = 0;
  // agglomerated coarse levels (tiled mode): levels >= agg_level live on the gathered global grid
  int agg_level = -1, agglomerate = 1, agg_size = 256;
  int mg_global_sum = 0;
  std::vector<SplitGeom> gsg;
  std::vector<double *> gda, gda_alt, gres;
  double *agg_send = nullptr, *agg_recv = nullptr;
  // scratch
  double *staging = nullptr;   // contiguous nl*ny*nx
  double *partial = nullptr;   // per-block partial sums
  double *partial_rr = nullptr;  // per-workgroup sums of q_out from the fused tendency pass (consumed by the next mg_solve)
  double *partial_umax = nullptr;  // per-block partial maxima of k_umax
  double *d_scal = nullptr, *h_scal = nullptr;
  double *d_wind = nullptr;    // per-row surface forcing profile
  double umax_pg[MSOM_MAXNL];
  int umax_ready = 0;  // h_scal[SC_UMAX..] holds max|u| of the current psi (from the last solve)
  hipStream_t st = nullptr;
  // tiled runs: every transport call (RCCL / LOCAL), with its pack and unpack kernels, is issued on the
  // communication stream st2 (higher priority); event pairs order it against the compute stream st, so a
  // halo exchange can run beside an interior kernel launched in between (option "overlap")
  hipStream_t st2 = nullptr;
  hipEvent_t ev_c2x = nullptr, ev_x2c = nullptr;
  int overlap = 1;
  // flags
  int const_set = 0, flag_topo = 0, have_pg = 0, have_zpg = 0, have_qforc = 0;
  int fr_uniform = 1, uniformS = 0, uniform_opt = -1 /* auto */;
  int stochastic = 0, corrector_step = 0, noise_mode = 0, stoch_fused = 1;
  int prolong_fused = 1;  // first red half-sweep of a level interpolates its neighbours from the coarser level
  int block_sweeps = 0;  // experimental temporally blocked smoother (2 sweeps per pass); measured not faster at nl = 6
  int restrict_pyr = 1;  // round 3: the restriction chain below that in launches of up to 5 levels (k_restrict_pyramid)
  int restrict2 = 1;     // round 3: the pre-cycle residual pass restricts two levels down (k_residual2, res_c2)
  int block8 = 1;        // round 3: prolongation + up to 8 half-sweeps of a launch-bound level in one launch (k_relax_block, halo 8)
  int block8_max = 1024; // ... on levels of at most this many cells a side (and not marched)
  int block_small = 0;   // the same kernel on the launch-bound levels only (not marched, <= block_small cells wide): 2 launches per level visit instead of 8
  int march = 1;         // chained half-sweeps in register windows (kernels_march.hip) on wide single-GPU levels
  int march_k = 4;       // at most this many half-sweeps per pass (2..4)
  // launch-bound grids (no level takes the marching or the blocked smoother, single tile): the launches of one multigrid cycle
  // are captured once per (nrelax, first_restrict) into a hipGraph and replayed -- the host then issues 1 launch instead of ~45
  int use_graph = 0;   // measured: 512^2 x 3 0.645 vs 0.647 ms per step, 1024^2 x 3 0.860 vs 0.879, 128^2 x 1 0.316 vs 0.305 -- these grids are
                       // bound by the duration of their ~5-us kernels on the GPU, not by the host's launch rate: option "graph", off
  std::map<long, hipGraphExec_t> cyc_graph;
  int march_partial = 1; // a pass that is followed by more half-sweeps stores only the colour of its last half-sweep
  int march_min_tiled = 22;  // the same threshold on tiles (see sweep_path)
  int march_min = 23;    // log2 of the cell-layers a level needs for the chained pass (2^23: 2048^2 x 3 1.83 -> 1.78 ms/step, and the 2048 x 1024 x 6 tiles of BASELINE's 2 x 4 layout qualify; 2^22 loses: 1024^2 x 6 2.76 -> 2.87)
  int march_correct = 1; // the last pass of the finest level writes psi + da instead of da (psi rows by LDS-DMA, deferred write): 7.02 -> 6.86 ms per step at 4096^2 x 6
  int march_visit = 1;   // the finest level's visit (PL + 4, 4 + correction) in one launch on its interior chunks (k_relax_visit);
                         // 1: on levels of at least 2^march_visit_min cell-layers, 2: wherever it applies (tests)
  int march_visit_min = 23;  // 4096^2 x 6: 1.01 -> 0.87 ms per visit.  2048^2 x 3 (2^23.6) lost with three launches and 28-row chunks (0.17 -> 0.21 ms);
                             // with the ring chunks inside the fused launches and the chunk height by rounds it wins: 0.162 -> 0.146 ms,
                             // 2048^2 x 2 (2^23) 0.124 -> 0.109, 2048^2 x 6 0.349 -> 0.255
  int march_visit_levels = -1;  // the same launch, its trailing wave storing the level's correction, on the marched levels below the finest:
                                // 0 the finest level only, 1 every marched level that qualifies, -1 the default (MARCH_VISIT_LEVELS_DEFAULT)
  int march_prolong = 1; // whole levels: prolongation folded into the first pass ((PL + 4) + 4 half-sweeps; coarse rows by LDS-DMA, kernels_march.hip): 7.63 -> 7.09 ms per step at 4096^2 x 6
  int mg_fused = 1;  // fused residual+restriction and correction+residual passes of the multigrid cycle
  double *psi_alt = nullptr;  // second psi buffer (the fused correction writes out of place)
  int rhs_variant = 6;  // 6: one layer per wavefront, register windows (kernels_lpw.hip, default); 1: LDS tiles, software-pipelined; 0: LDS tiles, phase by phase
  int fused = 1;  // one-pass PV tendency kernel (kernels_fused.hip) when the configuration allows
  unsigned seed = 1, noise_draw = 0;
  int quiet = 0;
  // wavelet scale filter (msqg/qg.h:509-560): pyramids s (restricted psi), r (filtered), sig_lev
  int wv_nlev = 0, wv_ready = 0;
  // tiles: levels 0 .. wv_kt live on the tile (halo exchange per level), the levels above on a gathered top grid that every
  // rank transforms on the host (a handful of cells); wv_top_sig[k - wv_kt]: sig_lev of the gathered levels
  int wv_kt = 0, wv_gx = 0, wv_gy = 0;
  std::vector<std::vector<double>> wv_top_sig;
  double *wv_gsend = nullptr, *wv_grecv = nullptr;
  int nme_ft = 0;  // msqg/qg_energy.h:17
  // coarse levels (<= MGC_MAXDIM cells a side) solved by ONE launch (k_mg_coarse)
  CoarseArgs *d_cargs = nullptr;
  int mgc_dim = MGC_MAXDIM;  // widest level of that group
  int mgc_pfused = 1;   // option: prolongation fused into the first red phase inside k_mg_coarse (nl <= 4)
  int umax_clean = 0;  // the max|u| accumulators were zeroed with the solve's scalars and not used since
  int mgc_first = -1, mgc_opt = 4;  // first (finest) level of the group, -1: none; option "mg_coarse" (1: through global memory, 2: levels resident in LDS,
                                    // 3: as 2 with a NaN-filled pool, 4: the lean LDS form k_mg_coarse_lean where it applies, else 2)
  int mgc_lean = 0;
  int psi_ghosts_stale = 0;  // filter_de zeroed the cells of MSOM_PSI and left its ghost values, as the reference does: the next mg_solve refills them after its first residual
  int res_ready = -1;  // field id whose first multigrid residual (levels 0, 1; SC_RESF; partial sums) the last tendency pass already produced
  int adv_fused = 1;   // fold q_out = q_in + dt dq into the tendency pass
  int rhs_resid = -1;  // let the fused tendency + advance pass produce it: 1 / 0, -1 = where it measurably wins (rhs_resid_on).  k_rhs_lpw's RES
                       // instantiation (rhs_variant 6); in the LDS-tile kernel (rhs_variant 1) it lost: 23 spilled VGPRs, 2.21 ms vs 1.63 + 0.50 ms
  int rr_nparts = 0;   // partial sums of q_out the last such pass wrote
  int rhs_close = -1;  // the speculative tendency pass also closes the solve in front of it (k_rhs_lpw CLS, max|res| of the solve's b) in place of
                       // k_resmax_march: 0 never, 1 first RK stage (a psi-only max|u| pass stays), 2 both stages, -1 = where it measurably wins
  // back-and-forth nudging loop on the device (msom_bfn_*)
  int bfn_begun = 0;                      // msom_bfn_begin since the last msom_set_const
  int bfn_obs_set = 0, bfn_gain_set = 0;  // MSOM_BFN_OBS / MSOM_BFN_GAIN came in through msom_set_field (gain never set: 1 everywhere)
  double *bfn_partial = nullptr;          // per-block partial sums of msom_bfn_misfit
  // running statistics on the device (msom_stats_*, msom_time_filter); nothing is allocated until one of them is called
  unsigned stats_mask = 0;                // accumulators selected by the last msom_stats_begin since msom_set_const (0: none)
  StatsAcc stats = {};                    // the selected accumulators, natural layout, nl layers each
  double *stats_W = nullptr;              // device scalar: sum of the weights
  double *stats_qme = nullptr;            // qo_me of time_filter (allocated by the first msom_time_filter after msom_set_const)
  int stats_on = 0, stats_every = 1;      // options "stats", "stats_every"
  long stats_count = 0;                   // msom_step calls seen since msom_stats_begin (every stats_every-th one samples)
  long stats_ndev = 0;                    // ... of whose samples, those that read their weight from the device (tests ask: stats_dev_samples)
  double tau_f = 20;                      // option "tau_f" (msqg/qg.h:495)
  // Lagrangian floats (msom_floats_*, msom_floats.hip); nothing is allocated until msom_floats_begin
  fh::Opts floats;                        // the state and the options "floats", "floats_tiles", "floats_msg_cap" (floats_host.h)
  // vertical normal modes (msom_modes_*, msqg/eigmode.h); nothing is allocated until msom_modes_compute
  int modes_ready = 0;                    // a successful msom_modes_compute since the last msom_set_const
  int modes_compact = 0;                  // ... which left the compact form (modes_mc) rather than one array per number (modes_md)
  int modes_compact_opt = -1;             // option "modes_compact": -1 compact where the stratification is uniform, 0 always per column
  ModeCoef modes_mc = {};                 // compact form: M2L[k * nl + m] and iBu_m, passed to the kernels by value
  double *modes_md = nullptr;             // general form: nl*nl + nl natural layers (M2L arrays, then iBu)
  double *modes_dev = nullptr;            // device scratch: the numbers of the compact solve, then the 2 nl sums of msom_modes_energy
  int *modes_flag = nullptr;              // device word the eigen kernel ORs its failures into
  double *modes_partial = nullptr;        // per-block partial sums of msom_modes_energy
  // modal PV inversion (option mode_pv_invert, msqg/qg.h:116-157); nothing is allocated until the first modal solve
  int mode_pv_invert = 0;                 // option: invertq goes through the modes (one tile only)
  std::vector<double *> helm_ibu;         // general form: iBu_m per cell on every level, split layout (built by the first modal solve after msom_modes_compute, dropped with the modes)
  double *helm_pm = nullptr, *helm_qm = nullptr;   // mode-space natural fields: p_m (warm start, the reference's pom; valid ghosts) and q_m
  double *helm_scal = nullptr;            // device scalar block of the modal solve: HS_* below, MSOM_MAXNL each
  double *helm_partial = nullptr;         // per-workgroup sums of q_m (mgstats.sum per mode)
  HelmSolve helm = {};                    // per-mode mg_solve state (helm_inl.h)
  int helm_solved = 0;                    // a modal solve since the last msom_set_const (msom_modes_mgstats)
  ProfSlot prof_helm_relax, prof_helm_resid, prof_helm_coarse;   // finest-level sweeps, residual passes, levels of <= 64 cells a side
  // wavenumber spectra (msom_spec_*, msqg/scripts/fftlib.py); nothing is allocated until the first spectrum call after msom_set_const
  int spc_batch = 0;                      // layers the work arrays hold (0: not allocated)
  int spc_smax = 0;                       // last shell: floor(sqrt(2) * max(nx, ny) / 2)
  double2 *spc_z = nullptr, *spc_zt = nullptr;   // row-transformed batch [batch][ny][nx] and its transpose [batch][nx][ny]
  double2 *spc_tw = nullptr;              // exp(-2 pi i t / nmax), t < nmax / 2 (host long double, rounded once)
  double *spc_v = nullptr;                // spec_2D of the half plane [batch][nx / 2 + 1][ny]
  double *spc_te = nullptr, *spc_res = nullptr;  // shell sums [batch][2][smax + 1]; bin sums and fluxes [batch][2][nbins]
  double *spc_hin = nullptr;              // device copies of a caller's host arrays [2][batch][ny][nx] (first host input)
  double *spc_o2d = nullptr;              // plane of msom_spec_2d for a host `out` [batch][ny][nx] (first such call)
  size_t spc_bytes = 0;                   // all of the above
  std::vector<long> spc_count;            // points per bin (msom_spec_layout of this grid)
  int s_zero = 0;  // pystep_de(onlyKE = 1) zeroed the stretching field S (msqg/qg_energy.h:319-325); undone by msom_set_const
  std::vector<NatGeom> wv_g;
  std::vector<double *> wv_s, wv_r, wv_sig;
  // newqg dialect (msom_create_newqg): the cell-centred one-layer model of newqg/qg.h runs on this handle; 0 on every other
  int model = 0;
  NewqgParams nq = {};
  int nq_fused = 1;      // option: the tendency in one pass (k_nq_rhs); 0: one launch per reference loop (validation chain)
  int nq_adv_fused = 1;  // option: q_out = q_in + dt dq folded into that pass
  int nq_rows = 0;       // option: chunk height of k_nq_rhs (0: automatic)
  // state file (msom_state.hip): options "ckpt_steps" / "resume" of msom_run, the test aid of msom_state_dbg_flip, and msom_run's
  // own locals (next output and filter events, number of the output directory) as the last load found them in the file
  int ckpt_steps = 0, resume = 0;
  long state_flip = -1;
  int run_loaded = 0, run_outdir = 0;
  double run_tout = 0, run_tflt = 0;
  // time loop
  double t = 0, dt = 1., tnext = HUGE_VAL, previous = 0;
  int iter = 0;
  msom_mgstats mg = {0, 0, 0, 0, 0};
  // profiling of the finest-level smoother sweep
  int profile = 0;
  ProfSlot prof_sweep, prof_resid, prof_block, prof_march[5];  // prof_march[K]: passes of K chained half-sweeps
  ProfSlot prof_march_pl;  // first pass of a level with the prolongation folded in
  ProfSlot prof_march_visit;  // the finest level's fused visit (k_relax_visit and the two passes on the chunks around it)
  ProfSlot prof_march_visit_coarse;  // the fused visits of the marched levels below the finest (profile = 1)
  ProfSlot prof_march_corr, prof_resmax;  // last pass of the finest level with the correction folded in; max-only residual pass after it
  ProfSlot prof_rhs, prof_redprol, prof_rescorr, prof_respre;   // tendency pass, finest red+prolongation, post- / pre-cycle residual passes
  ProfSlot prof_floats;   // the floats' stages queued by msom_step (k_floats_stage)
  ProfSlot prof_floats_emig, prof_floats_immig;   // on tiles, per phase of the migration pass: k_floats_emigrate with its header launch, k_floats_immigrate
};

// ---- what travels with one call (nothing of it is kept on the handle)
// One tendency pass as rhs_terms is asked for it: comp_del2, advection_pv, dissip, ekman_friction, surface_forcing, [qforcing],
// [bottom_topography] (msqg/qg.h:622-630 / qg_bfn.h:67-76) with the coefficients iRe, iRe4, Eks, Ekb of m->p.
struct RhsPass {
  int qfield, dqfield, with_qforcing;
  int adv_out = -1, adv_in = -1;     // adv_out >= 0 asks for q[adv_out] = q[adv_in] + adv_dt * dq in the same pass (the corrector's advance_qg)
  double adv_dt = 0.;
  double *out = nullptr;             // written in place of f[adv_out]
  const double *dt_dev = nullptr;    // adv_dt is read from this device scalar instead (k_rhs_lpw only)
  int cls = 0;                       // the pass closes the solve that made psi (k_rhs_lpw CLS): 1 max|res|, 2 max|res| and max|u|, as
  const double *cls_b = nullptr;     // k_resmax_march would leave them; cls_b: that solve's right-hand side
  int emit_resid = -1;               // the first residual of the inversion of q[adv_out] as a by-product: -1 as option rhs_resid says, 1, 0
  bool advanced = false;             // result: the advance did ride in the pass (else the caller runs advance_qg)
};
// Speculative tendency pass (one tile): right after the first multigrid cycle of a solve the tendency kernel is queued BEFORE the
// host has read max|res| and max|u| -- with dt computed on the device (k_step_dt) in the first RK stage -- so the GPU works through
// the host round trip instead of idling (0.49 -> 0.43 ms per step at 256^2 x 3 with the read skipped altogether,
// tools/ab_nosync.py).  If the solve turns out to need another cycle the pass is simply run again afterwards: its output went to
// the predictor (stage 1) or to a spare buffer that only replaces q when the solve had converged (stage 2).
// mg_solve, invertq and solve_and_dt take a pointer to this description of what to queue; null: nothing.
struct SpecPass {
  int stage;               // 1: dt on the device (k_step_dt in front of the pass); 2: dt known, output to q_alt
  RhsPass pass;
  bool launched = false;   // results: the pass was queued,
  int rc = MSOM_OK;        // ... what rhs_terms returned,
  bool counts = false;     // ... and the solve ended after that cycle: the output of the pass stands
};

// slots of the modal solve's device scalar block (helm_scal): max |res_m| before the first cycle, after the last one, sum of q_m
enum { HS_RES0 = 0, HS_RES1 = MSOM_MAXNL, HS_BSUM = 2 * MSOM_MAXNL, HS_COUNT = 3 * MSOM_MAXNL };

// One multigrid level as the smoother sees it: either this rank's tile of level k (halo
// exchange with the neighbour tiles after every colour) or, below the agglomeration level, the
// whole coarse grid gathered on every rank (walls only, no communication).
struct Lev {
  double **da, **da_alt;
  double *res;
  const double *S;
  const SplitGeom *sg;
  const RelaxCoef *rc;
  int walls;
  bool tiled;   // needs halo exchanges
  bool fine;    // level 0 (profiling tag)
  int k;        // tile level index (-1: gathered global level)
};

// ---- the two dialects of a msom_t.  An entry point of the msqg dialect answers a newqg handle with MSOM_ERR_CONFIG: this one guard,
// first statement of each of them; the calls both dialects have dispatch to the nq_* functions of msom_newqg.hip.
#define MSQG_ONLY(m)                                  \
  do {                                                \
    if ((m) && (m)->model) return nq_refuse(__func__); \
  } while (0)
#define NEED_CONST(m)                                                    \
  do {                                                                   \
    if (!(m)) return MSOM_ERR_ARG;                                       \
    if (!(m)->const_set) {                                               \
      int r__ = msom_set_const(m);                                       \
      if (r__) return r__;                                               \
    }                                                                    \
  } while (0)
#define NEED_MODES(m, fn)                                                                   \
  do {                                                                                      \
    if (!(m)->const_set || !(m)->modes_ready) {                                             \
      msom_set_error(fn ": no successful msom_modes_compute since msom_set_const");         \
      return MSOM_ERR_STATE;                                                                \
    }                                                                                       \
  } while (0)

// ---- host functions that cross a unit boundary.  Hidden: the fast and the strict library are loaded side by side, and none of
// these names may be resolvable from outside its own library.
#pragma GCC visibility push(hidden)
// msom_api.hip (core)
int sync_stream(msom *m);
void prof_begin(msom *m, ProfSlot &ps, hipStream_t st = nullptr);   // st: the stream the timed launches go to (default: m->st)
void prof_end(msom *m, ProfSlot &ps, hipStream_t st = nullptr);
void prof_collect(msom *m, ProfSlot &ps);
NatGeom make_nat(int nx, int ny);
void comm_begin(msom *m);
void comm_end(msom *m);
int reduce_scal(msom *m, int slot, int n, int op);
int exch_nat_g(msom *m, double *f, const NatGeom &g, int nl, int bc, int depth);
int exch_split(msom *m, double *f, const SplitGeom &sg, int nl, int corners);
msom *create_common(const Params &p0, int px, int py, int rank, const void *id128, const NewqgParams *nq = nullptr);
int check_field(msom *m, int field);
int ensure_field(msom *m, int field);
int fill_bc(msom *m, int field);
int upload(msom *m, int field, const double *a);
int download(msom *m, int field, double *a);
int build_coefs(msom *m);
Lev tile_lev(const msom *m, int k);
bool relax_sweeps(msom *m, Lev &L, const Lev *coarse, int nrelax, int corners_last, bool corr_req);
void residual(msom *m, const double *a, const double *b, int slot, int want_sum);
void residual2(msom *m, int mode, const double *b, int slot, int want_sum);
int invertq(msom *m, const double *q, SpecPass *sp = nullptr);
double limiter(msom *m, double umax, double dtmax);
void comp_del2(msom *m, int in, int out, double add, double fac);
void comp_stretch(msom *m, int in, int out, double add, double fac);
int rhs_terms(msom *m, RhsPass &ps);
int check_shape(msom *m, int a, int b, int c);
double dtnext(msom *m, double dt, double *tnext_out);
// msom_helm.hip
void helm_drop_pyramid(msom *m);
int helm_partial_stride(const msom *m);
int helm_ensure(msom *m);
int helm_relax_level(msom *m, int k, int nhalf, const HelmCount &cnt, ProfSlot *ps);
int helm_residual(msom *m, const double *a, const double *b, int slot, int want_sum);
int helm_read(msom *m, double *h);
void helm_fill(msom *m, double *f);
int helm_run(msom *m, double *a, const double *b);
int helm_solve(msom *m, const double *q);
// msom_diag.hip
void stats_drop(msom *m);
void stats_sample(msom *m, const double *w_dev, double w);
void modes_drop(msom *m);
ModesLayers modes_layers(const msom *m);
const ModeCoef *modes_mc(const msom *m);
int modes_energy_launch(msom *m);
void spec_drop(msom *m);
int spec_guard(msom *m, const char *fn);
int spec_ensure(msom *m);
SpecIn spec_in_nat(const msom *m, int mode, const double *a, const double *b);
void spec_batch_2d(msom *m, const SpecIn &in, int cnt, int kind, double *o2d);
void spec_batch_1d(msom *m, int cnt);
// msom_floats.hip (is_device_ptr: floats_host.h)
void floats_drop(msom *m);
void floats_hook(msom *m, int stage, double tnext);   // one stage of msom_step's floats, queued on m->st with m->dt; no host wait
bool floats_param(msom *m, const char *key, double *v);
// msom_newqg.hip
int nq_refuse(const char *fn);
bool nq_has_field(int field);
int nq_alloc(msom *m);
int nq_set_option(msom *m, const char *key, double v);
double nq_get_param(msom *m, const char *key);
int nq_after_upload(msom *m, int field);
int nq_set_const(msom *m);
double nq_update(msom *m, const double *q, double *dqdt, double dtmax);
int nq_advance(msom *m, double *qout, const double *qin, const double *dqdt, double dt);
int nq_invertq(msom *m, const double *q, double *psi, msom_mgstats *st);
int nq_comp_q_api(msom *m, const double *psi, double *q);
int nq_step(msom *m, double *dt_used);
int nq_bench_kernel(msom *m, const char *kernel, int reps, double *avg_ms);
// msom_wavelet.hip
int filter_de(msom *m, int pm_field, double dtflt, double ediag);
// msom_state.hip: msom_state_save with msom_run's locals (tout, tflt, number of the output directory; null: none) in a record
int state_save_run(msom *m, const char *path, unsigned flags, const double *run3);
// msom_hooks.hip: the profile slots of a handle under the names msom_profile_read takes
std::vector<std::pair<const char *, ProfSlot *>> prof_slots(msom *m);
#pragma GCC visibility pop

#endif
