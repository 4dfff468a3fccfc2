// kernels.h -- launch wrappers of the HIP kernels (internal).
#ifndef MSOM_KERNELS_H
#define MSOM_KERNELS_H

#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "msom_internal.h"
#include "modes_inl.h"   // ModesLayers, the per-column eigen routine
#include "floats_inl.h"  // FloatsGeom, the arithmetic of the Lagrangian floats

// Run-time value -> template argument.  with_int<LO, HI>(v, f) calls f(std::integral_constant<int, v>{}) and returns true when
// LO <= v <= HI; otherwise it calls nothing and returns false.  The range is the list of instantiations a launcher has: a launcher
// that returns int answers false with -1, a void one with no_kernel() -- never with a silent skip.
template <int LO, int HI, class F>
static inline bool with_int(int v, F &&f) {
  if constexpr (LO > HI) return false;
  else {
    if (v == LO) { f(std::integral_constant<int, LO>{}); return true; }
    return with_int<LO + 1, HI>(v, std::forward<F>(f));
  }
}
// f(std::true_type{}) or f(std::false_type{})
template <class F>
static inline void with_bool(bool b, F &&f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
[[noreturn]] static inline void no_kernel(const char *launcher, int nl) {
  fprintf(stderr, "msom: %s: no kernel for nl = %d\n", launcher, nl);
  abort();
}

// layer metrics idh0/idh1 (msqg/qg.h:1017-1027), passed by value to kernels
struct LayerCoef {
  double idh0[MSOM_MAXNL], idh1[MSOM_MAXNL];
};

// per-level constants of the column solver
struct RelaxCoef {
  double D, sqD;              // Delta and Delta^2 of the level
  double idh0[MSOM_MAXNL], idh1[MSOM_MAXNL];
  // uniform-S fast path: the tridiagonal is the same in every column, so the Thomas
  // factorisation is done once on the host (msqg/poisson_layer.h:137-140)
  double t2[MSOM_MAXNL];      // super-diagonal
  double w[MSOM_MAXNL];       // t0[l] / t1'[l-1]
  double it1[MSOM_MAXNL];     // 1 / t1'[l]
  double S[MSOM_MAXNL];       // uniform S_l (residual, stretching)
};

// kernel-selection options of one handle, named after their msom_set_option keys; the defaults are the product configuration
struct KernelOpts {
  int march_rows = 0;         // chunk height of k_relax_march (0: automatic)
  int march_xcd = 1;          // XCD-contiguous block numbering of the marching passes
  int march_flip = 1;         // odd chunks march down
  int march_dbg = 0;          // timing experiments of the marching passes
  int march_lean = 2;         // interior chunks of the LDS-DMA pass take the lean body (2: requests two steps ahead where LDS allows)
  int march_dma = 2;          // LDS-DMA version of the pass (0 register-window kernel, 1 one strip, 2 four strips per workgroup)
  int march_visit_rows = 0;   // chunk height of k_relax_visit (0: by rounds of wave-pair slots, relax_visit_rows; 28 on the finest level at 4096^2)
  int march_visit_pairs = 2;  // wave pairs per workgroup of k_relax_visit (1 or 2; 4096^2 x 6: 0.866 / 0.873 ms with 2, 0.881 / 0.883 with 1)
  int march_visit_ring = 2;   // the wall-ring chunks around k_relax_visit: 0 two launches over the whole chunk grid with a skip rectangle,
                              // 1 two launches over the ring chunks only, 2 workgroups of two k_relax_visit launches
  int march_visit_split = 0;  // march_visit_ring = 2: fused chunk rows in the first of the two launches (0: a third of them; rounded down to even; < 0: none)
  int resmax_rows = 0;        // rows per chunk of k_resmax_march (0: 32), -1: the LDS-tiled kernel instead
  int block_variant = 0;      // tile shape of k_relax_block (tools/bench_kernels.py)
  int rhs_dbg = 0;            // bits 128, 256, 512: plain residual / red-prolongation kernels; rows << 8 overrides k_rhs_lpw's chunk height
  int lpw_dbg = 0;            // bits 1, 2 timing experiments of k_rhs_lpw; 4: every wavefront takes the instantiation with the ghost-line code
};
int device_cu_count();   // CUs of the current device, asked once per device

// ---- kernels_floats.hip: Lagrangian floats (msom_floats_*), one float per lane, structure of arrays
struct FloatsDev {
  double *x, *y;     // positions at the last step boundary
  double *xh, *yh;   // positions after stage 1
  const int *layer;
  unsigned long long *cnt;   // [0] clamped to the box, [1] lost (not finite); on tiles also [2] unsent, [3] records sent
};
// on tiles the arrays above are n slots: slot k < *hw with live[k] != 0 holds float id[k]; (ox, oy) is the tile's origin in cells
// (vertex model: in vertices)
struct FloatsTileDev {
  const int *id, *live, *hw;
  int ox, oy;
};
// the same slots as the migration kernels write them, with the free stack and the record counters of the two messages of a phase
struct FloatsMig {
  double *x, *y, *xh, *yh;
  int *layer, *id, *live;
  int *hw, *nfree, *free;    // high-water mark; the slots below it that are empty
  int *msgcnt;               // [2]: records taken in the lo (W / S) and the hi (E / N) message
  unsigned long long *cnt;
};
// stage 1: (xh, yh) = (x, y) + dt / 2 U(x, y); stage 2: (x, y) += dt U(xh, yh), also stored to rec[0 .. n), rec[n .. 2n) when rec is given.
// U from psi (+ pg per corner when pg is given), natural layout with its ghost ring.  t (tiles): over the slots, fg the global
// geometry, the record indexed by id with rec[2n + id] = 1
void launch_floats_stage(hipStream_t st, int stage, const FloatsDev &d, int n, const double *psi, const double *pg, const NatGeom &g,
                         const FloatsGeom &fg, double dt, double *rec, const FloatsTileDev *t = nullptr);
// at (x, y): o0 = u, o1 = v of f (+ pg) when o1 is given, else o0 = the bilinear value of f.  t (tiles): o0 is [3][n], indexed by id:
// the one or two results and the presence word
void launch_floats_interp(hipStream_t st, const FloatsDev &d, int n, const double *f, const double *pg, const NatGeom &g, const FloatsGeom &fg,
                          double *o0, double *o1, const FloatsTileDev *t = nullptr);
// one phase (x: W / E, y: S / N) of the migration pass: records of 6 doubles into the messages mlo, mhi (1 + 6 K doubles each, the
// header word written by a one-lane launch behind it; null: no neighbour), then the records of the received messages into free slots.
// node: the vertex grid's owner rule (nfloats_locate, nfloats_owner) in place of floats_locate, floats_owner
void launch_floats_emigrate(hipStream_t st, const FloatsMig &s, int n, const FloatsGeom &fg, const FloatsTiling &t, int yphase, int half, double *mlo,
                            double *mhi, int K, bool node = false);
void launch_floats_immigrate(hipStream_t st, const FloatsMig &s, int n, int nl, const double *rlo, const double *rhi, int K);
// out [3][n] (zeroed): a, b of the live slots by id and the presence word; all [nranks][3][n] -> o0, o1 [n] (o1 may be null)
void launch_floats_scatter(hipStream_t st, const double *a, const double *b, const FloatsTileDev &t, int n, double *out);
void launch_floats_select(hipStream_t st, const double *all, int nranks, int n, double *o0, double *o1);

// ---- kernels_node_floats.hip: Lagrangian floats of the vertex-grid model (msomn_floats_*).  g: the natural layout of the level-0
// fields, fg = {N, N, 0, N / L0, L0, L0}; psi, pg, f, rf: fields of nl layers, mk: the mask (one layer).  t (tiles): over the slots,
// g the tile's layout, fg still the global geometry, t->ox, t->oy the tile's vertex origin
// stage 1: (xh, yh) = (x, y) + dt / 2 U(x, y); stage 2: (x, y) += dt U(xh, yh), also stored to rec[0 .. n), rec[n .. 2n) when rec is given,
// with the bilinear value of rf at the new position in rec[2n .. 3n) when rf is given too.  t: the record is indexed by id with
// rec[2n + id] = 1, and rf is not read
void launch_nfloats_stage(hipStream_t st, int stage, const FloatsDev &d, int n, const double *psi, const double *pg, const NatGeom &g,
                          const FloatsGeom &fg, double dt, double *rec, const double *rf, const FloatsTileDev *t = nullptr);
// at (x, y): o0 = u, o1 = v of f (+ pg) when o1 is given, else o0 = the bilinear value of f.  t: o0 is [3][n], indexed by id: the one
// or two results and the presence word
void launch_nfloats_interp(hipStream_t st, const FloatsDev &d, int n, const double *f, const double *pg, const NatGeom &g, const FloatsGeom &fg,
                           double *o0, double *o1, const FloatsTileDev *t = nullptr);
// *out += the floats that are not lost and whose cell has mk == 0 at all four corners.  t: those of the rank's live slots
void launch_nfloats_on_land(hipStream_t st, const FloatsDev &d, int n, const double *mk, const NatGeom &g, const FloatsGeom &fg,
                            unsigned long long *out, const FloatsTileDev *t = nullptr);

// ---- kernels_rhs.hip
void launch_fill_ghost(hipStream_t st, double *f, const NatGeom &g, int nl, int bc, int walls, int depth = 1);
void launch_fill_periodic(hipStream_t st, double *f, const NatGeom &g, int nl, int depth);
void launch_fill_lin_dirichlet(hipStream_t st, double *f, const NatGeom &g, int nl, const double *upg, const double *vpg, double D, double Lx,
                               double Ly, int ox = 0, int oy = 0, int sides = WALL_ALL);
void launch_slip_bc(hipStream_t st, const double *po, double *zeta, const NatGeom &g, int nl, double c, int walls);
void launch_pack(hipStream_t st, const double *src, double *dst, const NatGeom &g, int nl);
void launch_unpack(hipStream_t st, const double *src, double *dst, const NatGeom &g, int nl);
void launch_del2(hipStream_t st, const double *po, double *zeta, const NatGeom &g, int nl, double add, double fac, double D);
void launch_stretch(hipStream_t st, const double *po, double *out, const double *S, const NatGeom &g, int nl, double add, double fac,
                    const LayerCoef &lc);
void launch_advection(hipStream_t st, const double *zeta, const double *psi, const double *psipg, const double *zetapg, const double *S,
                      const double *qot, double *dq, const NatGeom &g, int nl, int have_pg, int have_zpg, int stochastic, double D,
                      double beta, double itr_stoch, const LayerCoef &lc);
void launch_umax(hipStream_t st, const double *f, double *partial, double *out, const NatGeom &g, int nl, double D);
void launch_axpy(hipStream_t st, double *dq, const double *x, const NatGeom &g, int nl, double c);
void launch_forcing(hipStream_t st, const double *zeta, const double *psi, const double *qforc, const double *topo, const double *Ro,
                    const double *wind, double *dq, const NatGeom &g, int nl, int have_qforc, int flag_topo, double cs, double cb,
                    double D, double dhb);
void launch_advance(hipStream_t st, double *qo, const double *qi, const double *dq, const double *noise, const NatGeom &g, int nl, double dt,
                    double dts);
// nudging + AB3 update of msom_bfn_steps; obs == nullptr: no nudging term, gain == nullptr: gain 1
void launch_bfn_ab3(hipStream_t st, double *q, double *f1, const double *f2, const double *f3, const double *obs, const double *gain,
                    const NatGeom &g, int nl, double dt12, double k);
int bfn_misfit_blocks(const NatGeom &g);
void launch_bfn_misfit(hipStream_t st, const double *q, const double *obs, const double *gain, double *partial, double *out2, const NatGeom &g,
                       int nl);
// running statistics (msom_stats_*): s[k] = accumulator MSOM_ST_k (natural layout) or null where the mask does not select it
struct StatsAcc {
  double *s[MSOM_ST_NACC];
};
// one sample of weight *w_dev (w_dev != nullptr) or w into the accumulators of `mask`; *W += the weight.  D2 = 2 Delta
void launch_stats_acc(hipStream_t st, unsigned mask, const double *psi, const double *q, const StatsAcc &a, const NatGeom &g, int nl,
                      const double *w_dev, double w, double D2, double *W);
void launch_stats_mean(hipStream_t st, double *out, const double *s, const double *W, const NatGeom &g, int nl);
// which = MSOM_ST_EKE / UQ_EDDY / VQ_EDDY from the mean psi pm (ghosts filled), sa = KE / UQ / VQ, sq = Q (eddy fluxes); out: [nl][ny][nx]
void launch_stats_derive(hipStream_t st, double *out, const double *pm, const double *sa, const double *sq, const double *W, const NatGeom &g,
                         int nl, int which, double D2);
void launch_time_filter(hipStream_t st, double *me, const double *q, const NatGeom &g, int nl, double a);
int partial_count(const NatGeom &g);
void launch_sum_final(hipStream_t st, const double *partial, double *out, int n);
void launch_ke(hipStream_t st, const double *po, double *partial, double *out, const NatGeom &g, double D);
void launch_sum_layers(hipStream_t st, const double *f, double *partial, double *out, const NatGeom &g, int nl);
void launch_sub_layer_const(hipStream_t st, double *f, const double *sums, const NatGeom &g, int nl, double inv_count);
void launch_make_S(hipStream_t st, const double *Fr, const double *Ro, double *S, const NatGeom &g, int nlm);

void launch_noise(hipStream_t st, double *n, const double *sigma, const NatGeom &g, int nl, double amp, unsigned seed, unsigned draw, int gx0,
                  int gy0, int gnx);

void launch_ptr_rhs(hipStream_t st, const double *psi, const double *c, const double *rel, double *dp, const NatGeom &g, int nl, int np,
                    const double *iPe, const double *ptr_ir, double D);

// energy / PV budgets (msqg/qg_energy.h)
void launch_advection_de(hipStream_t st, const double *zeta, const double *psi, const double *psipg, const double *zetapg, const double *S, double *j1,
                         double *j2, double *j3, const NatGeom &g, int nl, double D, double beta, double dt, double ediag, const LayerCoef &lc);
void launch_dissip_de(hipStream_t st, const double *p4, const double *str, const double *po, double *dq, const NatGeom &g, int nl, double iRe,
                      double iRe4, double dt, double ediag, double D, int stage);
void launch_ekman_de(hipStream_t st, const double *zeta, const double *po, double *dq, const NatGeom &g, int nl, double cs, double cb, double dt,
                     double ediag);
void launch_running_mean(hipStream_t st, double *pm, const double *po, const NatGeom &g, int nl, int n);
void launch_filter_de(hipStream_t st, double *ft, const double *tmp2, double *pm, const NatGeom &g, int nl, double dtflt, double ediag);

// ---- kernels_fused.hip
// optional by-product of the fused tendency + advance pass: the first residual of the next inversion
struct RhsResid {
  double *res, *res_c;       // level-0 residual (split layout) and its restriction to level 1 (or null)
  double *res_max;           // device scalar: max|res| (zeroed by the launcher)
  double *bsum_partial;      // one partial sum of q_out per workgroup (rhs_pipe_blocks / rhs_lpw_blocks entries)
  SplitGeom sg, cg;
  // k_rhs_lpw only (option rhs_close): the pass also closes the solve that produced its psi.  cls = 1: b of that solve is q_in; 2: b is a
  // field of its own, and max|u| of psi per layer comes out as well.  Both accumulators were zeroed with the solve's scalars
  int cls = 0;
  const double *cls_b = nullptr;   // cls = 2: the solve's right-hand side
  double *cls_max = nullptr;       // device scalar: max|b - (lap + Gamma) psi|
  double *cls_umax = nullptr;      // cls = 2: nl device scalars, max|u| per layer
};
int rhs_fused_blocks(const NatGeom &g);
void launch_rhs_fused(hipStream_t st, const KernelOpts &o, const double *psi, const double *S, const double *qforc, const double *wind, double *dq,
                      double *umax_partial, double *umax_out, const NatGeom &g, int nl, int walls, int uniformS, const double *Su,
                      int have_qforc, double D, double beta, double iRe, double iRe4, double cs, double cb, double slip_c,
                      const LayerCoef &lc, int variant, const double *q_in = nullptr, double *q_out = nullptr, double dt = 0.,
                      const RhsResid *rr = nullptr, int region = 0, const double *dt_ptr = nullptr);
int rhs_pipe_blocks(const NatGeom &g);
// ---- kernels_lpw.hip: same pass, one layer per wavefront, register windows + DPP (chunk height: rhs_dbg >> 8, 0: automatic)
void launch_rhs_lpw(hipStream_t st, const KernelOpts &o, const double *psi, const double *S, const double *qforc, const double *wind, double *dq,
                    const NatGeom &g, int nl, int walls, int uniformS, const double *Su, int have_qforc, double D, double beta, double iRe, double iRe4,
                    double cs, double cb, double slip_c, const LayerCoef &lc, const double *q_in, double *q_out, double dt, int stoch = 0,
                    const double *q_stage = nullptr, const double *noise = nullptr, double crelax = 0., double dts = 0., int region = 0,
                    const double *dt_ptr = nullptr, const RhsResid *rr = nullptr);
int rhs_lpw_blocks(const KernelOpts &o, const NatGeom &g, int nl);   // workgroups of that launch with the residual by-product

// ---- kernels_mg.hip
// coarse part of the multigrid cycle in one launch (k_mg_coarse): lev[0] = finest of the group
#define MGC_MAXLEV 8
#define MGC_MAXDIM 32
#define MGC_NT 512
struct CoarseLev { double *da, *res; const double *S; SplitGeom g; RelaxCoef rc; };
struct CoarseArgs { CoarseLev lev[MGC_MAXLEV]; int n, walls, prolong_fused, lds; };
void launch_mg_coarse(hipStream_t st, const CoarseArgs *d_args, int nrelax, int nl, int uniformS, int lean = 0);
size_t mg_coarse_lean_doubles(const CoarseArgs &h, int nl);   // LDS doubles the lean form needs (<= MGC_POOL)
#define MGC_POOL 19200  // doubles of LDS pool of the one-launch coarse kernels: 150 KB
size_t mg_coarse_static_lds();  // bytes of static LDS k_mg_coarse declares (its launch needs a device that grants them)
void launch_nat_to_split(hipStream_t st, const double *nat, const NatGeom &g, double *sp, const SplitGeom &sg, int nl);
void launch_split_to_nat(hipStream_t st, const double *sp, const SplitGeom &sg, double *nat, const NatGeom &g, int nl);
void launch_split_pack(hipStream_t st, const double *src, double *sp, const SplitGeom &sg, int nl, int bc, int walls);
void launch_split_unpack(hipStream_t st, const double *sp, const SplitGeom &sg, double *dst, int nl);
void launch_residual(hipStream_t st, const double *a, const double *b, const double *S, const NatGeom &g, double *res, const SplitGeom &sg,
                     int nl, const RelaxCoef &rc, int uniformS, double *maxres, double *sum_partial, int want_sum);
int residual2_blocks(const NatGeom &g);
void launch_residual2(hipStream_t st, const KernelOpts &o, int mode, const double *a, const double *da, double *a_out, const double *b, const double *S,
                      const NatGeom &g, double *res, const SplitGeom &sg, double *res_c, const SplitGeom &cg, int nl, const RelaxCoef &rc,
                      int uniformS, int walls, double *maxres, double *sum_partial, int want_sum, double *umax_partial, double *umax_out,
                      int umax_clean = 0,
                      double *res_c2 = nullptr, const SplitGeom *cg2 = nullptr);
void launch_restrict(hipStream_t st, const double *fine, const SplitGeom &fg, double *coarse, const SplitGeom &cg, int nl);
void launch_restrict_pyramid(hipStream_t st, const double *fine, double *const *out, const SplitGeom *g, int n, int nl);   // g[0] fine, g[1..n] outputs; n <= 5
void launch_prolong(hipStream_t st, const double *coarse, const SplitGeom &cg, double *fine, const SplitGeom &fg, int nl, int walls);
void launch_relax_color(hipStream_t st, double *da, const double *res, const double *S, const SplitGeom &sg, int nl, const RelaxCoef &rc,
                        int uniformS, int color, int walls, int fine, int region = 0);
void launch_relax_ring(hipStream_t st, double *da, const double *res, const double *S, const SplitGeom &sg, int nl, const RelaxCoef &rc,
                       int uniformS, int color, int walls);
int launch_relax_block8(hipStream_t st, const KernelOpts &o, const double *da_in, const double *coarse, const SplitGeom &cg, const double *res, double *da_out,
                        const SplitGeom &sg, int nl, const RelaxCoef &rc, int walls, int nh, int c0, const double *S = nullptr);
void launch_relax_block2(hipStream_t st, const KernelOpts &o, const double *da_in, const double *coarse, const SplitGeom &cg, const double *res, double *da_out,
                         const SplitGeom &sg, int nl, const RelaxCoef &rc, int walls, int fine);
void launch_relax_red_prolong(hipStream_t st, const KernelOpts &o, double *da, const double *coarse, const SplitGeom &cg, const double *res, const double *S,
                              const SplitGeom &sg, int nl, const RelaxCoef &rc, int uniformS, int walls);
void launch_correct(hipStream_t st, double *a, const NatGeom &g, const double *da, const SplitGeom &sg, int nl, int walls);

// ---- kernels_march.hip: K = 2..4 consecutive half-sweeps in one pass (register windows, out of place)
// tiles: the `rows` nearest rows of the S / N neighbour tiles of the input and of the residual (null at a wall), laid
// out like `rows` rows of the level (ls doubles per layer)
// last pass of the finest level: psi_out = psi + da instead of storing da
// more_follow: further half-sweeps of the level come after this pass, so it only stores the colour of its last half-sweep
// (the other colour is recomputed by the next half-sweep before anything reads it): w/2 fewer bytes written
// compact grid of the chunks a pass around the fused visit runs on: four disjoint bands of (strip, chunk row) ranges, n chunks in all
struct VisitRingBands { int s0[4], ns[4], c0[4], nc[4], n; };
struct MarchCorrect { const double *psi; double *psi_out; NatGeom g; };
struct MarchHalo { const double *in_s, *in_n, *res_s, *res_n; size_t ls; int rows; };
int launch_relax_march(hipStream_t st, const KernelOpts &o, const double *in, double *out, const double *res, const SplitGeom &sg, int nl, const RelaxCoef &rc, int c1,
                       int K, int walls, int chunk_rows = 0, const MarchHalo *h = nullptr, const double *coarse = nullptr, const SplitGeom *cg = nullptr,
                       const MarchCorrect *mc = nullptr, int more_follow = 0, const MarchHalo *coarse_halo = nullptr, int region = 0,
                       const int *skip = nullptr, int skip_compact = 0);
// a marched level's visit, 4 + 4 half-sweeps with the prolongation, fused where chunks are interior (k_relax_visit); mc: the finest
// level, the second four apply the correction; nullptr: a level below it, they leave the level's correction in da.
// Returns -1 (nothing launched) where it does not apply.  Chunk height and wave pairs per workgroup: options march_visit_rows / _pairs
int launch_relax_visit(hipStream_t st, const KernelOpts &o, double *da, double *da_alt, const double *res, const SplitGeom &sg, int nl, const RelaxCoef &rc,
                       int walls, const double *coarse, const SplitGeom &cg, const MarchCorrect *mc);
bool relax_visit_fits(int nl, const SplitGeom &sg, int rows, int pairs);
// the chunk height the visit takes on a level (option march_visit_rows; 0: by rounds of the device's wave-pair slots)
int relax_visit_rows(const KernelOpts &o, int nl, const SplitGeom &sg, bool corr);
// the rule by rounds as host arithmetic (no device; tests/test_visit_levels_host.py): -1 where no chunk fits
extern "C" int msom_visit_rows(int hk, int ny, int pairs, int slots);
// host arithmetic of the visit's chunk grid and of the ring chunks around it (no device; tests/test_visit_ring_host.py)
extern "C" int msom_visit_ring(int hk, int ny, int march_rows, int visit_rows, int pairs, int corr, int *geom, int *bands);
// can the lean interior body of the pass address every layer of the level (sg) and, with the correction, of psi (ng)?
bool march_lean_fits(int nl, const SplitGeom &sg, const NatGeom *ng);

// ---- kernels_modes.hip: vertical normal modes (msom_modes_*, msqg/eigmode.h).  One decomposition is nl*nl + nl numbers per column:
// M2L array k*nl + m (layer k from mode m), then iBu_m; `md` holds them as one natural padded layer each (general form), a ModeCoef
// by value (compact form: the same stratification in every column).  mc != nullptr selects the compact instantiation.
struct ModeCoef {
  double m2l[MSOM_MAXNL * MSOM_MAXNL], ibu[MSOM_MAXNL];   // m2l[k * nl + m]
};
// eigenproblem of every column of an ncx x ncy grid from S (geometry g); output array a at out[a * ols + (per_column ? cell : 0)];
// *flag |= MODES_BAD_S / MODES_NOCONV / MODES_WEAK (modes_inl.h) of any column, which then writes nothing.  MODES_WEAK: the column's
// second smallest computed eigenvalue is <= 8 nl 2^-52 times its largest -- below the method's eigenvalue error, so the sign of
// lambda_1 and the choice of the barotropic vector are undetermined.  -1: no kernel for nl
int launch_modes_eig(hipStream_t st, const double *S, const NatGeom &g, int nl, int ncx, int ncy, double *out, size_t ols, int per_column,
                     const ModesLayers &l, int *flag);
// arrays first .. first + cnt - 1 of MSOM_MD_`which` into out, contiguous [cnt][ny][nx]
int launch_modes_get(hipStream_t st, double *out, const double *md, const ModeCoef *mc, const NatGeom &g, int nl, const ModesLayers &l, int which,
                     int first, int cnt);
int launch_modes_rd(hipStream_t st, double *rd, const double *md, const ModeCoef *mc, const NatGeom &g, int nl, int mode);   // interior of MSOM_RD
// in, out: contiguous [nl][ny][nx], may be the same array
int launch_modes_project(hipStream_t st, const double *in, double *out, const double *md, const ModeCoef *mc, const NatGeom &g, int nl,
                         const ModesLayers &l, int to_modes);
// out[0 .. nl) = ke[m], out[nl .. 2 nl) = pe[m] of this tile; partial: 2 nl * modes_energy_stride(g) doubles
int modes_energy_blocks(const NatGeom &g);
int modes_energy_stride(const NatGeom &g);
int launch_modes_energy(hipStream_t st, const double *psi, const double *md, const ModeCoef *mc, const NatGeom &g, int nl, const ModesLayers &l,
                        double *partial, double *out, double D);

// ---- kernels_helm.hip: the nl independent Helmholtz problems lap(p_m) + iBu_m p_m = q_m of the modal PV inversion (msqg/qg.h:136-141),
// every mode of a level in one launch.  Fields are laid out as the layered solver's (mode = layer).  Compact form (hc != nullptr): iBu_m
// by value; general form: iBu per cell from a split-layout array of the level (nl layers).
struct HelmCoef {
  double ibu[MSOM_MAXNL];   // iBu_m
  double rd[MSOM_MAXNL];    // 1 / helm_diag(iBu_m, Delta^2) of the level (product build)
};
struct HelmCount {
  int n[MSOM_MAXNL];        // sweeps mode m takes (0: frozen)
};
// the diagonal 4 - Delta^2 iBu in the documented order (include/msom.h); host and device round alike
MSOM_HD double helm_diag(double ibu, double sqD) {
#ifdef MSOM_STRICT
  return (-(ibu * sqD) + 2.) + 2.;
#else
  return fma(-ibu, sqD, 4.);
#endif
}
HelmCoef helm_coef(const double *ibu, int nl, double sqD);
// one half-sweep of colour `color`, sweep number `sweep`: mode m takes part while cnt.n[m] > sweep.  -1: no kernel for nl
int launch_helm_relax(hipStream_t st, double *da, const double *res, const double *ibu_sp, const HelmCoef *hc, const SplitGeom &sg, int nl,
                      double sqD, int color, int sweep, const HelmCount &cnt, int walls);
// res_m = b_m - lap(a_m) - iBu_m a_m (a, b natural, res split); maxres[m] = max(maxres[m], max |res_m|); want_sum: sum_partial[m * stride + block]
// = sums of b_m per workgroup, helm_residual_blocks(g) of them per mode (second stage: launch_sum_final)
int helm_residual_blocks(const NatGeom &g);
int launch_helm_residual(hipStream_t st, const double *a, const double *b, const double *ibu_sp, const HelmCoef *hc, const NatGeom &g, double *res,
                         const SplitGeom &sg, int nl, double D, double *maxres, double *sum_partial, int stride, int want_sum);

// ---- kernels_spec.hip: wavenumber spectra and spectral fluxes (msom_spec_*, msqg/scripts/fftlib.py); spec_inl.h has the line transform
enum { SPEC_IN_AB = 0, SPEC_IN_UV = 1, SPEC_IN_G = 2 };   // what the row pass transforms: a + i b (b null: a + 0 i), u + i v of psi, g + 0 i
enum { SPEC_CROSS = 0, SPEC_SUM = 1 };                    // what the column pass forms: Re(A conj B) or |A|^2 + |B|^2
// element (layer l, row y, column x) of an input is at off + (l0 + l) * ls + y * pitch + x: a contiguous array or a natural field
struct SpecIn {
  const double *a, *b;      // AB: the two arrays; UV: a = psi; G: a = psi, b = S
  size_t off, ls;
  int pitch, l0, mode;
  double D2, rD2;           // 2 Delta and its reciprocal (UV)
  double dhc[MSOM_MAXNL];   // (G)
};
int spec_prepare_device();   // once per process, before the first launch: the line kernels' dynamic LDS.  -1: refused
// tw: exp(-2 pi i t / nt), t < nt / 2, nt >= nx, ny.  Z, ZT: [layers][ny][nx] / [layers][nx][ny] complex; V: [layers][nx / 2 + 1][ny];
// out2d: null or [layers][ny][nx]; TE: [layers][2][smax + 1]; res: [layers][2][nbins] (bin sums, fluxes)
void launch_spec_rows(hipStream_t st, const SpecIn &in, int nx, int ny, int layers, double2 *Z, const double2 *tw, int nt);
void launch_spec_transpose(hipStream_t st, const double2 *Z, double2 *ZT, int nx, int ny, int layers);
void launch_spec_cols(hipStream_t st, const double2 *ZT, int nx, int ny, int layers, int kind, double scale, double *V, double *out2d, const double2 *tw,
                      int nt);
void launch_spec_shells(hipStream_t st, const double *V, int nx, int ny, int layers, int smax, double *TE);
void launch_spec_final(hipStream_t st, const double *TE, int smax, int nbins, int layers, double dk2, double *res);

// ---- kernels_newqg.hip: tendency of the cell-centred one-layer model (newqg/qg.h:264-284), one layer, one tile.
// One pass psi -> zeta (always stored) and dq, or q_out = q_in + dt * dq when q_out != nullptr (dq then not stored).  psi carries its
// ghost ring (walls) or wrapped copies two cells deep (walls & WALL_PER).  qforc == nullptr: no forcing term.  cek = (hEkb f0) / (2 dh0).
// rows: chunk height (0: automatic); nq_rhs_rows gives the height a launch takes.
int nq_rhs_rows(const NatGeom &g, int rows);
void launch_nq_rhs(hipStream_t st, const double *psi, const double *qforc, double *zeta, double *dq, const NatGeom &g, int walls, double D,
                   double beta, double nu, double cek, double bc_fac, const double *q_in, double *q_out, double dt, int rows);
// the validation chain: ghost ring f[ghost] = bc_fac * (psi[interior] - psi[ghost]) of zeta / q (newqg/qg.h:310-318, corners by the
// y rule), and dq = 0 + ((-J(psi, zeta)) - beta_effect(psi)) (:199-200) from fields with their ghost rings
void launch_nq_ghost(hipStream_t st, const double *psi, double *f, const NatGeom &g, double bc_fac);
void launch_nq_adv(hipStream_t st, const double *psi, const double *zeta, double *dq, const NatGeom &g, double D, double beta);

// ---- kernels_wavelet.hip
void launch_wv_restrict(hipStream_t st, const double *f, const NatGeom &fg, double *c, const NatGeom &cg, int nl);
void launch_wv_recon(hipStream_t st, const double *s, const double *sc, const double *rc, const double *sig, double *out, const NatGeom &fg,
                     const NatGeom &cg, int nl);
void launch_wv_root(hipStream_t st, const double *s, const double *sig, double *r, const NatGeom &g, int nl);
void launch_wv_recon_m(hipStream_t st, const double *s, const double *sc, const double *rc, const double *sig, const double *mc, double *out,
                       const NatGeom &fg, const NatGeom &cg, int nl);
void launch_wv_root_m(hipStream_t st, const double *s, const double *sig, const double *mc, double *r, const NatGeom &g, int nl);
void launch_wv_vert2cell(hipStream_t st, const double *v, const NatGeom &vg, double *c, const NatGeom &cg, int nl);
void launch_wv_vertex_update(hipStream_t st, double *psi, double *psif, const double *c, const double *mask, const NatGeom &vg, const NatGeom &cg, int nl,
                             double dtflt, int nbar, int update_mean);
void launch_wv_qof(hipStream_t st, double *qof, double *q, const double *tmp, const NatGeom &g, int nl, double dtflt, int nbar, int restore);

// ---- kernels_node.hip (vertex-grid variant, qg-node/)
void launch_n_bnd_from(hipStream_t st, double *f, const double *g, const NatGeom &ge, int nl, double c, int use_g_bnd, double gbc, int walls = WALL_ALL);
void launch_n_bnd_const(hipStream_t st, double *f, const NatGeom &ge, int nl, double v, int sp = 0, int walls = WALL_ALL);
void launch_n_mul_mask(hipStream_t st, double *a, double *b, const double *mk, const NatGeom &g, int nl);
void launch_n_del2(hipStream_t st, const double *in, double *out, const NatGeom &g, int nl, double add, double fac, double D);
void launch_n_stretch(hipStream_t st, const double *in, double *out, const double *S2, const NatGeom &g, int nl, double add, double fac,
                      const LayerCoef &lc);
void launch_n_stretch_sqg(hipStream_t st, const double *in, const double *bs, const double *S2S, double *out, const double *S2, const NatGeom &g, int nl,
                          double add, double fac, const LayerCoef &lc);
void launch_n_lap_bs(hipStream_t st, const double *bs, double *out, const NatGeom &g, double D, int walls);
void launch_n_sqg_rhs(hipStream_t st, const double *q, const double *S2S, const double *bs, double *qeff, const NatGeom &g, int nl, double idh00);
void launch_n_rhs_main(hipStream_t st, const double *psi, const double *zeta, const double *pg, const double *S2, const double *topo, double *dq,
                       const NatGeom &g, int nl, int have_pg, int have_topo, double D, double beta, double drag, double f0, double dhb, const LayerCoef &lc);
void launch_n_axpy(hipStream_t st, double *dq, const double *x, const NatGeom &g, int nl, double c);
void launch_n_rhs_pre(hipStream_t st, double *q, const double *psi, double *psi_out, double *zeta, const double *mk, const NatGeom &g, int nl, double D,
                      double bc, double gbc);
void launch_n_del2_bnd(hipStream_t st, const double *in, double *out, const NatGeom &g, int nl, double D, double bc, int use_bnd, double gbc);
void launch_n_rhs_all(hipStream_t st, const double *psi, const double *zeta, const double *tmp, const double *pg, const double *S2, const double *topo,
                      const double *qf, const double *qf3d, const double *mk, const double *d2bs, const double *S2S, double *dq, const NatGeom &g, int nl,
                      double D, double beta, double drag, double f0, double dhb, double nu, double mnu4, const LayerCoef &lc, int have_pg, int have_topo);
void launch_n_add2d(hipStream_t st, double *dq, const double *qf, const NatGeom &g);
void launch_n_rhs_barotropic(hipStream_t st, const double *psi, const double *q, const double *qf, double *dq, const NatGeom &g, double D, double beta,
                             double drag, double nu);
void launch_n_helm(hipStream_t st, const double *psi, double *q, const NatGeom &g, double D, double iRd2);
void launch_n_rowfill(hipStream_t st, double *f, const double *row, const NatGeom &g);
// sp = 1: a, b, mk, S2 in the x-parity split layout (g = their geometry)
void launch_n_relax(hipStream_t st, double *a, const double *b, const double *mk, const double *S2, const NatGeom &g, int nl, int color, double D,
                    double iRd2, const LayerCoef &lc, int sp = 0, const double *S2row = nullptr, int walls = WALL_ALL);
int launch_n_relax_march(hipStream_t st, const double *a_in, double *a_out, const double *b, const double *mk, const double *S2, const NatGeom &g, int nl,
                         int color, int K, double D, double iRd2, const LayerCoef &lc, int rows);
int launch_n_relax_march_s(hipStream_t st, const double *a_in, double *a_out, const double *b, const double *mk, const NatGeom &g, int nl, int color, int K,
                           double D, double iRd2, const LayerCoef &lc, const double *S2row, int partial, int rows);
int launch_n_relax_tile_s(hipStream_t st, const double *a_in, double *a_out, const double *b, const double *mk, const NatGeom &g, int nl, int color, int K,
                          double D, double iRd2, const LayerCoef &lc, const double *S2row);
int launch_n_relax_tile(hipStream_t st, const double *a_in, double *a_out, const double *b, const double *mk, const double *S2, const NatGeom &g,
                        int nl, int ns, double D, double iRd2, const LayerCoef &lc);
void launch_n_residual(hipStream_t st, const double *a, const double *b, const double *mk, const double *S2, double *res, double *maxres,
                       const NatGeom &g, int nl, double D, double iRd2, const LayerCoef &lc, const NatGeom *gres = nullptr,
                       const double *S2row = nullptr, int zb = 0, int walls = WALL_ALL);  // gres: res in the split layout; S2row: row table of an x-independent S2; zb: 0 on the boundary vertices
// coarse levels of a vpoisson cycle in one launch (k_n_mg_coarse): lev[0] = finest of the group
#define NMGC_MAXLEV 8
#define NMGC_NT 1024
struct NCoarseLev { double *da, *res; const double *mask, *S2; NatGeom g; double sqD; };
struct NCoarseArgs { NCoarseLev lev[NMGC_MAXLEV]; int n; double iRd2; LayerCoef lc; };
void launch_n_mg_coarse(hipStream_t st, const NCoarseArgs &a, int nrelax, int nl);
void launch_n_restrict(hipStream_t st, const double *f, const NatGeom &fg, double *c, const NatGeom &cg, int nl, int kind, int fsp = 0, int csp = 0, int zb = 0, int walls = WALL_ALL);
void launch_n_prolong(hipStream_t st, const double *c, const NatGeom &cg, double *f, const NatGeom &fg, int nl, int csp = 0, int fsp = 0, int walls = WALL_ALL);
void launch_n_correct(hipStream_t st, double *a, const double *da, const NatGeom &g, int nl, double bcv, const NatGeom *gda = nullptr, int walls = WALL_ALL);
void launch_n_correct_residual(hipStream_t st, const double *a, double *a_out, const double *da, const NatGeom *gda, double bcv, const double *b, const double *mk,
                               const double *S2, double *res, double *maxres, const NatGeom &g, int nl, double D, double iRd2, const LayerCoef &lc,
                               const NatGeom *gres, const double *S2row, int march);
void launch_n_row_table(hipStream_t st, const double *f, const NatGeom &g, int nl, double *out);
void launch_n_relax_prolong(hipStream_t st, double *a, const double *b, const double *mk, const double *S2, const NatGeom &g, int nl, double D,
                            double iRd2, const LayerCoef &lc, const double *S2row, const double *coarse, const NatGeom &cg, int csp);
void launch_n_relayout(hipStream_t st, const double *src, const NatGeom &sg, int ssp, double *dst, const NatGeom &dg, int dsp, int nl);
void launch_n_umax(hipStream_t st, const double *psi, double *out, const NatGeom &g, int nl, double D);
void launch_n_noise(hipStream_t st, double *n, const NatGeom &g, double amp, unsigned seed, unsigned draw);  // cells and their ghost ring
void launch_n_add_noise(hipStream_t st, double *q, const double *n, const NatGeom &g, const NatGeom &cg, double dts);
void launch_n_diag1d(hipStream_t st, const double *psi, const double *q, const double *qf, double *partial, double *out3, const NatGeom &g, double nu, double D);
void launch_n_ke(hipStream_t st, const double *psi, double *partial, double *out, const NatGeom &g, double D, int walls = WALL_ALL);
// vertex model on tiles: halo strips of a field in either layout, the gather of a level and the tile's window of a gathered level
void launch_n_pack_strip(hipStream_t st, const double *f, const NatGeom &g, int sp, int nl, int i0, int j0, int w, int h, double *buf);
void launch_n_unpack_strip(hipStream_t st, double *f, const NatGeom &g, int sp, int nl, int i0, int j0, int w, int h, const double *buf);
void launch_n_assemble(hipStream_t st, const double *recv, double *f, const NatGeom &g, int nl, int N, int px, int py, int k);
void launch_n_extract(hipStream_t st, const double *f, const NatGeom &g, double *t, const NatGeom &tg, int nl, int ox, int oy);
// cell pyramids on tiles: the noise draw of a tile with its ring, keyed by the global cell; the gathered cell pieces -> a global level
void launch_n_noise_tile(hipStream_t st, double *n, const NatGeom &g, double amp, unsigned seed, unsigned draw, int ox, int oy, int N);
void launch_c_assemble(hipStream_t st, const double *recv, double *f, const NatGeom &g, int nl, int N, int px, int py, int k);

// ---- kernels_node_stats.hip: running statistics of the vertex model (msomn_stats_*); StatsAcc as above, on the held vertices
struct NStatsTile { int ox, oy, N; };   // global index of the tile's vertex (0, 0) and the global side in cells: i or j in {0, N} is the domain boundary
// one sample of weight w into the accumulators of `mask` (1 .. 2^MSOM_ST_NACC - 1); mk: the land mask (1 layer); D2 = 2 Delta.
// -1: no kernel for that mask
int launch_n_stats_acc(hipStream_t st, unsigned mask, const double *psi, const double *q, const double *mk, const StatsAcc &a, const NatGeom &g,
                       int nl, const NStatsTile &t, double w, double D2);
void launch_n_stats_mean(hipStream_t st, double *out, const double *s, double W, const NatGeom &g, int nl);
// which = MSOM_ST_EKE / UQ_EDDY / VQ_EDDY from the mean psi pm (sides set, halo exchanged), sa = KE / UQ / VQ, sq = Q (eddy fluxes); out: natural
void launch_n_stats_derive(hipStream_t st, double *out, const double *pm, const double *mk, const double *sa, const double *sq, double W,
                           const NatGeom &g, int nl, int which, const NStatsTile &t, double D2);

// ---- kernels_state.hip: rows of one layer of a natural field <-> a contiguous staging chunk, with the record digest of the state file
struct StateChunk {
  NatGeom g;        // the tile's natural layout
  int ring;         // 1: the record carries the ghost ring (one tile only): rows and columns count from the ghost cell
  int layer;        // layer of the record
  int y0, rows;     // record rows y0 .. y0 + rows - 1 of that layer, all inside this tile
  int ox, oy;       // the tile's offset in the global grid (cells)
  int gW, gH;       // row width and rows per layer of the record on the GLOBAL grid (ring included): the digest's index space
  int sx0, sw;      // staging: record column of its first column, and its row width
};
void launch_state_pack(hipStream_t st, const double *nat, double *stage, const StateChunk &c, unsigned long long *digest);
void launch_state_unpack(hipStream_t st, const double *stage, double *nat, const StateChunk &c);
void launch_state_digest(hipStream_t st, const double *nat, const StateChunk &c, unsigned long long *digest);
void launch_state_flip(hipStream_t st, double *nat, size_t idx);

#endif
