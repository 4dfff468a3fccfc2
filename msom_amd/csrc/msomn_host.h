// msomn_host.h -- the vertex-grid handle (struct msomn) and the host helpers its units share: msom_node.hip (model and multigrid),
// msomn_tiles.hip (the model on tiles: decomposition, halo exchange, gather), msomn_io.hip (NetCDF IO and the driver msomn_run),
// msomn_state.hip (state file, include/msomn_state.h), msomn_floats.hip (Lagrangian floats, include/msomn_floats.h).  The profile slots (prof_slot.h) are the layered model's.  Not installed.
// The floats' host engine (floats_host.hip) does not include it; its header is included here for fh::Opts.
#ifndef MSOMN_HOST_H
#define MSOMN_HOST_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <string>
#include <vector>

#include "comm.h"
#include "floats_host.h"
#include "kernels.h"
#include "node_tile_inl.h"
#include "prof_slot.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e__ = (x);                                                                  \
    if (e__ != hipSuccess) {                                                               \
      msom_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e__), __FILE__, __LINE__, #x); \
      return MSOM_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)

struct NLevel {
  int n;        // cells per side: (n + 1)^2 vertices
  double D;     // L0 / n
  NatGeom g;
  double *da = nullptr, *res = nullptr, *mask = nullptr, *S2 = nullptr;  // level 0: mask and S2 alias the model fields
  double *da2 = nullptr;         // second correction buffer (the tiled smoother works out of place)
  // wide levels (option node_split): da and res in the x-parity split layout of geometry ga, with split copies of mask and S2
  int sp = 0;
  NatGeom ga;                    // geometry of da / res: g, or the split geometry
  double *mask_s = nullptr, *S2_s = nullptr;
  double *S2row_buf = nullptr;   // allocation behind S2row
  double *S2row = nullptr;       // [nlm][n + 1] when S2 does not depend on x (and the option s2_rows is on), else null
  // vertex model on tiles: a level above the gather level holds the tile's window (g rectangular, n still the global side); walls are
  // the sides of g that are sides of the domain
  int tiled = 0, walls = WALL_ALL;
};
// a tile's window of level kg of a cell pyramid with its ring: what the rank gives to the gather (s) and takes back from the gathered
// levels (s and r), msomn_cells.hip
struct CellPiece {
  NatGeom g;
  double *s = nullptr, *r = nullptr;
};
enum { NSC_RES = 0, NSC_UMAX = 1, NSC_KE = 2, NSC_DIAG = 3 /* 3 slots */, NSC_FLOATS = 6 /* 2 slots */, NSC_COUNT = 8 };

// option profile: HIP-event pairs around the finest-level launches of the vertex model (bench.py's per-kernel entries)
enum { NP_RELAX, NP_RELAX_PROLONG, NP_RESIDUAL, NP_CORRECT, NP_RHS, NP_COARSE, NP_MARCH, NP_CORR_RES, NP_COUNT };
static const char *const NP_NAMES[NP_COUNT] = {"relax_fine", "relax_prolong_fine", "residual", "correct", "rhs", "coarse", "march_fine", "correct_residual"};

struct msomn {
  NodeParams p;
  int profile = 0;
  ProfSlot prof[NP_COUNT];
  std::string params_text;
  int N = 0, nl = 1, nlm = 1;
  double D = 0, psi_bc = 0., iRd2_low = 0.;
  double tolerance = 1e-3;
  int nitermax = 100, nitermin = 1, nrelax = 5, quiet = 0;  // nodal-poisson.h:19-23
  // stochastic forcing (-D_STOCHASTIC of the reference): cell-scalar noise n_stoch, wavelet-filtered (qg-node/qg_stochastic.h)
  int stochastic = 0, corrector_step = 0, cnlev = 0;
  // option noise_mode: 0 the reference's serial rand() stream on the host (one per process), 1 the counter-based device generator
  // k_n_noise, keyed by the handle's seed and numbered by the handle's draw counter (set_const: 0)
  int noise_mode = 0;
  unsigned seed = 1, noise_draw = 0;
  int pg_set = 0, topo_set = 0;   // psi_pg / topo have been set (zero until then: their terms of the tendency are skipped by k_n_rhs_all)
  int forcing_3d = 0;  // -DFORCING_3D: switched on by setting MSOMN_QFORC3D
  int sqg = 0;         // surface-QG variant (params key sqg): sqg_baroclinic_ms.h:77-98,502,545-547
  double *qeff = nullptr, *d2bs = nullptr;  // sqg scratch: rhs of the inversion, laplacian(bs)
  // wavelet filter of the vertex model (qg_baroclinic_ms.h:346-400): cell pyramids of s, r (nl layers), sig_lev, mask_c
  std::vector<NatGeom> wg;
  std::vector<double *> ws, wr, wsig, wmc;
  int wv_ready = 0, nbar = 0;
  std::vector<NatGeom> cg;
  std::vector<double *> cs, cr, csig;  // cs[0] = n_stoch
  int mg_coarse = 32;   // the levels of <= (mg_coarse + 1)^2 vertices of a cycle in one launch (k_n_mg_coarse); 0: off
  int node_march_rows = 0;  // option: chunk height of the marching passes (0: automatic; k_n_relax_march_s: 12)
  int node_march = 0;   // levels of >= node_march vertices per side: K = 4 chained colour half-sweeps per pass (k_n_relax_march, rows
                        // software-prefetched one step ahead).  Measured at 2049^2 x 3: 27.1 vs 26.6 ms per step, 513^2 x 3: 4.2 vs 3.1 --
                        // half the bytes, but in the natural layout half of the lanes idle in every half-sweep and the vertex column
                        // solve (vertex-dependent coefficients, one reciprocal per layer) is arithmetic-bound: off
  int node_pfused = 1;   // option: prolongation folded into the first colour pass of the split levels
  int node_tile_max = 513;  // option: ... and of <= node_tile_max vertices per side (wider levels: the colour passes are no longer launch-bound)
  int node_march_tail1 = 1; // option: 9 half-sweeps as passes of 4 + 4 + a colour pass (measured 13.96 -> 13.43 ms per step) instead of 4 + 3 + 2 (0)
  int node_tile_k = 8;      // option: half-sweeps per LDS-tiled pass (2..8)
  int node_tile_s = 65;     // option: split levels of >= node_tile_s (and < node_march_s) vertices per side: LDS-tiled passes of up to 4 colour half-sweeps (0: off)
  int node_rhs_fused = 1;   // option: the baroclinic tendency in three passes (k_n_rhs_pre, k_n_del2_bnd, k_n_rhs_all) instead of twelve
  int node_corr_fused = 2;  // option: the correction a += da rides in the next cycle's residual pass (k_n_correct_residual)
  double *psi_alt = nullptr;
  hipEvent_t ev_res = nullptr;   // marks the copy of max |res| to the host inside vpoisson
  int node_march_s = 2049;  // option: split levels of >= node_march_s vertices per side chain up to 4 colour half-sweeps per pass (k_n_relax_march_s,
                            // round 3).  2049^2 x 3, 9 cycles per solve (tools/ab_node_prof.py): 3 passes of 83 us replace 9 colour launches of 33 us:
                            // 17.3 -> 16.6 ms per step; on the 1025^2 and 513^2 levels the pass loses (17.4 / 18.4): too few chunks for a
                            // marching wavefront; three steps of software prefetch instead of one and chunk heights 8 .. 24 change nothing
  int s2_xuniform = 0;   // set_const: S2 does not depend on x
  int s2_rows = 1;       // option: use row tables of S2 in the smoother and the residual when S2 does not depend on x
  int node_split = 65;   // option: levels of >= node_split vertices per side keep da / res / mask / S2 copies in the x-parity split layout (0: off)
  int tiled_relax = 0;  // option: LDS-tiled smoother passes (1-2 sweeps per pass) on the wide levels; measured 3 % faster at 4097^2 x 3, 7 % slower at 2049^2 x 3
  NatGeom g;
  double *f[MSOMN_NFIELDS] = {nullptr};
  int fl[MSOMN_NFIELDS] = {0};
  LayerCoef lc;
  int nlev = 0;
  std::vector<NLevel> lev;
  double *d_scal = nullptr, *h_scal = nullptr, *partial = nullptr, *d_row = nullptr, *h_row = nullptr;
  hipStream_t st = nullptr;
  int const_set = 0;
  double t = 0, dt = 1., tnext = HUGE_VAL, previous = 0;
  int iter = 0;
  msom_mgstats mg = {0, 0, 0, 0, 0};
  // vertex model on tiles (msomn_create_tiled, msomn_tiles.hip, node_tile_inl.h).  One tile: ntiles = 1, walls = WALL_ALL, g square,
  // no communicator, and none of the rest is used
  int px = 1, py = 1, rank = 0, ntiles = 1, walls = WALL_ALL;
  int ox = 0, oy = 0;          // global index of the tile's vertex (0, 0)
  int kg = 0;                  // gather level (msomn_set_const): levels below live on the tiles, kg and up on the global grid on every rank; one tile: 0
  Comm *comm = nullptr;
  int nb[4] = {-1, -1, -1, -1};   // ranks behind the W, E, S, N sides (DIR_* of comm.h), -1: wall
  NLevel piece;                // the tile's window of level kg in the natural layout: what the rank gives to and takes from the gather
  double *gsend = nullptr, *grecv = nullptr;   // gather buffers: one piece, ntiles pieces
  size_t gcount = 0;           // doubles of gsend
  int tile_err = 0;            // a halo exchange inside a sweep failed: the solve answers with it
  // option wavelet_tiles: the noise and the scale filter run on tiles (msomn_cells.hip); the pyramids above then hold the tile's windows
  // below the gather level and the global levels from it on
  int wavelet_tiles = 0;
  CellPiece cpiece, wpiece;
  // option io_tiles: msomn_state_save / _load, msomn_write_nc / _read_nc and msomn_run are collective calls on tiles instead of refused
  int io_tiles = 0;
  long nexch = 0;              // halo exchanges since the last msomn_profile_reset (msomn_get_param("exchanges"))
  // state file and the driver's checkpoints (include/msomn_state.h)
  long state_flip = -1;             // msomn_state_dbg_flip: element the next load flips on the device (< 0: off)
  int ckpt_steps = 0, resume = 0;   // options of msomn_run
  int run_loaded = 0;               // the last load found the driver record `run`: run_ev holds it
  double run_ev[6] = {0, 0, 0, 0, 0, 0};   // tout, tdiag, tflt, output directory number, records of vars.nc, bytes of diag_1d.dat
  // running statistics on the device (msomn_stats_*, msomn_stats.hip); nothing is allocated until msomn_stats_begin
  unsigned stats_mask = 0;                // accumulators selected by the last msomn_stats_begin since msomn_set_const (0: none)
  StatsAcc stats = {};                    // the selected accumulators, natural layout of the tile, nl layers each
  double *stats_scr = nullptr;            // where a derived quantity is formed (allocated by the first msomn_stats_get that needs it)
  double stats_W = 0.;                    // sum of the weights: every weight is known on the host, so W = W + w is formed there
  int stats_on = 0, stats_every = 1;      // options "stats", "stats_every"
  long stats_count = 0;                   // msomn_step calls seen since msomn_stats_begin (every stats_every-th one samples)
  long stats_samples = 0;                 // samples taken since msomn_stats_begin, automatic and by hand
  // Lagrangian floats (msomn_floats_*, msomn_floats.hip); nothing is allocated until msomn_floats_begin
  fh::Opts floats;                        // the state and the options "floats", "floats_tiles", "floats_msg_cap" (floats_host.h)
};

// ---- msom_node.hip
// [layers][n+1][n+1] contiguous (host or device) <-> padded natural layout
int upload_g(msomn *m, double *dst, const NatGeom &g, int nl, const double *a);
int download_g(msomn *m, const double *src, const NatGeom &g, int nl, double *a);
// msomn_set_const in two parts.  node_const_inputs transforms the inputs in place (S2: N^2 -> f^2 / N^2, S2S: N^2 -> f / N^2, topo *=
// scale_topo) and is not idempotent; node_const_derived builds everything that follows from the transformed values (layer metrics,
// iRd2_low, s2_xuniform, the levels and their layouts, the noise pyramid, the DT clamps, boundary(psi)) and leaves q and noise_draw alone.
int node_const_inputs(msomn *m);
int node_const_derived(msomn *m);
double node_clamped_dt(const msomn *m);   // p.DT after the clamps of node_const_derived
NatGeom cell_geom(int n);                 // natural layout of an n x n cell field (the noise and wavelet pyramids)
void node_noise_ghosts(msomn *m);         // the ghost ring of the noise field cs[0], as the filter leaves it

// ---- msomn_tiles.hip
NatGeom node_geom_rect(int tx, int ty);         // natural layout of a tile of tx x ty cells: (tx + 1) x (ty + 1) vertices
NatGeom node_geom_split_rect(int tx, int ty);   // its x-parity split layout
// one-deep halo of a field of the tile in either layout, corners included: x phase, then y phase over the fresh halo columns.
// Collective; a no-op on one tile
int nt_exchange(msomn *m, double *f, const NatGeom &g, int sp, int nl);
int nt_reduce(msomn *m, int slot, int n, int op);   // all-reduce of d_scal[slot .. slot + n) into h_scal (one tile: a plain read)
// the tiles' pieces of level kg (natural layout, geometry pg) -> the global level (geometry gg) on every rank
int nt_gather(msomn *m, const double *piece, const NatGeom &pg, int nl, double *global, const NatGeom &gg);
int nt_setup(msomn *m, int px, int py, int rank, const void *id128);   // decomposition, communicator, the fused options off
void nt_free_gather(msomn *m);   // the piece and the gather buffers (msomn_set_const allocates them again)
void nt_free(msomn *m);
// MSOM_ERR_CONFIG with a message naming the call if the handle has more than one tile
int nt_refuse(const msomn *m, const char *call);
int nt_io_refuse(const msomn *m, const char *call);   // the same unless the option io_tiles is on
// One code on every rank (collective; one tile: r as it is).  r is this rank's verdict on something only it could see, with its message
// set; the ranks' codes meet in one all-reduce and every rank returns the lowest.  A rank that had nothing to object says so
int nt_agree(msomn *m, int r, const char *call);
// the owned window of `rank` (ntile_owned_range; cells = 1: its cells, which no other tile holds) of a field of layout g on the tile
struct NodeOwned { NatGeom g; int ox, oy, gn; };   // g: the field's layout with nx, ny the owned extent; gn: the global side
NodeOwned nt_owned(const msomn *m, const NatGeom &g, int cells, int rank);
// The owned windows of dev ([layers] in geometry g) of all ranks -> the global [layers][gn][gn] array in `out` on rank 0 (the others:
// left empty).  digest: device word that takes this rank's share of the record digest (k_state_rows).  Collective
int nt_gather_owned(msomn *m, const double *dev, const NatGeom &g, int layers, int cells, unsigned long long *digest, std::vector<double> &out);

// ---- msomn_cells.hip: the cell pyramids on tiles (option wavelet_tiles), all collective
NatGeom cell_geom_rect(int nx, int ny);   // natural layout of a tile of nx x ny cells
int nt_exchange_cells(msomn *m, double *f, const NatGeom &g, int nl);   // ring of a cell field: the neighbours' edge cells, corners included
int ct_ring(msomn *m, double *f, const NatGeom &g, int nl, int bc);     // the boundary condition on the tile's walls, then the exchange
int ct_stoch_setup(msomn *m);                  // stoch_setup: the noise pyramid and csig
int ct_wv_setup(msomn *m);                     // wv_setup: the filter pyramid, wsig and wmc
int ct_noise_filter(msomn *m, int ghosts_set); // cell_wavelet_filter: 2 kg - 1 exchanges and one all-gather
int ct_masked_apply(msomn *m);                 // wv_masked_apply: the same
void ct_free_piece(CellPiece &P);

// ---- msomn_stats.hip
void nstats_drop(msomn *m);               // frees everything msomn_stats_begin allocated (msomn_set_const, msomn_destroy)
int nstats_sample(msomn *m, double w);    // one sample of MSOMN_PSI / MSOMN_Q as held (halo of psi fresh), W = W + w; queued, not synchronised

// ---- msomn_floats.hip
void nfloats_drop(msomn *m);                          // frees everything msomn_floats_begin allocated (msomn_set_const, msomn_destroy)
int nfloats_hook(msomn *m, int stage, double tnext);  // one stage of msomn_step's floats, queued on m->st with m->dt; no host wait
bool nfloats_param(msomn *m, const char *key, double *v);   // the "floats*" keys of msomn_get_param (on tiles the counters are collective)

// ---- msomn_state.hip
// msomn_state_save with the driver record `run` (run6: tout, tdiag, tflt, directory number, records of vars.nc, bytes of diag_1d.dat)
int nstate_save_run(msomn *m, const char *path, unsigned flags, const double *run6);

#endif
