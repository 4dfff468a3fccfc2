// msom_node.hip -- host side of the vertex-grid QG variant (C ABI msomn_*, include/msom.h).
//
// Restates the control flow of qg-node/qg.h (update_qg :334-354, advance_qg :291-302, adjust_dt
// :258-284, set_vars :404-450, set_const :465-524), qg_baroclinic_ms.h (rhs_pv_baroclinic :104-196,
// comp_q :199-211, invert_q :217-225, init :449-510), qg_barotropic.h and the nodal multigrid
// vpoisson (nodal-poisson.h:19-143) on top of the kernels of kernels_node.hip.  No CPU fallback.
#include "msomn_host.h"
#include "step_dt_inl.h"

// option profile: the launches queued while a Timed lives count as one launch of the slot (on = false: not timed)
struct Timed {
  msomn *m;
  ProfSlot &ps;
  const bool on;
  Timed(msomn *m, int slot, bool on = true) : m(m), ps(m->prof[slot]), on(on && m->profile) { prof_slot_begin(ps, m->st, this->on); }
  ~Timed() { prof_slot_end(ps, m->st, on); }
};

// the square grid of n x n cells (msomn_tiles.hip has the rectangular forms a tile uses)
static NatGeom node_geom(int n) { return node_geom_rect(n, n); }
static NatGeom node_geom_split(int n) { return node_geom_split_rect(n, n); }
static void free_level(NLevel &L, int k);
static int dalloc(double **p, size_t n) {
  HIPCHK(hipMalloc((void **)p, n * sizeof(double)));
  HIPCHK(hipMemset(*p, 0, n * sizeof(double)));
  return MSOM_OK;
}
static int field_layers(const msomn *m, int f) {
  if (f == MSOMN_PSIF) return m->nl;
  return f == MSOMN_S2 ? m->nlm : (f == MSOMN_TOPO || f == MSOMN_QFORC || f == MSOMN_MASK || f == MSOMN_BS || f == MSOMN_S2S) ? 1 : m->nl;
}

// [layers][ny][nx] contiguous (host or device) <-> padded natural layout
int upload_g(msomn *m, double *dst, const NatGeom &g, int nl, const double *a) {
  const size_t n1 = g.nx, n2 = g.ny;
  for (int l = 0; l < nl; l++)
    HIPCHK(hipMemcpy2DAsync(dst + nat_idx(g, l, 0, 0), g.pitch * sizeof(double), a + (size_t)l * n1 * n2, n1 * sizeof(double), n1 * sizeof(double), n2,
                            hipMemcpyDefault, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
int download_g(msomn *m, const double *src, const NatGeom &g, int nl, double *a) {
  const size_t n1 = g.nx, n2 = g.ny;
  for (int l = 0; l < nl; l++)
    HIPCHK(hipMemcpy2DAsync(a + (size_t)l * n1 * n2, n1 * sizeof(double), src + nat_idx(g, l, 0, 0), g.pitch * sizeof(double), n1 * sizeof(double), n2,
                            hipMemcpyDefault, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

static void free_level(NLevel &L, int k) {
  for (double **q : {&L.da, &L.da2, &L.res, &L.mask_s, &L.S2_s, &L.S2row_buf}) { if (*q) (void)hipFree(*q); *q = nullptr; }
  if (k > 0) for (double **q : {&L.mask, &L.S2}) { if (*q) (void)hipFree(*q); *q = nullptr; }
  L.S2row = nullptr;
}
// buffers of level k with the natural geometry g: da and res are sized for either layout (the layout is chosen in choose_layouts from
// the option node_split); level 0's mask and S2 are the model fields
static int alloc_level(msomn *m, NLevel &L, int k, const NatGeom &g) {
  L.n = m->N >> k;
  L.D = m->p.L0 / L.n;
  L.g = L.ga = g;
  L.sp = 0;
  int r;
  const size_t lsa = std::max(g.ls, node_geom_split_rect(g.nx - 1, g.ny - 1).ls);
  if ((r = dalloc(&L.da, lsa * m->nl)) || (r = dalloc(&L.da2, lsa * m->nl)) || (r = dalloc(&L.res, lsa * m->nl))) return r;
  if (k == 0) { L.mask = m->f[MSOMN_MASK]; L.S2 = m->f[MSOMN_S2]; }
  else if ((r = dalloc(&L.mask, g.ls)) || (r = dalloc(&L.S2, g.ls * m->nlm))) return r;
  return MSOM_OK;
}
extern "C" void msomn_destroy(msomn_t *m) {
  if (!m) return;
  for (int k = 0; k < MSOMN_NFIELDS; k++) if (m->f[k]) (void)hipFree(m->f[k]);
  for (size_t k = 0; k < m->lev.size(); k++) free_level(m->lev[k], (int)k);
  nt_free(m);
  nstats_drop(m);
  nfloats_drop(m);
  for (size_t k = 0; k < m->cs.size(); k++) {
    if (m->cs[k]) (void)hipFree(m->cs[k]);
    if (m->cr[k]) (void)hipFree(m->cr[k]);
    if (m->csig[k]) (void)hipFree(m->csig[k]);
  }
  for (auto *v : {&m->ws, &m->wr, &m->wsig, &m->wmc})
    for (double *q : *v) if (q) (void)hipFree(q);
  ct_free_piece(m->cpiece);
  ct_free_piece(m->wpiece);
  if (m->psi_alt) (void)hipFree(m->psi_alt);
  if (m->ev_res) (void)hipEventDestroy(m->ev_res);
  if (m->qeff) (void)hipFree(m->qeff);
  if (m->d2bs) (void)hipFree(m->d2bs);
  if (m->d_scal) (void)hipFree(m->d_scal);
  if (m->partial) (void)hipFree(m->partial);
  if (m->d_row) (void)hipFree(m->d_row);
  if (m->h_scal) (void)hipHostFree(m->h_scal);
  if (m->h_row) (void)hipHostFree(m->h_row);
  if (m->st) (void)hipStreamDestroy(m->st);
  delete m;
}

static int node_alloc(msomn *m) {
  for (int k = 0; k < MSOMN_NFIELDS; k++) {
    m->fl[k] = field_layers(m, k);
    int r = dalloc(&m->f[k], m->g.ls * m->fl[k]);
    if (r) return r;
  }
  m->lev.resize(m->nlev);
  // on tiles the levels are allocated by msomn_set_const: which of them live on the tile depends on the option mg_coarse
  for (int k = 0; k < m->nlev && m->ntiles == 1; k++) {
    int r = alloc_level(m, m->lev[k], k, node_geom(m->N >> k));
    if (r) return r;
  }
  int r;
  if ((r = dalloc(&m->d_scal, NSC_COUNT))) return r;
  const int nblk = ((m->g.nx + 63) / 64) * ((m->g.ny + 3) / 4);
  // three partial arrays, each followed by the chunk sums of launch_sum_final
  if ((r = dalloc(&m->partial, 3 * ((size_t)nblk + 64))) || (r = dalloc(&m->d_row, m->N + 1))) return r;
  HIPCHK(hipHostMalloc((void **)&m->h_scal, NSC_COUNT * sizeof(double)));
  HIPCHK(hipHostMalloc((void **)&m->h_row, (m->N + 1) * sizeof(double)));
  // set_vars qg-node/qg.h:426-430: mask = 1 on every vertex, its BC 0 on the four walls; S2 = N2[l]
  // (qg_baroclinic_ms.h:471-476)
  // (a tile: the walls are the sides of the tile that are sides of the domain)
  const size_t n1 = m->g.nx, n2 = m->g.ny;
  std::vector<double> h(n1 * n2 * (m->nlm > 1 ? m->nlm : 1));
  for (size_t j = 0; j < n2; j++)
    for (size_t i = 0; i < n1; i++)
      h[j * n1 + i] = ((i == 0 && (m->walls & WALL_W)) || (j == 0 && (m->walls & WALL_S)) || (i == n1 - 1 && (m->walls & WALL_E)) || (j == n2 - 1 && (m->walls & WALL_N))) ? 0. : 1.;
  if ((r = upload_g(m, m->f[MSOMN_MASK], m->g, 1, h.data()))) return r;
  if (m->nl > 1) {
    // sqg: N2 = [surface, interfaces ...]; S2 layers 1..nl-1 of sqg_baroclinic_ms.h are the interfaces below layers 0..nl-2
    for (int l = 0; l < m->nlm; l++) for (size_t k = 0; k < n1 * n2; k++) h[l * n1 * n2 + k] = m->p.N2[l + (m->sqg ? 1 : 0)];
    if ((r = upload_g(m, m->f[MSOMN_S2], m->g, m->nlm, h.data()))) return r;
    if (m->sqg) {
      for (size_t k = 0; k < n1 * n2; k++) h[k] = m->p.N2[0];
      if ((r = upload_g(m, m->f[MSOMN_S2S], m->g, 1, h.data())) || (r = dalloc(&m->qeff, m->g.ls * m->nl)) || (r = dalloc(&m->d2bs, m->g.ls))) return r;
    }
  }
  return MSOM_OK;
}

static msomn *node_create(const NodeParams &p, const char *text, int px = 1, int py = 1, int rank = 0, const void *id128 = nullptr) {
  if (p.nl < 1 || p.nl > MSOM_FASTNL) { msom_set_error("nl = %d outside the supported range 1..%d", p.nl, MSOM_FASTNL); return nullptr; }
  if (p.N < 2 || (p.N & (p.N - 1))) { msom_set_error("N = %d must be a power of two >= 2", p.N); return nullptr; }
  if (p.bc_fac == -1) { msom_set_error("bc_fac = -1 (periodic vertex grid) is not supported"); return nullptr; }
  if (p.sqg && p.nl < 2) { msom_set_error("sqg = 1 needs nl >= 2 (qg-node/sqg_baroclinic_ms.h is the multi-layer model)"); return nullptr; }
  if (const char *why = ntile_check(p.N, px, py, rank)) {
    msom_set_error("msomn_create_tiled: %s (N = %d, %d x %d tiles, rank %d)", why, p.N, px, py, rank);
    return nullptr;
  }
  if (px * py > 1 && !id128) { msom_set_error("msomn_create_tiled: null communicator id"); return nullptr; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    msom_set_error("no HIP device available: libmsomhip has no CPU fallback");
    return nullptr;
  }
  msomn *m = new msomn;
  m->p = p;
  if (text) m->params_text = text;
  m->N = p.N; m->nl = p.nl; m->nlm = p.nl > 1 ? p.nl - 1 : 1;
  m->sqg = p.sqg != 0;
  m->D = p.L0 / p.N;
  m->tolerance = p.TOLERANCE;
  m->nlev = ntile_nlev(p.N);  // coarsest level: 2 x 2 cells, one interior vertex
  memset(&m->lc, 0, sizeof m->lc);
  if (hipStreamCreate(&m->st) != hipSuccess) { msom_set_error("hipStreamCreate failed"); delete m; return nullptr; }
  if (nt_setup(m, px, py, rank, id128) != MSOM_OK || node_alloc(m) != MSOM_OK) { msomn_destroy(m); return nullptr; }
  return m;
}
extern "C" msomn_t *msomn_create_tiled(const char *text, int px, int py, int rank, const void *id128) {
  if (!text) { msom_set_error("null params text"); return nullptr; }
  NodeParams p;
  msom_node_params_defaults(&p);
  msom_node_params_parse_text(&p, text);
  return node_create(p, text, px, py, rank, id128);
}
extern "C" msomn_t *msomn_create_str(const char *text) {
  if (!text) { msom_set_error("null params text"); return nullptr; }
  NodeParams p;
  msom_node_params_defaults(&p);
  msom_node_params_parse_text(&p, text);
  return node_create(p, text);
}
extern "C" msomn_t *msomn_create(const char *path) {
  NodeParams p;
  msom_node_params_defaults(&p);
  const char *pp = path ? path : "params.in";
  if (msom_node_params_parse_file(&p, pp)) return nullptr;
  std::string text;
  if (FILE *fp = fopen(pp, "rb")) {
    char buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, k);
    fclose(fp);
  }
  return node_create(p, text.c_str());
}

static int choose_layouts(msomn *m);
extern "C" int msomn_set_option(msomn_t *m, const char *key, double v) {
  if (!m || !key) return MSOM_ERR_ARG;
  if (m->ntiles > 1) {
    // the fused passes have no tiled form: they stay off, whatever is asked for (msomn_get_param shows the resolved value)
    for (const char *off : {"tiled_relax", "node_pfused", "node_corr_fused", "node_rhs_fused", "node_tile_s", "node_march", "node_march_s"})
      if (!strcmp(key, off)) return MSOM_OK;
    if (!strcmp(key, "stochastic") && v != 0. && !m->wavelet_tiles) return nt_refuse(m, "option stochastic");
    if (!strcmp(key, "mg_coarse") && m->const_set) {
      msom_set_error("option mg_coarse decides which levels live on the tiles: set it before msomn_set_const");
      return MSOM_ERR_STATE;
    }
  }
  if (!strcmp(key, "TOLERANCE")) m->tolerance = v;
  else if (!strcmp(key, "NITERMAX")) m->nitermax = (int)v;
  else if (!strcmp(key, "NITERMIN")) m->nitermin = (int)v;
  else if (!strcmp(key, "DT")) m->p.DT = v;
  else if (!strcmp(key, "quiet")) m->quiet = (int)v;
  else if (!strcmp(key, "profile")) m->profile = (int)v;
  else if (!strcmp(key, "tiled_relax")) m->tiled_relax = (int)v;
  else if (!strcmp(key, "node_pfused")) m->node_pfused = (int)v;
  else if (!strcmp(key, "node_corr_fused")) m->node_corr_fused = (int)v;
  else if (!strcmp(key, "node_rhs_fused")) m->node_rhs_fused = (int)v;
  else if (!strcmp(key, "node_tile_s")) m->node_tile_s = (int)v;
  else if (!strcmp(key, "node_march_tail1")) m->node_march_tail1 = (int)v;
  else if (!strcmp(key, "node_tile_max")) m->node_tile_max = (int)v;
  else if (!strcmp(key, "node_tile_k")) { if (v < 2 || v > 8) return MSOM_ERR_ARG; m->node_tile_k = (int)v; }
  else if (!strcmp(key, "s2_rows")) { m->s2_rows = (int)v; if (m->const_set) return choose_layouts(m); }
  else if (!strcmp(key, "node_split")) { m->node_split = (int)v; if (m->const_set) return choose_layouts(m); }
  else if (!strcmp(key, "node_march")) m->node_march = (int)v;
  else if (!strcmp(key, "node_march_s")) m->node_march_s = (int)v;
  else if (!strcmp(key, "node_march_rows")) m->node_march_rows = (int)v;
  else if (!strcmp(key, "mg_coarse")) { m->mg_coarse = (int)v; if (m->const_set) return choose_layouts(m); }
  else if (!strcmp(key, "stochastic")) m->stochastic = (int)v;
  else if (!strcmp(key, "wavelet_tiles")) {   // the noise and the scale filter on tiles (msomn_cells.hip); one tile: accepted, no effect
    if (v != 0. && v != 1.) { msom_set_error("wavelet_tiles = %g: 0 (the wavelet pyramid is refused on tiles) or 1", v); return MSOM_ERR_ARG; }
    m->wavelet_tiles = (int)v;
  }
  else if (!strcmp(key, "io_tiles")) {   // state files, NetCDF and msomn_run as collective calls (msomn_state.hip, msomn_io.hip); one tile: accepted, no effect
    if (v != 0. && v != 1.) { msom_set_error("io_tiles = %g: 0 (state files, NetCDF and msomn_run are refused on tiles) or 1", v); return MSOM_ERR_ARG; }
    m->io_tiles = (int)v;
  }
  else if (!strcmp(key, "ckpt_steps")) m->ckpt_steps = (int)v;   // msomn_run, include/msomn_state.h
  else if (!strcmp(key, "resume")) m->resume = (int)v;
  else if (!strcmp(key, "stats")) {   // msomn_step takes one sample per stats_every steps (msomn_stats.hip)
    if ((int)v && !m->stats_mask) { msom_set_error("option stats = 1 before msomn_stats_begin"); return MSOM_ERR_STATE; }
    m->stats_on = (int)v != 0;
  }
  else if (!strcmp(key, "stats_every")) {
    if (!(v >= 1)) { msom_set_error("option stats_every = %g", v); return MSOM_ERR_ARG; }
    m->stats_every = (int)v;
  }
  else if (!strncmp(key, "floats", 6)) return fh::set_option(m->floats, key, v);   // floats, floats_tiles, floats_msg_cap (msomn_floats.h)
  else if (!strcmp(key, "seed")) { m->seed = (unsigned)v; srand(m->seed); }
  else if (!strcmp(key, "noise_mode")) {
    if (v != 0. && v != 1.) { msom_set_error("noise_mode = %g: 0 (serial rand() stream on the host) or 1 (device generator)", v); return MSOM_ERR_ARG; }
    m->noise_mode = (int)v;
  }
  else { msom_set_error("unknown option %s", key); return MSOM_ERR_ARG; }
  return MSOM_OK;
}
// average duration of a profile slot ("relax_fine", "relax_prolong_fine", "residual", "correct", "rhs", "coarse") since the last reset
extern "C" int msomn_profile_read(msomn_t *m, const char *slot, double *avg_ms, long *launches) {
  if (!m || !slot) return MSOM_ERR_ARG;
  for (int k = 0; k < NP_COUNT; k++)
    if (!strcmp(slot, NP_NAMES[k])) {
      prof_slot_collect(m->prof[k], m->st);
      if (avg_ms) *avg_ms = m->prof[k].launches ? m->prof[k].total_ms / m->prof[k].launches : 0.;
      if (launches) *launches = m->prof[k].launches;
      return MSOM_OK;
    }
  msom_set_error("unknown profile slot %s", slot);
  return MSOM_ERR_ARG;
}
extern "C" int msomn_profile_reset(msomn_t *m) {
  if (!m) return MSOM_ERR_ARG;
  hipStreamSynchronize(m->st);
  for (auto &ps : m->prof) { ps.used = 0; ps.total_ms = 0; ps.launches = 0; }
  m->nexch = 0;
  return MSOM_OK;
}
// K cap of the chained split pass (k_n_relax_march_s) on level L: windows of K stages x nl layers in registers.  0 where the pass
// cannot run: nl > 6, or nl > 1 without row tables of S2.  relax_sweeps and msomn_get_param("node_march_kmax")
static int node_march_kmax(const msomn *m, const NLevel &L) {
  if (m->nl > 6 || (m->nl > 1 && !L.S2row)) return 0;
  return m->nl <= 4 ? 4 : 3;
}
// the path of level k's sweeps (msomn_get_param("relax_path_<k>")): natural colour passes, split colour passes, LDS-tiled split passes
// (k_n_relax_tile_s; relax_sweeps takes them only for 2 sweeps or more), chained split passes (k_n_relax_march_s), inside the one-launch
// coarse group (k_n_mg_coarse), and the natural-layout options node_march (k_n_relax_march) and tiled_relax (k_n_relax_tile)
enum { NRP_COLOR = 0, NRP_SPLIT = 1, NRP_TILE_S = 2, NRP_MARCH_S = 3, NRP_COARSE = 4, NRP_MARCH = 5, NRP_TILE = 6 };
static int sweep_path(const msomn *m, int k) {
  const NLevel &L = m->lev[k];
  if (L.tiled) return L.sp ? NRP_SPLIT : NRP_COLOR;   // a tiled level: one launch and one halo exchange per colour
  if (L.sp && m->node_march_s && L.n + 1 >= m->node_march_s && node_march_kmax(m, L)) return NRP_MARCH_S;
  if (L.sp && m->node_tile_s && L.n + 1 >= m->node_tile_s && L.n + 1 <= m->node_tile_max && m->nl <= 4 && (m->nl == 1 || L.S2row)) return NRP_TILE_S;
  if (L.sp) return NRP_SPLIT;
  if (m->node_march && L.n + 1 >= m->node_march && L.n + 1 >= 64) return NRP_MARCH;
  if (m->tiled_relax && L.n + 1 >= 64) return NRP_TILE;
  return NRP_COLOR;
}
// first level of the group that one workgroup handles in one launch (k_n_mg_coarse: <= 33^2 vertices, at least two levels); nlev: none
static int coarse_first(const msomn *m) {
  if (!m->mg_coarse) return m->nlev;
  int k0 = 0;
  while (k0 < m->nlev && m->lev[k0].n > m->mg_coarse) k0++;
  return m->nlev - k0 >= 2 && m->nlev - k0 <= NMGC_MAXLEV ? k0 : m->nlev;
}
// the correction of a cycle rides in the next residual pass as rows marched by k_n_correct_residual_m<NL> (node_corr_fused 2)
static int node_corr_march(const msomn *m) { return m->node_corr_fused >= 2 && m->nl <= MSOM_FASTNL; }
extern "C" double msomn_get_param(msomn_t *m, const char *k) {
  if (!m || !k) return NAN;
  if (!strcmp(k, "N")) return m->N;
  if (!strcmp(k, "nl")) return m->nl;
  if (!strcmp(k, "L0")) return m->p.L0;
  if (!strcmp(k, "DT")) return m->p.DT;
  if (!strcmp(k, "tend")) return m->p.tend;
  if (!strcmp(k, "dtout")) return m->p.dtout;
  if (!strcmp(k, "nlevels")) return m->nlev;
  if (!strcmp(k, "iRd2_low")) return m->iRd2_low;
  if (!strcmp(k, "bc_fac")) return m->p.bc_fac;
  if (!strcmp(k, "sqg")) return m->sqg;
  if (!strcmp(k, "s2_xuniform")) return m->s2_xuniform;
  if (!strcmp(k, "noise_mode")) return m->noise_mode;
  if (!strcmp(k, "seed")) return m->seed;
  if (!strcmp(k, "noise_draw")) return m->noise_draw;   // number of the next draw of the device generator
  if (!strcmp(k, "wavelet_tiles")) return m->wavelet_tiles;
  if (!strcmp(k, "io_tiles")) return m->io_tiles;
  // tiles: the decomposition, the gather level (levels below live on the tiles), halo exchanges since the last msomn_profile_reset
  if (!strcmp(k, "px")) return m->px;
  if (!strcmp(k, "py")) return m->py;
  if (!strcmp(k, "agg_level")) return m->ntiles > 1 ? (m->const_set ? m->kg : ntile_kg(m->N, m->px, m->py, m->mg_coarse)) : m->nlev;
  if (!strcmp(k, "exchanges")) return (double)m->nexch;
  // running statistics: the mask, 8 nl ny nx bytes per accumulator held (the tile's vertices), samples since msomn_stats_begin
  if (!strcmp(k, "stats_mask")) return m->stats_mask;
  if (!strcmp(k, "stats_bytes")) return (double)__builtin_popcount(m->stats_mask) * m->nl * m->g.ny * m->g.nx * 8;
  if (!strcmp(k, "stats_samples")) return (double)m->stats_samples;
  // Lagrangian floats (include/msomn_floats.h): floats, floats_records, floats_dropped, floats_clamped, floats_lost, floats_on_land,
  // floats_tiles, floats_msg_cap, floats_resident, floats_unsent, floats_migrated
  if (double fv; nfloats_param(m, k, &fv)) return fv;
  if (!strcmp(k, "mg_coarse")) return m->mg_coarse;
  if (!strcmp(k, "node_split")) return m->node_split;
  if (!strcmp(k, "node_pfused")) return m->node_pfused;
  if (!strcmp(k, "node_tile_s")) return m->node_tile_s;
  if (!strcmp(k, "node_march")) return m->node_march;
  if (!strcmp(k, "tiled_relax")) return m->tiled_relax;
  if (!strcmp(k, "node_corr_fused")) return m->node_corr_fused;
  if (!strcmp(k, "node_rhs_fused")) return m->node_rhs_fused;
  if (!strcmp(k, "node_march_s")) return m->node_march_s;   // split levels of >= this many vertices a side take k_n_relax_march_s
  if (!strcmp(k, "node_march_rows")) return m->node_march_rows;
  if (!strncmp(k, "split_", 6)) { int l = atoi(k + 6); return l >= 0 && l < m->nlev ? m->lev[l].sp : NAN; }
  // the paths the solve takes (set_const decides the layouts and row tables): the K cap of the chained split pass (level 0's row
  // tables), the path of level k's sweeps (NRP_*), the correction marched inside the residual pass
  if (!strcmp(k, "node_march_kmax")) return m->nlev ? node_march_kmax(m, m->lev[0]) : NAN;
  if (!strncmp(k, "relax_path_", 11)) { int l = atoi(k + 11); return l >= 0 && l < m->nlev ? (l >= coarse_first(m) ? NRP_COARSE : sweep_path(m, l)) : NAN; }
  if (!strcmp(k, "corr_march")) return node_corr_march(m);
  if (!strncmp(k, "idh0_", 5)) { int l = atoi(k + 5); return l >= 0 && l < MSOM_MAXNL ? m->lc.idh0[l] : NAN; }
  if (!strncmp(k, "idh1_", 5)) { int l = atoi(k + 5); return l >= 0 && l < MSOM_MAXNL ? m->lc.idh1[l] : NAN; }
  return NAN;
}
#define NEED_FIELD(m, f) if (!(m) || (f) < 0 || (f) >= MSOMN_NFIELDS) { msom_set_error("bad field id %d", (int)(f)); return MSOM_ERR_ARG; }
#define NEED_NCONST(m) if (!(m)) return MSOM_ERR_ARG; if (!(m)->const_set) { msom_set_error("call msomn_set_const first"); return MSOM_ERR_STATE; }

extern "C" int msomn_field_layers(msomn_t *m, int f) { NEED_FIELD(m, f); return m->fl[f]; }
extern "C" int msomn_set_field(msomn_t *m, int f, const double *a) {
  NEED_FIELD(m, f);
  if (!a) return MSOM_ERR_ARG;
  if (f == MSOMN_QFORC3D) m->forcing_3d = 1;
  if (f == MSOMN_PSIPG) m->pg_set = 1;
  if (f == MSOMN_TOPO) m->topo_set = 1;
  int r = upload_g(m, m->f[f], m->g, m->fl[f], a);
  // tiles: every stencil that reads the field across a tile edge finds its halo (collective)
  return r ? r : nt_exchange(m, m->f[f], m->g, 0, m->fl[f]);
}
extern "C" int msomn_get_field(msomn_t *m, int f, double *a) {
  NEED_FIELD(m, f);
  if (!a) return MSOM_ERR_ARG;
  return download_g(m, m->f[f], m->g, m->fl[f], a);
}

// ---- boundary conditions with set_bc_ms() in force (qg-node/qg.h:197-214, qg_baroclinic_ms.h:55-70)
static double bcc(const msomn *m) { return 2 * m->p.bc_fac / (m->D * m->D); }
static void bnd_psi(msomn *m) { launch_n_bnd_const(m->st, m->f[MSOMN_PSI], m->g, m->nl, m->psi_bc, 0, m->walls); }
static void bnd_q(msomn *m, double *q) { launch_n_bnd_from(m->st, q, m->f[MSOMN_PSI], m->g, m->nl, bcc(m), 0, m->psi_bc, m->walls); }
// sqg_baroclinic_ms.h:64-67: the tmp rule subtracts psi_bc instead of the boundary value of zeta
static void bnd_tmp(msomn *m) { launch_n_bnd_from(m->st, m->f[MSOMN_TMP], m->f[MSOMN_ZETA], m->g, m->nl, bcc(m), m->sqg ? 0 : 1, m->sqg ? m->psi_bc : 0., m->walls); }


// comp_q_baroclinic / comp_q_barotropic
static int comp_q(msomn *m, const double *psi, double *q) {
  int rx = nt_exchange(m, const_cast<double *>(psi), m->g, 0, m->nl);   // the laplacian reads psi across the tile edges
  if (rx) return rx;
  if (m->nl == 1) launch_n_helm(m->st, psi, q, m->g, m->D, m->iRd2_low);
  else {
    launch_n_del2(m->st, psi, q, m->g, m->nl, 0., 1., m->D);
    // sqg: the reference's comp_q_baroclinic (:232-243) still calls the 4-argument comp_stretch; completed with bs
    if (m->sqg) launch_n_stretch_sqg(m->st, psi, m->f[MSOMN_BS], m->f[MSOMN_S2S], q, m->f[MSOMN_S2], m->g, m->nl, 1., 1., m->lc);
    else launch_n_stretch(m->st, psi, q, m->f[MSOMN_S2], m->g, m->nl, 1., 1., m->lc);
  }
  bnd_q(m, q);
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

// second psi buffer of the out-of-place passes (k_n_rhs_pre, k_n_correct_residual): the pad cells around the grid are written by
// no kernel and no upload, they are zero in both
static int need_psi_alt(msomn *m) {
  if (m->psi_alt) return MSOM_OK;
  HIPCHK(hipMalloc((void **)&m->psi_alt, m->g.ls * m->nl * sizeof(double)));
  HIPCHK(hipMemsetAsync(m->psi_alt, 0, m->g.ls * m->nl * sizeof(double), m->st));   // in the stream of the kernels that follow
  return MSOM_OK;
}
// rhs_pv_baroclinic qg_baroclinic_ms.h:104-196 / rhs_pv_barotropic qg_barotropic.h:16-29
static int rhs_pv_body(msomn *m, double *q, double *dq);
static int rhs_pv(msomn *m, double *q, double *dq) {
  Timed t(m, NP_RHS);
  return rhs_pv_body(m, q, dq);
}
static int rhs_pv_body(msomn *m, double *q, double *dq) {
  const NodeParams &p = m->p;
  const int nl = m->nl;
  const double drag = p.hEkb * p.f0 / (2 * p.dh[nl - 1]);
  int rx;
  if (nl == 1) {
    if ((rx = nt_exchange(m, m->f[MSOMN_PSI], m->g, 0, 1)) || (rx = nt_exchange(m, q, m->g, 0, 1))) return rx;   // the Jacobian reads both
    launch_n_rhs_barotropic(m->st, m->f[MSOMN_PSI], q, m->f[MSOMN_QFORC], dq, m->g, m->D, p.beta, drag, p.nu);
    HIPCHK(hipGetLastError());
    return MSOM_OK;
  }
  double *psi = m->f[MSOMN_PSI], *zeta = m->f[MSOMN_ZETA], *tmp = m->f[MSOMN_TMP], *S2 = m->f[MSOMN_S2];
  if (m->node_rhs_fused) {   // the same arithmetic in three passes (four with the surface term of the SQG variant), kernels_node.hip
    int ra = need_psi_alt(m);
    if (ra) return ra;
    launch_n_rhs_pre(m->st, q, psi, m->psi_alt, zeta, m->f[MSOMN_MASK], m->g, nl, m->D, bcc(m), m->psi_bc);
    std::swap(m->f[MSOMN_PSI], m->psi_alt);
    psi = m->f[MSOMN_PSI];
    launch_n_del2_bnd(m->st, zeta, tmp, m->g, nl, m->D, bcc(m), m->sqg ? 0 : 1, m->sqg ? m->psi_bc : 0.);
    if (m->sqg) launch_n_lap_bs(m->st, m->f[MSOMN_BS], m->d2bs, m->g, m->D, m->walls);
    launch_n_rhs_all(m->st, psi, zeta, tmp, m->f[MSOMN_PSIPG], S2, m->f[MSOMN_TOPO], m->f[MSOMN_QFORC], m->forcing_3d ? m->f[MSOMN_QFORC3D] : nullptr,
                     m->f[MSOMN_MASK], m->sqg ? m->d2bs : nullptr, m->f[MSOMN_S2S], dq, m->g, nl, m->D, p.beta, drag, p.f0, p.dh[nl - 1], p.nu, -p.nu4, m->lc, m->pg_set, m->topo_set);
    HIPCHK(hipGetLastError());
    return MSOM_OK;
  }
  // tiles run this chain (node_rhs_fused resolves to off): psi, zeta and tmp get their halos before the stencils that read them
  launch_n_mul_mask(m->st, q, psi, m->f[MSOMN_MASK], m->g, nl);                 // :110-116
  if ((rx = nt_exchange(m, psi, m->g, 0, nl))) return rx;
  launch_n_del2(m->st, psi, zeta, m->g, nl, 0., 1., m->D);                      // comp_del2(psi, zeta, 0, 1)
  bnd_q(m, zeta);
  if ((rx = nt_exchange(m, zeta, m->g, 0, nl))) return rx;
  launch_n_rhs_main(m->st, psi, zeta, m->f[MSOMN_PSIPG], S2, m->f[MSOMN_TOPO], dq, m->g, nl, 1, 1, m->D, p.beta, drag, p.f0, p.dh[nl - 1], m->lc);
  if (m->sqg) {                                                                 // sqg_baroclinic_ms.h:160-174: del2_bs = laplacian(bs)
    launch_n_lap_bs(m->st, m->f[MSOMN_BS], m->d2bs, m->g, m->D, m->walls);
    launch_n_stretch_sqg(m->st, zeta, m->d2bs, m->f[MSOMN_S2S], dq, S2, m->g, nl, 1., p.nu, m->lc);
  } else launch_n_stretch(m->st, zeta, dq, S2, m->g, nl, 1., p.nu, m->lc);      // :160
  launch_n_del2(m->st, zeta, tmp, m->g, nl, 0., 1.0, m->D);                     // :162 + boundary(tmp)
  bnd_tmp(m);
  if ((rx = nt_exchange(m, tmp, m->g, 0, nl))) return rx;
  launch_n_axpy(m->st, dq, tmp, m->g, nl, p.nu);                               // :164-167
  const double minus_nu4 = -p.nu4;
  if (m->sqg) launch_n_stretch_sqg(m->st, tmp, m->d2bs, m->f[MSOMN_S2S], dq, S2, m->g, nl, 1., minus_nu4, m->lc);   // del4_bs is laplacian(bs) again, :187-201
  else launch_n_stretch(m->st, tmp, dq, S2, m->g, nl, 1., minus_nu4, m->lc);   // :172
  launch_n_del2(m->st, tmp, dq, m->g, nl, 1., minus_nu4, m->D);                 // :173
  launch_n_add2d(m->st, dq, m->f[MSOMN_QFORC], m->g);                           // :176-180 surface forcing
  if (m->forcing_3d) launch_n_axpy(m->st, dq, m->f[MSOMN_QFORC3D], m->g, nl, 1.);   // :179-185 (FORCING_3D)
  launch_n_mul_mask(m->st, dq, nullptr, m->f[MSOMN_MASK], m->g, nl);            // :186-190
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

// ---- nodal multigrid
// one colour half-sweep of level k on L.da, in the level's layout.  timed = false: the left-over half-sweep of a chained path
static void colour_pass(msomn *m, int k, int c, bool timed = true) {
  NLevel &L = m->lev[k];
  {
    Timed t(m, NP_RELAX, timed && k == 0);
    if (L.sp) launch_n_relax(m->st, L.da, L.res, L.mask_s, L.S2_s, L.ga, m->nl, c, L.D, m->iRd2_low, m->lc, 1, L.S2row, L.walls);
    else launch_n_relax(m->st, L.da, L.res, L.mask, L.S2, L.g, m->nl, c, L.D, m->iRd2_low, m->lc, 0, L.S2row, L.walls);
  }
  // a tiled level: the other colour of the neighbours reads this one across the edge (an error stays in msom_last_error and
  // stops the solve at its next reduction)
  if (L.tiled && nt_exchange(m, L.da, L.ga, L.sp, m->nl)) m->tile_err = 1;
}
// nh colour half-sweeps of L, the first of colour c, as out-of-place passes of up to kmax: pass(c, K, left) goes from L.da to L.da2,
// which then change places (L.da always the current one); `left` half-sweeps follow it.  A single left-over half-sweep runs in
// place as the colour pass single(c); no_tail: a pass gives one half-sweep away so that none is left over
template <class Pass, class Single>
static void chained_passes(NLevel &L, int nh, int c, int kmax, bool no_tail, Pass pass, Single single) {
  while (nh >= 2) {
    int K = nh < kmax ? nh : kmax;
    if (no_tail && nh - K == 1 && K > 2) K--;
    pass(c, K, nh - K);
    std::swap(L.da, L.da2);
    nh -= K; c = (c + K) & 1;
  }
  if (nh == 1) single(c);
}
// nsweeps red-black sweeps of level k on L.da, by the path sweep_path names.
// prolong = 1: the correction of level k + 1 has not been prolongated yet; the first colour pass does it on the fly (split levels)
static void relax_sweeps(msomn *m, int k, int nsweeps, int prolong = 0) {
  NLevel &L = m->lev[k];
  int path = sweep_path(m, k);
  if (path == NRP_TILE_S && nsweeps < 2) path = NRP_SPLIT;
  int nh = 2 * nsweeps, c = 0;
  if (prolong && nsweeps >= 1) {
    const NLevel &C = m->lev[k + 1];
    Timed t(m, NP_RELAX_PROLONG, k == 0);
    launch_n_relax_prolong(m->st, L.da, L.res, L.mask_s, L.S2_s, L.ga, m->nl, L.D, m->iRd2_low, m->lc, L.S2row, C.da, C.ga, C.sp);
    nh--; c = 1;
  }
  const auto single = [&](int c1) { colour_pass(m, k, c1, false); };
  switch (path) {
  case NRP_MARCH_S:
    // chained colour half-sweeps (round 3) in passes of up to node_march_kmax; node_march_tail1 = 1 lets a single half-sweep stay
    // behind (9 as 4 + 4 + 1, not 4 + 3 + 2).  A pass stores only the colour of its last half-sweep if ANOTHER PASS follows (which
    // recomputes the other colour before anything reads it); a single colour pass that follows updates interior vertices only, so
    // the pass before it stores both colours
    chained_passes(L, nh, c, node_march_kmax(m, L), !m->node_march_tail1, [&](int c1, int K, int left) {
      Timed t(m, NP_MARCH, k == 0);
      launch_n_relax_march_s(m->st, L.da, L.da2, L.res, L.mask_s, L.ga, m->nl, c1, K, L.D, m->iRd2_low, m->lc, L.S2row, left >= 2, m->node_march_rows);
    }, single);
    return;
  case NRP_TILE_S:
    // launch-bound split levels (round 3): LDS-tiled passes (k_n_relax_tile_s) of up to node_tile_k half-sweeps; a left-over single
    // half-sweep is cheaper as a colour pass than as a tile pass
    chained_passes(L, nh, c, m->node_tile_k, false, [&](int c1, int K, int) {
      Timed t(m, NP_RELAX, k == 0);
      launch_n_relax_tile_s(m->st, L.da, L.da2, L.res, L.mask_s, L.ga, m->nl, c1, K, L.D, m->iRd2_low, m->lc, L.S2row);
    }, single);
    return;
  case NRP_MARCH:   // natural layout, passes of up to 4, never a single half-sweep left behind
    chained_passes(L, nh, c, 4, true, [&](int c1, int K, int) {
      launch_n_relax_march(m->st, L.da, L.da2, L.res, L.mask, L.S2, L.g, m->nl, c1, K, L.D, m->iRd2_low, m->lc, m->node_march_rows);
    }, [&](int c1) { launch_n_relax(m->st, L.da, L.res, L.mask, L.S2, L.g, m->nl, c1, L.D, m->iRd2_low, m->lc); });
    return;
  case NRP_TILE:    // natural layout, LDS-tiled passes of 2 (or 1) whole sweeps
    for (int s = 0; s < nsweeps;) {
      s += launch_n_relax_tile(m->st, L.da, L.da2, L.res, L.mask, L.S2, L.g, m->nl, nsweeps - s >= 2 ? 2 : 1, L.D, m->iRd2_low, m->lc);
      std::swap(L.da, L.da2);
    }
    return;
  default:          // NRP_COLOR, NRP_SPLIT: one launch per colour (the split layout already moves only the bytes a colour uses)
    for (; nh > 0; nh--, c ^= 1) colour_pass(m, k, c);
  }
}
// layout of the correction / residual of every level (option node_split; da and res hold nothing between cycles, so the choice
// may change at any time); the levels one workgroup handles (mg_coarse) stay natural
static int choose_layouts(msomn *m) {
  for (int k = 0; k < m->nlev; k++) {   // row tables of an x-independent S2 (levels: injection keeps it x-independent)
    NLevel &L = m->lev[k];
    L.S2row = nullptr;
    if (m->nl > 1 && m->s2_xuniform && m->s2_rows) {
      int r;
      if (!L.S2row_buf && (r = dalloc(&L.S2row_buf, (size_t)m->nlm * L.g.ny))) return r;
      launch_n_row_table(m->st, L.S2, L.g, m->nlm, L.S2row_buf);
      L.S2row = L.S2row_buf;
    }
  }
  for (int k = 0; k < m->nlev; k++) {
    NLevel &L = m->lev[k];
    L.sp = m->node_split > 0 && L.n + 1 >= m->node_split && L.n >= 64 && L.n > m->mg_coarse;
    // (a tiled level compares the GLOBAL side with node_split, so a tiled handle takes the layouts of the single tile)
    const int was = L.ga.pitch;
    L.ga = L.sp ? node_geom_split_rect(L.g.nx - 1, L.g.ny - 1) : L.g;
    if (L.tiled && was != L.ga.pitch) {   // the halo slots of the new layout hold whatever the old one kept there
      const size_t bytes = std::max(L.g.ls, node_geom_split_rect(L.g.nx - 1, L.g.ny - 1).ls) * m->nl * sizeof(double);
      for (double *q : {L.da, L.da2, L.res}) HIPCHK(hipMemsetAsync(q, 0, bytes, m->st));
    }
    if (!L.sp) continue;
    int r;
    if (!L.mask_s && ((r = dalloc(&L.mask_s, L.ga.ls)) || (m->nl > 1 && (r = dalloc(&L.S2_s, L.ga.ls * m->nlm))))) return r;
    launch_n_relayout(m->st, L.mask, L.g, 0, L.mask_s, L.ga, 1, 1);
    if (m->nl > 1) launch_n_relayout(m->st, L.S2, L.g, 0, L.S2_s, L.ga, 1, m->nlm);
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
// mask and S2 of every level from those of level 0.  Tiles: levels below the gather level kg hold the tile's window, kg and up the
// global grid (the same values on every rank, the ones the single tile holds): the level-kg mask and S2 are restricted on the tiles,
// gathered once, and the coarser ones built from them as the single tile builds all of its levels (kg = 0, allocated by node_alloc)
static int build_levels(msomn *m) {
  int r;
  m->kg = m->ntiles > 1 ? ntile_kg(m->N, m->px, m->py, m->mg_coarse) : 0;
  if (m->ntiles > 1) {   // which levels live on the tile depends on the option mg_coarse: allocated here
    for (int k = 0; k < m->nlev; k++) free_level(m->lev[k], k);
    nt_free_gather(m);
    for (int k = 0; k <= m->nlev; k++) {   // k == nlev: the piece, the tile's window of level kg
      const bool piece = k == m->nlev;
      if (!piece && k >= m->kg) { if ((r = alloc_level(m, m->lev[k], k, node_geom(m->N >> k)))) return r; m->lev[k].tiled = 0; m->lev[k].walls = WALL_ALL; continue; }
      const NodeTile t = ntile_level(m->N, m->px, m->py, m->rank, piece ? m->kg : k);
      NLevel &L = piece ? m->piece : m->lev[k];
      if ((r = alloc_level(m, L, piece ? m->kg : k, node_geom_rect(t.tx, t.ty)))) return r;
      L.tiled = 1; L.walls = m->walls;
    }
    m->gcount = (size_t)(m->nl > m->nlm ? m->nl : m->nlm) * m->piece.g.nx * m->piece.g.ny;
    HIPCHK(hipMalloc((void **)&m->gsend, m->gcount * sizeof(double)));
    HIPCHK(hipMalloc((void **)&m->grecv, m->gcount * m->ntiles * sizeof(double)));
  }
  launch_n_bnd_const(m->st, m->f[MSOMN_MASK], m->g, 1, 0., 0, m->walls);
  // the static fields the tendency reads across the tile edges (the inputs were transformed in place since msomn_set_field)
  for (int f : {MSOMN_MASK, MSOMN_S2, MSOMN_TOPO, MSOMN_PSIPG})
    if ((r = nt_exchange(m, m->f[f], m->g, 0, m->fl[f]))) return r;
  for (int k = 1; k <= m->kg; k++) {   // the tiled levels (one tile: none)
    NLevel &F = m->lev[k - 1], &C = k < m->kg ? m->lev[k] : m->piece;
    launch_n_restrict(m->st, F.mask, F.g, C.mask, C.g, 1, 1);   // the 9-point full weighting reads the halo with its corners
    launch_n_bnd_const(m->st, C.mask, C.g, 1, 0., 0, m->walls);
    if ((r = nt_exchange(m, C.mask, C.g, 0, 1))) return r;
    if (m->nl > 1) {
      launch_n_restrict(m->st, F.S2, F.g, C.S2, C.g, m->nlm, 2);
      if ((r = nt_exchange(m, C.S2, C.g, 0, m->nlm))) return r;
    }
  }
  NLevel &G = m->lev[m->kg];
  if (m->ntiles > 1 && (r = nt_gather(m, m->piece.mask, m->piece.g, 1, G.mask, G.g))) return r;
  if (m->ntiles > 1 && m->nl > 1 && (r = nt_gather(m, m->piece.S2, m->piece.g, m->nlm, G.S2, G.g))) return r;
  for (int k = m->kg + 1; k < m->nlev; k++) {   // the levels that live whole on this rank
    launch_n_restrict(m->st, m->lev[k - 1].mask, m->lev[k - 1].g, m->lev[k].mask, m->lev[k].g, 1, 1);
    launch_n_bnd_const(m->st, m->lev[k].mask, m->lev[k].g, 1, 0.);
    if (m->nl > 1) launch_n_restrict(m->st, m->lev[k - 1].S2, m->lev[k - 1].g, m->lev[k].S2, m->lev[k].g, m->nlm, 2);
  }
  return choose_layouts(m);
}
// host array <-> a level's da / res in whatever layout the level uses (parity tests); da2 is the natural staging buffer
static int upload_lev(msomn *m, NLevel &L, double *dst, const double *a) {
  if (!L.sp) return upload_g(m, dst, L.g, m->nl, a);
  int r = upload_g(m, L.da2, L.g, m->nl, a);
  if (r) return r;
  launch_n_relayout(m->st, L.da2, L.g, 0, dst, L.ga, 1, m->nl);
  return MSOM_OK;
}
static int download_lev(msomn *m, NLevel &L, const double *src, double *a) {
  if (!L.sp) return download_g(m, src, L.g, m->nl, a);
  launch_n_relayout(m->st, src, L.ga, 1, L.da2, L.g, 0, m->nl);
  return download_g(m, L.da2, L.g, m->nl, a);
}
// the passes over level 0 with the model's field a: each carries the layout of res / da, the row tables and the tile's walls
static void residual_pass(msomn *m, const double *a, const double *b, int zb) {
  NLevel &L = m->lev[0];
  launch_n_residual(m->st, a, b, L.mask, L.S2, L.res, m->d_scal + NSC_RES, m->g, m->nl, m->D, m->iRd2_low, m->lc, L.sp ? &L.ga : nullptr, L.S2row, zb, m->walls);
}
static void correct_pass(msomn *m, double *a) {
  NLevel &L = m->lev[0];
  Timed t(m, NP_CORRECT);
  launch_n_correct(m->st, a, L.da, m->g, m->nl, m->psi_bc, L.sp ? &L.ga : nullptr, m->walls);
}
// The levels k0 .. nlev - 1 of a cycle, which live whole on this rank (one tile: k0 = 0; tiles: k0 = kg, the gathered global grid, the
// same on every rank): lev[k0].res -> lev[k0].da.  Down to the one-launch group where coarse_first qualifies (it starts at k0 at the
// earliest), level by level otherwise; every level in its own layout.  whole_restrict is the way down on its own: the single tile
// queues it before it knows whether the cycle runs
static void whole_restrict(msomn *m, int k0) {
  const int kc = std::max(coarse_first(m), k0);
  for (int k = k0 + 1; k < m->nlev && k <= kc; k++) {
    NLevel &F = m->lev[k - 1], &C = m->lev[k];
    launch_n_restrict(m->st, F.res, F.ga, C.res, C.ga, m->nl, 0, F.sp, C.sp, 1);
  }
}
static void coarse_group(msomn *m, int kc, int nrelax) {
  NCoarseArgs ca;
  ca.n = m->nlev - kc; ca.iRd2 = m->iRd2_low; ca.lc = m->lc;
  for (int k = kc; k < m->nlev; k++) {
    NLevel &L = m->lev[k];
    ca.lev[k - kc] = NCoarseLev{L.da, L.res, L.mask, L.S2, L.g, L.D * L.D};
  }
  Timed t(m, NP_COARSE);
  launch_n_mg_coarse(m->st, ca, nrelax, m->nl);
}
static int whole_solve(msomn *m, int k0, int nrelax, bool restricted) {
  const int nl = m->nl, nlev = m->nlev, kc = std::max(coarse_first(m), k0);
  if (!restricted) whole_restrict(m, k0);
  if (kc < nlev) coarse_group(m, kc, nrelax);
  else HIPCHK(hipMemsetAsync(m->lev[nlev - 1].da, 0, m->lev[nlev - 1].g.ls * nl * sizeof(double), m->st));
  // prolongation into level kf: a launch, or (split levels, option node_pfused) left to the first colour pass of that level
  auto prolong_into = [&](int kf) -> int {
    NLevel &C = m->lev[kf + 1], &F = m->lev[kf];
    if (F.sp && m->node_pfused && nrelax >= 1) return 1;
    launch_n_prolong(m->st, C.da, C.ga, F.da, F.ga, nl, C.sp, F.sp);
    return 0;
  };
  int pending = (kc < nlev && kc > k0) ? prolong_into(kc - 1) : 0;
  for (int k = (kc < nlev ? kc : nlev) - 1; k >= k0; k--) {
    relax_sweeps(m, k, nrelax, pending);
    pending = k > k0 ? prolong_into(k - 1) : 0;
  }
  return MSOM_OK;
}
// vpoisson, nodal-poisson.h:19-143: residual first, then (unless converged) one cycle; the correction a += da of a cycle waits for
// the next residual pass, or for the end of the loop.  On tiles (kg > 0) every rank takes the same decision from the all-reduced
// max |res|; the residual then goes down the tiled levels (halo, restriction), the level-kg pieces are gathered, every rank solves
// the gathered levels, takes its window of the level-kg correction and goes up the tiled levels (prolongation, halo, colour passes
// with a halo each).  One tile: kg = 0, no tiled levels, no gather, the exchanges are no-ops.
static int vpoisson(msomn *m, double *&a, const double *b) {
  msom_mgstats mg;
  mg.sum = HUGE_VAL; mg.resa = HUGE_VAL; mg.resb = 0; mg.nrelax = m->nrelax;
  const int nl = m->nl, kg = m->kg;
  const bool tiles = m->ntiles > 1;
  NLevel &L0 = m->lev[0], &P = m->piece, &G = m->lev[kg];
  const NodeTile tg = ntile_level(m->N, m->px, m->py, m->rank, kg);
  bool pending_correct = false;
  int r;
  m->tile_err = 0;
  for (mg.i = 0; mg.i < m->nitermax; mg.i++) {
    HIPCHK(hipMemsetAsync(m->d_scal + NSC_RES, 0, sizeof(double), m->st));
    // the correction of the previous cycle rides in this residual pass (option node_corr_fused, off on tiles; a second psi buffer)
    if (pending_correct && m->node_corr_fused) {
      if ((r = need_psi_alt(m))) return r;
      Timed t(m, NP_CORR_RES);
      launch_n_correct_residual(m->st, a, m->psi_alt, L0.da, L0.sp ? &L0.ga : nullptr, m->psi_bc, b, L0.mask, L0.S2, L0.res, m->d_scal + NSC_RES, m->g, nl, m->D,
                                m->iRd2_low, m->lc, L0.sp ? &L0.ga : nullptr, L0.S2row, node_corr_march(m));
      std::swap(a, m->psi_alt);
    } else {
      if (pending_correct) correct_pass(m, a);
      if ((r = nt_exchange(m, a, m->g, 0, nl))) return r;
      Timed t(m, NP_RESIDUAL);
      residual_pass(m, a, b, 1);
    }
    pending_correct = false;
    if (tiles) {   // reduce, decide, and only then post the exchanges of the cycle
      if ((r = nt_reduce(m, NSC_RES, 1, RED_MAX))) return r;
    } else {
      // max |res| travels to the host; the restrictions of the cycle that follows unless the solve ends here are queued behind the copy
      // (round 3): the GPU works through them while the host waits for the number and decides -- they write nothing but the coarse levels'
      // residuals, which nobody reads if the solve is over.  (boundary_level of the residual: the pass above stored 0 on the boundary
      // vertices, zb = 1; the boundary vertices of every coarser level end up 0 as well)
      HIPCHK(hipMemcpyAsync(m->h_scal + NSC_RES, m->d_scal + NSC_RES, sizeof(double), hipMemcpyDeviceToHost, m->st));
      if (!m->ev_res) HIPCHK(hipEventCreateWithFlags(&m->ev_res, hipEventDisableTiming));
      HIPCHK(hipEventRecord(m->ev_res, m->st));
      whole_restrict(m, 0);
      HIPCHK(hipEventSynchronize(m->ev_res));
    }
    const double max = m->h_scal[NSC_RES];
    mg.resa = max;
    if (mg.i == 0) mg.resb = max;
    if (max < m->tolerance && mg.i >= m->nitermin) break;
    for (int k = 1; k <= kg; k++) {
      NLevel &F = m->lev[k - 1], &C = k < kg ? m->lev[k] : P;
      if ((r = nt_exchange(m, F.res, F.ga, F.sp, nl))) return r;
      launch_n_restrict(m->st, F.res, F.ga, C.res, C.ga, nl, 0, F.sp, C.sp, 1, m->walls);
    }
    if (tiles && (r = nt_gather(m, P.res, P.g, nl, G.res, G.g))) return r;
    if ((r = whole_solve(m, kg, mg.nrelax, !tiles))) return r;
    if (tiles) launch_n_extract(m->st, G.da, G.g, P.da, P.g, nl, tg.ox, tg.oy);
    for (int k = kg - 1; k >= 0; k--) {
      NLevel &C = k + 1 < kg ? m->lev[k + 1] : P, &L = m->lev[k];
      launch_n_prolong(m->st, C.da, C.ga, L.da, L.ga, nl, C.sp, L.sp, m->walls);
      if ((r = nt_exchange(m, L.da, L.ga, L.sp, nl))) return r;
      relax_sweeps(m, k, mg.nrelax);
      if (m->tile_err) return MSOM_ERR_COMM;
    }
    pending_correct = true;
  }
  if (pending_correct) correct_pass(m, a);
  HIPCHK(hipGetLastError());
  if (mg.resa > m->tolerance && !m->quiet)
    fprintf(stderr, "Convergence for psi not reached.\nmg.i = %d, mg.resb: %g mg.resa: %g\n", mg.i, mg.resb, mg.resa);
  m->mg = mg;
  return MSOM_OK;
}
static int invert_q(msomn *m, double *q) {
  const double *b = q;
  if (m->sqg) {  // the known surface term of the top layer moves to the right-hand side (completion, see include/msom.h)
    launch_n_sqg_rhs(m->st, q, m->f[MSOMN_S2S], m->f[MSOMN_BS], m->qeff, m->g, m->nl, m->lc.idh0[0]);
    b = m->qeff;
  }
  int r = vpoisson(m, m->f[MSOMN_PSI], b);
  if (r) return r;
  bnd_psi(m);
  bnd_q(m, q);
  return MSOM_OK;
}
// adjust_dt qg-node/qg.h:258-284 with the `previous` memory of Basilisk's timestep()
static int adjust_dt(msomn *m, double dtmax, double *out) {
  HIPCHK(hipMemsetAsync(m->d_scal + NSC_UMAX, 0, sizeof(double), m->st));
  launch_n_umax(m->st, m->f[MSOMN_PSI], m->d_scal + NSC_UMAX, m->g, m->nl, m->D);
  // (tiles: a face on a shared edge is seen by both tiles, the maximum does not mind)
  int r = nt_reduce(m, NSC_UMAX, 1, RED_MAX);
  if (r) return r;
  *out = step_limit(m->h_scal[NSC_UMAX], dtmax, m->D, m->p.CFL, &m->previous);
  return MSOM_OK;
}

// ---- stochastic forcing: qg-node/qg_stochastic.h (init_stoch :15-47, generate_noise :49-65), advance qg-node/qg.h:306-320
NatGeom cell_geom(int n) {
  NatGeom g;
  g.nx = g.ny = n;
  g.pitch = ((n + 15) / 16) * 16 + 2 * MSOM_XP;
  g.rows = n + 2 * MSOM_YP;
  g.ls = (size_t)g.pitch * g.rows;
  return g;
}
static int stoch_setup(msomn *m) {  // pyramids of the cell scalar + wavelet coefficients of the uniform filter length L_filt
  const NodeParams &p = m->p;
  int r;
  if (m->ntiles > 1) return ct_stoch_setup(m);   // windows below the gather level of this msomn_set_const, global levels from it on
  if (m->cnlev == 0) {
    int c = 1;
    while ((m->N >> c) >= 1) c++;
    m->cnlev = c;
    m->cg.resize(c); m->cs.assign(c, nullptr); m->cr.assign(c, nullptr); m->csig.assign(c, nullptr);
    for (int k = 0; k < c; k++) {
      m->cg[k] = cell_geom(m->N >> k);
      if ((r = dalloc(&m->cs[k], m->cg[k].ls)) || (r = dalloc(&m->cr[k], m->cg[k].ls)) || (r = dalloc(&m->csig[k], m->cg[k].ls))) return r;
    }
  }
  const int K = m->cnlev;
  std::vector<std::vector<double>> sl(K);
  for (int k = 0; k < K; k++) {  // low pass from the finest level down
    const int n = m->N >> k, fx = 2 * n;
    const double Delta = p.L0 / n;
    sl[k].resize((size_t)n * n);
    for (int j = 0; j < n; j++)
      for (int i = 0; i < n; i++) {
        double ref_flag = 0;
        if (k > 0) {
          ref_flag += sl[k - 1][(size_t)(2 * j) * fx + 2 * i]; ref_flag += sl[k - 1][(size_t)(2 * j + 1) * fx + 2 * i];
          ref_flag += sl[k - 1][(size_t)(2 * j) * fx + 2 * i + 1]; ref_flag += sl[k - 1][(size_t)(2 * j + 1) * fx + 2 * i + 1];
        }
        double v;
        if (ref_flag > 0) v = 1;
        else if (p.L_filt > 2 * Delta) v = 0;
        else if (p.L_filt <= 2 * Delta && p.L_filt > Delta) v = 1 - (p.L_filt - Delta) / Delta;
        else v = 1;
        sl[k][(size_t)j * n + i] = v;
      }
  }
  for (int k = 0; k < K; k++) {  // high pass, then to the device
    for (double &v : sl[k]) v = 1 - v;
    const NatGeom &g = m->cg[k];
    HIPCHK(hipMemcpy2DAsync(m->csig[k] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), sl[k].data(), g.nx * sizeof(double), g.nx * sizeof(double), g.ny,
                            hipMemcpyHostToDevice, m->st));
  }
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
static void cell_bc(msomn *m, double *f, const NatGeom &g) { launch_fill_ghost(m->st, f, g, 1, BC_NEUMANN, WALL_ALL); }
// the calls of the wavelet pyramid on a tiled handle: refused unless the option wavelet_tiles is on (then they are collective)
static int wv_refuse(const msomn *m, const char *call) { return m && m->wavelet_tiles ? MSOM_OK : nt_refuse(m, call); }
// noise_mode 0 is the serial rand() stream of the host: one state per process, while the in-process tiles are threads of one process,
// so the tiles could not draw the single tile's numbers.  Asked before anything is posted
static int noise_mode_refuse(const msomn *m, const char *call) {
  if (m->ntiles == 1 || m->noise_mode == 1) return MSOM_OK;
  msom_set_error("%s: noise_mode = 0 is not available on a tiled vertex-grid handle (%d x %d tiles): the host's rand() stream is one state per process "
                 "and cannot be shared by tiles; set noise_mode = 1 (device generator)", call, m->px, m->py);
  return MSOM_ERR_CONFIG;
}
void node_noise_ghosts(msomn *m) { cell_bc(m, m->cs[0], m->cg[0]); }
// wavelet -> scale by sig_lev -> inverse wavelet of the cell field cs[0] (kernels_wavelet.hip, one layer, default BC)
// ghosts_set: the ghost ring of cs[0] is already what cell_bc would write (k_n_noise)
static int cell_wavelet_filter(msomn *m, int ghosts_set = 0) {
  if (m->ntiles > 1) return ct_noise_filter(m, ghosts_set);
  const int K = m->cnlev;
  if (!ghosts_set) cell_bc(m, m->cs[0], m->cg[0]);
  for (int k = 1; k < K; k++) {
    launch_wv_restrict(m->st, m->cs[k - 1], m->cg[k - 1], m->cs[k], m->cg[k], 1);
    cell_bc(m, m->cs[k], m->cg[k]);
  }
  if (K == 1) launch_wv_root(m->st, m->cs[0], m->csig[0], m->cs[0], m->cg[0], 1);
  else {
    launch_wv_root(m->st, m->cs[K - 1], m->csig[K - 1], m->cr[K - 1], m->cg[K - 1], 1);
    cell_bc(m, m->cr[K - 1], m->cg[K - 1]);
  }
  for (int k = K - 2; k >= 0; k--) {
    double *out = k == 0 ? m->cs[0] : m->cr[k];
    launch_wv_recon(m->st, m->cs[k], m->cs[k + 1], m->cr[k + 1], m->csig[k], out, m->cg[k], m->cg[k + 1], 1);
    cell_bc(m, out, m->cg[k]);
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
static int upload_cells(msomn *m, const double *a) {
  const NatGeom &g = m->cg[0];
  HIPCHK(hipMemcpy2DAsync(m->cs[0] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), a, g.nx * sizeof(double), g.nx * sizeof(double), g.ny, hipMemcpyDefault, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  if (m->ntiles > 1) return ct_ring(m, m->cs[0], g, 1, BC_NEUMANN);   // k_n_add_noise reads the ring
  cell_bc(m, m->cs[0], g);
  return MSOM_OK;
}
// noise_mode 0, reference-exact noise: Box-Muller on the serial rand() stream in foreach order (x outer, y inner),
// qg_stochastic.h:13,51-53.  noise_mode 1: the handle's next draw of the device generator with its ghost ring, then the filter,
// all queued on the handle's stream (no host buffer, no synchronisation)
static int generate_noise(msomn *m, int filter = 1) {
  const int N = m->N;
  if (int rt = noise_mode_refuse(m, "noise draw")) return rt;
  if (m->noise_mode == 1) {
    // (tiles: every cell of the window and of its ring is keyed by the global cell it is or mirrors; the counter moves alike on all ranks)
    if (m->ntiles > 1) launch_n_noise_tile(m->st, m->cs[0], m->cg[0], m->p.amp_stoch, m->seed, m->noise_draw++, m->ox, m->oy, N);
    else launch_n_noise(m->st, m->cs[0], m->cg[0], m->p.amp_stoch, m->seed, m->noise_draw++);
    HIPCHK(hipGetLastError());
    return filter ? cell_wavelet_filter(m, 1) : MSOM_OK;
  }
  std::vector<double> h((size_t)N * N);
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) {
      const double a = sqrt(-2. * log(((double)(rand()) + 1.) / ((double)(RAND_MAX) + 2.)));
      h[(size_t)j * N + i] = m->p.amp_stoch * (a * cos(2 * M_PI * rand() / (double)RAND_MAX));
    }
  int r = upload_cells(m, h.data());
  return r || !filter ? r : cell_wavelet_filter(m);
}
extern "C" int msomn_noise_draw(msomn_t *m, int filter) {
  if (int rt = wv_refuse(m, "msomn_noise_draw")) return rt;
  NEED_NCONST(m);
  if (m->cnlev == 0) { msom_set_error("stochastic forcing is off"); return MSOM_ERR_STATE; }
  if (int rt = noise_mode_refuse(m, "msomn_noise_draw")) return rt;
  return generate_noise(m, filter);
}
extern "C" int msomn_dbg_noise(msomn_t *m, const double *set, int filter, double *get) {
  if (int rt = wv_refuse(m, "msomn_dbg_noise")) return rt;
  NEED_NCONST(m);
  if (m->cnlev == 0) { msom_set_error("stochastic forcing is off"); return MSOM_ERR_STATE; }
  int r;
  if (set && (r = upload_cells(m, set))) return r;
  if (filter && (r = cell_wavelet_filter(m))) return r;
  if (get) {
    const NatGeom &g = m->cg[0];
    HIPCHK(hipMemcpy2DAsync(get, g.nx * sizeof(double), m->cs[0] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), g.nx * sizeof(double), g.ny, hipMemcpyDefault, m->st));
  }
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
extern "C" int msomn_dbg_csig(msomn_t *m, int level, double *out) {
  if (int rt = wv_refuse(m, "msomn_dbg_csig")) return rt;
  NEED_NCONST(m);
  if (level < 0 || level >= m->cnlev || !out) { msom_set_error("bad level %d", level); return MSOM_ERR_ARG; }
  const NatGeom &g = m->cg[level];
  HIPCHK(hipMemcpy2DAsync(out, g.nx * sizeof(double), m->csig[level] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), g.nx * sizeof(double), g.ny, hipMemcpyDefault, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

// ---- wavelet filter of the vertex model: wavelet_filter qg_baroclinic_ms.h:346-400, sig_lev / mask_c :525-578,
// wavelet_mask / inverse_wavelet_mask qg-node/wavelet_vertex.h:10-46 (the transform runs on the CELL average of psi)
static int wv_setup(msomn *m) {
  const NodeParams &p = m->p;
  int r;
  if (m->ntiles > 1) return ct_wv_setup(m);
  if (m->wg.empty()) {
    int c = 1;
    while ((m->N >> c) >= 1) c++;
    m->wg.resize(c); m->ws.assign(c, nullptr); m->wr.assign(c, nullptr); m->wsig.assign(c, nullptr); m->wmc.assign(c, nullptr);
    for (int k = 0; k < c; k++) {
      m->wg[k] = cell_geom(m->N >> k);
      if ((r = dalloc(&m->ws[k], m->wg[k].ls * m->nl)) || (r = dalloc(&m->wr[k], m->wg[k].ls * m->nl)) || (r = dalloc(&m->wsig[k], m->wg[k].ls)) ||
          (r = dalloc(&m->wmc[k], m->wg[k].ls)))
        return r;
    }
  }
  const int K = (int)m->wg.size(), N = m->N;
  const size_t n1 = N + 1;
  // sig_lev :527-552 (low pass only): a vertex scalar read at the cell with the same index
  std::vector<double> s2;
  if (p.fac_filt_Rd > 0) {
    if (m->nl < 2) { msom_set_error("fac_filt_Rd > 0 needs the stratification S2 (nl >= 2)"); return MSOM_ERR_CONFIG; }
    s2.resize(n1 * n1 * m->nlm);
    if ((r = download_g(m, m->f[MSOMN_S2], m->g, m->nlm, s2.data()))) return r;
  }
  std::vector<std::vector<double>> sl(K);
  for (int k = 0; k < K; k++) {
    const int n = N >> k, fx = 2 * n;
    const double Delta = p.L0 / n;
    sl[k].resize((size_t)n * n);
    for (int j = 0; j < n; j++)
      for (int i = 0; i < n; i++) {
        double ref_flag = 0;
        if (k > 0) {
          ref_flag += sl[k - 1][(size_t)(2 * j) * fx + 2 * i]; ref_flag += sl[k - 1][(size_t)(2 * j + 1) * fx + 2 * i];
          ref_flag += sl[k - 1][(size_t)(2 * j) * fx + 2 * i + 1]; ref_flag += sl[k - 1][(size_t)(2 * j + 1) * fx + 2 * i + 1];
        }
        double v;
        if (ref_flag > 0) v = 1;
        else {
          double L2;
          if (p.fac_filt_Rd > 0) L2 = fmin(p.fac_filt_Rd * p.dh[0] / sqrt(s2[((size_t)j << k) * n1 + ((size_t)i << k)]), p.Lfmax);
          else L2 = p.Lfmax + (j * Delta / p.L0) * (p.Lfmin - p.Lfmax);
          if (L2 > 2 * Delta) v = 0;
          else if (L2 <= 2 * Delta && L2 > Delta) v = 1 - (L2 - Delta) / Delta;
          else v = 1;
        }
        sl[k][(size_t)j * n + i] = v;
      }
    const NatGeom &g = m->wg[k];
    HIPCHK(hipMemcpy2DAsync(m->wsig[k] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), sl[k].data(), g.nx * sizeof(double), g.nx * sizeof(double), g.ny,
                            hipMemcpyHostToDevice, m->st));
  }
  HIPCHK(hipStreamSynchronize(m->st));
  // mask_c :567-575: cell average of the vertex mask, restricted to every level
  launch_wv_vert2cell(m->st, m->f[MSOMN_MASK], m->g, m->wmc[0], m->wg[0], 1);
  for (int k = 1; k < K; k++) launch_wv_restrict(m->st, m->wmc[k - 1], m->wg[k - 1], m->wmc[k], m->wg[k], 1);
  HIPCHK(hipGetLastError());
  m->wv_ready = 1;
  return MSOM_OK;
}
// ws[0] <- inverse_wavelet_mask(sig_lev * wavelet_mask(ws[0])), all layers at once; dirichlet(0) ghost cells on every level
static int wv_masked_apply(msomn *m) {
  if (m->ntiles > 1) return ct_masked_apply(m);   // the result comes with its ring (k_wv_vertex_update reads it)
  const int K = (int)m->wg.size(), nl = m->nl;
  auto bc = [&](double *f, const NatGeom &g) { launch_fill_ghost(m->st, f, g, nl, BC_DIRICHLET0, WALL_ALL); };
  bc(m->ws[0], m->wg[0]);
  for (int k = 1; k < K; k++) {
    launch_wv_restrict(m->st, m->ws[k - 1], m->wg[k - 1], m->ws[k], m->wg[k], nl);
    bc(m->ws[k], m->wg[k]);
  }
  if (K == 1) launch_wv_root_m(m->st, m->ws[0], m->wsig[0], m->wmc[0], m->ws[0], m->wg[0], nl);
  else {
    launch_wv_root_m(m->st, m->ws[K - 1], m->wsig[K - 1], m->wmc[K - 1], m->wr[K - 1], m->wg[K - 1], nl);
    bc(m->wr[K - 1], m->wg[K - 1]);
  }
  for (int k = K - 2; k >= 0; k--) {
    double *out = k == 0 ? m->ws[0] : m->wr[k];
    launch_wv_recon_m(m->st, m->ws[k], m->ws[k + 1], m->wr[k + 1], m->wsig[k], m->wmc[k], out, m->wg[k], m->wg[k + 1], nl);
    bc(out, m->wg[k]);
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
static int invert_q(msomn *m, double *q);
static int comp_q(msomn *m, const double *psi, double *q);
extern "C" int msomn_wavelet_filter(msomn_t *m, double dtflt) {
  if (int rt = wv_refuse(m, "msomn_wavelet_filter")) return rt;
  NEED_NCONST(m);
  int r;
  if (!m->wv_ready && (r = wv_setup(m))) return r;
  if ((r = invert_q(m, m->f[MSOMN_Q]))) return r;
  launch_wv_vert2cell(m->st, m->f[MSOMN_PSI], m->g, m->ws[0], m->wg[0], m->nl);
  if ((r = wv_masked_apply(m))) return r;
  if (m->p.Lfmax < 1e30)  // `if (Lfmax < HUGE)`, :380
    launch_wv_vertex_update(m->st, m->f[MSOMN_PSI], m->f[MSOMN_PSIF], m->ws[0], m->f[MSOMN_MASK], m->g, m->wg[0], m->nl, dtflt, m->nbar, 1);
  launch_n_bnd_const(m->st, m->f[MSOMN_PSI], m->g, m->nl, m->psi_bc, 0, m->walls);
  if ((r = comp_q(m, m->f[MSOMN_PSI], m->f[MSOMN_Q]))) return r;
  m->nbar++;
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
// what = 0: sig_lev as used at the cells, 1: mask_c; level k, out [n][n]
extern "C" int msomn_dbg_wv_get(msomn_t *m, int what, int level, double *out) {
  if (int rt = wv_refuse(m, "msomn_dbg_wv_get")) return rt;
  NEED_NCONST(m);
  int r;
  if (!m->wv_ready && (r = wv_setup(m))) return r;
  if (level < 0 || level >= (int)m->wg.size() || !out) { msom_set_error("bad level %d", level); return MSOM_ERR_ARG; }
  const NatGeom &g = m->wg[level];
  const double *src = what ? m->wmc[level] : m->wsig[level];
  HIPCHK(hipMemcpy2DAsync(out, g.nx * sizeof(double), src + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), g.nx * sizeof(double), g.ny, hipMemcpyDefault, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
// the masked transform pair alone on a cell field [nl][N][N]
extern "C" int msomn_dbg_wv_apply(msomn_t *m, const double *in, double *out) {
  if (int rt = wv_refuse(m, "msomn_dbg_wv_apply")) return rt;
  NEED_NCONST(m);
  int r;
  if (!m->wv_ready && (r = wv_setup(m))) return r;
  if (!in || !out) return MSOM_ERR_ARG;
  const NatGeom &g = m->wg[0];
  for (int l = 0; l < m->nl; l++)
    HIPCHK(hipMemcpy2DAsync(m->ws[0] + nat_idx(g, l, 0, 0), g.pitch * sizeof(double), in + (size_t)l * g.nx * g.ny, g.nx * sizeof(double), g.nx * sizeof(double), g.ny,
                            hipMemcpyDefault, m->st));
  if ((r = wv_masked_apply(m))) return r;
  for (int l = 0; l < m->nl; l++)
    HIPCHK(hipMemcpy2DAsync(out + (size_t)l * g.nx * g.ny, g.nx * sizeof(double), m->ws[0] + nat_idx(g, l, 0, 0), g.pitch * sizeof(double), g.nx * sizeof(double), g.ny,
                            hipMemcpyDefault, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

// msomn_set_const in two parts (msomn_host.h): the state file holds the inputs after node_const_inputs, and a load into a handle
// without constants installs them as they are and runs node_const_derived alone
static int check_dh(const msomn *m) {
  for (int l = 0; m->nl > 1 && l < m->nl; l++)
    if (m->p.dh[l] == 0.) { msom_set_error("thickness = 0: check the definition of dh in params.in"); return MSOM_ERR_CONFIG; }
  return MSOM_OK;
}
int node_const_inputs(msomn *m) {
  const NodeParams &p = m->p;
  const int nl = m->nl;
  const size_t n1 = m->g.nx, n2 = m->g.ny;   // the tile's vertices; y of row j is that of the GLOBAL row oy + j
  int r;
  if ((r = check_dh(m))) return r;
  if (nl == 1) return MSOM_OK;
  // S2: N^2 -> f^2 / N^2 with f = f0 + flag_ms beta (y - L0/2)  (qg_baroclinic_ms.h:501-505); init-time host pass
  std::vector<double> h(n1 * n2 * m->nlm);
  if ((r = download_g(m, m->f[MSOMN_S2], m->g, m->nlm, h.data()))) return r;
  for (int l = 0; l < nl - 1; l++) for (size_t j = 0; j < n2; j++) {
    const double f = p.f0 + p.flag_ms * p.beta * ((j + m->oy) * m->D - 0.5 * p.L0);
    for (size_t i = 0; i < n1; i++) { double &s = h[(l * n2 + j) * n1 + i]; s = f * f / s; }
  }
  if ((r = upload_g(m, m->f[MSOMN_S2], m->g, m->nlm, h.data()))) return r;
  if (m->sqg) {  // :545 surface layer: f / N^2 (f, not f^2)
    std::vector<double> hs(n1 * n2);
    if ((r = download_g(m, m->f[MSOMN_S2S], m->g, 1, hs.data()))) return r;
    for (size_t j = 0; j < n2; j++) {
      const double f = p.f0 + p.flag_ms * p.beta * ((j + m->oy) * m->D - 0.5 * p.L0);
      for (size_t i = 0; i < n1; i++) hs[j * n1 + i] = f / hs[j * n1 + i];
    }
    if ((r = upload_g(m, m->f[MSOMN_S2S], m->g, 1, hs.data()))) return r;
  }
  if (p.scale_topo != 1.) {
    std::vector<double> tp(n1 * n2);
    if ((r = download_g(m, m->f[MSOMN_TOPO], m->g, 1, tp.data()))) return r;
    for (double &v : tp) v *= p.scale_topo;
    if ((r = upload_g(m, m->f[MSOMN_TOPO], m->g, 1, tp.data()))) return r;
  }
  return MSOM_OK;
}
double node_clamped_dt(const msomn *m) {
  const NodeParams &p = m->p;
  double DT = p.DT;
  if (p.nu != 0) DT = 0.5 * fmin(DT, m->D * m->D / p.nu / 4.);  // qg-node/qg.h:511-512
  if (p.beta != 0) DT = fmin(DT, 1 / (2. * p.beta * p.L0));
  return DT;
}
int node_const_derived(msomn *m) {
  NodeParams &p = m->p;
  const int nl = m->nl;
  const size_t n1 = m->g.nx, n2 = m->g.ny;
  int r;
  if ((r = check_dh(m))) return r;
  if (nl > 1) {
    double dhc[MSOM_MAXNL];
    for (int l = 0; l < nl - 1; l++) dhc[l] = 0.5 * (p.dh[l] + p.dh[l + 1]);
    m->lc.idh0[0] = m->sqg ? 1. / p.dh[0] : 0.;  // sqg_baroclinic_ms.h:502 "surface layer: 1/h"
    m->lc.idh1[0] = 1. / (dhc[0] * p.dh[0]);
    for (int l = 1; l < nl - 1; l++) { m->lc.idh0[l] = 1. / (dhc[l - 1] * p.dh[l]); m->lc.idh1[l] = 1. / (dhc[l] * p.dh[l]); }
    m->lc.idh0[nl - 1] = 1. / (dhc[nl - 2] * p.dh[nl - 1]); m->lc.idh1[nl - 1] = 0.;
    std::vector<double> h(n1 * n2 * m->nlm);   // the transformed S2
    if ((r = download_g(m, m->f[MSOMN_S2], m->g, m->nlm, h.data()))) return r;
    m->s2_xuniform = 1;
    for (size_t r0 = 0; r0 < (size_t)(nl - 1) * n2 && m->s2_xuniform; r0++)
      for (size_t i = 1; i < n1; i++) if (h[r0 * n1 + i] != h[r0 * n1]) { m->s2_xuniform = 0; break; }
    if (m->ntiles > 1) {   // every tile takes the same path: row tables only if S2 is x-independent on all of them
      m->h_scal[NSC_RES] = m->s2_xuniform;
      HIPCHK(hipMemcpyAsync(m->d_scal + NSC_RES, m->h_scal + NSC_RES, sizeof(double), hipMemcpyHostToDevice, m->st));
      if ((r = nt_reduce(m, NSC_RES, 1, RED_MIN))) return r;
      m->s2_xuniform = m->h_scal[NSC_RES] != 0.;
    }
  } else if (p.gp_low != 0.) m->iRd2_low = p.f0 * p.f0 / (p.gp_low * p.dh[nl - 1]);
  if ((r = build_levels(m))) return r;
  if (m->stochastic && (r = stoch_setup(m))) return r;  // event init_stoch
  bnd_psi(m);
  p.DT = node_clamped_dt(m);
  return MSOM_OK;
}
extern "C" int msomn_set_const(msomn_t *m) {
  if (!m) return MSOM_ERR_ARG;
  int r;
  HIPCHK(hipStreamSynchronize(m->st));   // a sample may still be running into the arrays that go
  nstats_drop(m);
  nfloats_drop(m);
  if ((r = node_const_inputs(m)) || (r = node_const_derived(m))) return r;
  m->noise_draw = 0;
  if ((r = comp_q(m, m->f[MSOMN_PSI], m->f[MSOMN_Q]))) return r;
  HIPCHK(hipStreamSynchronize(m->st));
  m->const_set = 1;
  m->wv_ready = 0;
  return MSOM_OK;
}

extern "C" int msomn_update(msomn_t *m, int qf, int dqf, double dtmax, double *dt_out) {
  NEED_NCONST(m); NEED_FIELD(m, qf); NEED_FIELD(m, dqf);
  int r;
  if ((r = invert_q(m, m->f[qf])) || (r = rhs_pv(m, m->f[qf], m->f[dqf]))) return r;
  double dt;
  if ((r = adjust_dt(m, dtmax, &dt))) return r;
  if (dt_out) *dt_out = dt;
  return MSOM_OK;
}
extern "C" int msomn_advance(msomn_t *m, int out, int in, int dq, double dt) {
  NEED_FIELD(m, out); NEED_FIELD(m, in); NEED_FIELD(m, dq);
  if (m->stochastic && noise_mode_refuse(m, "msomn_advance")) return MSOM_ERR_CONFIG;
  launch_advance(m->st, m->f[out], m->f[in], m->f[dq], nullptr, m->g, m->nl, dt, 0.);
  if (m->stochastic) {  // qg-node/qg.h:306-320
    if (m->cnlev == 0) { msom_set_error("stochastic: call msomn_set_const after switching it on"); return MSOM_ERR_STATE; }
    m->corrector_step = (m->corrector_step + 1) % 2;
    double dts = sqrt(dt);
    if (m->corrector_step) {
      int r = generate_noise(m);
      if (r) return r;
      dts = dts / sqrt(2);  // to get sqrt(dt)/2 (in the predictor step, dt = dt/2)
    }
    if (m->nl > 1 && !m->quiet) fprintf(stdout, "Stochastic not ready for multilayer yet \n");
    launch_n_add_noise(m->st, m->f[out], m->cs[0], m->g, m->cg[0], dts);
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
extern "C" int msomn_invert_q(msomn_t *m, int qf, msom_mgstats *st) {
  NEED_NCONST(m); NEED_FIELD(m, qf);
  int r = invert_q(m, m->f[qf]);
  if (st) *st = m->mg;
  if (!r) HIPCHK(hipStreamSynchronize(m->st));
  return r;
}
extern "C" int msomn_comp_q(msomn_t *m, int pf, int qf) { NEED_NCONST(m); NEED_FIELD(m, pf); NEED_FIELD(m, qf); return comp_q(m, m->f[pf], m->f[qf]); }
extern "C" int msomn_rhs_pv(msomn_t *m, int qf, int dqf) { NEED_NCONST(m); NEED_FIELD(m, qf); NEED_FIELD(m, dqf); return rhs_pv(m, m->f[qf], m->f[dqf]); }
extern "C" int msomn_dbg_del2_zeta(msomn_t *m) {
  if (int rt = nt_refuse(m, "msomn_dbg_del2_zeta")) return rt;
  NEED_NCONST(m);
  launch_n_del2(m->st, m->f[MSOMN_PSI], m->f[MSOMN_ZETA], m->g, m->nl, 0., 1., m->D);
  bnd_q(m, m->f[MSOMN_ZETA]);
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
// event forcing (i++), qg-node/qg.c:136-145: q_forcing depends on y and t only -> one row on the host
extern "C" int msomn_forcing(msomn_t *m) {
  if (!m) return MSOM_ERR_ARG;
  const NodeParams &p = m->p;
  const double L0 = p.L0, t = m->t;
  HIPCHK(hipStreamSynchronize(m->st));
  for (int j = 0; j <= m->N; j++) {
    const double y = j * m->D;
    m->h_row[j] = -(p.tau0 + p.tau1 * cos(2 * M_PI * t / p.tf1)) / p.dh[0] * p.forc_mode * M_PI / L0 *
                  sin(p.forc_mode * M_PI * (y + y * (y - L0) * 2 / (L0 * L0) * p.dy_ws * sin(2 * M_PI * t / p.tf2)) / L0);
  }
  HIPCHK(hipMemcpyAsync(m->d_row, m->h_row, (m->N + 1) * sizeof(double), hipMemcpyHostToDevice, m->st));
  launch_n_rowfill(m->st, m->f[MSOMN_QFORC], m->d_row + m->oy, m->g);   // a tile takes its rows of the global profile
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
extern "C" int msomn_step(msomn_t *m, int with_forcing_event) {
  NEED_NCONST(m);
  if (m->stats_on && !m->stats_mask) { msom_set_error("msomn_step: option stats = 1 and no msomn_stats_begin since msomn_set_const"); return MSOM_ERR_STATE; }
  int r;
  double d, tn;
  if (m->stochastic && (r = noise_mode_refuse(m, "msomn_step"))) return r;
  if (with_forcing_event && (r = msomn_forcing(m))) return r;
  if ((r = msomn_update(m, MSOMN_Q, MSOMN_DQ, m->p.DT, &d))) return r;
  m->dt = step_dtnext(m->t, m->tnext, d, &tn);   // dtnext() [Basilisk, SURVEY App. B]
  // the automatic sample: q_n and the psi stage 1 inverted from it (masked, sides set, on tiles exchanged by the tendency), weight dt_n
  if (m->stats_on && m->stats_count++ % m->stats_every == 0 && (r = nstats_sample(m, m->dt))) return r;
  // the floats' stage 1 reads the same psi_n, before the second update overwrites it
  if (m->floats.on && (r = nfloats_hook(m, 1, tn))) return r;
  if ((r = msomn_advance(m, MSOMN_QPRED, MSOMN_Q, MSOMN_DQ, m->dt / 2.))) return r;
  if ((r = msomn_update(m, MSOMN_QPRED, MSOMN_DQ, m->dt, &d))) return r;
  if ((r = msomn_advance(m, MSOMN_Q, MSOMN_Q, MSOMN_DQ, m->dt))) return r;
  // ... and their stage 2 psi_{n + 1/2}, behind the final advance: a recorded sample of q is q_{n + 1} at x_{n + 1}
  if (m->floats.on && (r = nfloats_hook(m, 2, tn))) return r;
  m->t = tn;
  m->iter++;
  return MSOM_OK;
}
extern "C" int msomn_set_tnext(msomn_t *m, double t) { if (!m) return MSOM_ERR_ARG; m->tnext = t; return MSOM_OK; }
extern "C" double msomn_time(msomn_t *m) { return m ? m->t : NAN; }
extern "C" double msomn_dt(msomn_t *m) { return m ? m->dt : NAN; }
extern "C" int msomn_iter(msomn_t *m) { return m ? m->iter : MSOM_ERR_ARG; }
extern "C" int msomn_last_mgstats(msomn_t *m, msom_mgstats *s) { if (!m || !s) return MSOM_ERR_ARG; *s = m->mg; return MSOM_OK; }
extern "C" int msomn_ke(msomn_t *m, double *ke) {
  if (!m || !ke) return MSOM_ERR_ARG;
  // tiles: every vertex is counted once (a tile leaves out its east and north edge unless that edge is a wall)
  int r = nt_exchange(m, m->f[MSOMN_PSI], m->g, 0, 1);
  if (r) return r;
  launch_n_ke(m->st, m->f[MSOMN_PSI], m->partial, m->d_scal + NSC_KE, m->g, m->D, m->walls);
  if ((r = nt_reduce(m, NSC_KE, 1, RED_SUM))) return r;
  *ke = -m->h_scal[NSC_KE];
  return MSOM_OK;
}

// event write_1d_diag (qg-node/qg.h:361-399): out = {ke, dissipation, forcing}
extern "C" int msomn_diag1d(msomn_t *m, double *out3) {
  if (!m || !out3) return MSOM_ERR_ARG;
  // (the cell loop leaves out the last column and row of vertices: on tiles that is the east and north edge of every tile)
  int r;
  if ((r = nt_exchange(m, m->f[MSOMN_PSI], m->g, 0, 1)) || (r = nt_exchange(m, m->f[MSOMN_Q], m->g, 0, 1))) return r;
  launch_n_diag1d(m->st, m->f[MSOMN_PSI], m->f[MSOMN_Q], m->f[MSOMN_QFORC], m->partial, m->d_scal + NSC_DIAG, m->g, m->p.nu, m->D);
  if ((r = nt_reduce(m, NSC_DIAG, 3, RED_SUM))) return r;
  for (int k = 0; k < 3; k++) out3[k] = -m->h_scal[NSC_DIAG + k];
  return MSOM_OK;
}

// ---- raw multigrid pieces (parity tests)
// (a tiled handle: the levels that live on the tile; a gathered level has no tile-sized arrays)
#define NEED_LEVEL(m, k) if (!(m) || (k) < 0 || (k) >= ((m)->ntiles > 1 ? (m)->kg : (m)->nlev)) { msom_set_error("bad level %d", (int)(k)); return MSOM_ERR_ARG; }
extern "C" int msomn_dbg_relax(msomn_t *m, int k, double *da, const double *res, int nsweeps) {
  NEED_NCONST(m); NEED_LEVEL(m, k);
  NLevel &L = m->lev[k];
  int r;
  if ((r = upload_lev(m, L, L.da, da)) || (r = upload_lev(m, L, L.res, res))) return r;
  launch_n_bnd_const(m->st, L.da, L.ga, m->nl, 0., L.sp, L.walls);
  if (L.tiled && (r = nt_exchange(m, L.da, L.ga, L.sp, m->nl))) return r;
  m->tile_err = 0;
  relax_sweeps(m, k, nsweeps);
  if (m->tile_err) return MSOM_ERR_COMM;
  HIPCHK(hipGetLastError());
  return download_lev(m, L, L.da, da);
}
extern "C" int msomn_dbg_residual(msomn_t *m, const double *a, const double *b, double *res, double *maxres) {
  NEED_NCONST(m);
  int r;
  if ((r = upload_g(m, m->f[MSOMN_TMP], m->g, m->nl, a)) || (r = upload_g(m, m->f[MSOMN_DQ], m->g, m->nl, b))) return r;
  HIPCHK(hipMemsetAsync(m->d_scal + NSC_RES, 0, sizeof(double), m->st));
  if ((r = nt_exchange(m, m->f[MSOMN_TMP], m->g, 0, m->nl))) return r;
  residual_pass(m, m->f[MSOMN_TMP], m->f[MSOMN_DQ], 0);
  if ((r = nt_reduce(m, NSC_RES, 1, RED_MAX))) return r;
  if (maxres) *maxres = m->h_scal[NSC_RES];
  return download_lev(m, m->lev[0], m->lev[0].res, res);
}
extern "C" int msomn_dbg_restrict(msomn_t *m, int k, const double *fine, double *coarse) {
  NEED_NCONST(m); NEED_LEVEL(m, k); NEED_LEVEL(m, k + 1);
  int r;
  NLevel &Lf = m->lev[k], &Lc = m->lev[k + 1];
  if ((r = upload_lev(m, Lf, Lf.res, fine))) return r;
  launch_n_bnd_const(m->st, Lf.res, Lf.ga, m->nl, 0., Lf.sp, Lf.walls);
  if (Lf.tiled && (r = nt_exchange(m, Lf.res, Lf.ga, Lf.sp, m->nl))) return r;
  launch_n_restrict(m->st, Lf.res, Lf.ga, Lc.res, Lc.ga, m->nl, 0, Lf.sp, Lc.sp);
  launch_n_bnd_const(m->st, Lc.res, Lc.ga, m->nl, 0., Lc.sp, Lc.walls);
  return download_lev(m, Lc, Lc.res, coarse);
}
extern "C" int msomn_dbg_prolong(msomn_t *m, int k, const double *coarse, double *fine) {
  NEED_NCONST(m); NEED_LEVEL(m, k); NEED_LEVEL(m, k - 1);
  int r;
  NLevel &Lc = m->lev[k], &Lf = m->lev[k - 1];
  if ((r = upload_lev(m, Lc, Lc.da, coarse))) return r;
  launch_n_bnd_const(m->st, Lc.da, Lc.ga, m->nl, 0., Lc.sp, Lc.walls);
  launch_n_prolong(m->st, Lc.da, Lc.ga, Lf.da, Lf.ga, m->nl, Lc.sp, Lf.sp, Lf.walls);
  return download_lev(m, Lf, Lf.da, fine);
}
extern "C" int msomn_dbg_level_mask(msomn_t *m, int k, double *out) {
  NEED_NCONST(m); NEED_LEVEL(m, k);
  return download_g(m, m->lev[k].mask, m->lev[k].g, 1, out);
}
