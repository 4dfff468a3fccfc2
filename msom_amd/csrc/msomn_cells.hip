// msomn_cells.hip -- the cell-centred wavelet pyramids of the vertex model on tiles (option wavelet_tiles; DESIGN.md section 7,
// "Wavelet pyramid on tiles").  Index arithmetic: node_tile_inl.h (ctile_*).
//
// The pyramids are the single tile's (msom_node.hip: cs / cr / csig of the noise, ws / wr / wsig / wmc of the scale filter) with the
// geometry of the multigrid on tiles: levels k < kg hold the tile's window, levels k >= kg the global grid on every rank, down to the
// 1-cell root.  A cell belongs to one tile, so the gather has no copies to choose between.  Every kernel of the transform is the single
// tile's, launched on the window; what it reads beyond the window is the ring, which holds the single tile's bits: beyond a wall
// launch_fill_ghost with the tile's wall bits, beyond a seam the neighbour's edge cell (nt_exchange_cells).
#include "msomn_host.h"

NatGeom cell_geom_rect(int nx, int ny) {
  NatGeom g;
  g.nx = nx; g.ny = ny;
  g.pitch = ((nx + 15) / 16) * 16 + 2 * MSOM_XP;
  g.rows = ny + 2 * MSOM_YP;
  g.ls = (size_t)g.pitch * g.rows;
  return g;
}

static int dalloc0(double **p, size_t n) {
  HIPCHK(hipMalloc((void **)p, n * sizeof(double)));
  HIPCHK(hipMemset(*p, 0, n * sizeof(double)));
  return MSOM_OK;
}
static void dfree(double *&p) { if (p) (void)hipFree(p); p = nullptr; }

// one pyramid of the handle: the noise's (one layer, Neumann, no mask) or the scale filter's (nl layers, dirichlet(0), mask_c)
struct CellPyr {
  std::vector<NatGeom> &g;
  std::vector<double *> &s, &r, &sig, *mc;
  CellPiece &P;
  int nl, bc;
};
static CellPyr noise_pyr(msomn *m) { return {m->cg, m->cs, m->cr, m->csig, nullptr, m->cpiece, 1, BC_NEUMANN}; }
static CellPyr filter_pyr(msomn *m) { return {m->wg, m->ws, m->wr, m->wsig, &m->wmc, m->wpiece, m->nl, BC_DIRICHLET0}; }

void ct_free_piece(CellPiece &P) { dfree(P.s); dfree(P.r); }
// (re)allocates the pyramid for the gather level of this msomn_set_const: no global array of a tiled level
static int ct_alloc(msomn *m, CellPyr y) {
  for (auto *v : {&y.s, &y.r, &y.sig}) { for (double *&q : *v) dfree(q); v->clear(); }
  if (y.mc) { for (double *&q : *y.mc) dfree(q); y.mc->clear(); }
  ct_free_piece(y.P);
  int K = 1, r;
  while ((m->N >> K) >= 1) K++;
  y.g.resize(K); y.s.assign(K, nullptr); y.r.assign(K, nullptr); y.sig.assign(K, nullptr);
  if (y.mc) y.mc->assign(K, nullptr);
  for (int k = 0; k < K; k++) {
    const NodeTile t = ntile_level(m->N, m->px, m->py, m->rank, k);
    y.g[k] = k < m->kg ? cell_geom_rect(t.tx, t.ty) : cell_geom(m->N >> k);
    if ((r = dalloc0(&y.s[k], y.g[k].ls * y.nl)) || (r = dalloc0(&y.r[k], y.g[k].ls * y.nl)) || (r = dalloc0(&y.sig[k], y.g[k].ls))) return r;
    if (y.mc && (r = dalloc0(&(*y.mc)[k], y.g[k].ls))) return r;
  }
  const NodeTile tg = ntile_level(m->N, m->px, m->py, m->rank, m->kg);
  y.P.g = cell_geom_rect(tg.tx, tg.ty);
  if ((r = dalloc0(&y.P.s, y.P.g.ls * y.nl)) || (r = dalloc0(&y.P.r, y.P.g.ls * y.nl))) return r;
  return MSOM_OK;
}

// the ring of a cell field of the tile, corners included.  x phase: the edge columns with their ghost rows (at a wall in y the
// boundary condition has filled them, so a corner with one wall side and one seam side gets the neighbour's ghost cell, the single
// tile's number); y phase: the edge rows with their fresh ring columns.  Collective; call it after the wall fill
int nt_exchange_cells(msomn *m, double *f, const NatGeom &g, int nl) {
  if (m->ntiles == 1) return MSOM_OK;
  Comm *c = m->comm;
  if ((size_t)nl * ((g.nx > g.ny ? g.nx : g.ny) + 2) > comm_bufcount(c)) {
    msom_set_error("halo message of %d layers of a tile of %d x %d cells exceeds the communication buffers (%zu)", nl, g.nx, g.ny, comm_bufcount(c));
    return MSOM_ERR_ARG;
  }
  Xfer x[2];
  int n = 0, r;
  const int h = g.ny + 2, w = g.nx + 2;
  for (int dir : {DIR_W, DIR_E}) {
    if (m->nb[dir] < 0) continue;
    launch_n_pack_strip(m->st, f, g, 0, nl, dir == DIR_W ? 0 : g.nx - 1, -1, 1, h, comm_sendbuf(c, dir));
    x[n++] = {m->nb[dir], dir, comm_sendbuf(c, dir), comm_recvbuf(c, dir), (size_t)h * nl};
  }
  if ((r = comm_exchange(c, x, n))) return r;
  for (int dir : {DIR_W, DIR_E})
    if (m->nb[dir] >= 0) launch_n_unpack_strip(m->st, f, g, 0, nl, dir == DIR_W ? -1 : g.nx, -1, 1, h, comm_recvbuf(c, dir));
  n = 0;
  for (int dir : {DIR_S, DIR_N}) {
    if (m->nb[dir] < 0) continue;
    launch_n_pack_strip(m->st, f, g, 0, nl, -1, dir == DIR_S ? 0 : g.ny - 1, w, 1, comm_sendbuf(c, dir));
    x[n++] = {m->nb[dir], dir, comm_sendbuf(c, dir), comm_recvbuf(c, dir), (size_t)w * nl};
  }
  if ((r = comm_exchange(c, x, n))) return r;
  for (int dir : {DIR_S, DIR_N})
    if (m->nb[dir] >= 0) launch_n_unpack_strip(m->st, f, g, 0, nl, -1, dir == DIR_S ? -1 : g.ny, w, 1, comm_recvbuf(c, dir));
  HIPCHK(hipGetLastError());
  m->nexch++;
  return MSOM_OK;
}
// wall fill, then the exchange: the whole ring of a cell field of the tile
int ct_ring(msomn *m, double *f, const NatGeom &g, int nl, int bc) {
  launch_fill_ghost(m->st, f, g, nl, bc, m->walls);
  return nt_exchange_cells(m, f, g, nl);
}
// the tiles' windows of level kg (geometry pg, interior only) -> the global level on every rank: one all-gather
static int ct_gather(msomn *m, const double *piece, const NatGeom &pg, int nl, double *global, const NatGeom &gg) {
  const size_t count = (size_t)nl * pg.nx * pg.ny;
  if (count > m->gcount) { msom_set_error("gather of %zu doubles exceeds its buffer (%zu)", count, m->gcount); return MSOM_ERR_ARG; }
  launch_n_pack_strip(m->st, piece, pg, 0, nl, 0, 0, pg.nx, pg.ny, m->gsend);
  int r = comm_allgather(m->comm, m->gsend, m->grecv, count);
  if (r) return r;
  launch_c_assemble(m->st, m->grecv, global, gg, nl, m->N, m->px, m->py, m->kg);
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

// s[0] <- inverse transform(sig * transform(s[0])) on the tiles: kg - 1 exchanges and one all-gather on the way down, kg exchanges on
// the way up (the last one is the ring of the result, which k_n_add_noise and k_wv_vertex_update read): 2 kg - 1 in all.
// ghosts_set: the ring of s[0] is in place (k_n_noise_tile)
static int ct_transform(msomn *m, CellPyr y, int ghosts_set) {
  const int K = (int)y.g.size(), kg = m->kg, nl = y.nl;
  hipStream_t st = m->st;
  int r;
  auto wall = [&](double *f, const NatGeom &g) { launch_fill_ghost(st, f, g, nl, y.bc, WALL_ALL); };
  auto root = [&](const double *s, int k, double *out) {
    if (y.mc) launch_wv_root_m(st, s, y.sig[k], (*y.mc)[k], out, y.g[k], nl);
    else launch_wv_root(st, s, y.sig[k], out, y.g[k], nl);
  };
  auto recon = [&](int k, const double *sc, const double *rc, const NatGeom &cg, double *out) {
    if (y.mc) launch_wv_recon_m(st, y.s[k], sc, rc, y.sig[k], (*y.mc)[k], out, y.g[k], cg, nl);
    else launch_wv_recon(st, y.s[k], sc, rc, y.sig[k], out, y.g[k], cg, nl);
  };
  if (!ghosts_set) launch_fill_ghost(st, y.s[0], y.g[0], nl, y.bc, m->walls);   // (nothing of the transform reads the ring of s[0])
  for (int k = 1; k < kg; k++) {   // the tiled levels: the reconstruction reads s[k] one coarse cell beyond the window
    launch_wv_restrict(st, y.s[k - 1], y.g[k - 1], y.s[k], y.g[k], nl);
    if ((r = ct_ring(m, y.s[k], y.g[k], nl, y.bc))) return r;
  }
  launch_wv_restrict(st, y.s[kg - 1], y.g[kg - 1], y.P.s, y.P.g, nl);
  if ((r = ct_gather(m, y.P.s, y.P.g, nl, y.s[kg], y.g[kg]))) return r;
  wall(y.s[kg], y.g[kg]);
  for (int k = kg + 1; k < K; k++) {   // the gathered levels, the root and the way up to r[kg]: the single tile's launches
    launch_wv_restrict(st, y.s[k - 1], y.g[k - 1], y.s[k], y.g[k], nl);
    wall(y.s[k], y.g[k]);
  }
  root(y.s[K - 1], K - 1, y.r[K - 1]);
  wall(y.r[K - 1], y.g[K - 1]);
  for (int k = K - 2; k >= kg; k--) {
    recon(k, y.s[k + 1], y.r[k + 1], y.g[k + 1], y.r[k]);
    wall(y.r[k], y.g[k]);
  }
  const NodeTile tg = ntile_level(m->N, m->px, m->py, m->rank, kg);
  launch_n_extract(st, y.s[kg], y.g[kg], y.P.s, y.P.g, nl, tg.ox, tg.oy);   // the windows with their ring: walls from the global ghost ring
  launch_n_extract(st, y.r[kg], y.g[kg], y.P.r, y.P.g, nl, tg.ox, tg.oy);
  for (int k = kg - 1; k >= 0; k--) {
    const bool top = k + 1 == kg;
    double *out = k == 0 ? y.s[0] : y.r[k];
    recon(k, top ? y.P.s : y.s[k + 1], top ? y.P.r : y.r[k + 1], top ? y.P.g : y.g[k + 1], out);
    if ((r = ct_ring(m, out, y.g[k], nl, y.bc))) return r;
  }
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}
int ct_noise_filter(msomn *m, int ghosts_set) { return ct_transform(m, noise_pyr(m), ghosts_set); }
int ct_masked_apply(msomn *m) { return ct_transform(m, filter_pyr(m), 0); }

static int upload_window(msomn *m, double *dst, const NatGeom &g, const std::vector<double> &a) {
  HIPCHK(hipMemcpy2DAsync(dst + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), a.data(), g.nx * sizeof(double), g.nx * sizeof(double), g.ny, hipMemcpyHostToDevice,
                          m->st));
  return MSOM_OK;
}
// sig_lev of every level (init_stoch qg_stochastic.h:15-47, qg_baroclinic_ms.h:527-552): 1 where a child is > 0, else from the filter
// length L2 of the cell against the cell size.  A cell's value depends on its own children only: the windows of the tiled levels and
// of level kg come from the tile's own cells, level kg is gathered once, the levels above it are built from it on every rank.
// L2(k, i, j, local): the filter length of cell (i, j) of level k; local: indices of the tile's window (k <= kg), else global ones.
// highpass: store 1 - sig (the noise)
template <class F>
static int ct_build_sig(msomn *m, CellPyr y, F L2, bool highpass) {
  const int K = (int)y.g.size(), kg = m->kg;
  int r;
  std::vector<std::vector<double>> sl(K);
  auto level = [&](int k, int nx, int ny, const std::vector<double> *fine, bool local) {
    const double Delta = m->p.L0 / (m->N >> k);
    const int fx = 2 * nx;
    std::vector<double> out((size_t)nx * ny);
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        double ref_flag = 0;
        if (fine) {
          ref_flag += (*fine)[(size_t)(2 * j) * fx + 2 * i]; ref_flag += (*fine)[(size_t)(2 * j + 1) * fx + 2 * i];
          ref_flag += (*fine)[(size_t)(2 * j) * fx + 2 * i + 1]; ref_flag += (*fine)[(size_t)(2 * j + 1) * fx + 2 * i + 1];
        }
        double v;
        if (ref_flag > 0) v = 1;
        else {
          const double l2 = L2(k, i, j, local);
          if (l2 > 2 * Delta) v = 0;
          else if (l2 <= 2 * Delta && l2 > Delta) v = 1 - (l2 - Delta) / Delta;
          else v = 1;
        }
        out[(size_t)j * nx + i] = v;
      }
    return out;
  };
  for (int k = 0; k < kg; k++) sl[k] = level(k, y.g[k].nx, y.g[k].ny, k ? &sl[k - 1] : nullptr, true);
  const std::vector<double> piece = level(kg, y.P.g.nx, y.P.g.ny, &sl[kg - 1], true);
  if ((r = upload_window(m, y.P.s, y.P.g, piece)) || (r = ct_gather(m, y.P.s, y.P.g, 1, y.sig[kg], y.g[kg]))) return r;
  sl[kg].resize((size_t)y.g[kg].nx * y.g[kg].ny);
  HIPCHK(hipMemcpy2DAsync(sl[kg].data(), y.g[kg].nx * sizeof(double), y.sig[kg] + nat_idx(y.g[kg], 0, 0, 0), y.g[kg].pitch * sizeof(double),
                          y.g[kg].nx * sizeof(double), y.g[kg].ny, hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  for (int k = kg + 1; k < K; k++) sl[k] = level(k, y.g[k].nx, y.g[k].ny, &sl[k - 1], false);
  for (int k = 0; k < K; k++) {
    if (highpass) for (double &v : sl[k]) v = 1 - v;
    if ((r = upload_window(m, y.sig[k], y.g[k], sl[k]))) return r;
  }
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

// stoch_setup on tiles: the noise pyramid and the high pass of the uniform filter length L_filt
int ct_stoch_setup(msomn *m) {
  int r;
  if ((r = ct_alloc(m, noise_pyr(m)))) return r;
  m->cnlev = (int)m->cg.size();
  const double L_filt = m->p.L_filt;
  return ct_build_sig(m, noise_pyr(m), [=](int, int, int, bool) { return L_filt; }, true);
}
// wv_setup on tiles: sig_lev (the Lfmax / Lfmin gradient in the global row, or fac_filt_Rd with S2 of layer 0 at vertex (i << k, j << k),
// which the tile holds for its own cells and the gathered multigrid level kg for every cell of the levels above) and mask_c
int ct_wv_setup(msomn *m) {
  const NodeParams &p = m->p;
  int r;
  if ((r = ct_alloc(m, filter_pyr(m)))) return r;
  const CellPyr y = filter_pyr(m);
  const int kg = m->kg;
  std::vector<double> s2, s2g;
  const size_t n1 = m->g.nx, ng1 = m->lev[kg].g.nx;
  if (p.fac_filt_Rd > 0) {
    if (m->nl < 2) { msom_set_error("fac_filt_Rd > 0 needs the stratification S2 (nl >= 2)"); return MSOM_ERR_CONFIG; }
    s2.resize(n1 * m->g.ny * m->nlm);
    s2g.resize(ng1 * m->lev[kg].g.ny * m->nlm);
    if ((r = download_g(m, m->f[MSOMN_S2], m->g, m->nlm, s2.data())) || (r = download_g(m, m->lev[kg].S2, m->lev[kg].g, m->nlm, s2g.data()))) return r;
  }
  const int N = m->N, px = m->px, py = m->py, rank = m->rank;
  auto L2 = [&](int k, int i, int j, bool local) {
    if (p.fac_filt_Rd > 0) {
      const double s = local ? s2[((size_t)j << k) * n1 + ((size_t)i << k)] : s2g[((size_t)j << (k - kg)) * ng1 + ((size_t)i << (k - kg))];
      return fmin(p.fac_filt_Rd * p.dh[0] / sqrt(s), p.Lfmax);
    }
    const int J = local ? ntile_level(N, px, py, rank, k).oy + j : j;
    const double Delta = p.L0 / (N >> k);
    return p.Lfmax + (J * Delta / p.L0) * (p.Lfmin - p.Lfmax);
  };
  if ((r = ct_build_sig(m, y, L2, false))) return r;
  // mask_c: cell average of the tile's vertex mask, restricted on the tile, gathered at level kg, restricted on from there
  launch_wv_vert2cell(m->st, m->f[MSOMN_MASK], m->g, m->wmc[0], m->wg[0], 1);
  for (int k = 1; k < kg; k++) launch_wv_restrict(m->st, m->wmc[k - 1], m->wg[k - 1], m->wmc[k], m->wg[k], 1);
  launch_wv_restrict(m->st, m->wmc[kg - 1], m->wg[kg - 1], y.P.s, y.P.g, 1);
  if ((r = ct_gather(m, y.P.s, y.P.g, 1, m->wmc[kg], m->wg[kg]))) return r;
  for (int k = kg + 1; k < (int)m->wg.size(); k++) launch_wv_restrict(m->st, m->wmc[k - 1], m->wg[k - 1], m->wmc[k], m->wg[k], 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(m->st));
  m->wv_ready = 1;
  return MSOM_OK;
}
