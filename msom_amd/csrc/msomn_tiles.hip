// msomn_tiles.hip -- the vertex model on tiles: decomposition of a handle, halo exchange, reductions and the gather of the coarse
// levels over the transport of comm.hip ("Vertex model on tiles").  Index arithmetic: node_tile_inl.h.
//
// A tile HOLDS the vertices on its interior edges; every holder of a shared vertex computes it with the same device functions on the
// same operand values, so the tiled result equals the single tile's bit for bit.  The halo of a field is the neighbour's first inner
// column or row; everything runs on the handle's one stream.
#include "msomn_host.h"

NatGeom node_geom_rect(int tx, int ty) {
  NatGeom g;
  g.nx = tx + 1; g.ny = ty + 1;
  g.pitch = ((tx + 1 + 15) / 16) * 16 + 2 * MSOM_XP;
  g.rows = ty + 1 + 2 * MSOM_YP;
  g.ls = (size_t)g.pitch * g.rows;
  return g;
}
// x-parity split rows [even-i half | odd-i half]: tx / 2 + 1 and tx / 2 vertices, one pad slot at least after each half (the halo
// columns i = -1 and i = tx + 1 land there)
NatGeom node_geom_split_rect(int tx, int ty) {
  NatGeom g;
  g.nx = tx + 1; g.ny = ty + 1;
  const int hp = ((tx / 2 + 2 + 15) / 16) * 16;
  g.pitch = 2 * hp + 2 * MSOM_XP;
  g.rows = ty + 1 + 2 * MSOM_YP;
  g.ls = (size_t)g.pitch * g.rows;
  return g;
}

int nt_refuse(const msomn *m, const char *call) {
  if (!m || m->ntiles == 1) return MSOM_OK;
  msom_set_error("%s is not available on a tiled vertex-grid handle (%d x %d tiles)", call, m->px, m->py);
  return MSOM_ERR_CONFIG;
}

int nt_io_refuse(const msomn *m, const char *call) { return m && m->io_tiles ? MSOM_OK : nt_refuse(m, call); }

int nt_agree(msomn *m, int r, const char *call) {
  if (m->ntiles == 1) return r;
  const double mine = (double)r;   // the codes are <= 0: the minimum is the gravest
  HIPCHK(hipMemcpyAsync(m->d_scal + NSC_RES, &mine, sizeof mine, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  if (int rr = nt_reduce(m, NSC_RES, 1, RED_MIN)) return rr;
  const int all = (int)m->h_scal[NSC_RES];
  if (all && !r) msom_set_error("%s: another rank refuses (error %d): nothing was changed here", call, all);
  return all;
}

NodeOwned nt_owned(const msomn *m, const NatGeom &g, int cells, int rank) {
  const NodeTile t = ntile_level(m->N, m->px, m->py, rank, 0);
  const NodeRange w = ntile_owned_range(m->N, m->px, m->py, rank, 0);
  NodeOwned o;
  o.g = g; o.ox = t.ox; o.oy = t.oy;
  o.g.nx = cells ? t.tx : w.i1 + 1; o.g.ny = cells ? t.ty : w.j1 + 1;
  o.gn = cells ? m->N : m->N + 1;
  return o;
}

int nt_gather_owned(msomn *m, const double *dev, const NatGeom &g, int layers, int cells, unsigned long long *digest, std::vector<double> &out) {
  const NodeOwned o = nt_owned(m, g, cells, m->rank);
  const NodeTile t = ntile_level(m->N, m->px, m->py, m->rank, 0);
  // every rank sends as much as the largest owned window takes
  const size_t per = (size_t)(t.tx + 1) * (t.ty + 1), cnt = (size_t)layers * per, own = (size_t)o.g.nx * o.g.ny;
  struct Bufs { double *send = nullptr, *recv = nullptr; ~Bufs() { if (send) (void)hipFree(send); if (recv) (void)hipFree(recv); } } b;
  HIPCHK(hipMalloc(&b.send, cnt * sizeof(double)));
  HIPCHK(hipMemsetAsync(b.send, 0, cnt * sizeof(double), m->st));
  if (m->ntiles > 1) HIPCHK(hipMalloc(&b.recv, cnt * m->ntiles * sizeof(double)));
  for (int l = 0; l < layers; l++) {
    StateChunk c;
    c.g = o.g; c.ring = 0; c.layer = l; c.y0 = o.oy; c.rows = o.g.ny; c.ox = o.ox; c.oy = o.oy; c.gW = c.gH = o.gn; c.sx0 = o.ox; c.sw = o.g.nx;
    launch_state_pack(m->st, dev, b.send + (size_t)l * own, c, digest);
  }
  HIPCHK(hipGetLastError());
  int r = m->ntiles > 1 ? comm_allgather(m->comm, b.send, b.recv, cnt) : MSOM_OK;
  if (r) return r;
  out.clear();
  if (m->rank != 0) { HIPCHK(hipStreamSynchronize(m->st)); return MSOM_OK; }
  std::vector<double> h(cnt * m->ntiles);
  HIPCHK(hipMemcpyAsync(h.data(), m->ntiles > 1 ? b.recv : b.send, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  const size_t gn = (size_t)o.gn;
  out.resize((size_t)layers * gn * gn);
  for (int q = 0; q < m->ntiles; q++) {
    const NodeOwned oq = nt_owned(m, g, cells, q);
    const size_t w = (size_t)oq.g.nx, hh = (size_t)oq.g.ny;
    for (int l = 0; l < layers; l++)
      for (size_t j = 0; j < hh; j++)
        memcpy(&out[((size_t)l * gn + oq.oy + j) * gn + oq.ox], &h[q * cnt + ((size_t)l * hh + j) * w], w * sizeof(double));
  }
  return MSOM_OK;
}

int nt_setup(msomn *m, int px, int py, int rank, const void *id128) {
  const NodeTile t = ntile_level(m->N, px, py, rank, 0);
  m->px = px; m->py = py; m->rank = rank; m->ntiles = px * py;
  m->walls = t.walls; m->ox = t.ox; m->oy = t.oy;
  m->g = node_geom_rect(t.tx, t.ty);
  if (m->ntiles == 1) return MSOM_OK;
  m->nb[DIR_W] = ntile_neighbour(px, py, rank, -1, 0); m->nb[DIR_E] = ntile_neighbour(px, py, rank, 1, 0);
  m->nb[DIR_S] = ntile_neighbour(px, py, rank, 0, -1); m->nb[DIR_N] = ntile_neighbour(px, py, rank, 0, 1);
  // the passes that reach across more than one half-sweep, or fuse a pass with its neighbour in the cycle, have no tiled form yet:
  // they resolve to off (msomn_set_option keeps them there, msomn_get_param shows it)
  m->node_pfused = m->node_tile_s = m->node_march_s = m->node_march = m->tiled_relax = m->node_corr_fused = m->node_rhs_fused = 0;
  // a halo message: one column or one row with both halo columns, every layer
  const size_t longest = (size_t)(m->g.nx > m->g.ny ? m->g.nx : m->g.ny) + 2;
  return comm_create(&m->comm, rank, m->ntiles, id128, m->st, longest * (m->nl > m->nlm ? m->nl : m->nlm));
}
void nt_free_gather(msomn *m) {
  NLevel &P = m->piece;
  for (double **q : {&P.da, &P.da2, &P.res, &P.mask, &P.S2}) { if (*q) (void)hipFree(*q); *q = nullptr; }
  if (m->gsend) (void)hipFree(m->gsend);
  if (m->grecv) (void)hipFree(m->grecv);
  m->gsend = m->grecv = nullptr;
  m->gcount = 0;
}
void nt_free(msomn *m) {
  nt_free_gather(m);
  if (m->comm) comm_destroy(m->comm);
  m->comm = nullptr;
}

int nt_exchange(msomn *m, double *f, const NatGeom &g, int sp, int nl) {
  if (m->ntiles == 1) return MSOM_OK;
  Comm *c = m->comm;
  if ((size_t)nl * ((g.nx > g.ny ? g.nx : g.ny) + 2) > comm_bufcount(c)) {
    msom_set_error("halo message of %d layers of a %d x %d tile exceeds the communication buffers (%zu)", nl, g.nx, g.ny, comm_bufcount(c));
    return MSOM_ERR_ARG;
  }
  // every rank posts both phases, with no message where it has a wall: the in-process transport meets in a barrier
  Xfer x[2];
  int n = 0, r;
  for (int dir : {DIR_W, DIR_E}) {   // my first inner column is the neighbour's halo
    if (m->nb[dir] < 0) continue;
    launch_n_pack_strip(m->st, f, g, sp, nl, dir == DIR_W ? 1 : g.nx - 2, 0, 1, g.ny, comm_sendbuf(c, dir));
    x[n++] = {m->nb[dir], dir, comm_sendbuf(c, dir), comm_recvbuf(c, dir), (size_t)g.ny * nl};
  }
  if ((r = comm_exchange(c, x, n))) return r;
  for (int dir : {DIR_W, DIR_E})
    if (m->nb[dir] >= 0) launch_n_unpack_strip(m->st, f, g, sp, nl, dir == DIR_W ? -1 : g.nx, 0, 1, g.ny, comm_recvbuf(c, dir));
  n = 0;
  const int w = g.nx + 2;            // rows travel with their halo columns (beyond a wall: the pad, 0 on both sides): the corners
  for (int dir : {DIR_S, DIR_N}) {
    if (m->nb[dir] < 0) continue;
    launch_n_pack_strip(m->st, f, g, sp, nl, -1, dir == DIR_S ? 1 : g.ny - 2, w, 1, comm_sendbuf(c, dir));
    x[n++] = {m->nb[dir], dir, comm_sendbuf(c, dir), comm_recvbuf(c, dir), (size_t)w * nl};
  }
  if ((r = comm_exchange(c, x, n))) return r;
  for (int dir : {DIR_S, DIR_N})
    if (m->nb[dir] >= 0) launch_n_unpack_strip(m->st, f, g, sp, nl, -1, dir == DIR_S ? -1 : g.ny, w, 1, comm_recvbuf(c, dir));
  HIPCHK(hipGetLastError());
  m->nexch++;
  return MSOM_OK;
}

int nt_reduce(msomn *m, int slot, int n, int op) {
  if (m->ntiles > 1) return comm_allreduce(m->comm, m->d_scal + slot, m->h_scal + slot, n, op);
  HIPCHK(hipMemcpyAsync(m->h_scal + slot, m->d_scal + slot, n * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

int nt_gather(msomn *m, const double *piece, const NatGeom &pg, int nl, double *global, const NatGeom &gg) {
  const size_t count = (size_t)nl * pg.nx * pg.ny;
  if (count > m->gcount) { msom_set_error("gather of %zu doubles exceeds its buffer (%zu)", count, m->gcount); return MSOM_ERR_ARG; }
  launch_n_pack_strip(m->st, piece, pg, 0, nl, 0, 0, pg.nx, pg.ny, m->gsend);
  int r = comm_allgather(m->comm, m->gsend, m->grecv, count);
  if (r) return r;
  launch_n_assemble(m->st, m->grecv, global, gg, nl, m->N, m->px, m->py, m->kg);
  HIPCHK(hipGetLastError());
  return MSOM_OK;
}

extern "C" int msomn_tile_info(msomn_t *m, int *px, int *py, int *ix, int *iy, int *nx_local, int *ny_local) {
  if (!m) return MSOM_ERR_ARG;
  if (px) *px = m->px;
  if (py) *py = m->py;
  if (ix) *ix = m->rank % m->px;
  if (iy) *iy = m->rank / m->px;
  if (nx_local) *nx_local = m->g.nx;
  if (ny_local) *ny_local = m->g.ny;
  return MSOM_OK;
}
