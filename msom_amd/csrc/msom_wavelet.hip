// msom_wavelet.hip -- wavelet scale filter (msqg/qg.h:509-560, its coefficients :1059-1090), the energy / PV budgets
// (msqg/qg_energy.h, pystep_de :296-349) and their msom_dbg_wavelet_* hooks.
#include "msom_host.h"

// ------------------------------------------------------------------ wavelet scale filter (msqg/qg.h:509-560)

// pyramid geometry + filter coefficients sig_lev (set_const, msqg/qg.h:1059-1090): init-time host pass
// all-gather of a small tile block [nlay][ny][nx] (host in / host out: [rank][nlay][ny][nx]) through the communicator
static int wv_gather(msom *m, const std::vector<double> &mine, std::vector<double> &all) {
  const size_t cnt = mine.size();
  all.resize(cnt * m->nranks);
  HIPCHK(hipMemcpyAsync(m->wv_gsend, mine.data(), cnt * sizeof(double), hipMemcpyHostToDevice, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  comm_begin(m);
  int r = comm_allgather(m->comm, m->wv_gsend, m->wv_grecv, cnt);
  comm_end(m);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(all.data(), m->wv_grecv, cnt * m->nranks * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}
// gathered tile blocks -> one global array [nlay][gy][gx]
static void wv_assemble(const msom *m, const std::vector<double> &all, int nlay, int bx, int by, std::vector<double> &out) {
  const int gx = bx * m->px, gy = by * m->py;
  out.assign((size_t)nlay * gx * gy, 0.);
  for (int r = 0; r < m->nranks; r++) {
    const int ox = (r % m->px) * bx, oy = (r / m->px) * by;
    for (int l = 0; l < nlay; l++)
      for (int j = 0; j < by; j++)
        for (int i = 0; i < bx; i++) out[((size_t)l * gy + oy + j) * gx + ox + i] = all[(size_t)r * nlay * bx * by + ((size_t)l * by + j) * bx + i];
  }
}
// pyramid geometry + filter coefficients sig_lev (set_const, msqg/qg.h:1059-1090): init-time host pass
static int wavelet_setup(msom *m) {
  if (m->wv_ready) return MSOM_OK;
  const Params &p = m->p;
  int r;
  const bool tiled = m->nranks > 1;
  if (m->wv_nlev == 0) {
    int n = 1;   // Basilisk levels depth() ... 0 of the GLOBAL grid
    while ((m->gnx >> n) >= 1 && (m->gny >> n) >= 1 && ((m->gnx >> n) << n) == m->gnx && ((m->gny >> n) << n) == m->gny) n++;
    m->wv_nlev = n;
    int kt = 0;  // coarsest level that still has a cell of every tile
    while (kt + 1 < n && (m->nx >> (kt + 1)) >= 1 && (m->ny >> (kt + 1)) >= 1) kt++;
    m->wv_kt = tiled ? kt : n - 1;
    const int nt = m->wv_kt + 1;
    m->wv_g.resize(nt); m->wv_s.assign(nt, nullptr); m->wv_r.assign(nt, nullptr); m->wv_sig.assign(nt, nullptr);
    for (int k = 0; k < nt; k++) {
      m->wv_g[k] = make_nat(m->nx >> k, m->ny >> k);
      const size_t ls = m->wv_g[k].ls;
      HIPCHK(hipMalloc(&m->wv_sig[k], ls * sizeof(double)));
      HIPCHK(hipMemsetAsync(m->wv_sig[k], 0, ls * sizeof(double), m->st));
      if (k == 0) continue;  // level 0 works in place on the field
      HIPCHK(hipMalloc(&m->wv_s[k], ls * m->nl * sizeof(double)));
      HIPCHK(hipMalloc(&m->wv_r[k], ls * m->nl * sizeof(double)));
      HIPCHK(hipMemsetAsync(m->wv_s[k], 0, ls * m->nl * sizeof(double), m->st));
      HIPCHK(hipMemsetAsync(m->wv_r[k], 0, ls * m->nl * sizeof(double), m->st));
    }
    if (tiled) {
      const size_t blk = (size_t)(m->nx >> kt) * (m->ny >> kt) * (m->nl > 2 ? m->nl : 2);
      HIPCHK(hipMalloc(&m->wv_gsend, blk * sizeof(double)));
      HIPCHK(hipMalloc(&m->wv_grecv, blk * m->nranks * sizeof(double)));
      m->wv_gx = (m->nx >> kt) * m->px; m->wv_gy = (m->ny >> kt) * m->py;
    }
  }
  const int K = m->wv_kt + 1;   // levels on the tile
  std::vector<std::vector<double>> sf(K), sl(K);
  sf[0].resize((size_t)m->nx * m->ny);
  HIPCHK(hipStreamSynchronize(m->st));
  launch_unpack(m->st, m->f[MSOM_RD], m->staging, m->g, 1);
  HIPCHK(hipMemcpyAsync(sf[0].data(), m->staging, sf[0].size() * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  for (double &v : sf[0]) v = fmin(p.afilt * v, p.Lfmax);  // sig_filt = min(afilt * Rd, Lfmax) :1060
  auto restrict_host = [](const std::vector<double> &f, int nx, int ny, std::vector<double> &c) {  // restriction({sig_filt}) :1063
    const int fx = nx * 2;
    c.resize((size_t)nx * ny);
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        double sum = 0.;
        sum += f[(size_t)(2 * j) * fx + 2 * i]; sum += f[(size_t)(2 * j + 1) * fx + 2 * i];
        sum += f[(size_t)(2 * j) * fx + 2 * i + 1]; sum += f[(size_t)(2 * j + 1) * fx + 2 * i + 1];
        c[(size_t)j * nx + i] = sum / 4;
      }
  };
  auto lowpass_host = [&](const std::vector<double> &sfk, const std::vector<double> *child, int nx, int ny, int k, std::vector<double> &out) {  // :1066-1083
    const int fx = nx * 2;
    const double Delta = p.L0 / (double)(m->gnx >> k);
    out.resize((size_t)nx * ny);
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        double ref_flag = 0;
        if (child) {
          ref_flag += (*child)[(size_t)(2 * j) * fx + 2 * i]; ref_flag += (*child)[(size_t)(2 * j + 1) * fx + 2 * i];
          ref_flag += (*child)[(size_t)(2 * j) * fx + 2 * i + 1]; ref_flag += (*child)[(size_t)(2 * j + 1) * fx + 2 * i + 1];
        }
        const double sv = sfk[(size_t)j * nx + i];
        double v;
        if (ref_flag > 0) v = 1;
        else if (sv > 2 * Delta) v = 0;
        else if (sv <= 2 * Delta && sv > Delta) v = 1 - (sv - Delta) / Delta;
        else v = 1;
        out[(size_t)j * nx + i] = v;
      }
  };
  for (int k = 1; k < K; k++) restrict_host(sf[k - 1], m->nx >> k, m->ny >> k, sf[k]);
  for (int k = 0; k < K; k++) lowpass_host(sf[k], k > 0 ? &sl[k - 1] : nullptr, m->nx >> k, m->ny >> k, k, sl[k]);
  if (tiled) {  // the levels above the tiles: gathered sig_filt and low-pass flags of level kt, continued on the global top grid
    const int kt = m->wv_kt, bx = m->nx >> kt, by = m->ny >> kt;
    std::vector<double> mine((size_t)2 * bx * by), all, top;
    std::copy(sf[kt].begin(), sf[kt].end(), mine.begin());
    std::copy(sl[kt].begin(), sl[kt].end(), mine.begin() + (size_t)bx * by);
    if ((r = wv_gather(m, mine, all))) return r;
    wv_assemble(m, all, 2, bx, by, top);
    int gx = m->wv_gx, gy = m->wv_gy;
    std::vector<double> tsf(top.begin(), top.begin() + (size_t)gx * gy), tsl(top.begin() + (size_t)gx * gy, top.end());
    m->wv_top_sig.assign(m->wv_nlev - kt, std::vector<double>());
    m->wv_top_sig[0] = tsl;
    for (int k = kt + 1; k < m->wv_nlev; k++) {
      std::vector<double> csf, csl;
      gx >>= 1; gy >>= 1;
      restrict_host(tsf, gx, gy, csf);
      lowpass_host(csf, &tsl, gx, gy, k, csl);
      m->wv_top_sig[k - kt] = csl;
      tsf.swap(csf); tsl.swap(csl);
    }
    for (auto &v : m->wv_top_sig) for (double &q : v) q = 1 - q;   // high pass :1086-1090
  }
  for (int k = 0; k < K; k++) {  // high pass :1086-1090, then to the device
    for (double &v : sl[k]) v = 1 - v;
    const NatGeom &g = m->wv_g[k];
    HIPCHK(hipMemcpy2DAsync(m->wv_sig[k] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), sl[k].data(), g.nx * sizeof(double), g.nx * sizeof(double), g.ny,
                            hipMemcpyHostToDevice, m->st));
  }
  HIPCHK(hipStreamSynchronize(m->st));
  m->wv_ready = 1;
  return MSOM_OK;
}
static void wv_fill(msom *m, double *f, const NatGeom &g) {
  if (m->nranks > 1) { STICKY(m, exch_nat_g(m, f, g, m->nl, m->bc, 1)); return; }
  if (m->bc == BC_PERIODIC) launch_fill_periodic(m->st, f, g, m->nl, 1);
  else launch_fill_ghost(m->st, f, g, m->nl, m->bc, m->walls);
}
// host arrays of the gathered top levels: [nl][gy + 2][gx + 2] with a ghost ring filled like boundary() does
struct WvTop {
  int gx, gy, nl;
  std::vector<double> v;
  double &at(int l, int j, int i) { return v[((size_t)l * (gy + 2) + (j + 1)) * (gx + 2) + (i + 1)]; }
  void init(int gx_, int gy_, int nl_) { gx = gx_; gy = gy_; nl = nl_; v.assign((size_t)nl * (gx + 2) * (gy + 2), 0.); }
  void fill(int bc) {  // x sides first, then y over the x-ghost columns (corners = y rule of the x ghost)
    for (int l = 0; l < nl; l++) {
      for (int j = 0; j < gy; j++) {
        if (bc == BC_PERIODIC) { at(l, j, -1) = at(l, j, gx - 1); at(l, j, gx) = at(l, j, 0); }
        else if (bc == BC_NEUMANN) { at(l, j, -1) = at(l, j, 0); at(l, j, gx) = at(l, j, gx - 1); }
        else { at(l, j, -1) = -at(l, j, 0); at(l, j, gx) = -at(l, j, gx - 1); }
      }
      for (int i = -1; i <= gx; i++) {
        if (bc == BC_PERIODIC) { at(l, -1, i) = at(l, gy - 1, i); at(l, gy, i) = at(l, 0, i); }
        else if (bc == BC_NEUMANN) { at(l, -1, i) = at(l, 0, i); at(l, gy, i) = at(l, gy - 1, i); }
        else { at(l, -1, i) = -at(l, 0, i); at(l, gy, i) = -at(l, gy - 1, i); }
      }
    }
  }
  double bilin(int l, int i, int j) {  // fine cell (i, j) of the next finer level from this one, as k_wv_recon's bilin()
    const int I = i >> 1, J = j >> 1, cx = (i & 1) ? 1 : -1, cy = (j & 1) ? 1 : -1;
    return (9. * at(l, J, I) + 3. * (at(l, J, I + cx) + at(l, J + cy, I)) + at(l, J + cy, I + cx)) / 16.;
  }
};
// field <- inverse_wavelet(sig_lev * wavelet(field)), all layers (msqg/qg.h:524-539)
static int wavelet_apply(msom *m, double *f) {
  m->res_ready = -1;
  int r = wavelet_setup(m);
  if (r) return r;
  const int K = m->wv_kt + 1, nl = m->nl;   // levels on the tile (all of them on a single tile)
  const bool tiled = m->nranks > 1;
  wv_fill(m, f, m->g);
  for (int k = 1; k < K; k++) {
    launch_wv_restrict(m->st, k == 1 ? f : m->wv_s[k - 1], m->wv_g[k - 1], m->wv_s[k], m->wv_g[k], nl);
    wv_fill(m, m->wv_s[k], m->wv_g[k]);
  }
  if (!tiled) {
    if (K == 1) launch_wv_root(m->st, f, m->wv_sig[0], f, m->g, nl);
    else launch_wv_root(m->st, m->wv_s[K - 1], m->wv_sig[K - 1], m->wv_r[K - 1], m->wv_g[K - 1], nl);
    if (K > 1) wv_fill(m, m->wv_r[K - 1], m->wv_g[K - 1]);
  } else {
    // levels kt .. depth 0 on the gathered top grid, on the host (a few cells), every rank the same arithmetic as the kernels:
    // s_k+1 = mean of the 4 children, w = (s - bilinear(s coarse)) sig, r = bilinear(r coarse) + w, root r = s sig
    // a recorded error of THIS rank must not keep it out of the collective below (the other ranks would wait in it):
    // gather first (whatever the block holds), report afterwards
    const int sticky_before = m->sticky;
    const int kt = m->wv_kt, bx = m->nx >> kt, by = m->ny >> kt, nt = m->wv_nlev - kt;
    const NatGeom &gk = m->wv_g[kt];
    const double *src = kt == 0 ? f : m->wv_s[kt];
    std::vector<double> mine((size_t)nl * bx * by), all, top;
    for (int l = 0; l < nl; l++)
      HIPCHK(hipMemcpy2DAsync(mine.data() + (size_t)l * bx * by, bx * sizeof(double), src + nat_idx(gk, l, 0, 0), gk.pitch * sizeof(double), bx * sizeof(double), by,
                              hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    if ((r = wv_gather(m, mine, all))) return r;
    if (sticky_before) return sticky_before;
    wv_assemble(m, all, nl, bx, by, top);
    std::vector<WvTop> S(nt), R(nt);
    int gx = m->wv_gx, gy = m->wv_gy;
    S[0].init(gx, gy, nl);
    for (int l = 0; l < nl; l++) for (int j = 0; j < gy; j++) for (int i = 0; i < gx; i++) S[0].at(l, j, i) = top[((size_t)l * gy + j) * gx + i];
    S[0].fill(m->bc);
    for (int q = 1; q < nt; q++) {
      S[q].init(S[q - 1].gx >> 1, S[q - 1].gy >> 1, nl);
      for (int l = 0; l < nl; l++) for (int j = 0; j < S[q].gy; j++) for (int i = 0; i < S[q].gx; i++) {
        double sum = 0.;
        sum += S[q - 1].at(l, 2 * j, 2 * i); sum += S[q - 1].at(l, 2 * j + 1, 2 * i); sum += S[q - 1].at(l, 2 * j, 2 * i + 1); sum += S[q - 1].at(l, 2 * j + 1, 2 * i + 1);
        S[q].at(l, j, i) = sum / 4;
      }
      S[q].fill(m->bc);
    }
    R[nt - 1].init(S[nt - 1].gx, S[nt - 1].gy, nl);
    for (int l = 0; l < nl; l++) for (int j = 0; j < R[nt - 1].gy; j++) for (int i = 0; i < R[nt - 1].gx; i++)
      R[nt - 1].at(l, j, i) = S[nt - 1].at(l, j, i) * m->wv_top_sig[nt - 1][(size_t)j * R[nt - 1].gx + i];
    R[nt - 1].fill(m->bc);
    for (int q = nt - 2; q >= 0; q--) {
      R[q].init(S[q].gx, S[q].gy, nl);
      for (int l = 0; l < nl; l++) for (int j = 0; j < R[q].gy; j++) for (int i = 0; i < R[q].gx; i++) {
        double d = S[q].at(l, j, i);
        d -= S[q + 1].bilin(l, i, j);
        const double w = d * m->wv_top_sig[q][(size_t)j * R[q].gx + i];
        double rr = R[q + 1].bilin(l, i, j);
        rr += w;
        R[q].at(l, j, i) = rr;
      }
      R[q].fill(m->bc);
    }
    // this tile's block of the filtered level kt, with its ring (neighbour cells or wall ghosts), back to the device
    double *dst = kt == 0 ? f : m->wv_r[kt];
    std::vector<double> blk((size_t)nl * (bx + 2) * (by + 2));
    for (int l = 0; l < nl; l++) for (int j = -1; j <= by; j++) for (int i = -1; i <= bx; i++)
      blk[((size_t)l * (by + 2) + j + 1) * (bx + 2) + i + 1] = R[0].at(l, m->iy * by + j, m->ix * bx + i);
    for (int l = 0; l < nl; l++)
      HIPCHK(hipMemcpy2DAsync(dst + nat_idx(gk, l, -1, -1), gk.pitch * sizeof(double), blk.data() + (size_t)l * (bx + 2) * (by + 2), (bx + 2) * sizeof(double),
                              (bx + 2) * sizeof(double), by + 2, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
  }
  for (int k = K - 2; k >= 0; k--) {
    double *s = k == 0 ? f : m->wv_s[k], *out = k == 0 ? f : m->wv_r[k];
    launch_wv_recon(m->st, s, m->wv_s[k + 1], m->wv_r[k + 1], m->wv_sig[k], out, m->wv_g[k], m->wv_g[k + 1], nl);
    wv_fill(m, out, m->wv_g[k]);
  }
  HIPCHK(hipGetLastError());
  return m->sticky;
}
static int wavelet_filter(msom *m, int qof_field, double dtflt) {
  NEED_CONST(m);
  int r;
  if ((r = wavelet_setup(m)) || (r = ensure_field(m, qof_field))) return r;
  const int nl = m->nl;
  // tmp = q (interior; the saved copy is restored into q when dtflt < 0)
  HIPCHK(hipMemcpyAsync(m->f[MSOM_TMP], m->f[MSOM_Q], m->g.ls * nl * sizeof(double), hipMemcpyDeviceToDevice, m->st));
  if ((r = invertq(m, m->f[MSOM_Q]))) return r;
  if ((r = wavelet_apply(m, m->f[MSOM_PSI]))) return r;
  m->umax_ready = 0;
  comp_del2(m, MSOM_PSI, MSOM_Q, 0., 1.);
  comp_stretch(m, MSOM_PSI, MSOM_Q, 1., 1.);
  // `nbar` is a by-value argument in the reference (msqg/qg.h:510,558): the running mean never advances
  launch_wv_qof(m->st, m->f[qof_field], m->f[MSOM_Q], m->f[MSOM_TMP], m->g, nl, dtflt, 0, dtflt < 0.0);
  if (dtflt < 0.0) fill_bc(m, MSOM_Q);
  fill_bc(m, qof_field);
  return sync_stream(m);
}
extern "C" int msom_wavelet_filter(msom_t *m, double dtflt) {
  MSQG_ONLY(m);
  return wavelet_filter(m, MSOM_QOF, dtflt);
}

// ------------------------------------------------------------------ energy / PV budgets (msqg/qg_energy.h)

static int ensure_de_fields(msom *m) {
  for (int k = MSOM_DE_BF; k <= MSOM_PO_MFT; k++) {
    int r = ensure_field(m, k);
    if (r) return r;
  }
  return MSOM_OK;
}
// advection_de + dissip_de + ekman_friction_de on the current psi / zeta (energy_tend :229-232, pystep_de :327-329)
static int de_terms(msom *m, double dt, double ediag) {
  const Params &p = m->p;
  const int nl = m->nl;
  const double D = p.L0 / m->gnx;
  launch_advection_de(m->st, m->f[MSOM_ZETA], m->f[MSOM_PSI], m->f[MSOM_PSIPG], m->f[MSOM_ZETAPG], m->f[MSOM_S], m->f[MSOM_DE_J1], m->f[MSOM_DE_J2],
                      m->f[MSOM_DE_J3], m->g, nl, D, p.beta, dt, ediag, m->lc);
  comp_del2(m, MSOM_ZETA, MSOM_TMP, 0., 1.);
  comp_stretch(m, MSOM_ZETA, MSOM_TMP2, 0., 1.);
  launch_dissip_de(m->st, m->f[MSOM_TMP], m->f[MSOM_TMP2], m->f[MSOM_PSI], m->f[MSOM_DE_VD], m->g, nl, p.iRe, p.iRe4, dt, ediag, D, 0);
  comp_stretch(m, MSOM_TMP, MSOM_TMP2, 0., 1.);
  launch_dissip_de(m->st, m->f[MSOM_TMP], m->f[MSOM_TMP2], m->f[MSOM_PSI], m->f[MSOM_DE_VD], m->g, nl, p.iRe, p.iRe4, dt, ediag, D, 1);
  launch_ekman_de(m->st, m->f[MSOM_ZETA], m->f[MSOM_PSI], m->f[MSOM_DE_BF], m->g, nl, p.Eks / (p.Rom * 2 * m->dhf[0]),
                  p.Ekb / (p.Rom * 2 * m->dhf[nl - 1]), dt, ediag);
  HIPCHK(hipGetLastError());
  return m->sticky;
}
extern "C" int msom_energy_tend(msom_t *m, double dt) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  int r;
  if ((r = ensure_de_fields(m))) return r;
  comp_del2(m, MSOM_PSI, MSOM_ZETA, 0., 1.0);
  if ((r = de_terms(m, dt, (double)m->p.ediag))) return r;
  launch_running_mean(m->st, m->f[MSOM_PO_MFT], m->f[MSOM_PSI], m->g, m->nl, m->nme_ft);
  m->nme_ft += 1;
  return sync_stream(m);
}
int filter_de(msom *m, int pm_field, double dtflt, double ediag) {
  int r;
  if ((r = ensure_de_fields(m))) return r;
  if ((r = wavelet_filter(m, MSOM_TMP2, -dtflt))) return r;  // tmp2: tmp is used inside wavelet_filter (:210-213)
  launch_filter_de(m->st, m->f[MSOM_DE_FT], m->f[MSOM_TMP2], m->f[pm_field], m->g, m->nl, dtflt, ediag);
  if (pm_field == MSOM_PSI) m->psi_ghosts_stale = 1;   // pm[] = 0 in the cells only (msqg/qg_energy.h:223): pystep_de leaves psi like this
  m->nme_ft = 0;
  return sync_stream(m);
}
extern "C" int msom_filter_de(msom_t *m, int pm_field, double dtflt) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  if (pm_field < 0 || pm_field >= MSOM_NFIELDS || m->flayers[pm_field] != m->nl) { msom_set_error("bad field id %d", pm_field); return MSOM_ERR_ARG; }
  int r = ensure_field(m, pm_field);
  return r ? r : filter_de(m, pm_field, dtflt, (double)m->p.ediag);
}
extern "C" int msom_reset_de(msom_t *m) {
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  int r;
  if ((r = ensure_de_fields(m))) return r;
  for (int k = MSOM_DE_BF; k <= MSOM_DE_FT; k++) HIPCHK(hipMemsetAsync(m->f[k], 0, m->g.ls * m->nl * sizeof(double), m->st));
  return sync_stream(m);
}
// pystep_de, msqg/qg_energy.h:296-349 (SWIG: msqg/qg_energy.i:31; caller msqg/scripts/energy_offline.py:113).
// ediag = 1 and dt = 1 are locals of the reference routine; filter_de runs with po_mft = pol (so the
// stream function is zeroed on exit) and the global dtflt.
extern "C" int pystep_de(msom_t *m, const double *po_py, int len1, int len2, int len3, double *de_bf_py, int len4, int len5, int len6,
                         double *de_vd_py, int len7, int len8, int len9, double *de_j1_py, int len10, int len11, int len12,
                         double *de_j2_py, int len13, int len14, int len15, double *de_j3_py, int len16, int len17, int len18,
                         double *de_ft_py, int len19, int len20, int len21, int onlyKE) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  if (check_shape(m, len1, len2, len3) || check_shape(m, len4, len5, len6) || check_shape(m, len7, len8, len9) || check_shape(m, len10, len11, len12) ||
      check_shape(m, len13, len14, len15) || check_shape(m, len16, len17, len18) || check_shape(m, len19, len20, len21))
    return MSOM_ERR_ARG;
  if (!po_py) return MSOM_ERR_ARG;
  const double ediag = 1., dt = 1.;
  int r;
  if ((r = upload(m, MSOM_PSI, po_py)) || (r = msom_reset_de(m))) return r;
  m->umax_ready = 0;
  comp_del2(m, MSOM_PSI, MSOM_ZETA, 0., 1.0);
  comp_del2(m, MSOM_PSI, MSOM_Q, 0., 1.);
  comp_stretch(m, MSOM_PSI, MSOM_Q, 1., 1.);
  if (onlyKE == 1 && !m->s_zero) {  // :319-325 strl = 0 (stays so until the next set_const)
    m->s_zero = 1;
    if ((r = build_coefs(m))) return r;
  }
  if ((r = de_terms(m, dt, ediag)) || (r = filter_de(m, MSOM_PSI, m->p.dtflt, ediag))) return r;
  double *outs[6] = {de_bf_py, de_vd_py, de_j1_py, de_j2_py, de_j3_py, de_ft_py};
  for (int k = 0; k < 6; k++)
    if (outs[k] && (r = download(m, MSOM_DE_BF + k, outs[k]))) return r;
  return MSOM_OK;
}

extern "C" int msom_dbg_wavelet_levels(msom_t *m) {
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  int r = wavelet_setup(m);
  return r ? r : m->wv_nlev;
}
extern "C" int msom_dbg_siglev(msom_t *m, int level, double *out) {
  MSQG_ONLY(m);
  if (!m || !out) return MSOM_ERR_ARG;
  int r = wavelet_setup(m);
  if (r) return r;
  if (level < 0 || level >= (int)m->wv_g.size()) { msom_set_error("bad level %d (tiles: only the levels that live on the tile)", level); return MSOM_ERR_ARG; }
  const NatGeom &g = m->wv_g[level];
  HIPCHK(hipMemcpy2DAsync(out, g.nx * sizeof(double), m->wv_sig[level] + nat_idx(g, 0, 0, 0), g.pitch * sizeof(double), g.nx * sizeof(double), g.ny,
                          hipMemcpyDefault, m->st));
  return sync_stream(m);
}
extern "C" int msom_dbg_wavelet_apply(msom_t *m, int field) {
  MSQG_ONLY(m);
  NEED_CONST(m);
  if (field < 0 || field >= MSOM_NFIELDS || !m->f[field] || m->flayers[field] != m->nl) { msom_set_error("bad field id %d", field); return MSOM_ERR_ARG; }
  int r = wavelet_apply(m, m->f[field]);
  return r ? r : sync_stream(m);
}
