// msomn_stats.hip -- running time means and eddy statistics of the vertex-grid model on the device (msomn_stats_*, include/msom.h;
// DESIGN section 8j).  The twin of the msom_stats_* block of msom_diag.hip on the vertices a handle or a tile holds; kernels:
// kernels_node_stats.hip.  The automatic sample is queued by msomn_step (msom_node.hip) through nstats_sample.
#include <cmath>

#include "msomn_host.h"

void nstats_drop(msomn *m) {
  for (int k = 0; k < MSOM_ST_NACC; k++) {
    if (m->stats.s[k]) (void)hipFree(m->stats.s[k]);
    m->stats.s[k] = nullptr;
  }
  if (m->stats_scr) (void)hipFree(m->stats_scr);
  m->stats_scr = nullptr;
  m->stats_mask = 0;
  m->stats_W = 0.;
  m->stats_count = m->stats_samples = 0;
}
static NStatsTile stats_tile(const msomn *m) { return NStatsTile{m->ox, m->oy, m->N}; }
int nstats_sample(msomn *m, double w) {
  if (launch_n_stats_acc(m->st, m->stats_mask, m->f[MSOMN_PSI], m->f[MSOMN_Q], m->f[MSOMN_MASK], m->stats, m->g, m->nl, stats_tile(m), w, 2. * m->D)) {
    msom_set_error("no k_n_stats_acc for mask 0x%x", m->stats_mask);
    return MSOM_ERR_ARG;
  }
  HIPCHK(hipGetLastError());
  m->stats_W = m->stats_W + w;
  m->stats_samples++;
  return MSOM_OK;
}
#define NEED_NSTATS(m, fn)                                                                  \
  do {                                                                                      \
    if (!(m)->const_set || !(m)->stats_mask) {                                              \
      msom_set_error(fn ": no msomn_stats_begin since msomn_set_const");                    \
      return MSOM_ERR_STATE;                                                                \
    }                                                                                       \
  } while (0)

extern "C" int msomn_stats_begin(msomn_t *m, unsigned mask) {
  if (!m) return MSOM_ERR_ARG;
  if (mask == 0 || mask >> MSOM_ST_NACC) { msom_set_error("msomn_stats_begin: mask 0x%x", mask); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msomn_stats_begin before msomn_set_const"); return MSOM_ERR_STATE; }
  HIPCHK(hipStreamSynchronize(m->st));   // a sample of an earlier mask may still be running
  const size_t bytes = m->g.ls * m->nl * sizeof(double);
  for (int k = 0; k < MSOM_ST_NACC; k++) {
    const bool want = (mask >> k) & 1u;
    if (!want && m->stats.s[k]) { HIPCHK(hipFree(m->stats.s[k])); m->stats.s[k] = nullptr; }
    if (want && !m->stats.s[k]) HIPCHK(hipMalloc(&m->stats.s[k], bytes));
    if (want) HIPCHK(hipMemsetAsync(m->stats.s[k], 0, bytes, m->st));
  }
  m->stats_mask = mask;
  m->stats_W = 0.;
  m->stats_count = m->stats_samples = 0;
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

extern "C" int msomn_stats_accumulate(msomn_t *m, double w) {
  if (!m) return MSOM_ERR_ARG;
  if (!std::isfinite(w)) { msom_set_error("msomn_stats_accumulate: w = %g", w); return MSOM_ERR_ARG; }
  NEED_NSTATS(m, "msomn_stats_accumulate");
  // tiles: psi may have been set or solved since its last exchange; the differences read it across the tile edges (collective)
  int r = nt_exchange(m, m->f[MSOMN_PSI], m->g, 0, m->nl);
  return r ? r : nstats_sample(m, w);
}

extern "C" int msomn_stats_weight(msomn_t *m, double *W) {
  if (!m || !W) return MSOM_ERR_ARG;
  NEED_NSTATS(m, "msomn_stats_weight");
  *W = m->stats_W;
  return MSOM_OK;
}

extern "C" int msomn_stats_get(msomn_t *m, int which, double *out) {
  if (!m || !out) return MSOM_ERR_ARG;
  unsigned need;
  int sa = -1;
  if (which >= 0 && which < MSOM_ST_NACC) need = 1u << which;
  else if (which == MSOM_ST_EKE) need = 1u << MSOM_ST_PSI | 1u << (sa = MSOM_ST_KE);
  else if (which == MSOM_ST_UQ_EDDY) need = 1u << MSOM_ST_PSI | 1u << MSOM_ST_Q | 1u << (sa = MSOM_ST_UQ);
  else if (which == MSOM_ST_VQ_EDDY) need = 1u << MSOM_ST_PSI | 1u << MSOM_ST_Q | 1u << (sa = MSOM_ST_VQ);
  else { msom_set_error("msomn_stats_get: unknown id %d (the vertex model's running mean is psi_f: MSOM_ST_QME is not offered)", which); return MSOM_ERR_ARG; }
  NEED_NSTATS(m, "msomn_stats_get");
  if ((m->stats_mask & need) != need) { msom_set_error("msomn_stats_get: id %d needs accumulators 0x%x, the mask is 0x%x", which, need, m->stats_mask); return MSOM_ERR_ARG; }
  const double W = m->stats_W;
  if (W == 0) { msom_set_error("msomn_stats_get: the sum of the weights is 0"); return MSOM_ERR_STATE; }
  // the mean goes into the scratch field MSOMN_TMP (layers of psi; the tendency rewrites it before it reads it)
  double *tmp = m->f[MSOMN_TMP];
  launch_n_stats_mean(m->st, tmp, m->stats.s[sa < 0 ? which : MSOM_ST_PSI], W, m->g, m->nl);
  HIPCHK(hipGetLastError());
  if (sa < 0) return download_g(m, tmp, m->g, m->nl, out);
  // boundary(psi) on the copy of the mean psi, then its halo: the one collective step of the derived ids
  launch_n_bnd_const(m->st, tmp, m->g, m->nl, m->psi_bc, 0, m->walls);
  int r = nt_exchange(m, tmp, m->g, 0, m->nl);
  if (r) return r;
  if (!m->stats_scr) HIPCHK(hipMalloc(&m->stats_scr, m->g.ls * m->nl * sizeof(double)));
  launch_n_stats_derive(m->st, m->stats_scr, tmp, m->f[MSOMN_MASK], m->stats.s[sa], m->stats.s[MSOM_ST_Q], W, m->g, m->nl, which, stats_tile(m),
                        2. * m->D);
  HIPCHK(hipGetLastError());
  return download_g(m, m->stats_scr, m->g, m->nl, out);
}
