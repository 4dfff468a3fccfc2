// msom_helm.hip -- modal PV inversion (option mode_pv_invert): the per-mode Helmholtz multigrid behind invertq, and the one-problem
// solve of the newqg dialect.  Restates msqg/qg.h:116-157 (MODE_PV_INVERT) and mg_solve / mg_cycle of mspg/elliptic.h:43-99.
#include "msom_host.h"

// ------------------------------------------------------------------ modal PV inversion (MODE_PV_INVERT, msqg/qg.h:116-157)

void helm_drop_pyramid(msom *m) {   // the iBu pyramid of the modal inversion (general form)
  for (double *p : m->helm_ibu)
    if (p) hipFree(p);
  m->helm_ibu.clear();
}
int helm_partial_stride(const msom *m) { return helm_residual_blocks(m->g) + 64; }   // room for the chunk sums of launch_sum_final

// General form: iBu_m per cell on every multigrid level, the mean of the 4 children level by level (poisson()'s
// restriction({alpha, lambda})), in the split layout of the level.  Built at the first modal solve (or helm hook) after a
// msom_modes_compute -- a handle that only decomposes never pays its 4/3 nl layers -- and dropped with the modes.
static int helm_build_pyramid(msom *m) {
  const int nl = m->nl;
  m->helm_ibu.assign(m->nlev, nullptr);
  for (int k = 0; k < m->nlev; k++) {
    HIPCHK(hipMalloc(&m->helm_ibu[k], m->sg[k].ls * nl * sizeof(double)));
    HIPCHK(hipMemsetAsync(m->helm_ibu[k], 0, m->sg[k].ls * nl * sizeof(double), m->st));
  }
  if (m->nlev > 0) launch_nat_to_split(m->st, m->modes_md + (size_t)nl * nl * m->g.ls, m->g, m->helm_ibu[0], m->sg[0], nl);
  for (int k = 1; k < m->nlev; k++) launch_restrict(m->st, m->helm_ibu[k - 1], m->sg[k - 1], m->helm_ibu[k], m->sg[k], nl);
  return MSOM_OK;
}
// the modes (computed if they are not ready: the effect and the errors of msom_modes_compute) and the buffers of the modal solve
int helm_ensure(msom *m) {
  if (m->nranks > 1) { msom_set_error("the modal inversion runs on a single tile"); return MSOM_ERR_CONFIG; }
  if (!m->modes_ready) {
    int r = msom_modes_compute(m);
    if (r) return r;
  }
  if (!m->modes_compact && m->helm_ibu.empty()) {
    int r = helm_build_pyramid(m);
    if (r) { helm_drop_pyramid(m); return r; }
  }
  const size_t bytes = m->g.ls * m->nl * sizeof(double);
  if (!m->helm_pm) {
    HIPCHK(hipMalloc(&m->helm_pm, bytes));
    HIPCHK(hipMemsetAsync(m->helm_pm, 0, bytes, m->st));
  }
  if (!m->helm_qm) {
    HIPCHK(hipMalloc(&m->helm_qm, bytes));
    HIPCHK(hipMemsetAsync(m->helm_qm, 0, bytes, m->st));
  }
  if (!m->helm_scal) HIPCHK(hipMalloc(&m->helm_scal, HS_COUNT * sizeof(double)));
  if (!m->helm_partial) HIPCHK(hipMalloc(&m->helm_partial, (size_t)MSOM_MAXNL * helm_partial_stride(m) * sizeof(double)));
  return MSOM_OK;
}
// coefficient source of level k: iBu_m by value (compact form; *hc filled) or the level's array of the pyramid
static const HelmCoef *helm_level_coef(const msom *m, int k, HelmCoef *hc, const double **ibu_sp) {
  if (m->model) {   // newqg dialect: one problem, lambda = iRd2_low (uniform, newqg/qg.h:348-354)
    *hc = helm_coef(&m->nq.iRd2_low, 1, m->rc[k].sqD);
    *ibu_sp = nullptr;
    return hc;
  }
  if (m->modes_compact) {
    *hc = helm_coef(m->modes_mc.ibu, m->nl, m->rc[k].sqD);
    *ibu_sp = nullptr;
    return hc;
  }
  *ibu_sp = m->helm_ibu[k];
  return nullptr;
}
// nhalf half-sweeps of level k starting with colour 0; half-sweep h is sweep h / 2 of the per-mode counts
int helm_relax_level(msom *m, int k, int nhalf, const HelmCount &cnt, ProfSlot *ps) {
  HelmCoef hc;
  const double *ibu_sp;
  const HelmCoef *phc = helm_level_coef(m, k, &hc, &ibu_sp);
  for (int h = 0; h < nhalf; h++) {
    if (ps && !(h & 1)) prof_begin(m, *ps);
    if (launch_helm_relax(m->st, m->da[k], m->res[k], ibu_sp, phc, m->sg[k], m->nl, m->rc[k].sqD, h & 1, h >> 1, cnt, m->walls)) {
      msom_set_error("modal inversion: no kernel for nl = %d", m->nl);
      return MSOM_ERR_CONFIG;
    }
    if (ps && ((h & 1) || h == nhalf - 1)) prof_end(m, *ps);
  }
  return MSOM_OK;
}
int helm_residual(msom *m, const double *a, const double *b, int slot, int want_sum) {
  HelmCoef hc;
  const double *ibu_sp;
  const HelmCoef *phc = helm_level_coef(m, 0, &hc, &ibu_sp);
  if (m->profile) prof_begin(m, m->prof_helm_resid);
  const int r = launch_helm_residual(m->st, a, b, ibu_sp, phc, m->g, m->res[0], m->sg[0], m->nl, m->rc[0].D, m->helm_scal + slot, m->helm_partial,
                                     helm_partial_stride(m), want_sum);
  if (m->profile) prof_end(m, m->prof_helm_resid);
  if (r) { msom_set_error("modal inversion: no kernel for nl = %d", m->nl); return MSOM_ERR_CONFIG; }
  return MSOM_OK;
}
// one cycle of mspg/elliptic.h:53-89 (minlevel = 1) for every mode at once, level by level: the residual restricted to all levels,
// then from the coarsest level up prolongation (zero on the coarsest) and max-count sweeps, each mode stopping at its own count.
// A frozen mode (count 0) is swept nowhere: its correction stays the zero the coarsest level starts from.
static int helm_cycle(msom *m, const HelmCount &cnt, int nrelax) {
  const int nl = m->nl;
  for (int k = 1; k < m->nlev; k++) launch_restrict(m->st, m->res[k - 1], m->sg[k - 1], m->res[k], m->sg[k], nl);
  int kc = m->nlev;   // finest of the launch-bound levels (<= 64 cells a side); profile slot "helm_coarse" times them as one span
  for (int k = m->nlev - 1; k >= 1 && m->sg[k].nx <= 64 && m->sg[k].ny <= 64; k--) kc = k;
  for (int k = m->nlev - 1; k >= 0; k--) {
    if (m->profile && k == m->nlev - 1 && kc < m->nlev) prof_begin(m, m->prof_helm_coarse);
    if (k == m->nlev - 1) HIPCHK(hipMemsetAsync(m->da[k], 0, m->sg[k].ls * nl * sizeof(double), m->st));
    else launch_prolong(m->st, m->da[k + 1], m->sg[k + 1], m->da[k], m->sg[k], nl, m->walls);
    int r = helm_relax_level(m, k, 2 * nrelax, cnt, m->profile && k == 0 ? &m->prof_helm_relax : nullptr);
    if (r) return r;
    if (m->profile && k == kc) prof_end(m, m->prof_helm_coarse);
  }
  return MSOM_OK;
}
int helm_read(msom *m, double *h) {
  HIPCHK(hipMemcpyAsync(h, m->helm_scal, HS_COUNT * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  return m->sticky;
}
// natural [nl] field <-> the other space, through the staging buffer (k_modes_project works on contiguous arrays)
static int helm_project(msom *m, const double *in, double *out, int to_modes) {
  launch_unpack(m->st, in, m->staging, m->g, m->nl);
  if (launch_modes_project(m->st, m->staging, m->staging, m->modes_md, modes_mc(m), m->g, m->nl, modes_layers(m), to_modes)) return MSOM_ERR_CONFIG;
  launch_pack(m->st, m->staging, out, m->g, m->nl);
  return MSOM_OK;
}
// ghosts of a mode-space field: homogeneous Dirichlet at the faces, or wrapped
void helm_fill(msom *m, double *f) {
  if (m->walls & WALL_PER) launch_fill_periodic(m->st, f, m->g, m->nl, 1);
  else launch_fill_ghost(m->st, f, m->g, m->nl, BC_DIRICHLET0, m->walls);
}

// nl times mg_solve(a_m, b_m, lambda = iBu_m), run side by side: a cycle of the batch is a cycle of every mode that still wants one
// (helm_inl.h has the bookkeeping).  The host reads the nl maxima once per cycle.  a: natural field with valid ghosts, warm start and
// result (its ghosts are the correction's on return); b: natural field.  The sources: the modal inversion's mode-space fields
// (helm_solve), or psi and q themselves with one problem (nq_solve).
int helm_run(msom *m, double *a, const double *b) {
  const Params &p = m->p;
  const int nl = m->nl;
  int r;
  HIPCHK(hipMemsetAsync(m->helm_scal, 0, HS_COUNT * sizeof(double), m->st));
  HelmSolve &h = m->helm;
  helm_begin(h, nl, p.nitermin, p.nitermax, p.tolerance);
  double hs[HS_COUNT];
  if ((r = helm_residual(m, a, b, HS_RES0, 1))) return r;
  for (int k = 0; k < nl; k++)
    launch_sum_final(m->st, m->helm_partial + (size_t)k * helm_partial_stride(m), m->helm_scal + HS_BSUM + k, helm_residual_blocks(m->g));
  if (p.nitermin < 1) {   // the first cycle depends on the warm start's residual
    if ((r = helm_read(m, hs))) return r;
    helm_first(h, hs + HS_RES0, hs + HS_BSUM);
  }
  HelmCount cnt = {};
  int nrelax;
  while ((nrelax = helm_counts(h, cnt.n)) > 0) {
    if ((r = helm_cycle(m, cnt, nrelax))) return r;
    launch_correct(m->st, a, m->g, m->da[0], m->sg[0], nl, m->walls);   // a frozen mode adds its zero correction
    HIPCHK(hipMemsetAsync(m->helm_scal + HS_RES1, 0, MSOM_MAXNL * sizeof(double), m->st));
    if ((r = helm_residual(m, a, b, HS_RES1, 0))) return r;
    if ((r = helm_read(m, hs))) return r;
    helm_first(h, hs + HS_RES0, hs + HS_BSUM);
    helm_cycle_done(h, cnt.n, hs + HS_RES1);
  }
  if (!h.have_first) {   // NITERMAX == 0
    if ((r = helm_read(m, hs))) return r;
    helm_first(h, hs + HS_RES0, hs + HS_BSUM);
  }
  for (int k = 0; k < nl; k++)
    if (h.s[k].resa > p.tolerance && !m->quiet)
      fprintf(stderr, "WARNING: convergence not reached after %d iterations\n  mode: %d res: %g sum: %g nrelax: %d\n", h.s[k].i, k, h.s[k].resa,
              h.s[k].sum, h.s[k].nrelax);
  m->mg = h.s[nl - 1];   // the reference's mgpsi is overwritten by every poisson() call: the last mode's stay
  return m->sticky;
}
int helm_solve(msom *m, const double *q) {
  int r = helm_ensure(m);
  if (r) return r;
  m->res_ready = -1;
  m->umax_ready = 0;
  if ((r = helm_project(m, q, m->helm_qm, 1))) return r;
  if ((r = helm_run(m, m->helm_pm, m->helm_qm))) return r;
  m->helm_solved = 1;
  if ((r = helm_project(m, m->helm_pm, m->f[MSOM_PSI], 0))) return r;
  fill_bc(m, MSOM_PSI);
  return m->sticky;
}
