// msom_newqg.hip -- the newqg dialect of a msom_t (msom_create_newqg*) and the nq_* targets the shared entry points dispatch to.
// Restates newqg/qg.h (set_vars :291-336, set_const :345-358, invertq :148-157, update_qg :264-284, advance_qg :249-261), see below.
#include "msom_host.h"

// ------------------------------------------------------------------ newqg dialect (msom_create_newqg)
//
// The cell-centred one-layer model of newqg/qg.h with the optional Helmholtz ("1.5-layer", gp_low) inversion on a msom_t: set_vars
// :291-336, set_const :345-358, invertq :148-157 (Basilisk's poisson(psi, q, lambda = iRd2_low): the multigrid of helm_run with one
// problem, a = psi in place, b = q), comp_q :184-189, update_qg :264-284, advection_pv's limiter :202-219, advance_qg :249-261, one
// iteration of run().  One tile; fields MSOM_PSI, Q, ZETA, DQ, QPRED, QFORC, one layer each.

int nq_refuse(const char *fn) {
  msom_set_error("%s: not available on a newqg handle (msom_create_newqg)", fn);
  return MSOM_ERR_CONFIG;
}
bool nq_has_field(int field) {
  return field == MSOM_PSI || field == MSOM_Q || field == MSOM_ZETA || field == MSOM_DQ || field == MSOM_QPRED || field == MSOM_QFORC;
}

int nq_alloc(msom *m) {
  for (int k = 0; k < m->nlev; k++) {   // Delta of every level for the Helmholtz cycle (make_relax_coef's part of it)
    memset(&m->rc[k], 0, sizeof m->rc[k]);
    m->rc[k].D = m->p.L0 / (double)(m->gnx >> k);
    m->rc[k].sqD = m->rc[k].D * m->rc[k].D;
  }
  HIPCHK(hipMalloc(&m->helm_scal, HS_COUNT * sizeof(double)));
  HIPCHK(hipMalloc(&m->helm_partial, (size_t)MSOM_MAXNL * helm_partial_stride(m) * sizeof(double)));
  return MSOM_OK;
}

static msom *nq_create(NewqgParams &q, const char *text) {
  if (msom_newqg_params_derive(&q)) return nullptr;
  Params p;   // what the shared parts of the handle read: grid, solver controls, limiter
  msom_params_defaults(&p);
  p.N = q.N; p.Ny = q.Ny; p.nl = 1; p.L0 = q.L0; p.DT = q.DT; p.CFL = q.CFL; p.tolerance = q.TOLERANCE;
  p.nitermax = q.nitermax; p.nitermin = q.nitermin; p.sbc = q.sbc; p.beta = q.beta; p.tau0 = q.tau0; p.tend = q.tend; p.dtout = q.dtout;
  p.dhu[0] = q.dh[0];
  msom *m = create_common(p, 1, 1, 0, nullptr, &q);
  if (m) m->params_text = text;
  return m;
}
extern "C" msom_t *msom_create_newqg_str(const char *text) {
  if (!text) { msom_set_error("null params text"); return nullptr; }
  NewqgParams q;
  msom_newqg_params_defaults(&q);
  msom_newqg_params_parse_text(&q, text);
  return nq_create(q, text);
}
extern "C" msom_t *msom_create_newqg(const char *path) {
  const char *pp = path ? path : "params.in";
  FILE *fp = fopen(pp, "rt");
  if (!fp) {
    msom_set_error("file %s not found", pp);   // reference: message + exit(0), newqg/extra.h:63-66
    return nullptr;
  }
  std::string text;   // kept as the handle's copy of the file; the parameters come from the file parser, as the reference reads them
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, n);
  fclose(fp);
  NewqgParams q;
  msom_newqg_params_defaults(&q);
  if (msom_newqg_params_parse_file(&q, pp)) return nullptr;
  return nq_create(q, text.c_str());
}

int nq_set_option(msom *m, const char *key, double v) {
  if (!strcmp(key, "TOLERANCE")) m->p.tolerance = v;
  else if (!strcmp(key, "NITERMAX")) m->p.nitermax = (int)v;
  else if (!strcmp(key, "NITERMIN")) m->p.nitermin = (int)v;
  else if (!strcmp(key, "DT")) m->p.DT = v;
  else if (!strcmp(key, "quiet")) m->quiet = (int)v;
  else if (!strcmp(key, "profile")) m->profile = (int)v;
  else if (!strcmp(key, "nq_fused")) m->nq_fused = (int)v != 0;
  else if (!strcmp(key, "nq_adv_fused")) m->nq_adv_fused = (int)v != 0;
  else if (!strcmp(key, "nq_rows")) {
    if (!(v >= 0) || v > 4096) { msom_set_error("option nq_rows = %g", v); return MSOM_ERR_ARG; }
    m->nq_rows = (int)v;
  } else {
    msom_set_error("unknown option %s (newqg handle)", key);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}
double nq_get_param(msom *m, const char *key) {
  const NewqgParams &q = m->nq;
  if (!strcmp(key, "N") || !strcmp(key, "nx")) return m->gnx;
  if (!strcmp(key, "ny")) return m->gny;
  if (!strcmp(key, "nl")) return 1;
  if (!strcmp(key, "L0")) return q.L0;
  if (!strcmp(key, "DT")) return m->p.DT;
  if (!strcmp(key, "CFL")) return q.CFL;
  if (!strcmp(key, "TOLERANCE")) return m->p.tolerance;
  if (!strcmp(key, "tend")) return q.tend;
  if (!strcmp(key, "dtout")) return q.dtout;
  if (!strcmp(key, "f0")) return q.f0;
  if (!strcmp(key, "beta")) return q.beta;
  if (!strcmp(key, "nu")) return q.nu;
  if (!strcmp(key, "hEkb")) return q.hEkb;
  if (!strcmp(key, "tau0")) return q.tau0;
  if (!strcmp(key, "gp_low")) return q.gp_low;
  if (!strcmp(key, "sbc")) return q.sbc;
  if (!strcmp(key, "bc_fac")) return q.bc_fac;
  if (!strcmp(key, "iRd2_low")) return q.iRd2_low;
  if (!strcmp(key, "dh_0")) return q.dh[0];
  if (!strcmp(key, "nlevels")) return m->nlev;
  if (!strcmp(key, "nq_fused")) return m->nq_fused;
  if (!strcmp(key, "nq_adv_fused")) return m->nq_adv_fused;
  if (!strcmp(key, "nq_rows")) return nq_rhs_rows(m->g, m->nq_rows);   // the chunk height a launch of k_nq_rhs takes
  return NAN;
}

// boundary() of the three kinds of field.  psi: dirichlet(0), corners by the y rule over the x-ghost column (newqg/qg.h:304-307);
// periodic: wrapped copies, two cells deep because k_nq_rhs forms zeta at the ghost positions from them
static void nq_fill_psi(msom *m) {
  if (m->walls & WALL_PER) launch_fill_periodic(m->st, m->f[MSOM_PSI], m->g, 1, 2);
  else launch_fill_ghost(m->st, m->f[MSOM_PSI], m->g, 1, BC_DIRICHLET0, m->walls);
}
// zeta and q: bc_fac * (psi[interior] - psi[ghost]) (:310-318), or wrapped
static void nq_fill_zq(msom *m, int field) {
  if (m->walls & WALL_PER) launch_fill_periodic(m->st, m->f[field], m->g, 1, 1);
  else launch_nq_ghost(m->st, m->f[MSOM_PSI], m->f[field], m->g, m->nq.bc_fac);
}
// msom_set_field: upload() applied the generic ghost fill; the fields with a rule of their own take it here
int nq_after_upload(msom *m, int field) {
  if (field == MSOM_PSI) nq_fill_psi(m);
  else if (field == MSOM_Q || field == MSOM_ZETA) nq_fill_zq(m, field);
  return MSOM_OK;
}

// comp_q, newqg/qg.h:184-189: q = lap(psi); gp_low != 0: q = q + iRd2_low * psi; boundary(q)
static void nq_comp_q(msom *m) {
  launch_del2(m->st, m->f[MSOM_PSI], m->f[MSOM_Q], m->g, 1, 0., 1., m->p.L0 / m->gnx);
  if (m->nq.gp_low != 0.) launch_axpy(m->st, m->f[MSOM_Q], m->f[MSOM_PSI], m->g, 1, m->nq.iRd2_low);
  nq_fill_zq(m, MSOM_Q);
}
// set_const, newqg/qg.h:345-358 (event init): the start of a run -- time, iteration count and the limiter's static `previous` (:203)
// are what they are when the reference's process starts
int nq_set_const(msom *m) {
  nq_fill_psi(m);
  nq_comp_q(m);
  m->const_set = 1;
  m->previous = 0.;
  m->t = 0.;
  m->iter = 0;
  return sync_stream(m);
}
#define NQ_NEED_CONST(m, fn)                                          \
  do {                                                                \
    if (!(m)->const_set) {                                            \
      msom_set_error("%s: msom_set_const has not been called", fn);   \
      return MSOM_ERR_STATE;                                          \
    }                                                                 \
  } while (0)

// invertq, newqg/qg.h:148-157: psi is warm start and result; boundary(psi) after the last correction
static int nq_solve(msom *m, const double *q) {
  int r = helm_run(m, m->f[MSOM_PSI], q);
  if (r) return r;
  nq_fill_psi(m);
  return m->sticky;
}
// the solve and the dt limiter of advection_pv (:202-219): one pass over the faces with one static `previous`.  D / max|u| is the
// minimum over the faces of D / |u| exactly (division is monotone), so the maximum comes from launch_umax as on the modal path
static double nq_solve_dt(msom *m, int qfield, double dtmax) {
  if (nq_solve(m, m->f[qfield])) return -1;
  launch_umax(m->st, m->f[MSOM_PSI], m->partial_umax, m->d_scal + SC_UMAX, m->g, 1, m->p.L0 / m->gnx);
  if (reduce_scal(m, SC_UMAX, 1, RED_MAX)) return -1;
  if (m->sticky) return -1;
  return limiter(m, m->h_scal[SC_UMAX], dtmax);
}
// the tendency after the inversion (:276-281) into MSOM_ZETA and MSOM_DQ; adv_out >= 0 asks for q[adv_out] = q[adv_in] + dt * dq as
// well (advance_qg), folded into the pass where the options allow (dq is then not stored)
static int nq_rhs(msom *m, int adv_out, int adv_in, double dt) {
  const NewqgParams &q = m->nq;
  const double D = m->p.L0 / m->gnx, cek = q.hEkb * q.f0 / (2 * q.dh[0]);
  const double *qforc = m->have_qforc ? m->f[MSOM_QFORC] : nullptr;
  if (m->profile) prof_begin(m, m->prof_rhs);
  if (m->nq_fused) {
    const bool adv = adv_out >= 0 && m->nq_adv_fused;
    launch_nq_rhs(m->st, m->f[MSOM_PSI], qforc, m->f[MSOM_ZETA], m->f[MSOM_DQ], m->g, m->walls, D, q.beta, q.nu, cek, q.bc_fac,
                  adv ? m->f[adv_in] : nullptr, adv ? m->f[adv_out] : nullptr, dt, m->nq_rows);
    if (adv) adv_out = -1;
  } else {   // one launch per loop of the reference
    launch_del2(m->st, m->f[MSOM_PSI], m->f[MSOM_ZETA], m->g, 1, 0., 1., D);                 // comp_del2(psi, zeta, 0., 1.)
    nq_fill_zq(m, MSOM_ZETA);
    launch_nq_adv(m->st, m->f[MSOM_PSI], m->f[MSOM_ZETA], m->f[MSOM_DQ], m->g, D, q.beta);   // advection_pv on the zeroed updates
    launch_del2(m->st, m->f[MSOM_ZETA], m->f[MSOM_DQ], m->g, 1, 1., q.nu, D);                // dissip: comp_del2(zeta, dqdt, 1., nu)
    launch_axpy(m->st, m->f[MSOM_DQ], m->f[MSOM_ZETA], m->g, 1, -cek);                       // ekman_friction
    if (qforc) launch_axpy(m->st, m->f[MSOM_DQ], qforc, m->g, 1, 1.);                        // surface_forcing: the handle's MSOM_QFORC
  }
  if (adv_out >= 0) launch_advance(m->st, m->f[adv_out], m->f[adv_in], m->f[MSOM_DQ], nullptr, m->g, 1, dt, 0.);
  if (m->profile) prof_end(m, m->prof_rhs);
  return MSOM_OK;
}

double nq_update(msom *m, const double *q, double *dqdt, double dtmax) {
  NQ_NEED_CONST(m, "msom_update");
  int qf = MSOM_Q;
  if (q) {
    if (upload(m, MSOM_QPRED, q)) return -1;
    qf = MSOM_QPRED;
  }
  const double d = nq_solve_dt(m, qf, dtmax);
  if (d < 0) return d;
  if (nq_rhs(m, -1, -1, 0.)) return -1;
  if (dqdt && download(m, MSOM_DQ, dqdt)) return -1;
  if (sync_stream(m)) return -1;
  return d;
}
int nq_advance(msom *m, double *qout, const double *qin, const double *dqdt, double dt) {
  NQ_NEED_CONST(m, "msom_advance");
  int f = MSOM_Q, r;
  if (qin) {
    if ((r = upload(m, MSOM_QPRED, qin))) return r;
    f = MSOM_QPRED;
  }
  if (dqdt && (r = upload(m, MSOM_DQ, dqdt))) return r;
  launch_advance(m->st, m->f[f], m->f[f], m->f[MSOM_DQ], nullptr, m->g, 1, dt, 0.);
  if (qout) return download(m, f, qout);
  return sync_stream(m);
}
int nq_invertq(msom *m, const double *q, double *psi, msom_mgstats *st) {
  NQ_NEED_CONST(m, "msom_invertq");
  int qf = MSOM_Q, r;
  if (q) {
    if ((r = upload(m, MSOM_QPRED, q))) return r;
    qf = MSOM_QPRED;
  }
  if (psi) {
    if ((r = upload(m, MSOM_PSI, psi))) return r;
    nq_fill_psi(m);
  }
  if ((r = nq_solve(m, m->f[qf]))) return r;
  if (st) *st = m->mg;
  if (psi) return download(m, MSOM_PSI, psi);
  return sync_stream(m);
}
int nq_comp_q_api(msom *m, const double *psi, double *q) {
  NQ_NEED_CONST(m, "msom_comp_q");
  int r;
  if (psi) {
    if ((r = upload(m, MSOM_PSI, psi))) return r;
    nq_fill_psi(m);
  }
  nq_comp_q(m);
  if (q) return download(m, MSOM_Q, q);
  return sync_stream(m);
}
// one iteration of run() [Basilisk predictor-corrector.h] by the rules of msom_step; the limiter is applied once per update and its
// `previous` moves in the second update as well (advection_pv has one static, :203,216-218).  Synchronous.
int nq_step(msom *m, double *dt_used) {
  NQ_NEED_CONST(m, "msom_step");
  double tnext;
  int r;
  const double d = nq_solve_dt(m, MSOM_Q, m->p.DT);
  if (d < 0) return m->sticky ? m->sticky : MSOM_ERR_HIP;
  m->dt = dtnext(m, d, &tnext);
  if ((r = nq_rhs(m, MSOM_QPRED, MSOM_Q, m->dt / 2.))) return r;
  const double d2 = nq_solve_dt(m, MSOM_QPRED, m->dt);
  if (d2 < 0) return m->sticky ? m->sticky : MSOM_ERR_HIP;
  if ((r = nq_rhs(m, MSOM_Q, MSOM_Q, m->dt))) return r;
  if ((r = sync_stream(m))) return r;
  m->t = tnext;
  m->iter++;
  if (dt_used) *dt_used = m->dt;
  return MSOM_OK;
}
// back-to-back launches, HIP-event timed: "nq_rhs" (k_nq_rhs with the advance folded in, as a step's first stage runs it),
// "nq_rhs_dq" (tendency only), "helm_sweep" / "helm_residual" (finest level of the solve)
int nq_bench_kernel(msom *m, const char *kernel, int reps, double *avg_ms) {
  NQ_NEED_CONST(m, "msom_bench_kernel");
  if (!kernel || reps < 1 || !avg_ms) return MSOM_ERR_ARG;
  const int which = !strcmp(kernel, "nq_rhs") ? 0 : !strcmp(kernel, "nq_rhs_dq") ? 1 : !strcmp(kernel, "helm_sweep") ? 2 : !strcmp(kernel, "helm_residual") ? 3 : -1;
  if (which < 0) { msom_set_error("unknown kernel %s (newqg handle)", kernel); return MSOM_ERR_ARG; }
  const NewqgParams &q = m->nq;
  const double D = m->p.L0 / m->gnx, cek = q.hEkb * q.f0 / (2 * q.dh[0]);
  const double *qforc = m->have_qforc ? m->f[MSOM_QFORC] : nullptr;
  HelmCount all = {};
  all.n[0] = 1;
  hipEvent_t a = nullptr, b = nullptr;
  struct Events {   // destroyed on every way out
    hipEvent_t &a, &b;
    ~Events() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
  } events{a, b};
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  auto one = [&](void) {
    if (which == 0)
      launch_nq_rhs(m->st, m->f[MSOM_PSI], qforc, m->f[MSOM_ZETA], m->f[MSOM_DQ], m->g, m->walls, D, q.beta, q.nu, cek, q.bc_fac, m->f[MSOM_Q],
                    m->f[MSOM_QPRED], 1e-9, m->nq_rows);
    else if (which == 1)
      launch_nq_rhs(m->st, m->f[MSOM_PSI], qforc, m->f[MSOM_ZETA], m->f[MSOM_DQ], m->g, m->walls, D, q.beta, q.nu, cek, q.bc_fac, nullptr, nullptr,
                    0., m->nq_rows);
    else if (which == 2) helm_relax_level(m, 0, 2, all, nullptr);
    else helm_residual(m, m->f[MSOM_PSI], m->f[MSOM_Q], HS_RES1, 0);
  };
  for (int k = 0; k < 3; k++) one();
  HIPCHK(hipEventRecord(a, m->st));
  for (int k = 0; k < reps; k++) one();
  HIPCHK(hipEventRecord(b, m->st));
  HIPCHK(hipEventSynchronize(b));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, a, b));
  *avg_ms = ms / reps;
  return MSOM_OK;
}
