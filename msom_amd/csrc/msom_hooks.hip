// msom_hooks.hip -- debug / test hooks (msom_dbg_*), the profile slots (msom_profile_*) and msom_bench_kernel.  No reference call
// stack of its own: the hooks run single passes of the solver (mspg/elliptic.h) and of the tendency (msqg/qg.h:609-650) of msom_api.hip.
#include "msom_host.h"

// ------------------------------------------------------------------ debug / test hooks

extern "C" int msom_dbg_nlevels(msom_t *m) { return m ? m->nlev : MSOM_ERR_ARG; }
extern "C" int msom_dbg_level_dims(msom_t *m, int lev, int *nx, int *ny) {
  if (!m || lev < 0 || lev >= m->nlev) return MSOM_ERR_ARG;
  *nx = m->sg[lev].nx; *ny = m->sg[lev].ny;
  return MSOM_OK;
}
static int split_upload(msom *m, double *sp, const SplitGeom &sg, const double *a, int nl, int bc) {
  HIPCHK(hipMemcpyAsync(m->staging, a, (size_t)nl * sg.nx * sg.ny * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemsetAsync(sp, 0, sg.ls * nl * sizeof(double), m->st));
  launch_split_pack(m->st, m->staging, sp, sg, nl, bc, m->walls);
  return MSOM_OK;
}
static int split_download(msom *m, const double *sp, const SplitGeom &sg, double *a, int nl) {
  launch_split_unpack(m->st, sp, sg, m->staging, nl);
  HIPCHK(hipMemcpyAsync(a, m->staging, (size_t)nl * sg.nx * sg.ny * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}
// nsweeps red-black relaxations on level `lev`: da in/out, res in (both [layer][y][x] of that level)
extern "C" int msom_dbg_relax(msom_t *m, int lev, double *da, const double *res, int nsweeps) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (lev < 0 || lev >= m->nlev || !da || !res) return MSOM_ERR_ARG;
  int r;
  if ((r = split_upload(m, m->da[lev], m->sg[lev], da, m->nl, BC_DIRICHLET0))) return r;
  if ((r = split_upload(m, m->res[lev], m->sg[lev], res, m->nl, BC_NEUMANN))) return r;
  STICKY(m, exch_split(m, m->da[lev], m->sg[lev], m->nl, 0));
  const int prof = m->profile;
  m->profile = 0;
  {
    Lev L = tile_lev(m, lev);
    relax_sweeps(m, L, nullptr, nsweeps, 0, false);
  }
  m->profile = prof;
  return split_download(m, m->da[lev], m->sg[lev], da, m->nl);
}
// One tendency + advance pass q_pred = q + dt dq on the handle's psi and q, then the first residual of the inversion of q_pred on levels 0 and
// 1 as mg_solve would take it: fused = 1 out of the pass itself (option rhs_resid), 0 from k_residual2<write + restrict>.  res0 / res1: the
// raw split arrays (split_ls_0 / split_ls_1 doubles per layer), filled with NaN beforehand so that what a kernel leaves alone shows
extern "C" int msom_dbg_rhs_resid(msom_t *m, int fused, double dt, double *res0, double *res1, double *maxres, double *bsum) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (!res0 || !res1 || m->nlev < 2) return MSOM_ERR_ARG;
  for (int k = 0; k < 2; k++) HIPCHK(hipMemsetAsync(m->res[k], 0xFF, m->sg[k].ls * m->nl * sizeof(double), m->st));
  HIPCHK(hipMemsetAsync(m->d_scal, 0, (SC_UMAX + MSOM_MAXNL) * sizeof(double), m->st));
  RhsPass ps{MSOM_Q, MSOM_DQ, 1, MSOM_QPRED, MSOM_Q, dt};
  ps.emit_resid = fused ? 1 : 0;
  int r = rhs_terms(m, ps);
  if (r) return r;
  const bool adv = ps.advanced;
  const bool emitted = m->res_ready == MSOM_QPRED;
  m->res_ready = -1;
  if (!adv || (fused && !emitted)) { msom_set_error("msom_dbg_rhs_resid: this handle's tendency pass does not %s", adv ? "emit the residual" : "advance"); return MSOM_ERR_CONFIG; }
  int slot = SC_RESF;
  if (fused) launch_sum_final(m->st, m->partial_rr, m->d_scal + SC_BSUM, m->rr_nparts);
  else {
    residual2(m, 2 | 4, m->f[MSOM_QPRED], SC_RES0, 1);
    launch_sum_final(m->st, m->partial, m->d_scal + SC_BSUM, residual2_blocks(m->g));
    slot = SC_RES0;
  }
  double h[2] = {0., 0.};
  HIPCHK(hipMemcpyAsync(&h[0], m->d_scal + slot, sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipMemcpyAsync(&h[1], m->d_scal + SC_BSUM, sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipMemcpyAsync(res0, m->res[0], m->sg[0].ls * m->nl * sizeof(double), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipMemcpyAsync(res1, m->res[1], m->sg[1].ls * m->nl * sizeof(double), hipMemcpyDeviceToHost, m->st));
  if ((r = sync_stream(m))) return r;
  if (maxres) *maxres = h[0];
  if (bsum) *bsum = h[1];
  return MSOM_OK;
}
extern "C" int msom_dbg_residual(msom_t *m, const double *a, const double *b, double *res, double *maxres) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  int r;
  if ((r = upload(m, MSOM_TMP, a))) return r;
  if ((r = upload(m, MSOM_QPRED, b))) return r;
  HIPCHK(hipMemsetAsync(m->d_scal, 0, 8 * sizeof(double), m->st));
  residual(m, m->f[MSOM_TMP], m->f[MSOM_QPRED], SC_RES0, 0);
  HIPCHK(hipMemcpyAsync(m->h_scal + SC_RES0, m->d_scal + SC_RES0, sizeof(double), hipMemcpyDeviceToHost, m->st));
  if ((r = split_download(m, m->res[0], m->sg[0], res, m->nl))) return r;
  if (maxres) *maxres = m->h_scal[SC_RES0];
  return MSOM_OK;
}
extern "C" int msom_dbg_helm_relax(msom_t *m, int lev, double *da, const double *res, int nhalf, const int *count_per_mode) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (lev < 0 || lev >= m->nlev || !da || !res || nhalf < 0) return MSOM_ERR_ARG;
  int r;
  if ((r = helm_ensure(m))) return r;
  if ((r = split_upload(m, m->da[lev], m->sg[lev], da, m->nl, BC_DIRICHLET0))) return r;
  if ((r = split_upload(m, m->res[lev], m->sg[lev], res, m->nl, BC_NEUMANN))) return r;
  HelmCount cnt = {};
  for (int k = 0; k < m->nl; k++) cnt.n[k] = count_per_mode ? count_per_mode[k] : (nhalf + 1) / 2;
  if ((r = helm_relax_level(m, lev, nhalf, cnt, nullptr))) return r;
  return split_download(m, m->da[lev], m->sg[lev], da, m->nl);
}
extern "C" int msom_dbg_helm_residual(msom_t *m, const double *a, const double *b, double *res, double *maxres_per_mode) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (!a || !b || !res) return MSOM_ERR_ARG;
  int r;
  if ((r = helm_ensure(m))) return r;
  const size_t n = (size_t)m->nl * m->nx * m->ny * sizeof(double);
  HIPCHK(hipMemcpyAsync(m->staging, a, n, hipMemcpyDefault, m->st));
  launch_pack(m->st, m->staging, m->f[MSOM_TMP], m->g, m->nl);
  helm_fill(m, m->f[MSOM_TMP]);
  HIPCHK(hipMemcpyAsync(m->staging, b, n, hipMemcpyDefault, m->st));
  launch_pack(m->st, m->staging, m->helm_qm, m->g, m->nl);
  HIPCHK(hipMemsetAsync(m->helm_scal, 0, HS_COUNT * sizeof(double), m->st));
  if ((r = helm_residual(m, m->f[MSOM_TMP], m->helm_qm, HS_RES0, 0))) return r;
  double hs[HS_COUNT];
  if ((r = helm_read(m, hs))) return r;
  if ((r = split_download(m, m->res[0], m->sg[0], res, m->nl))) return r;
  if (maxres_per_mode) for (int k = 0; k < m->nl; k++) maxres_per_mode[k] = hs[HS_RES0 + k];
  return MSOM_OK;
}
extern "C" int msom_dbg_restrict(msom_t *m, int lev_fine, const double *fine, double *coarse) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (lev_fine < 0 || lev_fine + 1 >= m->nlev) return MSOM_ERR_ARG;
  int r;
  if ((r = split_upload(m, m->res[lev_fine], m->sg[lev_fine], fine, m->nl, BC_NEUMANN))) return r;
  launch_restrict(m->st, m->res[lev_fine], m->sg[lev_fine], m->res[lev_fine + 1], m->sg[lev_fine + 1], m->nl);
  return split_download(m, m->res[lev_fine + 1], m->sg[lev_fine + 1], coarse, m->nl);
}
extern "C" int msom_dbg_prolong(msom_t *m, int lev_coarse, const double *coarse, double *fine) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (lev_coarse < 1 || lev_coarse >= m->nlev) return MSOM_ERR_ARG;
  int r;
  if ((r = split_upload(m, m->da[lev_coarse], m->sg[lev_coarse], coarse, m->nl, BC_DIRICHLET0))) return r;
  STICKY(m, exch_split(m, m->da[lev_coarse], m->sg[lev_coarse], m->nl, 1));
  launch_prolong(m->st, m->da[lev_coarse], m->sg[lev_coarse], m->da[lev_coarse - 1], m->sg[lev_coarse - 1], m->nl, m->walls);
  return split_download(m, m->da[lev_coarse - 1], m->sg[lev_coarse - 1], fine, m->nl);
}
// single operators on the internal fields: "del2", "stretch", "advection", "dissip", "forcing"
extern "C" int msom_dbg_op(msom_t *m, const char *op, int f_in, int f_out, double add, double fac) {
  MSQG_ONLY(m);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (check_field(m, f_in) || check_field(m, f_out) || !op) return MSOM_ERR_ARG;
  const Params &p = m->p;
  const double D = p.L0 / m->gnx;
  if (!strcmp(op, "del2")) comp_del2(m, f_in, f_out, add, fac);
  else if (!strcmp(op, "stretch")) comp_stretch(m, f_in, f_out, add, fac);
  else if (!strcmp(op, "advection")) {  // f_in = zeta field, psi = PSI, dq = f_out (accumulates)
    launch_advection(m->st, m->f[f_in], m->f[MSOM_PSI], m->f[MSOM_PSIPG], m->f[MSOM_ZETAPG], m->f[MSOM_S], m->f[MSOM_Q], m->f[f_out], m->g,
                     m->nl, m->have_pg, m->have_zpg, m->stochastic, D, p.beta, p.itr_stoch, m->lc);
  } else {
    msom_set_error("unknown op %s", op);
    return MSOM_ERR_ARG;
  }
  return sync_stream(m);
}

// ------------------------------------------------------------------ measurement

// the one list of the profile slots: msom_destroy, msom_profile_reset and msom_profile_read all go through it (prof_march[0] and
// prof_march[1] never hold events)
std::vector<std::pair<const char *, ProfSlot *>> prof_slots(msom *m) {
  return {{"sweep", &m->prof_sweep}, {"residual", &m->prof_resid}, {"block2", &m->prof_block}, {"march2", &m->prof_march[2]},
          {"march3", &m->prof_march[3]}, {"march4", &m->prof_march[4]}, {"march_pl", &m->prof_march_pl}, {"march_corr", &m->prof_march_corr},
          {"march_visit", &m->prof_march_visit}, {"march_visit_coarse", &m->prof_march_visit_coarse}, {"resid_max", &m->prof_resmax}, {"rhs", &m->prof_rhs}, {"red_prolong", &m->prof_redprol},
          {"resid_correct", &m->prof_rescorr}, {"resid_restrict", &m->prof_respre}, {"helm_relax", &m->prof_helm_relax},
          {"helm_residual", &m->prof_helm_resid}, {"helm_coarse", &m->prof_helm_coarse}, {"floats", &m->prof_floats},
          {"floats_emigrate", &m->prof_floats_emig}, {"floats_immigrate", &m->prof_floats_immig}};
}
extern "C" int msom_profile_reset(msom_t *m) {
  if (!m) return MSOM_ERR_ARG;
  for (const auto &s : prof_slots(m)) { s.second->used = 0; s.second->total_ms = 0; s.second->launches = 0; }
  return MSOM_OK;
}
extern "C" int msom_profile_read(msom_t *m, const char *kernel, double *avg_ms, long *launches) {
  if (!m || !kernel) return MSOM_ERR_ARG;
  ProfSlot *ps = nullptr;
  for (const auto &s : prof_slots(m))
    if (!strcmp(kernel, s.first)) ps = s.second;
  if (!ps) { msom_set_error("unknown kernel %s", kernel); return MSOM_ERR_ARG; }
  prof_collect(m, *ps);
  if (avg_ms) *avg_ms = ps->launches ? ps->total_ms / ps->launches : 0.;
  if (launches) *launches = ps->launches;
  return MSOM_OK;
}
// back-to-back launches of one kernel on the finest level, HIP-event timed
extern "C" int msom_bench_kernel(msom_t *m, const char *kernel, int reps, double *avg_ms) {
  if (m && m->model) return nq_bench_kernel(m, kernel, reps, avg_ms);
  if (m) m->res_ready = -1;
  NEED_CONST(m);
  if (!kernel || reps < 1 || !avg_ms) return MSOM_ERR_ARG;
  // the solver's guard for these launchers is sweep_path / fuse_prolong; here the caller names them
  if (m->nl > MSOM_FASTNL && (!strncmp(kernel, "block2", 6) || !strcmp(kernel, "red_prolong"))) {
    msom_set_error("kernel %s has no instantiation for nl = %d (1..%d)", kernel, m->nl, MSOM_FASTNL);
    return MSOM_ERR_ARG;
  }
  if (!strncmp(kernel, "modes_", 6)) {
    if (strcmp(kernel, "modes_project") && strcmp(kernel, "modes_energy")) { msom_set_error("unknown kernel %s", kernel); return MSOM_ERR_ARG; }
    NEED_MODES(m, "msom_bench_kernel");
    if (!m->modes_partial) HIPCHK(hipMalloc(&m->modes_partial, (size_t)2 * MSOM_MAXNL * modes_energy_stride(m->g) * sizeof(double)));
  }
  int spec_cnt = 0;
  if (!strncmp(kernel, "spec_", 5)) {   // the passes of msom_spec_energy's KE half on one batch of layers (the work arrays are overwritten)
    if (strcmp(kernel, "spec_rows") && strcmp(kernel, "spec_transpose") && strcmp(kernel, "spec_cols") && strcmp(kernel, "spec_shells")) {
      msom_set_error("unknown kernel %s", kernel);
      return MSOM_ERR_ARG;
    }
    int r = spec_guard(m, "msom_bench_kernel");
    if (r || (r = spec_ensure(m))) return r;
    spec_cnt = std::min(m->nl, m->spc_batch);
    spec_batch_2d(m, spec_in_nat(m, SPEC_IN_UV, m->f[MSOM_PSI], nullptr), spec_cnt, SPEC_SUM, nullptr);   // every pass finds its input
  }
  HelmCount helm_all = {};
  if (!strncmp(kernel, "helm_", 5)) {   // "helm_sweep": both half-sweeps of the finest level, every mode; "helm_residual"
    if (strcmp(kernel, "helm_sweep") && strcmp(kernel, "helm_residual")) { msom_set_error("unknown kernel %s", kernel); return MSOM_ERR_ARG; }
    int r = helm_ensure(m);
    if (r) return r;
    for (int k = 0; k < m->nl; k++) helm_all.n[k] = 1;
  }
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  const double D = m->p.L0 / m->gnx;
  auto one = [&](void) {
    if (!strcmp(kernel, "helm_sweep")) {
      helm_relax_level(m, 0, 2, helm_all, nullptr);
    } else if (!strcmp(kernel, "helm_residual")) {
      helm_residual(m, m->helm_pm, m->helm_qm, HS_RES1, 0);
    } else if (!strcmp(kernel, "sweep")) {
      for (int c = 0; c < 2; c++) launch_relax_color(m->st, m->da[0], m->res[0], m->S[0], m->sg[0], m->nl, m->rc[0], m->uniformS, c, m->walls, 1);
    } else if (!strcmp(kernel, "residual")) {
      launch_residual(m->st, m->f[MSOM_PSI], m->f[MSOM_Q], m->f[MSOM_S], m->g, m->res[0], m->sg[0], m->nl, m->rc[0], m->uniformS, m->d_scal + SC_RES1, m->partial, 0);
    } else if (!strcmp(kernel, "advection")) {
      launch_advection(m->st, m->f[MSOM_ZETA], m->f[MSOM_PSI], m->f[MSOM_PSIPG], m->f[MSOM_ZETAPG], m->f[MSOM_S], m->f[MSOM_Q], m->f[MSOM_TMP], m->g,
                       m->nl, m->have_pg, m->have_zpg, m->stochastic, D, m->p.beta, m->p.itr_stoch, m->lc);
    } else if (!strncmp(kernel, "march", 5) && kernel[5] >= '2' && kernel[5] <= '4') {
      const bool rev = kernel[6] == 'r';  // "march3r": da_alt -> da (the direction of the second pass of a level)
      const bool pl = kernel[6] == 'p';   // "march4p": the pass with the prolongation (coarse = level 1)
      if (pl) launch_relax_march(m->st, m->opt, nullptr, m->da_alt[0], m->res[0], m->sg[0], m->nl, m->rc[0], 0, kernel[5] - '0', m->walls, m->opt.march_rows, nullptr,
                                 m->da[1], &m->sg[m->nlev > 1 ? 1 : 0], nullptr, 1);
      else launch_relax_march(m->st, m->opt, rev ? m->da_alt[0] : m->da[0], rev ? m->da[0] : m->da_alt[0], m->res[0], m->sg[0], m->nl, m->rc[0], 1,
                              kernel[5] - '0', m->walls, m->opt.march_rows);
    } else if (!strcmp(kernel, "block2")) {
      launch_relax_block2(m->st, m->opt, m->da[0], nullptr, m->sg[0], m->res[0], m->da_alt[0], m->sg[0], m->nl, m->rc[0], m->walls, 1);
    } else if (!strcmp(kernel, "block2p")) {
      launch_relax_block2(m->st, m->opt, m->da[0], m->da[1], m->sg[1], m->res[0], m->da_alt[0], m->sg[0], m->nl, m->rc[0], m->walls, 1);
    } else if (!strcmp(kernel, "rhs")) {
      RhsPass ps{MSOM_Q, MSOM_DQ, 1};
      rhs_terms(m, ps);
    } else if (!strcmp(kernel, "resid_correct")) {
      residual2(m, 1, m->f[MSOM_Q], SC_RES1, 0);
    } else if (!strcmp(kernel, "resid_restrict")) {
      residual2(m, 2 | 4, m->f[MSOM_Q], SC_RES1, 1);
    } else if (!strcmp(kernel, "red_prolong")) {
      launch_relax_red_prolong(m->st, m->opt, m->da[0], m->da[1], m->sg[1], m->res[0], m->S[0], m->sg[0], m->nl, m->rc[0], m->uniformS, m->walls);
    } else if (!strcmp(kernel, "rhs_adv")) {
      RhsPass ps{MSOM_Q, MSOM_DQ, 1, MSOM_QPRED, MSOM_Q, 1e-9};
      rhs_terms(m, ps);
    } else if (!strcmp(kernel, "advance")) {
      launch_advance(m->st, m->f[MSOM_QPRED], m->f[MSOM_Q], m->f[MSOM_DQ], nullptr, m->g, m->nl, 1e-9, 0.);
    } else if (!strcmp(kernel, "modes_project")) {   // in place on the staging buffer, in the form the handle holds
      launch_modes_project(m->st, m->staging, m->staging, m->modes_md, modes_mc(m), m->g, m->nl, modes_layers(m), 1);
    } else if (!strcmp(kernel, "modes_energy")) {
      modes_energy_launch(m);
    } else if (!strcmp(kernel, "spec_rows")) {
      launch_spec_rows(m->st, spec_in_nat(m, SPEC_IN_UV, m->f[MSOM_PSI], nullptr), m->nx, m->ny, spec_cnt, m->spc_z, m->spc_tw, std::max(m->nx, m->ny));
    } else if (!strcmp(kernel, "spec_transpose")) {
      launch_spec_transpose(m->st, m->spc_z, m->spc_zt, m->nx, m->ny, spec_cnt);
    } else if (!strcmp(kernel, "spec_cols")) {
      launch_spec_cols(m->st, m->spc_zt, m->nx, m->ny, spec_cnt, SPEC_SUM, pow(D, 4), m->spc_v, nullptr, m->spc_tw, std::max(m->nx, m->ny));
    } else if (!strcmp(kernel, "spec_shells")) {
      spec_batch_1d(m, spec_cnt);
    }
  };
  for (int k = 0; k < 3; k++) one();
  HIPCHK(hipEventRecord(a, m->st));
  for (int k = 0; k < reps; k++) one();
  HIPCHK(hipEventRecord(b, m->st));
  HIPCHK(hipEventSynchronize(b));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, a, b));
  *avg_ms = ms / reps;
  m->res_ready = -1;   // "rhs_adv" goes through rhs_terms, which arms it for MSOM_QPRED again: the handle leaves a measurement disarmed
  hipEventDestroy(a);
  hipEventDestroy(b);
  return MSOM_OK;
}
