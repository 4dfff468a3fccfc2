// msom_diag.hip -- diagnostics on the device: running statistics and msom_time_filter (time_filter msqg/qg.h:491-507), vertical normal
// modes (msqg/eigmode.h; products of msqg/qg.h:117-157), wavenumber spectra and spectral fluxes (msqg/scripts/fftlib.py).
#include "msom_host.h"

// ------------------------------------------------------------------ running statistics on the device, time_filter (msqg/qg.h:491-507)

void stats_drop(msom *m) {
  for (int k = 0; k < MSOM_ST_NACC; k++) {
    if (m->stats.s[k]) hipFree(m->stats.s[k]);
    m->stats.s[k] = nullptr;
  }
  if (m->stats_W) hipFree(m->stats_W);
  if (m->stats_qme) hipFree(m->stats_qme);
  m->stats_W = m->stats_qme = nullptr;
  m->stats_mask = 0;
  m->stats_count = m->stats_ndev = 0;
}
// one sample of the handle's psi and q: weight *w_dev (device scalar) or w
void stats_sample(msom *m, const double *w_dev, double w) {
  launch_stats_acc(m->st, m->stats_mask, m->f[MSOM_PSI], m->f[MSOM_Q], m->stats, m->g, m->nl, w_dev, w, 2. * (m->p.L0 / m->gnx), m->stats_W);
}
#define NEED_STATS(m, fn)                                                                   \
  do {                                                                                      \
    if (!(m)->const_set || !(m)->stats_mask) {                                              \
      msom_set_error(fn ": no msom_stats_begin since msom_set_const");                      \
      return MSOM_ERR_STATE;                                                                \
    }                                                                                       \
  } while (0)

extern "C" int msom_stats_begin(msom_t *m, unsigned mask) {
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  if (mask == 0 || mask >> MSOM_ST_NACC) { msom_set_error("msom_stats_begin: mask 0x%x", mask); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msom_stats_begin before msom_set_const"); return MSOM_ERR_STATE; }
  HIPCHK(hipStreamSynchronize(m->st));   // a sample of an earlier mask may still be running
  const size_t bytes = m->g.ls * m->nl * sizeof(double);
  for (int k = 0; k < MSOM_ST_NACC; k++) {
    const bool want = (mask >> k) & 1u;
    if (!want && m->stats.s[k]) { HIPCHK(hipFree(m->stats.s[k])); m->stats.s[k] = nullptr; }
    if (want && !m->stats.s[k]) HIPCHK(hipMalloc(&m->stats.s[k], bytes));
    if (want) HIPCHK(hipMemsetAsync(m->stats.s[k], 0, bytes, m->st));
  }
  if (!m->stats_W) HIPCHK(hipMalloc(&m->stats_W, sizeof(double)));
  HIPCHK(hipMemsetAsync(m->stats_W, 0, sizeof(double), m->st));
  m->stats_mask = mask;
  m->stats_count = m->stats_ndev = 0;
  return sync_stream(m);
}

extern "C" int msom_stats_accumulate(msom_t *m, double w) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  if (!std::isfinite(w)) { msom_set_error("msom_stats_accumulate: w = %g", w); return MSOM_ERR_ARG; }
  NEED_STATS(m, "msom_stats_accumulate");
  stats_sample(m, nullptr, w);
  return m->sticky;
}

extern "C" int msom_stats_weight(msom_t *m, double *W) {
  MSQG_ONLY(m);
  if (!m || !W) return MSOM_ERR_ARG;
  NEED_STATS(m, "msom_stats_weight");
  HIPCHK(hipMemcpyAsync(W, m->stats_W, sizeof(double), hipMemcpyDeviceToHost, m->st));
  return sync_stream(m);
}

extern "C" int msom_stats_get(msom_t *m, int which, double *out) {
  MSQG_ONLY(m);
  if (!m || !out) return MSOM_ERR_ARG;
  const size_t n = (size_t)m->nl * m->nx * m->ny;
  if (which == MSOM_ST_QME) {
    if (!m->const_set || !m->stats_qme) { msom_set_error("msom_stats_get: no msom_time_filter since msom_set_const"); return MSOM_ERR_STATE; }
    launch_unpack(m->st, m->stats_qme, m->staging, m->g, m->nl);
    HIPCHK(hipMemcpyAsync(out, m->staging, n * sizeof(double), hipMemcpyDefault, m->st));
    return sync_stream(m);
  }
  unsigned need;
  int sa = -1;
  if (which >= 0 && which < MSOM_ST_NACC) need = 1u << which;
  else if (which == MSOM_ST_EKE) need = 1u << MSOM_ST_PSI | 1u << (sa = MSOM_ST_KE);
  else if (which == MSOM_ST_UQ_EDDY) need = 1u << MSOM_ST_PSI | 1u << MSOM_ST_Q | 1u << (sa = MSOM_ST_UQ);
  else if (which == MSOM_ST_VQ_EDDY) need = 1u << MSOM_ST_PSI | 1u << MSOM_ST_Q | 1u << (sa = MSOM_ST_VQ);
  else { msom_set_error("msom_stats_get: unknown id %d", which); return MSOM_ERR_ARG; }
  NEED_STATS(m, "msom_stats_get");
  if ((m->stats_mask & need) != need) { msom_set_error("msom_stats_get: id %d needs accumulators 0x%x, the mask is 0x%x", which, need, m->stats_mask); return MSOM_ERR_ARG; }
  double W = 0;
  int r = msom_stats_weight(m, &W);
  if (r) return r;
  if (W == 0) { msom_set_error("msom_stats_get: the sum of the weights is 0"); return MSOM_ERR_STATE; }
  // the mean goes into the scratch field MSOM_TMP (layers and boundary condition of psi)
  launch_stats_mean(m->st, m->f[MSOM_TMP], m->stats.s[sa < 0 ? which : MSOM_ST_PSI], m->stats_W, m->g, m->nl);
  if (sa < 0) return download(m, MSOM_TMP, out);
  if ((r = fill_bc(m, MSOM_TMP))) return r;   // boundary() on the copy of the mean psi: collective on tiles
  launch_stats_derive(m->st, m->staging, m->f[MSOM_TMP], m->stats.s[sa], m->stats.s[MSOM_ST_Q], m->stats_W, m->g, m->nl, which,
                      2. * (m->p.L0 / m->gnx));
  HIPCHK(hipMemcpyAsync(out, m->staging, n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

// time_filter, msqg/qg.h:491-507 (alpha_f = dt / tau_f; qo_me starts from the zeros of a freshly created field)
extern "C" int msom_time_filter(msom_t *m, double dt) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  if (!std::isfinite(dt)) { msom_set_error("msom_time_filter: dt = %g", dt); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msom_time_filter before msom_set_const"); return MSOM_ERR_STATE; }
  if (!m->stats_qme) {
    const size_t bytes = m->g.ls * m->nl * sizeof(double);
    HIPCHK(hipMalloc(&m->stats_qme, bytes));
    HIPCHK(hipMemsetAsync(m->stats_qme, 0, bytes, m->st));
  }
  launch_time_filter(m->st, m->stats_qme, m->f[MSOM_Q], m->g, m->nl, dt / m->tau_f);
  return sync_stream(m);
}

// ------------------------------------------------------------------ vertical normal modes (msqg/eigmode.h; products of msqg/qg.h:117-157)

void modes_drop(msom *m) {
  if (m->modes_md) hipFree(m->modes_md);
  m->modes_md = nullptr;
  helm_drop_pyramid(m);
  m->modes_ready = m->modes_compact = 0;
}
ModesLayers modes_layers(const msom *m) {
  ModesLayers l = {};
  for (int k = 0; k < m->nl; k++) l.dhf[k] = m->dhf[k];
  for (int k = 0; k < m->nl - 1; k++) l.dhc[k] = m->dhc[k];
  return l;
}
const ModeCoef *modes_mc(const msom *m) { return m->modes_compact ? &m->modes_mc : nullptr; }

extern "C" int msom_modes_compute(msom_t *m) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  NEED_CONST(m);
  const int nl = m->nl, na = nl * nl + nl;
  const int compact = m->modes_compact_opt != 0 && m->fr_uniform;
  modes_drop(m);
  if (!m->modes_flag) HIPCHK(hipMalloc(&m->modes_flag, sizeof(int)));
  if (!m->modes_dev) HIPCHK(hipMalloc(&m->modes_dev, sizeof(ModeCoef)));
  HIPCHK(hipMemsetAsync(m->modes_flag, 0, sizeof(int), m->st));
  int r;
  if (compact) {   // the same kernel on a one-column grid: cell (0, 0) of S
    r = launch_modes_eig(m->st, m->f[MSOM_S], m->g, nl, 1, 1, m->modes_dev, 1, 0, modes_layers(m), m->modes_flag);
  } else {
    const size_t bytes = (size_t)na * m->g.ls * sizeof(double);
    HIPCHK(hipMalloc(&m->modes_md, bytes));
    HIPCHK(hipMemsetAsync(m->modes_md, 0, bytes, m->st));
    r = launch_modes_eig(m->st, m->f[MSOM_S], m->g, nl, m->nx, m->ny, m->modes_md, m->g.ls, 1, modes_layers(m), m->modes_flag);
  }
  if (r) { modes_drop(m); msom_set_error("msom_modes_compute: no kernel for nl = %d", nl); return MSOM_ERR_CONFIG; }
  int flag = 0;
  double h[MSOM_MAXNL * MSOM_MAXNL + MSOM_MAXNL];
  HIPCHK(hipMemcpyAsync(&flag, m->modes_flag, sizeof(int), hipMemcpyDeviceToHost, m->st));
  if (compact) HIPCHK(hipMemcpyAsync(h, m->modes_dev, na * sizeof(double), hipMemcpyDeviceToHost, m->st));
  if ((r = sync_stream(m))) { modes_drop(m); return r; }
  if (flag) {
    modes_drop(m);
    if (flag & MODES_BAD_S) msom_set_error("msom_modes_compute: S = (Fr/Ro)^2 is not positive and finite on every interface: the spectrum is degenerate");
    else if (flag & MODES_WEAK)
      msom_set_error("msom_modes_compute: an interface is too weakly stratified for fp64 to separate the first baroclinic mode from the barotropic "
                     "one (lambda_1 <= 8 nl eps lambda_max): neither its sign nor the barotropic vector is determined");
    else msom_set_error("msom_modes_compute: the Jacobi iteration did not converge within %d sweeps", MODES_MAXSWEEP);
    return MSOM_ERR_CONFIG;
  }
  if (compact) {
    memset(&m->modes_mc, 0, sizeof m->modes_mc);
    for (int k = 0; k < nl * nl; k++) m->modes_mc.m2l[k] = h[k];
    for (int k = 0; k < nl; k++) m->modes_mc.ibu[k] = h[nl * nl + k];
  }
  m->modes_compact = compact;
  m->modes_ready = 1;
  return MSOM_OK;
}

extern "C" int msom_modes_layers(msom_t *m, int which) {
  MSQG_ONLY(m);
  if (!m || which < 0 || which >= MSOM_MD_N) return MSOM_ERR_ARG;
  NEED_MODES(m, "msom_modes_layers");
  return which == MSOM_MD_IBU || which == MSOM_MD_RD ? m->nl : m->nl * m->nl;
}

extern "C" int msom_modes_get(msom_t *m, int which, double *out) {
  MSQG_ONLY(m);
  if (!m || which < 0 || which >= MSOM_MD_N || !out) return MSOM_ERR_ARG;
  NEED_MODES(m, "msom_modes_get");
  const int nl = m->nl, n = which == MSOM_MD_IBU || which == MSOM_MD_RD ? nl : nl * nl;
  const size_t cells = (size_t)m->nx * m->ny;
  for (int first = 0; first < n; first += nl) {   // the staging buffer holds nl arrays
    const int cnt = std::min(nl, n - first);
    if (launch_modes_get(m->st, m->staging, m->modes_md, modes_mc(m), m->g, nl, modes_layers(m), which, first, cnt)) return MSOM_ERR_CONFIG;
    HIPCHK(hipMemcpyAsync(out + first * cells, m->staging, cnt * cells * sizeof(double), hipMemcpyDefault, m->st));
  }
  return sync_stream(m);
}

extern "C" int msom_modes_project(msom_t *m, int to_modes, const double *in, double *out) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  if (!m || !in || !out) return MSOM_ERR_ARG;
  NEED_MODES(m, "msom_modes_project");
  const size_t bytes = (size_t)m->nl * m->nx * m->ny * sizeof(double);
  if (is_device_ptr(in) && is_device_ptr(out)) {   // in place on the caller's arrays, queued on the stream and not waited for
    if (launch_modes_project(m->st, in, out, m->modes_md, modes_mc(m), m->g, m->nl, modes_layers(m), to_modes != 0)) return MSOM_ERR_CONFIG;
    return m->sticky;
  }
  HIPCHK(hipMemcpyAsync(m->staging, in, bytes, hipMemcpyDefault, m->st));
  if (launch_modes_project(m->st, m->staging, m->staging, m->modes_md, modes_mc(m), m->g, m->nl, modes_layers(m), to_modes != 0)) return MSOM_ERR_CONFIG;
  HIPCHK(hipMemcpyAsync(out, m->staging, bytes, hipMemcpyDefault, m->st));
  return sync_stream(m);
}

// the launch of msom_modes_energy: the 2 nl sums of this tile into modes_dev
int modes_energy_launch(msom *m) {
  if (!m->modes_partial) HIPCHK(hipMalloc(&m->modes_partial, (size_t)2 * MSOM_MAXNL * modes_energy_stride(m->g) * sizeof(double)));
  if (launch_modes_energy(m->st, m->f[MSOM_PSI], m->modes_md, modes_mc(m), m->g, m->nl, modes_layers(m), m->modes_partial, m->modes_dev,
                          m->p.L0 / m->gnx))
    return MSOM_ERR_CONFIG;
  return MSOM_OK;
}
extern "C" int msom_modes_energy(msom_t *m, double *ke, double *pe) {
  MSQG_ONLY(m);
  if (!m || (!ke && !pe)) return MSOM_ERR_ARG;
  NEED_MODES(m, "msom_modes_energy");
  const int nl = m->nl;
  int r = modes_energy_launch(m);
  if (r) return r;
  double *dst[2] = {ke, pe};
  for (int part = 0; part < 2; part++) {   // nl sums at a time through the scalar slots (summed over the tiles there)
    HIPCHK(hipMemcpyAsync(m->d_scal + SC_LSUM, m->modes_dev + part * nl, nl * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    if ((r = reduce_scal(m, SC_LSUM, nl, RED_SUM))) return r;
    if (dst[part]) for (int k = 0; k < nl; k++) dst[part][k] = m->h_scal[SC_LSUM + k];
  }
  return sync_stream(m);
}

extern "C" int msom_modes_set_rd(msom_t *m, int mode) {
  if (m) m->res_ready = -1;   // nothing cached from psi and q outlives a call that may change them or the solver path
  MSQG_ONLY(m);
  if (!m || mode < 1 || mode > m->nl - 1) return MSOM_ERR_ARG;
  NEED_MODES(m, "msom_modes_set_rd");
  if (launch_modes_rd(m->st, m->f[MSOM_RD], m->modes_md, modes_mc(m), m->g, m->nl, mode)) return MSOM_ERR_CONFIG;
  fill_bc(m, MSOM_RD);   // what msom_set_field(MSOM_RD) does after its pack
  m->wv_ready = 0;
  return sync_stream(m);
}

// ------------------------------------------------------------------ wavenumber spectra and spectral fluxes (msqg/scripts/fftlib.py)

static bool spec_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
// nbins and the points per bin from the integer rule of include/msom.h, on the quarter plane with weights; no device
extern "C" int msom_spec_layout(int nx, int ny, int *nbins, long *count) {
  if (!spec_pow2(nx) || !spec_pow2(ny) || std::min(nx, ny) < SPEC_MINN || std::max(nx, ny) > 32768) {
    msom_set_error("msom_spec_layout: %d x %d: both sides must be powers of two, 8 .. 32768", nx, ny);
    return MSOM_ERR_CONFIG;
  }
  const int nmax = std::max(nx, ny), sx = nmax / nx, sy = nmax / ny, nb = nmax / 2 - 2, hx = nx / 2, hy = ny / 2;
  if (nbins) *nbins = nb;
  if (!count) return MSOM_OK;
  for (int r = 0; r < nb; r++) count[r] = 0;
  for (int i = 0; i <= hx; i++) {
    const long wi = (i == 0 || i == hx) ? 1 : 2;   // +-i; -nx/2 has no partner
    int s = i * sx;                                 // floor(sqrt(R2)) at j = 0, then followed upwards
    for (int j = 0; j <= hy; j++) {
      const long w = wi * ((j == 0 || j == hy) ? 1 : 2);
      const long R2 = (long)(i * sx) * (i * sx) + (long)(j * sy) * (j * sy);
      while ((long)(s + 1) * (s + 1) <= R2) s++;
      if (s < nb) count[s] += w;
      if ((long)s * s == R2 && s >= 1 && s - 1 < nb) count[s - 1] += w;   // on the circle of radius s: also the bin below
    }
  }
  return MSOM_OK;
}

void spec_drop(msom *m) {
  for (void *p : {(void *)m->spc_z, (void *)m->spc_zt, (void *)m->spc_tw, (void *)m->spc_v, (void *)m->spc_te, (void *)m->spc_res, (void *)m->spc_hin,
                  (void *)m->spc_o2d})
    if (p) hipFree(p);
  m->spc_z = m->spc_zt = m->spc_tw = nullptr;
  m->spc_v = m->spc_te = m->spc_res = m->spc_hin = m->spc_o2d = nullptr;
  m->spc_batch = 0;
  m->spc_bytes = 0;
}
// the guards every handle call shares: argument, dialect, tiling, state, size -- in that order
int spec_guard(msom *m, const char *fn) {
  if (m->nranks > 1) { msom_set_error("%s: the spectra run on a single tile, this handle is one of %d", fn, m->nranks); return MSOM_ERR_CONFIG; }
  if (!m->const_set) { msom_set_error("%s: call msom_set_const first", fn); return MSOM_ERR_STATE; }
  if (!spec_pow2(m->nx) || !spec_pow2(m->ny) || std::min(m->nx, m->ny) < SPEC_MINN || std::max(m->nx, m->ny) > SPEC_MAXN) {
    msom_set_error("%s: %d x %d: both sides must be powers of two, %d .. %d", fn, m->nx, m->ny, SPEC_MINN, SPEC_MAXN);
    return MSOM_ERR_CONFIG;
  }
  return MSOM_OK;
}
#define SPEC_SCRATCH_CAP ((size_t)1 << 30)   // work arrays of one batch of layers: 4096^2 goes layer by layer (576 MiB), 2048^2 seven at a time
int spec_ensure(msom *m) {
  if (m->spc_batch) return MSOM_OK;
  if (spec_prepare_device()) { msom_set_error("msom_spec: the device refuses the line kernels' %d KiB of LDS", (int)(2 * spec_line_len(SPEC_MAXN) * 16 / 1024)); return MSOM_ERR_HIP; }
  const int nx = m->nx, ny = m->ny, nmax = std::max(nx, ny);
  const size_t cells = (size_t)nx * ny, vcells = (size_t)(nx / 2 + 1) * ny;
  const size_t per_layer = cells * 2 * sizeof(double2) + vcells * sizeof(double);
  const int batch = (int)std::min<size_t>(MSOM_MAXNL, std::max<size_t>(1, SPEC_SCRATCH_CAP / per_layer));
  int nbins = 0;
  m->spc_count.assign(nmax / 2, 0);
  msom_spec_layout(nx, ny, &nbins, m->spc_count.data());
  m->spc_count.resize(nbins);
  m->spc_smax = (int)floor(sqrt(2. * (nmax / 2) * (double)(nmax / 2)));
  while ((long)m->spc_smax * m->spc_smax > 2L * (nmax / 2) * (nmax / 2)) m->spc_smax--;
  while ((long)(m->spc_smax + 1) * (m->spc_smax + 1) <= 2L * (nmax / 2) * (nmax / 2)) m->spc_smax++;
  const size_t bz = batch * cells * sizeof(double2), bv = batch * vcells * sizeof(double), btw = (size_t)(nmax / 2) * sizeof(double2),
               bte = (size_t)batch * 2 * (m->spc_smax + 1) * sizeof(double), bres = (size_t)batch * 2 * nbins * sizeof(double);
  if (hipMalloc(&m->spc_z, bz) != hipSuccess || hipMalloc(&m->spc_zt, bz) != hipSuccess || hipMalloc(&m->spc_v, bv) != hipSuccess ||
      hipMalloc(&m->spc_tw, btw) != hipSuccess || hipMalloc(&m->spc_te, bte) != hipSuccess || hipMalloc(&m->spc_res, bres) != hipSuccess) {
    (void)hipGetLastError();
    spec_drop(m);
    msom_set_error("msom_spec: no device memory for the work arrays (%zu bytes)", 2 * bz + bv + btw + bte + bres);
    return MSOM_ERR_HIP;
  }
  std::vector<double2> tw(nmax / 2);
  for (int t = 0; t < nmax / 2; t++) {
    const long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)t / (long double)nmax;
    tw[t] = make_double2((double)cosl(a), (double)sinl(a));
  }
  HIPCHK(hipMemcpy(m->spc_tw, tw.data(), btw, hipMemcpyHostToDevice));
  m->spc_batch = batch;
  m->spc_bytes = 2 * bz + bv + btw + bte + bres;
  return MSOM_OK;
}
static int spec_nbins(const msom *m) { return std::max(m->nx, m->ny) / 2 - 2; }
SpecIn spec_in_nat(const msom *m, int mode, const double *a, const double *b) {
  SpecIn in = {};
  in.a = a; in.b = b; in.mode = mode;
  in.off = nat_idx(m->g, 0, 0, 0); in.ls = m->g.ls; in.pitch = m->g.pitch;
  const double D = m->p.L0 / m->gnx;
  in.D2 = 2. * D; in.rD2 = 1. / (2. * D);
  for (int k = 0; k < m->nl - 1 && k < MSOM_MAXNL; k++) in.dhc[k] = m->dhc[k];
  return in;
}
// the passes of one batch: layers l0 .. l0 + cnt - 1 of `in` into spc_v (and the shifted plane into o2d when it is not null)
void spec_batch_2d(msom *m, const SpecIn &in, int cnt, int kind, double *o2d) {
  const double D = m->p.L0 / m->gnx;
  const int nt = std::max(m->nx, m->ny);
  launch_spec_rows(m->st, in, m->nx, m->ny, cnt, m->spc_z, m->spc_tw, nt);
  launch_spec_transpose(m->st, m->spc_z, m->spc_zt, m->nx, m->ny, cnt);
  launch_spec_cols(m->st, m->spc_zt, m->nx, m->ny, cnt, kind, (D * D) * (D * D), m->spc_v, o2d, m->spc_tw, nt);
}
void spec_batch_1d(msom *m, int cnt) {
  const double D = m->p.L0 / m->gnx;
  launch_spec_shells(m->st, m->spc_v, m->nx, m->ny, cnt, m->spc_smax, m->spc_te);
  launch_spec_final(m->st, m->spc_te, m->spc_smax, spec_nbins(m), cnt, (1. / (m->nx * D)) * (1. / (m->ny * D)), m->spc_res);
}
// `layers` layers of `in` (AB with caller's arrays: ua / ub host or device, contiguous; otherwise the handle's fields).  out2d: the caller's
// [layers][ny][nx] or null; spec / flux: host [layers][nbins] or null (spec already 2 pi kr sum / count).  Synchronises.
static int spec_run(msom *m, SpecIn in, const double *ua, const double *ub, int layers, int kind, double *out2d, double *spec, double *flux) {
  int r = spec_ensure(m);
  if (r) return r;
  const int nb = spec_nbins(m), batch = m->spc_batch;
  const size_t cells = (size_t)m->nx * m->ny;
  const bool a_host = ua && !is_device_ptr(ua), b_host = ub && !is_device_ptr(ub), o_host = out2d && !is_device_ptr(out2d);
  if ((a_host || b_host) && !m->spc_hin) {
    HIPCHK(hipMalloc(&m->spc_hin, 2 * batch * cells * sizeof(double)));
    m->spc_bytes += 2 * batch * cells * sizeof(double);
  }
  if (o_host && !m->spc_o2d) {
    HIPCHK(hipMalloc(&m->spc_o2d, batch * cells * sizeof(double)));
    m->spc_bytes += batch * cells * sizeof(double);
  }
  std::vector<double> h((size_t)layers * 2 * nb);
  for (int l0 = 0; l0 < layers; l0 += batch) {
    const int cnt = std::min(batch, layers - l0);
    SpecIn bi = in;
    bi.l0 = l0;
    if (ua) {   // the caller's arrays: this batch starts at layer 0 of what the kernel is given
      bi.l0 = 0;
      bi.a = ua + l0 * cells;
      if (a_host) {
        HIPCHK(hipMemcpyAsync(m->spc_hin, ua + l0 * cells, cnt * cells * sizeof(double), hipMemcpyHostToDevice, m->st));
        bi.a = m->spc_hin;
      }
      bi.b = ub ? ub + l0 * cells : nullptr;
      if (b_host) {
        HIPCHK(hipMemcpyAsync(m->spc_hin + batch * cells, ub + l0 * cells, cnt * cells * sizeof(double), hipMemcpyHostToDevice, m->st));
        bi.b = m->spc_hin + batch * cells;
      }
    }
    spec_batch_2d(m, bi, cnt, kind, !out2d ? nullptr : o_host ? m->spc_o2d : out2d + l0 * cells);
    if (o_host) HIPCHK(hipMemcpyAsync(out2d + l0 * cells, m->spc_o2d, cnt * cells * sizeof(double), hipMemcpyDeviceToHost, m->st));
    if (spec || flux) {
      spec_batch_1d(m, cnt);
      HIPCHK(hipMemcpyAsync(h.data() + (size_t)l0 * 2 * nb, m->spc_res, (size_t)cnt * 2 * nb * sizeof(double), hipMemcpyDeviceToHost, m->st));
    }
    if ((a_host || b_host || o_host) && (r = sync_stream(m))) return r;   // the copy buffers are reused by the next batch
  }
  if ((r = sync_stream(m))) return r;
  const double dk = 1. / (std::max(m->nx, m->ny) * (m->p.L0 / m->gnx));
  for (int l = 0; l < layers; l++)
    for (int k = 0; k < nb; k++) {
      if (spec) spec[(size_t)l * nb + k] = 2. * M_PI * ((k + 1) * dk) * h[((size_t)l * 2) * nb + k] / (double)m->spc_count[k];
      if (flux) flux[(size_t)l * nb + k] = h[((size_t)l * 2 + 1) * nb + k];
    }
  return MSOM_OK;
}
#define SPEC_ENTRY(m, fn)                  \
  do {                                     \
    int g__ = spec_guard(m, fn);           \
    if (g__) return g__;                   \
  } while (0)

extern "C" int msom_spec_bins(msom_t *m) {
  MSQG_ONLY(m);
  if (!m) return MSOM_ERR_ARG;
  SPEC_ENTRY(m, "msom_spec_bins");
  return spec_nbins(m);
}
extern "C" int msom_spec_kr(msom_t *m, double *kr) {
  MSQG_ONLY(m);
  if (!m || !kr) return MSOM_ERR_ARG;
  SPEC_ENTRY(m, "msom_spec_kr");
  const double dk = 1. / (std::max(m->nx, m->ny) * (m->p.L0 / m->gnx));
  for (int k = 0; k < spec_nbins(m); k++) kr[k] = (k + 1) * dk;
  return MSOM_OK;
}
static SpecIn spec_in_user(const msom *m) {
  SpecIn in = {};
  in.mode = SPEC_IN_AB;
  in.off = 0; in.ls = (size_t)m->nx * m->ny; in.pitch = m->nx;
  return in;
}
extern "C" int msom_spec_2d(msom_t *m, const double *a, const double *b, int layers, double *out) {
  MSQG_ONLY(m);
  if (!m || !a || !b || !out || layers < 1) return MSOM_ERR_ARG;
  SPEC_ENTRY(m, "msom_spec_2d");
  return spec_run(m, spec_in_user(m), a, a == b ? nullptr : b, layers, a == b ? SPEC_SUM : SPEC_CROSS, out, nullptr, nullptr);
}
extern "C" int msom_spec_cross(msom_t *m, const double *a, const double *b, int layers, double *spec, double *flux) {
  MSQG_ONLY(m);
  if (!m || !a || !b || layers < 1 || (!spec && !flux)) return MSOM_ERR_ARG;
  SPEC_ENTRY(m, "msom_spec_cross");
  return spec_run(m, spec_in_user(m), a, a == b ? nullptr : b, layers, a == b ? SPEC_SUM : SPEC_CROSS, nullptr, spec, flux);
}
extern "C" int msom_spec_fields(msom_t *m, int field_a, int field_b, double *spec, double *flux) {
  MSQG_ONLY(m);
  if (!m || (!spec && !flux)) return MSOM_ERR_ARG;
  SPEC_ENTRY(m, "msom_spec_fields");
  for (int f : {field_a, field_b})
    if ((f == MSOM_QOF || (f >= MSOM_DE_BF && f < MSOM_NFIELDS)) && ensure_field(m, f)) return MSOM_ERR_HIP;
  if (check_field(m, field_a) || check_field(m, field_b)) return MSOM_ERR_ARG;
  if (m->flayers[field_a] != m->flayers[field_b]) {
    msom_set_error("msom_spec_fields: field %d has %d layers, field %d has %d", field_a, m->flayers[field_a], field_b, m->flayers[field_b]);
    return MSOM_ERR_ARG;
  }
  const bool same = field_a == field_b;
  return spec_run(m, spec_in_nat(m, SPEC_IN_AB, m->f[field_a], same ? nullptr : m->f[field_b]), nullptr, nullptr, m->flayers[field_a],
                  same ? SPEC_SUM : SPEC_CROSS, nullptr, spec, flux);
}
extern "C" int msom_spec_energy(msom_t *m, double *ke, double *pe) {
  MSQG_ONLY(m);
  if (!m || (!ke && !pe)) return MSOM_ERR_ARG;
  SPEC_ENTRY(m, "msom_spec_energy");
  const int nl = m->nl, nb = spec_nbins(m);
  int r;
  if (ke) {   // Z = u + i v: |U|^2 + |V|^2 through the symmetric pair
    if ((r = spec_run(m, spec_in_nat(m, SPEC_IN_UV, m->f[MSOM_PSI], nullptr), nullptr, nullptr, nl, SPEC_SUM, nullptr, ke, nullptr))) return r;
    for (int l = 0; l < nl; l++)
      for (int k = 0; k < nb; k++) ke[(size_t)l * nb + k] = 0.5 * ke[(size_t)l * nb + k] * m->dhf[l];
  }
  if (pe && nl > 1) {
    if ((r = spec_run(m, spec_in_nat(m, SPEC_IN_G, m->f[MSOM_PSI], m->f[MSOM_S]), nullptr, nullptr, nl - 1, SPEC_SUM, nullptr, pe, nullptr))) return r;
    for (int l = 0; l < nl - 1; l++)
      for (int k = 0; k < nb; k++) pe[(size_t)l * nb + k] = 0.5 * pe[(size_t)l * nb + k] * m->dhc[l];
  }
  return MSOM_OK;
}
