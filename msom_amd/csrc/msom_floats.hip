// msom_floats.hip -- Lagrangian floats advected with the model's RK2 stages (include/msom_floats.h): the
// msom_floats_* entry points and the hook rk_stage calls behind each of its two tendency passes.  Arithmetic: floats_inl.h; kernels:
// kernels_floats.hip.
#include "msom_host.h"

#include "../../include/msom_floats.h"

struct FloatsState {
  int n = 0;
  double *buf = nullptr;               // x, y, xh, yh and two output arrays of the by-hand calls, n doubles each
  int *layer = nullptr;
  unsigned long long *cnt = nullptr;   // clamped, lost
  int staged = 0;                      // a stage 1 since msom_floats_begin or the last stage 2
  // trajectory buffer [cap][2][n]; times on the host
  double *rec = nullptr;
  int every = 1, cap = 0, nrec = 0;
  long steps = 0, dropped = 0;         // stage-2 hooks seen since msom_floats_record; records that found the buffer full
  std::vector<double> t;
};

static FloatsDev fl_dev(const FloatsState *s) {
  return FloatsDev{s->buf, s->buf + s->n, s->buf + 2 * (size_t)s->n, s->buf + 3 * (size_t)s->n, s->layer, s->cnt};
}
static FloatsGeom fl_geom(const msom *m) {
  return FloatsGeom{m->gnx, m->gny, m->bc == BC_PERIODIC, m->gnx / m->p.L0, m->p.L0, m->p.L0 * m->gny / m->gnx};
}
static const double *fl_pg(const msom *m) { return m->have_pg ? m->f[MSOM_PSIPG] : nullptr; }
static void fl_free(FloatsState *s) {
  if (!s) return;
  if (s->buf) hipFree(s->buf);
  if (s->layer) hipFree(s->layer);
  if (s->cnt) hipFree(s->cnt);
  if (s->rec) hipFree(s->rec);
  delete s;
}

void floats_drop(msom *m) {
  if (!m->fl) return;
  hipStreamSynchronize(m->st);   // a stage may still be running
  fl_free(m->fl);
  m->fl = nullptr;
  m->fl_on = 0;
}

void floats_hook(msom *m, int stage, double tnext) {
  FloatsState *s = m->fl;
  double *rec = nullptr;
  if (stage == 2 && s->rec && ++s->steps % s->every == 0) {
    if (s->nrec < s->cap) {
      rec = s->rec + (size_t)s->nrec++ * 2 * s->n;
      s->t.push_back(tnext);
    } else
      s->dropped++;
  }
  prof_begin(m, m->prof_floats);
  launch_floats_stage(m->st, stage, fl_dev(s), s->n, m->f[MSOM_PSI], fl_pg(m), m->g, fl_geom(m), m->dt, rec);
  prof_end(m, m->prof_floats);
  s->staged = stage == 1;
}

bool floats_param(msom *m, const char *key, double *v) {
  if (strncmp(key, "floats", 6)) return false;
  const FloatsState *s = m->fl;
  const char *k = key + 6;
  if (!*k) *v = s ? s->n : 0;
  else if (!strcmp(k, "_records")) *v = s ? s->nrec : 0;
  else if (!strcmp(k, "_dropped")) *v = s ? (double)s->dropped : 0;
  else if (!strcmp(k, "_clamped") || !strcmp(k, "_lost")) {
    unsigned long long c[2] = {0, 0};
    if (s && (hipStreamSynchronize(m->st) != hipSuccess || hipMemcpy(c, s->cnt, sizeof c, hipMemcpyDeviceToHost) != hipSuccess)) { *v = NAN; return true; }
    *v = (double)c[k[1] == 'l'];
  } else
    return false;
  return true;
}

// what every call checks first: the dialect, the handle, one rank; need: floats begun
static int fl_guard(msom *m, const char *fn, bool need) {
  if (!m) { msom_set_error("%s: null handle", fn); return MSOM_ERR_ARG; }
  if (m->nranks > 1) { msom_set_error("%s: floats that cross tiles are not supported (%d ranks)", fn, m->nranks); return MSOM_ERR_CONFIG; }
  if (need && !m->fl) { msom_set_error("%s: no msom_floats_begin since msom_set_const", fn); return MSOM_ERR_STATE; }
  return MSOM_OK;
}

extern "C" int msom_floats_begin(msom_t *m, int n, const double *x, const double *y, const int *layer) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_begin", false);
  if (r) return r;
  if (n < 1 || !x || !y || !layer) { msom_set_error("msom_floats_begin: n = %d, x, y or layer null", n); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msom_floats_begin before msom_set_const"); return MSOM_ERR_STATE; }
  // the arrays on the host, for the checks
  std::vector<double> hx, hy;
  std::vector<int> hl;
  if (is_device_ptr(x)) { hx.resize(n); HIPCHK(hipMemcpy(hx.data(), x, n * sizeof(double), hipMemcpyDeviceToHost)); x = hx.data(); }
  if (is_device_ptr(y)) { hy.resize(n); HIPCHK(hipMemcpy(hy.data(), y, n * sizeof(double), hipMemcpyDeviceToHost)); y = hy.data(); }
  if (is_device_ptr(layer)) { hl.resize(n); HIPCHK(hipMemcpy(hl.data(), layer, n * sizeof(int), hipMemcpyDeviceToHost)); layer = hl.data(); }
  const FloatsGeom fg = fl_geom(m);
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(x[k]) || !std::isfinite(y[k])) { msom_set_error("msom_floats_begin: float %d at (%g, %g)", k, x[k], y[k]); return MSOM_ERR_ARG; }
    if (!fg.periodic && !(x[k] >= 0 && x[k] <= fg.Lx && y[k] >= 0 && y[k] <= fg.Ly)) {
      msom_set_error("msom_floats_begin: float %d at (%g, %g) outside [0, %g] x [0, %g]", k, x[k], y[k], fg.Lx, fg.Ly);
      return MSOM_ERR_ARG;
    }
    if (layer[k] < 0 || layer[k] >= m->nl) { msom_set_error("msom_floats_begin: float %d in layer %d of %d", k, layer[k], m->nl); return MSOM_ERR_ARG; }
  }
  FloatsState *s = new FloatsState;
  s->n = n;
  const size_t nb = n * sizeof(double);
  if (hipMalloc(&s->buf, 6 * nb) != hipSuccess || hipMalloc(&s->layer, n * sizeof(int)) != hipSuccess ||
      hipMalloc(&s->cnt, 2 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    fl_free(s);
    msom_set_error("msom_floats_begin: no device memory for %d floats", n);
    return MSOM_ERR_HIP;
  }
  floats_drop(m);   // a second begin replaces the first
  m->fl = s;
  m->fl_on = 1;
  HIPCHK(hipMemsetAsync(s->buf, 0, 6 * nb, m->st));
  HIPCHK(hipMemsetAsync(s->cnt, 0, 2 * sizeof(unsigned long long), m->st));
  HIPCHK(hipMemcpyAsync(s->buf, x, nb, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipMemcpyAsync(s->buf + n, y, nb, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipMemcpyAsync(s->layer, layer, n * sizeof(int), hipMemcpyHostToDevice, m->st));
  return sync_stream(m);   // the host copies go out of scope
}

extern "C" int msom_floats_end(msom_t *m) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_end", false);
  if (r) return r;
  floats_drop(m);
  return MSOM_OK;
}

extern "C" int msom_floats_get(msom_t *m, double *x, double *y) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_get", true);
  if (r) return r;
  if (!x || !y) { msom_set_error("msom_floats_get: null array"); return MSOM_ERR_ARG; }
  const FloatsState *s = m->fl;
  HIPCHK(hipMemcpyAsync(x, s->buf, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(y, s->buf + s->n, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

extern "C" int msom_floats_velocity(msom_t *m, double *u, double *v) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_velocity", true);
  if (r) return r;
  if (!u || !v) { msom_set_error("msom_floats_velocity: null array"); return MSOM_ERR_ARG; }
  const FloatsState *s = m->fl;
  double *o0 = s->buf + 4 * (size_t)s->n, *o1 = o0 + s->n;
  launch_floats_interp(m->st, fl_dev(s), s->n, m->f[MSOM_PSI], fl_pg(m), m->g, fl_geom(m), o0, o1);
  HIPCHK(hipMemcpyAsync(u, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(v, o1, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

// a field of nl layers that the handle holds
static int fl_field(msom *m, const char *fn, int field) {
  if (field < 0 || field >= MSOM_NFIELDS || !m->f[field] || m->flayers[field] != m->nl) {
    msom_set_error("%s: field id %d is not a field of %d layers of this handle", fn, field, m->nl);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}

extern "C" int msom_floats_sample(msom_t *m, int field, double *out) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_sample", true);
  if (r || (r = fl_field(m, "msom_floats_sample", field))) return r;
  if (!out) { msom_set_error("msom_floats_sample: null array"); return MSOM_ERR_ARG; }
  const FloatsState *s = m->fl;
  double *o0 = s->buf + 4 * (size_t)s->n;
  launch_floats_interp(m->st, fl_dev(s), s->n, m->f[field], nullptr, m->g, fl_geom(m), o0, nullptr);
  HIPCHK(hipMemcpyAsync(out, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return sync_stream(m);
}

extern "C" int msom_floats_stage(msom_t *m, int stage, double dt) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_stage", true);
  if (r) return r;
  if ((stage != 1 && stage != 2) || !std::isfinite(dt)) { msom_set_error("msom_floats_stage: stage %d, dt = %g", stage, dt); return MSOM_ERR_ARG; }
  FloatsState *s = m->fl;
  if (stage == 2 && !s->staged) { msom_set_error("msom_floats_stage: stage 2 without a stage 1 before it"); return MSOM_ERR_STATE; }
  launch_floats_stage(m->st, stage, fl_dev(s), s->n, m->f[MSOM_PSI], fl_pg(m), m->g, fl_geom(m), dt, nullptr);
  s->staged = stage == 1;
  return sync_stream(m);
}

extern "C" int msom_floats_record(msom_t *m, int every, int capacity) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_record", true);
  if (r) return r;
  if (every < 1 || capacity < 1) { msom_set_error("msom_floats_record: every = %d, capacity = %d", every, capacity); return MSOM_ERR_ARG; }
  FloatsState *s = m->fl;
  HIPCHK(hipStreamSynchronize(m->st));   // a stage may still be writing a record
  double *rec = nullptr;
  HIPCHK(hipMalloc(&rec, (size_t)capacity * 2 * s->n * sizeof(double)));
  if (s->rec) hipFree(s->rec);
  s->rec = rec;
  s->every = every;
  s->cap = capacity;
  s->nrec = 1;
  s->steps = s->dropped = 0;
  s->t.assign(1, m->t);
  HIPCHK(hipMemcpyAsync(rec, s->buf, 2 * (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, m->st));   // record 0: x then y, as they lie
  return sync_stream(m);
}

extern "C" int msom_floats_track(msom_t *m, int first, int count, double *t, double *x, double *y) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_track", true);
  if (r) return r;
  const FloatsState *s = m->fl;
  if (!s->rec) { msom_set_error("msom_floats_track: no msom_floats_record since msom_floats_begin"); return MSOM_ERR_STATE; }
  if (first < 0 || count < 1 || first > s->nrec - count) {
    msom_set_error("msom_floats_track: records %d .. %d of %d", first, first + count - 1, s->nrec);
    return MSOM_ERR_ARG;
  }
  for (int k = 0; t && k < count; k++) t[k] = s->t[first + k];
  const size_t nb = s->n * sizeof(double);
  const double *src = s->rec + (size_t)first * 2 * s->n;
  if (x) HIPCHK(hipMemcpy2DAsync(x, nb, src, 2 * nb, nb, count, hipMemcpyDefault, m->st));
  if (y) HIPCHK(hipMemcpy2DAsync(y, nb, src + s->n, 2 * nb, nb, count, hipMemcpyDefault, m->st));
  return sync_stream(m);
}

extern "C" int msom_floats_dbg_ghosted(msom_t *m, int field, double *out) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_dbg_ghosted", false);
  if (r || (r = fl_field(m, "msom_floats_dbg_ghosted", field))) return r;
  if (!out) { msom_set_error("msom_floats_dbg_ghosted: null array"); return MSOM_ERR_ARG; }
  const size_t w = (size_t)(m->nx + 2) * sizeof(double), h = m->ny + 2;
  for (int l = 0; l < m->nl; l++)
    HIPCHK(hipMemcpy2DAsync(out + (size_t)l * h * (m->nx + 2), w, m->f[field] + nat_idx(m->g, l, -1, -1), m->g.pitch * sizeof(double), w, h,
                            hipMemcpyDefault, m->st));
  return sync_stream(m);
}
