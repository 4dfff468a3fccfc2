// msomn_floats.hip -- Lagrangian floats of the vertex-grid model, advected with the model's RK2 stages (include/msomn_floats.h,
// DESIGN.md section 8l): the msomn_floats_* entry points and the hook msomn_step (msom_node.hip) calls behind its first update and
// behind its final advance.  Arithmetic: the vertex part of floats_inl.h; kernels: kernels_node_floats.hip.  One tile only: a handle
// of more than one tile answers every call with MSOM_ERR_CONFIG.
#include <cmath>

#include "msomn_host.h"

#include "../../include/msomn_floats.h"

bool is_device_ptr(const void *p);   // msom_diag.hip

struct NFloatsState {
  int n = 0;
  double *buf = nullptr;               // x, y, xh, yh and two output arrays of the by-hand calls, n doubles each
  int *layer = nullptr;
  unsigned long long *cnt = nullptr;   // clamped, lost, and the scratch word of "floats_on_land"
  int staged = 0;                      // a stage 1 since msomn_floats_begin or the last stage 2
  // trajectory buffer [cap][2 or 3][n]; times on the host
  double *rec = nullptr;
  int every = 1, cap = 0, nrec = 0;
  int field = -1;                      // the field recorded along the trajectories (< 0: positions only)
  long steps = 0, dropped = 0;         // stage-2 hooks seen since msomn_floats_record; records that found the buffer full
  std::vector<double> t;
};

static FloatsDev nfl_dev(const NFloatsState *s) {
  return FloatsDev{s->buf, s->buf + s->n, s->buf + 2 * (size_t)s->n, s->buf + 3 * (size_t)s->n, s->layer, s->cnt};
}
static FloatsGeom nfl_geom(const msomn *m) { return FloatsGeom{m->N, m->N, 0, m->N / m->p.L0, m->p.L0, m->p.L0}; }
static const double *nfl_pg(const msomn *m) { return m->pg_set ? m->f[MSOMN_PSIPG] : nullptr; }
static size_t nfl_rows(const NFloatsState *s) { return s->field < 0 ? 2 : 3; }
static void nfl_free(NFloatsState *s) {
  if (!s) return;
  for (void *p : {(void *)s->buf, (void *)s->layer, (void *)s->cnt, (void *)s->rec})
    if (p) (void)hipFree(p);
  delete s;
}

void nfloats_drop(msomn *m) {
  if (!m->floats) return;
  (void)hipStreamSynchronize(m->st);   // a stage may still be running
  nfl_free(m->floats);
  m->floats = nullptr;
  m->floats_on = 0;
}

int nfloats_hook(msomn *m, int stage, double tnext) {
  NFloatsState *s = m->floats;
  double *rec = nullptr;
  if (stage == 2 && s->rec && ++s->steps % s->every == 0) {
    if (s->nrec < s->cap) {
      rec = s->rec + (size_t)s->nrec++ * nfl_rows(s) * s->n;
      s->t.push_back(tnext);
    } else
      s->dropped++;
  }
  launch_nfloats_stage(m->st, stage, nfl_dev(s), s->n, m->f[MSOMN_PSI], nfl_pg(m), m->g, nfl_geom(m), m->dt, rec,
                       rec && s->field >= 0 ? m->f[s->field] : nullptr);
  HIPCHK(hipGetLastError());
  s->staged = stage == 1;
  return MSOM_OK;
}

bool nfloats_param(msomn *m, const char *key, double *v) {
  if (strncmp(key, "floats", 6)) return false;
  const NFloatsState *s = m->floats;
  const char *k = key + 6;
  if (!*k) *v = s ? s->n : 0;
  else if (!strcmp(k, "_records")) *v = s ? s->nrec : 0;
  else if (!strcmp(k, "_dropped")) *v = s ? (double)s->dropped : 0;
  else if (!strcmp(k, "_clamped") || !strcmp(k, "_lost") || !strcmp(k, "_on_land")) {
    unsigned long long c[3] = {0, 0, 0};
    *v = NAN;
    if (s) {
      if (k[1] == 'o') {   // counted now, behind whatever the stream still holds
        if (hipMemsetAsync(s->cnt + 2, 0, sizeof(unsigned long long), m->st) != hipSuccess) return true;
        launch_nfloats_on_land(m->st, nfl_dev(s), s->n, m->f[MSOMN_MASK], m->g, nfl_geom(m), s->cnt + 2);
      }
      if (hipStreamSynchronize(m->st) != hipSuccess || hipMemcpy(c, s->cnt, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return true;
    }
    *v = (double)c[k[1] == 'c' ? 0 : k[1] == 'l' ? 1 : 2];
  } else
    return false;
  return true;
}

// what every call checks first: the handle, one tile; need: floats begun
static int nfl_guard(msomn *m, const char *fn, bool need) {
  if (!m) { msom_set_error("%s: null handle", fn); return MSOM_ERR_ARG; }
  if (int r = nt_refuse(m, fn)) return r;
  if (need && !m->floats) { msom_set_error("%s: no msomn_floats_begin since msomn_set_const", fn); return MSOM_ERR_STATE; }
  return MSOM_OK;
}
// a field of nl layers
static int nfl_field(msomn *m, const char *fn, int field) {
  if (field < 0 || field >= MSOMN_NFIELDS || !m->f[field] || m->fl[field] != m->nl) {
    msom_set_error("%s: field id %d is not a field of %d layers of this handle", fn, field, m->nl);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}
static int nfl_sync(msomn *m) {
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

extern "C" int msomn_floats_begin(msomn_t *m, int n, const double *x, const double *y, const int *layer) {
  int r = nfl_guard(m, "msomn_floats_begin", false);
  if (r) return r;
  if (n < 1 || !x || !y || !layer) { msom_set_error("msomn_floats_begin: n = %d, x, y or layer null", n); return MSOM_ERR_ARG; }
  if (!m->const_set) { msom_set_error("msomn_floats_begin before msomn_set_const"); return MSOM_ERR_STATE; }
  // the arrays on the host, for the checks
  std::vector<double> hx, hy;
  std::vector<int> hl;
  if (is_device_ptr(x)) { hx.resize(n); HIPCHK(hipMemcpy(hx.data(), x, n * sizeof(double), hipMemcpyDeviceToHost)); x = hx.data(); }
  if (is_device_ptr(y)) { hy.resize(n); HIPCHK(hipMemcpy(hy.data(), y, n * sizeof(double), hipMemcpyDeviceToHost)); y = hy.data(); }
  if (is_device_ptr(layer)) { hl.resize(n); HIPCHK(hipMemcpy(hl.data(), layer, n * sizeof(int), hipMemcpyDeviceToHost)); layer = hl.data(); }
  const double L0 = m->p.L0;
  for (int k = 0; k < n; k++) {
    if (!std::isfinite(x[k]) || !std::isfinite(y[k])) { msom_set_error("msomn_floats_begin: float %d at (%g, %g)", k, x[k], y[k]); return MSOM_ERR_ARG; }
    if (!(x[k] >= 0 && x[k] <= L0 && y[k] >= 0 && y[k] <= L0)) {
      msom_set_error("msomn_floats_begin: float %d at (%g, %g) outside [0, %g] x [0, %g]", k, x[k], y[k], L0, L0);
      return MSOM_ERR_ARG;
    }
    if (layer[k] < 0 || layer[k] >= m->nl) { msom_set_error("msomn_floats_begin: float %d in layer %d of %d", k, layer[k], m->nl); return MSOM_ERR_ARG; }
  }
  NFloatsState *s = new NFloatsState;
  s->n = n;
  const size_t nb = n * sizeof(double);
  if (hipMalloc(&s->buf, 6 * nb) != hipSuccess || hipMalloc(&s->layer, n * sizeof(int)) != hipSuccess ||
      hipMalloc(&s->cnt, 3 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    nfl_free(s);
    msom_set_error("msomn_floats_begin: no device memory for %d floats", n);
    return MSOM_ERR_HIP;
  }
  nfloats_drop(m);   // a second begin replaces the first
  m->floats = s;
  m->floats_on = 1;
  HIPCHK(hipMemsetAsync(s->buf, 0, 6 * nb, m->st));
  HIPCHK(hipMemsetAsync(s->cnt, 0, 3 * sizeof(unsigned long long), m->st));
  HIPCHK(hipMemcpyAsync(s->buf, x, nb, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipMemcpyAsync(s->buf + n, y, nb, hipMemcpyHostToDevice, m->st));
  HIPCHK(hipMemcpyAsync(s->layer, layer, n * sizeof(int), hipMemcpyHostToDevice, m->st));
  return nfl_sync(m);   // the host copies go out of scope
}

extern "C" int msomn_floats_end(msomn_t *m) {
  int r = nfl_guard(m, "msomn_floats_end", false);
  if (r) return r;
  nfloats_drop(m);
  return MSOM_OK;
}

extern "C" int msomn_floats_get(msomn_t *m, double *x, double *y) {
  int r = nfl_guard(m, "msomn_floats_get", true);
  if (r) return r;
  if (!x || !y) { msom_set_error("msomn_floats_get: null array"); return MSOM_ERR_ARG; }
  const NFloatsState *s = m->floats;
  HIPCHK(hipMemcpyAsync(x, s->buf, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(y, s->buf + s->n, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return nfl_sync(m);
}

extern "C" int msomn_floats_velocity(msomn_t *m, double *u, double *v) {
  int r = nfl_guard(m, "msomn_floats_velocity", true);
  if (r) return r;
  if (!u || !v) { msom_set_error("msomn_floats_velocity: null array"); return MSOM_ERR_ARG; }
  const NFloatsState *s = m->floats;
  double *o0 = s->buf + 4 * (size_t)s->n, *o1 = o0 + s->n;
  launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[MSOMN_PSI], nfl_pg(m), m->g, nfl_geom(m), o0, o1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(u, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  HIPCHK(hipMemcpyAsync(v, o1, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return nfl_sync(m);
}

extern "C" int msomn_floats_sample(msomn_t *m, int field, double *out) {
  int r = nfl_guard(m, "msomn_floats_sample", true);
  if (r || (r = nfl_field(m, "msomn_floats_sample", field))) return r;
  if (!out) { msom_set_error("msomn_floats_sample: null array"); return MSOM_ERR_ARG; }
  const NFloatsState *s = m->floats;
  double *o0 = s->buf + 4 * (size_t)s->n;
  launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[field], nullptr, m->g, nfl_geom(m), o0, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, o0, s->n * sizeof(double), hipMemcpyDefault, m->st));
  return nfl_sync(m);
}

extern "C" int msomn_floats_stage(msomn_t *m, int stage, double dt) {
  int r = nfl_guard(m, "msomn_floats_stage", true);
  if (r) return r;
  if ((stage != 1 && stage != 2) || !std::isfinite(dt)) { msom_set_error("msomn_floats_stage: stage %d, dt = %g", stage, dt); return MSOM_ERR_ARG; }
  NFloatsState *s = m->floats;
  if (stage == 2 && !s->staged) { msom_set_error("msomn_floats_stage: stage 2 without a stage 1 before it"); return MSOM_ERR_STATE; }
  launch_nfloats_stage(m->st, stage, nfl_dev(s), s->n, m->f[MSOMN_PSI], nfl_pg(m), m->g, nfl_geom(m), dt, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  s->staged = stage == 1;
  return nfl_sync(m);
}

extern "C" int msomn_floats_record(msomn_t *m, int every, int capacity, int field) {
  int r = nfl_guard(m, "msomn_floats_record", true);
  if (r) return r;
  if (every < 1 || capacity < 1) { msom_set_error("msomn_floats_record: every = %d, capacity = %d", every, capacity); return MSOM_ERR_ARG; }
  if (field >= 0 && (r = nfl_field(m, "msomn_floats_record", field))) return r;
  NFloatsState *s = m->floats;
  HIPCHK(hipStreamSynchronize(m->st));   // a stage may still be writing a record
  double *rec = nullptr;
  const size_t rows = field < 0 ? 2 : 3;
  HIPCHK(hipMalloc(&rec, (size_t)capacity * rows * s->n * sizeof(double)));
  if (s->rec) (void)hipFree(s->rec);
  s->rec = rec;
  s->every = every;
  s->cap = capacity;
  s->field = field < 0 ? -1 : field;
  s->nrec = 1;
  s->steps = s->dropped = 0;
  s->t.assign(1, m->t);
  // record 0: x then y, as they lie, and the sample of the field at them
  HIPCHK(hipMemcpyAsync(rec, s->buf, 2 * (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, m->st));
  if (field >= 0) {
    launch_nfloats_interp(m->st, nfl_dev(s), s->n, m->f[field], nullptr, m->g, nfl_geom(m), rec + 2 * (size_t)s->n, nullptr);
    HIPCHK(hipGetLastError());
  }
  return nfl_sync(m);
}

extern "C" int msomn_floats_track(msomn_t *m, int first, int count, double *t, double *x, double *y, double *val) {
  int r = nfl_guard(m, "msomn_floats_track", true);
  if (r) return r;
  const NFloatsState *s = m->floats;
  if (!s->rec) { msom_set_error("msomn_floats_track: no msomn_floats_record since msomn_floats_begin"); return MSOM_ERR_STATE; }
  if (first < 0 || count < 1 || first > s->nrec - count) {
    msom_set_error("msomn_floats_track: records %d .. %d of %d", first, first + count - 1, s->nrec);
    return MSOM_ERR_ARG;
  }
  if (val && s->field < 0) { msom_set_error("msomn_floats_track: val given, but msomn_floats_record chose no field"); return MSOM_ERR_ARG; }
  for (int k = 0; t && k < count; k++) t[k] = s->t[first + k];
  const size_t nb = s->n * sizeof(double), rs = nfl_rows(s);
  const double *src = s->rec + (size_t)first * rs * s->n;
  if (x) HIPCHK(hipMemcpy2DAsync(x, nb, src, rs * nb, nb, count, hipMemcpyDefault, m->st));
  if (y) HIPCHK(hipMemcpy2DAsync(y, nb, src + s->n, rs * nb, nb, count, hipMemcpyDefault, m->st));
  if (val) HIPCHK(hipMemcpy2DAsync(val, nb, src + 2 * (size_t)s->n, rs * nb, nb, count, hipMemcpyDefault, m->st));
  return nfl_sync(m);
}
