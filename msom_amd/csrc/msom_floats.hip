// msom_floats.hip -- Lagrangian floats advected with the model's RK2 stages (include/msom_floats.h): the
// msom_floats_* entry points and the hook rk_stage calls behind each of its two tendency passes.  An entry point runs its guard, fills
// the context of the host engine both models share (floats_host.h) from the handle, makes one engine call and ends in sync_stream.
// Arithmetic: floats_inl.h; kernels: kernels_floats.hip.  On tiles (option floats_tiles, "On tiles" in section 8k) every call is
// collective: each rank holds the floats it owns in n slots, a migration pass behind every stage kernel takes them to their new owner,
// readouts are combined over the ranks.
#include "msom_host.h"

#include "../../include/msom_floats.h"

static void fl_bracket(void *h, bool open) { open ? comm_begin((msom *)h) : comm_end((msom *)h); }
static void fl_prof(void *h, int slot, bool begin, hipStream_t st) {
  msom *m = (msom *)h;
  ProfSlot &ps = slot == fh::PROF_STAGE ? m->prof_floats : slot == fh::PROF_EMIGRATE ? m->prof_floats_emig : m->prof_floats_immig;
  begin ? prof_begin(m, ps, st) : prof_end(m, ps, st);
}
static void fl_stage(hipStream_t st, int stage, const FloatsDev &d, int n, const double *psi, const double *pg, const NatGeom &g, const FloatsGeom &fg,
                     double dt, double *rec, const double *, const FloatsTileDev *t) {
  launch_floats_stage(st, stage, d, n, psi, pg, g, fg, dt, rec, t);
}
// what the engine sees of the handle: the migration and gather launches go to st2 inside comm_begin / comm_end, no field is recorded
static fh::Ctx fl_ctx(msom *m) {
  fh::Ctx c{};
  c.model = "msom";
  c.st = m->st; c.cst = m->st2;
  c.comm = m->comm; c.nranks = m->nranks; c.nb = m->nb;
  c.nl = m->nl;
  c.fg = FloatsGeom{m->gnx, m->gny, m->bc == BC_PERIODIC, m->gnx / m->p.L0, m->p.L0, m->p.L0 * m->gny / m->gnx};
  c.tl = FloatsTiling{m->px, m->py, m->ix, m->iy, m->nx, m->ny};
  c.ox = m->ix * m->nx; c.oy = m->iy * m->ny;
  c.g = m->g;
  c.psi = m->f[MSOM_PSI]; c.pg = m->have_pg ? m->f[MSOM_PSIPG] : nullptr;
  c.msg_cap = m->floats.msg_cap; c.ncnt = 4;
  c.stage = fl_stage; c.interp = launch_floats_interp;
  c.h = m; c.bracket = fl_bracket; c.prof = fl_prof;
  return c;
}

void floats_drop(msom *m) {
  if (!m->floats.s) return;
  hipStreamSynchronize(m->st);   // a stage may still be running
  if (m->st2) hipStreamSynchronize(m->st2);
  fh::free_state(m->floats.s);
  m->floats.s = nullptr;
  m->floats.on = 0;
}

void floats_hook(msom *m, int stage, double tnext) { STICKY(m, fh::hook(fl_ctx(m), m->floats.s, stage, m->dt, tnext)); }

bool floats_param(msom *m, const char *key, double *v) { return !strncmp(key, "floats", 6) && fh::param(fl_ctx(m), m->floats, key + 6, v); }

// what every call checks first: the dialect, the handle, one rank or option floats_tiles; need: floats begun
static int fl_guard(msom *m, const char *fn, bool need) {
  if (!m) { msom_set_error("%s: null handle", fn); return MSOM_ERR_ARG; }
  if (m->nranks > 1 && !m->floats.tiles) { msom_set_error("%s: floats that cross tiles are not supported (%d ranks)", fn, m->nranks); return MSOM_ERR_CONFIG; }
  if (need && !m->floats.s) { msom_set_error("%s: no msom_floats_begin since msom_set_const", fn); return MSOM_ERR_STATE; }
  return MSOM_OK;
}
// a field of nl layers that the handle holds
static int fl_field(msom *m, const char *fn, int field) {
  if (field < 0 || field >= MSOM_NFIELDS || !m->f[field] || m->flayers[field] != m->nl) {
    msom_set_error("%s: field id %d is not a field of %d layers of this handle", fn, field, m->nl);
    return MSOM_ERR_ARG;
  }
  return MSOM_OK;
}

extern "C" int msom_floats_begin(msom_t *m, int n, const double *x, const double *y, const int *layer) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_begin", false);
  if (r) return r;
  const fh::Ctx c = fl_ctx(m);
  if ((r = fh::begin_args(c, n, x, y, layer))) return r;
  if (!m->const_set) { msom_set_error("msom_floats_begin before msom_set_const"); return MSOM_ERR_STATE; }
  fh::HostArrays host;
  if ((r = fh::begin_check(c, n, x, y, layer, host))) return r;
  fh::State *s = fh::begin_alloc(c, n);
  if (!s) return MSOM_ERR_HIP;
  floats_drop(m);   // a second begin replaces the first
  m->floats.s = s;
  m->floats.on = 1;
  if ((r = fh::begin_fill(c, s, x, y, layer, host))) return r;
  // The host formed x * idx - 0.5 with two roundings; the product build's kernels fuse it.  A float within an ulp of a cell-centre line
  // may thus belong to the neighbour in the kernels' eyes: one pass by their own rule takes it there (and counts it in floats_migrated)
  if (s->tiled && (r = fh::migrate(c, s, 0))) return r;
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
  if (r || (r = fh::get(fl_ctx(m), m->floats.s, x, y))) return r;
  return sync_stream(m);
}

extern "C" int msom_floats_velocity(msom_t *m, double *u, double *v) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_velocity", true);
  if (r) return r;
  const fh::Ctx c = fl_ctx(m);
  if ((r = fh::interp(c, m->floats.s, "floats_velocity", c.psi, c.pg, true, u, v))) return r;
  return sync_stream(m);
}

extern "C" int msom_floats_sample(msom_t *m, int field, double *out) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_sample", true);
  if (r || (r = fl_field(m, "msom_floats_sample", field))) return r;
  if ((r = fh::interp(fl_ctx(m), m->floats.s, "floats_sample", m->f[field], nullptr, false, out, nullptr))) return r;
  return sync_stream(m);
}

extern "C" int msom_floats_stage(msom_t *m, int stage, double dt) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_stage", true);
  if (r || (r = fh::stage_by_hand(fl_ctx(m), m->floats.s, stage, dt))) return r;
  return sync_stream(m);
}

extern "C" int msom_floats_record(msom_t *m, int every, int capacity) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_record", true);
  if (r || (r = fh::record(fl_ctx(m), m->floats.s, every, capacity, -1, nullptr, m->t))) return r;
  return sync_stream(m);
}

extern "C" int msom_floats_track(msom_t *m, int first, int count, double *t, double *x, double *y) {
  MSQG_ONLY(m);
  int r = fl_guard(m, "msom_floats_track", true);
  if (r || (r = fh::track(fl_ctx(m), m->floats.s, first, count, t, x, y, nullptr))) return r;
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
