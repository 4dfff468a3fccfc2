// msomn_floats.hip -- Lagrangian floats of the vertex-grid model, advected with the model's RK2 stages (include/msomn_floats.h,
// DESIGN.md section 8l): the msomn_floats_* entry points and the hook msomn_step (msom_node.hip) calls behind its first update and
// behind its final advance.  Arithmetic: the vertex part of floats_inl.h; kernels: kernels_node_floats.hip.  On tiles (option
// floats_tiles, "On tiles" in section 8l) every call is collective: each rank holds the floats it owns in n slots, a migration pass
// behind every stage kernel takes them to their new owner (the kernels of kernels_floats.hip), readouts are combined over the ranks.
// Without the option a handle of more than one tile answers every call with MSOM_ERR_CONFIG.  An entry point runs its guard, fills the
// context of the host engine both models share (floats_host.h) from the handle, makes one engine call and waits for the stream.
#include <cmath>

#include "msomn_host.h"

#include "../../include/msomn_floats.h"

// what the engine sees of the handle: everything on the handle's stream, the vertex grid's owner rule, a fifth counter for "floats_on_land"
static fh::Ctx nfl_ctx(msomn *m) {
  fh::Ctx c{};
  const fh::State *s = m->floats.s;
  c.model = "msomn";
  c.st = c.cst = m->st;
  c.comm = m->comm; c.nranks = m->ntiles; c.nb = m->nb;
  c.nl = m->nl;
  c.fg = FloatsGeom{m->N, m->N, 0, m->N / m->p.L0, m->p.L0, m->p.L0};   // the global geometry, on a tile too
  c.tl = FloatsTiling{m->px, m->py, m->rank % m->px, m->rank / m->px, m->g.nx - 1, m->g.ny - 1};
  c.ox = m->ox; c.oy = m->oy;
  c.g = m->g;
  c.psi = m->f[MSOMN_PSI]; c.pg = m->pg_set ? m->f[MSOMN_PSIPG] : nullptr;
  c.rf = s && s->field >= 0 ? m->f[s->field] : nullptr;
  c.msg_cap = m->floats.msg_cap; c.ncnt = 5;
  c.node = true;
  c.stage = launch_nfloats_stage; c.interp = launch_nfloats_interp;
  c.on_land = launch_nfloats_on_land; c.mask = m->f[MSOMN_MASK];
  return c;
}

void nfloats_drop(msomn *m) {
  if (!m->floats.s) return;
  (void)hipStreamSynchronize(m->st);   // a stage may still be running
  fh::free_state(m->floats.s);
  m->floats.s = nullptr;
  m->floats.on = 0;
}

int nfloats_hook(msomn *m, int stage, double tnext) { return fh::hook(nfl_ctx(m), m->floats.s, stage, m->dt, tnext); }

bool nfloats_param(msomn *m, const char *key, double *v) { return !strncmp(key, "floats", 6) && fh::param(nfl_ctx(m), m->floats, key + 6, v); }

// what every call checks first: the handle, one tile or option floats_tiles; need: floats begun
static int nfl_guard(msomn *m, const char *fn, bool need) {
  if (!m) { msom_set_error("%s: null handle", fn); return MSOM_ERR_ARG; }
  if (!m->floats.tiles)
    if (int r = nt_refuse(m, fn)) return r;
  if (need && !m->floats.s) { msom_set_error("%s: no msomn_floats_begin since msomn_set_const", fn); return MSOM_ERR_STATE; }
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
  const fh::Ctx c = nfl_ctx(m);
  const bool tiled = m->ntiles > 1;
  if (!tiled && (r = fh::begin_args(c, n, x, y, layer))) return r;
  if (!m->const_set) { msom_set_error("msomn_floats_begin before msomn_set_const"); return MSOM_ERR_STATE; }
  fh::HostArrays host;
  r = fh::begin_check(c, n, x, y, layer, host);
  if (tiled) {
    // the messages of a pass have a size that follows from n: ranks that do not pass the same n, or of which one refuses its
    // arrays, all leave here, before a float message is posted.  One reduction: max n, max -n, +inf from a rank that refuses
    const double mine[2] = {r ? (double)INFINITY : (double)n, r ? (double)INFINITY : -(double)n};
    HIPCHK(hipMemcpyAsync(m->d_scal + NSC_FLOATS, mine, sizeof mine, hipMemcpyHostToDevice, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    if (int rr = nt_reduce(m, NSC_FLOATS, 2, RED_MAX)) return rr;
    const double hi = m->h_scal[NSC_FLOATS], lo = -m->h_scal[NSC_FLOATS + 1];
    if (!r && hi != lo) {
      if (std::isfinite(hi)) msom_set_error("msomn_floats_begin: n = %d here, %g .. %g over the ranks: every rank passes the same floats", n, lo, hi);
      else msom_set_error("msomn_floats_begin: another rank refuses its arguments");
      return MSOM_ERR_ARG;
    }
  }
  if (r) return r;
  fh::State *s = fh::begin_alloc(c, n);
  if (!s) return MSOM_ERR_HIP;
  nfloats_drop(m);   // a second begin replaces the first
  m->floats.s = s;
  m->floats.on = 1;
  // the host locates with the kernels' own function (no contraction in nfloats_axis, in either build): every float starts on the rank
  // the kernels take for its owner, no pass is needed
  if ((r = fh::begin_fill(c, s, x, y, layer, host))) return r;
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
  if (r || (r = fh::get(nfl_ctx(m), m->floats.s, x, y))) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_velocity(msomn_t *m, double *u, double *v) {
  int r = nfl_guard(m, "msomn_floats_velocity", true);
  if (r) return r;
  const fh::Ctx c = nfl_ctx(m);
  if ((r = fh::interp(c, m->floats.s, "floats_velocity", c.psi, c.pg, true, u, v))) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_sample(msomn_t *m, int field, double *out) {
  int r = nfl_guard(m, "msomn_floats_sample", true);
  if (r || (r = nfl_field(m, "msomn_floats_sample", field))) return r;
  if ((r = fh::interp(nfl_ctx(m), m->floats.s, "floats_sample", m->f[field], nullptr, false, out, nullptr))) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_stage(msomn_t *m, int stage, double dt) {
  int r = nfl_guard(m, "msomn_floats_stage", true);
  if (r || (r = fh::stage_by_hand(nfl_ctx(m), m->floats.s, stage, dt))) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_record(msomn_t *m, int every, int capacity, int field) {
  int r = nfl_guard(m, "msomn_floats_record", true);
  if (r) return r;
  const double *f = nullptr;
  if (every >= 1 && capacity >= 1 && field >= 0) {   // a wrong every or capacity is the engine's to refuse, before the field
    if ((r = nfl_field(m, "msomn_floats_record", field))) return r;
    f = m->f[field];
  }
  if ((r = fh::record(nfl_ctx(m), m->floats.s, every, capacity, field, f, m->t))) return r;
  return nfl_sync(m);
}

extern "C" int msomn_floats_track(msomn_t *m, int first, int count, double *t, double *x, double *y, double *val) {
  int r = nfl_guard(m, "msomn_floats_track", true);
  if (r || (r = fh::track(nfl_ctx(m), m->floats.s, first, count, t, x, y, val))) return r;
  return nfl_sync(m);
}
