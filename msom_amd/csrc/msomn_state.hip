// msomn_state.hip -- lossless checkpoint and bit-exact restart of the vertex-grid model (include/msomn_state.h).
// Same container and the same device pass as msom_state.hip: k_state_rows of kernels_state.hip takes any natural geometry, so the
// vertex fields go through it with the handle's NatGeom (nx = ny = N + 1, no ring, one tile: global offsets 0) and the cell-scalar
// noise with the geometry of cs[0].  Nothing here runs inside msomn_step.
#include <unistd.h>

#include <map>

#include "msomn_host.h"
#include "state_io.h"
#include "state_pipe.h"
#include "../../include/msomn_state.h"

namespace {

enum { NSTATE_DIALECT = 2 };
enum { EVOLVING = 0, CONSTANT = 1 };
enum { F_NOISE = -1, F_ACC0 = -2 };   // not one of m->f: the cell scalar cs[0]; accumulator k of the running statistics is F_ACC0 - k
struct RecName { const char *name; int field, role; };
const RecName NAMES[] = {
    {"psi", MSOMN_PSI, EVOLVING}, {"q", MSOMN_Q, EVOLVING}, {"q_forcing", MSOMN_QFORC, EVOLVING}, {"psi_f", MSOMN_PSIF, EVOLVING},
    {"noise", F_NOISE, EVOLVING}, {"qpred", MSOMN_QPRED, EVOLVING},
    {"mask", MSOMN_MASK, CONSTANT}, {"S2", MSOMN_S2, CONSTANT}, {"S2S", MSOMN_S2S, CONSTANT}, {"bs", MSOMN_BS, CONSTANT},
    {"topo", MSOMN_TOPO, CONSTANT}, {"psi_pg", MSOMN_PSIPG, CONSTANT}, {"q_forcing_3d", MSOMN_QFORC3D, CONSTANT},
    // the accumulators of msomn_stats_begin, in the order of MSOM_ST_PSI .. MSOM_ST_VQ
    {"st_psi", F_ACC0 - MSOM_ST_PSI, EVOLVING}, {"st_q", F_ACC0 - MSOM_ST_Q, EVOLVING}, {"st_psi2", F_ACC0 - MSOM_ST_PSI2, EVOLVING},
    {"st_q2", F_ACC0 - MSOM_ST_Q2, EVOLVING}, {"st_ke", F_ACC0 - MSOM_ST_KE, EVOLVING}, {"st_uq", F_ACC0 - MSOM_ST_UQ, EVOLVING},
    {"st_vq", F_ACC0 - MSOM_ST_VQ, EVOLVING}};
const char *acc_name(int k) {
  for (const RecName &n : NAMES)
    if (n.field == F_ACC0 - k) return n.name;
  return nullptr;
}
bool is_acc(const RecName &n) { return n.field <= F_ACC0; }
const RecName *find_name(const char *name) {
  for (const RecName &n : NAMES)
    if (!strcmp(n.name, name)) return &n;
  return nullptr;
}
// the scalars of record `stats` (written only by a handle with stats_mask != 0)
enum { SS_MASK, SS_COUNT, SS_EVERY, SS_ON, SS_W, SS_SAMPLES, SS_N };
// the scalars of record `node`
enum { NS_SEED, NS_DRAW, NS_CORRECTOR, NS_NBAR, NS_PG, NS_TOPO, NS_F3D, NS_SQG, NS_DT, NS_COUNT };

struct Item { const char *name; const double *dev; int layers; NatGeom g; };
struct Scal { const char *name; std::vector<double> v; };

NatGeom rec_geom(const msomn *m, const RecName &n) { return n.field == F_NOISE ? cell_geom(m->N) : m->g; }
int rec_layers(const msomn *m, const RecName &n) { return n.field == F_NOISE ? 1 : is_acc(n) ? m->nl : m->fl[n.field]; }

StateChunk chunk_of(const NatGeom &g, int layer, int y0, int rows) {
  StateChunk c;
  c.g = g; c.ring = 0; c.layer = layer; c.y0 = y0; c.rows = rows; c.ox = 0; c.oy = 0;
  c.gW = g.nx; c.gH = g.ny; c.sx0 = 0; c.sw = g.nx;
  return c;
}
struct Rows { int layer, y0, rows; };
std::vector<Rows> chunks_of(const Pipe &pp, const NatGeom &g, int layers) {
  int rows_max = (int)std::min<size_t>(pp.cap / g.nx, (size_t)g.ny);
  if (rows_max < 1) rows_max = 1;
  std::vector<Rows> cs;
  for (int l = 0; l < layers; l++)
    for (int y = 0; y < g.ny; y += rows_max) cs.push_back({l, y, std::min(rows_max, g.ny - y)});
  return cs;
}
int pipe_init(Pipe &pp, const msomn *m) {   // a layer, at most CHUNK_DOUBLES (and never less than a row)
  size_t cap = (size_t)m->g.nx * m->g.ny;
  if (cap > CHUNK_DOUBLES) cap = std::max(CHUNK_DOUBLES, (size_t)m->g.nx);
  return pp.init(cap, 1);
}
int digest_read(msomn *m, Pipe &pp, uint64_t *out) {
  HIPCHK(hipMemcpyAsync(pp.h_dig, pp.dig, sizeof(unsigned long long), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  *out = pp.h_dig[0];
  return MSOM_OK;
}

// ---- save: the record's rows go through the two chunk buffers -- while chunk c is packed and copied to the host on the second stream,
// chunk c - 1 is written -- and the digest ends in pp.dig[0]
int save_record(msomn *m, Pipe &pp, const Item &it, FILE *fp, bool *io_ok) {
  const std::vector<Rows> cs = chunks_of(pp, it.g, it.layers);
  const int n = (int)cs.size();
  for (int c = 0; c <= n; c++) {
    if (c < n) {
      const int b = c & 1;
      launch_state_pack(m->st, it.dev, pp.d[b], chunk_of(it.g, cs[c].layer, cs[c].y0, cs[c].rows), pp.dig);
      HIPCHK(hipEventRecord(pp.packed[b], m->st));
      HIPCHK(hipStreamWaitEvent(pp.s2, pp.packed[b], 0));
      HIPCHK(hipMemcpyAsync(pp.h[b], pp.d[b], (size_t)cs[c].rows * it.g.nx * sizeof(double), hipMemcpyDeviceToHost, pp.s2));
      HIPCHK(hipEventRecord(pp.copied[b], pp.s2));
    }
    if (c >= 1) {
      const int b = (c - 1) & 1;
      HIPCHK(hipEventSynchronize(pp.copied[b]));   // the next pack into d[b] is launched after this: no event needed the other way
      const size_t cnt = (size_t)cs[c - 1].rows * it.g.nx;
      if (*io_ok && fwrite(pp.h[b], sizeof(double), cnt, fp) != cnt) *io_ok = false;
    }
  }
  return MSOM_OK;
}

void collect(msomn *m, unsigned flags, const double *run6, std::vector<Item> &items, std::vector<Scal> &scal) {
  auto fld = [&](const char *name, int id) { items.push_back({name, m->f[id], m->fl[id], m->g}); };
  scal.push_back({"time", {m->t, m->dt, m->previous, m->tnext, (double)m->iter}});
  // without mgstats.sum, as for msom_t: a loaded handle reports sum = 0 until its next solve
  scal.push_back({"mgstats", {(double)m->mg.i, m->mg.resb, m->mg.resa, (double)m->mg.nrelax}});
  scal.push_back({"node", {(double)m->seed, (double)m->noise_draw, (double)m->corrector_step, (double)m->nbar, (double)m->pg_set, (double)m->topo_set,
                           (double)m->forcing_3d, (double)m->sqg, m->p.DT}});
  if (run6) scal.push_back({"run", std::vector<double>(run6, run6 + 6)});
  fld("psi", MSOMN_PSI);   // through the live pointer: the out-of-place passes swap it with psi_alt
  fld("q", MSOMN_Q);
  fld("q_forcing", MSOMN_QFORC);
  if (m->nbar > 0) fld("psi_f", MSOMN_PSIF);
  if (m->stochastic && m->cnlev > 0) items.push_back({"noise", m->cs[0], 1, m->cg[0]});
  // between the two stages of a step (only a stochastic handle knows that it is: corrector_step) the second update reads the predictor;
  // at a step boundary QPRED is scratch and is not written
  if (m->stochastic && m->corrector_step) fld("qpred", MSOMN_QPRED);
  if (m->stats_mask) {   // a handle without statistics writes the records it always wrote
    scal.push_back({"stats", {(double)m->stats_mask, (double)m->stats_count, (double)m->stats_every, (double)m->stats_on, m->stats_W,
                              (double)m->stats_samples}});
    for (int k = 0; k < MSOM_ST_NACC; k++)
      if (m->stats.s[k]) items.push_back({acc_name(k), m->stats.s[k], m->nl, m->g});
  }
  if (flags & MSOM_STATE_CONSTANTS) {
    fld("mask", MSOMN_MASK);
    if (m->nl > 1) fld("S2", MSOMN_S2);
    if (m->sqg) { fld("S2S", MSOMN_S2S); fld("bs", MSOMN_BS); }
    if (m->topo_set) fld("topo", MSOMN_TOPO);
    if (m->pg_set) fld("psi_pg", MSOMN_PSIPG);
    if (m->forcing_3d) fld("q_forcing_3d", MSOMN_QFORC3D);
  }
}

}  // namespace

int nstate_save_run(msomn *m, const char *path, unsigned flags, const double *run6) {
  if (!m || !path) { msom_set_error("msomn_state_save: null argument"); return MSOM_ERR_ARG; }
  if (int rt = nt_refuse(m, "msomn_state_save")) return rt;
  if (!m->const_set) { msom_set_error("msomn_state_save: call msomn_set_const first"); return MSOM_ERR_STATE; }
  if (m->stochastic && m->noise_mode == 0) {
    msom_set_error("msomn_state_save: a stochastic run with noise_mode = 0 draws from libc's process-wide rand(), whose state cannot be "
                   "saved: run with noise_mode = 1");
    return MSOM_ERR_CONFIG;
  }
  HIPCHK(hipStreamSynchronize(m->st));
  std::vector<Item> items;
  std::vector<Scal> scal;
  collect(m, flags, run6, items, scal);
  Pipe pp;
  int r = pipe_init(pp, m);
  if (r) return r;
  const std::string tmp = std::string(path) + ".tmp";
  FILE *fp = fopen(tmp.c_str(), "wb");
  bool io_ok = fp != nullptr;
  msom_sfile sf;
  memset(&sf, 0, sizeof sf);
  sf.version = MSOM_STATE_VERSION; sf.dialect = NSTATE_DIALECT; sf.nx = sf.ny = (uint32_t)(m->N + 1); sf.nl = (uint32_t)m->nl;
  sf.stochastic = (uint32_t)(m->stochastic != 0); sf.noise_mode = (uint32_t)m->noise_mode; sf.flag_topo = (uint32_t)(m->topo_set != 0);
  sf.nrec = (uint32_t)(items.size() + scal.size());
  sf.params_len = (uint32_t)m->params_text.size();
  sf.params = const_cast<char *>(m->params_text.c_str());
  if (fp && msom_swrite_header(fp, &sf)) io_ok = false;
  uint64_t dsum = 0;
  for (const Scal &s : scal) {
    msom_srec rec;
    memset(&rec, 0, sizeof rec);
    snprintf(rec.name, sizeof rec.name, "%s", s.name);
    rec.kind = MSOM_SK_SCALARS; rec.layers = (uint32_t)s.v.size(); rec.ny = rec.nx = 1;
    rec.nbytes = 8 * (uint64_t)s.v.size();
    rec.digest = msom_state_digest(s.v.data(), s.v.size(), 0);
    dsum += rec.digest;
    if (fp && io_ok && (msom_swrite_rechdr(fp, &rec) || fwrite(s.v.data(), sizeof(double), s.v.size(), fp) != s.v.size())) io_ok = false;
  }
  for (const Item &it : items) {
    msom_srec rec;
    memset(&rec, 0, sizeof rec);
    snprintf(rec.name, sizeof rec.name, "%s", it.name);
    rec.kind = MSOM_SK_FIELD; rec.layers = (uint32_t)it.layers; rec.ny = (uint32_t)it.g.ny; rec.nx = (uint32_t)it.g.nx;
    rec.nbytes = 8 * msom_srec_count(&rec);
    const long at = fp && io_ok ? ftell(fp) : -1;
    if (fp && io_ok && msom_swrite_rechdr(fp, &rec)) io_ok = false;   // digest 0 for now: it is known after the payload
    HIPCHK(hipMemsetAsync(pp.dig, 0, sizeof(unsigned long long), m->st));
    uint64_t d = 0;
    if (!(r = save_record(m, pp, it, fp, &io_ok))) r = digest_read(m, pp, &d);
    if (r) { if (fp) { fclose(fp); unlink(tmp.c_str()); } return r; }
    rec.digest = d;
    dsum += d;
    if (fp && io_ok && (fseek(fp, at, SEEK_SET) || msom_swrite_rechdr(fp, &rec) || fseek(fp, 0, SEEK_END))) io_ok = false;
  }
  if (fp && io_ok && msom_swrite_trailer(fp, dsum)) io_ok = false;
  if (fp && fclose(fp)) io_ok = false;
  if (io_ok && rename(tmp.c_str(), path)) io_ok = false;
  if (!io_ok) {
    unlink(tmp.c_str());
    msom_set_error("msomn_state_save: cannot write %s", path);
    return MSOM_ERR_IO;
  }
  return MSOM_OK;
}

extern "C" int msomn_state_save(msomn_t *m, const char *path, unsigned flags) { return nstate_save_run(m, path, flags, nullptr); }

extern "C" int msomn_state_dbg_flip(msomn_t *m, long element) {
  if (!m) return MSOM_ERR_ARG;
  m->state_flip = element;
  return MSOM_OK;
}

// ---- load

namespace {

struct Loaded {   // a field record verified on the device, not yet in the handle
  const RecName *n = nullptr;
  const msom_srec *rec = nullptr;
  NatGeom g;
  double *nat = nullptr;
};
struct Temps {
  std::vector<Loaded> v;
  ~Temps() { for (Loaded &l : v) if (l.nat) (void)hipFree(l.nat); }
  const Loaded *find(const char *name) const {
    for (const Loaded &l : v) if (!strcmp(l.n->name, name)) return &l;
    return nullptr;
  }
};

int read_scalars(const char *path, const msom_srec *r, std::vector<double> &v) {
  v.resize(r->layers);
  FILE *fp = fopen(path, "rb");
  const bool ok = fp && !fseek(fp, r->offset, SEEK_SET) && fread(v.data(), sizeof(double), v.size(), fp) == v.size();
  if (fp) fclose(fp);
  if (!ok) { msom_set_error("state file %s: short read in record %s", path, r->name); return MSOM_ERR_IO; }
  if (msom_state_digest(v.data(), v.size(), 0) != r->digest) { msom_set_error("state file %s: record %s: digest mismatch", path, r->name); return MSOM_ERR_IO; }
  return MSOM_OK;
}

// the record's rows: file -> pinned chunk -> device chunk (second stream) -> natural layout, two chunks in flight; then the digest of
// what the natural array holds
int upload_record(msomn *m, Pipe &pp, FILE *fp, const char *path, const Loaded &l, bool flip, uint64_t *digest) {
  const NatGeom &g = l.g;
  const std::vector<Rows> cs = chunks_of(pp, g, (int)l.rec->layers);
  for (int c = 0; c < (int)cs.size(); c++) {
    const int b = c & 1;
    const size_t cnt = (size_t)cs[c].rows * g.nx;
    if (c >= 2) HIPCHK(hipEventSynchronize(pp.packed[b]));   // the unpack of chunk c - 2 has read d[b]; its copy has left h[b] before that
    if (fseek(fp, l.rec->offset + (long)((((size_t)cs[c].layer * g.ny + cs[c].y0) * g.nx) * sizeof(double)), SEEK_SET) ||
        fread(pp.h[b], sizeof(double), cnt, fp) != cnt) {
      msom_set_error("state file %s: short read in record %s", path, l.rec->name);
      return MSOM_ERR_IO;
    }
    HIPCHK(hipMemcpyAsync(pp.d[b], pp.h[b], cnt * sizeof(double), hipMemcpyHostToDevice, pp.s2));
    HIPCHK(hipEventRecord(pp.copied[b], pp.s2));
    HIPCHK(hipStreamWaitEvent(m->st, pp.copied[b], 0));
    launch_state_unpack(m->st, pp.d[b], l.nat, chunk_of(g, cs[c].layer, cs[c].y0, cs[c].rows));
    HIPCHK(hipEventRecord(pp.packed[b], m->st));
  }
  if (flip) {
    const size_t e = (size_t)m->state_flip % ((size_t)g.nx * g.ny);
    launch_state_flip(m->st, l.nat, nat_idx(g, 0, (int)(e / g.nx), (int)(e % g.nx)));
  }
  HIPCHK(hipMemsetAsync(pp.dig, 0, sizeof(unsigned long long), m->st));
  for (int k = 0; k < (int)l.rec->layers; k++) launch_state_digest(m->st, l.nat, chunk_of(g, k, 0, g.ny), pp.dig);
  return digest_read(m, pp, digest);
}

double *target_ptr(msomn *m, const RecName &n) {
  if (is_acc(n)) return m->stats.s[F_ACC0 - n.field];
  return n.field == F_NOISE ? (m->cnlev > 0 ? m->cs[0] : nullptr) : m->f[n.field];
}

}  // namespace

extern "C" int msomn_state_load(msomn_t *m, const char *path) {
  if (int rt = nt_refuse(m, "msomn_state_load")) return rt;
  if (!m || !path) { msom_set_error("msomn_state_load: null argument"); return MSOM_ERR_ARG; }
  msom_sfile sf;
  int r = msom_sfile_open(path, &sf, 0);   // the whole structure: header, every record header against the file size, trailer
  if (r) return r;
  struct Free { msom_sfile *s; ~Free() { msom_sfile_free(s); } } free_sf{&sf};
  const bool flip = m->state_flip >= 0;
  // ---- everything that can be refused is refused before the handle changes
  if ((int)sf.dialect != NSTATE_DIALECT || (int)sf.nx != m->N + 1 || (int)sf.ny != m->N + 1 || (int)sf.nl != m->nl || sf.nptr != 0) {
    msom_set_error("msomn_state_load: %s holds dialect %u, grid %u x %u, nl %u; the handle is dialect %d (vertex model), %d x %d vertices, nl %d", path,
                   sf.dialect, sf.nx, sf.ny, sf.nl, (int)NSTATE_DIALECT, m->N + 1, m->N + 1, m->nl);
    return MSOM_ERR_CONFIG;
  }
  if ((int)sf.stochastic != (m->stochastic != 0) || (sf.stochastic && (int)sf.noise_mode != m->noise_mode)) {
    msom_set_error("msomn_state_load: %s was saved with stochastic %u, noise_mode %u; the handle has %d, %d", path, sf.stochastic, sf.noise_mode,
                   m->stochastic != 0, m->noise_mode);
    return MSOM_ERR_CONFIG;
  }
  if (m->const_set && m->stochastic && m->cnlev == 0) {
    msom_set_error("msomn_state_load: stochastic was switched on after msomn_set_const: call msomn_set_const again first");
    return MSOM_ERR_CONFIG;
  }
  std::map<std::string, std::vector<double>> sc;
  Temps tmp;
  for (uint32_t k = 0; k < sf.nrec; k++) {
    const msom_srec *rec = &sf.rec[k];
    if (rec->kind == MSOM_SK_SCALARS) {
      static const struct { const char *name; uint32_t n; } known[] = {{"time", 5}, {"mgstats", 4}, {"node", NS_COUNT}, {"run", 6}, {"stats", SS_N}};
      bool ok = false;
      for (const auto &kn : known) ok |= !strcmp(kn.name, rec->name) && rec->layers == kn.n;
      if (!ok) { msom_set_error("msomn_state_load: %s: scalar record %s with %u numbers is not one this library reads", path, rec->name, rec->layers); return MSOM_ERR_CONFIG; }
      if ((r = read_scalars(path, rec, sc[rec->name]))) return r;
      continue;
    }
    const RecName *n = find_name(rec->name);
    Loaded l;
    l.n = n; l.rec = rec;
    if (n) l.g = rec_geom(m, *n);
    if (!n || tmp.find(rec->name) || rec->ring || (int)rec->layers != rec_layers(m, *n) || (int)rec->ny != l.g.ny || (int)rec->nx != l.g.nx ||
        (n->field == F_NOISE && !m->stochastic)) {
      msom_set_error("msomn_state_load: %s: record %s [%u][%u][%u] has no place in this handle", path, rec->name, rec->layers, rec->ny, rec->nx);
      return MSOM_ERR_CONFIG;
    }
    tmp.v.push_back(l);
  }
  unsigned file_mask = 0;
  {  // the statistics: a mask msomn_stats_begin would take, and exactly the accumulators it selects
    unsigned recs = 0;
    for (const Loaded &l : tmp.v) if (is_acc(*l.n)) recs |= 1u << (F_ACC0 - l.n->field);
    if (sc.count("stats")) {
      const double fm = sc["stats"][SS_MASK];
      if (!(fm >= 1) || fm >= (double)(1u << MSOM_ST_NACC) || fm != floor(fm)) { msom_set_error("msomn_state_load: %s: statistics mask %g", path, fm); return MSOM_ERR_CONFIG; }
      file_mask = (unsigned)fm;
    }
    if (recs != file_mask) { msom_set_error("msomn_state_load: %s: accumulator records 0x%x, the mask of record `stats` is 0x%x", path, recs, file_mask); return MSOM_ERR_CONFIG; }
  }
  if (!sc.count("node") || !sc.count("time")) { msom_set_error("msomn_state_load: %s has no record `%s`", path, sc.count("node") ? "time" : "node"); return MSOM_ERR_CONFIG; }
  const std::vector<double> &ns = sc["node"];
  const bool file_const = tmp.find("mask") != nullptr, take_const = !m->const_set && file_const;
  if ((ns[NS_SQG] != 0) != (m->sqg != 0) ||
      (m->const_set && ((ns[NS_TOPO] != 0) != (m->topo_set != 0) || (ns[NS_PG] != 0) != (m->pg_set != 0) || (ns[NS_F3D] != 0) != (m->forcing_3d != 0)))) {
    msom_set_error("msomn_state_load: %s was saved with sqg %g, topo_set %g, pg_set %g, forcing_3d %g; the handle has %d, %d, %d, %d", path, ns[NS_SQG],
                   ns[NS_TOPO], ns[NS_PG], ns[NS_F3D], m->sqg, m->topo_set, m->pg_set, m->forcing_3d);
    return MSOM_ERR_CONFIG;
  }
  {  // msomn_set_const clamps DT; a handle without constants will be clamped on the way
    const double dt_handle = m->const_set ? m->p.DT : node_clamped_dt(m);
    if (ns[NS_DT] != dt_handle) {
      msom_set_error("msomn_state_load: %s was saved with DT = %.17g after the clamps of msomn_set_const; the handle has %.17g", path, ns[NS_DT], dt_handle);
      return MSOM_ERR_CONFIG;
    }
  }
  {  // the records this load needs
    std::vector<const char *> need = {"psi", "q", "q_forcing"};
    if (sf.stochastic) need.push_back("noise");
    if (ns[NS_NBAR] > 0) need.push_back("psi_f");
    if (sf.stochastic && ns[NS_CORRECTOR] != 0) need.push_back("qpred");
    if (take_const) {
      if (m->nl > 1) need.push_back("S2");
      if (m->sqg) { need.push_back("S2S"); need.push_back("bs"); }
      if (ns[NS_TOPO] != 0) need.push_back("topo");
      if (ns[NS_PG] != 0) need.push_back("psi_pg");
      if (ns[NS_F3D] != 0) need.push_back("q_forcing_3d");
    }
    for (const char *name : need)
      if (!tmp.find(name)) { msom_set_error("msomn_state_load: %s has no record `%s`", path, name); return MSOM_ERR_CONFIG; }
  }
  HIPCHK(hipStreamSynchronize(m->st));
  // ---- every field into a spare natural array (pads: the target's own, or zero), its digest recomputed there on the device
  {
    Pipe pp;
    if ((r = pipe_init(pp, m))) return r;
    FILE *fp = fopen(path, "rb");
    if (!fp) { msom_set_error("state file %s not found", path); return MSOM_ERR_IO; }
    struct Close { FILE *f; ~Close() { fclose(f); } } close_fp{fp};
    bool first = true;
    for (Loaded &l : tmp.v) {
      const size_t bytes = l.g.ls * l.rec->layers * sizeof(double);
      HIPCHK(hipMalloc(&l.nat, bytes));
      const double *cur = target_ptr(m, *l.n);
      if (cur) HIPCHK(hipMemcpyAsync(l.nat, cur, bytes, hipMemcpyDeviceToDevice, m->st));
      else HIPCHK(hipMemsetAsync(l.nat, 0, bytes, m->st));
      uint64_t d = 0;
      r = upload_record(m, pp, fp, path, l, flip && first, &d);
      first = false;
      if (r) { m->state_flip = -1; (void)hipStreamSynchronize(pp.s2); (void)hipStreamSynchronize(m->st); return r; }
      if (d != l.rec->digest) {
        m->state_flip = -1;
        msom_set_error("msomn_state_load: %s: record %s: the device holds digest %016llx, the file says %016llx", path, l.rec->name,
                       (unsigned long long)d, (unsigned long long)l.rec->digest);
        return MSOM_ERR_IO;
      }
    }
  }
  m->state_flip = -1;
  // ---- commit.  Constants first: the stored ones as they are and what follows from them (node_const_derived), or msomn_set_const on
  // what the handle holds if the file brings none; then the evolving state (msomn_set_const overwrites q)
  auto put = [&](const Loaded &l, double *dst) -> int {
    HIPCHK(hipMemcpyAsync(dst, l.nat, l.g.ls * l.rec->layers * sizeof(double), hipMemcpyDeviceToDevice, m->st));
    return MSOM_OK;
  };
  if (take_const) {
    for (const Loaded &l : tmp.v)
      if (l.n->role == CONSTANT && (r = put(l, m->f[l.n->field]))) return r;
    m->pg_set = ns[NS_PG] != 0; m->topo_set = ns[NS_TOPO] != 0; m->forcing_3d = ns[NS_F3D] != 0;
    if ((r = node_const_derived(m))) return r;
    m->const_set = 1;
  } else if (!m->const_set && (r = msomn_set_const(m))) return r;
  if (file_mask) {   // the arrays the file holds, allocated as msomn_stats_begin allocates them; then its counters
    if (file_mask != m->stats_mask && (r = msomn_stats_begin(m, file_mask))) return r;
    const std::vector<double> &s = sc["stats"];
    m->stats_count = (long)s[SS_COUNT]; m->stats_every = (int)s[SS_EVERY] < 1 ? 1 : (int)s[SS_EVERY]; m->stats_on = s[SS_ON] != 0;
    m->stats_W = s[SS_W]; m->stats_samples = (long)s[SS_SAMPLES];
  }
  for (const Loaded &l : tmp.v) {
    if (l.n->role == CONSTANT) continue;
    // psi through the live pointer.  The buffer that is not psi (psi_alt, if the handle has one yet) stays as it is: k_n_rhs_pre and
    // k_n_correct_residual write every vertex of it before anything reads it, and its pad cells are zero in both buffers
    if ((r = put(l, target_ptr(m, *l.n)))) return r;
    if (l.n->field == F_NOISE) node_noise_ghosts(m);
  }
  const std::vector<double> &tv = sc["time"];
  m->t = tv[0]; m->dt = tv[1]; m->previous = tv[2]; m->tnext = tv[3]; m->iter = (int)tv[4];
  if (sc.count("mgstats")) {
    const std::vector<double> &v = sc["mgstats"];
    m->mg.i = (int)v[0]; m->mg.resb = v[1]; m->mg.resa = v[2]; m->mg.sum = 0.; m->mg.nrelax = (int)v[3];
  }
  m->seed = (unsigned)ns[NS_SEED]; m->noise_draw = (unsigned)ns[NS_DRAW]; m->corrector_step = (int)ns[NS_CORRECTOR]; m->nbar = (int)ns[NS_NBAR];
  m->run_loaded = sc.count("run") ? 1 : 0;
  if (m->run_loaded) std::copy(sc["run"].begin(), sc["run"].end(), m->run_ev);
  m->wv_ready = 0;   // the filter's pyramids follow mask and S2: rebuilt by the next msomn_wavelet_filter
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(m->st));
  return MSOM_OK;
}

extern "C" msomn_t *msomn_create_from_state(const char *path) {
  if (!path) { msom_set_error("msomn_create_from_state: null path"); return nullptr; }
  msom_sfile sf;
  if (msom_sfile_open(path, &sf, 0)) return nullptr;
  if (sf.dialect != NSTATE_DIALECT) {
    msom_set_error("msomn_create_from_state: %s holds dialect %u, a cell-centred model: use msom_create_from_state", path, sf.dialect);
    msom_sfile_free(&sf);
    return nullptr;
  }
  if (!msom_sfile_find(&sf, "mask")) {
    msom_set_error("msomn_create_from_state: %s was saved without MSOM_STATE_CONSTANTS: create the handle, set its constants and call msomn_state_load", path);
    msom_sfile_free(&sf);
    return nullptr;
  }
  msomn_t *m = msomn_create_str(sf.params);
  int r = m ? MSOM_OK : MSOM_ERR_CONFIG;
  if (m && sf.stochastic) {
    const msom_srec *nr = msom_sfile_find(&sf, "node");
    std::vector<double> v;
    r = msomn_set_option(m, "stochastic", 1);
    if (!r) r = msomn_set_option(m, "noise_mode", sf.noise_mode);
    if (!r && nr && nr->layers == NS_COUNT && !(r = read_scalars(path, nr, v))) m->seed = (unsigned)v[NS_SEED];   // not the option: it calls srand
  }
  msom_sfile_free(&sf);
  if (m && !r) r = msomn_state_load(m, path);
  if (m && r) {
    const std::string keep = msom_last_error();
    msomn_destroy(m);
    msom_set_error("%s", keep.c_str());
    return nullptr;
  }
  return m;
}
