// msom_state.hip -- lossless checkpoint and bit-exact restart of a msom_t (include/msom_state.h; format: DESIGN "State file").
// The model state of a handle goes to the file in fp64, field by field through kernels_state.hip; everything in the table of DESIGN
// "State a handle keeps across calls" is dropped by a load and rebuilt by the plain path.  Nothing here runs inside msom_step.
#include "msom_host.h"
#include "state_io.h"
#include "state_xfer.h"
#include "../../include/msom_state.h"

namespace {

enum { T_FIELD = 0, T_ACC = 1, T_QME = 2, T_HELM = 3 };   // where a field record lives in the handle
enum { EVOLVING = 0, CONSTANT = 1 };
struct RecName { const char *name; int target, id, role; };
const RecName NAMES[] = {
    {"psi", T_FIELD, MSOM_PSI, EVOLVING}, {"q", T_FIELD, MSOM_Q, EVOLVING}, {"ptr", T_FIELD, MSOM_PTR, EVOLVING},
    {"qof", T_FIELD, MSOM_QOF, EVOLVING}, {"de_bf", T_FIELD, MSOM_DE_BF, EVOLVING}, {"de_vd", T_FIELD, MSOM_DE_VD, EVOLVING},
    {"de_j1", T_FIELD, MSOM_DE_J1, EVOLVING}, {"de_j2", T_FIELD, MSOM_DE_J2, EVOLVING}, {"de_j3", T_FIELD, MSOM_DE_J3, EVOLVING},
    {"de_ft", T_FIELD, MSOM_DE_FT, EVOLVING}, {"po_mft", T_FIELD, MSOM_PO_MFT, EVOLVING}, {"noise", T_FIELD, MSOM_NOISE, EVOLVING},
    {"bfn_f1", T_FIELD, MSOM_BFN_F1, EVOLVING}, {"bfn_f2", T_FIELD, MSOM_BFN_F2, EVOLVING}, {"bfn_f3", T_FIELD, MSOM_BFN_F3, EVOLVING},
    {"zeta", T_FIELD, MSOM_ZETA, EVOLVING}, {"dq", T_FIELD, MSOM_DQ, EVOLVING}, {"qpred", T_FIELD, MSOM_QPRED, EVOLVING},   // newqg only
    {"st_acc0", T_ACC, 0, EVOLVING}, {"st_acc1", T_ACC, 1, EVOLVING}, {"st_acc2", T_ACC, 2, EVOLVING}, {"st_acc3", T_ACC, 3, EVOLVING},
    {"st_acc4", T_ACC, 4, EVOLVING}, {"st_acc5", T_ACC, 5, EVOLVING}, {"st_acc6", T_ACC, 6, EVOLVING},
    {"st_qme", T_QME, 0, EVOLVING}, {"helm_pm", T_HELM, 0, EVOLVING},
    {"psipg", T_FIELD, MSOM_PSIPG, CONSTANT}, {"fr", T_FIELD, MSOM_FR, CONSTANT}, {"rd", T_FIELD, MSOM_RD, CONSTANT},
    {"qforc", T_FIELD, MSOM_QFORC, CONSTANT}, {"topo", T_FIELD, MSOM_TOPO, CONSTANT}, {"sigma", T_FIELD, MSOM_SIGMA, CONSTANT},
    {"ptr_relax", T_FIELD, MSOM_PTR_RELAX, CONSTANT}, {"bfn_obs", T_FIELD, MSOM_BFN_OBS, CONSTANT}, {"bfn_gain", T_FIELD, MSOM_BFN_GAIN, CONSTANT}};
static_assert(MSOM_ST_NACC == 7, "one st_acc<k> name per accumulator");
const RecName *find_name(const char *name) {
  for (const RecName &n : NAMES)
    if (!strcmp(n.name, name)) return &n;
  return nullptr;
}
// layers of a field record in this handle (0: the handle has no such field)
int target_layers(const msom *m, const RecName &n) {
  if (n.target != T_FIELD) return m->model ? 0 : m->nl;
  if (m->model) return nq_has_field(n.id) ? 1 : 0;
  if (n.id >= MSOM_PTR && n.id <= MSOM_PTR_PRED && m->p.nptr <= 0) return 0;
  if (n.id == MSOM_ZETA || n.id == MSOM_DQ || n.id == MSOM_QPRED) return 0;   // scratch of a step in the msqg dialect
  return m->flayers[n.id];
}

using sx::Field;
using sx::Loaded;
using sx::Pipe;
using sx::Scal;

sx::RecView view_of(const msom *m, int ring) { return {m->g, ring, m->ix * m->nx, m->iy * m->ny, m->gnx, m->gny}; }

// this rank's digest word, summed over the ranks (tiles: one all-gather of the words; integer sums, so the order is free)
int digest_total(msom *m, Pipe &pp, uint64_t *out) {
  const int n = m->nranks;
  if (n == 1) return sx::digest_word0(m->st, pp, out);
  comm_begin(m);
  const int r = comm_allgather(m->comm, (const double *)pp.dig, (double *)(pp.dig + 1), 1);
  comm_end(m);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(pp.h_dig, pp.dig, (size_t)(n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->st));
  HIPCHK(hipStreamSynchronize(m->st));
  *out = 0;
  for (int k = 1; k <= n; k++) *out += pp.h_dig[k];
  return MSOM_OK;
}

// ---- save

// tiles (collective): every rank packs its tile with the global indices in the digest, the tiles are gathered as gather_global does
// and rank 0 writes the global array
int save_record_tiled(msom *m, Pipe &pp, const Field &it, FILE *fp, bool *io_ok) {
  const size_t cnt = (size_t)it.layers * m->nx * m->ny;
  double *send = nullptr, *recv = nullptr;
  HIPCHK(hipMalloc(&send, cnt * sizeof(double)));
  if (hipMalloc(&recv, cnt * m->nranks * sizeof(double)) != hipSuccess) { (void)hipFree(send); msom_set_error("msom_state_save: out of device memory"); return MSOM_ERR_HIP; }
  for (int l = 0; l < it.layers; l++)
    launch_state_pack(m->st, it.dev, send + (size_t)l * m->nx * m->ny, sx::chunk_of(it.v, l, it.v.oy, m->ny, it.v.ox, m->nx), pp.dig);
  comm_begin(m);
  int r = comm_allgather(m->comm, send, recv, cnt);
  comm_end(m);
  std::vector<double> h, g;
  if (!r && m->rank == 0) {
    h.resize(cnt * m->nranks);
    hipError_t e = hipMemcpyAsync(h.data(), recv, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->st);
    if (e == hipSuccess) e = hipStreamSynchronize(m->st);
    if (e != hipSuccess) { msom_set_error("HIP error %s in msom_state_save", hipGetErrorString(e)); r = MSOM_ERR_HIP; }
  } else if (!r && hipStreamSynchronize(m->st) != hipSuccess) r = MSOM_ERR_HIP;
  (void)hipFree(send);
  (void)hipFree(recv);
  if (r || m->rank != 0) return r;
  g.resize((size_t)it.layers * m->gnx * m->gny);
  for (int q = 0; q < m->nranks; q++) {
    const int tx = q % m->px, ty = q / m->px;
    for (int l = 0; l < it.layers; l++)
      for (int j = 0; j < m->ny; j++)
        memcpy(&g[((size_t)l * m->gny + ty * m->ny + j) * m->gnx + (size_t)tx * m->nx], &h[q * cnt + ((size_t)l * m->ny + j) * m->nx], m->nx * sizeof(double));
  }
  if (*io_ok && fwrite(g.data(), sizeof(double), g.size(), fp) != g.size()) *io_ok = false;
  return MSOM_OK;
}

void collect(msom *m, unsigned flags, const double *run3, std::vector<Field> &items, std::vector<Scal> &scal) {
  auto fld = [&](const char *name, int id, int ring = 0) {
    if (m->f[id]) items.push_back({name, m->f[id], m->model ? 1 : m->flayers[id], view_of(m, ring)});
  };
  scal.push_back({"time", {m->t, m->dt, m->previous, m->tnext, (double)m->iter}});
  // without mgstats.sum: a sum over the grid whose order, and so whose last bit, depends on the path that made it (the cached and the
  // plain path write the same file byte for byte); a loaded handle reports sum = 0 until its next solve
  scal.push_back({"mgstats", {(double)m->mg.i, m->mg.resb, m->mg.resa, (double)m->mg.nrelax}});
  if (m->model) {
    static const struct { const char *name; int id; } six[] = {{"psi", MSOM_PSI}, {"q", MSOM_Q}, {"zeta", MSOM_ZETA}, {"dq", MSOM_DQ}, {"qpred", MSOM_QPRED}};
    for (const auto &k : six) fld(k.name, k.id);
    if ((flags & MSOM_STATE_CONSTANTS) && m->have_qforc) fld("qforc", MSOM_QFORC);
    return;
  }
  fld("psi", MSOM_PSI, m->psi_ghosts_stale ? 1 : 0);
  fld("q", MSOM_Q);
  if (m->p.nptr > 0) fld("ptr", MSOM_PTR);
  fld("qof", MSOM_QOF);
  const char *de[6] = {"de_bf", "de_vd", "de_j1", "de_j2", "de_j3", "de_ft"};
  for (int k = 0; k < 6; k++) fld(de[k], MSOM_DE_BF + k);
  fld("po_mft", MSOM_PO_MFT);
  if (m->stochastic) {
    fld("noise", MSOM_NOISE);
    scal.push_back({"noise_ctr", {(double)m->seed, (double)m->noise_draw, (double)m->corrector_step}});
  }
  if (m->bfn_begun) { fld("bfn_f1", MSOM_BFN_F1); fld("bfn_f2", MSOM_BFN_F2); fld("bfn_f3", MSOM_BFN_F3); }
  scal.push_back({"bfn", {(double)m->bfn_begun, m->p.iRe, m->p.iRe4, m->p.Eks, m->p.Ekb}});
  static const char *acc[MSOM_ST_NACC] = {"st_acc0", "st_acc1", "st_acc2", "st_acc3", "st_acc4", "st_acc5", "st_acc6"};
  for (int k = 0; k < MSOM_ST_NACC; k++)
    if (m->stats.s[k]) items.push_back({acc[k], m->stats.s[k], m->nl, view_of(m, 0)});
  if (m->stats_qme) items.push_back({"st_qme", m->stats_qme, m->nl, view_of(m, 0)});
  if (m->stats_mask || m->stats_qme)   // W is read from the device by the caller, which fills slot 4
    scal.push_back({"stats", {(double)m->stats_mask, (double)m->stats_count, (double)m->stats_every, (double)m->stats_on, 0., (double)m->stats_ndev}});
  if (m->mode_pv_invert && m->helm_pm) {   // the modal solver's warm start, with the ghost values the last correction left
    items.push_back({"helm_pm", m->helm_pm, m->nl, view_of(m, 1)});
    std::vector<double> v;
    for (int k = 0; k < m->nl; k++) {
      const msom_mgstats &s = m->helm.s[k];
      for (double x : {(double)s.i, s.resb, s.resa, (double)s.nrelax}) v.push_back(x);
    }
    scal.push_back({"helm_mg", v});
  }
  scal.push_back({"misc", {(double)m->nme_ft, (double)m->helm_solved}});
  if (run3) scal.push_back({"run", {run3[0], run3[1], run3[2]}});
  if (flags & MSOM_STATE_CONSTANTS) {
    if (m->have_pg) fld("psipg", MSOM_PSIPG);
    if (!m->fr_uniform) fld("fr", MSOM_FR);
    fld("rd", MSOM_RD);
    if (m->have_qforc) fld("qforc", MSOM_QFORC);
    if (m->flag_topo) fld("topo", MSOM_TOPO);
    if (m->stochastic) fld("sigma", MSOM_SIGMA);
    if (m->p.nptr > 0) fld("ptr_relax", MSOM_PTR_RELAX);
    if (m->bfn_obs_set) fld("bfn_obs", MSOM_BFN_OBS);
    if (m->bfn_gain_set) fld("bfn_gain", MSOM_BFN_GAIN);
    scal.push_back({"dh", std::vector<double>(m->dhf, m->dhf + m->nl)});
  }
}

}  // namespace

int state_save_run(msom *m, const char *path, unsigned flags, const double *run3) {
  if (!m || !path) { msom_set_error("msom_state_save: null argument"); return MSOM_ERR_ARG; }
  if (m->stochastic && m->noise_mode == 0) {
    msom_set_error("msom_state_save: a stochastic run with noise_mode = 0 draws from libc's process-wide rand(), whose state cannot be "
                   "saved: run with noise_mode = 1");
    return MSOM_ERR_CONFIG;
  }
  if (m->nranks > 1 && m->psi_ghosts_stale) {
    msom_set_error("msom_state_save: psi carries stale ghost values (pystep_de); on tiles they cannot be stored: invert first");
    return MSOM_ERR_CONFIG;
  }
  int r = sync_stream(m);   // the lazy stream: nothing is read ahead of the step's last pass
  if (r) return r;
  std::vector<Field> items;
  std::vector<Scal> scal;
  collect(m, flags, run3, items, scal);
  for (Scal &s : scal)
    if (!strcmp(s.name, "stats") && m->stats_W) HIPCHK(hipMemcpy(&s.v[4], m->stats_W, sizeof(double), hipMemcpyDeviceToHost));
  msom_sfile sf;
  memset(&sf, 0, sizeof sf);
  sf.version = MSOM_STATE_VERSION; sf.dialect = (uint32_t)m->model; sf.nx = (uint32_t)m->gnx; sf.ny = (uint32_t)m->gny; sf.nl = (uint32_t)m->nl;
  sf.nptr = (uint32_t)(m->p.nptr > 0 ? m->p.nptr : 0); sf.stochastic = (uint32_t)(m->stochastic != 0); sf.noise_mode = (uint32_t)m->noise_mode;
  sf.mode_pv_invert = (uint32_t)m->mode_pv_invert; sf.flag_topo = (uint32_t)(m->flag_topo != 0);
  sf.params_len = (uint32_t)m->params_text.size();
  sf.params = const_cast<char *>(m->params_text.c_str());
  const bool tiled = m->nranks > 1;   // the gather stages nothing: the pipe is there for its digest words
  return sx::write_file("msom_state_save", path, m->rank == 0, m->st, tiled ? 8 : sx::pipe_capacity(m->gnx + 2, m->ny + 2), m->nranks, sf, scal, items,
                        [&](Pipe &pp, const Field &f, FILE *fp, bool *io_ok) {
                          return tiled ? save_record_tiled(m, pp, f, fp, io_ok) : sx::save_record(m->st, pp, f, fp, io_ok);
                        },
                        [&](Pipe &pp, uint64_t *d) { return digest_total(m, pp, d); });
}

extern "C" int msom_state_save(msom_t *m, const char *path, unsigned flags) { return state_save_run(m, path, flags, nullptr); }

extern "C" int msom_state_dbg_flip(msom_t *m, long element) {
  if (!m) return MSOM_ERR_ARG;
  m->state_flip = element;
  return MSOM_OK;
}

// ---- load

namespace {

const RecName &nm(const Loaded &l) { return NAMES[l.name]; }

double *target_ptr(msom *m, const RecName &n) {
  switch (n.target) {
    case T_FIELD: return m->f[n.id];
    case T_ACC: return m->stats.s[n.id];
    case T_QME: return m->stats_qme;
    default: return m->helm_pm;
  }
}

// a verified array into the handle: the whole allocation (its pads are the target's own: the spare array began as a copy of it)
int commit_field(msom *m, const Loaded &l) {
  HIPCHK(hipMemcpyAsync(target_ptr(m, nm(l)), l.nat, l.bytes(), hipMemcpyDeviceToDevice, m->st));
  if (l.rec->ring || nm(l).target != T_FIELD) return MSOM_OK;   // ghosts from the file, or never read
  int r = fill_bc(m, nm(l).id);
  if (!r && m->model) r = nq_after_upload(m, nm(l).id);
  return r;
}

}  // namespace

extern "C" int msom_state_load(msom_t *m, const char *path) {
  if (!m || !path) { msom_set_error("msom_state_load: null argument"); return MSOM_ERR_ARG; }
  msom_sfile sf;
  int r = msom_sfile_open(path, &sf, 0);   // the whole structure: header, every record header against the file size, trailer
  if (r) return r;
  struct Free { msom_sfile *s; ~Free() { msom_sfile_free(s); } } free_sf{&sf};
  // ---- everything that can be refused is refused before the handle changes
  if ((int)sf.dialect != m->model || (int)sf.nx != m->gnx || (int)sf.ny != m->gny || (int)sf.nl != m->nl ||
      (int)sf.nptr != (m->p.nptr > 0 ? m->p.nptr : 0)) {
    msom_set_error("msom_state_load: %s holds dialect %u, grid %u x %u, nl %u, nptr %u; the handle is dialect %d, %d x %d, nl %d, nptr %d", path,
                   sf.dialect, sf.nx, sf.ny, sf.nl, sf.nptr, m->model, m->gnx, m->gny, m->nl, m->p.nptr > 0 ? m->p.nptr : 0);
    return MSOM_ERR_CONFIG;
  }
  if ((int)sf.stochastic != (m->stochastic != 0) || (sf.stochastic && (int)sf.noise_mode != m->noise_mode) ||
      (int)sf.mode_pv_invert != m->mode_pv_invert || (int)sf.flag_topo != (m->flag_topo != 0)) {
    msom_set_error("msom_state_load: %s was saved with stochastic %u, noise_mode %u, mode_pv_invert %u, flag_topo %u; the handle has %d, %d, %d, %d",
                   path, sf.stochastic, sf.noise_mode, sf.mode_pv_invert, sf.flag_topo, m->stochastic != 0, m->noise_mode, m->mode_pv_invert,
                   m->flag_topo != 0);
    return MSOM_ERR_CONFIG;
  }
  const bool take_const = !m->const_set;
  std::map<std::string, std::vector<double>> sc;
  sx::Temps tmp;
  const std::vector<sx::KnownScalar> known = {{"time", 5}, {"mgstats", 4}, {"noise_ctr", 3}, {"bfn", 5}, {"stats", 6}, {"helm_mg", 4 * sf.nl},
                                              {"misc", 2}, {"run", 3}, {"dh", sf.nl}};
  for (uint32_t k = 0; k < sf.nrec; k++) {
    const msom_srec *rec = &sf.rec[k];
    if (rec->kind == MSOM_SK_SCALARS) {
      if ((r = sx::read_known_scalars("msom_state_load", path, rec, known, sc))) return r;
      continue;
    }
    const RecName *n = find_name(rec->name);
    const int nlay = n ? target_layers(m, *n) : 0;
    if (!n || !nlay || (int)rec->layers != nlay || (int)rec->ny != m->gny || (int)rec->nx != m->gnx) {
      msom_set_error("msom_state_load: %s: record %s [%u][%u][%u] has no place in this handle", path, rec->name, rec->layers, rec->ny, rec->nx);
      return MSOM_ERR_CONFIG;
    }
    if (rec->ring && m->nranks > 1) { msom_set_error("msom_state_load: %s: record %s carries a ghost ring: one tile only", path, rec->name); return MSOM_ERR_CONFIG; }
    if (n->target == T_HELM && !m->mode_pv_invert) { msom_set_error("msom_state_load: %s: record helm_pm needs mode_pv_invert", path); return MSOM_ERR_CONFIG; }
    Loaded l;
    l.name = (int)(n - NAMES); l.rec = rec; l.v = view_of(m, (int)rec->ring);
    l.ylo = rec->ring ? 0 : l.v.oy;   // a ring record is one tile's: all its rows
    l.yhi = rec->ring ? l.v.H() : l.ylo + m->ny;
    tmp.v.push_back(l);
  }
  if (sc.count("stats") && sc["stats"][0] != 0 && (!(sc["stats"][0] > 0) || sc["stats"][0] >= (double)(1u << MSOM_ST_NACC))) {
    msom_set_error("msom_state_load: %s: statistics mask %g", path, sc["stats"][0]);
    return MSOM_ERR_CONFIG;
  }
  if ((r = sync_stream(m))) return r;
  // ---- every field into a spare natural array, its digest recomputed there on the device
  if ((r = sx::stage_records("msom_state_load", path, m->st, sx::pipe_capacity(m->gnx + 2, m->ny + 2), m->nranks, tmp, &m->state_flip,
                             [&](const Loaded &l) { return target_ptr(m, nm(l)); }, [&](Pipe &pp, uint64_t *d) { return digest_total(m, pp, d); })))
    return r;
  // ---- commit.  Constants first (a handle that has none yet), msom_set_const, then the evolving state: set_const overwrites q
  m->res_ready = -1;
  if (take_const) {
    for (const Loaded &l : tmp.v) {
      if (nm(l).role != CONSTANT) continue;
      // through msom_set_field, which keeps the flags that go with a constant input: the array goes back to [layer][y][x] on the device
      double *flat = nullptr;
      const size_t per = (size_t)m->nx * m->ny;
      HIPCHK(hipMalloc(&flat, per * l.rec->layers * sizeof(double)));
      launch_unpack(m->st, l.nat, flat, m->g, (int)l.rec->layers);
      r = msom_set_field(m, nm(l).id, flat);
      (void)hipFree(flat);
      if (r) return r;
    }
    if (sc.count("dh")) for (int k = 0; k < m->nl; k++) m->dhf[k] = sc["dh"][k];
    if ((r = msom_set_const(m))) return r;
  }
  if (!m->model) {
    // the statistics: the arrays the file holds, allocated as msom_stats_begin / msom_time_filter allocate them
    unsigned mask = sc.count("stats") ? (unsigned)sc["stats"][0] : 0;
    bool qme = false;
    for (const Loaded &l : tmp.v) qme |= nm(l).target == T_QME;
    if (mask && mask != m->stats_mask && (r = msom_stats_begin(m, mask))) return r;
    for (const Loaded &l : tmp.v)
      if (nm(l).target == T_ACC && !m->stats.s[nm(l).id]) { msom_set_error("msom_state_load: %s: accumulator %d is not in the file's mask", path, nm(l).id); return MSOM_ERR_CONFIG; }
    if (qme && !m->stats_qme) HIPCHK(hipMalloc(&m->stats_qme, m->g.ls * m->nl * sizeof(double)));
    if (sc.count("stats")) {
      const std::vector<double> &s = sc["stats"];
      m->stats_count = (long)s[1]; m->stats_every = (int)s[2] < 1 ? 1 : (int)s[2]; m->stats_on = s[3] != 0; m->stats_ndev = (long)s[5];
      if (m->stats_W) HIPCHK(hipMemcpyAsync(m->stats_W, &s[4], sizeof(double), hipMemcpyHostToDevice, m->st));
      if ((r = sync_stream(m))) return r;   // s lives until the end of the call, the copy is done here all the same
    }
    for (const Loaded &l : tmp.v) {
      if (nm(l).target == T_FIELD && !m->f[nm(l).id] && (r = ensure_field(m, nm(l).id))) return r;   // qof, the budgets, the AB3 history
      if (nm(l).target == T_HELM && !m->helm_pm && (r = helm_ensure(m))) return r;
    }
  }
  int ring_psi = 0;
  for (const Loaded &l : tmp.v) {
    if (nm(l).role == CONSTANT) continue;
    if ((r = commit_field(m, l))) return r;
    if (nm(l).target == T_FIELD && nm(l).id == MSOM_PSI) ring_psi = (int)l.rec->ring;
  }
  if (sc.count("time")) {
    const std::vector<double> &v = sc["time"];
    m->t = v[0]; m->dt = v[1]; m->previous = v[2]; m->tnext = v[3]; m->iter = (int)v[4];
  }
  if (sc.count("mgstats")) {
    const std::vector<double> &v = sc["mgstats"];
    m->mg.i = (int)v[0]; m->mg.resb = v[1]; m->mg.resa = v[2]; m->mg.sum = 0.; m->mg.nrelax = (int)v[3];
  }
  if (sc.count("noise_ctr")) {
    const std::vector<double> &v = sc["noise_ctr"];
    m->seed = (unsigned)v[0]; m->noise_draw = (unsigned)v[1]; m->corrector_step = (int)v[2];
  }
  if (sc.count("bfn") && !m->model) {
    const std::vector<double> &v = sc["bfn"];
    m->bfn_begun = v[0] != 0; m->p.iRe = v[1]; m->p.iRe4 = v[2]; m->p.Eks = v[3]; m->p.Ekb = v[4];
  }
  if (sc.count("misc") && !m->model) { m->nme_ft = (int)sc["misc"][0]; m->helm_solved = sc["misc"][1] != 0; }
  if (sc.count("helm_mg") && !m->model)
    for (int k = 0; k < m->nl; k++) {
      const double *v = &sc["helm_mg"][4 * k];
      m->helm.s[k].i = (int)v[0]; m->helm.s[k].resb = v[1]; m->helm.s[k].resa = v[2]; m->helm.s[k].sum = 0.; m->helm.s[k].nrelax = (int)v[3];
    }
  m->run_loaded = sc.count("run") ? 1 : 0;
  if (m->run_loaded) { m->run_tout = sc["run"][0]; m->run_tflt = sc["run"][1]; m->run_outdir = (int)sc["run"][2]; }
  // ---- every row of DESIGN "State a handle keeps across calls" goes; the plain path rebuilds what the next call needs
  m->res_ready = -1;
  m->umax_ready = 0;
  m->umax_clean = 0;
  m->psi_ghosts_stale = ring_psi;
  if (!m->model) {
    if ((r = msom_set_option(m, "graph", (double)m->use_graph))) return r;   // drops the captured cycles
    m->wv_ready = 0;
    spec_drop(m);
    if (!take_const) {   // msom_set_const above has just rebuilt them otherwise
      modes_drop(m);
      if (m->mode_pv_invert && (r = msom_modes_compute(m))) return r;
    }
  }
  return sync_stream(m);
}

extern "C" msom_t *msom_create_from_state(const char *path) {
  if (!path) { msom_set_error("msom_create_from_state: null path"); return nullptr; }
  msom_sfile sf;
  if (msom_sfile_open(path, &sf, 0)) return nullptr;
  if (sf.dialect > 1) {   // a newer dialect must not become a newqg handle
    msom_set_error("msom_create_from_state: %s holds dialect %u%s", path, sf.dialect, sf.dialect == 2 ? ", the vertex model: use msomn_create_from_state" : "");
    msom_sfile_free(&sf);
    return nullptr;
  }
  msom_t *m = sf.dialect ? msom_create_newqg_str(sf.params) : msom_create_str(sf.params);
  int r = m ? MSOM_OK : MSOM_ERR_CONFIG;
  if (m && !sf.dialect) {
    if (sf.stochastic) {
      const msom_srec *nc = msom_sfile_find(&sf, "noise_ctr");
      std::vector<double> v;
      if (!r) r = msom_set_option(m, "stochastic", 1);
      if (!r) r = msom_set_option(m, "noise_mode", sf.noise_mode);
      if (!r && nc && !(r = sx::read_scalars(path, nc, v))) r = msom_set_option(m, "seed", v[0]);
    }
    if (!r && sf.mode_pv_invert) r = msom_set_option(m, "mode_pv_invert", 1);
    if (!r && sf.flag_topo) r = msom_set_option(m, "flag_topo", 1);
  }
  msom_sfile_free(&sf);
  if (m && !r) r = msom_state_load(m, path);
  if (m && r) {
    sx::destroy_keeping_error([&] { msom_destroy(m); });
    return nullptr;
  }
  return m;
}
