// msomn_state.hip -- lossless checkpoint and bit-exact restart of the vertex-grid model (include/msomn_state.h).
// Same container and the same device pass as msom_state.hip: k_state_rows of kernels_state.hip takes any natural geometry, so the
// vertex fields go through it with the handle's NatGeom (nx = ny = N + 1, no ring, one tile: global offsets 0) and the cell-scalar
// noise with the geometry of cs[0]; the transfers and the file writer are those of state_xfer.hip.  Nothing here runs inside msomn_step.
// On tiles (option io_tiles) the calls are collective: a record is the global array, a rank's digest word covers the window it OWNS
// (node_tile_inl.h) with the global indices, the words add up over the ranks, and what only one rank can see ends in nt_agree.
#include "msomn_host.h"
#include "state_xfer.h"
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

using sx::Field;
using sx::Loaded;
using sx::Pipe;
using sx::Scal;

const RecName &nm(const Loaded &l) { return NAMES[l.name]; }
// no ring; the record is the global array (one tile: the handle's), the tile's window of it starts at (ox, oy)
sx::RecView view_of(const msomn *m, const NatGeom &g, bool cells) { return {g, 0, m->ox, m->oy, cells ? m->N : m->N + 1, cells ? m->N : m->N + 1}; }
NatGeom noise_geom(const msomn *m) {
  if (m->ntiles == 1) return cell_geom(m->N);
  const NodeTile t = ntile_level(m->N, m->px, m->py, m->rank, 0);
  return cell_geom_rect(t.tx, t.ty);
}
NatGeom rec_geom(const msomn *m, const RecName &n) { return n.field == F_NOISE ? noise_geom(m) : m->g; }
int rec_layers(const msomn *m, const RecName &n) { return n.field == F_NOISE ? 1 : is_acc(n) ? m->nl : m->fl[n.field]; }
// a load stages whole record rows of the tile's rows; a tiled save stages nothing (the gather moves the tiles)
size_t pipe_cap(const msomn *m) { return sx::pipe_capacity((size_t)m->N + 1, m->g.ny); }
// this rank's digest word, summed over the ranks (tiles: one all-gather of the words; integer sums, so the order is free)
sx::DigestTotal total_of(msomn *m) {
  if (m->ntiles == 1) return [m](Pipe &pp, uint64_t *d) { return sx::digest_word0(m->st, pp, d); };
  return [m](Pipe &pp, uint64_t *d) {
    const int n = m->ntiles;
    if (int r = comm_allgather(m->comm, (const double *)pp.dig, (double *)(pp.dig + 1), 1)) return r;
    HIPCHK(hipMemcpyAsync(pp.h_dig, pp.dig, (size_t)(n + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->st));
    HIPCHK(hipStreamSynchronize(m->st));
    *d = 0;
    for (int k = 1; k <= n; k++) *d += pp.h_dig[k];
    return (int)MSOM_OK;
  };
}
// tiles (collective): every rank packs the window it owns, the digest over it, the windows are gathered and rank 0 writes the record
int save_record_tiled(msomn *m, Pipe &pp, const Field &f, FILE *fp, bool *io_ok) {
  std::vector<double> g;
  if (int r = nt_gather_owned(m, f.dev, f.v.g, f.layers, f.v.gnx == m->N, pp.dig, g)) return r;
  if (fp && *io_ok && fwrite(g.data(), sizeof(double), g.size(), fp) != g.size()) *io_ok = false;
  return MSOM_OK;
}

// ---- save

void collect(msomn *m, unsigned flags, const double *run6, std::vector<Field> &items, std::vector<Scal> &scal) {
  auto fld = [&](const char *name, int id) { items.push_back({name, m->f[id], m->fl[id], view_of(m, m->g, false)}); };
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
  if (m->stochastic && m->cnlev > 0) items.push_back({"noise", m->cs[0], 1, view_of(m, m->cg[0], true)});
  // between the two stages of a step (only a stochastic handle knows that it is: corrector_step) the second update reads the predictor;
  // at a step boundary QPRED is scratch and is not written
  if (m->stochastic && m->corrector_step) fld("qpred", MSOMN_QPRED);
  if (m->stats_mask) {   // a handle without statistics writes the records it always wrote
    scal.push_back({"stats", {(double)m->stats_mask, (double)m->stats_count, (double)m->stats_every, (double)m->stats_on, m->stats_W,
                              (double)m->stats_samples}});
    for (int k = 0; k < MSOM_ST_NACC; k++)
      if (m->stats.s[k]) items.push_back({acc_name(k), m->stats.s[k], m->nl, view_of(m, m->g, false)});
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
  if (int rt = nt_io_refuse(m, "msomn_state_save")) return rt;
  if (!m->const_set) { msom_set_error("msomn_state_save: call msomn_set_const first"); return MSOM_ERR_STATE; }
  if (m->stochastic && m->noise_mode == 0) {
    msom_set_error("msomn_state_save: a stochastic run with noise_mode = 0 draws from libc's process-wide rand(), whose state cannot be "
                   "saved: run with noise_mode = 1");
    return MSOM_ERR_CONFIG;
  }
  HIPCHK(hipStreamSynchronize(m->st));
  std::vector<Field> items;
  std::vector<Scal> scal;
  collect(m, flags, run6, items, scal);
  msom_sfile sf;
  memset(&sf, 0, sizeof sf);
  sf.version = MSOM_STATE_VERSION; sf.dialect = NSTATE_DIALECT; sf.nx = sf.ny = (uint32_t)(m->N + 1); sf.nl = (uint32_t)m->nl;
  sf.stochastic = (uint32_t)(m->stochastic != 0); sf.noise_mode = (uint32_t)m->noise_mode; sf.flag_topo = (uint32_t)(m->topo_set != 0);
  sf.params_len = (uint32_t)m->params_text.size();
  sf.params = const_cast<char *>(m->params_text.c_str());
  const bool tiled = m->ntiles > 1;
  const int r = sx::write_file("msomn_state_save", path, m->rank == 0, m->st, tiled ? 8 : pipe_cap(m), m->ntiles, sf, scal, items,
                               [m, tiled](Pipe &pp, const Field &f, FILE *fp, bool *io_ok) {
                                 return tiled ? save_record_tiled(m, pp, f, fp, io_ok) : sx::save_record(m->st, pp, f, fp, io_ok);
                               },
                               total_of(m));
  // rank 0 alone knows whether the file is in place: nobody returns before it is, and everybody with its verdict
  return nt_agree(m, r, "msomn_state_save");
}

extern "C" int msomn_state_save(msomn_t *m, const char *path, unsigned flags) { return nstate_save_run(m, path, flags, nullptr); }

extern "C" int msomn_state_dbg_flip(msomn_t *m, long element) {
  if (!m) return MSOM_ERR_ARG;
  m->state_flip = element;
  return MSOM_OK;
}

// ---- load

namespace {

double *target_ptr(msomn *m, const RecName &n) {
  if (is_acc(n)) return m->stats.s[F_ACC0 - n.field];
  return n.field == F_NOISE ? (m->cnlev > 0 ? m->cs[0] : nullptr) : m->f[n.field];
}

}  // namespace

extern "C" int msomn_state_load(msomn_t *m, const char *path) {
  if (int rt = nt_io_refuse(m, "msomn_state_load")) return rt;
  if (!m || !path) { msom_set_error("msomn_state_load: null argument"); return MSOM_ERR_ARG; }
  msom_sfile sf;
  memset(&sf, 0, sizeof sf);
  struct Free { msom_sfile *s; ~Free() { msom_sfile_free(s); } } free_sf{&sf};
  std::map<std::string, std::vector<double>> sc;
  sx::Temps tmp;
  unsigned file_mask = 0;
  bool take_const = false;
  int r;
  // ---- the host's part: the file and what it says against what the handle is.  Every rank reads the shared file; on tiles the verdicts
  // meet in nt_agree before anything is posted
  auto validate = [&]() -> int {
    int r = msom_sfile_open(path, &sf, 0);   // the whole structure: header, every record header against the file size, trailer
    if (r) return r;
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
    const std::vector<sx::KnownScalar> known = {{"time", 5}, {"mgstats", 4}, {"node", NS_COUNT}, {"run", 6}, {"stats", SS_N}};
    for (uint32_t k = 0; k < sf.nrec; k++) {
      const msom_srec *rec = &sf.rec[k];
      if (rec->kind == MSOM_SK_SCALARS) {
        if ((r = sx::read_known_scalars("msomn_state_load", path, rec, known, sc))) return r;
        continue;
      }
      const RecName *n = find_name(rec->name);
      Loaded l;
      l.rec = rec;
      if (n) {
        const bool cells = n->field == F_NOISE;
        l.name = (int)(n - NAMES); l.v = view_of(m, rec_geom(m, *n), cells);
        l.ylo = m->oy; l.yhi = m->oy + l.v.g.ny;   // the rows the tile holds, shared ones included
        if (m->ntiles > 1) {   // the digest word and the test flip: the window the tile owns
          const NodeOwned o = nt_owned(m, l.v.g, cells, m->rank);
          l.own_nx = o.g.nx; l.own_ny = o.g.ny;
        }
      }
      if (!n || tmp.find(rec->name) || rec->ring || (int)rec->layers != rec_layers(m, *n) || (int)rec->ny != l.v.gny || (int)rec->nx != l.v.gnx ||
          (n->field == F_NOISE && !m->stochastic)) {
        msom_set_error("msomn_state_load: %s: record %s [%u][%u][%u] has no place in this handle", path, rec->name, rec->layers, rec->ny, rec->nx);
        return MSOM_ERR_CONFIG;
      }
      tmp.v.push_back(l);
    }
    {  // the statistics: a mask msomn_stats_begin would take, and exactly the accumulators it selects
      unsigned recs = 0;
      for (const Loaded &l : tmp.v) if (is_acc(nm(l))) recs |= 1u << (F_ACC0 - nm(l).field);
      if (sc.count("stats")) {
        const double fm = sc["stats"][SS_MASK];
        if (!(fm >= 1) || fm >= (double)(1u << MSOM_ST_NACC) || fm != floor(fm)) { msom_set_error("msomn_state_load: %s: statistics mask %g", path, fm); return MSOM_ERR_CONFIG; }
        file_mask = (unsigned)fm;
      }
      if (recs != file_mask) { msom_set_error("msomn_state_load: %s: accumulator records 0x%x, the mask of record `stats` is 0x%x", path, recs, file_mask); return MSOM_ERR_CONFIG; }
    }
    if (!sc.count("node") || !sc.count("time")) { msom_set_error("msomn_state_load: %s has no record `%s`", path, sc.count("node") ? "time" : "node"); return MSOM_ERR_CONFIG; }
    const std::vector<double> &ns = sc["node"];
    const bool file_const = tmp.find("mask") != nullptr;
    take_const = !m->const_set && file_const;
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
    return MSOM_OK;
  };
  if ((r = nt_agree(m, validate(), "msomn_state_load"))) return r;
  const std::vector<double> &ns = sc["node"];
  HIPCHK(hipStreamSynchronize(m->st));
  // ---- every field into a spare natural array (pads: the target's own, or zero), its digest recomputed there on the device
  if ((r = sx::stage_records("msomn_state_load", path, m->st, pipe_cap(m), m->ntiles, tmp, &m->state_flip,
                             [m](const Loaded &l) { return target_ptr(m, nm(l)); }, total_of(m))))
    return r;
  // ---- commit.  Constants first: the stored ones as they are and what follows from them (node_const_derived), or msomn_set_const on
  // what the handle holds if the file brings none; then the evolving state (msomn_set_const overwrites q)
  // tiles: a model field gets the halo msomn_set_field would have given it (the spare array began with the handle's old one)
  auto put = [&](const Loaded &l, double *dst) -> int {
    HIPCHK(hipMemcpyAsync(dst, l.nat, l.bytes(), hipMemcpyDeviceToDevice, m->st));
    return nm(l).field >= 0 ? nt_exchange(m, dst, m->g, 0, (int)l.rec->layers) : (int)MSOM_OK;
  };
  if (take_const) {
    for (const Loaded &l : tmp.v)
      if (nm(l).role == CONSTANT && (r = put(l, m->f[nm(l).field]))) return r;
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
    if (nm(l).role == CONSTANT) continue;
    // psi through the live pointer.  The buffer that is not psi (psi_alt, if the handle has one yet) stays as it is: k_n_rhs_pre and
    // k_n_correct_residual write every vertex of it before anything reads it, and its pad cells are zero in both buffers
    if ((r = put(l, target_ptr(m, nm(l))))) return r;
    if (nm(l).field == F_NOISE) {
      if (m->ntiles == 1) node_noise_ghosts(m);
      else if ((r = ct_ring(m, m->cs[0], m->cg[0], 1, BC_NEUMANN))) return r;
    }
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

namespace {

// px * py = 0: the plain handle of msomn_create_from_state
msomn_t *create_from_state(const char *entry, const char *path, int px, int py, int rank, const void *id128) {
  if (!path) { msom_set_error("%s: null path", entry); return nullptr; }
  msom_sfile sf;
  if (msom_sfile_open(path, &sf, 0)) return nullptr;
  if (sf.dialect != NSTATE_DIALECT) {
    msom_set_error("%s: %s holds dialect %u, a cell-centred model: use msom_create_from_state", entry, path, sf.dialect);
    msom_sfile_free(&sf);
    return nullptr;
  }
  if (!msom_sfile_find(&sf, "mask")) {
    msom_set_error("%s: %s was saved without MSOM_STATE_CONSTANTS: create the handle, set its constants and call msomn_state_load", entry, path);
    msom_sfile_free(&sf);
    return nullptr;
  }
  msomn_t *m = px * py ? msomn_create_tiled(sf.params, px, py, rank, id128) : msomn_create_str(sf.params);
  int r = m ? MSOM_OK : MSOM_ERR_CONFIG;
  if (m && px * py) {
    r = msomn_set_option(m, "io_tiles", 1);
    if (!r && (sf.stochastic || msom_sfile_find(&sf, "psi_f"))) r = msomn_set_option(m, "wavelet_tiles", 1);
  }
  if (m && !r && sf.stochastic) {
    const msom_srec *nr = msom_sfile_find(&sf, "node");
    std::vector<double> v;
    r = msomn_set_option(m, "stochastic", 1);
    if (!r) r = msomn_set_option(m, "noise_mode", sf.noise_mode);
    if (!r && nr && nr->layers == NS_COUNT && !(r = sx::read_scalars(path, nr, v))) m->seed = (unsigned)v[NS_SEED];   // not the option: it calls srand
  }
  msom_sfile_free(&sf);
  if (m && !r) r = msomn_state_load(m, path);
  if (m && r) {
    sx::destroy_keeping_error([&] { msomn_destroy(m); });
    return nullptr;
  }
  return m;
}

}  // namespace

extern "C" msomn_t *msomn_create_from_state(const char *path) { return create_from_state("msomn_create_from_state", path, 0, 0, 0, nullptr); }

extern "C" msomn_t *msomn_create_tiled_from_state(const char *path, int px, int py, int rank, const void *id128) {
  if (px < 1 || py < 1) { msom_set_error("msomn_create_tiled_from_state: %d x %d tiles", px, py); return nullptr; }
  return create_from_state("msomn_create_tiled_from_state", path, px, py, rank, id128);
}
