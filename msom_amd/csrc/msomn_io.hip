// msomn_io.hip -- NetCDF-3 IO of the vertex-grid model and its driver msomn_run (main() + events of qg-node/qg.c:58-181), with the
// options ckpt_steps / resume of include/msomn_state.h.  Nothing here runs inside msomn_step.
#include <unistd.h>

#include "msomn_host.h"
#include "../../include/msomn_state.h"

#define NEED_FIELD(m, f) if (!(m) || (f) < 0 || (f) >= MSOMN_NFIELDS) { msom_set_error("bad field id %d", (int)(f)); return MSOM_ERR_ARG; }

// ---- NetCDF-3 IO of vertex fields (qg-node/netcdf_vertex_bas.h:95-424)
// On tiles (option io_tiles) both calls are collective: the owned windows are gathered and rank 0 creates and appends; every rank reads
// the shared file and takes its window.  What one rank alone can see of the file ends in nt_agree
static int nc_put(msomn *m, const char *path, const double *psi, const double *q) {
  const size_t n1 = m->N + 1;
  const char *names[2] = {"psi", "q"};
  struct stat sb;
  if (stat(path, &sb) != 0 && msom_nc_create2(path, m->nl, (int)n1, (int)n1, m->p.L0, 2, names, 1)) return MSOM_ERR_IO;
  const double *fields[2] = {psi, q};
  return msom_nc_append(path, m->nl, (int)n1, (int)n1, 2, names, m->t, fields) < 0 ? MSOM_ERR_IO : MSOM_OK;
}
extern "C" int msomn_write_nc(msomn_t *m, const char *path) {
  if (int rt = nt_io_refuse(m, "msomn_write_nc")) return rt;
  if (!m || !path) return MSOM_ERR_ARG;
  const size_t n1 = m->N + 1, sz = n1 * n1 * m->nl;
  int r;
  if (m->ntiles > 1) {
    std::vector<double> psi, q;
    unsigned long long *word = nullptr;   // the pack pass sums a digest: nobody reads this one
    HIPCHK(hipMalloc(&word, sizeof *word));
    HIPCHK(hipMemsetAsync(word, 0, sizeof *word, m->st));
    if (!(r = nt_gather_owned(m, m->f[MSOMN_PSI], m->g, m->nl, 0, word, psi))) r = nt_gather_owned(m, m->f[MSOMN_Q], m->g, m->nl, 0, word, q);
    (void)hipFree(word);
    if (r) return r;
    return nt_agree(m, m->rank == 0 ? nc_put(m, path, psi.data(), q.data()) : (int)MSOM_OK, "msomn_write_nc");
  }
  std::vector<double> psi(sz), q(sz);
  if ((r = download_g(m, m->f[MSOMN_PSI], m->g, m->nl, psi.data())) || (r = download_g(m, m->f[MSOMN_Q], m->g, m->nl, q.data()))) return r;
  return nc_put(m, path, psi.data(), q.data());
}
extern "C" int msomn_read_nc(msomn_t *m, int field, const char *path, const char *varname, int record) {
  if (int rt = nt_io_refuse(m, "msomn_read_nc")) return rt;
  NEED_FIELD(m, field);
  if (!path || !varname) return MSOM_ERR_ARG;
  const size_t n1 = m->N + 1, w = m->g.nx, hgt = m->g.ny;
  const int nl = m->fl[field];
  std::vector<double> h(n1 * n1 * nl);
  if (int r = nt_agree(m, msom_nc_read(path, varname, record, nl, (int)n1, (int)n1, h.data(), nullptr) ? MSOM_ERR_IO : MSOM_OK, "msomn_read_nc")) return r;
  if (field == MSOMN_PSIPG) m->pg_set = 1;
  if (field == MSOMN_TOPO) m->topo_set = 1;
  if (m->ntiles > 1) {   // the tile's window, shared vertices included; then the halo, as msomn_set_field
    std::vector<double> t(w * hgt * nl);
    for (int l = 0; l < nl; l++)
      for (size_t j = 0; j < hgt; j++) memcpy(&t[(l * hgt + j) * w], &h[(l * n1 + m->oy + j) * n1 + m->ox], w * sizeof(double));
    h.swap(t);
  }
  int r = upload_g(m, m->f[field], m->g, nl, h.data());
  return r ? r : nt_exchange(m, m->f[field], m->g, 0, nl);
}

// main() + events of qg-node/qg.c:58-181
extern "C" int msomn_run(msomn_t *m, const char *workdir, long nsteps_max) {
  if (int rt = nt_io_refuse(m, "msomn_run")) return rt;
  if (!m) return MSOM_ERR_ARG;
  // tiles (option io_tiles): collective.  Rank 0 alone touches the output directory, prints and writes; the others take part in the
  // collectives (the gathers, the reductions of the diagnostics, the checkpoints)
  const bool tiled = m->ntiles > 1, root = m->rank == 0;
  const NodeParams &p = m->p;
  const char *wd = workdir ? workdir : ".";
  char dpath[600] = "", name[800], ckpt[700];
  int r;
  const size_t n1 = m->N + 1;
  // option "resume": <workdir>/state.msom, if it is there, is loaded before anything else -- a handle without constants takes them from
  // the file -- and the loop below is entered where the checkpoint was taken: after the events of that iteration, before its step
  snprintf(ckpt, sizeof ckpt, "%s/state.msom", wd);
  struct stat sc;
  bool resumed = false;
  if (m->resume && stat(ckpt, &sc) == 0) {
    if ((r = msomn_state_load(m, ckpt))) return r;
    if (!m->run_loaded) { msom_set_error("msomn_run: %s was not written by msomn_run (no record `run`)", ckpt); return MSOM_ERR_CONFIG; }
    resumed = true;
  }
  if (tiled && !m->const_set) {
    // the init branch below draws psi from the process-wide rand() and belongs to a driver that has set nothing yet; the in-process
    // tiles are threads of one process and cannot share that stream (as noise_mode = 0)
    msom_set_error("msomn_run: a tiled vertex-grid handle (%d x %d tiles) has no cold start: set the fields and call msomn_set_const first, or "
                   "resume from a state.msom in the working directory", m->px, m->py);
    return MSOM_ERR_STATE;
  }
  if (tiled && m->p.dtflt > 0 && !m->wavelet_tiles) {
    msom_set_error("msomn_run: dtflt > 0 runs msomn_wavelet_filter, which on a tiled vertex-grid handle (%d x %d tiles) needs the option wavelet_tiles = 1", m->px, m->py);
    return MSOM_ERR_CONFIG;
  }
  int outdir = 0;
  for (int i = 1; root && !resumed && i < 10000; i++) {  // create_outdir, extra.h:122-135
    snprintf(dpath, sizeof dpath, "%s/outdir_%04d/", wd, i);
    if (mkdir(dpath, 0777) == 0) { fprintf(stdout, "Writing output in %s\n", dpath); outdir = i; break; }
  }
  if (root && !resumed) {
    snprintf(name, sizeof name, "%sparams.in", dpath);  // backup_config
    if (FILE *fp = fopen(name, "w")) { fwrite(m->params_text.data(), 1, m->params_text.size(), fp); fclose(fp); }
  }
  if (!m->const_set) {
    // init (qg_baroclinic_ms.h:478-492): optional input file, variables N2, psi_pg, mask, topo, q_forcing
    if (m->nl > 1) {
      snprintf(name, sizeof name, "%s/input_vars_%dl_N%d.nc", wd, m->nl, m->N);
      struct stat sb;
      if (stat(name, &sb) == 0) {
        fprintf(stdout, "Read input files:\n");
        const struct { int f; const char *v; } in[] = {{MSOMN_S2, "N2"}, {MSOMN_PSIPG, "psi_pg"}, {MSOMN_MASK, "mask"}, {MSOMN_TOPO, "topo"}, {MSOMN_QFORC, "q_forcing"}};
        for (auto &e : in) (void)msomn_read_nc(m, e.f, name, e.v, 0);  // absent variables keep their defaults
        {  // q_forcing_3d: only when the file has it (msomn_read_nc would switch FORCING_3D on)
          std::vector<double> h3((size_t)(m->N + 1) * (m->N + 1) * m->nl);
          if (!msom_nc_read(name, "q_forcing_3d", 0, m->nl, m->N + 1, m->N + 1, h3.data(), nullptr)) (void)msomn_set_field(m, MSOMN_QFORC3D, h3.data());
        }
        fprintf(stdout, "%s .. ok\n", name);
      }
    }
    // set_const qg-node/qg.h:475-479: psi = noise_init (noise() + sin(2 pi y / L0)); noise() in [-1, 1]
    std::vector<double> h(n1 * n1 * m->nl);
    for (size_t j = 0; j < n1; j++) for (size_t i = 0; i < n1; i++) for (int l = 0; l < m->nl; l++)
      h[(l * n1 + j) * n1 + i] = p.noise_init * ((1. - 2. * rand() / (double)RAND_MAX) + sin(2 * M_PI * (j * m->D) / p.L0));
    if ((r = upload_g(m, m->f[MSOMN_PSI], m->g, m->nl, h.data()))) return r;
    snprintf(name, sizeof name, "%s/restart.nc", wd);
    struct stat sb;
    if (stat(name, &sb) == 0) {
      fprintf(stdout, "Read restart file:\n");
      if ((r = msomn_read_nc(m, MSOMN_PSI, name, "psi", -1))) return r;
      fprintf(stdout, "%s .. ok\n", name);
    }
    if ((r = msomn_set_const(m))) return r;
  }
  double tout = 0., tdiag = 0., tflt = p.dtflt;   // event filter (t = dtflt; t <= tend + 1e-10; t += dtflt), qg_baroclinic_ms.h:405-408
  const bool diag = p.dtdiag > 0, filt = p.dtflt > 0;
  long nrec = 0;   // records vars.nc holds
  if (resumed) {   // the recorded event schedule and output directory
    tout = m->run_ev[0]; tdiag = m->run_ev[1]; tflt = m->run_ev[2]; outdir = (int)m->run_ev[3]; nrec = (long)m->run_ev[4];
    snprintf(dpath, sizeof dpath, "%s/outdir_%04d/", wd, outdir);
    if (root) mkdir(dpath, 0777);
    if (root) fprintf(stdout, "Resuming from %s at i = %d, output in %s\n", ckpt, m->iter, dpath);
  }
  snprintf(name, sizeof name, "%svars.nc", dpath);
  char dname[800];
  snprintf(dname, sizeof dname, "%sdiag_1d.dat", dpath);
  if (resumed) {   // what a run that died wrote after the checkpoint goes: the continued run writes it again
    auto set_back = [&]() -> int {
      struct stat sb;
      if (nrec == 0) unlink(name);
      else if (stat(name, &sb) == 0 && msom_nc_truncate(name, nrec)) return MSOM_ERR_IO;
      if (stat(dname, &sb) == 0 && (off_t)m->run_ev[5] < sb.st_size && truncate(dname, (off_t)m->run_ev[5])) {
        msom_set_error("msomn_run: cannot truncate %s", dname);
        return MSOM_ERR_IO;
      }
      return MSOM_OK;
    };
    if ((r = nt_agree(m, root ? set_back() : (int)MSOM_OK, "msomn_run"))) return r;
  }
  long steps = 0;
  for (;;) {
    const bool skip = resumed;   // resumed: the events of this iteration ran before the checkpoint was written
    resumed = false;
    if (!skip && diag && tdiag <= p.tend + 1e-10 && m->t >= tdiag - 1e-12 * fmax(1., fabs(tdiag))) {  // write_1d_diag (qg.h:361-399)
      double d3[3] = {0., 0., 0.};
      if (m->iter != 0 && (r = msomn_diag1d(m, d3))) return r;   // tiles: a reduction over the ranks
      if (FILE *fp = root ? fopen(dname, "a") : nullptr) {
        if (m->iter == 0) fprintf(fp, "# time, ke, dissipation, forcing\n");
        else fprintf(fp, "%e, %e, %e, %e\n", m->t, d3[0], d3[1], d3[2]);
        fclose(fp);
      }
      tdiag += p.dtdiag;
    }
    if (!skip && (r = msomn_forcing(m))) return r;  // forcing (i++)
    if (!skip && filt && tflt <= p.tend + 1e-10 && m->t >= tflt - 1e-12 * fmax(1., fabs(tflt))) {
      if (root) fprintf(stdout, "Filter solution\n");
      if ((r = msomn_wavelet_filter(m, p.dtflt))) return r;
      tflt += p.dtflt;
    }
    bool pending = tout <= p.tend + 1e-10;
    if (!skip && pending && m->t >= tout - 1e-12 * fmax(1., fabs(tout))) {  // output (t = 0; t <= tend + 1e-10; t += dtout)
      if (root) fprintf(stdout, "write file\n");
      if (m->iter == 0 && (r = msomn_invert_q(m, MSOMN_Q, nullptr))) return r;
      if ((r = msomn_write_nc(m, name))) return r;
      if (root) fprintf(stdout, "file written \n");
      nrec++;
      tout += p.dtout;
      pending = tout <= p.tend + 1e-10;
    }
    if (!skip) {
      double ke;
      if ((r = msomn_ke(m, &ke))) return r;
      if (root) fprintf(stdout, "i = %i, dt = %g, t = %g, ke_1 = %g\n", m->iter, m->dt, m->t, ke);  // writestdout
    }
    if (!pending) break;
    // option "ckpt_steps": the checkpoint never moves tnext, so the run takes the dt sequence of a run without it
    if (!skip && m->ckpt_steps > 0 && steps > 0 && m->iter % m->ckpt_steps == 0) {
      struct stat sb;
      // (tiles: rank 0 writes the record, so the directory number and the size of diag_1d.dat are its own)
      const double run6[6] = {tout, tdiag, tflt, (double)outdir, (double)nrec, root && stat(dname, &sb) == 0 ? (double)sb.st_size : 0.};
      if ((r = nstate_save_run(m, ckpt, MSOM_STATE_CONSTANTS, run6))) return r;
    }
    if (nsteps_max >= 0 && steps >= nsteps_max) break;
    m->tnext = diag && tdiag <= p.tend + 1e-10 ? fmin(tout, tdiag) : tout;
    if (filt && tflt <= p.tend + 1e-10) m->tnext = fmin(m->tnext, tflt);
    if ((r = msomn_step(m, 0))) return r;
    steps++;
  }
  fflush(stdout);
  return m->iter;
}
