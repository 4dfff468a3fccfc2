/*
 * msomn_state.h -- lossless checkpoint and bit-exact restart of the vertex-grid model msomn_t (exported by both libraries).
 * The reference restarts the vertex model from restart.nc: psi as float32, q recomputed, t, the dt limiter's memory, the noise draw
 * counter, the filter's running mean and the event schedule from zero.  These calls save the state of a handle in fp64 with everything
 * the next step reads, so that a run that is stopped, saved, destroyed, re-created, loaded and continued gives the bits of the run
 * that was never stopped.  Same container as msom_state.h (version 1), dialect 2; format and reasoning: DESIGN.md section 8i.
 * msom_state_check and msom_state_info of msom_state.h are the host-only entry points for this dialect too.
 *
 * Header of the file: nx = ny = N + 1 (vertices), nl, nptr = 0, mode_pv_invert = 0, stochastic, noise_mode, flag_topo = topo has been
 *   set, the params text the handle was created from.
 * What is saved, always: psi (the solver's first guess), q, q_forcing (msomn_step(m, 0) reads it without refreshing it), psi_f once
 *   the wavelet filter has run, the cell-scalar noise as [1][N][N] when stochastic, the predictor qpred when a stochastic handle is
 *   saved between the two stages of a step (corrector_step = 1: the second msomn_update reads it); scalars `time` (t, dt, the dt
 *   limiter's previous, tnext, iter), `mgstats` (i, resb, resa, nrelax; sum is not saved: 0 after a load) and `node` (seed, noise_draw,
 *   corrector_step, nbar, pg_set, topo_set, forcing_3d, sqg, the clamped DT).
 *   A handle with running statistics (msomn_stats_begin, stats_mask != 0) also saves its accumulators as st_psi, st_q, st_psi2, st_q2,
 *   st_ke, st_uq, st_vq (the selected ones) and the scalars `stats` (mask, steps counted, stats_every, option stats, W, samples); a
 *   load allocates the mask the file holds and restores them.  A handle without statistics writes none of these records.
 * flags & MSOM_STATE_CONSTANTS: the constants too, as msomn_set_const left them -- mask, S2 (f^2 / N^2), S2S and bs when sqg, topo
 *   (times scale_topo) when set, psi_pg when set, q_forcing_3d when on -- so that the file alone restarts a run.
 * msomn_state_save: waits for the stream, writes `path`.tmp and renames it to `path`.  Changes nothing the next step reads.  Before
 *   msomn_set_const: MSOM_ERR_STATE.  A stochastic handle with noise_mode = 0 draws from libc's process-wide rand(), whose state cannot
 *   be saved: MSOM_ERR_CONFIG (use noise_mode = 1).
 * msomn_state_load: into a handle of the same N, nl, stochastic, noise_mode and sqg (else MSOM_ERR_CONFIG).  A handle that has its
 *   constants keeps them, must agree with the file on topo_set, pg_set and forcing_3d, and takes the evolving records.  A handle without
 *   constants installs the stored ones as they are (msomn_set_const transforms its inputs in place, so it is not run on them), builds
 *   what follows from them, and takes the evolving records: q from the file, not recomputed; noise_draw from the file, not 0.  A file
 *   without constants into a handle without them: msomn_set_const on what the handle holds, then the evolving records.  The clamped DT of
 *   the file must be the handle's: MSOM_ERR_CONFIG otherwise.  The whole file is validated on the host, then every field record is
 *   uploaded into a spare array and its digest recomputed there on the device, before the handle changes: bad magic, unknown version,
 *   short file, digest mismatch: MSOM_ERR_IO, message in msom_last_error, handle as before the call.
 * msomn_create_from_state: msomn_create_str of the params text in the file, the options the file records (stochastic, noise_mode,
 *   seed) and msomn_state_load; the file must hold the constants.  NULL on error, and on a file of dialect 0 or 1
 *   (msom_create_from_state of msom_state.h makes those, and returns NULL on a file of this dialect).
 * msomn_state_dbg_flip: test aid.  The next msomn_state_load on this handle flips the lowest mantissa bit of element `element` of the
 *   first field record on the device, between the upload and the device digest (element < 0: off).  That load must fail.
 * On tiles (msomn_create_tiled, option io_tiles = 1; refused with MSOM_ERR_CONFIG without it): save and load are COLLECTIVE.  The file
 *   does not know its tiling: a px x py handle writes, byte for byte, the file the single tile writes at the same point of the same run
 *   (run with the option values the tiled handle reports), and a file of any tiling loads on any other.  A rank's digest word covers
 *   the vertices it owns (include/msom.h), with their global indices; the words add up over the ranks, so every rank reaches the same
 *   verdict.  Every rank returns the same code; a save has returned on no rank before the file is in place.  msomn_state_dbg_flip
 *   takes its element modulo the tile's owned window.  msomn_create_tiled_from_state (declared in msom.h beside msomn_create_tiled):
 *   msomn_create_tiled of the params text in the file, io_tiles = 1, wavelet_tiles = 1 when the file is stochastic or holds psi_f, the
 *   options the file records, the load.
 * Options of msomn_set_option that use these calls: "ckpt_steps" [0 = off]: msomn_run writes <workdir>/state.msom (with constants and
 *   its own event schedule) every that many steps; "resume" [0]: msomn_run continues from <workdir>/state.msom if it exists, in the
 *   output directory the file names, with vars.nc and diag_1d.dat set back to what they held at the checkpoint.
 */
#ifndef MSOMN_STATE_H
#define MSOMN_STATE_H

#include "msom_state.h"

#ifdef __cplusplus
extern "C" {
#endif

int msomn_state_save(msomn_t *m, const char *path, unsigned flags);
int msomn_state_load(msomn_t *m, const char *path);
msomn_t *msomn_create_from_state(const char *path);
int msomn_state_dbg_flip(msomn_t *m, long element);

#ifdef __cplusplus
}
#endif
#endif
