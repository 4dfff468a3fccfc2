/*
 * msomn_floats.h -- Lagrangian floats of the vertex-grid model (msomn_*, qg-node/), advected on the device with the model's own RK2
 * stages; on one tile, and with option floats_tiles on tiles; exported by both libraries.  The twin of msom_floats.h on the grid that
 * has a land mask, islands and coastlines.
 * DESIGN.md section 8l has the arithmetic, where the stages sit in msomn_step and the counted memory traffic.
 *
 * A float is a position (x, y) in the domain [0, L0] x [0, L0] and a layer in [0, nl).  The domain has N x N cells, vertex i sits at
 * i * Delta and psi lives on the vertices, so the velocity is that of the bilinear psi of the grid cell the float is in: no ghost
 * ring is read.  With idx = N / L0 (rounded once),
 *     xi = x * idx;  f = floor(xi) clamped to [0, N - 1];  i0 = (int) f;  a = xi - f clamped to [0, 1]      (j0, b likewise from y)
 *     u = -((1 - a) * (P01 - P00) + a * (P11 - P10)) * idx
 *     v =  ((1 - b) * (P10 - P00) + b * (P11 - P01)) * idx    Pcd = P[layer][j0 + d][i0 + c]
 *   P is MSOMN_PSI as the handle holds it, plus MSOMN_PSIPG per corner where a psi_pg has been set.  It is not multiplied by the mask:
 *   the model has masked psi already, and the floats read what the model holds.  A float at x = L0 reads column N with weight exactly
 *   1; no column beyond N is ever read, whatever the bits of x.  Inside a cell u = -dpsi/dy does not depend on y, v = dpsi/dx not on x,
 *   and du/dx = -dv/dy = -(P11 - P10 - P01 + P00) * idx^2: the velocity of the bilinear psi is non-divergent.  Three things follow:
 *   - a cell with four land corners has velocity exactly +-0 when no psi_pg is set: a float started there stays, bit for bit;
 *   - the velocity normal to an edge along which P is constant is exactly +-0 on that edge: a float on a domain wall, or on a coast
 *     edge between two land vertices, slides along it;
 *   - x * idx is a single rounding with nothing to fuse: the product and the strict build locate the same cell for the same position.
 * One msomn_step moves every float by its two stages, with the step's dt and the two stream functions the step inverts:
 *     stage 1: (xh, yh) = (x, y) + dt / 2 U(x, y; psi_n)        stage 2: (x, y) += dt U(xh, yh; psi_{n + 1/2})
 *   Stage 1 is queued behind the step's first msomn_update (psi_n inverted, masked, sides set; dt fixed), stage 2 behind its second
 *   msomn_update AND its final msomn_advance; no host wait is added, and a handle without floats makes the launches it always made.
 *   Both results are clamped to the box (counted in "floats_clamped", once per float and stage).  A result that is not finite makes
 *   the float lost: both coordinates become NaN and stay so, nothing is read for it, "floats_lost" counts it once.
 *
 * msomn_floats_begin: n >= 1 floats after msomn_set_const (else MSOM_ERR_STATE).  x, y [n] doubles, layer [n] ints, host or device
 *   pointers.  A value that is not finite, a position outside the box or a layer outside [0, nl): MSOM_ERR_ARG, nothing is allocated
 *   and earlier floats stay.  A start in a land cell is accepted.  A second begin replaces the first.  Sets option "floats" = 1.
 * msomn_floats_end: frees everything (as msomn_destroy and msomn_set_const do); without floats: MSOM_OK.
 * msomn_floats_get: the current positions in the caller's order, x, y [n], host or device.  Waits for the stream.
 * msomn_floats_velocity: (u, v) [n] at the current positions from the psi (+ psi_pg) the handle holds now.
 * msomn_floats_sample: out [n] = (1 - b) * ((1 - a) * P00 + a * P10) + b * ((1 - a) * P01 + a * P11) of any field of nl layers, in
 *   each float's layer, as the handle holds it.  A lost float gives NaN in both calls.
 * msomn_floats_stage: the advection by hand, for callers that drive msomn_update / msomn_advance themselves: stage 1 or 2 above with
 *   the psi the handle holds at the call.  Stage 2 without a stage 1 since msomn_floats_begin or the last stage 2: MSOM_ERR_STATE.
 * msomn_floats_record: a trajectory buffer [capacity][2 or 3][n] on the device; field: a field of nl layers to record along the
 *   trajectories, or < 0 for positions only.  Record 0 is the positions at the call and the sample of the field at them; after that
 *   one record is written behind every `every`-th msomn_step that moves the floats, by its stage-2 kernel: the new position and the
 *   bilinear value of the field there, in the float's layer.  At that point MSOMN_Q is q_{n + 1}, so a recorded q is q_{n + 1} at
 *   x_{n + 1}: PV on parcels.  Any other field is sampled as the handle holds it then; MSOMN_PSI is psi_{n + 1/2}.  A full buffer
 *   stops recording: "floats_dropped" counts the records that found no room.  Times are kept on the host.
 * msomn_floats_track: records first .. first + count - 1: t [count] (host memory), x, y, val [count][n] (host or device); any of the
 *   four may be NULL.  val on a recording without a field: MSOM_ERR_ARG.
 * msomn_get_param: "floats" (n, 0: none), "floats_records", "floats_dropped"; "floats_clamped", "floats_lost" (each waits for the
 *   stream); "floats_on_land": the floats that are not lost and whose current cell has mask == 0 at all four corners, counted on
 *   the device at the call.  msomn_set_option("floats", 0) pauses the stages of msomn_step, 1 resumes them; accepted and without
 *   effect on a handle without floats.
 * Errors: null handle or array, n < 1, stage not 1 or 2, dt not finite, every < 1, capacity < 1, a field that has not nl layers, a
 *   range outside the records written: MSOM_ERR_ARG; any call but begin / end without floats: MSOM_ERR_STATE; a handle of more than
 *   one tile without option floats_tiles: MSOM_ERR_CONFIG from every call, no field changed.  Every call names itself in
 *   msom_last_error.
 * The floats are not part of the state file: msomn_state_save writes the same bytes with and without them, msomn_state_load leaves
 *   them alone, and msomn_floats_get before the save, msomn_floats_begin after the load, at a step boundary, continues with the same
 *   bits.
 *
 * On tiles (msomn_create_tiled, more than one tile): msomn_set_option(m, "floats_tiles", 1), set before msomn_floats_begin and alike on
 *   every rank, makes the eight calls above accepted and COLLECTIVE: every rank makes the same call with the same arguments in the
 *   same order, as with msomn_step.  Default 0: MSOM_ERR_CONFIG as before.  On one tile the option has no effect.  The promise is the
 *   tile layer's: for every float id, positions, velocities, samples, records and the counters equal the single tile's bit for bit, in
 *   the strict and the product build.
 *   Owner: with i0, j0 of the formulas above on the GLOBAL grid, a float belongs to tile (i0 / Tx, j0 / Ty), Tx x Ty the cells of a
 *     tile.  The owner's corners are vertices it holds, its shared edges included, so no halo is read and nothing is exchanged for the
 *     floats but the floats themselves.  A position whose x * idx lies exactly on a seam belongs to the upper tile, x = L0 to the last.
 *     A float is homed by the position its next stage evaluates: (xh, yh) behind stage 1, (x, y) behind stage 2.  Behind every stage,
 *     in msomn_step and in msomn_floats_stage, one migration pass of two phases (W / E, then S / N over all residents, arrivals
 *     included: a diagonal move needs no diagonal message) takes every float to its owner, on the handle's stream and with no host
 *     wait but the transport's own.  Every id is resident on exactly one rank; a lost float stays where it is and is never read.
 *   Messages have the fixed size 1 + 6 K doubles; K is option "floats_msg_cap", 0 (default): min(n, max(1024, n / 16)).  A float that
 *     finds its message full, or whose owner is farther than a neighbouring tile, becomes lost on the sender: NaN from then on,
 *     counted in "floats_unsent" (and not in "floats_lost").
 *   msomn_floats_begin takes the same global arrays on every rank and keeps what the rank owns; ranks that pass different n, or of
 *     which one refuses its arrays, all answer MSOM_ERR_ARG before any float message is posted.  get, velocity, sample and track hand
 *     every rank the full arrays in the caller's order.  velocity and sample between a stage 1 and its stage 2 answer MSOM_ERR_STATE:
 *     the float is homed by (xh, yh) then, and (x, y) may lie on another tile; so does msomn_floats_record with a field.  A record's
 *     positions are written by the rank the float is resident on before the stage's pass, its field value by the new position's owner
 *     behind it.
 *   msomn_get_param: "floats_clamped", "floats_lost", "floats_unsent", "floats_migrated" (records sent) and "floats_on_land" are sums
 *     over the ranks and collective; "floats_resident" is the rank's own count; "floats_tiles", "floats_msg_cap" (the K in use once
 *     floats are begun).  On one tile: resident = n, unsent = migrated = 0.
 *   msomn_set_const and msomn_destroy drop the floats, as on one tile.  The model is untouched: Q, PSI, dt, the multigrid statistics
 *     and the count of halo exchanges of a run with floats equal those of the run without.
 */
#ifndef MSOMN_FLOATS_H
#define MSOMN_FLOATS_H

#include "msom.h"

#ifdef __cplusplus
extern "C" {
#endif

int msomn_floats_begin(msomn_t *m, int n, const double *x, const double *y, const int *layer);
int msomn_floats_end(msomn_t *m);
int msomn_floats_get(msomn_t *m, double *x, double *y);
int msomn_floats_velocity(msomn_t *m, double *u, double *v);
int msomn_floats_sample(msomn_t *m, int field, double *out);
int msomn_floats_stage(msomn_t *m, int stage, double dt);
int msomn_floats_record(msomn_t *m, int every, int capacity, int field);
int msomn_floats_track(msomn_t *m, int first, int count, double *t, double *x, double *y, double *val);

#ifdef __cplusplus
}
#endif
#endif
