// helm_inl.h -- host state of the modal PV inversion: nl independent mg_solve loops (mspg/elliptic.h:145-229) that share their
// launches.  Plain C++, no HIP: msom_helm.hip drives it with the maxima the device returns, tools/helm_host_check.cpp with a script.
//
// A cycle of the batch is a cycle of every mode that still wants one.  helm_counts gives the sweeps each mode takes in it -- its own
// nrelax, or 0 for a frozen mode (TOLERANCE met after NITERMIN cycles, or NITERMAX done) -- and helm_cycle_done books the cycle on
// the modes that ran: i, resa, the 1.2 / 10 rule on nrelax, resb.  A frozen mode's numbers no longer change.
#ifndef MSOM_HELM_INL_H
#define MSOM_HELM_INL_H

#include "../../include/msom.h"

struct HelmSolve {
  int nl, nitermin, nitermax, have_first;
  double tol;
  msom_mgstats s[MSOM_MAXNL];
  double resb[MSOM_MAXNL];   // residual before the next cycle (mg_solve's local resb)
};

static inline void helm_begin(HelmSolve &h, int nl, int nitermin, int nitermax, double tol) {
  h.nl = nl; h.nitermin = nitermin; h.nitermax = nitermax; h.tol = tol; h.have_first = 0;
  for (int m = 0; m < MSOM_MAXNL; m++) {
    h.s[m].i = 0; h.s[m].nrelax = 4; h.s[m].resb = h.s[m].resa = h.s[m].sum = 0.;
    h.resb[m] = 0.;
  }
}
// the residual of the warm start and the sum of the right-hand side, per mode (read before the first cycle where NITERMIN < 1,
// else together with the first cycle's result)
static inline void helm_first(HelmSolve &h, const double *res0, const double *sum) {
  if (h.have_first) return;
  for (int m = 0; m < h.nl; m++) {
    h.resb[m] = h.s[m].resb = h.s[m].resa = res0[m];
    h.s[m].sum = sum[m];
  }
  h.have_first = 1;
}
// mg_solve's loop condition.  Before helm_first resa is unknown: only NITERMIN can ask for the cycle (the caller reads first otherwise)
static inline bool helm_wants(const HelmSolve &h, int m) {
  const msom_mgstats &s = h.s[m];
  return s.i < h.nitermax && (s.i < h.nitermin || (h.have_first && s.resa > h.tol));
}
// sweeps per mode of the next cycle; returns their maximum (0: every mode is frozen, the solve is over)
static inline int helm_counts(const HelmSolve &h, int *count) {
  int mx = 0;
  for (int m = 0; m < h.nl; m++) {
    count[m] = helm_wants(h, m) ? h.s[m].nrelax : 0;
    if (count[m] > mx) mx = count[m];
  }
  return mx;
}
// resa[m]: max |res_m| after the cycle that ran with `count`
static inline void helm_cycle_done(HelmSolve &h, const int *count, const double *resa) {
  for (int m = 0; m < h.nl; m++) {
    if (count[m] <= 0) continue;
    msom_mgstats &s = h.s[m];
    s.resa = resa[m];
    if (s.resa > h.tol) {
      if (h.resb[m] / s.resa < 1.2 && s.nrelax < 100) s.nrelax++;
      else if (h.resb[m] / s.resa > 10 && s.nrelax > 2) s.nrelax--;
    }
    h.resb[m] = s.resa;
    s.i++;
  }
}

#endif
