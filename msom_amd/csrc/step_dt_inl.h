// step_dt_inl.h -- the step-size arithmetic of the time loop, written once for the host (limiter and dtnext of msom_api.hip, the
// newqg dialect, msomn_step) and for the device (k_step_dt).  Plain values in and out, no handle: both models call it.  No
// contraction in either build and correctly rounded divisions, so the host and the device form the same numbers.
#ifndef STEP_DT_INL_H
#define STEP_DT_INL_H

#include <hip/hip_runtime.h>
#include <math.h>

// one call of timestep() [Basilisk; algorithm text newqg/qg.h:202-219] with its static `previous`
__host__ __device__ inline double step_limit(double umax, double dtmax, double D, double CFL, double *previous) {
#pragma clang fp contract(off)
  dtmax /= CFL;
  if (umax != 0.) {
    const double dt = D / umax;
    if (dt < dtmax) dtmax = dt;
  }
  dtmax *= CFL;
  if (dtmax > *previous) dtmax = (*previous + 0.1 * dtmax) / 1.1;
  *previous = dtmax;
  return dtmax;
}

// dtnext() [Basilisk, SURVEY App. B]: dt shortened so that a whole number of steps lands on the event time tnext;
// *tnext_out: the time after this step
__host__ __device__ inline double step_dtnext(double t, double tnext, double dt, double *tnext_out) {
#pragma clang fp contract(off)
  if (tnext != HUGE_VAL && tnext > t) {
    const unsigned int n = (unsigned int)((tnext - t) / dt);
    if (n == 0) dt = tnext - t;
    else {
      const double dt1 = (tnext - t) / n;
      if (dt1 > dt * (1. + 1e-9)) dt = (tnext - t) / (n + 1);
      else if (dt1 < dt) dt = dt1;
      tnext = t + dt;
    }
  } else
    tnext = t + dt;
  *tnext_out = tnext;
  return dt;
}

#endif
