// spec_inl.h -- the pieces of the wavenumber spectra (msom_spec_*) that the host and the device share: the in-place
// power-of-two transform of one line held in (padded) local memory, and the integer geometry of the radial bins.
// Everything here compiles for the host as well, so that tools/spec_host_check.cpp can run the butterflies and the bin
// ranges on a CPU against a direct sum.
#ifndef MSOM_SPEC_INL_H
#define MSOM_SPEC_INL_H

#ifdef __HIPCC__
#include "msom_internal.h"
#define SPEC_HD MSOM_HD
#else   // a plain C++ compiler (the host check): no HIP headers
#include <math.h>
#include <stddef.h>
struct double2 { double x, y; };
static inline double2 make_double2(double x, double y) { return double2{x, y}; }
#define SPEC_HD static inline
#endif

#define SPEC_MINN 8
#define SPEC_MAXN 4096   // one line of complex fp64 (64 KiB) and, in the column pass, two of them fit the 160 KiB of LDS
#define SPEC_NT 256      // threads per workgroup of the line kernels

// Line layout in LDS: one complex of padding after every 16.  A butterfly stage of span q has the lanes of a wavefront 4 q (the merged
// radix-4 stage) complex apart; ds_read_b128 serves 16 lanes at a time and a complex spans 4 of the 64 banks, so without the pad every
// power-of-two stride of 4 complex or more puts those 16 lanes on 4 bank groups or fewer.  With it the strides 4 and 16 are conflict-free
// and the strides of 64 and more (the first stages never have them: their lanes are 1 apart; the bit-reversed read-out does) are 4-way.
SPEC_HD int spec_pad(int i) { return i + (i >> 4); }
SPEC_HD int spec_line_len(int n) { return n + (n >> 4) + 1; }   // complex numbers of LDS for a line of n

SPEC_HD double2 spec_cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// The transform is decimation in frequency, in place, natural order in, bit-reversed order out: X[k] ends at index bitrev(k).
// tw[t] = exp(-2 pi i t / nt), t < nt / 2, from the host's long double table (rounded once); a line of n reads it at the stride nt / n.
// One radix-2 stage of span h (sub-transforms of 2 h): butterfly t of n / 2.
SPEC_HD void spec_bfly2(double2 *buf, int n, int h, int t, const double2 *tw, int tws) {
  const int j = t & (h - 1), i0 = ((t - j) << 1) + j, i1 = i0 + h;
  const double2 a = buf[spec_pad(i0)], b = buf[spec_pad(i1)];
  const double2 w = tw[(size_t)j * (n / (2 * h)) * tws];
  buf[spec_pad(i0)] = make_double2(a.x + b.x, a.y + b.y);
  buf[spec_pad(i1)] = spec_cmul(make_double2(a.x - b.x, a.y - b.y), w);
}
// Two radix-2 stages (spans h and q = h / 2) on the 4 numbers they couple, held in registers in between: butterfly t of n / 4.
// The second pair of the first stage has the twiddle of the first times exp(-i pi / 2) = -i; both pairs of the second stage share one.
SPEC_HD void spec_bfly4(double2 *buf, int n, int h, int t, const double2 *tw, int tws) {
  const int q = h >> 1, j = t & (q - 1), i0 = ((t - j) << 2) + j;
  const int p0 = spec_pad(i0), p1 = spec_pad(i0 + q), p2 = spec_pad(i0 + h), p3 = spec_pad(i0 + h + q);
  const double2 a0 = buf[p0], a1 = buf[p1], a2 = buf[p2], a3 = buf[p3];
  const double2 w1 = tw[(size_t)j * (n / (2 * h)) * tws], w2 = tw[(size_t)j * (n / h) * tws];
  const double2 s0 = make_double2(a0.x + a2.x, a0.y + a2.y), d0 = spec_cmul(make_double2(a0.x - a2.x, a0.y - a2.y), w1);
  const double2 s1 = make_double2(a1.x + a3.x, a1.y + a3.y);
  const double2 e1 = make_double2(a1.x - a3.x, a1.y - a3.y);
  const double2 d1 = spec_cmul(make_double2(e1.y, -e1.x), w1);   // (a1 - a3) * (-i) * w1
  buf[p0] = make_double2(s0.x + s1.x, s0.y + s1.y);
  buf[p1] = spec_cmul(make_double2(s0.x - s1.x, s0.y - s1.y), w2);
  buf[p2] = make_double2(d0.x + d1.x, d0.y + d1.y);
  buf[p3] = spec_cmul(make_double2(d0.x - d1.x, d0.y - d1.y), w2);
}
SPEC_HD int spec_log2(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}
SPEC_HD int spec_bitrev(int k, int log2n) {
  unsigned r = 0, u = (unsigned)k;
  for (int b = 0; b < log2n; b++) { r = (r << 1) | (u & 1u); u >>= 1; }
  return (int)r;
}

// ---- the radial bins (include/msom.h).  R2(i, j) = (i sx)^2 + (j sy)^2 on signed indices; shell s holds s^2 <= R2 < (s + 1)^2.
SPEC_HD int spec_isqrt(int v) {   // floor(sqrt(v)), v >= 0 (v <= 2 * 2048^2)
  int r = (int)sqrt((double)v);
  while (r * r > v) r--;
  while ((r + 1) * (r + 1) <= v) r++;
  return r;
}
// |j| range of row index I = |i| sx inside shell s: false if empty.  *jex = the |j| with R2 == s^2 exactly, or -1.
SPEC_HD bool spec_shell_range(int s, int I, int sy, int nyh, int *jlo, int *jhi, int *jex) {
  const int hi2 = (s + 1) * (s + 1) - 1 - I * I, lo2 = s * s - I * I;
  *jex = -1;
  if (hi2 < 0) return false;
  int Jlo = 0;
  if (lo2 > 0) {
    Jlo = spec_isqrt(lo2);
    if (Jlo * Jlo < lo2) Jlo++;
  }
  const int Jhi = spec_isqrt(hi2);
  *jlo = (Jlo + sy - 1) / sy;
  *jhi = Jhi / sy;
  if (*jhi > nyh) *jhi = nyh;
  if (*jlo > *jhi) return false;
  if (lo2 >= 0 && (*jlo) * sy * (*jlo) * sy == lo2) *jex = *jlo;
  return true;
}

#endif
