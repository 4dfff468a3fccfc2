// spec_host_check.cpp -- the shared pieces of the wavenumber spectra (msom_amd/csrc/spec_inl.h) on a CPU, no HIP: the line transform
// against a direct DFT in long double, and the whole chain of passes of kernels_spec.hip (rows, transpose, paired columns, shells, bins and
// fluxes) replayed with the same index arithmetic against a brute-force evaluation of the contract of include/msom.h.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/spec_host_check.cpp -o spec_host_check && ./spec_host_check
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../msom_amd/csrc/spec_inl.h"

static int fails = 0;
static void report(const char *what, double err, double tol) {
  const bool ok = err <= tol;
  printf("%-46s err %.3e (tol %.1e): %s\n", what, err, tol, ok ? "ok" : "FAIL");
  if (!ok) fails++;
}
static std::vector<double2> table(int nt) {
  std::vector<double2> tw(nt / 2);
  for (int t = 0; t < nt / 2; t++) {
    const long double a = -2.0L * 3.14159265358979323846264338327950288L * t / nt;
    tw[t] = make_double2((double)cosl(a), (double)sinl(a));
  }
  return tw;
}
// the stage loop of spec_line_fft, threads replayed one after the other (a stage only couples the numbers of one butterfly)
static void line_fft(double2 *buf, int n, const double2 *tw, int tws) {
  int h = n >> 1;
  for (; h >= 2; h >>= 2)
    for (int t = 0; t < (n >> 2); t++) spec_bfly4(buf, n, h, t, tw, tws);
  if (h == 1)
    for (int t = 0; t < (n >> 1); t++) spec_bfly2(buf, n, 1, t, tw, tws);
}
static double rnd() { return rand() / (double)RAND_MAX - 0.3; }

static void check_line(int n, int nt) {
  const std::vector<double2> tw = table(nt);
  std::vector<double2> x(n), buf(spec_line_len(n));
  for (auto &v : x) v = make_double2(rnd(), rnd());
  for (int i = 0; i < n; i++) buf[spec_pad(i)] = x[i];
  line_fft(buf.data(), n, tw.data(), nt / n);
  const int lg = spec_log2(n);
  double err = 0, mx = 0;
  for (int k = 0; k < n; k += (n > 512 ? 37 : 1)) {   // long lines: a sample of the outputs
    long double re = 0, im = 0;
    for (int i = 0; i < n; i++) {
      const long double a = -2.0L * 3.14159265358979323846264338327950288L * ((long)k * i % n) / n;
      re += x[i].x * cosl(a) - x[i].y * sinl(a);
      im += x[i].x * sinl(a) + x[i].y * cosl(a);
    }
    const double2 g = buf[spec_pad(spec_bitrev(k, lg))];
    err = std::max(err, std::max(fabs((double)(g.x - re)), fabs((double)(g.y - im))));
    mx = std::max(mx, std::max(fabs((double)re), fabs((double)im)));
  }
  char what[64];
  snprintf(what, sizeof what, "line transform n = %d (table of %d)", n, nt);
  report(what, err / mx, 8 * lg * 2.2e-16);
}

// the chain of passes on one layer; kind 0: Re(A conj B), 1: |A|^2 + |B|^2
static void check_chain(int nx, int ny, int kind) {
  const int nmax = std::max(nx, ny), sx = nmax / nx, sy = nmax / ny, nb = nmax / 2 - 2, hx = nx / 2, hy = ny / 2;
  const std::vector<double2> tw = table(nmax);
  std::vector<double> a(nx * ny), b(nx * ny);
  for (auto &v : a) v = rnd();
  for (auto &v : b) v = rnd();
  // rows
  std::vector<double2> Z(nx * ny), ZT(nx * ny), buf(2 * spec_line_len(nmax));
  for (int y = 0; y < ny; y++) {
    for (int x = 0; x < nx; x++) buf[spec_pad(x)] = make_double2(a[y * nx + x], b[y * nx + x]);
    line_fft(buf.data(), nx, tw.data(), nmax / nx);
    for (int k = 0; k < nx; k++) Z[y * nx + k] = buf[spec_pad(spec_bitrev(k, spec_log2(nx)))];
  }
  for (int y = 0; y < ny; y++)
    for (int x = 0; x < nx; x++) ZT[x * ny + y] = Z[y * nx + x];
  // paired columns
  std::vector<double> V((hx + 1) * ny), o2d(nx * ny, -1e300);
  for (int n = 0; n <= hx; n++) {
    const int nm = (nx - n) & (nx - 1);
    const bool self = nm == n;
    double2 *bp = buf.data(), *bq = self ? bp : bp + spec_line_len(ny);
    for (int y = 0; y < ny; y++) {
      bp[spec_pad(y)] = ZT[n * ny + y];
      if (!self) bq[spec_pad(y)] = ZT[nm * ny + y];
    }
    line_fft(bp, ny, tw.data(), nmax / ny);
    if (!self) line_fft(bq, ny, tw.data(), nmax / ny);
    for (int m = 0; m < ny; m++) {
      const int mm = (ny - m) & (ny - 1), lg = spec_log2(ny);
      const double2 P = bp[spec_pad(spec_bitrev(m, lg))], Q = bq[spec_pad(spec_bitrev(mm, lg))];
      const double v = kind == 0 ? 0.5 * (P.x * Q.y + P.y * Q.x) : 0.5 * ((P.x * P.x + P.y * P.y) + (Q.x * Q.x + Q.y * Q.y));
      V[n * ny + m] = v;
      o2d[((m + hy) & (ny - 1)) * nx + ((n + hx) & (nx - 1))] = v;
      if (!self) o2d[((mm + hy) & (ny - 1)) * nx + ((nm + hx) & (nx - 1))] = v;
    }
  }
  // shells
  int smax = 0;
  while ((smax + 1) * (smax + 1) <= 2 * (nmax / 2) * (nmax / 2)) smax++;
  std::vector<double> T(smax + 1, 0.), E(smax + 1, 0.);
  for (int s = 0; s <= smax; s++)
    for (int n = 0; n <= hx; n++) {
      int jlo, jhi, jex;
      if (!spec_shell_range(s, n * sx, sy, hy, &jlo, &jhi, &jex)) continue;
      const double *vr = &V[n * ny];
      const double w = (n == 0 || n == hx) ? 1. : 2.;
      for (int j = jlo; j <= jhi; j++) {
        const double v = (j == 0 || j == hy) ? vr[j] : vr[j] + vr[ny - j];
        T[s] += w * v;
        if (j == jex) E[s] += w * v;
      }
    }
  // brute force: direct DFTs in long double, every point of the plane, the membership rule as written in the header
  std::vector<long double> ref2d(nx * ny), bin(nb, 0.L), flux(nb, 0.L);
  std::vector<long> cnt(nb, 0);
  const long double tp = 2.0L * 3.14159265358979323846264338327950288L;
  for (int j = -hy; j < hy; j++)
    for (int i = -hx; i < hx; i++) {
      long double ar = 0, ai = 0, br = 0, bi = 0;
      for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++) {
          const long double ph = -tp * ((long double)(((long)i * x) % nx) / nx + (long double)(((long)j * y) % ny) / ny);
          ar += a[y * nx + x] * cosl(ph); ai += a[y * nx + x] * sinl(ph);
          br += b[y * nx + x] * cosl(ph); bi += b[y * nx + x] * sinl(ph);
        }
      const long double v = kind == 0 ? ar * br + ai * bi : ar * ar + ai * ai + br * br + bi * bi;
      ref2d[(j + hy) * nx + (i + hx)] = v;
      const long R2 = (long)(i * sx) * (i * sx) + (long)(j * sy) * (j * sy);
      for (int r = 0; r < nb; r++) {
        if ((long)r * r <= R2 && R2 <= (long)(r + 1) * (r + 1)) { bin[r] += v; cnt[r]++; }
        if ((long)(r + 1) * (r + 1) <= R2) flux[r] += v;
      }
    }
  double e2 = 0, eb = 0, ef = 0, m2 = 0, mb = 0, mf = 0;
  for (int k = 0; k < nx * ny; k++) { e2 = std::max(e2, fabs((double)(o2d[k] - ref2d[k]))); m2 = std::max(m2, fabs((double)ref2d[k])); }
  for (int r = 0; r < nb; r++) {
    long double f = 0;
    for (int s = smax; s > r; s--) f += T[s];
    eb = std::max(eb, fabs((double)(T[r] + E[r + 1] - bin[r]))); mb = std::max(mb, fabs((double)bin[r]));
    ef = std::max(ef, fabs((double)(f - flux[r]))); mf = std::max(mf, fabs((double)flux[r]));
  }
  char what[80];
  snprintf(what, sizeof what, "%d x %d kind %d: plane", nx, ny, kind); report(what, e2 / m2, 1e-13);
  snprintf(what, sizeof what, "%d x %d kind %d: bin sums", nx, ny, kind); report(what, eb / mb, 1e-13);
  snprintf(what, sizeof what, "%d x %d kind %d: fluxes", nx, ny, kind); report(what, ef / mf, 1e-13);
}

int main() {
  srand(7);
  for (int n = 8; n <= 4096; n *= 2) check_line(n, n);
  check_line(8, 4096);
  check_line(64, 1024);
  const int shapes[][2] = {{8, 8}, {16, 16}, {32, 8}, {8, 64}, {32, 32}};
  for (auto &s : shapes)
    for (int kind = 0; kind < 2; kind++) check_chain(s[0], s[1], kind);
  printf(fails ? "FAILED: %d\n" : "all ok\n", fails);
  return fails != 0;
}
