// kernels_spec.hip -- isotropic wavenumber spectra and spectral fluxes (msom_spec_*), gfx950 / CDNA4, fp64.
//
// Reference: get_spec_2D / radial_average / get_spec_1D / get_flux of msqg/scripts/fftlib.py, restated with integers in include/msom.h.
// One complex transform serves a pair of real fields: with Z = fft2(a + i b), P = Z(k) and Q = Z(-k),
//   Re(A conj B)(k) = Im(P Q) / 2          (SPEC_CROSS)
//   |A|^2 + |B|^2   = (|P|^2 + |Q|^2) / 2  (SPEC_SUM; with b = 0 this is |A|^2, the route of an auto-spectrum)
// and both are even in k, so only the half plane 0 <= kx index <= nx / 2 is formed; the other half counts through a weight of 2.
//
// Passes over a batch of layers:
//   k_spec_rows       one workgroup per row: load a + i b (from two arrays, or u + i v / g + 0 i formed from psi), transform the row in
//                     LDS, store Z[l][y][kx]
//   k_spec_transpose  Z -> ZT[l][kx][y] through 16 x 16 LDS tiles: 256-byte segments on both sides
//   k_spec_cols       one workgroup per pair of lines kx = n and (nx - n) mod nx of ZT: transform both in LDS, form spec_2D of line n
//                     and store it to V[l][n][ky] (8 bytes a point of the half plane; the transform itself is not written back);
//                     msom_spec_2d also gets the fftshift-ed plane from here
//   k_spec_shells     one workgroup per shell s = floor(sqrt(R2)): the sum T[s] over the shell and E[s] over its points with R2 == s^2,
//                     every thread over its lines in ascending order, then a fixed tree: no atomics, the same bits on every run
//   k_spec_final      bin[r] = T[r] + E[r + 1] (both ends of a bin are inclusive), flux[r] = sum of T[s], s from the top down to r + 1
#include "kernels.h"
#include "spec_inl.h"

// every stage of the line transform, all threads of the workgroup; a barrier after each
__device__ __forceinline__ void spec_line_fft(double2 *buf, int n, const double2 *__restrict__ tw, int tws) {
  int h = n >> 1;
  for (; h >= 2; h >>= 2) {
    for (int t = threadIdx.x; t < (n >> 2); t += SPEC_NT) spec_bfly4(buf, n, h, t, tw, tws);
    __syncthreads();
  }
  if (h == 1) {
    for (int t = threadIdx.x; t < (n >> 1); t += SPEC_NT) spec_bfly2(buf, n, 1, t, tw, tws);
    __syncthreads();
  }
}

// ------------------------------------------------------------------ rows

__global__ void __launch_bounds__(SPEC_NT) k_spec_rows(SpecIn in, int nx, int ny, int log2nx, double2 *__restrict__ Z, const double2 *__restrict__ tw,
                                                        int tws) {
  extern __shared__ double2 spec_lds[];
  const int y = blockIdx.x, l = blockIdx.y;
  const size_t base = in.off + (size_t)(in.l0 + l) * in.ls + (size_t)y * in.pitch;
  for (int x = threadIdx.x; x < nx; x += SPEC_NT) {
    const size_t c = base + x;
    double re, im;
    if (in.mode == SPEC_IN_AB) {
      re = in.a[c];
      im = in.b ? in.b[c] : 0.;
    } else if (in.mode == SPEC_IN_UV) {   // u, v of the msom_stats_* block; the ghost values of psi are read
#ifdef MSOM_STRICT
      re = (in.a[c - in.pitch] - in.a[c + in.pitch]) / in.D2;
      im = (in.a[c + 1] - in.a[c - 1]) / in.D2;
#else
      re = (in.a[c - in.pitch] - in.a[c + in.pitch]) * in.rD2;
      im = (in.a[c + 1] - in.a[c - 1]) * in.rD2;
#endif
    } else {                              // g_l = sqrt(S_l) (psi_l+1 - psi_l) / dhc_l
      re = sqrt(in.b[c]) * (in.a[c + in.ls] - in.a[c]) / in.dhc[in.l0 + l];
      im = 0.;
    }
    spec_lds[spec_pad(x)] = make_double2(re, im);
  }
  __syncthreads();
  spec_line_fft(spec_lds, nx, tw, tws);
  double2 *zr = Z + ((size_t)l * ny + y) * nx;
  for (int k = threadIdx.x; k < nx; k += SPEC_NT) zr[k] = spec_lds[spec_pad((int)(__brev((unsigned)k) >> (32 - log2nx)))];
}

// ------------------------------------------------------------------ transpose

#define SPEC_TT 16
__global__ void __launch_bounds__(SPEC_TT *SPEC_TT) k_spec_transpose(const double2 *__restrict__ Z, double2 *__restrict__ ZT, int nx, int ny) {
  __shared__ double2 tile[SPEC_TT][SPEC_TT + 1];
  const size_t lo = (size_t)blockIdx.z * nx * ny;
  const int x0 = blockIdx.x * SPEC_TT, y0 = blockIdx.y * SPEC_TT;
  int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x < nx && y < ny) tile[threadIdx.y][threadIdx.x] = Z[lo + (size_t)y * nx + x];
  __syncthreads();
  x = x0 + threadIdx.y; y = y0 + threadIdx.x;
  if (x < nx && y < ny) ZT[lo + (size_t)x * ny + y] = tile[threadIdx.x][threadIdx.y];
}

// ------------------------------------------------------------------ columns

// line n of the half plane (0 <= n <= nx / 2) of layer blockIdx.y.  V[l][n][m], m the unsigned ky index.
// out2d (or null): the fftshift-ed plane [l][ny][nx]; line n and, through the symmetry, line nx - n
__global__ void __launch_bounds__(SPEC_NT) k_spec_cols(const double2 *__restrict__ ZT, int nx, int ny, int log2ny, int kind, double scale,
                                                        double *__restrict__ V, double *__restrict__ out2d, const double2 *__restrict__ tw, int tws) {
  extern __shared__ double2 spec_lds[];
  const int n = blockIdx.x, l = blockIdx.y, nm = (nx - n) & (nx - 1);
  const bool self = nm == n;   // n = 0 and n = nx / 2
  double2 *bp = spec_lds, *bq = self ? spec_lds : spec_lds + spec_line_len(ny);
  const double2 *zp = ZT + ((size_t)l * nx + n) * ny, *zq = ZT + ((size_t)l * nx + nm) * ny;
  for (int y = threadIdx.x; y < ny; y += SPEC_NT) {
    bp[spec_pad(y)] = zp[y];
    if (!self) bq[spec_pad(y)] = zq[y];
  }
  __syncthreads();
  spec_line_fft(bp, ny, tw, tws);
  if (!self) spec_line_fft(bq, ny, tw, tws);
  const int sh = 32 - log2ny, hx = nx >> 1, hy = ny >> 1;
  double *vr = V + ((size_t)l * (hx + 1) + n) * ny;
  for (int m = threadIdx.x; m < ny; m += SPEC_NT) {
    const int mm = (ny - m) & (ny - 1);
    const double2 P = bp[spec_pad((int)(__brev((unsigned)m) >> sh))], Q = bq[spec_pad((int)(__brev((unsigned)mm) >> sh))];
    double v;
    if (kind == SPEC_CROSS) v = 0.5 * (P.x * Q.y + P.y * Q.x);
    else v = 0.5 * ((P.x * P.x + P.y * P.y) + (Q.x * Q.x + Q.y * Q.y));
    v *= scale;
    vr[m] = v;
    if (out2d) {
      double *o = out2d + (size_t)l * nx * ny;
      o[(size_t)((m + hy) & (ny - 1)) * nx + ((n + hx) & (nx - 1))] = v;
      if (!self) o[(size_t)((mm + hy) & (ny - 1)) * nx + ((nm + hx) & (nx - 1))] = v;
    }
  }
}

// ------------------------------------------------------------------ shells

// TE[l][0][s] = T[s], TE[l][1][s] = E[s], s = blockIdx.x <= smax
__global__ void __launch_bounds__(SPEC_NT) k_spec_shells(const double *__restrict__ V, int nx, int ny, int sx, int sy, int smax, double *__restrict__ TE) {
  const int s = blockIdx.x, l = blockIdx.y, hx = nx >> 1, hy = ny >> 1;
  double t = 0., e = 0.;
  for (int n = threadIdx.x; n <= hx; n += SPEC_NT) {
    int jlo, jhi, jex;
    if (!spec_shell_range(s, n * sx, sy, hy, &jlo, &jhi, &jex)) continue;
    const double *vr = V + ((size_t)l * (hx + 1) + n) * ny;
    double a = 0., x = 0.;
    for (int j = jlo; j <= jhi; j++) {
      const double v = (j == 0 || j == hy) ? vr[j] : vr[j] + vr[ny - j];   // j and -j; -ny/2 has no partner, 0 is its own
      a += v;
      if (j == jex) x = v;
    }
    const double w = (n == 0 || n == hx) ? 1. : 2.;   // line nx - n holds the same values
    t += w * a;
    e += w * x;
  }
  __shared__ double st[SPEC_NT], se[SPEC_NT];
  st[threadIdx.x] = t;
  se[threadIdx.x] = e;
  __syncthreads();
  for (int o = SPEC_NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      st[threadIdx.x] += st[threadIdx.x + o];
      se[threadIdx.x] += se[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *o = TE + (size_t)l * 2 * (smax + 1);
    o[s] = st[0];
    o[smax + 1 + s] = se[0];
  }
}

// res[l][0][r] = bin sum, res[l][1][r] = flux
__global__ void __launch_bounds__(SPEC_NT) k_spec_final(const double *__restrict__ TE, int smax, int nbins, double dk2, double *__restrict__ res) {
  const int r = blockIdx.x * SPEC_NT + threadIdx.x, l = blockIdx.y;
  if (r >= nbins) return;
  const double *T = TE + (size_t)l * 2 * (smax + 1), *E = T + smax + 1;
  double f = 0.;
  for (int s = smax; s > r; s--) f += T[s];
  res[((size_t)l * 2) * nbins + r] = T[r] + E[r + 1];
  res[((size_t)l * 2 + 1) * nbins + r] = f * dk2;
}

// ------------------------------------------------------------------ launchers

static size_t spec_lds_bytes(int n, int lines) { return (size_t)lines * spec_line_len(n) * sizeof(double2); }
// the line kernels ask for up to 2 lines of 4096 (139 KiB) of dynamic LDS: above the 64 KiB a launch gets unasked
int spec_prepare_device() {
  static int done = 0;
  if (done) return 0;
  const int big = (int)spec_lds_bytes(SPEC_MAXN, 2);
  if (hipFuncSetAttribute((const void *)k_spec_rows, hipFuncAttributeMaxDynamicSharedMemorySize, big) != hipSuccess) return -1;
  if (hipFuncSetAttribute((const void *)k_spec_cols, hipFuncAttributeMaxDynamicSharedMemorySize, big) != hipSuccess) return -1;
  done = 1;
  return 0;
}
void launch_spec_rows(hipStream_t st, const SpecIn &in, int nx, int ny, int layers, double2 *Z, const double2 *tw, int nt) {
  hipLaunchKernelGGL(k_spec_rows, dim3(ny, layers), dim3(SPEC_NT), spec_lds_bytes(nx, 1), st, in, nx, ny, spec_log2(nx), Z, tw, nt / nx);
}
void launch_spec_transpose(hipStream_t st, const double2 *Z, double2 *ZT, int nx, int ny, int layers) {
  hipLaunchKernelGGL(k_spec_transpose, dim3((nx + SPEC_TT - 1) / SPEC_TT, (ny + SPEC_TT - 1) / SPEC_TT, layers), dim3(SPEC_TT, SPEC_TT), 0, st, Z, ZT, nx, ny);
}
void launch_spec_cols(hipStream_t st, const double2 *ZT, int nx, int ny, int layers, int kind, double scale, double *V, double *out2d, const double2 *tw,
                      int nt) {
  hipLaunchKernelGGL(k_spec_cols, dim3(nx / 2 + 1, layers), dim3(SPEC_NT), spec_lds_bytes(ny, 2), st, ZT, nx, ny, spec_log2(ny), kind, scale, V, out2d, tw,
                     nt / ny);
}
void launch_spec_shells(hipStream_t st, const double *V, int nx, int ny, int layers, int smax, double *TE) {
  const int nmax = nx > ny ? nx : ny;
  hipLaunchKernelGGL(k_spec_shells, dim3(smax + 1, layers), dim3(SPEC_NT), 0, st, V, nx, ny, nmax / nx, nmax / ny, smax, TE);
}
void launch_spec_final(hipStream_t st, const double *TE, int smax, int nbins, int layers, double dk2, double *res) {
  hipLaunchKernelGGL(k_spec_final, dim3((nbins + SPEC_NT - 1) / SPEC_NT, layers), dim3(SPEC_NT), 0, st, TE, smax, nbins, dk2, res);
}
