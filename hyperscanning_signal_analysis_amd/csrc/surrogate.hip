// Surrogate significance of the sliding-window measures: the surrogate windows and the per-cell null statistics.
//
// A block of surrogates x windows is laid out surrogate-major: item k = s * n_win + w (surrogate s of window w).
//   surrogate_shift_kernel    one workgroup per (item, channel): window w of its recording, the channels >= split read
//                             circularly shifted by shift[s][rec] (wrapping past T) -> item buffer [item][m][n]
//   surrogate_phase_kernel    one thread per (item, channel, bin): the window's spectrum times exp(i phi[s][c][bin]);
//                             bin 0 and, for even n, bin n/2 are copied -> [item][m][n/2 + 1] (the inverse transform
//                             is rocFFT plumbing in the engine)
//   null_valid_kernel         one thread per window: n_valid += surrogates of the block whose fit succeeded
//   null_max_kernel           one workgroup per (item, band): M = max of the surrogate's values over the tested pairs
//   null_accumulate_kernel    one thread per (window, i, j, band): exceedance counts, the Welford mean / M2, walked in
//                             surrogate order (no atomics: the bits do not depend on how the surrogates are blocked),
//                             and, when asked, the p-values, null mean and null std from the running state
#include <math.h>

#include <algorithm>

#include "../../include/hypermvar.h"
#include "hmv_common.h"
#include "hmv_kernels.h"

namespace hmv {

// grid: n_surr * n_win * m; block 256.  The caller has checked that every window lies inside its recording.
__global__ void __launch_bounds__(256) surrogate_shift_kernel(const double* __restrict__ x, long long rec_stride, long long ld,
                                                              long long T, const long long* __restrict__ item_rec,
                                                              const long long* __restrict__ item_start, long long n_win,
                                                              const long long* __restrict__ shift, long long n_rec, int m,
                                                              int n, int split, double* __restrict__ out) {
  const long long row = blockIdx.x;                 // (s * n_win + w) * m + c
  const int c = (int)(row % m);
  const long long k = row / m;
  const long long w = k % n_win, s = k / n_win;
  const long long r = item_rec[w];
  const double* src = x + r * rec_stride + (long long)c * ld;
  double* dst = out + row * n;
  long long base = item_start[w];
  if (c < split) {
    for (int t = threadIdx.x; t < n; t += 256) dst[t] = src[base + t];
    return;
  }
  long long d = shift[s * n_rec + r] % T;
  if (d < 0) d += T;
  base += d;
  if (base >= T) base -= T;                         // base in [0, T), t < n <= T: one wrap at most
  for (int t = threadIdx.x; t < n; t += 256) {
    long long u = base + t;
    if (u >= T) u -= T;
    dst[t] = src[u];
  }
}

// grid-stride over n_surr * n_win * m * nf complex outputs.
__global__ void __launch_bounds__(256) surrogate_phase_kernel(const double2* __restrict__ spec, long long n_win,
                                                              const double* __restrict__ phi, int n_surr, int m, int nf, int n,
                                                              double2* __restrict__ out) {
#pragma clang fp contract(off)
  const long long total = (long long)n_surr * n_win * m * nf;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int f = (int)(e % nf);
    const long long row = e / nf;                   // (s * n_win + w) * m + c
    const int c = (int)(row % m);
    const long long k = row / m;
    const long long w = k % n_win, s = k / n_win;
    const double2 z = spec[(w * m + c) * nf + f];
    if (f == 0 || 2 * f == n) {                     // the real bins stay what they are
      out[e] = z;
      continue;
    }
    double sn, cs;
    sincos(phi[(s * m + c) * nf + f], &sn, &cs);
    out[e] = make_double2(z.x * cs - z.y * sn, z.x * sn + z.y * cs);
  }
}

// grid: ceil(n_win / 256); block 256.
__global__ void __launch_bounds__(256) null_valid_kernel(const unsigned char* __restrict__ bad, long long n_win, int n_surr,
                                                         int* __restrict__ n_valid) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_win) return;
  int v = n_valid[w];
  for (int s = 0; s < n_surr; ++s) v += bad[s * n_win + w] ? 0 : 1;
  n_valid[w] = v;
}

// grid: n_items * nb; block 256.  NaN values are skipped (a comparison with NaN is false); -inf if nothing is left.
__global__ void __launch_bounds__(256) null_max_kernel(const double* __restrict__ surr, const unsigned char* __restrict__ tested,
                                                       int m, int nb, double* __restrict__ M) {
  __shared__ double red[256];
  const long long ib = blockIdx.x;                  // item * nb + b
  const int b = (int)(ib % nb);
  const long long item = ib / nb;
  const int t = threadIdx.x;
  const double* v = surr + item * m * m * nb + b;
  double best = -INFINITY;
  for (int k = t; k < m * m; k += 256)
    if (tested[k]) {
      const double u = v[(long long)k * nb];
      if (u > best) best = u;
    }
  red[t] = best;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h && red[t + h] > red[t]) red[t] = red[t + h];
    __syncthreads();
  }
  if (t == 0) M[ib] = red[0];
}

// grid: ceil(n_win * m * m * nb / 256); block 256.  Cell = (w * m * m + i * m + j) * nb + b.
__global__ void __launch_bounds__(256) null_accumulate_kernel(
    const double* __restrict__ obs, const double* __restrict__ surr, const unsigned char* __restrict__ bad,
    const unsigned char* __restrict__ tested, const double* __restrict__ M, long long n_win, int n_surr, int m, int nb,
    const int* __restrict__ n_valid, int* __restrict__ cnt, int* __restrict__ cnt_fwe, int* __restrict__ n_cell,
    double* __restrict__ mean, double* __restrict__ m2, double* __restrict__ p, double* __restrict__ p_fwe,
    double* __restrict__ null_mean, double* __restrict__ null_std) {
#pragma clang fp contract(off)
  const long long per_win = (long long)m * m * nb;
  const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cell >= n_win * per_win) return;
  const long long w = cell / per_win;
  const long long in_win = cell - w * per_win;      // (i * m + j) * nb + b
  const int b = (int)(in_win % nb);
  if (!tested[in_win / nb]) {
    if (p) p[cell] = p_fwe[cell] = null_mean[cell] = null_std[cell] = NAN;
    return;
  }
  const double o = obs[cell];
  int c = cnt[cell], cf = cnt_fwe[cell], k = n_cell[cell];
  double mu = mean[cell], s2 = m2[cell];
  for (int s = 0; s < n_surr; ++s) {
    const long long item = s * n_win + w;
    if (bad[item]) continue;
    if (M[item * nb + b] >= o) ++cf;
    const double v = surr[item * per_win + in_win];
    if (v != v) continue;
    if (v >= o) ++c;
    ++k;
    const double dlt = v - mu;
    mu += dlt / k;
    s2 += dlt * (v - mu);
  }
  cnt[cell] = c; cnt_fwe[cell] = cf; n_cell[cell] = k;
  mean[cell] = mu; m2[cell] = s2;
  if (p) {
    const double den = 1.0 + n_valid[w];
    p[cell] = (1.0 + c) / den;
    p_fwe[cell] = (1.0 + cf) / den;
    null_mean[cell] = k > 0 ? mu : NAN;
    null_std[cell] = k > 1 ? sqrt(s2 / (k - 1)) : NAN;
  }
}

int launch_surrogate_shift(const double* x, long long rec_stride, long long ld, long long T, const long long* item_rec,
                           const long long* item_start, long long n_win, const long long* shift, long long n_rec, int n_surr,
                           int m, int n, int split, double* out, hipStream_t st) {
  const long long rows = (long long)n_surr * n_win * m;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(surrogate_shift_kernel, dim3((unsigned)rows), dim3(256), 0, st, x, rec_stride, ld, T, item_rec, item_start,
                     n_win, shift, n_rec, m, n, split, out);
  return (int)hipGetLastError();
}

int launch_surrogate_phase(const double* spec, long long n_win, const double* phi, int n_surr, int m, int n, double* out,
                           hipStream_t st) {
  const int nf = n / 2 + 1;
  const long long total = (long long)n_surr * n_win * m * nf;
  if (total == 0) return 0;
  const long long blocks = std::min<long long>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(surrogate_phase_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                     reinterpret_cast<const double2*>(spec), n_win, phi, n_surr, m, nf, n, reinterpret_cast<double2*>(out));
  return (int)hipGetLastError();
}

int launch_null_accumulate(const NullAccArgs& a, hipStream_t st) {
  if (a.n_win == 0) return 0;
  const long long items = (long long)a.n_surr * a.n_win;
  const long long cells = a.n_win * a.m * a.m * a.nb;
  hipLaunchKernelGGL(null_valid_kernel, dim3((unsigned)((a.n_win + 255) / 256)), dim3(256), 0, st, a.bad, a.n_win, a.n_surr,
                     a.n_valid);
  hipLaunchKernelGGL(null_max_kernel, dim3((unsigned)(items * a.nb)), dim3(256), 0, st, a.surr, a.tested, a.m, a.nb, a.M);
  hipLaunchKernelGGL(null_accumulate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, a.obs, a.surr, a.bad,
                     a.tested, a.M, a.n_win, a.n_surr, a.m, a.nb, a.n_valid, a.cnt, a.cnt_fwe, a.n_cell, a.mean, a.m2, a.p,
                     a.p_fwe, a.null_mean, a.null_std);
  return (int)hipGetLastError();
}

}  // namespace hmv
