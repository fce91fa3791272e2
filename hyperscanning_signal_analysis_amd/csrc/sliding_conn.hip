// Sliding-window dDTF and GPDC on top of K1 / K2 (and, for dDTF, K3's fused ffDTF) -- the per-window forms of
// `direct_dtf` (/root/reference/src/mtmvar.py:341-385) and `gen_partial_directed_coherence` (mtmvar.py:388-468).
//
// dDTF.  The reference builds S = H V H^T (plain transpose, mtmvar.py:199) with H = A^-1, takes the minors of S
// (partial_coherence, mtmvar.py:287-338) and returns ffDTF * |kappa|, kappa_ij = M_ij / sqrt(M_ii M_jj).  With
// M_ij = (-1)^(i+j) det S (S^-1)_ji and S^-1 = A^T V^-1 A =: W(f), |det S| cancels:
//     |kappa_ij| = |W_ji| / sqrt(|W_ii| |W_jj|)            (1 on the diagonal, 0 where the denominator vanishes)
// No minor, no determinant, no second inversion.  A(f) = sum_{k=0..p} A_k z^k with A_0 = I, A_k = -ar_k and
// z = exp(-2 pi i f / fs), so with V = L L^T and B_k = L^-1 A_k
//     W(f) = sum_{d=0..2p} G_d z^d,     G_d = sum_{k+l=d} B_k^T B_l        (real, symmetric)
// W is a trigonometric polynomial with 2p + 1 real coefficient matrices per WINDOW: they cost (p+1)^2 real MP^3
// products once per window (v_mfma_f64_16x16x4_f64), and every frequency after that is a Horner evaluation of 2p + 1
// terms per matrix element -- instead of building, multiplying and inverting complex matrices per (window, frequency).
//   ddtf_factor_kernel   one workgroup per window: L = chol(V) (V not positive definite: info_yw = -(column + 1)),
//                        B_0 = L^-1, B_k = -L^-1 ar_k
//   ddtf_gram_kernel     one workgroup per (window, d): G_d on the f64 MFMA
//   ddtf_apply_kernel    one workgroup per (window, 64 frequencies): |W_ii| first, then every pair i < j once,
//                        out_ij = ff_ij |kappa_ij|, out_ji = ff_ji |kappa_ij|, out_ii = ff_ii (kappa_ii = 1);
//                        |kappa_ij| = |W_ij| r_i r_j with r_i = 1 / sqrt|W_ii| (0 where W_ii = 0: the reference's
//                        "denominator == 0 -> 0")
// GPDC.  GPDC_ij(f) = (|A_ij| / sigma_i) / sqrt(sum_k |A_kj|^2 / sigma_k^2) needs A(f) and diag(V) only: no inversion.
//   gpdc_sliding_kernel  one workgroup per (window, column j, 64 frequencies): A(:, j) is built on chip from ar and the
//                        twiddles of hmv_twiddles_f64 and never written; the output is the reference's (m, m, F) array.
#include "../../include/hypermvar.h"
#include "hmv_common.h"
#include "hmv_kernels.h"

namespace hmv {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// grid: n_items; block 256.  ar [item][MP][MP][p], V [item][MP][MP] -> B [item][p+1][MP][MP] (zero padding).
__global__ void __launch_bounds__(256) ddtf_factor_kernel(const double* ar, const double* V, int* info_yw, double* B, int m,
                                                          int MP, int p) {
  __shared__ double Ls[64][65];      // V, then L (lower triangle); later ar_k
  __shared__ double Xs[64][65];      // L^-1
  const long long item = blockIdx.x;
  const int t = threadIdx.x;
  const size_t TILE = (size_t)MP * MP;
  const double* Vi = V + item * TILE;
  for (int e = t; e < 64 * 64; e += 256) {
    const int i = e >> 6, j = e & 63;
    Ls[i][j] = (i < m && j < m) ? Vi[(size_t)i * MP + j] : 0.0;
    Xs[i][j] = 0.0;
  }
  // right-looking Cholesky; every thread reads the same pivot after a barrier, so the failure exit is uniform
  int bad = 0;
  for (int c = 0; c < m; ++c) {
    __syncthreads();
    const double d = Ls[c][c];
    if (!(d > 0.0) || !(d < INFINITY)) {
      bad = c + 1;
      break;
    }
    const double lc = sqrt(d);
    __syncthreads();
    for (int i = c + t; i < m; i += 256) Ls[i][c] = (i == c) ? lc : Ls[i][c] / lc;
    __syncthreads();
    const int r = m - c - 1;
    for (int e = t; e < r * r; e += 256) {
      const int i = c + 1 + e / r, j = c + 1 + e % r;
      if (j <= i) Ls[i][j] -= Ls[i][c] * Ls[j][c];
    }
  }
  __syncthreads();
  double* Bi = B + item * (p + 1) * TILE;
  if (bad) {
    if (t == 0 && info_yw[item] == 0) info_yw[item] = -bad;
    for (size_t e = t; e < (p + 1) * TILE; e += 256) Bi[e] = 0.0;
    return;
  }
  // X = L^-1, one column per thread (forward substitution; column j is zero above row j)
  if (t < m) {
    const int j = t;
    for (int i = j; i < m; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int r = j; r < i; ++r) s -= Ls[i][r] * Xs[r][j];
      Xs[i][j] = s / Ls[i][i];
    }
  }
  __syncthreads();
  const int j = t & 63, i0 = t >> 6;
  if (j < MP)
    for (int i = i0; i < MP; i += 4) Bi[(size_t)i * MP + j] = Xs[i][j];
  for (int k = 1; k <= p; ++k) {
    __syncthreads();                                   // previous ar_k consumed
    const double* ak = ar + item * TILE * p + (k - 1);
    for (int e = t; e < 64 * 64; e += 256) {
      const int r = e >> 6, c = e & 63;
      Ls[r][c] = (r < m && c < m) ? ak[((size_t)r * MP + c) * p] : 0.0;
    }
    __syncthreads();
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0;
    for (int r = 0; r < m; ++r) {
      const double a = Ls[r][j];
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] += Xs[i0 + 4 * q][r] * a;
    }
    double* Bk = Bi + k * TILE;
    if (j < MP)
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (i0 + 4 * q < MP) Bk[(size_t)(i0 + 4 * q) * MP + j] = -acc[q];
  }
}

// grid: n_items * (2p+1); block 256.  G_d = sum_{k+l=d} B_k^T B_l on v_mfma_f64_16x16x4_f64: lane l supplies
// A[i = l&15][r = l>>4] = B_k[r][i] and B[r = l>>4][j = l&15] = B_l[r][j] (both 16-double runs of a row of B), and holds
// D[row = (l>>4) + 4 q][col = l&15] in element q (the f64 C/D map).  Wave w owns the 16 x 16 tiles w, w + 4, ...
template <int NT>
__global__ void __launch_bounds__(256) ddtf_gram_kernel(const double* B, double* G, int p) {
  constexpr int MP = 16 * NT, TILE = MP * MP, NS = (NT * NT + 3) / 4;
  const int D = 2 * p + 1;
  const long long item = blockIdx.x / D;
  const int d = blockIdx.x % D;
  const int w = uni(threadIdx.x >> 6), l = threadIdx.x & 63;
  const double* Bi = B + item * (p + 1) * (size_t)TILE;
  f64x4 acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int k_lo = d > p ? d - p : 0, k_hi = d < p ? d : p;
  for (int k = k_lo; k <= k_hi; ++k) {
    const double* X = Bi + (size_t)k * TILE + (l >> 4) * MP + (l & 15);
    const double* Y = Bi + (size_t)(d - k) * TILE + (l >> 4) * MP + (l & 15);
#pragma unroll
    for (int r0 = 0; r0 < MP; r0 += 4) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int tt = w + 4 * s;
        if (tt < NT * NT) {
          const int I = tt / NT, J = tt % NT;
          const double a = X[r0 * MP + 16 * I], b = Y[r0 * MP + 16 * J];
          acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
        }
      }
    }
  }
  double* Gd = G + (item * D + d) * (size_t)TILE;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int tt = w + 4 * s;
    if (tt < NT * NT) {
      const int I = tt / NT, J = tt % NT;
#pragma unroll
      for (int q = 0; q < 4; ++q) Gd[(size_t)(16 * I + (l >> 4) + 4 * q) * MP + 16 * J + (l & 15)] = acc[s][q];
    }
  }
}

// W_ij(f) by Horner's rule in z = exp(-2 pi i f / fs) over G_{2p} .. G_0 (element (i, j) of each); two elements at a
// time, so that two independent chains are in flight
__device__ __forceinline__ double2 horner_w(const double* g, size_t stride, int D, double zr, double zi) {
  double re = 0.0, im = 0.0;
  for (int d = D - 1; d >= 0; --d) {
    const double nr = re * zr - im * zi + g[(size_t)d * stride];
    im = re * zi + im * zr;
    re = nr;
  }
  return make_double2(re, im);
}
__device__ __forceinline__ void horner_w2(const double* g, size_t stride, int D, double zr, double zi, double2& v0,
                                          double2& v1) {
  double r0 = 0.0, i0 = 0.0, r1 = 0.0, i1 = 0.0;
  for (int d = D - 1; d >= 0; --d) {
    const double n0 = r0 * zr - i0 * zi + g[(size_t)d * stride];
    const double n1 = r1 * zr - i1 * zi + g[(size_t)d * stride + 1];
    i0 = r0 * zi + i0 * zr;
    i1 = r1 * zi + i1 * zr;
    r0 = n0;
    r1 = n1;
  }
  v0 = make_double2(r0, i0);
  v1 = make_double2(r1, i1);
}

// grid: n_items * ceil(F/64); block 256.  ff, out: [item][m][m][F] (out may be ff: every element is read and written by
// the same thread).  Lane = frequency, so every row of the output is written in 512-byte runs.  Wave w takes rows
// w, w + 4, ... and, per row i, the pairs (i, j > i) two at a time (between 480 and 528 pairs per wave at 64 channels).
__global__ void __launch_bounds__(256) ddtf_apply_kernel(const double* G, const double* freqs, double fs, const double* ff,
                                                         double* out, int F, int m, int MP, int p) {
  __shared__ double rs[64][64];                        // 1 / sqrt|W_ii| of this block's frequencies (0 where W_ii = 0)
  const int D = 2 * p + 1, nft = (F + 63) / 64;
  const long long item = blockIdx.x / nft;
  const int f0 = (blockIdx.x % nft) * 64;
  const int w = uni(threadIdx.x >> 6), l = threadIdx.x & 63;
  const int f = f0 + l;
  const bool on = f < F;
  const double th = (double)(-2) * 3.141592653589793 * (on ? freqs[f] : 0.0) / fs;    // twiddle_kernel's order, k = 1
  double zi, zr;
  sincos(th, &zi, &zr);
  const size_t TILE = (size_t)MP * MP;
  const double* Gi = G + item * D * TILE;
  const size_t base = (size_t)item * m * m * F + f;
  for (int i = w; i < m; i += 4) {
    const double2 v = horner_w(Gi + (size_t)i * MP + i, TILE, D, zr, zi);
    const double a = sqrt(v.x * v.x + v.y * v.y);
    rs[i][l] = (a != 0.0) ? 1.0 / sqrt(a) : 0.0;
    const size_t oii = base + ((size_t)i * m + i) * F;
    if (on) out[oii] = ff[oii];                        // kappa_ii = 1
  }
  __syncthreads();
  for (int i = w; i < m; i += 4) {
    const double ri = rs[i][l];
    int j = i + 1;
    for (; j + 1 < m; j += 2) {
      double2 v0, v1;
      horner_w2(Gi + (size_t)i * MP + j, TILE, D, zr, zi, v0, v1);
      const double k0 = sqrt(v0.x * v0.x + v0.y * v0.y) * ri * rs[j][l];
      const double k1 = sqrt(v1.x * v1.x + v1.y * v1.y) * ri * rs[j + 1][l];
      if (on) {
        const size_t oij = base + ((size_t)i * m + j) * F, oji = base + ((size_t)j * m + i) * F;
        out[oij] = ff[oij] * k0;
        out[oji] = ff[oji] * k0;
        out[oij + F] = ff[oij + F] * k1;
        out[oji + (size_t)m * F] = ff[oji + (size_t)m * F] * k1;
      }
    }
    if (j < m) {
      const double2 v = horner_w(Gi + (size_t)i * MP + j, TILE, D, zr, zi);
      const double k = sqrt(v.x * v.x + v.y * v.y) * ri * rs[j][l];
      if (on) {
        const size_t oij = base + ((size_t)i * m + j) * F, oji = base + ((size_t)j * m + i) * F;
        out[oij] = ff[oij] * k;
        out[oji] = ff[oji] * k;
      }
    }
  }
}

// grid: n_items * m * ceil(F/64); block 256.  ar [item][MP][MP][p], V [item][MP][MP], tw [F][p][2] ->
// out [item][m][m][F].  Wave w builds rows w, w + 4, ... of column j of A(f) (lane = frequency) in the reference's
// operation order (A = I; A -= ar_k z_k, mtmvar.py:156-158), keeps |A_ij| in registers and adds |A_ij|^2 / sigma_i^2.
__global__ void __launch_bounds__(256) gpdc_sliding_kernel(const double* ar, const double* V, const double* tw, double* out,
                                                           int F, int m, int MP, int p) {
  __shared__ double zc[HMV_MAX_ORDER][64], zs[HMV_MAX_ORDER][64];
  __shared__ double part[4][64];
  const int nft = (F + 63) / 64;
  long long b = blockIdx.x;
  const int ft = (int)(b % nft);
  b /= nft;
  const int j = (int)(b % m);
  const long long item = b / m;
  const int w = uni(threadIdx.x >> 6), l = threadIdx.x & 63;
  const int f0 = ft * 64, f = f0 + l;
  const bool on = f < F;
  for (int e = threadIdx.x; e < p * 64; e += 256) {
    const int k = e >> 6, ll = e & 63;
    const bool in = f0 + ll < F;
    zc[k][ll] = in ? tw[((size_t)(f0 + ll) * p + k) * 2] : 0.0;
    zs[k][ll] = in ? tw[((size_t)(f0 + ll) * p + k) * 2 + 1] : 0.0;
  }
  __syncthreads();
  const size_t TILE = (size_t)MP * MP;
  const double* ari = ar + item * TILE * p;
  const double* Vi = V + item * TILE;
  double mag[16];
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = w + 4 * q;
    mag[q] = 0.0;
    if (i < m) {
      double re = (i == j) ? 1.0 : 0.0, im = 0.0;
      const double* a = ari + ((size_t)i * MP + j) * p;
      for (int k = 0; k < p; ++k) {
        const double c = a[k];
        re -= c * zc[k][l];
        im -= c * zs[k][l];
      }
      const double ab = hypot(re, im);
      mag[q] = ab;
      acc += (ab * ab) / Vi[(size_t)i * MP + i];
    }
  }
  part[w][l] = acc;
  __syncthreads();
  const double cs = sqrt(part[0][l] + part[1][l] + part[2][l] + part[3][l]);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = w + 4 * q;
    if (i < m && on) {
      const double g = (cs != 0.0) ? (mag[q] / sqrt(Vi[(size_t)i * MP + i])) / cs : 0.0;
      out[(((size_t)item * m + i) * m + j) * F + f] = g;
    }
  }
}

int launch_ddtf_factor(const double* ar, const double* V, int* info_yw, double* B, long long n_items, int m, int m_pad, int p,
                       hipStream_t st) {
  if (n_items == 0) return 0;
  hipLaunchKernelGGL(ddtf_factor_kernel, dim3((unsigned)n_items), dim3(256), 0, st, ar, V, info_yw, B, m, m_pad, p);
  return (int)hipGetLastError();
}

int launch_ddtf_sliding(const DdtfArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0 || a.F == 0) return 0;
  const int D = 2 * a.p + 1;
  hipLaunchKernelGGL(ddtf_factor_kernel, dim3((unsigned)a.n_items), dim3(256), 0, st, a.ar, a.V, a.info_yw, a.B, a.m, m_pad,
                     a.p);
  const dim3 gg((unsigned)(a.n_items * D));
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(ddtf_gram_kernel<nt>, gg, dim3(256), 0, st, a.B, a.G, a.p); })) return -3;
  const int nft = (a.F + 63) / 64;
  hipLaunchKernelGGL(ddtf_apply_kernel, dim3((unsigned)(a.n_items * nft)), dim3(256), 0, st, a.G, a.freqs, a.fs, a.ff, a.out,
                     a.F, a.m, m_pad, a.p);
  return (int)hipGetLastError();
}

int launch_gpdc_sliding(const double* ar, const double* V, const double* tw, double* out, long long n_items, int F, int m,
                        int m_pad, int p, hipStream_t st) {
  if (n_items == 0 || F == 0) return 0;
  if (p < 1 || p > HMV_MAX_ORDER) return -3;
  const long long nb = n_items * m * ((F + 63) / 64);
  hipLaunchKernelGGL(gpdc_sliding_kernel, dim3((unsigned)nb), dim3(256), 0, st, ar, V, tw, out, F, m, m_pad, p);
  return (int)hipGetLastError();
}

}  // namespace hmv
