// Model validation -- the residuals of every window's MVAR fit and the whiteness statistics of their lag covariances
// (include/hypermvar.h, "Model validation"; DESIGN.md has the definitions).  Beyond the reference, which computes the
// residual covariance (ar_coeff, src/mtmvar.py:119) but never the residuals.
//
//   resid_pack_kernel   ar [item][MP][MP][p] (lag fastest: a poor operand read) -> -A_k in resid_kernel's A-operand order,
//                       once per item (the `arx` precedent of K3); the padding is packed as zeros whatever ar holds there.
//   resid_kernel<NT>    E = X[:, p:] - sum_k A_k X[:, p-k : n-k], a GEMM MP x (MP p) x N per window on
//                       v_mfma_f64_4x4x4_4b_f64, built like lagcov_kernel: one workgroup = one window x 64 residual columns,
//                       the chunk staged in LDS with its p preceding samples (row stride 6 mod 32 doubles), wave w owns the
//                       row strip 4 NT w .. of the MP x 64 output tile as NT x 4 accumulators (D layout, hmv_common.h).
//                       The accumulators are seeded with x_i[t]; the products follow in a fixed order -- lags ascending,
//                       then source channel ascending -- so an element's bits depend on its window alone.
//   whiteness_kernel<NT>  one workgroup per window: Cholesky C_0 = L L^T in LDS, X = L^-1, then per lag
//                       s_l = ||X C_l X^T||_F^2, the residual correlations r_l, their count above the threshold and the
//                       per-channel Ljung-Box sums.  Every reduction is a fixed tree over the 256 threads: no atomics.
// The lag covariances between the two are K1 itself (launch_lagcov over E as n_items recordings of N samples).
#include "hmv_common.h"
#include "hmv_kernels.h"
#include <cmath>

namespace hmv {

constexpr int RS_TC = 64;                     // residual columns per workgroup
constexpr int RS_HALO = 32;                   // max order: preceding samples staged with the chunk
constexpr int RS_S = RS_TC + RS_HALO + 6;     // 102 = 6 (mod 32), K1's row stride

// arp[item][lag][Ib][jb][k][i] = -ar[item][4 Ib + i][4 jb + k][lag]: the 16 doubles a wave reads as the A operand of the
// k-step (lag, source channels 4 jb ..) for its row block Ib are contiguous, and consecutive jb follow each other.
// grid: n_items, block 256.
__global__ void __launch_bounds__(256) resid_pack_kernel(const double* ar, double* arp, int m, int MP, int p) {
  const long long item = blockIdx.x;
  const int NB = MP >> 2;
  const size_t per = (size_t)MP * MP * p;
  const double* src = ar + item * per;
  double* dst = arp + item * per;
  for (size_t e = threadIdx.x; e < per; e += 256) {
    const int i = e & 3, k = (e >> 2) & 3;
    const size_t blk = e >> 4;
    const int jb = blk % NB, Ib = (blk / NB) % NB, lag = blk / ((size_t)NB * NB);
    const int row = 4 * Ib + i, col = 4 * jb + k;
    dst[e] = (row < m && col < m) ? -src[((size_t)row * MP + col) * p + lag] : 0.0;
  }
}

// grid (items, ceil(N / 64)), block 256.
template <int NT>
__global__ void __launch_bounds__(256, 2) resid_kernel(ResidArgs a) {
  constexpr int MP = 16 * NT, NB = MP / 4;
  __shared__ double xs[MP * RS_S];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int c0 = blockIdx.y * RS_TC;               // first residual column of this workgroup = first staged sample
  const int n = a.n, m = a.m, p = a.p, N = n - p;
  const double* x = a.x + a.item_rec[item] * a.rec_stride + a.item_start[item];

  // samples c0 .. c0 + 95 of the window: the chunk's 64 targets t = p + c0 + col and their p predecessors; samples past
  // the window end and channels past m are staged as zeros
  constexpr int W = RS_TC + RS_HALO;
  constexpr int NLD = (MP * W + 255) / 256;
  {
    double stg[NLD];
#pragma unroll
    for (int r = 0; r < NLD; ++r) {                  // all loads in flight, then the LDS stores
      const int idx = threadIdx.x + 256 * r;
      const int ch = idx / W, tt = idx - ch * W;
      const int t = c0 + tt;
      stg[r] = (idx < MP * W && ch < m && t < n) ? x[(size_t)ch * a.ld + t] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = threadIdx.x + 256 * r;
      const int ch = idx / W, tt = idx - ch * W;
      if (idx < MP * W) xs[ch * RS_S + tt] = stg[r];
    }
  }
  __syncthreads();

  const int i = l >> 4, cc = l & 15;
  double acc[NT][4];
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int J = 0; J < 4; ++J) acc[I][J] = xs[(4 * (NT * wv + I) + i) * RS_S + p + 16 * J + cc];   // x_i[t]

  // A operand: lane 16 k + 4 b + i holds -A_lag[4 Ib + i][4 jb + k] (the same for the four blocks b);
  // B operand: lane 16 k + 4 b + j holds x[4 jb + k][t - lag] of the chunk column 4 b + j of the column group J
  const double* ap = a.arp + (size_t)item * p * MP * MP + (size_t)(NT * wv) * NB * 16 + (l >> 4) * 4 + (l & 3);
  for (int lag = 1; lag <= p; ++lag) {
    const double* apk = ap + (size_t)(lag - 1) * NB * NB * 16;
    const double* xb = xs + (l >> 4) * RS_S + cc + p - lag;
#pragma unroll 4
    for (int jb = 0; jb < NB; ++jb) {
      double av[NT], bv[4];
#pragma unroll
      for (int I = 0; I < NT; ++I) av[I] = apk[(I * NB + jb) * 16];
#pragma unroll
      for (int J = 0; J < 4; ++J) bv[J] = xb[4 * jb * RS_S + 16 * J];
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < 4; ++J) acc[I][J] = mfma4(av[I], bv[J], acc[I][J]);
    }
  }

  double* E = a.E + (size_t)item * m * a.ldE;
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int J = 0; J < 4; ++J) {
      const int row = 4 * (NT * wv + I) + i, col = c0 + 16 * J + cc;
      if (row < m && col < N) E[(size_t)row * a.ldE + col] = acc[I][J];     // columns >= N and channels >= m are masked
    }
}

__global__ void __launch_bounds__(256) iota_items_kernel(long long* item_rec, long long* item_start, long long n) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) {
    item_rec[k] = k;
    item_start[k] = 0;
  }
}

// sum over the 256 threads by a fixed halving tree in LDS (all threads receive it); `red` is free again on return
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// grid: n_items, block 256.  Thread (bi, bj) = (t >> 4, t & 15) owns the elements (bi + 16 a, bj + 16 b), a, b < NT, of
// every MP x MP product: the row operand is a broadcast per 16 lanes, the column operand runs over consecutive doubles
// (C_l) or over rows of odd stride MP + 1 (X^T), both conflict-free.
template <int NT>
__global__ void __launch_bounds__(256) whiteness_kernel(WhiteArgs a) {
  constexpr int MP = 16 * NT, LD = MP + 1, TILE = MP * MP;
  __shared__ double Ls[MP * LD];      // C_0, then L (lower triangle); later C_l
  __shared__ double Xs[MP * LD];      // X = L^-1, exact zeros above the diagonal
  __shared__ double Ts[MP * LD];      // X C_l
  __shared__ double dg[MP];           // diagonal of C_0
  __shared__ double red[256];
  const long long item = blockIdx.x;
  const int t = threadIdx.x;
  const int m = a.m, h = a.h;
  const double* C = a.C + (size_t)item * (h + 1) * TILE;
  for (int e = t; e < TILE; e += 256) {
    const int i = e / MP, j = e - i * MP;
    const double v = C[e];
    if (a.resid_cov) a.resid_cov[(size_t)item * TILE + e] = v;
    Ls[i * LD + j] = (i < m && j < m) ? v : 0.0;
    Xs[i * LD + j] = 0.0;
    if (i == j) dg[i] = v;
  }
  // right-looking Cholesky; every thread reads the same pivot after a barrier, so the failure exit is uniform
  int bad = 0;
  for (int c = 0; c < m; ++c) {
    __syncthreads();
    const double d = Ls[c * LD + c];
    if (!(d > 0.0) || !(d < INFINITY)) {
      bad = c + 1;
      break;
    }
    const double lc = sqrt(d);
    __syncthreads();
    for (int i = c + t; i < m; i += 256) Ls[i * LD + c] = (i == c) ? lc : Ls[i * LD + c] / lc;
    __syncthreads();
    const int r = m - c - 1;
    for (int e = t; e < r * r; e += 256) {
      const int i = c + 1 + e / r, j = c + 1 + e % r;
      if (j <= i) Ls[i * LD + j] -= Ls[i * LD + c] * Ls[j * LD + c];
    }
  }
  __syncthreads();
  if (bad) {
    const double nan = __builtin_nan("");
    for (int e = t; e < h; e += 256) a.s[(size_t)item * h + e] = nan;
    for (int e = t; e < m; e += 256) a.q_ch[(size_t)item * m + e] = nan;
    if (t < 3) a.q[(size_t)item * 3 + t] = nan;
    if (t == 0) {
      a.acf_count[item] = -1;
      a.info[item] = bad;
    }
    return;
  }
  // X = L^-1, one column per thread (forward substitution; column j is zero above row j)
  if (t < m) {
    const int j = t;
    for (int i = j; i < m; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int r = j; r < i; ++r) s -= Ls[i * LD + r] * Xs[r * LD + j];
      Xs[i * LD + j] = s / Ls[i * LD + i];
    }
  }
  const int bi = t >> 4, bj = t & 15;
  const double N = (double)a.N;
  int cnt = 0;
  double qc = 0.0, sum_bp = 0.0, sum_h = 0.0;       // qc: thread i < m, channel i; the sums: thread 0
  for (int lag = 1; lag <= h; ++lag) {
    __syncthreads();                                  // X complete / the previous C_l consumed
    const double* Cl = C + (size_t)lag * TILE;
    for (int e = t; e < TILE; e += 256) {
      const int i = e / MP, j = e - i * MP;
      const bool in = i < m && j < m;
      const double v = in ? Cl[e] : 0.0;
      Ls[i * LD + j] = v;
      if (in) cnt += fabs(v / sqrt(dg[i] * dg[j])) > a.acf_thr;
    }
    __syncthreads();
    if (t < m) {
      const double r = Ls[t * LD + t] / sqrt(dg[t] * dg[t]);
      qc += r * r / (N - (double)lag);
    }
    double acc[NT][NT];
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int v = 0; v < NT; ++v) acc[u][v] = 0.0;
    for (int k = 0; k < m; ++k) {                     // T = X C_l
      double xv[NT], cv[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) xv[u] = Xs[(bi + 16 * u) * LD + k];
#pragma unroll
      for (int v = 0; v < NT; ++v) cv[v] = Ls[k * LD + bj + 16 * v];
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int v = 0; v < NT; ++v) acc[u][v] = __builtin_fma(xv[u], cv[v], acc[u][v]);
    }
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int v = 0; v < NT; ++v) {
        Ts[(bi + 16 * u) * LD + bj + 16 * v] = acc[u][v];
        acc[u][v] = 0.0;
      }
    __syncthreads();
    for (int k = 0; k < m; ++k) {                     // M = T X^T
      double tv[NT], xv[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u) tv[u] = Ts[(bi + 16 * u) * LD + k];
#pragma unroll
      for (int v = 0; v < NT; ++v) xv[v] = Xs[(bj + 16 * v) * LD + k];
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int v = 0; v < NT; ++v) acc[u][v] = __builtin_fma(tv[u], xv[v], acc[u][v]);
    }
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int v = 0; v < NT; ++v)
        if (bi + 16 * u < m && bj + 16 * v < m) ss = __builtin_fma(acc[u][v], acc[u][v], ss);
    const double sl = block_sum(ss, red);
    if (t == 0) {
      a.s[(size_t)item * h + lag - 1] = sl;
      sum_bp += sl;
      sum_h += sl / (N - (double)lag);
    }
  }
  // the count: integers, any order gives the same sum
  __shared__ int redi[256];
  redi[t] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) redi[t] += redi[t + s];
    __syncthreads();
  }
  if (t < m) a.q_ch[(size_t)item * m + t] = N * (N + 2.0) * qc;
  if (t == 0) {
    const double q_bp = N * sum_bp;
    a.q[(size_t)item * 3 + 0] = q_bp;
    a.q[(size_t)item * 3 + 1] = q_bp + (double)m * m * h * (h + 1) / (2.0 * N);
    a.q[(size_t)item * 3 + 2] = N * N * sum_h;
    a.acf_count[item] = redi[0];
    a.info[item] = 0;
  }
}

long long resid_pack_doubles(long long n_items, int m_pad, int p) { return n_items * (long long)m_pad * m_pad * p; }

int launch_residuals(const ResidArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  if (a.p < 1 || a.p > RS_HALO || a.n <= a.p) return -2;
  hipLaunchKernelGGL(resid_pack_kernel, dim3((unsigned)a.n_items), dim3(256), 0, st, a.ar, a.arp, a.m, m_pad, a.p);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const dim3 grid((unsigned)a.n_items, (unsigned)((a.n - a.p + RS_TC - 1) / RS_TC)), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(resid_kernel<nt>, grid, block, 0, st, a); })) return -1;
  return (int)hipGetLastError();
}

int launch_iota_items(long long* item_rec, long long* item_start, long long n, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(iota_items_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, item_rec, item_start, n);
  return (int)hipGetLastError();
}

int launch_whiteness(const WhiteArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(whiteness_kernel<nt>, grid, block, 0, st, a); })) return -1;
  return (int)hipGetLastError();
}

}  // namespace hmv
