// Block (multivariate) Granger causality between two groups of channels, per window: Geweke's time-domain values and his
// spectral decomposition.  Channels 0 .. split-1 are block A, split .. m-1 block B.  Not in the reference project; pinned
// to the textbook definition (tests/block_gc_restated.py).
//
// With the order-p Yule-Walker fit (ar, V =: Sigma) of the window, A(f) = I - sum_k ar_k z^k (z: hmv_twiddles_f64),
// H = A^-1 and S(f) = H Sigma H^H -- the CONJUGATE transpose, not the plain transpose of multivariate_spectra / K5 --
//     f_{s->d}(f) = ln det S_dd - ln det(S_dd - H_ds Sigma_{s|d} H_ds^H),      Sigma_{s|d} = Sigma_ss - Sigma_sd Sigma_dd^-1 Sigma_ds.
// Evaluated without H and without S (DESIGN.md has the derivation):
//     f_{s->d}(f) = ln det Sigma_{s|d} + ln det W_ss(f) - 2 ln |det At_ss(f)|
//     W(f)  = A^H Sigma^-1 A,   W_ss(f) = C_0 + sum_{d=1..p} (C_d z^d + C_d^T conj(z)^d),   C_d = sum_k (B_k)_{:,s}^T (B_{k+d})_{:,s}
//     At_ss(f) = A_ss - Sigma_sd Sigma_dd^-1 A_ds = sum_{k=0..p} D_k z^k,                   D_k = (A_k)_ss - Sigma_sd Sigma_dd^-1 (A_k)_ds
// with B_k = L^-1 A_k, Sigma = L L^T (ddtf_factor_kernel's output), A_0 = I, A_k = -ar_k.  C_d and D_k are real and belong
// to the WINDOW; a frequency costs two polynomial evaluations, one complex Hermitian Cholesky and one complex LU with
// partial pivoting, all n_src x n_src.  Direction 0 is A -> B (src = A), direction 1 is B -> A.
//   bgc_gather_kernel   one workgroup per (window, lag): R_k[X, X] of both blocks in the MP layout of their own padded
//                       sizes, K1's padding (identity on the padded lag-0 diagonal, zero elsewhere): input of the two
//                       restricted K2 runs
//   bgc_gram_kernel     one workgroup per (window, d, direction): C_d on v_mfma_f64_4x4x4_4b_f64
//   bgc_prep_kernel     one workgroup per window: the five Cholesky log-determinants and the time-domain values, and per
//                       direction Sigma_sd Sigma_dd^-1, ln det Sigma_{s|d} and D_k; a pivot of Sigma, Sigma_dd or
//                       Sigma_{s|d} that is not positive goes to info_yw where that is still 0
//   bgc_time_kernel     one workgroup per window: what bgc_prep_kernel does for the time-domain values and nothing else --
//                       the log-determinants of Sigma, Sigma_AA, Sigma_BB and of the two restricted residual covariances
//                       (or those read from a table of observed windows, BgcArgs::red_base); one LDS matrix, not two
//   bgc_freq_kernel     one group of lanes (a power of two >= n_src, at least 8) per (window, frequency), one launch per
//                       direction sized by n_src: W_ss and At_ss are built and factorised in the group's own slab of LDS,
//                       lane = matrix row
#include "../../include/hypermvar.h"
#include "hmv_common.h"
#include "hmv_kernels.h"

namespace hmv {

namespace {
__device__ __forceinline__ int bgc_s0(int dir, int split) { return dir ? split : 0; }
__device__ __forceinline__ int bgc_ns(int dir, int split, int m) { return dir ? m - split : split; }

// In-place Cholesky of the leading n x n block (lower triangle) by the 256 threads of a workgroup; returns the sum of the
// logs of the pivots (= ln det) or NaN, and in *bad the 1-based column of the first pivot that is not positive and finite.
// Every thread reads the same pivot after a barrier, so the exit is uniform.
__device__ double chol_logdet_256(double (*A)[65], int n, int t, int* bad) {
  double ld = 0.0;
  *bad = 0;
  for (int c = 0; c < n; ++c) {
    __syncthreads();
    const double d = A[c][c];
    if (!(d > 0.0) || !(d < INFINITY)) {
      *bad = c + 1;
      break;
    }
    ld += log(d);
    const double lc = sqrt(d);
    __syncthreads();
    for (int i = c + t; i < n; i += 256) A[i][c] = (i == c) ? lc : A[i][c] / lc;
    __syncthreads();
    const int r = n - c - 1;
    for (int e = t; e < r * r; e += 256) {
      const int i = c + 1 + e / r, j = c + 1 + e % r;
      if (j <= i) A[i][j] -= A[i][c] * A[j][c];
    }
  }
  __syncthreads();
  return *bad ? NAN : ld;
}

// The time-domain values of one window, the tail bgc_prep_kernel and bgc_time_kernel share: ln det of the two restricted
// residual covariances -- factorised here (Ls is free by now), or read from row base_a / base_b of a table that an earlier
// call wrote through red_out, with the infos that went with them -- then time, info_red and red_out.  Uniform per workgroup.
__device__ void bgc_time_values(double (*Ls)[65], const BgcRed& r, long long item, int t, double ld_full, const double* ld_blk,
                                int m, int MPa, int MPb, int split) {
  double ld_r[2];
  int ir[2], bad;
  for (int X = 0; X < 2; ++X) {
    if (r.red_base) {
      const long long row = (X ? r.base_b : r.base_a)[item];
      ld_r[X] = r.red_base[row * 2 + X];
      ir[X] = r.info_red_base[row * 2 + X];
      continue;
    }
    const int nx = bgc_ns(X, split, m), MPx = X ? MPb : MPa;
    const double* Vr = (X ? r.VrB : r.VrA) + (size_t)item * MPx * MPx;
    ir[X] = (X ? r.info_rB : r.info_rA)[item];
    __syncthreads();
    for (int e = t; e < nx * nx; e += 256) Ls[e / nx][e % nx] = Vr[(size_t)(e / nx) * MPx + e % nx];
    ld_r[X] = chol_logdet_256(Ls, nx, t, &bad);
    if (bad && ir[X] == 0) ir[X] = -bad;
  }
  if (t == 0) {
    const double fab = ld_r[1] - ld_blk[1], fba = ld_r[0] - ld_blk[0], fi = ld_blk[0] + ld_blk[1] - ld_full;
    double* ti = r.time + item * 4;
    ti[0] = fab;
    ti[1] = fba;
    ti[2] = fi;
    ti[3] = fab + fba + fi;
    r.info_red[item * 2] = ir[0];
    r.info_red[item * 2 + 1] = ir[1];
    if (r.red_out) {
      r.red_out[item * 2] = ld_r[0];
      r.red_out[item * 2 + 1] = ld_r[1];
    }
  }
}
}  // namespace

// grid: n_items * (p+1); block 256.  R [item][p+1][MP][MP] -> Ra [item][p+1][MPa][MPa], Rb [item][p+1][MPb][MPb]
__global__ void __launch_bounds__(256) bgc_gather_kernel(const double* R, double* Ra, double* Rb, int m, int MP, int MPa,
                                                         int MPb, int p, int split) {
  const long long item = blockIdx.x / (p + 1);
  const int k = blockIdx.x % (p + 1);
  const double* Rk = R + ((size_t)item * (p + 1) + k) * MP * MP;
  double* A = Ra + ((size_t)item * (p + 1) + k) * MPa * MPa;
  double* B = Rb + ((size_t)item * (p + 1) + k) * MPb * MPb;
  const int na = split, nb = m - split;
  for (int e = threadIdx.x; e < MPa * MPa; e += 256) {
    const int i = e / MPa, j = e % MPa;
    A[e] = (i < na && j < na) ? Rk[(size_t)i * MP + j] : ((k == 0 && i == j) ? 1.0 : 0.0);
  }
  for (int e = threadIdx.x; e < MPb * MPb; e += 256) {
    const int i = e / MPb, j = e % MPb;
    B[e] = (i < nb && j < nb) ? Rk[(size_t)(split + i) * MP + split + j] : ((k == 0 && i == j) ? 1.0 : 0.0);
  }
}

// grid: n_items * (p+1) * 2; block 256.  B [item][p+1][MP][MP] -> C [item][2][p+1][NSP][NSP], the padding written as zero.
// C_d[i][j] = sum_k sum_r B_k[r][s0+i] B_{k+d}[r][s0+j].  One v_mfma_f64_4x4x4_4b_f64 takes four rows r: its four 4x4
// blocks are four neighbouring column blocks of one 4-row strip of C (hmv_common.h): lane 16 k + 4 b + i supplies
// A[i][k] = B_k[r0+k][s0+4I+i] (the same for every b) and B[k][4b+j] = B_{k+d}[r0+k][s0+16J+4b+j], and holds
// C[4I + (l>>4)][16J + (l&15)].  Wave w takes the strips (I, J) numbered w, w + 4, ...
__global__ void __launch_bounds__(256) bgc_gram_kernel(const double* B, double* C, int m, int MP, int NSP, int p, int split) {
  long long b = blockIdx.x;
  const int dir = (int)(b % 2);
  b /= 2;
  const int d = (int)(b % (p + 1));
  const long long item = b / (p + 1);
  const int w = uni(threadIdx.x >> 6), l = threadIdx.x & 63;
  const int s0 = bgc_s0(dir, split), ns = bgc_ns(dir, split, m);
  const size_t TILE = (size_t)MP * MP;
  const double* Bi = B + item * (p + 1) * TILE;
  double* Cd = C + (((size_t)item * 2 + dir) * (p + 1) + d) * NSP * NSP;
  const int NJ = NSP / 16, NT = (NSP / 4) * NJ;
  const int kr = l >> 4;
  for (int tt = w; tt < NT; tt += 4) {
    const int I = tt / NJ, J = tt % NJ;
    const int ca = 4 * I + (l & 3), cb = 16 * J + (l & 15);
    const bool ona = ca < ns, onb = cb < ns;
    double acc = 0.0;
    for (int k = 0; k + d <= p; ++k) {
      const double* X = Bi + (size_t)k * TILE + s0 + ca;
      const double* Y = Bi + (size_t)(k + d) * TILE + s0 + cb;
      for (int r0 = 0; r0 < MP; r0 += 4) {
        const double av = ona ? X[(size_t)(r0 + kr) * MP] : 0.0;
        const double bv = onb ? Y[(size_t)(r0 + kr) * MP] : 0.0;
        acc = mfma4(av, bv, acc);
      }
    }
    Cd[(size_t)(4 * I + (l >> 4)) * NSP + 16 * J + (l & 15)] = acc;
  }
}

// grid: n_items; block 256.  See the head of the file.  red.VrA / VrB (restricted fits' residual covariances, in the MP
// layouts of the block sizes) and red.red_base may all be null: the stage on its own, which has no time-domain part.
__global__ void __launch_bounds__(256) bgc_prep_kernel(const double* ar, const double* V, BgcRed red, double* D, double* cst,
                                                       int* info_yw, int m, int MP, int MPa, int MPb, int NSP, int p,
                                                       int split) {
  __shared__ double Ls[64][65];      // the matrix being factorised, then its factor
  __shared__ double Gs[64][65];      // Sigma_sd Sigma_dd^-1 of the direction at hand
  const long long item = blockIdx.x;
  const int t = threadIdx.x;
  const size_t TILE = (size_t)MP * MP;
  const double* Vi = V + item * TILE;
  const double* ari = ar + item * TILE * p;
  int bad;
  for (int e = t; e < m * m; e += 256) Ls[e / m][e % m] = Vi[(size_t)(e / m) * MP + e % m];
  const double ld_full = chol_logdet_256(Ls, m, t, &bad);
  int first_bad = bad;                 // 1-based column of V of the first failed pivot of the spectral part (uniform)
  double ld_blk[2];
  for (int X = 0; X < 2; ++X) {        // X: the driven block; the direction it closes is src = the other block
    const int dir = 1 - X;
    const int x0 = bgc_s0(X, split), nx = bgc_ns(X, split, m);
    const int s0 = bgc_s0(dir, split), ns = bgc_ns(dir, split, m);
    __syncthreads();
    for (int e = t; e < nx * nx; e += 256) Ls[e / nx][e % nx] = Vi[(size_t)(x0 + e / nx) * MP + x0 + e % nx];
    ld_blk[X] = chol_logdet_256(Ls, nx, t, &bad);
    if (bad && !first_bad) first_bad = x0 + bad;
    // G = Sigma_sd Sigma_dd^-1: row i of Sigma_sd through L y = row, L^T g = y (one thread per row, in its row of Gs)
    if (t < ns && !bad) {
      for (int r = 0; r < nx; ++r) {
        double s = Vi[(size_t)(s0 + t) * MP + x0 + r];
        for (int q = 0; q < r; ++q) s -= Ls[r][q] * Gs[t][q];
        Gs[t][r] = s / Ls[r][r];
      }
      for (int r = nx - 1; r >= 0; --r) {
        double s = Gs[t][r];
        for (int q = r + 1; q < nx; ++q) s -= Ls[q][r] * Gs[t][q];
        Gs[t][r] = s / Ls[r][r];
      }
    } else if (t < ns) {
      for (int r = 0; r < nx; ++r) Gs[t][r] = NAN;
    }
    __syncthreads();
    // D_k, k = 1..p (lag fastest: consecutive threads read consecutive doubles of ar); D_0 = I
    double* Dd = D + ((size_t)item * 2 + dir) * (p + 1) * NSP * NSP;
    for (int e = t; e < ns * ns; e += 256) Dd[(size_t)(e / ns) * NSP + e % ns] = (e / ns == e % ns) ? 1.0 : 0.0;
    for (int e = t; e < p * ns * ns; e += 256) {
      const int k = e % p, j = (e / p) % ns, i = e / (p * ns);
      double acc = -ari[((size_t)(s0 + i) * MP + s0 + j) * p + k];
      for (int r = 0; r < nx; ++r) acc += Gs[i][r] * ari[((size_t)(x0 + r) * MP + s0 + j) * p + k];
      Dd[(size_t)(k + 1) * NSP * NSP + (size_t)i * NSP + j] = acc;
    }
    // Sigma_{s|d} = Sigma_ss - G Sigma_ds, and its log-determinant
    for (int e = t; e < ns * ns; e += 256) {
      const int i = e / ns, j = e % ns;
      double acc = Vi[(size_t)(s0 + i) * MP + s0 + j];
      for (int r = 0; r < nx; ++r) acc -= Gs[i][r] * Vi[(size_t)(x0 + r) * MP + s0 + j];
      Ls[i][j] = acc;
    }
    const double ld_c = chol_logdet_256(Ls, ns, t, &bad);
    if (bad && !first_bad) first_bad = s0 + bad;
    if (t == 0) cst[item * 2 + dir] = ld_c;
  }
  // Sigma passed ddtf_factor_kernel's Cholesky but a diagonal block or a rounded Schur complement did not: the window's
  // spectral rows are NaN, and nothing else would say so
  if (t == 0 && first_bad && info_yw[item] == 0) info_yw[item] = -first_bad;
  if (!red.VrA && !red.red_base) return;
  bgc_time_values(Ls, red, item, t, ld_full, ld_blk, m, MPa, MPb, split);
}

// grid: n_items; block 256.  bgc_prep_kernel without the spectral part: the same chol_logdet_256 on the same matrices in the
// same order (Sigma, Sigma_AA, Sigma_BB, then the restricted ones), so the time-domain values have its bits; no G, no D_k, no
// Schur complement, and one LDS matrix.  A pivot of Sigma or of a diagonal block that is not positive goes to info_yw where
// that is still 0.
__global__ void __launch_bounds__(256) bgc_time_kernel(const double* V, BgcRed red, int* info_yw, int m, int MP, int MPa,
                                                       int MPb, int split) {
  __shared__ double Ls[64][65];
  const long long item = blockIdx.x;
  const int t = threadIdx.x;
  const double* Vi = V + item * (size_t)MP * MP;
  int bad;
  for (int e = t; e < m * m; e += 256) Ls[e / m][e % m] = Vi[(size_t)(e / m) * MP + e % m];
  const double ld_full = chol_logdet_256(Ls, m, t, &bad);
  int first_bad = bad;
  double ld_blk[2];
  for (int X = 0; X < 2; ++X) {
    const int x0 = bgc_s0(X, split), nx = bgc_ns(X, split, m);
    __syncthreads();
    for (int e = t; e < nx * nx; e += 256) Ls[e / nx][e % nx] = Vi[(size_t)(x0 + e / nx) * MP + x0 + e % nx];
    ld_blk[X] = chol_logdet_256(Ls, nx, t, &bad);
    if (bad && !first_bad) first_bad = x0 + bad;
  }
  if (t == 0 && first_bad && info_yw[item] == 0) info_yw[item] = -first_bad;
  bgc_time_values(Ls, red, item, t, ld_full, ld_blk, m, MPa, MPb, split);
}

// grid: ceil(n_items * F / (WPB * G)); block 64 * WPB; dynamic LDS WPB * G * 2 * ns * RS doubles (RS = ns | 1).  A group of
// GS lanes (a power of two >= ns, at least 8; G = 64 / GS groups per wave) owns one (window, frequency) of direction `dir`:
// lane r of the group is matrix row r.  Every wave of a workgroup runs the same trip counts (they depend on ns only), so
// the barriers are workgroup barriers.  Matrix element (i, j) is the double2 at slab[i * RS + j].  The inner loops read
// four elements ahead of the four updates they feed: the updates of one row depend on nothing but the pivot row.
// info_gc [item * F + f]: -(c + 1) a pivot of W_ss that is not positive, +(c + 1) a zero pivot of At_ss; direction 0
// writes every entry, direction 1 (launched behind it) only where it fails and direction 0 did not.
__global__ void __launch_bounds__(256) bgc_freq_kernel(const double* C, const double* D, const double* cst, const double* tw,
                                                       double* out, int* info_gc, long long n_mat, int F, int m, int NSP, int p,
                                                       int split, int dir, int WPB, int GS) {
  extern __shared__ double2 bgc_lds[];
  const int w = uni(threadIdx.x >> 6), l = threadIdx.x & 63;
  const int G = 64 / GS, g = l / GS, r = l & (GS - 1);
  const int ns = bgc_ns(dir, split, m), RS = ns | 1;
  long long q = ((long long)blockIdx.x * WPB + w) * G + g;
  const bool active = q < n_mat;
  if (!active) q = n_mat - 1;
  const long long item = q / F;
  const int f = (int)(q % F);
  double2* M = bgc_lds + ((size_t)w * G + g) * ns * RS;
  const size_t NN = (size_t)NSP * NSP;
  const double* Ci = C + ((size_t)item * 2 + dir) * (p + 1) * NN;
  const double* Di = D + ((size_t)item * 2 + dir) * (p + 1) * NN;
  const double* twf = tw + (size_t)f * p * 2;
  const bool row = r < ns;
  int flag = 0;

  // W_ss(f), lower triangle
  for (int e = r; e < ns * ns; e += GS) {
    const int i = e / ns, j = e % ns;
    if (j <= i) {
      const double* cij = Ci + (size_t)i * NSP + j;
      const double* cji = Ci + (size_t)j * NSP + i;
      double re = cij[0], im = 0.0;
      for (int d0 = 1; d0 <= p; d0 += 4) {             // four lags' loads in flight (the last group clamped, not added)
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int d = d0 + u <= p ? d0 + u : p;
          a[u] = cij[d * NN];
          b[u] = cji[d * NN];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (d0 + u <= p) {
            re += (a[u] + b[u]) * twf[2 * (d0 + u - 1)];
            im += (a[u] - b[u]) * twf[2 * (d0 + u - 1) + 1];
          }
      }
      M[i * RS + j] = make_double2(re, im);
    }
  }
  double ldw = 0.0;
  double2* Mr = M + (row ? r : 0) * RS;                // this lane's row
  for (int c = 0; c < ns; ++c) {
    __syncthreads();
    const double dv = M[c * RS + c].x;
    if (!(dv > 0.0) || !(dv < INFINITY)) {
      if (!flag) flag = -(c + 1);
    }
    ldw += log(dv);
    const double lc = sqrt(dv);
    double2 a = make_double2(0.0, 0.0);
    if (r > c && row) {
      a = Mr[c];
      a.x /= lc;
      a.y /= lc;
      Mr[c] = a;
    }
    __syncthreads();
    if (r > c && row) {                                // M[r][j] -= a * conj(M[j][c]), j = c+1 .. r
      int j = c + 1;
      for (; j + 3 <= r; j += 4) {
        const double2 b0 = M[j * RS + c], b1 = M[(j + 1) * RS + c], b2 = M[(j + 2) * RS + c], b3 = M[(j + 3) * RS + c];
        double2 v0 = Mr[j], v1 = Mr[j + 1], v2 = Mr[j + 2], v3 = Mr[j + 3];
        v0.x -= a.x * b0.x + a.y * b0.y;  v0.y -= a.y * b0.x - a.x * b0.y;
        v1.x -= a.x * b1.x + a.y * b1.y;  v1.y -= a.y * b1.x - a.x * b1.y;
        v2.x -= a.x * b2.x + a.y * b2.y;  v2.y -= a.y * b2.x - a.x * b2.y;
        v3.x -= a.x * b3.x + a.y * b3.y;  v3.y -= a.y * b3.x - a.x * b3.y;
        Mr[j] = v0;  Mr[j + 1] = v1;  Mr[j + 2] = v2;  Mr[j + 3] = v3;
      }
      for (; j <= r; ++j) {
        const double2 bj = M[j * RS + c];
        double2 v = Mr[j];
        v.x -= a.x * bj.x + a.y * bj.y;
        v.y -= a.y * bj.x - a.x * bj.y;
        Mr[j] = v;
      }
    }
  }
  __syncthreads();

  // At_ss(f), full
  for (int e = r; e < ns * ns; e += GS) {
    const int i = e / ns, j = e % ns;
    const double* dij = Di + (size_t)i * NSP + j;
    double re = (i == j) ? 1.0 : 0.0, im = 0.0;
    for (int k0 = 1; k0 <= p; k0 += 8) {               // eight lags' loads in flight
      double a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = dij[(k0 + u <= p ? k0 + u : p) * NN];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k0 + u <= p) {
          re += a[u] * twf[2 * (k0 + u - 1)];
          im += a[u] * twf[2 * (k0 + u - 1) + 1];
        }
    }
    M[i * RS + j] = make_double2(re, im);
  }
  double lda = 0.0;
  for (int c = 0; c < ns; ++c) {
    __syncthreads();
    // pivot: the largest |re| + |im| of column c at or below the diagonal, the smallest row among (near-)equals: the max
    // over the group of a 64-bit key, the magnitude's bits with the low six replaced by 63 - row
    unsigned long long key = 0;
    if (r >= c && row) {
      const double2 v = Mr[c];
      const double av = fabs(v.x) + fabs(v.y);
      key = ((unsigned long long)__double_as_longlong(av) & ~63ull) | (unsigned long long)(63 - r);
    }
    for (int mm = 1; mm < GS; mm <<= 1) {
      const unsigned long long o = shfl_u64(key, l ^ mm);
      key = o > key ? o : key;
    }
    const int pr = 63 - (int)(key & 63ull);            // c <= pr < ns: row c itself is always a candidate
    const double2 pv = M[pr * RS + c];
    const double pa2 = pv.x * pv.x + pv.y * pv.y;
    if (!(pa2 > 0.0) || !(pa2 < INFINITY)) {
      if (!flag) flag = c + 1;
    }
    lda += 0.5 * log(pa2);
    double2 mine = make_double2(0.0, 0.0);
    if (r > c && row) mine = M[(r == pr ? c : r) * RS + c];         // row r's column-c element once rows c and pr are swapped
    __syncthreads();
    if (pr != c && r >= c && row) {                                  // swap rows c and pr, columns >= c (lane = column)
      const double2 u = M[c * RS + r], v = M[pr * RS + r];
      M[c * RS + r] = v;
      M[pr * RS + r] = u;
    }
    __syncthreads();
    if (r > c && row) {                                              // M[r][j] -= (mine / pv) * M[c][j], j = c+1 .. ns-1
      double2 lm;
      lm.x = (mine.x * pv.x + mine.y * pv.y) / pa2;
      lm.y = (mine.y * pv.x - mine.x * pv.y) / pa2;
      const double2* Mc = M + c * RS;
      int j = c + 1;
      for (; j + 3 < ns; j += 4) {
        const double2 u0 = Mc[j], u1 = Mc[j + 1], u2 = Mc[j + 2], u3 = Mc[j + 3];
        double2 v0 = Mr[j], v1 = Mr[j + 1], v2 = Mr[j + 2], v3 = Mr[j + 3];
        v0.x -= lm.x * u0.x - lm.y * u0.y;  v0.y -= lm.x * u0.y + lm.y * u0.x;
        v1.x -= lm.x * u1.x - lm.y * u1.y;  v1.y -= lm.x * u1.y + lm.y * u1.x;
        v2.x -= lm.x * u2.x - lm.y * u2.y;  v2.y -= lm.x * u2.y + lm.y * u2.x;
        v3.x -= lm.x * u3.x - lm.y * u3.y;  v3.y -= lm.x * u3.y + lm.y * u3.x;
        Mr[j] = v0;  Mr[j + 1] = v1;  Mr[j + 2] = v2;  Mr[j + 3] = v3;
      }
      for (; j < ns; ++j) {
        const double2 u = Mc[j];
        double2 v = Mr[j];
        v.x -= lm.x * u.x - lm.y * u.y;
        v.y -= lm.x * u.y + lm.y * u.x;
        Mr[j] = v;
      }
    }
  }
  if (active && r == 0) {
    out[((size_t)item * 2 + dir) * F + f] = cst[item * 2 + dir] + ldw - 2.0 * lda;
    int* ig = info_gc + (size_t)item * F + f;
    if (dir == 0)
      *ig = flag;
    else if (flag && *ig == 0)
      *ig = flag;
  }
}

int launch_bgc_gather(const double* R, double* Ra, double* Rb, long long n_items, int m, int m_pad, int p, int split,
                      hipStream_t st) {
  if (n_items == 0) return 0;
  const BgcPads pd = bgc_pads(m, split);
  hipLaunchKernelGGL(bgc_gather_kernel, dim3((unsigned)(n_items * (p + 1))), dim3(256), 0, st, R, Ra, Rb, m, m_pad, pd.mpa,
                     pd.mpb, p, split);
  return (int)hipGetLastError();
}

int launch_bgc(const BgcArgs& a, int m_pad, hipStream_t st) {
  const bool timed = a.red.VrA || a.red.red_base;
  const int want = a.want ? a.want : (timed ? 3 : 1);
  if (a.n_items == 0 || ((want & 1) && a.F == 0)) return 0;
  if (a.split < 1 || a.split >= a.m || a.p < 1 || a.p > HMV_MAX_ORDER || ((want & 2) && !timed)) return -3;
  const BgcPads pd = bgc_pads(a.m, a.split);
  const int nsp = pd.nsp;
  if (!(want & 1)) {
    hipLaunchKernelGGL(bgc_time_kernel, dim3((unsigned)a.n_items), dim3(256), 0, st, a.V, a.red, a.info_yw, a.m, m_pad, pd.mpa,
                       pd.mpb, a.split);
    return (int)hipGetLastError();
  }
  int rc = launch_ddtf_factor(a.ar, a.V, a.info_yw, a.B, a.n_items, a.m, m_pad, a.p, st);
  if (rc) return rc;
  hipLaunchKernelGGL(bgc_gram_kernel, dim3((unsigned)(a.n_items * (a.p + 1) * 2)), dim3(256), 0, st, a.B, a.C, a.m, m_pad, nsp,
                     a.p, a.split);
  hipLaunchKernelGGL(bgc_prep_kernel, dim3((unsigned)a.n_items), dim3(256), 0, st, a.ar, a.V, (want & 2) ? a.red : BgcRed{},
                     a.D, a.cst, a.info_yw, a.m, m_pad, pd.mpa, pd.mpb, nsp, a.p, a.split);
  const long long n_mat = a.n_items * a.F;
  for (int dir = 0; dir < 2; ++dir) {
    // a group of GS lanes per matrix (lane = row), and as many waves per workgroup (at most four) as fit 64 KiB of LDS with
    // their slabs: the larger block gets fewer waves per workgroup, the smaller one several matrices per wave -- each
    // direction pays for its own n_src only
    const int ns = dir ? a.m - a.split : a.split;
    int gs = 8;                             // (above 16 rows LDS, not lanes, bounds the matrices in flight: one per wave)
    while (gs < ns) gs *= 2;
    if (ns > 16) gs = 64;
    const int g = 64 / gs;
    const size_t slab = (size_t)g * ns * (ns | 1) * sizeof(double2);      // of one wave
    int wpb = (int)(65536 / slab);
    wpb = wpb > 4 ? 4 : (wpb < 1 ? 1 : wpb);
    const long long per_wg = (long long)wpb * g;
    hipLaunchKernelGGL(bgc_freq_kernel, dim3((unsigned)((n_mat + per_wg - 1) / per_wg)), dim3(64 * wpb), wpb * slab, st, a.C,
                       a.D, a.cst, a.tw, a.out, a.info_gc, n_mat, a.F, a.m, nsp, a.p, a.split, dir, wpb, gs);
  }
  return (int)hipGetLastError();
}

}  // namespace hmv
