// K2, pivoted fallback -- dense LU with partial pivoting of the windows that the two Yule-Walker solvers refuse.
//
// The recursion (yw_lwr.hip) and the unpivoted block LDL^T (yw_solve.hip) report "singular" as soon as rounding makes a
// pivot non-positive; the reference (`np.linalg.solve`, i.e. dgesv) returns numbers for every window whose normal
// equations are not EXACTLY singular.  This kernel does what dgesv does, for the windows selected by `info != 0` (or for
// every window: HMV_TUNE_YW_FORM = 5):
//   * the dense augmented system [G | B], N x (N + MP), N = MP p, is written into the window's own K2 scratch (p (p+1)
//     tiles of the 2 T(p+1) + 2p it has; whatever the LDL^T left there is dead; the guard word's tile is not touched
//     except for the word): G[a][b] = R_{a-b} (a >= b), R_{b-a}^T (a < b), B[a] = R_{a+1};
//   * right-looking LU, 4 columns at a time (the k of v_mfma_f64_4x4x4): the N x 4 panel is factored in LDS with
//     LAPACK's pivot rule (largest |a| on or below the diagonal, the first on ties), the interchanges are applied to the
//     whole augmented row, the 4 x (rest) block row of U is a unit-lower 4 x 4 solve per column, and the rank-4 update
//     of the trailing matrix AND of the B columns is one MFMA per 4 x 16 patch (so the forward substitution of the
//     right-hand sides happens on the way);
//   * back substitution 4 rows at a time from the bottom, again a 4 x 4 solve and a rank-4 MFMA update of the rows above;
//   * ar[i][j][k] = X[k MP + j][i];  V = R_0 - X^T B as one more MFMA GEMM, rows ascending;  info = 0, or c + 1 for an
//     exactly zero pivot column c (dgesv's info > 0; no solution is formed then: ar and V are NaN).
// Every sum has a fixed order and nothing depends on the other windows of the batch.  There is no absolute constant:
// samples * 2^k give G and B * 4^k, the same pivot choices, the same multipliers and X bit for bit, and V * 4^k.  The
// padded channels carry K1's identity block: their columns hold a single 1 on the diagonal, their rows are zero in every
// real column, so they never compete for the pivot of a real column, and they keep N a multiple of 16.
// One 256-thread workgroup per window; a window that is not selected costs one load.  This is the slow path of a slow
// path (every panel step streams the trailing matrix through one compute unit): it is sized for correctness.
#include "yw_common.h"

namespace hmv {

template <int NT>
__global__ void __launch_bounds__(256) yw_lu_kernel(YwArgs a, int all) {
  constexpr int MP = 16 * NT, TILE = MP * MP;
  __shared__ __attribute__((aligned(16))) double P[MP * 32 * 4];      // the panel: [row][4], rows 0 .. N-1 (N <= 32 MP)
  __shared__ double s_val[4];
  __shared__ int s_idx[4], s_piv[4], s_info;
  const long long item = blockIdx.x;
  if (!all && a.info[item] == 0) return;
  const int p = a.p, N = MP * p, W = N + MP;
  const int tid = threadIdx.x, l = tid & 63, wv = uni(tid >> 6);
  const int kk = l >> 4, cc = l & 15;
  const double* R = a.R + (size_t)item * (p + 1) * TILE;
  double* A = a.ws + (size_t)item * yw_ws_tiles_d(p) * TILE;            // [N][W], row-major

  // ---- [G | B] from the lag blocks
  for (int r = 0; r < N; ++r) {
    const int ab = r / MP, i = r - ab * MP;
    for (int c = tid; c < W; c += 256) {
      double v;
      if (c < N) {
        const int bb = c / MP, j = c - bb * MP;
        v = (ab >= bb) ? R[(size_t)(ab - bb) * TILE + i * MP + j] : R[(size_t)(bb - ab) * TILE + j * MP + i];
      } else {
        v = R[(size_t)(ab + 1) * TILE + i * MP + (c - N)];
      }
      A[(size_t)r * W + c] = v;
    }
  }
  if (tid == 0) s_info = 0;

  // ---- LU, panel by panel
  for (int k0 = 0; k0 < N; k0 += 4) {
    __syncthreads();                                   // the matrix (built, or updated by the previous step) is in memory
    for (int r = k0 + tid; r < N; r += 256) {
      const f64x2* src = reinterpret_cast<const f64x2*>(A + (size_t)r * W + k0);
      const f64x2 lo = src[0], hi = src[1];
      P[4 * r] = lo.x; P[4 * r + 1] = lo.y; P[4 * r + 2] = hi.x; P[4 * r + 3] = hi.y;
    }
    __syncthreads();
    for (int jj = 0; jj < 4; ++jj) {
      const int k = k0 + jj;
      // pivot: largest |a| in rows k .. N-1 of column k, the first on ties (idamax)
      double best = -1.0;
      int bi = 0x7fffffff;
      for (int r = k + tid; r < N; r += 256) {
        const double v = fabs(P[4 * r + jj]);
        if (v > best) { best = v; bi = r; }
      }
#pragma unroll
      for (int msk = 1; msk < 64; msk <<= 1) {
        const double ob = shfl_f64(best, l ^ msk);
        const int oi = __builtin_amdgcn_ds_bpermute((l ^ msk) << 2, bi);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (l == 0) { s_val[wv] = best; s_idx[wv] = bi; }
      __syncthreads();
      best = s_val[0]; bi = s_idx[0];
#pragma unroll
      for (int w2 = 1; w2 < 4; ++w2) {
        const double ob = s_val[w2];
        const int oi = s_idx[w2];
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      }
      if (bi >= N) bi = k;                             // (a column of NaNs: no interchange, the NaNs go their way)
      double prow[4], krow[4];
#pragma unroll
      for (int j2 = 0; j2 < 4; ++j2) { prow[j2] = P[4 * bi + j2]; krow[j2] = P[4 * k + j2]; }
      const double pv = prow[jj];
      __syncthreads();                                 // everybody has read the two rows and the candidates
      // the interchange (row k from the pivot row, by the first four threads; row bi from row k, by its owner below), the
      // multipliers and the update of the panel's later columns; an exactly zero column is left as it is (dgetf2)
      if (tid < 4) P[4 * k + tid] = prow[tid];
      if (tid == 0) {
        s_piv[jj] = bi;
        if (pv == 0.0 && s_info == 0) s_info = k + 1;
      }
      for (int r = k + 1 + tid; r < N; r += 256) {
        double x[4];
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) x[j2] = (r == bi) ? krow[j2] : P[4 * r + j2];
        if (pv != 0.0) {
          const double lm = x[jj] / pv;
#pragma unroll
          for (int j2 = 0; j2 < 4; ++j2) {
            if (j2 == jj) x[j2] = lm;
            else if (j2 > jj) x[j2] = __builtin_fma(-lm, prow[j2], x[j2]);
          }
        }
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) P[4 * r + j2] = x[j2];
      }
      __syncthreads();
    }
    // the factored panel back to memory; the four interchanges on every other column of the augmented rows (a thread
    // keeps its columns through the four of them, in order)
    for (int r = k0 + tid; r < N; r += 256) {
      f64x2* dst = reinterpret_cast<f64x2*>(A + (size_t)r * W + k0);
      f64x2 lo, hi;
      lo.x = P[4 * r]; lo.y = P[4 * r + 1]; hi.x = P[4 * r + 2]; hi.y = P[4 * r + 3];
      dst[0] = lo; dst[1] = hi;
    }
    for (int jj = 0; jj < 4; ++jj) {
      const int k = k0 + jj, bi = s_piv[jj];
      if (bi == k) continue;
      double* rk = A + (size_t)k * W;
      double* rb = A + (size_t)bi * W;
      for (int c = tid; c < W; c += 256) {
        if (c >= k0 && c < k0 + 4) continue;
        const double t = rk[c];
        rk[c] = rb[c];
        rb[c] = t;
      }
    }
    __syncthreads();
    // block row of U and the rank-4 update, 16 columns per wave and turn.  Lane l = 16 kk + cc holds, of column `col`,
    // U[k0 + kk][col] (the B operand of the MFMA) and element (r0 + kk, col) of every 4-row block of the trailing matrix.
    {
      const double l10 = P[4 * (k0 + 1)], l20 = P[4 * (k0 + 2)], l21 = P[4 * (k0 + 2) + 1];
      const double l30 = P[4 * (k0 + 3)], l31 = P[4 * (k0 + 3) + 1], l32 = P[4 * (k0 + 3) + 2];
      for (int q = (k0 + 4) / 16 + wv; q < W / 16; q += 4) {
        const int col = 16 * q + cc;
        const bool valid = col >= k0 + 4;
        double* colp = A + (size_t)k0 * W + col;
        double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
        if (valid) {
          u0 = colp[0];
          u1 = __builtin_fma(-l10, u0, colp[W]);
          u2 = __builtin_fma(-l21, u1, __builtin_fma(-l20, u0, colp[2 * (size_t)W]));
          u3 = __builtin_fma(-l32, u2, __builtin_fma(-l31, u1, __builtin_fma(-l30, u0, colp[3 * (size_t)W])));
        }
        const double b = kk == 0 ? u0 : (kk == 1 ? u1 : (kk == 2 ? u2 : u3));
        if (valid) colp[(size_t)kk * W] = b;
        double* cp = A + (size_t)(k0 + 4 + kk) * W + col;
        const double* lp = P + 4 * (k0 + 4 + (l & 3)) + kk;
        int r0 = k0 + 4;
        for (; r0 + 16 <= N; r0 += 16) {
          double c4[4], a4[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            c4[t] = valid ? cp[(size_t)(4 * t) * W] : 0.0;
            a4[t] = -lp[16 * t];
          }
#pragma unroll
          for (int t = 0; t < 4; ++t) c4[t] = mfma4(a4[t], b, c4[t]);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (valid) cp[(size_t)(4 * t) * W] = c4[t];
          cp += (size_t)16 * W;
          lp += 64;
        }
        for (; r0 < N; r0 += 4) {
          double c1 = valid ? cp[0] : 0.0;
          c1 = mfma4(-lp[0], b, c1);
          if (valid) cp[0] = c1;
          cp += (size_t)4 * W;
          lp += 16;
        }
      }
    }
  }
  __syncthreads();
  double* ar = a.ar + (size_t)item * TILE * p;
  double* Vo = a.V + (size_t)item * TILE;
  if (s_info != 0) {                                   // exactly singular: dgesv forms no solution
    const double qnan = __builtin_nan("");
    for (int idx = tid; idx < TILE * p; idx += 256) ar[idx] = qnan;
    for (int idx = tid; idx < TILE; idx += 256) Vo[idx] = qnan;
    if (tid == 0) {
      a.info[item] = s_info;
      *yw_guard_ptr(a.ws, item, p, TILE) = 2;
    }
    return;
  }

  // ---- back substitution: the B columns hold L^-1 P B; X overwrites them, 4 rows at a time from the bottom
  for (int k0 = N - 4; k0 >= 0; k0 -= 4) {
    __syncthreads();                                   // the updates of the previous step are in memory
    const double* ur = A + (size_t)k0 * W + k0;
    const double u00 = ur[0], u01 = ur[1], u02 = ur[2], u03 = ur[3];
    const double u11 = ur[W + 1], u12 = ur[W + 2], u13 = ur[W + 3];
    const double u22 = ur[2 * (size_t)W + 2], u23 = ur[2 * (size_t)W + 3], u33 = ur[3 * (size_t)W + 3];
    double xb[NT];
#pragma unroll
    for (int J = 0; J < NT; ++J) {
      const double* bp = A + (size_t)k0 * W + N + 16 * J + cc;
      const double x3 = bp[3 * (size_t)W] / u33;
      const double x2 = __builtin_fma(-u23, x3, bp[2 * (size_t)W]) / u22;
      const double x1 = __builtin_fma(-u13, x3, __builtin_fma(-u12, x2, bp[W])) / u11;
      const double x0 = __builtin_fma(-u03, x3, __builtin_fma(-u02, x2, __builtin_fma(-u01, x1, bp[0]))) / u00;
      xb[J] = kk == 0 ? x0 : (kk == 1 ? x1 : (kk == 2 ? x2 : x3));
    }
    __syncthreads();                                   // every wave has read the four rows before they become X
    if (wv == 0) {
#pragma unroll
      for (int J = 0; J < NT; ++J) A[(size_t)(k0 + kk) * W + N + 16 * J + cc] = xb[J];
    }
    for (int r0 = 4 * wv; r0 < k0; r0 += 16) {
      const double au = -A[(size_t)(r0 + (l & 3)) * W + k0 + kk];
#pragma unroll
      for (int J = 0; J < NT; ++J) {
        double* cp = A + (size_t)(r0 + kk) * W + N + 16 * J + cc;
        *cp = mfma4(au, xb[J], *cp);
      }
    }
  }
  __syncthreads();

  // ---- V = R_0 - X^T B (B from the lag blocks: the copy in the scratch is gone), rows of the system ascending; wave w
  // owns the row blocks w NT .. w NT + NT - 1 of V
  {
    double acc[NT][NT];
#pragma unroll
    for (int ii = 0; ii < NT; ++ii)
#pragma unroll
      for (int J = 0; J < NT; ++J) acc[ii][J] = 0.0;
    for (int r0 = 0; r0 < N; r0 += 4) {
      const int r = r0 + kk, rb = r / MP, rj = r - rb * MP;
      const double* xr = A + (size_t)r * W + N + 4 * wv * NT + (l & 3);
      const double* br = R + (size_t)(rb + 1) * TILE + rj * MP + cc;
      double av[NT], bv[NT];
#pragma unroll
      for (int ii = 0; ii < NT; ++ii) av[ii] = xr[4 * ii];
#pragma unroll
      for (int J = 0; J < NT; ++J) bv[J] = br[16 * J];
#pragma unroll
      for (int ii = 0; ii < NT; ++ii)
#pragma unroll
        for (int J = 0; J < NT; ++J) acc[ii][J] = mfma4(av[ii], bv[J], acc[ii][J]);
    }
#pragma unroll
    for (int ii = 0; ii < NT; ++ii)
#pragma unroll
      for (int J = 0; J < NT; ++J) {
        const int e = (4 * (wv * NT + ii) + kk) * MP + 16 * J + cc;
        Vo[e] = R[e] - acc[ii][J];
      }
  }
  // ---- ar[row][col][k] = X[k MP + col][row]  (lag fastest: the reference's (m, m, p) layout)
  for (int idx = tid; idx < TILE * p; idx += 256) {
    const int e = idx / p, k = idx - e * p;
    const int i = e / MP, j = e - i * MP;
    ar[idx] = A[(size_t)(k * MP + j) * W + N + i];
  }
  if (tid == 0) {
    a.info[item] = 0;
    *yw_guard_ptr(a.ws, item, p, TILE) = 2;
  }
}

// all != 0: every window; otherwise the windows whose info is not zero
int launch_yw_lu(const YwArgs& a, int m_pad, int all, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL((yw_lu_kernel<nt>), grid, block, 0, st, a, all); })) return -1;
  return (int)hipGetLastError();
}

// ---- the route word of every window (the last int of its scratch): 0 recursion, 1 LDL^T, 2 LU
__global__ void yw_route_set_kernel(double* ws, long long n_items, long long ws_item, int value) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item < n_items) reinterpret_cast<int*>(ws + (size_t)(item + 1) * ws_item)[-1] = value;
}
__global__ void yw_route_get_kernel(const double* ws, long long n_items, long long ws_item, int* route) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item < n_items) route[item] = reinterpret_cast<const int*>(ws + (size_t)(item + 1) * ws_item)[-1];
}
int launch_yw_route_set(double* ws, long long n_items, int m_pad, int p, int value, hipStream_t st) {
  if (n_items == 0) return 0;
  const long long ws_item = yw_ws_tiles_d(p) * (long long)m_pad * m_pad;
  hipLaunchKernelGGL(yw_route_set_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, ws, n_items, ws_item,
                     value);
  return (int)hipGetLastError();
}
int launch_yw_routes(const double* ws, long long n_items, int m_pad, int p, int* route, hipStream_t st) {
  if (n_items == 0) return 0;
  const long long ws_item = yw_ws_tiles_d(p) * (long long)m_pad * m_pad;
  hipLaunchKernelGGL(yw_route_get_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, st, ws, n_items, ws_item,
                     route);
  return (int)hipGetLastError();
}

}  // namespace hmv
