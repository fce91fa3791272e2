// The phase-lag family of analytic signals per window: PLI (Stam 2007), weighted PLI and debiased squared weighted PLI
// (Vinck 2011).  With x[t] = Im(z_i[t] conj z_j[t]) = rn(rn(im_i re_j) - rn(re_i im_j)) -- two rounded products and one
// subtraction, never an FMA, so that proportional channels give x = 0 exactly and NumPy computes the same bits --
//     P - N = sum sign(x)    S = sum x    A = sum |x|    Q = sum x^2    (each over t = 0 .. n - 1 ascending, Q by FMA)
//     pli = |P - N| / n      wpli = |S| / A      dwpli = (S^2 - Q) / (A^2 - Q).
// sign and |.| are per sample and per pair: no matrix product gives these sums, so this is f64 VALU work, not MFMA.
//
// One workgroup = one item, the window streamed through LDS in chunks of 64 samples as a re and an im plane
// (k1::stage_chunk2, torch's interleaved complex128 read as it lies, no normalisation).  A thread owns 2 x 2 blocks of
// pairs -- rows (r0, r1) against columns (c0, c1), eight LDS reads for four pair-samples -- and runs every sample of the
// window for them in turn, so a pair's sums are sequential in t whatever thread has them: the bits of a cell depend on the
// n samples of its two channels only.
//
// The work is dealt over the needed pairs in units of 32 lanes (half a wave, the group within which ds_read_b64 lanes can
// conflict).  The pairs are cut into the 16 x 16 channel tiles on or above the diagonal; a tile above the diagonal is two
// units (8 rows x 16 columns = 4 x 8 blocks each), a tile on it one unit: the 28 blocks above the diagonal of its 8 x 8
// blocks and four lanes that take the eight pairs (2k, 2k + 1) the diagonal blocks hold, two each.  At 64 channels that is
// 12 + 4 = 16 units = 512 blocks for 2016 pairs: two blocks in every thread and the same loop in every wave.  With
// `split` only the tiles that hold a cross cell are dealt (split 32 of 64: 8 units, one block per thread).  Within a unit
// a read touches at most 8 even (or 8 odd) channels of one tile plus the diagonal lanes' four, which the row stride of 70
// doubles (12 banks a channel) spreads over distinct banks, or it is a broadcast.
//
// The epilogue passes the results through LDS -- the planes' own memory: wpli above the diagonal of one MP x (MP + 1) image
// and dwpli below it, pli in a second image -- and every output element (r, c) is formed from cell (min, max).
#include "hmv_common.h"
#include "hmv_kernels.h"
#include "lagcov_core.h"
#include <cmath>

namespace hmv {

namespace {

struct LagAcc {
  double s, a, q;
  int d;                                 // P - N
};

// one sample of one pair.  contract(off): the two products of x are rounded before the subtraction
__device__ __forceinline__ void lag_step(LagAcc& c, double ri, double ii, double rj, double ij) {
#pragma clang fp contract(off)
  const double p0 = ii * rj, p1 = ri * ij;
  const double x = p0 - p1;
  c.s += x;
  c.a += fabs(x);
  c.q = __builtin_fma(x, x, c.q);
  c.d += (x > 0.0) - (x < 0.0);
}

// the block of unit `u` (in the order of the needed tiles) that lane `lam` of the unit owns: channels r0, r1, c0, c1 and
// which of its pairs (r0,c0) (r0,c1) (r1,c0) (r1,c1) are its to deliver (bits 0..3).  false: there is no unit u.
template <int NT>
__device__ __forceinline__ bool lag_block(int u, int lam, int m, int split, int& r0, int& r1, int& c0, int& c1, unsigned& own) {
  int I = -1, J = -1, half = 0, cnt = 0;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = i; j < NT; ++j) {
      const bool need = 16 * j < m && (split == 0 || (16 * i < split && 16 * j + 15 >= split));
      const int w = need ? (i == j ? 1 : 2) : 0;
      if (u >= cnt && u < cnt + w) { I = i; J = j; half = u - cnt; }
      cnt += w;
    }
  r0 = r1 = c0 = c1 = 0;
  own = 0;
  if (I < 0) return false;
  if (I == J) {
    if (lam < 28) {                      // block (bi, bj), bi < bj < 8
      int bi = 0, rem = lam;
      while (rem >= 7 - bi) { rem -= 7 - bi; ++bi; }
      r0 = 16 * I + 2 * bi; r1 = r0 + 1;
      c0 = 16 * I + 2 * (bi + 1 + rem); c1 = c0 + 1;
      own = 15u;
    } else {                             // the pairs of two diagonal blocks
      r0 = 16 * I + 4 * (lam - 28); c0 = r0 + 1; r1 = r0 + 2; c1 = r0 + 3;
      own = 9u;
    }
  } else {
    r0 = 16 * I + 2 * (4 * half + (lam >> 3)); r1 = r0 + 1;
    c0 = 16 * J + 2 * (lam & 7); c1 = c0 + 1;
    own = 15u;
  }
  const int rr[4] = {r0, r0, r1, r1}, cc[4] = {c0, c1, c0, c1};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (!(cc[k] < m && (split == 0 || (rr[k] < split && cc[k] >= split)))) own &= ~(1u << k);
  return true;
}

}  // namespace

template <int NT>
__global__ void __launch_bounds__(256, 2) phase_lag_kernel(PhaseLagArgs a) {
#pragma clang fp contract(off)
  constexpr int MP = 16 * NT, PLANE = MP * k1::S2, CS = MP + 1, R = (NT * NT + 7) / 8;
  static_assert(2 * MP * CS <= 2 * PLANE, "the epilogue's two images fit the two staging planes");
  __shared__ double xs[2 * PLANE];
  const long long item = blockIdx.x;
  const int n = a.n, m = a.m, split = a.split;
  const long long rec = a.item_rec[item], start = a.item_start[item];
  // samples with a value; a window the caller let reach outside its recording reads zeros there, never memory
  const bool inside = rec >= 0 && rec < a.n_rec && start >= 0 && start < a.T;
  const long long vlen = inside ? min((long long)n, a.T - start) : 0;
  const double2* z = inside ? a.z + rec * a.rec_stride + start : a.z;

  int ro0[R], ro1[R], co0[R], co1[R];    // the blocks of this thread, as offsets into a plane
  int ch[R][4];
  unsigned own[R];
  bool live[R];                          // wave-uniform: the wave has a unit in round r
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int r0, r1, c0, c1;
    lag_block<NT>(8 * r + (threadIdx.x >> 5), threadIdx.x & 31, m, split, r0, r1, c0, c1, own[r]);
    ro0[r] = r0 * k1::S2; ro1[r] = r1 * k1::S2; co0[r] = c0 * k1::S2; co1[r] = c1 * k1::S2;
    ch[r][0] = r0; ch[r][1] = r1; ch[r][2] = c0; ch[r][3] = c1;
    live[r] = __ballot(own[r] != 0) != 0;
  }
  LagAcc acc[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[r][k] = LagAcc{0.0, 0.0, 0.0, 0};

  double* xre = xs;
  double* xim = xs + PLANE;
  int nf = 0;                            // this thread staged a non-finite value
  for (int t0 = 0; t0 < n; t0 += k1::TC) {
    k1::stage_chunk2<NT>(xre, xim, t0, [&](int c, int t) __attribute__((always_inline)) {
      double2 v = make_double2(0.0, 0.0);
      if (c < m && t < vlen) {
        v = z[(size_t)c * a.ld + t];
        nf |= !(__builtin_isfinite(v.x) && __builtin_isfinite(v.y));
      }
      return v;
    });
    const int steps = min(k1::TC, n - t0);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live[r]) continue;
      const double* pr0 = xre + ro0[r];
      const double* pr1 = xre + ro1[r];
      const double* pc0 = xre + co0[r];
      const double* pc1 = xre + co1[r];
#pragma unroll 2
      for (int t = 0; t < steps; ++t) {
        const double r0r = pr0[t], r0i = pr0[PLANE + t], r1r = pr1[t], r1i = pr1[PLANE + t];
        const double c0r = pc0[t], c0i = pc0[PLANE + t], c1r = pc1[t], c1i = pc1[PLANE + t];
        lag_step(acc[r][0], r0r, r0i, c0r, c0i);
        lag_step(acc[r][1], r0r, r0i, c1r, c1i);
        lag_step(acc[r][2], r1r, r1i, c0r, c0i);
        lag_step(acc[r][3], r1r, r1i, c1r, c1i);
      }
    }
  }

  // the results of the owned pairs through LDS: wpli at [i][j], dwpli at [j][i] of one image, pli at [i][j] of the other
  __syncthreads();
  const double nan = __builtin_nan("");
  const double nn = (double)n;
  double* cw = xs;
  double* cp = xs + MP * CS;
  int flat = 0;                          // an owned pair with A == 0
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (own[r] & (1u << k)) {
        const int i = ch[r][k >> 1], j = ch[r][2 + (k & 1)];
        const LagAcc c = acc[r][k];
        const double den = c.a * c.a - c.q;
        cp[i * CS + j] = fabs((double)c.d) / nn;
        cw[i * CS + j] = c.a == 0.0 ? nan : fabs(c.s) / c.a;
        cw[j * CS + i] = den > 0.0 ? (c.s * c.s - c.q) / den : nan;
        flat |= c.a == 0.0;
      }
  const bool bad = __syncthreads_or(nf) != 0;
  const bool dead = __syncthreads_or(flat) != 0;
  if (threadIdx.x == 0) a.info[item] = bad ? 1 : dead ? 2 : 0;

  const size_t mm = (size_t)m * m;
  double* op = a.pli ? a.pli + (size_t)item * mm : nullptr;
  double* ow = a.wpli ? a.wpli + (size_t)item * mm : nullptr;
  double* od = a.dwpli ? a.dwpli + (size_t)item * mm : nullptr;
  for (int e = threadIdx.x; e < m * m; e += 256) {
    const int r = e / m, c = e - r * m;
    const int i = min(r, c), j = max(r, c);
    double vp = 0.0, vw = 0.0, vd = 0.0;
    if (i != j) {
      if (split == 0 || (i < split && j >= split)) {
        vp = cp[i * CS + j]; vw = cw[i * CS + j]; vd = cw[j * CS + i];
      } else {
        vp = vw = vd = nan;              // a pair that was not asked for
      }
    }
    if (bad) vp = vw = vd = nan;
    if (op) op[e] = vp;
    if (ow) ow[e] = vw;
    if (od) od[e] = vd;
  }
}

int launch_phase_lag(const PhaseLagArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(phase_lag_kernel<decltype(nt)::value>, grid, block, 0, st, a); }))
    return -1;
  return (int)hipGetLastError();
}

}  // namespace hmv
