// K1 -- lagged autocovariance of every window:  R_l = (1/n) X[:, :n-l] X[:, l:]^T,  l = 0..p.
//
// Replaces `count_corr` (/root/reference/src/mtmvar.py:35-87): p+1 `np.dot` calls per window, biased
// 1/n scaling for every lag (mtmvar.py:57,72), data NOT demeaned (quirk Q1).  The block-Toeplitz
// r_left / r_right of the reference are never materialised -- K2 consumes the p+1 blocks directly.
//
// The direct form below is lagcov_core.h's (mapping, chunks, k-steps): the window itself is the source, and in block mode
// the hop block with everything behind it up to the end of the recording.
#include "hmv_common.h"
#include "hmv_kernels.h"
#include "lagcov_core.h"
#include <cstdlib>

namespace hmv {

// grid (items, ceil((p+1) / LG)).  The staged chunk (the costly part: global loads, two barriers, LDS stores) is shared by
// the LG lags, and the window is fetched ceil((p+1)/LG) times instead of p+1 times (round 1, LG = 1: 21x over-fetch, 0.53
// of the f64 peak).
template <int NT, int LG>
__global__ void __launch_bounds__(256, 2) lagcov_kernel(LagcovArgs a) {
  constexpr int MP = 16 * NT;
  __shared__ double xs[MP * k1::S];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int lag0 = blockIdx.y * LG;
  const int nl = min(LG, a.p + 1 - lag0);          // lags of this workgroup (the last group may be short)
  const int n = a.n, m = a.m;            // n: samples summed over (window length, or hop in block mode)
  const bool blk = a.blocks != 0;
  const long long start = blk ? a.blk_first + item * (long long)n : a.item_start[item];
  const double* x = a.x + (blk ? 0 : a.item_rec[item] * a.rec_stride) + start;
  // samples with a value: the window itself, or in block mode everything up to the end of the recording (the lagged
  // partner x[t + l] of the last samples of a block lies in the next block)
  const long long vlen = blk ? a.blk_T - start : (long long)n;
  const bool mask_a = blk && (n & 3) != 0;  // block mode: the A operand must end at n even if real samples follow

  double acc[LG][NT][NT];
  k1::zero_acc(acc);
  for (int t0 = 0; t0 < n; t0 += k1::TC) {
    k1::stage_chunk<NT>(xs, t0, [&](int ch, int t) __attribute__((always_inline)) {
      return (ch < m && t < vlen) ? x[(size_t)ch * a.ld + t] : 0.0;
    });
    k1::ksteps<NT, LG>(k1::a_operand<NT>(xs, wv, l), k1::b_operand(xs, lag0, l), min(k1::TC, n - t0 + 3) >> 2, nl, mask_a,
                       n - t0, l, acc);
  }
  const double scale = blk ? 1.0 : 1.0 / (double)n;   // `corr_scale = 1 / n`, multiplied (mtmvar.py:57-59)
  k1::store_acc(acc, a.R + (size_t)item * (a.p + 1) * MP * MP, lag0, nl, wv, l, [&](int lag) __attribute__((always_inline)) {
    return [&, lag](int row, int col, double v) __attribute__((always_inline)) {
      v = v * scale;
      if (!blk && lag == 0 && row == col && row >= m) v = 1.0;       // padded channels: identity block keeps G SPD
      return v;
    };
  });
}

// ---- windows from hop blocks ------------------------------------------------------------------------------
// With windows of n = k * hop samples every hop, each product x_i[t] x_j[t + l] belongs to up to k windows.  The
// block sums Q_l(b) = sum_{t in block b} x[t] x[t + l]^T (lagcov_kernel in block mode) are computed once, and
//     R_l(w) = (Q_l(w) + ... + Q_l(w + k - 1) - C_l(w)) / n,
//     C_l(w) = sum_{t = n - l}^{n - 1} x[s_w + t] x[s_w + t + l]^T     (the l products that reach past the window end)
// -- half the flops of the direct form at 50 % overlap.  Same biased 1/n estimator, no demeaning (mtmvar.py:57-59,
// 72-73); the sums are merely associated differently, so results agree with the direct form to rounding (not bitwise).
// grid (n_win, p + 1), block 256: NT * NT elements per thread.
//
// The 2 l samples x[:, s+n-l .. s+n+l-1] that C_l needs are contiguous in time, so they are staged as ONE image
// xs[ch][v]: lane v of wave w fetches sample v of the channels w, w + 4, ... (no division, the bounds tests hoisted out
// of the channel loop).  The row stride LC_CS is odd: the element loop reads xs[row][u] (one address per wave at MP = 64:
// a broadcast) and xs[col][l + u] with col running over the lanes, which at the former stride of 32 doubles put every
// lane of a wave on the same bank.  The elements are taken LC_E at a time so that their block-sum loads are in flight
// together; each element's sums keep their order (Q blocks ascending, then the ascending FMA chain over u).
constexpr int LC_CS = 2 * k1::HALO + 1;     // 65
template <int NT>
__global__ void __launch_bounds__(256) lagcomb_kernel(LagcombArgs a) {
  constexpr int MP = 16 * NT, TILE = MP * MP, NE = TILE / 256;
  constexpr int LC_E = (NE % 4 == 0) ? 4 : (NE % 3 == 0) ? 3 : 1;
  __shared__ double xs[MP * LC_CS];
  const long long w = blockIdx.x;
  const int lag = blockIdx.y;
  const int n = (int)(a.hop * a.k), m = a.m;
  const long long s = a.first + w * a.hop;
  {
    const int v = threadIdx.x & 63, wv = uni(threadIdx.x >> 6);
    const long long t = s + n - lag + v;
    const bool staged = v < 2 * lag, in = staged && t < a.T;       // samples past the end of the recording are zeros
    const double* xt = a.x + t;
#pragma unroll
    for (int j = 0; j < MP / 4; ++j) {
      const int ch = 4 * j + wv;                                   // wave-uniform
      double val = 0.0;
      if (in && ch < m) val = xt[(size_t)ch * a.ld];
      if (staged) xs[ch * LC_CS + v] = val;
    }
  }
  __syncthreads();
  const double inv_n = 1.0 / (double)n;
  const size_t qstep = (size_t)(a.p + 1) * TILE;
  const double* Q = a.Q + ((size_t)w * (a.p + 1) + lag) * TILE;
  double* R = a.R + ((size_t)w * (a.p + 1) + lag) * TILE;
  const int k = a.k;
  for (int eb = 0; eb < NE; eb += LC_E) {
    double acc[LC_E], c[LC_E];
    const double *xa[LC_E], *xb[LC_E];
#pragma unroll
    for (int r = 0; r < LC_E; ++r) {
      const unsigned e = threadIdx.x + 256u * (eb + r), row = e / MP, col = e % MP;
      xa[r] = xs + row * LC_CS;
      xb[r] = xs + col * LC_CS + lag;
      acc[r] = 0.0;
      c[r] = 0.0;
    }
    for (int j = 0; j < k; ++j) {
#pragma unroll
      for (int r = 0; r < LC_E; ++r) acc[r] += Q[(size_t)j * qstep + threadIdx.x + 256u * (eb + r)];
    }
    for (int u = 0; u < lag; ++u) {
#pragma unroll
      for (int r = 0; r < LC_E; ++r) c[r] = __builtin_fma(xa[r][u], xb[r][u], c[r]);
    }
#pragma unroll
    for (int r = 0; r < LC_E; ++r) {
      const unsigned e = threadIdx.x + 256u * (eb + r), row = e / MP, col = e % MP;
      double v = (acc[r] - c[r]) * inv_n;
      if (lag == 0 && row == col && (int)row >= m) v = 1.0;    // padded channels: identity block keeps G SPD
      R[e] = v;
    }
  }
}

int launch_lagcomb(const LagcombArgs& a, int m_pad, hipStream_t st) {
  if (a.n_win == 0) return 0;
  if (a.p > k1::HALO) return -2;
  const dim3 grid((unsigned)a.n_win, a.p + 1), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(lagcomb_kernel<decltype(nt)::value>, grid, block, 0, st, a); }))
    return -1;
  return (int)hipGetLastError();
}

template <int LG>
static int launch_lagcov_lg(const LagcovArgs& a, int m_pad, hipStream_t st) {
  const dim3 grid((unsigned)a.n_items, (a.p + LG) / LG), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL((lagcov_kernel<decltype(nt)::value, LG>), grid, block, 0, st, a); }))
    return -1;
  return (int)hipGetLastError();
}

int launch_lagcov(const LagcovArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  if (a.p > k1::HALO) return -2;
  // every lag's sum runs over the same samples in the same order whatever the grouping: same bits for any LG
  const long long lg = tuning(2 /* HMV_TUNE_LAG_GROUP */);
  switch (lg) {
    case 1: return launch_lagcov_lg<1>(a, m_pad, st);
    case 2: return launch_lagcov_lg<2>(a, m_pad, st);
    default: return launch_lagcov_lg<3>(a, m_pad, st);
  }
}

}  // namespace hmv
