// K1 as a weighted sum over trials (hmv_lagcov_mix_f64, hmv_sliding_mix_f64): the trial-averaged lag covariances are
// linear in the per-trial ones, so every resampling of an event-locked ensemble that is a weighted trial sum -- the label
// permutations of the condition contrast -- is one skinny GEMM on the per-trial stack,
//     R[k][w] = scale[k] * sum_e W[k][e] * Rt[e][w],            [rows x trials] . [trials x (w, lag, i, j)]
// and the samples are read once, by the ensemble K1 with groups of one trial.
//
// Mapping: the columns are the flattened (lag, i, j) index of one window's stack of (p+1) MP x MP tiles; a lane owns two
// consecutive columns (one 16-byte load per trial, a wave reads 1 KB of consecutive doubles per trial row) and up to
// MIX_ROWS = 16 mix rows of them in registers, a workgroup 512 columns.  The weights of the tile's rows are wave-uniform:
// they come through the scalar cache, one FMA per (row, column, trial) takes them from SGPRs, and no LDS is used.  Per
// trial and lane that is 16 bytes for 32 FMAs, 4 flop per byte: memory-bound.  The stack is read once per tile of 16 rows.
//
// Order: every output element is ONE chain acc = fma(W[k][e], Rt[e], acc) over e = 0 .. n_trials-1 ascending, then one
// multiplication by scale[k].  No atomics, no split of the trial sum: the bits of element (k, w) depend on row k of W,
// scale[k] and the stack, and on nothing else -- not on the other rows of the tile, n_mix, or the item range of the launch.
// Padding (rows / columns >= m) is written by the kernel, whatever the stack holds there: zero, identity at lag 0.
#include "hmv_common.h"
#include "hmv_kernels.h"

namespace hmv {
namespace {
constexpr int MIX_ROWS = 16;      // mix rows per tile
constexpr int MIX_COLS = 512;     // columns per workgroup: 256 lanes x 2
constexpr int MIX_UNROLL = 2;     // trials in flight per lane (4: 128 SGPRs of weights per pass, which spill)

typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256) lagcov_mix_kernel(const LagcovMixArgs a) {
  const long long tile = (long long)a.m_pad * a.m_pad, stack = tile * (a.p + 1);
  const long long cb = (stack + MIX_COLS - 1) / MIX_COLS;
  const long long w = blockIdx.x / cb;                                  // window of this workgroup
  const long long col = (blockIdx.x - w * cb) * MIX_COLS + 2 * threadIdx.x;
  // the rows of this launch at window w: item k * n_win + w in [it0, it0 + n_items)
  const long long klo = (a.it0 - w + a.n_win - 1 >= 0) ? (a.it0 - w + a.n_win - 1) / a.n_win : 0;
  const long long last = a.it0 + a.n_items - 1 - w;
  if (last < 0) return;
  const long long khi = last / a.n_win;
  const long long k0 = klo + (long long)MIX_ROWS * blockIdx.y;
  if (k0 > khi || col >= stack) return;

  const double* src = a.Rt + w * stack + col;
  const long long ld = a.n_win * stack;                                 // doubles between trials
  // rows past khi read row khi and are not stored; 32-bit offsets from the tile's first row (the launcher checks the range)
  const double* __restrict__ Wt = a.W + k0 * a.n_trials;
  const int nt = (int)a.n_trials, rmax = (int)((khi - k0 < MIX_ROWS - 1) ? khi - k0 : MIX_ROWS - 1);
  f64x2 acc[MIX_ROWS];
#pragma unroll
  for (int r = 0; r < MIX_ROWS; ++r) acc[r] = f64x2{0.0, 0.0};
  int e = 0;
  for (; e + MIX_UNROLL <= nt; e += MIX_UNROLL) {
    f64x2 v[MIX_UNROLL];
#pragma unroll
    for (int u = 0; u < MIX_UNROLL; ++u) v[u] = *reinterpret_cast<const f64x2*>(src + (e + u) * ld);
    // the 16 row offsets are worked out again in every pass (two scalar operations each, on an otherwise idle scalar
    // unit): hoisted out of the loop they are 32 SGPRs that spill; the empty statement keeps them inside
    int rm = rmax;
    asm("" : "+s"(rm) : "s"(e));
    rm = uni(rm);                                                       // (the statement's result counts as divergent)
#pragma unroll
    for (int r = 0; r < MIX_ROWS; ++r) {
      const double* __restrict__ wr = Wt + (r < rm ? r : rm) * nt + e;
#pragma unroll
      for (int u = 0; u < MIX_UNROLL; ++u) {                            // ascending e within every accumulator
        const double wt = wr[u];
        acc[r].x = __builtin_fma(wt, v[u].x, acc[r].x);
        acc[r].y = __builtin_fma(wt, v[u].y, acc[r].y);
      }
    }
  }
  for (; e < nt; ++e) {
    const f64x2 v = *reinterpret_cast<const f64x2*>(src + e * ld);
#pragma unroll
    for (int r = 0; r < MIX_ROWS; ++r) {
      const double wt = Wt[(r < rmax ? r : rmax) * nt + e];
      acc[r].x = __builtin_fma(wt, v.x, acc[r].x);
      acc[r].y = __builtin_fma(wt, v.y, acc[r].y);
    }
  }
  const double* __restrict__ scale = a.scale;
  double sc[MIX_ROWS];
#pragma unroll
  for (int r = 0; r < MIX_ROWS; ++r) sc[r] = scale ? scale[k0 + (r < rmax ? r : rmax)] : 1.0;
  // (lag, i, j) of the lane's two columns: j is even and MP is even, so both lie in one row
  const int lag = (int)(col / tile), rem = (int)(col - (long long)lag * tile);
  const int i = rem / a.m_pad, j = rem - i * a.m_pad;
  const bool real0 = i < a.m && j < a.m, real1 = i < a.m && j + 1 < a.m;
  const double pad0 = (lag == 0 && i == j) ? 1.0 : 0.0, pad1 = (lag == 0 && i == j + 1) ? 1.0 : 0.0;
#pragma unroll
  for (int r = 0; r < MIX_ROWS; ++r) {
    const long long k = k0 + r;
    if (r > rmax) break;
    f64x2 o;
    o.x = real0 ? sc[r] * acc[r].x : pad0;
    o.y = real1 ? sc[r] * acc[r].y : pad1;
    *reinterpret_cast<f64x2*>(a.R + (k * a.n_win + w - a.it0) * stack + col) = o;
  }
}
}  // namespace

int launch_lagcov_mix(const LagcovMixArgs& a, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const long long stack = (long long)a.m_pad * a.m_pad * (a.p + 1);
  const long long cb = (stack + MIX_COLS - 1) / MIX_COLS;
  const long long rows = (a.n_items + a.n_win - 1) / a.n_win;           // most rows a window has in this launch
  const long long gx = a.n_win * cb, gy = (rows + MIX_ROWS - 1) / MIX_ROWS;
  if (gx > 0x7fffffffLL || gy > 65535 || a.n_trials > 0x7fffffffLL / MIX_ROWS) return (int)hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(lagcov_mix_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace hmv
