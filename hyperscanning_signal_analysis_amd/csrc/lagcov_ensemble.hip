// K1 for event-locked ensembles -- lag covariances of one window averaged over the trials of a group:
//     R_l(it) = (1/E_g) sum_{e in g} (1/n) X_e[:, :n-l] X_e[:, l:]^T,   X_e = x[trial_rec[e]][:, trial_start[e] + offset(it) : + n]
//
// Replaces `count_corr` on 3-D input (src/mtmvar.py:54-85 of the reference: the lag products of every trial, biased 1/n
// scaling, no demeaning, then the mean over the trials) for every window of an epoch at once.  Two forms:
//
//  * direct (lagcov_ens_kernel): the direct form of lagcov_core.h -- one workgroup = one item x LG = 3 lags, wave w owns a
//    strip of MP/4 rows -- with the loop over the group's trials INSIDE the kernel.  The LG*NT*NT accumulators stay
//    in registers across the trials and one R stack per item is written, never one per trial.  Trials are summed in
//    ascending order and every trial in lagcov_kernel's order (64-sample chunks, 4-sample k-steps), so a group of one
//    trial gives the bits of hmv_lagcov_f64 on that window.  (Loading the next (trial, chunk) into registers under the
//    k-steps of the current one was built and measured: no gain at 19 channels -- the second workgroup of the CU already
//    covers the load latency -- and no registers for it at 64; the chunks are staged as lagcov_kernel stages them.)
//  * shared overlap (lagens_block_kernel + lagens_comb_kernel), items on a regular grid offset = w * hop, n = k * hop:
//        Q_l(g, b) = sum_e sum_{t in block b} x_e[t] x_e[t + l]^T                 once per hop block, all trials
//        R_l(g, w) = (Q_l(g, w) + ... + Q_l(g, w + k - 1) - C_l(g, w)) / n / E_g   C_l: trial-summed products past the window end
//    -- the algebra of lagcomb_kernel, 1/k of the flops.  A hop block is a few k-steps per trial, so one LDS fill holds
//    the blocks (+ p lagged samples) of as many trials as fit into the 96 staged columns.
#include "hmv_common.h"
#include "hmv_kernels.h"
#include "lagcov_core.h"

namespace hmv {

constexpr int LE_MAX_TPF = 16;                 // shared form: trials per LDS fill
constexpr int LE_MAX_K = 32;                    // shared form: hops per window (HMV_MAX_HOPS_ENSEMBLE)
constexpr int LE_CS = 33;                      // combine step: row stride of the staged tail samples

// ---- direct form: grid (items, ceil((p+1) / LG)) -----------------------------------------------------------------
template <int NT, int LG>
__global__ void __launch_bounds__(256, 2) lagcov_ens_kernel(LagcovEnsArgs a) {
  constexpr int MP = 16 * NT;
  __shared__ double xs[MP * k1::S];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int lag0 = blockIdx.y * LG;
  const int nl = min(LG, a.p + 1 - lag0);
  const int n = a.n, m = a.m;
  const long long g = a.item_group[item], off = a.item_offset[item];
  const long long e0 = a.group_ptr[g], e1 = a.group_ptr[g + 1];
  const long long E = e1 - e0;

  double acc[LG][NT][NT];
  k1::zero_acc(acc);
  double stg[k1::NLD<NT>];
  const int nch = (n + k1::TC - 1) / k1::TC;
  const long long steps = E * nch;                      // (trial, chunk) steps, trial-major
  long long e = e0;
  int t0 = 0;
  const double* xa = k1::a_operand<NT>(xs, wv, l);
  const double* xb = k1::b_operand(xs, lag0, l);
  for (long long s = 0; s < steps; ++s) {
    const double* x = a.x + a.trial_rec[e] * a.rec_stride + a.trial_start[e] + off;
    k1::load_chunk<NT>(stg, t0, [&](int ch, int t) __attribute__((always_inline)) {
      return (ch < m && t < n) ? x[(size_t)ch * a.ld + t] : 0.0;
    });
    __syncthreads();                                    // the k-steps of the previous chunk have read xs
    k1::store_chunk<NT>(xs, stg);
    __syncthreads();
    const int tc = t0;
    t0 += k1::TC;
    if (t0 >= n) { t0 = 0; ++e; }
    k1::ksteps<NT, LG>(xa, xb, min(k1::TC, n - tc + 3) >> 2, nl, false, 0, l, acc);
  }
  const double scale = 1.0 / (double)n;                 // `corr_scale = 1 / n`, multiplied (mtmvar.py:57-59)
  const double Ed = (double)E;
  k1::store_acc(acc, a.R + (size_t)item * (a.p + 1) * MP * MP, lag0, nl, wv, l, [&](int lag) __attribute__((always_inline)) {
    return [&, lag](int row, int col, double v) __attribute__((always_inline)) {
      v = v * scale;
      if (E > 1) v = v / Ed;                                         // the mean over the trials (mtmvar.py:78-85)
      if (lag == 0 && row == col && row >= m) v = 1.0;               // padded channels: identity block keeps G SPD
      return v;
    };
  });
}

// ---- direct form with a second trial table (trial-shuffle surrogates) ----------------------------------------------------
// Trial step e stages the channels < split from trial (trial_rec[e], trial_start[e]) and the channels >= split from trial
// (trial_rec_b[e], trial_start_b[e]): x~_e = [a_e ; b_pi(e)], the permutation being nothing but the order of table B.  The
// mapping, the chunks, the k-steps and the order of products per accumulator are lagcov_ens_kernel's, so table B = table A
// gives its bits.
// With R_base the within-participant elements -- both indices < split or both >= split, padding counting as >= split --
// are sums over ALL trials that no permutation changes: they are copied from R_base[item_base[item]] and an accumulator
// whose real elements (row, col < m) are all of that kind never sees an MFMA (k1::need_mask, formed before the trial
// loop).  An accumulator that straddles split is computed whole and its within-participant elements are then overwritten,
// so the result does not depend on the tiling.
// This kernel takes the core's geometry, need mask, operand pointers and masked k-steps and keeps its own staging and
// accumulator store: on k1::load_chunk / store_chunk / store_acc its K1 time was 2 to 3.6 % above the parent's at both
// channel counts measured (profiles/k1_core_refactor.json, `split_kernel_on_shared_staging`) with nothing in the resource
// table or the k-step loop to account for it; written as here, its ISA is the parent's but for a few scalar instructions.
template <int NT, int LG>
__global__ void __launch_bounds__(256, 2) lagcov_ens_split_kernel(LagcovEnsArgs a) {
  constexpr int MP = 16 * NT;
  __shared__ double xs[MP * k1::S];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int lag0 = blockIdx.y * LG;
  const int nl = min(LG, a.p + 1 - lag0);
  const int i = l >> 4, cc = l & 15;
  const int n = a.n, m = a.m, split = a.split;
  const long long g = a.item_group[item], off = a.item_offset[item];
  const long long e0 = a.group_ptr[g], e1 = a.group_ptr[g + 1];
  const long long E = e1 - e0;
  const bool based = a.R_base != nullptr;

  const unsigned need = k1::need_mask<NT>(wv, split, m, based);

  double acc[LG][NT][NT];
  k1::zero_acc(acc);
  constexpr int NLD = (MP * k1::W + 255) / 256;
  double stg[NLD];
  auto load = [&](long long e, int t0) __attribute__((always_inline)) {
    const double* xA = a.x + a.trial_rec[e] * a.rec_stride + a.trial_start[e] + off;
    const double* xB = a.x + a.trial_rec_b[e] * a.rec_stride + a.trial_start_b[e] + off;
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = threadIdx.x + 256 * r;
      const int ch = idx / k1::W, tt = idx - ch * k1::W;
      const int t = t0 + tt;
      const double* x = ch < split ? xA : xB;
      stg[r] = (idx < MP * k1::W && ch < m && t < n) ? x[(size_t)ch * a.ld + t] : 0.0;
    }
  };
  const int nch = (n + k1::TC - 1) / k1::TC;
  const long long S = E * nch;                          // (trial, chunk) steps, trial-major
  long long e = e0;
  int t0 = 0;
  const double* xa = k1::a_operand<NT>(xs, wv, l);
  const double* xb = k1::b_operand(xs, lag0, l);
  for (long long s = 0; s < S; ++s) {
    load(e, t0);
    __syncthreads();                                    // the k-steps of the previous chunk have read xs
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = threadIdx.x + 256 * r;
      const int ch = idx / k1::W, tt = idx - ch * k1::W;
      if (idx < MP * k1::W) xs[ch * k1::S + tt] = stg[r];
    }
    __syncthreads();
    const int tc = t0;
    t0 += k1::TC;
    if (t0 >= n) { t0 = 0; ++e; }
    k1::ksteps_masked<NT, LG>(xa, xb, min(k1::TC, n - tc + 3) >> 2, nl, need, acc);
  }
  const double scale = 1.0 / (double)n;
  const double Ed = (double)E;
  static_for<LG>([&](auto gc) __attribute__((always_inline)) {
    constexpr int q = decltype(gc)::value;
    if (q < nl) {
      const int lag = lag0 + q;
      double* R = a.R + ((size_t)item * (a.p + 1) + lag) * MP * MP;
      const double* Rb = based ? a.R_base + ((size_t)a.item_base[item] * (a.p + 1) + lag) * MP * MP : nullptr;
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J) {
          const int row = 4 * (NT * wv + I) + i, col = 16 * J + cc;
          double v = acc[q][I][J] * scale;
          if (E > 1) v = v / Ed;
          if (lag == 0 && row == col && row >= m) v = 1.0;
          if (based && (row < split) == (col < split)) v = Rb[(size_t)row * MP + col];   // (split < m: padding is >= split)
          R[(size_t)row * MP + col] = v;
        }
    }
  });
}

// ---- pairs of recordings (pseudo-dyad surrogates) -------------------------------------------------------------------------
// Item `it` stages the channels < split from recording rec_a[it] and the channels >= split from recording rec_b[it], both at
// item_start[it]: participant A of one dyad beside participant B of another, time-locked.  One window per item, so there is
// no trial loop and no division by a trial count: every computed element has the bits hmv_lagcov_f64 gives for the same
// window written out as one recording.  With R_base the elements with both indices < split come from R_base[base_a[it]] and
// the elements with both indices >= split (padding and its lag-0 identity included) from R_base[base_b[it]] -- two different
// stacks, where lagcov_ens_split_kernel has one; the `need` mask and the rule for accumulators that straddle split are that
// kernel's.
template <int NT, int LG>
__global__ void __launch_bounds__(256, 2) lagcov_pairs_kernel(LagcovPairsArgs a) {
  constexpr int MP = 16 * NT;
  __shared__ double xs[MP * k1::S];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int lag0 = blockIdx.y * LG;
  const int nl = min(LG, a.p + 1 - lag0);
  const int n = a.n, m = a.m, split = a.split;
  const bool based = a.R_base != nullptr;
  const long long start = a.item_start[item];
  const double* xA = a.x + a.rec_a[item] * a.rec_stride + start;
  const double* xB = a.x + a.rec_b[item] * a.rec_stride + start;
  const unsigned need = k1::need_mask<NT>(wv, split, m, based);

  double acc[LG][NT][NT];
  k1::zero_acc(acc);
  const double* xa = k1::a_operand<NT>(xs, wv, l);
  const double* xb = k1::b_operand(xs, lag0, l);
  for (int t0 = 0; t0 < n; t0 += k1::TC) {
    k1::stage_chunk<NT>(xs, t0, [&](int ch, int t) __attribute__((always_inline)) {
      const double* x = ch < split ? xA : xB;
      return (ch < m && t < n) ? x[(size_t)ch * a.ld + t] : 0.0;
    });
    k1::ksteps_masked<NT, LG>(xa, xb, min(k1::TC, n - t0 + 3) >> 2, nl, need, acc);
  }
  const double scale = 1.0 / (double)n;                 // `corr_scale = 1 / n`, multiplied (mtmvar.py:57-59)
  const size_t stack = (size_t)(a.p + 1) * MP * MP;
  k1::store_acc(acc, a.R + (size_t)item * stack, lag0, nl, wv, l, [&](int lag) __attribute__((always_inline)) {
    const double* Ra = based ? a.R_base + (size_t)a.base_a[item] * stack + (size_t)lag * MP * MP : nullptr;
    const double* Rb = based ? a.R_base + (size_t)a.base_b[item] * stack + (size_t)lag * MP * MP : nullptr;
    return [&, lag, Ra, Rb](int row, int col, double v) __attribute__((always_inline)) {
      v = v * scale;
      if (lag == 0 && row == col && row >= m) v = 1.0;               // padded channels: identity block keeps G SPD
      if (based && (row < split) == (col < split))                   // (split < m: padding is >= split)
        v = (row < split ? Ra : Rb)[(size_t)row * MP + col];
      return v;
    };
  });
}

// ---- shared-overlap form --------------------------------------------------------------------------------------------
// Items it0 .. it0 + n_items - 1 of the grid (item = g * nwin + w) touch the groups g0 .. g0 + ngc - 1; group g0 + gi owns
// the Q slots gi * nblk .. + nblk - 1 (nblk = nwin + k - 1 hop blocks), of which only those under a window of the chunk
// are summed.
struct LeSpan {
  long long g, wlo, whi;     // group, its windows [wlo, whi) inside the chunk
};
__device__ __forceinline__ LeSpan le_span(const LagcovEnsArgs& a, long long gi) {
  LeSpan s;
  s.g = a.it0 / a.nwin + gi;
  const long long glo = s.g * a.nwin, ghi = glo + a.nwin, iend = a.it0 + a.n_items;
  const long long ilo = a.it0 > glo ? a.it0 : glo, ihi = iend < ghi ? iend : ghi;
  s.wlo = ilo - s.g * a.nwin;
  s.whi = ihi - s.g * a.nwin;
  return s;
}

// grid (ngc * nblk, ceil((p+1) / LG)): Q[slot][lag] = sum over the group's trials of the block's lag products, unscaled,
// padding zero.  The lagged partners x[t + l] of a block's last samples are read past the block, up to the end of the
// recording (zero beyond it).
template <int NT, int LG>
__global__ void __launch_bounds__(256, 2) lagens_block_kernel(LagcovEnsArgs a) {
  constexpr int MP = 16 * NT;
  __shared__ double xs[MP * k1::S];
  __shared__ long long tb_off[2][LE_MAX_TPF];           // per fill: where the block of trial slot j starts ...
  __shared__ int tb_vl[2][LE_MAX_TPF];                  // ... and how many samples from there exist (0: no trial)
  const long long nblk = a.nwin + a.k - 1;
  const long long gi = blockIdx.x / nblk, b = blockIdx.x - gi * nblk;
  const LeSpan sp = le_span(a, gi);
  if (b < sp.wlo || b >= sp.whi + a.k - 1) return;      // workgroup-uniform, before any barrier
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const int lag0 = blockIdx.y * LG;
  const int nl = min(LG, a.p + 1 - lag0);
  const int m = a.m, hop = (int)a.hop;
  const int hopr = (hop + 3) & ~3;                      // whole k-steps
  const int SW = hopr + a.p;                            // staged columns per trial: the block and its p lagged samples
  const int TPF = min(LE_MAX_TPF, k1::W / SW);           // >= 1: the launcher refuses SW > k1::W
  const long long e0 = a.group_ptr[sp.g], e1 = a.group_ptr[sp.g + 1];
  const long long E = e1 - e0;

  double acc[LG][NT][NT];
  k1::zero_acc(acc);

  // element r of this thread in every fill: channel (threadIdx.x + 256 r) / 96, staged column c = (threadIdx.x + 256 r)
  // mod 96 = trial slot * SW + column inside the slot.  256 * 3 is a multiple of 96: three distinct columns per thread.
  constexpr int NLD = k1::NLD<NT>;
  int cj[3], ct[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int c = (threadIdx.x + 256 * q) % k1::W;
    cj[q] = c / SW;
    ct[q] = c - cj[q] * SW;
    if (cj[q] >= TPF) { cj[q] = 0; ct[q] = k1::W; }       // columns past the last slot: staged as zeros, never read
  }
  auto table = [&](long long f, int buf) __attribute__((always_inline)) {
    if ((int)threadIdx.x < TPF) {
      const long long e = e0 + f * TPF + threadIdx.x;
      long long o = 0;
      int vl = 0;
      if (e < e1) {
        const long long start = a.trial_start[e] + b * a.hop;
        o = a.trial_rec[e] * a.rec_stride + start;
        const long long left = a.T - start;
        vl = (int)(left < 0 ? 0 : (left > SW ? SW : left));
      }
      tb_off[buf][threadIdx.x] = o;
      tb_vl[buf][threadIdx.x] = vl;
    }
  };
  double stg[NLD];
  auto load = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int idx = threadIdx.x + 256 * r;
      const int ch = idx / k1::W, j = cj[r % 3], tt = ct[r % 3];
      const bool in = idx < MP * k1::W && ch < m && tt < tb_vl[buf][j];
      stg[r] = in ? a.x[tb_off[buf][j] + (long long)ch * a.ld + tt] : 0.0;
    }
  };
  const long long nf = (E + TPF - 1) / TPF;
  if (nf > 0) {
    table(0, 0);
    __syncthreads();
  }
  const double* xa = k1::a_operand<NT>(xs, wv, l);
  const double* xb = k1::b_operand(xs, lag0, l);
  const bool mask_a = (hop & 3) != 0;                   // the A operand ends at the block even if real samples follow
  for (long long f = 0; f < nf; ++f) {
    load((int)(f & 1));
    __syncthreads();                                    // the k-steps of the previous fill have read xs
    k1::store_chunk<NT>(xs, stg);
    if (f + 1 < nf) table(f + 1, (int)((f + 1) & 1));   // for the next fill's loads; its buffer was last read a fill ago
    __syncthreads();
    const long long left = E - f * TPF;
    const int live = (int)(left < TPF ? left : TPF);
    for (int j = 0; j < live; ++j) k1::ksteps<NT, LG>(xa + j * SW, xb + j * SW, hopr >> 2, nl, mask_a, hop, l, acc);
  }
  k1::store_acc(acc, a.Q + (size_t)blockIdx.x * (a.p + 1) * MP * MP, lag0, nl, wv, l, [](int) __attribute__((always_inline)) {
    return [](int, int, double v) __attribute__((always_inline)) { return v; };   // unscaled, padding zero
  });
}

// grid (n_items, p + 1), block 256: NT * NT elements per thread.  The tails x[:, s+n-l .. s+n-1] and x[:, s+n .. s+n+l-1]
// of as many trials as fit into 32 columns are staged side by side, so the correction is one run of FMAs per fill.
template <int NT>
__global__ void __launch_bounds__(256) lagens_comb_kernel(LagcovEnsArgs a) {
  constexpr int MP = 16 * NT, TILE = MP * MP, NE = NT * NT;
  __shared__ double xa[MP * LE_CS], xb[MP * LE_CS];
  const long long item = a.it0 + blockIdx.x;
  const long long g = item / a.nwin, w = item - g * a.nwin;
  const long long gi = g - a.it0 / a.nwin;
  const long long nblk = a.nwin + a.k - 1;
  const int lag = blockIdx.y;
  const int n = a.n, m = a.m;
  const long long e0 = a.group_ptr[g], e1 = a.group_ptr[g + 1];
  const long long E = e1 - e0;
  double c[NE];
#pragma unroll
  for (int q = 0; q < NE; ++q) c[q] = 0.0;
  if (lag > 0) {
    const int tpf = 32 / lag;
    for (long long eb = e0; eb < e1; eb += tpf) {
      const int live = (int)((e1 - eb) < tpf ? (e1 - eb) : tpf);
      const int nq = live * lag;
      __syncthreads();
      for (int idx = threadIdx.x; idx < MP * nq; idx += 256) {
        const int ch = idx / nq, q = idx - ch * nq;
        const int j = q / lag, u = q - j * lag;
        const long long e = eb + j;
        const long long ta = a.trial_start[e] + w * a.hop + n - lag + u, tb = ta + lag;
        const double* x = a.x + a.trial_rec[e] * a.rec_stride + (long long)ch * a.ld;
        xa[ch * LE_CS + q] = (ch < m && ta < a.T) ? x[ta] : 0.0;
        xb[ch * LE_CS + q] = (ch < m && tb < a.T) ? x[tb] : 0.0;
      }
      __syncthreads();
      for (int q = 0; q < nq; ++q) {
#pragma unroll
        for (int r = 0; r < NE; ++r) {
          const int el = threadIdx.x + 256 * r;
          const int row = el / MP, col = el - row * MP;
          c[r] = __builtin_fma(xa[row * LE_CS + q], xb[col * LE_CS + q], c[r]);
        }
      }
    }
  }
  const double inv_n = 1.0 / (double)n;
  const double Ed = (double)E;
  const double* Q = a.Q + ((size_t)(gi * nblk + w) * (a.p + 1) + lag) * TILE;
  double* R = a.R + ((size_t)blockIdx.x * (a.p + 1) + lag) * TILE;
#pragma unroll
  for (int r = 0; r < NE; ++r) {
    const int el = threadIdx.x + 256 * r;
    const int row = el / MP, col = el - row * MP;
    double acc = 0.0;
    for (int j = 0; j < a.k; ++j) acc += Q[(size_t)j * (a.p + 1) * TILE + el];
    double v = (acc - c[r]) * inv_n;
    if (E > 1) v = v / Ed;
    if (lag == 0 && row == col && row >= m) v = 1.0;    // padded channels: identity block keeps G SPD
    R[el] = v;
  }
}

bool lagcov_ensemble_shared_ok(int n, long long hop, int p, int max_k) {
  if (hop < 1 || n % hop != 0 || hop <= p) return false;
  const long long k = n / hop;
  return k >= 2 && k <= max_k && ((hop + 3) & ~3LL) + p <= k1::W;   // one LDS fill holds a trial's block and its lags
}

long long lagcov_ensemble_q_tiles(long long n_items, long long nwin, int k) {
  if (n_items < 1 || nwin < 1 || k < 1) return 0;
  return ((n_items - 1) / nwin + 2) * (nwin + k - 1);             // a chunk may start and end inside a group
}

int launch_lagcov_ensemble(const LagcovEnsArgs& a, int m_pad, bool shared, hipStream_t st) {
  if (a.n_items == 0) return 0;
  if (a.p > k1::HALO) return -2;
  constexpr int LG = 3;
  const dim3 block(256), grid((unsigned)a.n_items, (a.p + LG) / LG);
  if (!shared) {
    if (for_nt(m_pad, [&](auto nt) {
          hipLaunchKernelGGL((lagcov_ens_kernel<decltype(nt)::value, LG>), grid, block, 0, st, a);
        }))
      return -1;
    return (int)hipGetLastError();
  }
  if (!lagcov_ensemble_shared_ok(a.n, a.hop, a.p, LE_MAX_K) || a.n / a.hop != a.k || a.nwin < 1 || !a.Q) return -3;
  const long long ngc = (a.it0 + a.n_items - 1) / a.nwin - a.it0 / a.nwin + 1;
  const dim3 gq((unsigned)(ngc * (a.nwin + a.k - 1)), (a.p + LG) / LG), gc((unsigned)a.n_items, a.p + 1);
  if (for_nt(m_pad, [&](auto nt) {
        hipLaunchKernelGGL((lagens_block_kernel<decltype(nt)::value, LG>), gq, block, 0, st, a);
        hipLaunchKernelGGL(lagens_comb_kernel<decltype(nt)::value>, gc, block, 0, st, a);
      }))
    return -1;
  return (int)hipGetLastError();
}

int launch_lagcov_ensemble_split(const LagcovEnsArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  if (a.p > k1::HALO) return -2;
  if (!a.trial_rec_b || !a.trial_start_b || a.split < 1 || a.split >= a.m || (a.R_base != nullptr) != (a.item_base != nullptr))
    return -4;
  constexpr int LG = 3;
  const dim3 block(256), grid((unsigned)a.n_items, (a.p + LG) / LG);
  if (for_nt(m_pad, [&](auto nt) {
        hipLaunchKernelGGL((lagcov_ens_split_kernel<decltype(nt)::value, LG>), grid, block, 0, st, a);
      }))
    return -1;
  return (int)hipGetLastError();
}

int launch_lagcov_pairs(const LagcovPairsArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  if (a.p > k1::HALO) return -2;
  if (!a.rec_a || !a.rec_b || !a.item_start || a.split < 1 || a.split >= a.m ||
      (a.R_base != nullptr) != (a.base_a != nullptr) || (a.R_base != nullptr) != (a.base_b != nullptr))
    return -4;
  constexpr int LG = 3;
  const dim3 block(256), grid((unsigned)a.n_items, (a.p + LG) / LG);
  if (for_nt(m_pad, [&](auto nt) {
        hipLaunchKernelGGL((lagcov_pairs_kernel<decltype(nt)::value, LG>), grid, block, 0, st, a);
      }))
    return -1;
  return (int)hipGetLastError();
}

}  // namespace hmv
