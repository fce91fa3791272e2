// K1's direct form, once: the pieces every lag-covariance kernel of lagcov.hip and lagcov_ensemble.hip is made of.
//
// Mapping: one workgroup = one item x a group of LG consecutive lags; wave w owns the row strip 4*NT*w .. of each lag's
// MP x MP accumulator (D layout, hmv_common.h; LG * NT * NT accumulators per lane).  The samples are streamed through LDS
// in chunks of TC samples plus a halo of HALO lagged ones -- all global loads of a chunk in flight before the LDS stores
// -- with samples that do not exist and channels past m staged as zeros, so every lag runs the same t-loop.  Per
// 4-sample k-step a wave reads NT A operands once and NT B operands per lag (ds_read_b64, conflict-free because the row
// stride is 6 mod 32 doubles) for LG*NT*NT v_mfma_f64_4x4x4_4b_f64.
//
// A kernel built on this is a source functor (where a staged sample comes from), the call sequence below and an
// epilogue functor (what becomes of a finished sum).  Every piece is inlined into its kernel; nothing here launches.
#pragma once
#include "hmv_common.h"
#include <type_traits>

namespace hmv {
namespace k1 {

constexpr int TC = 64;             // samples per chunk
constexpr int HALO = 32;           // max lag
constexpr int W = TC + HALO;       // 96 staged columns per channel
constexpr int S = W + 6;           // row stride 102 = 6 (mod 32)
static_assert(16 * W % 256 == 0, "every thread stages the same number of elements: no bound test on the element index");
template <int NT>
constexpr int NLD = 16 * NT * W / 256;           // staged elements per thread: 16 * W is a multiple of the 256 threads

template <int NT, int LG>
__device__ __forceinline__ void zero_acc(double (&acc)[LG][NT][NT]) {
#pragma unroll
  for (int g = 0; g < LG; ++g)
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = 0; J < NT; ++J) acc[g][I][J] = 0.0;
}

// where lane l of wave wv reads its A operands (rows of its strip) and its B operands (columns, lag0 samples later)
template <int NT>
__device__ __forceinline__ const double* a_operand(const double* xs, int wv, int l) {
  return xs + (4 * NT * wv + (l & 3)) * S + (l >> 4);
}
__device__ __forceinline__ const double* b_operand(const double* xs, int lag0, int l) {
  return xs + (l & 15) * S + lag0 + (l >> 4);
}

// the chunk that starts at sample t0 into registers: src(ch, t) is sample t of channel ch, zero where there is none
template <int NT, typename Src>
__device__ __forceinline__ void load_chunk(double (&stg)[NLD<NT>], int t0, Src&& src) {
#pragma unroll
  for (int r = 0; r < NLD<NT>; ++r) {
    const int idx = threadIdx.x + 256 * r;
    const int ch = idx / W, tt = idx - ch * W;
    stg[r] = src(ch, t0 + tt);
  }
}
template <int NT>
__device__ __forceinline__ void store_chunk(double* xs, const double (&stg)[NLD<NT>]) {
#pragma unroll
  for (int r = 0; r < NLD<NT>; ++r) {
    const int idx = threadIdx.x + 256 * r;
    const int ch = idx / W, tt = idx - ch * W;
    xs[ch * S + tt] = stg[r];
  }
}
// all loads of the chunk in flight, then the LDS stores; the first barrier waits for the k-steps of the previous chunk
template <int NT, typename Src>
__device__ __forceinline__ void stage_chunk(double* xs, int t0, Src&& src) {
  double stg[NLD<NT>];
  load_chunk<NT>(stg, t0, src);
  __syncthreads();
  store_chunk<NT>(xs, stg);
  __syncthreads();
}

// the k-steps of one staged chunk, same order of products per accumulator whatever NT and LG.  mask_a: the A operand
// ends `rem` samples into the chunk even if real samples are staged behind it (hop blocks).
template <int NT, int LG>
__device__ __forceinline__ void ksteps(const double* xa, const double* xb, int steps, int nl, bool mask_a, int rem, int l,
                                       double (&acc)[LG][NT][NT]) {
  for (int ts = 0; ts < steps; ++ts) {
    double av[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) av[I] = xa[4 * I * S + 4 * ts];
    if (mask_a && 4 * ts + 3 >= rem) {                  // uniform: only the last k-step of a block
      const bool in = 4 * ts + (l >> 4) < rem;
#pragma unroll
      for (int I = 0; I < NT; ++I) av[I] = in ? av[I] : 0.0;
    }
    static_for<LG>([&](auto gc) __attribute__((always_inline)) {
      constexpr int g = decltype(gc)::value;
      if (__builtin_expect(g < nl, 1)) {                // workgroup-uniform.  The hint is for block placement: the MFMAs of a
                                                        // lag fall through, as only the last lag group is short
        double bv[NT];
#pragma unroll
        for (int J = 0; J < NT; ++J) bv[J] = xb[16 * J * S + 4 * ts + g];
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
          for (int J = 0; J < NT; ++J) acc[g][I][J] = mfma4(av[I], bv[J], acc[g][I][J]);
      }
    });
  }
}

// One bit per accumulator [I][J] of wave wv: does it hold a real cross element (one index < split, the other in
// split .. m - 1)?  Without a base stack every accumulator is needed.  Depends on the wave, split and m only, so it
// lives in an SGPR.  An accumulator that straddles split is computed whole.
template <int NT>
__device__ __forceinline__ unsigned need_mask(int wv, int split, int m, bool based) {
  unsigned need = 0;
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int J = 0; J < NT; ++J) {
      const int r0 = 4 * (NT * wv + I), c0 = 16 * J;     // rows r0 .. r0 + 3, columns c0 .. c0 + 15
      const bool rows_a = r0 < split, rows_b = max(r0, split) <= min(r0 + 3, m - 1);
      const bool cols_a = c0 < split, cols_b = max(c0, split) <= min(c0 + 15, m - 1);
      if (!based || (rows_a && cols_b) || (rows_b && cols_a)) need |= 1u << (I * NT + J);
    }
  return (unsigned)uni((int)need);
}
// the k-steps with the accumulators outside `need` left alone: they never see an MFMA, nor their B operand a read
template <int NT, int LG>
__device__ __forceinline__ void ksteps_masked(const double* xa, const double* xb, int steps, int nl, unsigned need,
                                              double (&acc)[LG][NT][NT]) {
  for (int ts = 0; ts < steps; ++ts) {
    double av[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) av[I] = xa[4 * I * S + 4 * ts];
    static_for<LG>([&](auto gc) __attribute__((always_inline)) {
      constexpr int g = decltype(gc)::value;
      if (__builtin_expect(g < nl, 1)) {                // workgroup-uniform.  The hint is for block placement: the MFMAs of a
                                                        // lag fall through, as only the last lag group is short
        static_for<NT>([&](auto jc) __attribute__((always_inline)) {
          constexpr int J = decltype(jc)::value;
          constexpr unsigned COL = ((1u << (NT * NT)) - 1) / ((1u << NT) - 1) << J;   // bits I * NT + J, all I
          if (need & COL) {                             // wave-uniform
            const double bv = xb[16 * J * S + 4 * ts + g];
#pragma unroll
            for (int I = 0; I < NT; ++I)
              if (need & (1u << (I * NT + J))) acc[g][I][J] = mfma4(av[I], bv, acc[g][I][J]);
          }
        });
      }
    });
  }
}

// out[lag][row][col] = epi(lag)(row, col, sum) for the nl lags of this workgroup; `out` is the item's stack of p + 1
// tiles.  The epilogue comes in two steps so that what belongs to a lag (a base stack's tile) is formed once per lag and
// is not held across the lags: that costs the 48-channel pairs kernel its third wave (profiles/k1_core_resources.md).
template <int NT, int LG, typename Epi>
__device__ __forceinline__ void store_acc(const double (&acc)[LG][NT][NT], double* out, int lag0, int nl, int wv, int l,
                                          Epi&& epi) {
  constexpr int MP = 16 * NT;
  const int i = l >> 4, cc = l & 15;
  static_for<LG>([&](auto gc) __attribute__((always_inline)) {
    constexpr int g = decltype(gc)::value;
    if (g < nl) {
      const int lag = lag0 + g;
      double* o = out + (size_t)lag * MP * MP;
      auto e = epi(lag);
#pragma unroll
      for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J) {
          const int row = 4 * (NT * wv + I) + i, col = 16 * J + cc;
          o[(size_t)row * MP + col] = e(row, col, acc[g][I][J]);
        }
    }
  });
}

// ---- two planes, lag 0: the Hermitian Gram matrix C = U U^H of a complex block (phase_sync.hip) ---------------------
// The chunk is staged as two planes (re, im) of TC samples per channel and no halo; the row stride keeps the 6 (mod 32).
// Wave wv owns the row blocks 4 * I + wv, I < NT (interleaved, not a strip), so that in every wave the accumulator [I][J]
// lies on or above the diagonal exactly when J >= I: the triangle is a compile-time loop and the four waves carry the
// same NT (NT + 1) / 2 tiles each.  Lane l holds element (row 4 * (4 * I + wv) + (l >> 4), col 16 * J + (l & 15)).
constexpr int S2 = TC + 6;         // row stride 70 = 6 (mod 32)
template <int NT>
constexpr int NLD2 = 16 * NT * TC / 256;         // staged complex elements per thread

__device__ __forceinline__ const double* a_operand2(const double* xs, int wv, int l) {
  return xs + (4 * wv + (l & 3)) * S2 + (l >> 4);
}
__device__ __forceinline__ const double* b_operand2(const double* xs, int l) { return xs + (l & 15) * S2 + (l >> 4); }

// the chunk that starts at sample t0: src(ch, t) is the complex sample (re in .x, im in .y), zero where there is none.
// All loads in flight, then the LDS stores; the first barrier waits for the k-steps of the previous chunk.
template <int NT, typename Src>
__device__ __forceinline__ void stage_chunk2(double* xre, double* xim, int t0, Src&& src) {
  double2 stg[NLD2<NT>];
#pragma unroll
  for (int r = 0; r < NLD2<NT>; ++r) {
    const int idx = threadIdx.x + 256 * r;
    stg[r] = src(idx / TC, t0 + idx % TC);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NLD2<NT>; ++r) {
    const int idx = threadIdx.x + 256 * r;
    xre[(idx / TC) * S2 + idx % TC] = stg[r].x;
    xim[(idx / TC) * S2 + idx % TC] = stg[r].y;
  }
  __syncthreads();
}

// the k-steps of one staged chunk for the tiles J >= I:  re += re_i re_j + im_i im_j,  im += im_i re_j - re_i im_j, per
// accumulator in this order of products whatever NT.  xa / xb: a_operand2 / b_operand2 of the re plane; the im plane
// lies `plane` doubles behind it.  MASKED: only the tiles whose bit I * NT + J is set in `need` (workgroup-uniform, see
// herm_need) see an MFMA, and only the operands of those tiles an LDS read; a computed tile has the bits it has unmasked.
template <int NT, bool MASKED = false>
__device__ __forceinline__ void ksteps_herm(const double* xa, const double* xb, int plane, int steps, double (&re)[NT][NT],
                                            double (&im)[NT][NT], unsigned need = 0) {
  constexpr unsigned ROW = (1u << NT) - 1, COL = ((1u << (NT * NT)) - 1) / ROW;   // bits I * NT + J: all J of I = 0, all I of J = 0
  for (int ts = 0; ts < steps; ++ts) {
    double ar[NT], ai[NT], br[NT], bi[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) {
      if (!MASKED || (need & (ROW << (I * NT)))) {
        ar[I] = xa[16 * I * S2 + 4 * ts];
        ai[I] = xa[plane + 16 * I * S2 + 4 * ts];
      }
      if (!MASKED || (need & (COL << I))) {
        br[I] = xb[16 * I * S2 + 4 * ts];
        bi[I] = xb[plane + 16 * I * S2 + 4 * ts];
      }
    }
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
      for (int J = I; J < NT; ++J)
        if (!MASKED || (need & (1u << (I * NT + J)))) {
          re[I][J] = mfma4(ar[I], br[J], re[I][J]);
          re[I][J] = mfma4(ai[I], bi[J], re[I][J]);
          im[I][J] = mfma4(ai[I], br[J], im[I][J]);
          im[I][J] = mfma4_nega(ar[I], bi[J], im[I][J]);
        }
  }
}

// The tiles [I][J] of the pairs form (bit I * NT + J): those that hold a cross element (row < split <= column) -- not
// 16 I >= split, not 16 J + 15 < split, not J < I; a tile that straddles split is computed whole -- and, with `diag`, the
// diagonal tiles [I][I] (the RAW mode's C_ii).  The same in every wave: rows 16 I .. 16 I + 15 are spread over the four.
template <int NT>
__device__ __forceinline__ unsigned herm_need(int split, bool diag) {
  unsigned need = 0;
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int J = I; J < NT; ++J)
      if ((16 * I < split && 16 * J + 15 >= split) || (diag && I == J)) need |= 1u << (I * NT + J);
  return (unsigned)uni((int)need);
}

}  // namespace k1
}  // namespace hmv
