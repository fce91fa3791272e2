// The block Levinson-Whittle recursion of K2 as one device function, shared by its two kernels: yw_lwr.hip (a fixed order
// for the whole batch) and yw_auto.hip (AUTO: the same walk to the largest order with the model-order criterion, its first
// arg-min and a snapshot of the best model taken on the way).  The algebra, the numerics and the conditioning guard are
// described at the head of yw_lwr.hip; what AUTO adds is described at the head of yw_auto.hip.  AUTO is a compile-time
// switch: the fixed-order instantiations contain none of it.
//
// LEGACY is the second compile-time switch: the walk as it was before the lower-lag updates were paired (backward update
// indexed by k, so that every A_k / B_k tile is read twice several iterations apart; Vf_0 = Vb_0 = R_0 stored, loaded back
// and inverted twice; the model always emitted).  It computes the same bits and is kept, behind HMV_TUNE_YW_FORM = 4, as
// the reference the tests hold the default walk against.
#pragma once
#include "yw_common.h"

namespace hmv {

#ifndef HMV_LWR_GUARD
#define HMV_LWR_GUARD 1e-7
#endif

template <int NT, bool VQ, bool AUTO, bool LEGACY = false>
__device__ __forceinline__ void yw_lwr_body(const YwArgs& a, const YwAutoArgs& sel) {
  static_assert(VQ || !AUTO, "the selecting form needs every log det Vf_q");
  constexpr int MP = 16 * NT, KH = MP / 2, SH = KH + 6, NIW = NT, NJ = NT, TILE = MP * MP;
  constexpr int NV = (MP * KH / 2 + 255) / 256;
  constexpr int SI = YwCfg<NT>::S;
  // one inverse at order 0.  Not in the selecting form: there it cost two more spilled VGPRs at 64 channels, in every
  // arrangement tried (pointer selects, branches, the inverse ahead of the loop), and that kernel has none to give.
  constexpr bool ONE0 = !LEGACY && !AUTO;
  constexpr int GEMM_D = 2 * MP * SH, INV_D = MP * SI, BUF_D = GEMM_D > INV_D ? GEMM_D : INV_D;
  __shared__ __attribute__((aligned(16))) double buf[BUF_D];
  __shared__ double Pb[2 * MP * 4];            // two panel and four N buffers: both inverses of an order at once
  __shared__ double Nb[4 * MP * 4];
  __shared__ int s_info;
  __shared__ double s_ld[4];
  __shared__ double s_pm[4 + 4 * 4];
  __shared__ int s_guard;
  // AUTO only: log det Vf_q of the order just inverted, the best criterion so far, its order, "this order improved"
  __shared__ double s_logdet, s_best;
  __shared__ int s_qstar, s_take;
  double* Xh = buf;
  double* Yh = buf + MP * SH;
  const int wv = uni(threadIdx.x >> 6);
  const int p = a.p;
  const long long item = blockIdx.x;
  // scratch tiles of this window: A and B in two generations, Vf, Vb, their inverses, D, and one spare
  double* ws = a.ws + (size_t)item * yw_ws_tiles_d(p) * TILE;
  double* Agen[2] = {ws, ws + (size_t)p * TILE};
  double* Bgen[2] = {ws + (size_t)2 * p * TILE, ws + (size_t)3 * p * TILE};
  double* Vf = ws + (size_t)4 * p * TILE;
  double* Vb = Vf + TILE;
  double* VfI = Vb + TILE;
  double* VbI = VfI + TILE;
  double* Dq = VbI + TILE;
  const double* R = a.R + (size_t)item * (p + 1) * TILE;
  if (threadIdx.x == 0) {
    s_info = 0;
    s_guard = 0;
    if (AUTO) {
      s_best = __builtin_inf();
      s_qstar = 0;
    }
  }

  auto lane = [&]() __attribute__((always_inline)) {
    int lo;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lo));
    return lo;
  };
  auto zero = [&](double (&v)[NIW][NJ]) __attribute__((always_inline)) {
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
      for (int J = 0; J < NJ; ++J) v[ii][J] = 0.0;
  };
  // ---- addressing.  Every tile base is wave-uniform (it depends on blockIdx.x, q, k and p only), so a tile element is
  // addressed as that base, advanced by scalar adds for the steps that are compile-time or wave-uniform (wave strip, r,
  // ii, k-half), plus an UNSIGNED 32-bit byte offset per lane: the scalar-base form of the global instructions, with the
  // small steps (J) in their immediate field.  The per-lane offsets are shifts and masks of the thread index, recomputed
  // where they are used (tid() is opaque to the optimiser on purpose: offsets kept live across the recursion would be
  // spilled -- the kernel sits at its register ceiling).
  auto tid = [&]() __attribute__((always_inline)) {
    unsigned t;
    asm volatile("v_mov_b32 %0, %1" : "=v"(t) : "v"(threadIdx.x));
    return t;
  };
  // (a constant step beyond the instruction's 12-bit immediate is added to the base in scalar registers, where it is
  // used: the empty asm keeps the optimiser from moving it behind the per-lane offset, where it would need a 64-bit
  // vector add, and from keeping every stepped base live in scalar registers the kernel does not have)
  typedef const char __attribute__((address_space(1))) * gcptr;
  auto gptr = [&](const double* base, unsigned cbytes, unsigned off) __attribute__((always_inline)) {
    unsigned long long sb = reinterpret_cast<unsigned long long>(base) + (cbytes & ~0xfffu);
    if (cbytes & ~0xfffu) asm volatile("" : "+s"(sb));
    return reinterpret_cast<gcptr>(sb) + (cbytes & 0xfffu) + (size_t)off;
  };
  // ---- operand staging, one k-half at a time (as in yw_solve.hip).  Plain image: dst[row][k] = src[row][kh*KH + k];
  // transposed image: dst[col][k] = src[kh*KH + k][col].  Thread idx = t + 256 r moves the pair (row, 2 c2) resp.
  // (k, 2 c2); where 256 is a multiple of the pairs per row (NT = 1, 2, 4) the r step is a whole number of rows and goes
  // into the scalar base / the LDS immediate.
  constexpr unsigned PR = KH / 2, PT = MP / 2;          // pairs per row of the plain / the transposed image
  constexpr bool RSTEP = (256 % PR == 0) && (256 % PT == 0);
  auto fetch = [&](f64x2 (&v)[NV], const double* src, int kh, bool tr) __attribute__((always_inline)) {
    const unsigned t = tid();
    if (RSTEP) {
      const unsigned off = !tr ? ((t / PR) * MP + 2 * (t % PR)) * 8u : ((t / PT) * MP + 2 * (t % PT)) * 8u;
#pragma unroll
      for (int r = 0; r < NV; ++r) {
        const unsigned cb = !tr ? (r * (256 / PR) * MP + kh * KH) * 8u : (kh * KH + r * (256 / PT)) * MP * 8u;
        if (NV * 256 == MP * KH / 2 || t + 256 * r < MP * KH / 2) v[r] = *reinterpret_cast<const f64x2 __attribute__((address_space(1)))*>(gptr(src, cb, off));
      }
    } else {
#pragma unroll
      for (int r = 0; r < NV; ++r) {
        const unsigned idx = t + 256 * r;
        if (NV * 256 == MP * KH / 2 || idx < MP * KH / 2) {
          const unsigned off = !tr ? ((idx / PR) * MP + 2 * (idx % PR)) * 8u : ((idx / PT) * MP + 2 * (idx % PT)) * 8u;
          const unsigned cb = !tr ? kh * KH * 8u : kh * KH * MP * 8u;
          v[r] = *reinterpret_cast<const f64x2 __attribute__((address_space(1)))*>(gptr(src, cb, off));
        }
      }
    }
  };
  auto park = [&](double* dst, const f64x2 (&v)[NV], bool tr) __attribute__((always_inline)) {
    const unsigned t = tid();
#pragma unroll
    for (int r = 0; r < NV; ++r) {
      const unsigned idx = RSTEP ? t : t + 256 * r;       // (RSTEP: the r step is the constant added below)
      if (NV * 256 == MP * KH / 2 || t + 256 * r < MP * KH / 2) {
        if (!tr) {
          double* d = dst + (RSTEP ? r * (256 / PR) * SH : 0) + ((idx / PR) * SH + 2 * (idx % PR));
          d[0] = v[r].x;
          d[1] = v[r].y;
        } else {
          double* d = dst + (RSTEP ? r * (256 / PT) : 0) + ((2 * (idx % PT)) * SH + idx / PT);
          d[0] = v[r].x;
          d[SH] = v[r].y;
        }
      }
    }
  };
  // (whether column block J of the strip lies in k-half kh is known at compile time unless the half's edge cuts it)
  auto park_strip = [&](const double (&v)[NIW][NJ], int kh) __attribute__((always_inline)) {
    const unsigned l = lane(), i = l >> 4, cc = l & 15;
    double* d = Xh + (unsigned)(4 * wv * NT) * SH + (i * SH + cc);
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
      for (int J = 0; J < NJ; ++J) {
        const int c0 = 16 * J - kh * KH;                  // column of lane cc = 0
        if (c0 >= 0 && c0 + 15 < KH) d[4 * ii * SH + c0] = v[ii][J];
        else if (c0 + 15 >= 0 && c0 < KH) {
          const int col = c0 + (int)cc;
          if (col >= 0 && col < KH) d[4 * ii * SH + c0] = v[ii][J];
        }
      }
  };
  // One k-half of a product: KH / 4 k-steps of NIW + NJ operand reads and NIW * NJ MFMAs.  The operands of step s + 1 are
  // requested BEFORE the MFMAs of step s are issued (two register sets, ping-pong): written as "reads, wait, MFMAs" per
  // step the LDS latency of every step was exposed -- ~200 of ~450 cycles per step with one wave per SIMD, the reason a
  // 64^3 product took 10 -- 13 k cycles for 4.1 k cycles of matrix pipe (profiles/r03_k2_notes.md).
#ifndef HMV_LWR_GEMM_PIPE
#define HMV_LWR_GEMM_PIPE 1
#endif
  auto gemm_half = [&](double (&acc)[NIW][NJ]) __attribute__((always_inline)) {
    const unsigned l = lane();
    const double* xa = Xh + (unsigned)(4 * wv * NT) * SH + ((l & 3) * SH + (l >> 4));
    const double* yb = Yh + ((l & 15) * SH + (l >> 4));
#if HMV_LWR_GEMM_PIPE
    constexpr int NS = KH / 4;
    double av[2][NIW], bv[2][NJ];
    auto rd = [&](int set, int k0) __attribute__((always_inline)) {
#pragma unroll
      for (int ii = 0; ii < NIW; ++ii) av[set][ii] = xa[4 * ii * SH + k0];
#pragma unroll
      for (int J = 0; J < NJ; ++J) bv[set][J] = yb[16 * J * SH + k0];
    };
    rd(0, 0);
    static_for<NS>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value, cur = s & 1;
      if constexpr (s + 1 < NS) rd(cur ^ 1, 4 * (s + 1));
      __builtin_amdgcn_sched_barrier(0);          // the requests above stay above the MFMAs below
#pragma unroll
      for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
        for (int J = 0; J < NJ; ++J) acc[ii][J] = mfma4(av[cur][ii], bv[cur][J], acc[ii][J]);
      __builtin_amdgcn_sched_barrier(0);
    });
#else
#pragma unroll 2
    for (int k0 = 0; k0 < KH; k0 += 4) {
      double av[NIW], bv[NJ];
#pragma unroll
      for (int ii = 0; ii < NIW; ++ii) av[ii] = xa[4 * ii * SH + k0];
#pragma unroll
      for (int J = 0; J < NJ; ++J) bv[J] = yb[16 * J * SH + k0];
#pragma unroll
      for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
        for (int J = 0; J < NJ; ++J) acc[ii][J] = mfma4(av[ii], bv[J], acc[ii][J]);
    }
#endif
  };
  // acc += X' * Y'^T;  X' = srcX (global tile; transposed if trX) or, if srcX == nullptr, the register tile xr;
  // Y' = srcY (transposed if trY).  I.e. trY = false: X' Y^T, trY = true: X' Y.
  auto product = [&](double (&acc)[NIW][NJ], const double* srcX, bool trX, const double (&xr)[NIW][NJ], const double* srcY,
                     bool trY) __attribute__((always_inline)) {
    f64x2 vx[NV], vy[NV];
    if (srcX) fetch(vx, srcX, 0, trX);
    fetch(vy, srcY, 0, trY);
    __syncthreads();
    if (srcX) park(Xh, vx, trX); else park_strip(xr, 0);
    park(Yh, vy, trY);
    if (srcX) fetch(vx, srcX, 1, trX);
    fetch(vy, srcY, 1, trY);
    __syncthreads();
    gemm_half(acc);
    __syncthreads();
    if (srcX) park(Xh, vx, trX); else park_strip(xr, 1);
    park(Yh, vy, trY);
    __syncthreads();
    gemm_half(acc);
  };
  // register tile <-> global tile: the wave's strip and the ii step (4 rows) advance the scalar base, the J step (16
  // columns) is an immediate; the lane adds (i, cc)
  auto store_tile = [&](double* dst, const double (&v)[NIW][NJ]) __attribute__((always_inline)) {
    const unsigned l = lane(), off = ((l >> 4) * MP + (l & 15)) * 8u;
    const double* strip = dst + (unsigned)(4 * wv * NT) * MP;
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
      for (int J = 0; J < NJ; ++J)
        *(double __attribute__((address_space(1)))*)(gptr(strip, (4 * ii * MP + 16 * J) * 8u, off)) = v[ii][J];
  };
  // tile (or its transpose) -> this workgroup's register tile
  auto load_tile = [&](double (&v)[NIW][NJ], const double* src, bool tr) __attribute__((always_inline)) {
    const unsigned l = lane(), off = !tr ? ((l >> 4) * MP + (l & 15)) * 8u : ((l & 15) * MP + (l >> 4)) * 8u;
    const double* strip = src + (unsigned)(4 * wv * NT) * (!tr ? MP : 1);
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
      for (int J = 0; J < NJ; ++J) {
        const unsigned cb = !tr ? (4 * ii * MP + 16 * J) * 8u : (16 * J * MP + 4 * ii) * 8u;
        v[ii][J] = *reinterpret_cast<const double __attribute__((address_space(1)))*>(gptr(strip, cb, off));
      }
  };
  auto sub = [&](double (&g)[NIW][NJ], const double (&acc)[NIW][NJ]) __attribute__((always_inline)) {
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
      for (int J = 0; J < NJ; ++J) g[ii][J] -= acc[ii][J];
  };
  // inverse of the SPD register tile g -> global tile `out`; conditioning guard; optional log det
  // (AUTO: s_guard = 1 + the first order q whose inverses tripped the guard, so that the launcher's re-solve can be limited
  // to the windows whose SELECTED model went through a badly conditioned inverse)
  auto invert = [&](const double (&g)[NIW][NJ], double* out, double* logdet, int q) __attribute__((always_inline)) {
    const int info_base = q * MP;
    const int l = lane(), i = l >> 4, cc = l & 15;
    __syncthreads();
#pragma unroll
    for (int ii = 0; ii < NIW; ++ii)
#pragma unroll
      for (int J = 0; J < NJ; ++J) buf[(4 * (wv * NT + ii) + i) * SI + 16 * J + cc] = g[ii][J];
    __syncthreads();
    spd_inverse_coop<NT, SI>(buf, Pb, Nb, &s_info, s_ld, out, logdet, info_base, s_pm, a.m);
    if (threadIdx.x == 0 && !(s_pm[0] >= HMV_LWR_GUARD * s_pm[1])) {                 // also catches NaN
      if (!AUTO) s_guard = 1;
      else if (s_guard == 0) s_guard = q + 1;
    }
    __syncthreads();            // the inverse is in global memory for the whole workgroup
  };

  // both error covariances of an order inverted together (spd_inverse_coop2: their panels on different waves at the
  // same time, one barrier per block step for the two)
  auto invert2 = [&](const double (&ga)[NIW][NJ], const double (&gb)[NIW][NJ], double* out_a, double* out_b, double* logdet_b,
                     int q) __attribute__((always_inline)) {
    const int info_base = q * MP;
    spd_inverse_coop2<NT, SI>(ga, gb, buf, Pb, Nb, &s_info, s_ld, out_a, out_b, logdet_b, info_base, s_pm, a.m);
    if (threadIdx.x == 0 && (!(s_pm[0] >= HMV_LWR_GUARD * s_pm[1]) || !(s_pm[2] >= HMV_LWR_GUARD * s_pm[3]))) {
      if (!AUTO) s_guard = 1;
      else if (s_guard == 0) s_guard = q + 1;
    }
    __syncthreads();            // the inverses are in global memory for the whole workgroup
  };

  // log det Vf_q: the caller's [item][p] array, or (AUTO) the LDS word the selection reads
  auto ld_dst = [&](int q) __attribute__((always_inline)) -> double* {
    if (AUTO) return &s_logdet;
    return a.Vq_logdet + (size_t)item * p + (q - 1);
  };
  // the order-q model to the output: ar[item][e][k] = A_{k+1}[e], e = row * MP + col, k < q (lag fastest: the reference's
  // (m, m, p) layout).  Thread t takes idx = t, t + 256, ... with (e, k) = (idx / q, idx % q) carried along by the step
  // (256 / q, 256 % q): one division per thread instead of one per element.
  auto emit = [&](const double* Aq, int q) __attribute__((always_inline)) {
    double* ar = a.ar + (size_t)item * TILE * p;
    const int total = TILE * q, de = 256 / q, dk = 256 - de * q;
    int e = (int)threadIdx.x / q, k = (int)threadIdx.x - e * q;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
      ar[(size_t)e * p + k] = Aq[(size_t)k * TILE + e];
      e += de;
      k += dk;
      if (k >= q) {
        k -= q;
        ++e;
      }
    }
  };
  // AUTO: criterion of order q (mtmvar.py:551-601: log det V_q + c q m^2 / n, summed in the reference's order), first
  // arg-min by a strict <, and on every improvement the order-q model -- A^(q) in Agen[q & 1], Vf_q -- goes to the
  // outputs.  Orders are visited ascending, so a later snapshot only ever adds lags; lags >= q* are zeroed at the end.
  auto select = [&](int q) __attribute__((always_inline)) {
    if (threadIdx.x == 0) {
      const double ld = s_logdet;
      const double crit = ld + ((sel.crit_c * (double)q) * (double)(a.m * a.m)) / (double)sel.n;
      if (sel.crit_out) sel.crit_out[(size_t)item * p + (q - 1)] = crit;
      if (a.Vq_logdet) a.Vq_logdet[(size_t)item * p + (q - 1)] = ld;
      const int take = (crit < s_best) ? 1 : 0;          // NaN never wins; ties stay with the lower order (np.argmin)
      if (take) {
        s_best = crit;
        s_qstar = q;
      }
      s_take = take;
    }
    __syncthreads();
    if (s_take) {
      emit(Agen[q & 1], q);
      double* Vo = a.V + (size_t)item * TILE;
      for (int idx = threadIdx.x; idx < TILE; idx += 256) Vo[idx] = Vf[idx];
    }
  };

  double g[NIW][NJ], acc[NIW][NJ], dacc[NIW][NJ];
  const double (&none)[NIW][NJ] = g;
  // ---- order 0: Vf = Vb = C(0) = R_0 (symmetric), D_0 = C(1) = R_1^T.  With one inverse at order 0 nothing is stored for
  // them: the inverse and the Vf / Vb updates of order 0 read R_0, and Vf and Vb are first written by those updates.
  if (!ONE0) {
    load_tile(g, R, false);
    store_tile(Vf, g);
    store_tile(Vb, g);
    load_tile(g, R + TILE, true);
    store_tile(Dq, g);
  } else {
    load_tile(g, R + TILE, true);
    store_tile(Dq, g);
  }
  __syncthreads();
  for (int q = 0; q < p; ++q) {
    const double* Ao = Agen[q & 1];
    const double* Bo = Bgen[q & 1];
    double* An = Agen[(q + 1) & 1];
    double* Bn = Bgen[(q + 1) & 1];
    const bool last = (q == p - 1);
    // ---- inverses of the two error covariances of order q (log det Vf_q is the criterion's term of order q).
    // Order 0 has one (ONE0): Vf_0 = Vb_0 = R_0, so Vf_0^-1 is read from where Vb_0^-1 is written.
    const bool one0 = ONE0 && q == 0;
    load_tile(g, one0 ? R : Vb, false);
#ifndef HMV_LWR_SINGLE_INVERSES
    if (!one0 && (!last || (VQ && q >= 1))) {       // (the last order needs Vf^-1 only for its log det)
      load_tile(acc, Vf, false);
      invert2(g, acc, VbI, VfI, (VQ && q >= 1) ? ld_dst(q) : nullptr, q);
    } else {
      invert(g, VbI, nullptr, q);
    }
#else
    invert(g, VbI, nullptr, q);
    if (!one0 && (!last || (VQ && q >= 1))) {
      load_tile(g, Vf, false);
      invert(g, VfI, (VQ && q >= 1) ? ld_dst(q) : nullptr, q);
    }
#endif
    if (AUTO && q >= 1) select(q);
    // ---- A_{q+1} = D Vb^-1;  Vf <- Vf - A_{q+1} D^T
    zero(acc);
    product(acc, Dq, false, none, VbI, false);           // Vb^-1 is symmetric: X Y^T = D Vb^-1
    store_tile(An + (size_t)q * TILE, acc);
    zero(dacc);
    product(dacc, nullptr, false, acc, Dq, false);       // A_{q+1} D^T
    load_tile(g, one0 ? R : Vf, false);
    sub(g, dacc);
    store_tile(Vf, g);
    if (!last) {
      // ---- B_{q+1} = D^T Vf^-1;  Vb <- Vb - B_{q+1} D
      zero(acc);
      product(acc, Dq, true, none, one0 ? VbI : VfI, false);
      store_tile(Bn + (size_t)q * TILE, acc);
      zero(dacc);
      product(dacc, nullptr, false, acc, Dq, true);      // B_{q+1} D
      load_tile(g, one0 ? R : Vb, false);
      sub(g, dacc);
      store_tile(Vb, g);
    }
    __syncthreads();                                     // A_{q+1} / B_{q+1} are in global memory
    // ---- lower lags: A'_k = A_k - A_{q+1} B_{q-1-k},  B'_j = B_j - B_{q+1} A_{q-1-j}   (k, j = 0 .. q-1: lag k + 1)
    // and the next partial correlation D' = C(q+2) - sum_{k=0..q} A'_k C(q+1-k), C(l) = R_l^T.
    // The pair (A_k, B_{q-1-k}) is closed under the update, so iteration k takes the backward update of j = q-1-k: both
    // uses of either tile (operand of one product, seed of the other) fall inside one iteration, one or three products
    // apart, and the second finds the tile in the last-level cache instead of HBM.  Every product keeps its own sum
    // order and dacc still runs over ascending k: the same bits as the walk that indexed both updates by k.
    zero(dacc);
    for (int k = 0; k < q; ++k) {
      const int j = LEGACY ? k : q - 1 - k;             // backward lag updated in this iteration
      zero(acc);
      product(acc, An + (size_t)q * TILE, false, none, Bo + (size_t)(q - 1 - k) * TILE, true);
      load_tile(g, Ao + (size_t)k * TILE, false);
      sub(g, acc);
      store_tile(An + (size_t)k * TILE, g);
      if (!last) {
        product(dacc, nullptr, false, g, R + (size_t)(q + 1 - k) * TILE, false);       // A'_k R_{q+1-k}^T
        zero(acc);
        product(acc, Bn + (size_t)q * TILE, false, none, Ao + (size_t)(q - 1 - j) * TILE, true);
        load_tile(g, Bo + (size_t)j * TILE, false);
        sub(g, acc);
        store_tile(Bn + (size_t)j * TILE, g);
      }
    }
    if (!last) {
      product(dacc, An + (size_t)q * TILE, false, none, R + TILE, false);              // A_{q+1} R_1^T
      load_tile(g, R + (size_t)(q + 2) * TILE, true);
      sub(g, dacc);
      store_tile(Dq, g);
    }
    __syncthreads();                                     // generation q + 1 complete
  }
  if (VQ) {                                              // log det Vf_p
    load_tile(g, Vf, false);
    invert(g, VfI, ld_dst(p), p);
  }
  if (AUTO) {
    select(p);
    // ---- outputs of the selecting form: the snapshots above are the model; here the order, the failure and the guard.
    // A non-positive pivot at ANY order <= p fails the window (order 0, zero coefficients, V = R_0).
    __syncthreads();
    const int bad = s_info, qs = bad ? 0 : s_qstar;
    if (threadIdx.x == 0) {
      a.info[item] = bad ? bad : (qs == 0 ? -1 : 0);    // (no finite criterion without a bad pivot: cannot happen, but say so)
      sel.order_out[item] = qs;
      *yw_guard_ptr(a.ws, item, p, TILE) = (bad == 0 && qs > 0 && s_guard != 0 && s_guard - 1 <= qs) ? 1 : 0;
    }
    double* ar = a.ar + (size_t)item * TILE * p;
    const int total = TILE * p, dk = 256 % p;
    int k = (int)threadIdx.x % p;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
      if (k >= qs) ar[idx] = 0.0;
      k += dk;
      k = (k >= p) ? k - p : k;
    }
    if (qs == 0) {
      double* Vo = a.V + (size_t)item * TILE;
      for (int idx = threadIdx.x; idx < TILE; idx += 256) Vo[idx] = R[idx];
    }
    return;
  }
  // ---- outputs: V = Vf_p and the order-p model
  load_tile(g, Vf, false);
  store_tile(a.V + (size_t)item * TILE, g);
  if (threadIdx.x == 0) {
    a.info[item] = s_info;
    // (a singular window stays singular: nothing to re-solve)
    *yw_guard_ptr(a.ws, item, p, TILE) = (s_info == 0) ? s_guard : 0;
  }
  // (no_emit: the fused path's packing kernel reads the final generation's tiles where they are)
  if (LEGACY || !a.no_emit) emit(Agen[p & 1], p);
}

}  // namespace hmv
