// Phase synchrony of analytic signals per window: the Hermitian Gram matrix C = U U^H of the window's m x n complex block
// and what is read off it -- PLV and ciPLV of the unit phasors, coherence and imaginary coherence of the signal itself.
//
// K1's direct form at lag 0 with two planes (lagcov_core.h, "two planes"): one workgroup = one item, the window streamed
// through LDS in chunks of 64 samples as a re and an im plane, four v_mfma_f64_4x4x4_4b_f64 per tile and k-step
//     Re C += re_i re_j + im_i im_j        Im C += im_i re_j - re_i im_j   (the subtraction by the MFMA's NEG bit),
// every accumulator summed over the samples ascending in k-steps of 4 from the window start: an item's bits depend on its
// own samples only.  torch's interleaved complex128 is read as it lies (one 16-byte load per sample) and, in UNIT mode,
// normalised to the unit phasor between the load and the LDS store, so no packed copy of the signal exists.
//
// Only the tiles on or above the diagonal are computed (10 of 16 at 64 channels, the same in every wave); the epilogue
// passes C through LDS -- the planes' own memory -- and every output element (r, c) is formed from C[min][max], so mag and
// lagged are symmetric and Im R antisymmetric bit for bit, and the RAW mode finds C_ii and C_jj there.
//
// The pairs form (PAIRS) serves the null tests of the inter-brain cells: participant B's rows come from another place than
// participant A's -- the same recording read shift_b samples later modulo T (the analytic signal is a circular filter, so
// that is the shift surrogate), or another recording (the pseudo dyad) -- and only the tiles that hold a cross cell are
// computed, straight into the value columns hmv_null_accumulate_f64 reads.
#include "hmv_common.h"
#include "hmv_kernels.h"
#include "lagcov_core.h"
#include <cmath>

namespace hmv {

// One body for both forms.  PAIRS = false (PhaseSyncArgs): the item is one window of one recording, every tile on or above
// the diagonal, three optional outputs.  PAIRS = true (PhasePairsArgs): the channels < split are read from recording rec_a
// at item_start, the channels >= split from recording rec_b at (item_start + shift_b + t) mod T; only the tiles that hold a
// cross element (k1::herm_need; RAW mode: also the diagonal tiles, for C_ii) are computed, with the products of the full form
// in its order, so a cross cell has the bits the full form gives for the same window written out as one recording.
template <int NT, bool PAIRS = false>
__global__ void __launch_bounds__(256, 2) phase_gram_kernel(std::conditional_t<PAIRS, PhasePairsArgs, PhaseSyncArgs> a) {
  constexpr int MP = 16 * NT, PLANE = MP * k1::S2, CS = MP + 1;
  static_assert(MP * CS <= PLANE, "the epilogue's two images of C fit the two staging planes");
  static_assert(!PAIRS || k1::TC == 64, "the pairs source takes a staged row's channel from the wave's first lane");
  __shared__ double xs[2 * PLANE];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int n = a.n, m = a.m;
  const bool unit = a.mode == 0;
  // samples with a value; a window the caller let reach outside its recording reads zeros there, never memory
  long long vlen = 0, sb = 0;            // PAIRS: sb = where B's window starts, in 0..T-1
  bool in_a = false, in_b = false;
  const double2* z = a.z;
  const double2* zb = a.z;
  int split = 0, nf = 0;                 // PAIRS: nf = this thread staged a non-finite value
  unsigned need = 0;
  if constexpr (PAIRS) {
    const long long ra = a.rec_a[item], rb = a.rec_b[item], start = a.item_start[item], sh = a.shift_b ? a.shift_b[item] : 0;
    const bool in_t = start >= 0 && start <= a.T - n;                     // the entry refuses n > T
    in_a = in_t && ra >= 0 && ra < a.n_rec;
    in_b = in_t && rb >= 0 && rb < a.n_rec && sh >= 0 && sh < a.T;
    if (in_a) z = a.z + ra * a.rec_stride + start;
    if (in_b) {
      zb = a.z + rb * a.rec_stride;
      sb = start + sh >= a.T ? start + sh - a.T : start + sh;
    }
    split = a.split;
    need = k1::herm_need<NT>(split, !unit);
  } else {
    const long long rec = a.item_rec[item], start = a.item_start[item];
    const bool inside = rec >= 0 && rec < a.n_rec && start >= 0 && start < a.T;
    vlen = inside ? min((long long)n, a.T - start) : 0;
    z = inside ? a.z + rec * a.rec_stride + start : a.z;
  }

  double re[NT][NT], im[NT][NT];
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int J = 0; J < NT; ++J) re[I][J] = im[I][J] = 0.0;
  double* xre = xs;
  double* xim = xs + PLANE;
  for (int t0 = 0; t0 < n; t0 += k1::TC) {
    k1::stage_chunk2<NT>(xre, xim, t0, [&](int ch, int t) __attribute__((always_inline)) {
      double2 v = make_double2(0.0, 0.0);
      bool have;
      if constexpr (PAIRS) {                               // a wave stages whole rows (TC = its 64 lanes): the row, its side of
        ch = uni(ch);                                      // split and its base address are scalars
        have = ch < m && (ch < split ? in_a : in_b) && t < n;
      } else {
        have = ch < m && t < vlen;
      }
      if (have) {
        if constexpr (PAIRS) {
          const long long tb = sb + t;                     // sb + t < 2 T: the wrap is one subtraction
          const double2* row = (ch < split ? z : zb) + (size_t)ch * a.ld;
          v = row[ch < split ? (long long)t : tb >= a.T ? tb - a.T : tb];
        } else {
          v = z[(size_t)ch * a.ld + t];
        }
        if (unit) {                                        // z / |z|; exact under a power-of-two scaling of z
          const double r = sqrt(v.x * v.x + v.y * v.y);
          if (r == 0.0) v = make_double2(0.0, 0.0);
          else v = make_double2(v.x / r, v.y / r);         // a non-finite sample leaves a NaN here and on the diagonal of C
        }
        if constexpr (PAIRS) nf |= !(__builtin_isfinite(v.x) && __builtin_isfinite(v.y));
      }
      return v;
    });
    if constexpr (PAIRS)
      k1::ksteps_herm<NT, true>(k1::a_operand2(xre, wv, l), k1::b_operand2(xre, l), PLANE, min(k1::TC, n - t0 + 3) >> 2, re, im,
                                need);
    else
      k1::ksteps_herm<NT>(k1::a_operand2(xre, wv, l), k1::b_operand2(xre, l), PLANE, min(k1::TC, n - t0 + 3) >> 2, re, im);
  }

  // C[row][col] for col's tile on or above row's, through LDS
  __syncthreads();
  double* cre = xs;
  double* cim = xs + MP * CS;
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int J = I; J < NT; ++J) {
      const int row = 16 * I + 4 * wv + (l >> 4), col = 16 * J + (l & 15);
      cre[row * CS + col] = re[I][J];
      cim[row * CS + col] = im[I][J];
    }
  // the item's flags, in every wave alike: off the diagonal of C, which the pairs form has in RAW mode only -- in UNIT mode
  // it takes them from the staged phasors (a phasor is non-finite exactly where it makes its channel's C_ii non-finite)
  bool bad, dead;
  if (PAIRS && unit) {
    bad = __syncthreads_or(nf) != 0;
    dead = false;
  } else {
    __syncthreads();
    const double dl = l < m ? cre[l * CS + l] : 1.0;
    bad = __ballot(!__builtin_isfinite(dl)) != 0;
    dead = !unit && __ballot(dl == 0.0) != 0;
  }
  if (threadIdx.x == 0) a.info[item] = bad ? 1 : dead ? 2 : 0;

  const double nan = __builtin_nan("");
  const double nn = (double)n;
  const size_t mm = (size_t)m * m;
  double* oc = nullptr;
  double* om = nullptr;
  double* ol = nullptr;
  if constexpr (PAIRS) {                                   // columns of the item's [m][m][val_stride] cells
    if (a.col_mag >= 0) om = a.values + (size_t)item * mm * a.val_stride + a.col_mag;
    if (a.col_lagged >= 0) ol = a.values + (size_t)item * mm * a.val_stride + a.col_lagged;
  } else {
    oc = a.coherency ? a.coherency + (size_t)item * 2 * mm : nullptr;
    om = a.mag ? a.mag + (size_t)item * mm : nullptr;
    ol = a.lagged ? a.lagged + (size_t)item * mm : nullptr;
  }
  for (int e = threadIdx.x; e < m * m; e += 256) {
    const int r = e / m, c = e - r * m;
    const int i = min(r, c), j = max(r, c);
    const double di = cre[i * CS + i], dj = cre[j * CS + j];
    double rre, rim, mg, lg;
    if (unit) {
      rre = cre[i * CS + j] / nn;
      rim = i == j ? 0.0 : cim[i * CS + j] / nn;
      mg = sqrt(rre * rre + rim * rim);
      const double den = 1.0 - rre * rre;
      lg = den > 0.0 ? fmin(1.0, fabs(rim) / sqrt(den)) : 0.0;
    } else {
      const double s = sqrt(di * dj);
      rre = cre[i * CS + j] / s;
      rim = i == j ? 0.0 : cim[i * CS + j] / s;
      mg = sqrt(rre * rre + rim * rim);
      lg = fabs(rim);
    }
    if (i == j && di > 0.0) { mg = 1.0; lg = 0.0; }
    if (bad || (!unit && (di == 0.0 || dj == 0.0))) rre = rim = mg = lg = nan;
    if constexpr (PAIRS) {                                 // an untested cell (both indices on one side of split) is NaN
      if (!(i < split && j >= split)) mg = lg = nan;
      const size_t vs = (size_t)a.val_stride;
      if (om) om[e * vs] = mg;
      if (ol) ol[e * vs] = lg;
    } else {
      if (r > c) rim = -rim;
      if (oc) { oc[e] = rre; oc[mm + e] = rim; }
      if (om) om[e] = mg;
      if (ol) ol[e] = lg;
    }
  }
}

int launch_phase_sync(const PhaseSyncArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(phase_gram_kernel<decltype(nt)::value>, grid, block, 0, st, a); }))
    return -1;
  return (int)hipGetLastError();
}

int launch_phase_sync_pairs(const PhasePairsArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, [&](auto nt) {
        hipLaunchKernelGGL((phase_gram_kernel<decltype(nt)::value, true>), grid, block, 0, st, a);
      }))
    return -1;
  return (int)hipGetLastError();
}

}  // namespace hmv
