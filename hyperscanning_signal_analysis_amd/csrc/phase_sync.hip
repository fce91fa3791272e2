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
#include "hmv_common.h"
#include "hmv_kernels.h"
#include "lagcov_core.h"
#include <cmath>

namespace hmv {

template <int NT>
__global__ void __launch_bounds__(256, 2) phase_gram_kernel(PhaseSyncArgs a) {
  constexpr int MP = 16 * NT, PLANE = MP * k1::S2, CS = MP + 1;
  static_assert(MP * CS <= PLANE, "the epilogue's two images of C fit the two staging planes");
  __shared__ double xs[2 * PLANE];
  const int l = lane_id();
  const int wv = uni(threadIdx.x >> 6);
  const long long item = blockIdx.x;
  const int n = a.n, m = a.m;
  const bool unit = a.mode == 0;
  const long long rec = a.item_rec[item], start = a.item_start[item];
  // samples with a value; a window the caller let reach outside its recording reads zeros there, never memory
  const bool inside = rec >= 0 && rec < a.n_rec && start >= 0 && start < a.T;
  const long long vlen = inside ? min((long long)n, a.T - start) : 0;
  const double2* z = inside ? a.z + rec * a.rec_stride + start : a.z;

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
      if (ch < m && t < vlen) {
        v = z[(size_t)ch * a.ld + t];
        if (unit) {                                        // z / |z|; exact under a power-of-two scaling of z
          const double r = sqrt(v.x * v.x + v.y * v.y);
          if (r == 0.0) v = make_double2(0.0, 0.0);
          else v = make_double2(v.x / r, v.y / r);         // a non-finite sample leaves a NaN here and on the diagonal of C
        }
      }
      return v;
    });
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
  __syncthreads();

  // the item's flags off the diagonal of C, in every wave alike
  const double dl = l < m ? cre[l * CS + l] : 1.0;
  const bool bad = __ballot(!__builtin_isfinite(dl)) != 0;
  const bool dead = !unit && __ballot(dl == 0.0) != 0;
  if (threadIdx.x == 0) a.info[item] = bad ? 1 : dead ? 2 : 0;

  const double nan = __builtin_nan("");
  const double nn = (double)n;
  const size_t mm = (size_t)m * m;
  double* oc = a.coherency ? a.coherency + (size_t)item * 2 * mm : nullptr;
  double* om = a.mag ? a.mag + (size_t)item * mm : nullptr;
  double* ol = a.lagged ? a.lagged + (size_t)item * mm : nullptr;
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
    if (r > c) rim = -rim;
    if (oc) { oc[e] = rre; oc[mm + e] = rim; }
    if (om) om[e] = mg;
    if (ol) ol[e] = lg;
  }
}

int launch_phase_sync(const PhaseSyncArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  const dim3 grid((unsigned)a.n_items), block(256);
  if (k1::for_nt(m_pad, [&](auto nt) { hipLaunchKernelGGL(phase_gram_kernel<decltype(nt)::value>, grid, block, 0, st, a); }))
    return -1;
  return (int)hipGetLastError();
}

}  // namespace hmv
