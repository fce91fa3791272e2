// K2, second form -- block Levinson-Whittle recursion on the p + 1 lag blocks (Whittle 1963; Wiggins & Robinson 1965).
//
// Replaces `ar_coeff` (/root/reference/src/mtmvar.py:90-123) like yw_solve.hip, but uses what that solver ignores: the
// normal-equation matrix is block-TOEPLITZ.  With C(l) = R_l^T (l >= 0), C(-l) = R_l, the Yule-Walker equations read
//     sum_{k=1..q} A_k^(q) C(l - k) = C(l),  l = 1..q            (forward predictor of order q, error covariance Vf_q)
//     sum_{k=1..q} B_k^(q) C(k - l) = C(-l), l = 1..q            (backward predictor, error covariance Vb_q)
// and order q + 1 follows from order q with the partial correlation D_q = C(q+1) - sum_k A_k^(q) C(q+1-k):
//     A_{q+1}^(q+1) = D_q Vb_q^-1            B_{q+1}^(q+1) = D_q^T Vf_q^-1
//     A_k^(q+1) = A_k^(q) - A_{q+1}^(q+1) B_{q+1-k}^(q)        B_k^(q+1) = B_k^(q) - B_{q+1}^(q+1) A_{q+1-k}^(q)
//     Vf_{q+1} = Vf_q - A_{q+1}^(q+1) D_q^T                    Vb_{q+1} = Vb_q - B_{q+1}^(q+1) D_q
// ar[:, :, k] = A_{k+1}^(p), V = Vf_p, and the Vf_q of every lower order (the model-order criterion,
// mtmvar.py:551-601) come out on the way.  Per window: 115 tile products and 16 tile inverses at p = 8 against 184 + 8
// for the block LDL^T, and the state is 2p coefficient tiles instead of a (p+1)(p+2)/2-tile factor.  Tile moves per
// window at p = 8, counted from the loop structure: 367 (265 reads, 102 writes) with the model
// left in its tiles, 383 with it emitted; 388 (275 + 113) for the walk kept as form 4.  The LDL^T form moves ~360 and
// does 184 + 8 products and inverses for them.
//
// Numerics.  Levinson-type recursions are only weakly stable: the error grows with the condition of the lag-0 blocks'
// Schur complements (Vf_q, Vb_q), where the LDL^T of the whole Gram matrix loses cond * eps.  Measured against the
// reference's dgesv on the nearly collinear fixtures (tests/golden/g6_errors.npz): 3e-11 at cond 2e5 (LDL^T 3e-12),
// 4e-5 at cond 2e9 (2e-8).  Hence the guard: every tile inverse reports its smallest and largest pivot, and a window
// in which any inverse met min / max < HMV_LWR_GUARD is flagged in `guard[item]`; the launcher then re-solves exactly
// the flagged windows with the LDL^T kernel (one more launch whose other workgroups exit at once).  Well-conditioned
// windows (every window of the synthetic benchmark; cond ~ 1e4) never take that path.
// The ratio is taken over the pivots of the REAL channels only (yw_common.h): the padded channels' pivots are K1's unit
// diagonal, and with them in, a 19-channel recording in volts (variance 1e-10) or in ADC counts (1e8) had every window
// flagged.  Nothing in the recursion or in the tile inverse holds an absolute constant: samples times 2**k give the same
// coefficient bits, V times 4**k and the same guard decision (tests/test_gpu_amplitude.py).
//
// What the LDL^T delivers where it is the fallback (tests/test_gpu_high_order.py prints it; well-conditioned windows, cond
// 6e3 .. 8e4, against the oracle's dense solve): 5e-11 at p = 9, 2e-9 at p = 12, 6e-7 at p = 16, 1e-7 at p = 17, 5e-7 at
// p = 20, 2e-3 at p = 24 and 2e-1 at p = 32, where this recursion stays at ~1e-12 at every order up to 32.  Beyond p ~ 20 a
// guarded window therefore comes back OUTSIDE the 1e-5 contract.
//
// One workgroup of four waves per window walks the whole recursion in ONE launch; the tile products are the same
// MFMA kernel body as yw_solve.hip (operands staged through LDS in two k-halves, 39 KB, three workgroups per CU).
#include "yw_lwr_core.h"

namespace hmv {

template <int NT, bool VQ, bool LEGACY = false>
__global__ void __launch_bounds__(256, 3) yw_lwr_kernel(YwArgs a) {
  yw_lwr_body<NT, VQ, false, LEGACY>(a, YwAutoArgs{});        // the recursion itself: yw_lwr_core.h
}

// HMV_TUNE_YW_FORM = 4: the walk before the lower-lag updates were paired (LEGACY in yw_lwr_core.h), same bits; the
// tests hold the default walk against it
static int launch_yw_lwr_legacy(const YwArgs& a, int m_pad, hipStream_t st) {
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, a.Vq_logdet != nullptr, [&](auto nt, auto vq) {
        hipLaunchKernelGGL((yw_lwr_kernel<nt, vq, true>), grid, block, 0, st, a);
      }))
    return -1;
  return (int)hipGetLastError();
}

// HMV_TUNE_YW_FORM = 3 takes the software-pipelined form of the same recursion (yw_lwr2.hip): measured equal in time
// (1.73 vs 1.74 ms at 599 windows) and 4 % lower in HBM traffic -- see profiles/r03_k2_notes.md -- so this one stays
int launch_yw_lwr(const YwArgs& a, int m_pad, hipStream_t st) {
  if (a.n_items == 0) return 0;
  if (tuning(4 /* HMV_TUNE_YW_FORM */) == 3) return launch_yw_lwr2(a, m_pad, st);
  if (tuning(4) == 4) return launch_yw_lwr_legacy(a, m_pad, st);
  const dim3 grid((unsigned)a.n_items), block(256);
  if (for_nt(m_pad, a.Vq_logdet != nullptr, [&](auto nt, auto vq) {
        hipLaunchKernelGGL((yw_lwr_kernel<nt, vq>), grid, block, 0, st, a);
      }))
    return -1;
  return (int)hipGetLastError();
}

// Windows of the default form that one compute unit holds at once, asked of the runtime (registers and LDS of the build in
// use decide it, not a constant here); the sliding step sizes its K2 -> K3 hand-over by it (capi.hip, k3_split_point, for sliding_k2).  0: not known.
int yw_lwr_occupancy(int m_pad) {
  if (tuning(4 /* HMV_TUNE_YW_FORM */) == 3 || tuning(4) == 4) return 0;
  int occ = 0;
  hipError_t e = hipErrorInvalidValue;
  if (for_nt(m_pad, [&](auto nt) { e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, yw_lwr_kernel<nt, false>, 256, 0); }))
    return 0;
  return (e == hipSuccess && occ > 0) ? occ : 0;
}

}  // namespace hmv
