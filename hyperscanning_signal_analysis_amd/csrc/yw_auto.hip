// K2 with the model order chosen on the device, window by window.
//
// Replaces `mvar_criterion` (the reference's src/mtmvar.py:551-601) followed by `ar_coeff` at the order it returns
// (mtmvar.py:90-123) -- what every connectivity function of the reference does when it is called with
// `optimal_model_order=None` -- for every window of a batch in ONE pass.  The reference fits every order 1..pmax from
// scratch and takes the first arg-min of
//     crit_q = log det V_q + c q m^2 / n          c = 2 (AIC),  2 log log n (HQ),  log n (SC).
// The block Levinson-Whittle recursion (yw_lwr_core.h, described in yw_lwr.hip) holds the complete order-q model on its
// way to order pmax -- A_k^(q) in one generation of its coefficient scratch, Vf_q, and log det Vf_q from the inverse of
// Vf_q that the step to order q + 1 needs anyway -- and the lag covariances do not depend on the order, so the order-q
// Yule-Walker system is the leading part of the order-pmax one.  This kernel is that recursion (the same device function,
// instantiated with AUTO) plus three things, all done as soon as log det Vf_q is known:
//   * criterion: thread 0 forms crit_q in the reference's order of operations (m: the unpadded channel count; the padded
//     channels of the MP layout carry an identity block in R_0, hence unit pivots and log 1 = 0 in every log det);
//   * first arg-min: the smallest criterion so far is kept with a strict <, so ties go to the lower order (np.argmin), and
//     a NaN never wins;
//   * snapshot: on every strict improvement the order-q model is copied from the scratch to the outputs,
//     ar[item][MP][MP][pmax] (lag fastest, lags < q) and V[item] = Vf_q.  Orders are visited ascending, so a later snapshot
//     only adds lags; after the last order the lags >= q* are written as +0.0 and order_out[item] = q*.
// The criterion usually falls to its minimum and rises again, so a window takes about q* snapshots of 1 .. q* tiles:
// ~q* (q* + 1) / 2 tile copies beside the several hundred tile moves of the recursion.  (The alternative -- one recursion
// for the criterion, a second one that stops at order[item] -- walks orders 1..q* twice and was not built: see DESIGN.md.)
//
// Failure: a non-positive pivot at ANY order <= pmax fails the window: info[item] != 0, order_out[item] = 0, zero
// coefficients, V = R_0.  (The reference takes the log of a non-positive determinant there, gets NaN, and np.argmin
// returns that index; that is not reproduced -- INTEGRATION.md section 4.)
//
// Conditioning guard: the recursion records the first order whose tile inverses met min / max pivot < HMV_LWR_GUARD.  A
// window whose selected order is at or beyond it is re-solved by the one-launch block-LDL^T kernel (yw_solve.hip) AT ITS
// OWN ORDER, read from order_out on the device: no host round trip, and the selected order stays the recursion's choice.
#include "yw_lwr_core.h"

namespace hmv {

template <int NT, bool LEGACY = false>
__global__ void __launch_bounds__(256, 3) yw_auto_kernel(YwArgs a, YwAutoArgs sel) {
  yw_lwr_body<NT, true, true, LEGACY>(a, sel);
}

int launch_yw_auto(const YwArgs& a_in, const YwAutoArgs& sel, int m_pad, hipStream_t st) {
  YwArgs a = a_in;
  if (a.n_items == 0) return 0;
  a.order = nullptr;
  a.only_guarded = 0;
  a.no_emit = 0;                              // (the selecting form always writes its snapshots)
  const dim3 grid((unsigned)a.n_items), block(256);
  const bool legacy = tuning(4 /* HMV_TUNE_YW_FORM */) == 4;      // the walk kept for the tests (LEGACY in yw_lwr_core.h)
  if (for_nt(m_pad, legacy, [&](auto nt, auto leg) {
        hipLaunchKernelGGL((yw_auto_kernel<nt, leg>), grid, block, 0, st, a, sel);
      }))
    return -1;
  if (const int rc = (int)hipGetLastError()) return rc;
  // the flagged windows again, by the LDL^T of the first order_out[item] + 1 lag blocks (normally none: every other
  // workgroup of this launch reads one int and exits)
  a.order = sel.order_out;
  return launch_yw_guarded(a, m_pad, st);
}

}  // namespace hmv
