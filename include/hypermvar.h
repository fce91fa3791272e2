/* hypermvar -- C ABI of the MI355X (gfx950) sliding-window MVAR / ffDTF engine.
 *
 * This is the drop-in boundary for the hot path of the reference project
 * (SYNCC-IN/hyperscanning-signal-analysis, src/mtmvar.py:35-284, 551-601).  The reference is pure
 * Python/NumPy and has no FFI of its own; the "operator API" it exposes is the set of Python function
 * signatures in src/mtmvar.py.  Each entry point below names the reference function whose arithmetic it
 * replaces; `INTEGRATION.md` shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch-ROCm `tensor.data_ptr()`), float64 unless noted;
 *   - buffers are caller-allocated and caller-owned; the library never allocates, frees or retains them;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 = launched, < 0 = bad argument (see hmv_last_error()), > 0 = hipError_t;
 *   - numerical failures are reported per item through `info` arrays (LAPACK style: 0 = ok,
 *     k > 0 = zero / non-positive pivot met at column k); the Python layer turns them into
 *     numpy.linalg.LinAlgError("Singular matrix") like the reference's np.linalg.solve / inv;
 *   - channel counts are padded to MP = hmv_pad(m) = 16*ceil(m/16) <= 64 inside the library's
 *     intermediate buffers ("MP layout"); user-facing outputs are unpadded.
 */
#ifndef HYPERMVAR_H
#define HYPERMVAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMV_VERSION 160            /* 0.1.6 */
#define HMV_MAX_CHANNELS 64
#define HMV_MAX_ORDER 32

int hmv_version(void);
/* Thread-local text of the last argument error reported by this thread ("" if none). */
const char* hmv_last_error(void);
/* Padded channel count used by the MP-layout buffers, or -1 if m is unsupported (m < 1 or m > 64). */
int hmv_pad(int m);
/* Tuning knobs (process-wide; never needed for correct results -- every setting gives the same numbers up to the
 * documented bit-identity classes).  They replace the environment variables that earlier builds read inside the
 * launch path: the environment is looked at ONCE, when the library is loaded (HYPERMVAR_NORM_LAG,
 * HYPERMVAR_LAG_GROUP, HYPERMVAR_K3_FORM, HYPERMVAR_YW_FORM, HYPERMVAR_K3_SPLIT), and hmv_set_tuning overrides it afterwards.
 *   HMV_TUNE_NORM_LAG   windows between a K3 workgroup and the window whose rows it normalises (0 = built-in rule, >= 8)
 *   HMV_TUNE_LAG_GROUP  lags per K1 workgroup (1..3; 0 = default 3)
 *   HMV_TUNE_K3_FORM    0 = default, 1 = compiler-scheduled K3 body, 2 = hand-scheduled 64-channel K3 body
 *   HMV_TUNE_YW_FORM    0 = default, 1 = block LDL^T of the augmented matrix, 2 = block Levinson-Whittle recursion,
 *                       3 = the same recursion as a software pipeline (yw_lwr2.hip; equal in time, measurement form),
 *                       4 = the recursion with its lower-lag updates unpaired, two inverses at order 0 and the model
 *                       always emitted (same bits; the form the tests hold the default against),
 *                       5 = the dense LU with partial pivoting (yw_lu.hip) alone, for every window: a measurement and test
 *                       form of the fallback that HMV_FLAG_YW_PIVOTED puts behind the other solvers (not the same bits)
 *   HMV_TUNE_K3_LDS_PAD bytes of unused dynamic LDS added to every K3 workgroup (measurement only: fewer resident
 *                       workgroups per CU, to separate latency from throughput; 0 = none)
 *   HMV_TUNE_K3_SPLIT   the fused ffDTF calls with a second stream: where a chunk's K2 -> K3 hand-over is split, so that K3
 *                       starts on the chunk's first windows while K2 finishes the rest on the second stream.  0 = by rule
 *                       (the windows past the last full round of one K2 workgroup per compute unit; or, where the chunk's
 *                       K1 can be cut at the same point -- single windows or a regular grid inside one recording -- and
 *                       the chunk is more than one such round, after the first round, with the rest of K1 and K2's second
 *                       part on the second stream from there), -1 = never, n > 0 = after the chunk's first n windows,
 *                       K1 cut there too where it can be, HMV_K3_SPLIT_NO_FRONT + n = n (0 included) with K1 never cut:
 *                       the sequence of builds before the cut existed (same bits at every setting)
 * Returns 0, or -1 for an unknown key / value out of range.  hmv_get_tuning returns the value in force (-1: unknown key). */
#define HMV_TUNE_NORM_LAG 1
#define HMV_TUNE_LAG_GROUP 2
#define HMV_TUNE_K3_FORM 3
#define HMV_TUNE_YW_FORM 4
#define HMV_TUNE_K3_LDS_PAD 5
#define HMV_TUNE_K3_SPLIT 6
#define HMV_K3_SPLIT_NO_FRONT (1 << 19)
int hmv_set_tuning(int key, int64_t value);
int64_t hmv_get_tuning(int key);
/* Number of doubles of K2 scratch per item. */
int64_t hmv_yw_workspace_doubles(int m, int p);

/* K1.  R[item][l][MP][MP] = (1/n) X[:, :n-l] X[:, l:]^T for l = 0..p  (biased, not demeaned).
 * Replaces count_corr (src/mtmvar.py:35-87; lags :57-59, lag 0 :72-73).
 * x: [n_rec][m][ld-strided samples]; window `it` covers samples item_start[it] .. +n of recording
 * item_rec[it] (int64 device arrays -- arbitrary starts, as produced by
 * EEG_IBI_FFDTF_Pipeline._create_windows, src/eeg_alpha_ibi_ffdtf.py:451-518). */
int hmv_lagcov_f64(const double* x, int64_t rec_stride, int64_t ld,
                   const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                   int m, int n, int p, double* R, void* stream);

/* K1 for a REGULAR grid of overlapping windows of one recording: window w covers samples first + w*hop .. + n with
 * n a whole number k of hops (50 % overlap: k = 2).  Every product x_i[t] x_j[t+l] then belongs to up to k windows;
 * the hop blocks are summed once and the windows assembled from the block sums (minus the l products per lag that
 * reach past a window's end): half the flops of hmv_lagcov_f64 at 50 % overlap.  Same estimator (count_corr,
 * src/mtmvar.py:57-59, 72-73: biased 1/n, no demeaning) with the sums associated differently -- equal to
 * hmv_lagcov_f64 to rounding (~1e-16 relative), not bitwise.  x: [m][ld] (ONE recording of T samples), R:
 * [n_win][p+1][MP][MP], workspace: hmv_lagcov_regular_workspace_doubles(n_win, m, n, hop, p) doubles. */
#define HMV_MAX_HOPS_PER_WINDOW 8
int64_t hmv_lagcov_regular_workspace_doubles(int64_t n_win, int m, int n, int64_t hop, int p);
int hmv_lagcov_regular_f64(const double* x, int64_t ld, int64_t T, int64_t first, int64_t hop, int64_t n_win,
                           int m, int n, int p, double* R, double* workspace, void* stream);

/* K2.  Yule-Walker solve.  Replaces ar_coeff (src/mtmvar.py:90-123).
 * ar: [item][MP][MP][p] with ar[i][j][k] multiplying x_j(t-k-1) into x_i(t) (lag fastest: the
 * reference's own (m, m, p) layout when m == MP); V: [item][MP][MP] residual covariance.
 * vq_logdet (optional, may be NULL): [item][p] = log det V_q for model orders q = 1..p, all from the one
 * factorisation at order p (what mvar_criterion, src/mtmvar.py:551-601, gets from p separate fits).
 * flags: 0, HMV_FLAG_YW_TILED or HMV_FLAG_YW_ONE_LAUNCH (below), each optionally with HMV_FLAG_YW_PIVOTED.
 * The solvers are unpivoted (the normal equations are a Gram matrix): info != 0 reports a pivot that rounding made
 * non-positive, which happens from cond ~ 1e13 on.  With HMV_FLAG_YW_PIVOTED those windows are solved again by a dense LU
 * with partial pivoting (LAPACK's rule; what the reference's np.linalg.solve does): ar, V and info are overwritten, info
 * becomes 0, or c + 1 for an exactly zero pivot column c (dgesv's info > 0; ar and V are NaN then).  It promises what LU
 * promises -- a backward-stable solution -- not coefficient parity where cond(G) eps >~ 1.  Refused with -6 together with
 * vq_logdet (an LU gives no criterion curve).  Every window's route is left in the last int of its scratch:
 * hmv_yw_routes_i32 copies them out, route[item] = 0 recursion, 1 LDL^T, 2 LU (device pointers, same m and p). */
int hmv_yw_routes_i32(const double* ws, int64_t n_items, int m, int p, int32_t* route, void* stream);
int hmv_yw_solve_f64(const double* R, int64_t n_items, int m, int p, double* ws,
                     double* ar, double* V, double* vq_logdet, int32_t* info, int64_t flags, void* stream);

/* tw[f][k] = exp(-(k+1) * 2*pi*1j * freqs[f] / fs) as interleaved (re, im), k = 0..p-1
 * (src/mtmvar.py:151-153, same operation order). */
int hmv_twiddles_f64(const double* freqs, int F, double fs, int p, double* tw, void* stream);

/* K3.  A(f) = I - sum_k ar[:, :, k] tw[f][k];  H(f) = inv(A(f)).
 * Replaces mvar_transfer_function (src/mtmvar.py:126-162) and the |H|^2 of dtf_multivariate (:232).
 * Optional outputs (NULL to skip), kernel-natural layout [item][f][MP][MP]:
 *   P = |H|^2 with rowsum[item][f][MP] = sum_j |H_ij|^2 (required together), H, A (complex128 interleaved).
 * pivot_tau: 1.0 = partial pivoting on |re|+|im| (LAPACK zgetrf's choice); 0 < tau < 1 keeps the diagonal
 * pivot whenever it is within a factor tau of the column maximum.  info: [item*F + f].
 * ws: caller-owned scratch of hmv_tf_workspace_doubles(n_items, m, p) doubles (the coefficients re-ordered
 * once per item so that every per-frequency read is fully coalesced). */
int64_t hmv_tf_workspace_doubles(int64_t n_items, int m, int p);
int hmv_tf_f64(const double* ar, int64_t n_items, int m, int p, const double* tw, int F,
               double* P, double* rowsum, double* H, double* A, int32_t* info,
               double pivot_tau, double* ws, void* stream);

/* K4.  out[item][i][j][f] = P[item][f][i][j] / sum_{j',f'} P[item][f'][i][j']   (normalise = 1)
 * Replaces the normalisation loop of full_freq_dtf (src/mtmvar.py:281-283); normalise = 0 returns the
 * plain |H|^2 of dtf_multivariate in the reference's (m, m, F) layout.  den: [item][MP] scratch/out. */
int hmv_ffdtf_norm_f64(const double* P, const double* rowsum, double* den, double* out,
                       int64_t n_items, int F, int m, int normalise, void* stream);

/* complex128 [item][f][MP][MP] -> [item][m][m][F] (the reference's H / A / spectra array layout). */
int hmv_transpose_c128(const double* in, double* out, int64_t n_items, int F, int m, void* stream);

/* K5.  S[item][f] = H V H^T, plain transpose (src/mtmvar.py:199).  H, S complex128 [item][f][MP][MP]. */
int hmv_spectra_f64(const double* H, const double* V, double* S, int64_t n_items, int m, int F, void* stream);
/* The same product written by the kernel itself in the reference's array layout, complex128 [item][m][m][F] (what
 * multivariate_spectra returns, src/mtmvar.py:165-201) -- no separate hmv_transpose_c128 pass over S. */
int hmv_spectra_mmf_f64(const double* H, const double* V, double* S, int64_t n_items, int m, int F, void* stream);

/* ---- measures on top of the per-frequency matrices ----------------------------
 * hmv_pack_c128: complex (items, m, m, F) -- the reference's array layout -- to the kernel layout
 *   [item][f][MP][MP] with the identity on the padding (inverse of hmv_transpose_c128).
 * hmv_cinv_c128: Zinv[item][f] = inv(Z[item][f]) by K3's blocked Gauss-Jordan (same pivoting rule);
 *   detph (optional): [item*F + f][2] = det / |det| (product of the pivots, sign of the interchanges).
 *   Z may have any magnitude: the kernel brings the real m x m block to order one by an exact power of two and undoes
 *   it on the way out, so Z * 2^k returns Zinv * 2^-k bit for bit (the padding is expected to hold the identity).
 * hmv_partial_coherence_c128: kappa from Sinv = inverse spectral matrix and its detph; replaces
 *   partial_coherence (src/mtmvar.py:287-338: minors by np.linalg.det) through M_ij = (-1)^(i+j) det (S^-1)_ji;
 *   kappa: complex [item][f][MP][MP] (hmv_transpose_c128 brings it to (m, m, F)).
 * hmv_gpdc_f64: generalised partial directed coherence from A(f) (hmv_tf_f64's A output) and V
 *   (src/mtmvar.py:388-468); G: real [item][f][MP][MP] (hmv_ffdtf_norm_f64 with normalise = 0 transposes it). */
int hmv_pack_c128(const double* in, double* out, int64_t n_items, int F, int m, void* stream);
int hmv_cinv_c128(const double* Z, int64_t n_items, int m, int F, double* Zinv, double* detph, int32_t* info,
                  double pivot_tau, void* stream);
int hmv_partial_coherence_c128(const double* Sinv, const double* detph, double* kappa, int64_t n_items, int m,
                               int F, void* stream);
int hmv_gpdc_f64(const double* A, const double* V, double* G, int64_t n_items, int m, int F, void* stream);

/* Small elementwise companions, so that no arithmetic of the path is left to the host framework:
 * hmv_trial_mean_f64: R_mean[l] = (R[0][l] + ... + R[T-1][l]) / T over the lag covariances of T trials, the
 *   multi-trial average of count_corr (src/mtmvar.py:54-85; totals accumulated trial by trial, then divided).
 *   R_trials: [n_trials][p+1][MP][MP] (hmv_lagcov_f64 with one item per trial), R_mean: [p+1][MP][MP].
 * hmv_ddtf_f64: ddtf = ffdtf * |kappa|, the product of direct_dtf (src/mtmvar.py:341-385); ffdtf real and kappa
 *   complex128, both [item][m][m][F] (the reference's layout).
 * hmv_band_sums_f64: out[row][b] = sum_{bin_lo[b] <= f < bin_hi[b]} ffdtf[row][f] for the n_rows = items*m*m rows
 *   of an [item][m][m][F] array (bin_lo / bin_hi: int32 device arrays): the band-integrated ffDTF that is
 *   gathered across GPUs (the reference's graph plots integrate ffDTF over a band, src/mtmvar.py:984-987). */
int hmv_trial_mean_f64(const double* R_trials, int64_t n_trials, int m, int p, double* R_mean, void* stream);
int hmv_ddtf_f64(const double* ffdtf, const double* kappa, double* ddtf, int64_t n_items, int m, int F, void* stream);
int hmv_band_sums_f64(const double* ffdtf, int64_t n_rows, int F, const int32_t* bin_lo, const int32_t* bin_hi,
                      int n_bands, double* out, void* stream);

/* Multitaper PSD.  Replaces compute_psd_multitaper (src/psd.py:7-33), i.e.
 * mne.time_frequency.psd_array_multitaper(data, sfreq, fmin, fmax, bandwidth) of mne==1.11.0 with its defaults
 * (remove_dc, non-adaptive eigenvalue weights, normalization "length").  mne is NOT available offline: PARITY
 * UNPINNED -- the algorithm is restated from its published description and checked against an independent
 * NumPy restatement only.  x: [n_ch][ld] (n_times samples used), tapers: [n_tapers][n_times] DPSS windows and
 * weights[k] = sqrt(eigenvalue_k) (hmv_dpss_f64, or scipy.signal.windows.dpss on the host), bins bin_lo..bin_hi of the
 * one-sided spectrum (freq = bin * sfreq / n_times); psd: [n_ch][bin_hi - bin_lo + 1].  Transforms by hipFFT;
 * plans are cached per (n_times, batch).  workspace: hmv_psd_workspace_bytes(ch_chunk, n_times, n_tapers). */
/* DPSS (Slepian) tapers and their concentration ratios on the device: what scipy.signal.windows.dpss(n_times, half_nbw,
 * k_max, sym=bool(sym), norm=2, return_ratios=True) returns (mne's taper generator calls it with sym=False: the symmetric
 * window of n_times + 1 points without its last sample), by the same algorithm -- the k_max largest
 * eigenpairs of the commuting symmetric tridiagonal matrix by Sturm-count multisection and inverse iteration (LAPACK
 * dstebz / dstein restated), SciPy's sign convention, ratios through hipFFT.  tapers: [k_max][n_times], ratios (optional):
 * [k_max].  Agrees with SciPy to ~1e-10 (tests/test_psd.py); PARITY UNPINNED like the PSD itself.  The call synchronises
 * `stream` once when ratios are requested (the FFT plan is created and destroyed inside). */
int64_t hmv_dpss_workspace_bytes(int64_t n_times, int k_max, int sym);
int hmv_dpss_f64(int64_t n_times, double half_nbw, int k_max, int sym, double* tapers, double* ratios,
                 void* workspace, int64_t workspace_bytes, void* stream);
int64_t hmv_psd_workspace_bytes(int64_t ch_chunk, int64_t n_times, int n_tapers);
int hmv_psd_multitaper_f64(const double* x, int64_t n_ch, int64_t n_times, int64_t ld, const double* tapers,
                           const double* weights, int n_tapers, int64_t bin_lo, int64_t bin_hi, double* psd,
                           void* workspace, int64_t workspace_bytes, int64_t ch_chunk, void* stream);

/* Option bits of the fused entry points (`flags`).  0 = the fast defaults. */
#define HMV_FLAG_UNFUSED_NORM 1   /* ffDTF normalisation as a separate pass over |H|^2 (K4) instead of inside K3 */
#define HMV_FLAG_DIRECT_LAGCOV 8   /* K1 sums every window from its own samples even on a regular grid (results then do
                                     not depend on how the windows are laid out: bit-identical across grids) */
#define HMV_FLAG_YW_TILED 2       /* K2 as one workgroup per tile in p + 2 launches (tile column by tile column), and */
#define HMV_FLAG_YW_ONE_LAUNCH 4  /* K2 as one workgroup per window in one launch: same tile products in the same
                                     order, same bits.  Neither flag: one launch, except for large 64-channel
                                     batches, where both forms are HBM-bound and the launch chain is faster. */

#define HMV_FLAG_YW_PIVOTED 16     /* K2: windows that the solver leaves with info != 0 are solved again by the dense LU
                                     with partial pivoting (hmv_yw_solve_f64).  Honoured by every fixed-order fused entry
                                     (the restricted fits of the block Granger entries included); refused with -6 by the
                                     automatic-order entries.  Off: nothing changes, not a bit. */

/* K3 + K4 in one pass.  ffdtf[item][i][j][f] = |H_ij(f)|^2 / sum_{j',f'} |H_ij'(f')|^2, i.e. the arithmetic of
 * mvar_transfer_function (src/mtmvar.py:126-162), |H|^2 (:232) and the normalisation loop of full_freq_dtf
 * (:281-283).  K3 leaves |H|^2 and its row sums in `workspace` (write-through stores); the workgroup whose
 * matrix completes a window (device-scope arrival counter) adds up the row denominators, and the rows of that
 * window are turned into the output array by workgroups of a LATER window of the same launch while the rest of
 * the chip keeps inverting (nobody waits: a row whose window is not complete in time, and the rows of the last few
 * windows of the batch, which no later workgroup exists for, are done by a small kernel right behind K3).  Bit-identical
 * to hmv_tf_f64 + hmv_ffdtf_norm_f64.  Taken when F % 16 == 0 and ffdtf is 16-byte aligned, otherwise the separate K4
 * pass does all windows.  den: [item][MP] out; H (optional, may be NULL): complex128 [item][f][MP][MP] as from hmv_tf_f64 (what
 * hmv_spectra_f64 takes: ffDTF and spectra from one set of inverses); info: [item*F + f].
 * ev_k3_start / ev_k3_stop (optional hipEvent_t) are recorded on `stream` right before and after the K3 kernel itself
 * (not the coefficient-packing kernel in front of it, not the small kernel behind it). */
int64_t hmv_tf_ffdtf_workspace_bytes(int64_t n_items, int m, int p, int F);
int hmv_tf_ffdtf_f64(const double* ar, int64_t n_items, int m, int p, const double* tw, int F,
                     double* ffdtf, double* den, double* H, int32_t* info, double pivot_tau,
                     void* workspace, int64_t workspace_bytes, int64_t flags,
                     void* ev_k3_start, void* ev_k3_stop, void* stream);

/* The same pass with a REDUCED product: band_out[item][i][j][b] = sum_{bin_lo[b] <= f < bin_hi[b]} ffdtf[item][i][j][f]
 * (bin_lo / bin_hi: int32 device arrays of n_bands entries) -- what the reference's graph plots integrate
 * (src/mtmvar.py:984-987) and what crosses PCIe / xGMI per window instead of the 8.4 MB of the full array.  The row
 * workers inside K3 add the bands up from the published |H|^2 rows and the full-resolution array is never written
 * (only the last few windows of a batch pass through a scratch copy of it).  Same bits as hmv_tf_ffdtf_f64 followed by
 * hmv_band_sums_f64.  Needs F % 32 == 0 and F <= ~2700 / 1300 / 640 at 64 / 32 / 16 padded channels (one band's weights
 * must fit the row worker's LDS block); otherwise -10 and the caller takes the two-call route. */
int64_t hmv_tf_ffdtf_bands_workspace_bytes(int64_t n_items, int m, int p, int F);
int hmv_tf_ffdtf_bands_f64(const double* ar, int64_t n_items, int m, int p, const double* tw, int F,
                           double* band_out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                           double* den, int32_t* info, double pivot_tau,
                           void* workspace, int64_t workspace_bytes, int64_t flags,
                           void* ev_k3_start, void* ev_k3_stop, void* stream);

/* Fused sliding-window path K1 -> K2 -> K3 -> K4 over all items, processed `chunk` items at a time so the
 * scratch stays bounded.  Equivalent to calling full_freq_dtf(window, freqs, fs, optimal_model_order=p)
 * (src/mtmvar.py:237-284) on every window.  ffdtf: [n_items][m][m][F].
 * ar_out / V_out (optional): [n_items][MP][MP][p] / [n_items][MP][MP].
 * info_yw: [n_items], info_tf: [n_items*F].  workspace: hmv_sliding_workspace_bytes(chunk, m, p, F) bytes.
 * grid_hop > 0 declares a REGULAR window grid and lets K1 share the overlap (hmv_lagcov_regular_f64): the caller
 * vouches that item = rec * grid_nwin + w is the window starting at grid_first + w * grid_hop of recording rec
 * (item_rec / item_start must say the same; they are still what every other stage and the direct form read) and
 * that recordings are grid_T samples long.  Taken when n is 2..8 whole hops; grid_hop = 0: arbitrary windows.
 * ev_k3_start / ev_k3_stop (optional hipEvent_t, NULL to skip) are recorded on `stream` right before
 * and after the LAST chunk's K3 launch (both launches and what lies between them where K3 comes in two, see
 * aux_stream), so a caller can time the dominant kernel inside its own timed region without an extra synchronisation.
 * aux_stream (optional second hipStream_t, NULL to disable).  The tiled form of K2 is a chain of dependent
 * launches that cannot fill the chip -- it runs as two half-batches, one per stream (fork
 * after K1, join before K3), so their launches interleave on the device.  The default form of K2, when only the
 * ffDTF is asked for (no ar_out / V_out), uses it for the windows of its last, partly filled round: they are solved
 * on aux_stream while K3 already runs on the windows before them (HMV_TUNE_K3_SPLIT; same bits); where K1 can be
 * cut as well (single windows, or a regular grid with the chunk inside one recording), the windows behind the first
 * round go to aux_stream from K1 on.  Either way the call still behaves as one operation on `stream`. */
int64_t hmv_sliding_workspace_bytes(int64_t chunk, int m, int p, int F);
int hmv_sliding_ffdtf_f64(const double* x, int64_t rec_stride, int64_t ld,
                          const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                          int m, int n, int p, const double* freqs, int F, double fs,
                          double* ffdtf, double* ar_out, double* V_out,
                          int32_t* info_yw, int32_t* info_tf,
                          void* workspace, int64_t workspace_bytes, int64_t chunk,
                          double pivot_tau, int64_t flags,
                          int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T,
                          void* ev_k3_start, void* ev_k3_stop, void* stream, void* aux_stream);

/* hmv_sliding_ffdtf_f64 with the reduced product of hmv_tf_ffdtf_bands_f64: band_out: [n_items][m][m][n_bands].  The
 * per-dyad loop of the reference (load, compute, save: src/eeg_alpha_ibi_ffdtf.py:661-806) streams recordings through
 * this entry: 154 MB in, 98 MB out per 10-minute dyad instead of 5 GB. */
int64_t hmv_sliding_bands_workspace_bytes(int64_t chunk, int m, int p, int F);
int hmv_sliding_ffdtf_bands_f64(const double* x, int64_t rec_stride, int64_t ld,
                                const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                                int m, int n, int p, const double* freqs, int F, double fs,
                                double* band_out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                                double* ar_out, double* V_out,
                                int32_t* info_yw, int32_t* info_tf,
                                void* workspace, int64_t workspace_bytes, int64_t chunk,
                                double pivot_tau, int64_t flags,
                                int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T,
                                void* ev_k3_start, void* ev_k3_stop, void* stream, void* aux_stream);

/* hmv_sliding_ffdtf_f64 that ALSO returns the multivariate spectra S(f) = H(f) V H(f)^T (plain transpose, as
 * src/mtmvar.py:199) of every window -- the two products the reference's orchestrators always compute together, there
 * from two separate fits (src/eeg_alpha_ibi_ffdtf.py:592-604, src/mtmvar.py:1100-1113), here from ONE fit and ONE set of
 * inverses: K3 leaves H of a chunk in the workspace, K5 turns it into S_out: complex128 [n_items][m][m][F] (the
 * reference's layout).  V is this library's own residual covariance, symmetric up to rounding, so K5 computes the upper
 * triangle of S only and mirrors it (S_ij and S_ji of the reference differ by rounding; here they are equal). */
int64_t hmv_sliding_spectra_workspace_bytes(int64_t chunk, int m, int p, int F);
int hmv_sliding_ffdtf_spectra_f64(const double* x, int64_t rec_stride, int64_t ld,
                                  const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                                  int m, int n, int p, const double* freqs, int F, double fs,
                                  double* ffdtf, double* S_out, double* ar_out, double* V_out,
                                  int32_t* info_yw, int32_t* info_tf,
                                  void* workspace, int64_t workspace_bytes, int64_t chunk,
                                  double pivot_tau, int64_t flags,
                                  int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T,
                                  void* stream, void* aux_stream);

/* Sliding-window dDTF and GPDC: direct_dtf (src/mtmvar.py:341-385) and gen_partial_directed_coherence (:388-468) of
 * every window, with the conventions of hmv_sliding_ffdtf_f64 (device pointers, `chunk` items at a time, grid_hop /
 * grid_first / grid_nwin / grid_T for the shared-overlap K1, optional ar_out / V_out).
 * n_bands = 0: out is [n_items][m][m][F]; n_bands >= 1: out is [n_items][m][m][n_bands], band b the sum over the bins
 * bin_lo[b] <= f < bin_hi[b] (int32 device arrays) -- the chunk's full array passes through the workspace first.
 * dDTF = ffDTF * |kappa| (kappa_ii = 1).  The ffDTF is the one K3's fused pass writes for the chunk (hmv_tf_ffdtf_f64);
 * |kappa_ij| = |W_ji| / sqrt(|W_ii| |W_jj|) with W(f) = S(f)^-1 = A(f)^T V^-1 A(f), evaluated per window as a
 * trigonometric polynomial of degree 2p with real coefficients (no minors, no determinant, no inverse of S: equal to the
 * reference's minors-based kappa to rounding, not bitwise).  info_yw: [n_items] as K2, and -(c + 1) where V is not
 * positive definite (Cholesky pivot c); info_tf: [n_items*F] as hmv_sliding_ffdtf_f64.
 * GPDC_ij(f) = (|A_ij(f)| / sigma_i) / sqrt(sum_k |A_kj(f)|^2 / sigma_k^2), 0 where the denominator vanishes.  No K3 and
 * no inversion: A(f) is built on chip and never stored, so unlike the reference (which inverts A(f) in
 * mvar_transfer_function and raises on an exactly singular one) only the Yule-Walker failure is reported, in info_yw.
 * workspace: hmv_sliding_{ddtf,gpdc}_workspace_bytes(chunk, m, p, F, n_bands) bytes (-1 for bad arguments). */
int64_t hmv_sliding_ddtf_workspace_bytes(int64_t chunk, int m, int p, int F, int n_bands);
int hmv_sliding_ddtf_f64(const double* x, int64_t rec_stride, int64_t ld,
                         const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                         int m, int n, int p, const double* freqs, int F, double fs,
                         double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                         void* workspace, int64_t workspace_bytes, int64_t chunk,
                         double pivot_tau, int64_t flags,
                         int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T,
                         void* stream, void* aux_stream);
int64_t hmv_sliding_gpdc_workspace_bytes(int64_t chunk, int m, int p, int F, int n_bands);
int hmv_sliding_gpdc_f64(const double* x, int64_t rec_stride, int64_t ld,
                         const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                         int m, int n, int p, const double* freqs, int F, double fs,
                         double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* ar_out, double* V_out, int32_t* info_yw,
                         void* workspace, int64_t workspace_bytes, int64_t chunk, int64_t flags,
                         int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T,
                         void* stream, void* aux_stream);

/* Block (multivariate) Granger causality between two groups of channels, per window (csrc/block_gc.hip): channels
 * 0 .. split-1 are block A, split .. m-1 block B, 1 <= split <= m-1.  Geweke (1982); not a function of the reference.
 * From the window's order-p Yule-Walker fit (ar, V =: Sigma), A(f) = I - sum_k ar_k z^k (z: hmv_twiddles_f64), H = A^-1 and
 *   S(f) = H Sigma H^H  -- the CONJUGATE transpose, NOT the plain transpose that hmv_spectra_f64 reproduces from the
 *   reference --
 * spectral, src -> dst:  f(f) = ln det S_dd - ln det(S_dd - H_ds Sigma_{s|d} H_ds^H),  Sigma_{s|d} = Sigma_ss - Sigma_sd Sigma_dd^-1 Sigma_ds,
 * evaluated as ln det Sigma_{s|d} + ln det W_ss(f) - 2 ln|det At_ss(f)| with W = A^H Sigma^-1 A and
 * At_ss = A_ss - Sigma_sd Sigma_dd^-1 A_ds: no inverse of A(f), no S (equal to the definition to rounding);
 * time domain:  F_{A->B} = ln det Sr_BB - ln det Sigma_BB,  F_{B->A} = ln det Sr_AA - ln det Sigma_AA,
 *   F_{A.B} = ln(det Sigma_AA det Sigma_BB / det Sigma),  F_{A,B} = their sum;  Sr_XX is the residual covariance of the
 *   order-p Yule-Walker fit of block X alone from the same lag covariances (the classical Geweke estimator with the same
 *   order in the restricted fit; it differs from the state-space / spectral-factorisation estimators).
 *
 * hmv_block_gc_f64: the spectral stage on its own.  ar [item][MP][MP][p], V [item][MP][MP] (K2's layouts), freqs [F] ->
 *   spectral [item][2][F], index 0 = A -> B, 1 = B -> A.  info_v [item] (written): -(c + 1) where V, one of its two
 *   diagonal blocks or a Schur complement Sigma_{s|d} is not positive definite (c the column of V; the window's spectral
 *   rows are then NaN); info_gc [item*F + f]: -(c + 1) a non-positive pivot of W_ss(f), +(c + 1) a zero pivot of At_ss(f), either
 *   direction.  workspace: hmv_block_gc_workspace_bytes(n_items, m, p, split, F) bytes (-1 for bad arguments).
 * hmv_sliding_block_gc_f64: from samples to outputs, with the conventions of hmv_sliding_ddtf_f64 (device pointers,
 *   caller-owned buffers, `chunk` items at a time, grid_hop / grid_first / grid_nwin / grid_T for the shared-overlap K1,
 *   optional ar_out / V_out, flags).  One K1 and one K2 per window serve both directions and the time-domain values; the
 *   two restricted fits run in the form of K2 that `flags` (HMV_FLAG_YW_TILED / _ONE_LAUNCH) and HMV_TUNE_YW_FORM select
 *   for the full fit.
 *   spectral: [item][2][F] (n_bands = 0) or [item][2][n_bands], band b the sum over the bins bin_lo[b] <= f < bin_hi[b] --
 *   the bits of hmv_band_sums_f64 on the full output.  time: [item][4] = (F_{A->B}, F_{B->A}, F_{A.B}, F_{A,B}).
 *   info_yw [item]: K2's info of the full fit, or what info_v reports above;  info_red [item][2]: the restricted fits of block A and block B (K2's info, or
 *   -(c + 1) where the restricted residual covariance is not positive definite);  info_gc [item*F]: as above.
 *   workspace: hmv_block_gc_sliding_workspace_bytes(chunk, m, p, split, F, n_bands) bytes (-1 for bad arguments).
 * Refused before any launch, each with its own code: channel count (-1), p outside 1..HMV_MAX_ORDER (-2), n <= p (-3), a
 * null pointer, n_items < 0 or chunk < 1 (-4), workspace too small (-7), an inconsistent grid (-9), split outside 1..m-1 (-11), F < 1
 * (-12), a null spectral output (-13), n_bands < 0 (-14). */
int64_t hmv_block_gc_workspace_bytes(int64_t n_items, int m, int p, int split, int F);
int hmv_block_gc_f64(const double* ar, const double* V, int64_t n_items, int m, int p, int split,
                     const double* freqs, int F, double fs, double* spectral, int32_t* info_v, int32_t* info_gc,
                     void* workspace, int64_t workspace_bytes, void* stream);
int64_t hmv_block_gc_sliding_workspace_bytes(int64_t chunk, int m, int p, int split, int F, int n_bands);
int hmv_sliding_block_gc_f64(const double* x, int64_t rec_stride, int64_t ld,
                             const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                             int m, int n, int p, int split, const double* freqs, int F, double fs,
                             double* spectral, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                             double* time, double* ar_out, double* V_out,
                             int32_t* info_yw, int32_t* info_red, int32_t* info_gc,
                             void* workspace, int64_t workspace_bytes, int64_t chunk, int64_t flags,
                             int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T, void* stream);

/* Block Granger causality of pairs of recordings -- what the surrogate and pseudo-dyad tests of the block values run on.
 * hmv_sliding_block_gc_pairs_f64: hmv_sliding_block_gc_f64 of the window at item_start[it] whose channels < split are those
 *   of recording rec_a[it] and whose channels >= split are those of recording rec_b[it] (K1 of hmv_lagcov_pairs_f64, with its
 *   optional R_base / base_a / base_b; there is no grid).  With rec_b == rec_a every output has the bits of
 *   hmv_sliding_block_gc_f64; with rec_b != rec_a those of that call on the pair written out as one recording.
 *   want: bit 0 the spectral output, bit 1 the time-domain values; 0 is refused (-15).
 *     bit 0 clear: F may be 0 and spectral, freqs, bin_lo, bin_hi, info_gc null -- none of them is read or written, and
 *       no twiddles, factor, gram, per-frequency or band-sum kernel runs: K1, K2 and one kernel that takes the Cholesky
 *       log-determinants of Sigma, Sigma_AA, Sigma_BB and of the restricted residual covariances (bgc_time_kernel).
 *     bit 1 clear: time, info_red may be null, no restricted fit runs, red_out / red_base are ignored.
 *   red_out [item][2] (optional): (ln det Sr_AA, ln det Sr_BB) exactly as the time values use them (NaN where not positive
 *     definite).
 *   red_base [n_base][2] with info_red_base [n_base][2] (optional, both or neither; they need R_base, base_a, base_b: -4
 *     otherwise): red_out and info_red of an earlier call on the observed windows that R_base holds.  A pair changes only
 *     the cross-recording covariance blocks, so the restricted fit of block A is that of window base_a[it] and the one of
 *     block B that of window base_b[it]: ln det Sr_AA and its info are read from row base_a[it], column 0, ln det Sr_BB and
 *     its info from row base_b[it], column 1, and neither the gather nor the two restricted solves run.  Same bits.
 *   workspace: hmv_block_gc_pairs_workspace_bytes(chunk, m, n, p, split, F, n_bands, want) bytes (-1 for bad arguments; F and
 *     n_bands are not looked at with bit 0 of want clear).
 * Refusals: those of hmv_sliding_block_gc_f64, want outside 1..3 (-15), a null rec_b, R_base / base_a / base_b not all or
 * none, red_base without info_red_base or without R_base (-4). */
int64_t hmv_block_gc_pairs_workspace_bytes(int64_t chunk, int m, int n, int p, int split, int F, int n_bands, int want);
int hmv_sliding_block_gc_pairs_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                                   const int64_t* rec_a, const int64_t* rec_b, const int64_t* item_start, int64_t n_items,
                                   int m, int n, int p, int split, const double* freqs, int F, double fs,
                                   double* spectral, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                                   double* time, double* ar_out, double* V_out,
                                   int32_t* info_yw, int32_t* info_red, int32_t* info_gc,
                                   void* workspace, int64_t workspace_bytes, int64_t chunk, int64_t flags,
                                   const double* R_base, const int64_t* base_a, const int64_t* base_b,
                                   int want, double* red_out, const double* red_base, const int32_t* info_red_base,
                                   void* stream);

/* Automatic model order, window by window (csrc/yw_auto.hip).  Every connectivity function of the reference takes
 * `max_model_order=20, optimal_model_order=None, crit_type='AIC'`: with no order given it calls mvar_criterion
 * (src/mtmvar.py:551-601), which fits EVERY order 1..pmax with ar_coeff (:90-123) and returns the first arg-min of
 *   crit_q = log det V_q + c q m^2 / n,    c = 2 (AIC), 2 log log n (HQ), log n (SC),
 * and then fits that order once more.  The two entries below do this in one pass of K2's block Levinson-Whittle
 * recursion, which holds the complete order-q model (coefficients, V_q, log det V_q) on its way to order pmax.
 * crit: 0 AIC, 1 HQ, 2 SC (the numbering of hmv_fad_f64).
 *
 * hmv_yw_solve_auto_f64: K2 alone.  R [item][pmax+1][MP][MP] (K1 at p = pmax), n the window length, ws
 *   hmv_yw_workspace_doubles(m, pmax) doubles per item.  Outputs: order_out int32 [n_items], the selected order q*;
 *   ar [item][MP][MP][pmax], the order-q* coefficients with the lags >= q* written as +0.0;  V [item][MP][MP] = V_q*;
 *   crit_out [item][pmax] (optional) the criterion curve;  vq_logdet [item][pmax] (optional) log det V_q.
 *   info [item]: a non-positive pivot at ANY order <= pmax fails the window (info != 0, order_out = 0, ar = 0, V = R_0).
 *   The reference would take the log of a non-positive determinant there, get NaN, and let argmin return that index; that
 *   is not reproduced.  A window whose tile inverses were badly conditioned at an order <= q* is re-solved by the block
 *   LDL^T at its own order on the device (no host round trip); its selected order stays the recursion's.
 *   flags: 0 (the LDL^T forms HMV_FLAG_YW_TILED / _ONE_LAUNCH have no automatic order: refused).
 *
 * hmv_sliding_auto_f64: ONE entry for all fused sliding-window routes -- hmv_sliding_ffdtf_f64 / _bands / _spectra
 *   (full_freq_dtf, src/mtmvar.py:236-284; multivariate_spectra, :165-201), hmv_sliding_ddtf_f64 (direct_dtf, :341-385)
 *   and hmv_sliding_gpdc_f64 (gen_partial_directed_coherence, :388-468) -- with `optimal_model_order=None`:
 *   K1 sums pmax + 1 lags, K2 selects, and every later stage runs at p = pmax on the zero-padded coefficients (the added
 *   terms of A(f) = I - sum_k ar_k e^{-2 pi i f k / fs} are exact zeros).
 *   measure: HMV_MEASURE_FFDTF, _DDTF or _GPDC.  n_bands = 0: out is [n_items][m][m][F]; n_bands >= 1: out is
 *   [n_items][m][m][n_bands] (bin_lo / bin_hi as in the fixed-order entries).  S_out (optional; measure = FFDTF and
 *   n_bands = 0 only): complex128 [n_items][m][m][F] as hmv_sliding_ffdtf_spectra_f64.  order_out int32 [n_items]
 *   (required), crit_out [n_items][pmax] (optional), ar_out [n_items][MP][MP][pmax] zero-padded (optional), V_out
 *   (optional).  info_tf is unused for GPDC (may be NULL).  Grid arguments, chunk, flags, info_yw and info_tf as in the
 *   fixed-order entries.  Refused: pmax outside 1..HMV_MAX_ORDER, n <= pmax, crit outside 0..2, and what the fixed-order
 *   entries refuse.
 *   workspace: hmv_sliding_auto_workspace_bytes(measure, chunk, m, pmax, F, n_bands) bytes, with n_bands = -1 for the
 *   full ffDTF together with S_out (-1 for bad arguments). */
#define HMV_MEASURE_FFDTF 0
#define HMV_MEASURE_DDTF 1
#define HMV_MEASURE_GPDC 2
int hmv_yw_solve_auto_f64(const double* R, int64_t n_items, int m, int pmax, int n, int crit, double* ws, double* ar,
                          double* V, int32_t* order_out, double* crit_out, double* vq_logdet, int32_t* info,
                          int64_t flags, void* stream);
int64_t hmv_sliding_auto_workspace_bytes(int measure, int64_t chunk, int m, int pmax, int F, int n_bands);
int hmv_sliding_auto_f64(int measure, const double* x, int64_t rec_stride, int64_t ld,
                         const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                         int m, int n, int pmax, int crit, const double* freqs, int F, double fs,
                         double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out,
                         double* ar_out, double* V_out, int32_t* order_out, double* crit_out,
                         int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes, int64_t chunk,
                         double pivot_tau, int64_t flags,
                         int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T,
                         void* stream, void* aux_stream);

/* Event-locked ensembles (csrc/lagcov_ensemble.hip).  Every estimator of the reference takes `signals` of shape
 * (channels, samples, trials): count_corr (src/mtmvar.py:54-85) averages the lag covariances over the trials, ar_coeff
 * (:96, :106-108) fits ONE model to the average, and full_freq_dtf (:236-284), multivariate_spectra (:165-201), direct_dtf
 * (:341-385) and gen_partial_directed_coherence (:388-468) reach it through ar_coeff when a model order is given.  The
 * two entries below do that for every window of an epoch in one call.
 *   Trials: trial e is the epoch starting at sample trial_start[e] of recording trial_rec[e] (x: [n_rec][m][ld], T
 *   samples per recording).  Groups (one dyad x condition each), CSR: group g owns the trials group_ptr[g] ..
 *   group_ptr[g+1]-1 (group_ptr: n_groups + 1 entries; groups may differ in size, none may be empty).  Item `it` is the
 *   window of n samples that starts item_offset[it] samples after every trial start of group item_group[it]:
 *       R_l(it) = (1/E_g) sum_{e in g} (1/n) X_e[:, :n-l] X_e[:, l:]^T,  X_e = x[trial_rec[e]][:, trial_start[e] + item_offset[it] : + n]
 *   (biased, not demeaned).  All five index arrays are int64 DEVICE arrays whose contents the caller has checked
 *   (hyperscanning_signal_analysis_amd.engine.validate_trials): the kernels address with them.
 *   grid_hop = 0: arbitrary offsets.  grid_hop > 0 declares a regular grid: the caller vouches that n_items = n_groups *
 *   grid_nwin and that item g * grid_nwin + w belongs to group g and has offset w * grid_hop.  K1 then takes the
 *   shared-overlap form -- hop-block sums over all trials once, windows assembled from k = n / grid_hop blocks -- when
 *   n is a whole number of hops, 2 <= k <= HMV_MAX_HOPS_ENSEMBLE, grid_hop > p, the hop rounded up to 4 samples plus p is
 *   at most 96 and HMV_FLAG_DIRECT_LAGCOV is not set; otherwise the direct form (the trial loop inside lagcov_kernel's
 *   mapping), whose result for groups of ONE trial has the bits of hmv_lagcov_f64.  The two forms agree to rounding.
 *
 * hmv_lagcov_ensemble_f64: K1 alone.  R [n_items][p+1][MP][MP]; workspace: hmv_lagcov_ensemble_workspace_doubles(n_items,
 *   m, n, p, grid_hop, grid_nwin) doubles (0 without a grid; -1 for bad arguments), workspace_doubles its size.
 * hmv_sliding_ensemble_f64: the fused path K1 -> K2 -> K3 (-> K5) / dDTF / GPDC on the trial-averaged covariances; every
 *   stage after K1 is that of the single-trial entries.  measure, out, bin_lo / bin_hi / n_bands, S_out, ar_out, V_out,
 *   info_yw, info_tf, chunk, pivot_tau, flags as in hmv_sliding_auto_f64 (fixed order p).  workspace:
 *   hmv_sliding_ensemble_workspace_bytes(measure, chunk, m, n, p, F, n_bands, grid_hop, grid_nwin), n_bands = -1 for the
 *   full ffDTF together with S_out.
 * Refused before any launch: channel count (-1), order (-2), n <= p (-3), null pointers (-4), workspace too small (-7),
 *   an inconsistent grid (-9: grid_hop < 0, grid_nwin < 1, n_items != n_groups * grid_nwin, (grid_nwin - 1) * grid_hop + n >
 *   T, ld < T), n_groups < 1 (-10). */
#define HMV_MAX_HOPS_ENSEMBLE 32
int64_t hmv_lagcov_ensemble_workspace_doubles(int64_t n_items, int m, int n, int p, int64_t grid_hop, int64_t grid_nwin);
int hmv_lagcov_ensemble_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                            const int64_t* trial_rec, const int64_t* trial_start, const int64_t* group_ptr,
                            int64_t n_groups, const int64_t* item_group, const int64_t* item_offset, int64_t n_items,
                            int m, int n, int p, double* R, double* workspace, int64_t workspace_doubles,
                            int64_t grid_hop, int64_t grid_nwin, int64_t flags, void* stream);
int64_t hmv_sliding_ensemble_workspace_bytes(int measure, int64_t chunk, int m, int n, int p, int F, int n_bands,
                                             int64_t grid_hop, int64_t grid_nwin);
int hmv_sliding_ensemble_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                             const int64_t* trial_rec, const int64_t* trial_start, const int64_t* group_ptr,
                             int64_t n_groups, const int64_t* item_group, const int64_t* item_offset, int64_t n_items,
                             int m, int n, int p, const double* freqs, int F, double fs,
                             double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out,
                             double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                             void* workspace, int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                             int64_t grid_hop, int64_t grid_nwin, void* stream, void* aux_stream);

/* Trial-shuffle surrogates of an event-locked ensemble (csrc/lagcov_ensemble.hip, lagcov_ens_split_kernel).  A second
 * trial table (trial_rec_b, trial_start_b), indexed through the same group_ptr, names the partner of every trial: trial
 * step e of a group reads the channels < split from trial (trial_rec[e], trial_start[e]) and the channels >= split from
 * trial (trial_rec_b[e], trial_start_b[e]),
 *     x~_e = [a_e ; b_pi(e)],    R~_l(it) = (1/E_g) sum_e (1/n) X~_e[:, :n-l] X~_e[:, l:]^T
 * -- the second participant's trials permuted against the first's inside the group; the permutation is the order of table
 * B and nothing is written out.  Always the direct form (trial loop in the kernel, trials ascending, lagcov_kernel's order
 * of products): table B = table A gives the bits of hmv_lagcov_ensemble_f64 with HMV_FLAG_DIRECT_LAGCOV.
 *   R_base [n_base][p+1][MP][MP] with item_base int64 [n_items] (device; both or neither): an element (row, col) with both
 *   indices < split or both >= split (padded rows and columns count as >= split) is a sum over all trials of one
 *   participant, which no permutation changes.  Such an element is not computed but copied from
 *   R_base[item_base[it]][lag], the padding's identity included, and an accumulator (4 rows x 16 columns of one wave) whose
 *   real elements are all of this kind runs no MFMA.  Accumulators that straddle split are computed whole and their
 *   within-participant elements then overwritten, so the result does not depend on the tiling.  Without R_base every
 *   element is computed; the cross elements are the same bits either way.
 *   The contents of table B and of item_base (0 <= item_base[it] < n_base) are checked by the caller like the other index
 *   arrays (hyperscanning_signal_analysis_amd.engine.validate_trials): the kernel addresses with them.
 * hmv_lagcov_ensemble_split_f64: K1 alone, arguments as hmv_lagcov_ensemble_f64 without workspace and grid (flags is
 *   accepted and not looked at: there is one form).
 * hmv_sliding_ensemble_split_f64: the fused path of hmv_sliding_ensemble_f64 with this K1; everything after K1 is the
 *   existing path.  workspace: hmv_sliding_ensemble_workspace_bytes(..., grid_hop = 0, grid_nwin = 0).  item_base is
 *   indexed by the item of the call, whatever the chunk.
 * Refused before any launch, in addition to hmv_sliding_ensemble_f64's refusals: split outside 1..m-1 (-5), a null table
 *   B (-4), R_base without item_base or the reverse (-4). */
int hmv_lagcov_ensemble_split_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                                  const int64_t* trial_rec, const int64_t* trial_start, const int64_t* group_ptr,
                                  int64_t n_groups, const int64_t* item_group, const int64_t* item_offset, int64_t n_items,
                                  int m, int n, int p, double* R,
                                  const int64_t* trial_rec_b, const int64_t* trial_start_b, int split,
                                  const double* R_base, const int64_t* item_base, int64_t flags, void* stream);
int hmv_sliding_ensemble_split_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                                   const int64_t* trial_rec, const int64_t* trial_start, const int64_t* group_ptr,
                                   int64_t n_groups, const int64_t* item_group, const int64_t* item_offset, int64_t n_items,
                                   int m, int n, int p, const double* freqs, int F, double fs,
                                   double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out,
                                   double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                                   void* workspace, int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                                   const int64_t* trial_rec_b, const int64_t* trial_start_b, int split,
                                   const double* R_base, const int64_t* item_base, void* stream, void* aux_stream);

/* Pairs of recordings: the pseudo-dyad (shuffled-partner) surrogates of hyperscanning data (csrc/lagcov_ensemble.hip,
 * lagcov_pairs_kernel).  Item `it` is the window of n samples starting at item_start[it] whose channels < split are read
 * from recording rec_a[it] and whose channels >= split are read from recording rec_b[it] (x: [n_rec][m][ld], T samples per
 * recording) -- participant A of one dyad beside participant B of another at the same time points; nothing is written out:
 *     x~(it) = [x[rec_a[it]][:split] ; x[rec_b[it]][split:]][:, item_start[it] : + n],   R_l(it) = (1/n) X~[:, :n-l] X~[:, l:]^T
 * (count_corr's estimator, src/mtmvar.py:35-87: biased 1/n, not demeaned).  One form, lagcov_kernel's mapping, chunks and
 * order of products: every computed element has the bits hmv_lagcov_f64 gives for the same window written out as one
 * recording, and rec_b = rec_a without R_base gives hmv_lagcov_f64's whole result.
 *   R_base [n_base][p+1][MP][MP] with base_a, base_b int64 [n_items] (device; all three or none): an element (row, col) with
 *   both indices < split belongs to participant A alone and is copied from R_base[base_a[it]][lag]; one with both indices
 *   >= split (padded rows and columns count as >= split, their lag-0 identity included) is copied from
 *   R_base[base_b[it]][lag].  Only the cross elements are computed: an accumulator (4 rows x 16 columns of one wave) with no
 *   cross element among its real elements runs no MFMA, one that straddles split is computed whole and its
 *   within-participant elements then overwritten, so the result does not depend on the tiling.  Without R_base every
 *   element is computed; the cross elements are the same bits either way.
 *   rec_a, rec_b, item_start, base_a and base_b are int64 DEVICE arrays whose contents the caller has checked (0 <= rec <
 *   n_rec, 0 <= start, start + n <= T, 0 <= base < n_base; hyperscanning_signal_analysis_amd.engine.validate_items on
 *   both recording tables): the kernel addresses with them.
 * hmv_lagcov_pairs_f64: K1 alone, R [n_items][p+1][MP][MP].  flags is accepted and not looked at: there is one form.
 * hmv_sliding_pairs_f64: the fused path K1 -> K2 -> K3 (-> K5) / dDTF / GPDC with this K1; everything after K1 is the
 *   existing path.  The arguments are those of hmv_sliding_ensemble_split_f64 with (rec_a, rec_b, item_start) in place of
 *   the trial and group tables.  workspace: hmv_pairs_workspace_bytes(measure, chunk, m, n, p, F, n_bands), n_bands
 *   = -1 for the full ffDTF together with S_out (the same number as hmv_sliding_ensemble_workspace_bytes without a grid).
 *   base_a and base_b are indexed by the item of the call, whatever the chunk.
 * Refused before any launch: channel count (-1), order (-2), n <= p (-3), null pointers, R_base without both base tables or
 *   the reverse (-4), split outside 1..m-1 (-5), workspace too small (-7). */
int hmv_lagcov_pairs_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                         const int64_t* rec_a, const int64_t* rec_b, const int64_t* item_start, int64_t n_items,
                         int m, int n, int p, int split, double* R,
                         const double* R_base, const int64_t* base_a, const int64_t* base_b, int64_t flags, void* stream);
int64_t hmv_pairs_workspace_bytes(int measure, int64_t chunk, int m, int n, int p, int F, int n_bands);
int hmv_sliding_pairs_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                          const int64_t* rec_a, const int64_t* rec_b, const int64_t* item_start, int64_t n_items,
                          int m, int n, int p, const double* freqs, int F, double fs,
                          double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out,
                          double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                          void* workspace, int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                          int split, const double* R_base, const int64_t* base_a, const int64_t* base_b,
                          void* stream, void* aux_stream);

/* Weighted trial sums of an event-locked ensemble: the label permutations of the condition contrast (csrc/lagcov_mix.hip).
 * The trial-averaged lag covariances are linear in the per-trial ones, R_l(condition c, window w) = (1/E_c) sum_{e in c}
 * R_l(trial e, window w), so every relabelling of a pool of trials is a weighted sum over the trial axis of ONE per-trial
 * stack, and the samples are read once:
 *     R[k][w] = scale[k] * sum_{e = 0..n_trials-1} W[k][e] * Rt[e][w]
 *   Rt [n_trials][n_win][p+1][MP][MP]: the per-trial stack, exactly what hmv_lagcov_ensemble_f64 writes for n_trials groups
 *   of one trial with the items group-major (16-byte aligned).  W [n_mix][n_trials]: the weights, general doubles (0 / 1
 *   label rows with scale = 1 / E_c give the ensemble estimator to rounding).  scale [n_mix], or NULL for 1.
 *   R [n_mix][n_win][p+1][MP][MP]: item k * n_win + w is mix row k at window w.  All are DEVICE arrays.
 *   Every real element (row, col < m) of every lag is one chain acc = fma(W[k][e], Rt[e], acc) over the trials in
 *   ascending order, then one multiplication by scale[k]; no atomics, no split of the trial sum.  The bits of element
 *   (k, w) depend on row k of W, on scale[k] and on the stack, and on nothing else: not on the other rows of the call, on
 *   n_mix, or on how a caller chunks rows or windows.  The padding is written by the kernel, whatever Rt holds there:
 *   zero, with the lag-0 identity on the padded diagonal.
 * hmv_lagcov_mix_f64: K1 alone.
 * hmv_sliding_mix_f64: the fused path K1 -> K2 -> K3 (-> K5) / dDTF / GPDC with this K1; everything after K1 is the
 *   existing path, with measure, out, bin_lo / bin_hi / n_bands, S_out, ar_out, V_out, info_yw, info_tf, chunk, pivot_tau
 *   and flags as in hmv_sliding_ensemble_f64 (fixed order p; n is the window length the stack was computed with, which K1
 *   itself does not use).  A chunk is a contiguous range of items and may start or end inside a row.  workspace:
 *   hmv_mix_workspace_bytes(measure, chunk, m, p, F, n_bands), n_bands = -1 for the full ffDTF together with S_out
 *   (the same number as hmv_pairs_workspace_bytes).
 * Refused before any launch: channel count (-1), order (-2), n <= p (-3; hmv_sliding_mix_f64 only), null or misaligned
 *   pointers (-4), workspace too small (-7), n_trials, n_win or n_mix < 1 (-10). */
int hmv_lagcov_mix_f64(const double* Rt, int64_t n_trials, int64_t n_win, const double* W, const double* scale,
                       int64_t n_mix, int m, int p, double* R, void* stream);
int64_t hmv_mix_workspace_bytes(int measure, int64_t chunk, int m, int p, int F, int n_bands);
int hmv_sliding_mix_f64(int measure, const double* Rt, int64_t n_trials, int64_t n_win,
                        const double* W, const double* scale, int64_t n_mix,
                        int m, int n, int p, const double* freqs, int F, double fs,
                        double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out,
                        double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                        void* workspace, int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                        void* stream, void* aux_stream);

/* FAD (frequency-amplitude-damping) decomposition of univariate AR models, batched over series.  Replaces
 * fad_decomposition (src/mtmvar.py:607-757): order selection as mvar_criterion at m = 1 (:551-601), the fit of ar_coeff
 * (:90-123, count_corr :35-87: biased 1/n autocovariance, no demeaning) by Levinson-Durbin, and the partial-fraction
 * expansion of scipy.signal.residuez([1], [1, -a_1, .., -a_p]) with its default grouping (poles within 1e-3 averaged
 * and treated as one repeated pole, unique poles sorted by |z|, repeated-pole residues ascending in power).
 * Series s = item * m + ch is channel ch of window `item`, addressed as in hmv_lagcov_f64 (x: [n_rec][m][ld]; window
 * item covers samples item_start[item] .. + n of recording item_rec[item]).  pmax: 1..32, n > pmax.
 * order: 0 = automatic (first arg-min of log V_p + c p / n, p = 1..pmax, c = 2 / 2 log log n / log n for
 * crit = 0 / 1 / 2 = AIC / HQ / SC), else the fixed order 1..pmax.
 * Outputs, one row of pmax per series (entries past the series' order: NaN, osc_mask 0, paired -1):
 *   order_out int32 [S];  crit_out [S][pmax] (optional, automatic mode: the criterion curve);  ar [S][pmax];
 *   noise_variance [S] = r_0 - a . r_{1..p};  poles, C, alpha complex128 [S][pmax] (alpha = log(z) fs);  freq = Im alpha
 *   / 2 pi, beta = -Re alpha, bandwidth = beta / 2 pi, phi = arg C, B = 2 |C|  [S][pmax];  osc_mask uint8 [S][pmax]
 *   (|Im z| > imag_tol);  paired int32 [S][pmax] + n_paired int32 [S]: the poles with Im z > imag_tol sorted by
 *   frequency (pair_conjugates != 0), else every oscillatory pole in pole order;
 *   info int32 [S]: bit 0 fit breakdown (r_0 = 0, V <= 0 or non-finite; outputs NaN), bit 1 root iteration did not
 *   converge (outputs NaN), bit 2 a chain of poles within 1e-3 wider than 1e-3 (residuez's grouping would depend on
 *   the root order; grouped here by connected components).
 * hmv_fad_workspace_bytes: scratch of hmv_fad_f64 -- 0 for valid arguments (every intermediate lives in LDS), -1
 * otherwise; there so that callers size buffers the same way as for the other entries. */
int64_t hmv_fad_workspace_bytes(int64_t n_series, int pmax);
int hmv_fad_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec, const int64_t* item_start,
                int64_t n_items, int m, int n, int pmax, int order, int crit, double fs, double imag_tol,
                int pair_conjugates, int32_t* order_out, double* crit_out, double* ar, double* noise_variance,
                double* poles, double* C, double* alpha, double* freq, double* beta, double* bandwidth, double* phi,
                double* B, uint8_t* osc_mask, int32_t* paired, int32_t* n_paired, int32_t* info, void* stream);
/* Stages C-D of hmv_fad_f64 on given coefficients ar [S][p] (residuez on [1, -a_1, .., -a_p], src/mtmvar.py:643-652
 * onwards); outputs as above with pmax = p. */
int hmv_fad_decompose_f64(const double* ar, int64_t n_series, int p, double fs, double imag_tol, int pair_conjugates,
                          double* poles, double* C, double* alpha, double* freq, double* beta, double* bandwidth,
                          double* phi, double* B, uint8_t* osc_mask, int32_t* paired, int32_t* n_paired, int32_t* info,
                          void* stream);

/* Surrogate significance of the sliding-window measures (hmv_sliding_ffdtf_bands_f64, hmv_sliding_ddtf_f64,
 * hmv_sliding_gpdc_f64 with bands).  A block of surrogates x windows is laid out surrogate-major: item
 * k = s * n_win + w is surrogate s of window w.  The surrogate windows go through the sliding entries as n_items
 * recordings of n samples (start 0, no grid); their band values come back as surr [n_surr][n_win][m][m][n_bands].
 * hmv_surrogate_shift_f64: out[k][c][t] = x[rec][c][start + t] for c < split and x[rec][c][(start + t + shift[s][rec])
 *   mod T] for c >= split (t = 0..n-1; rec = item_rec[w], start = item_start[w]; shift: int64 [n_surr][n_rec]) -- the
 *   second participant circularly shifted against the first.  out: [n_surr][n_win][m][n].  The windows must lie inside
 *   their recordings (the caller checks item_rec / item_start as for hmv_lagcov_f64).
 * hmv_surrogate_phase_c128: out[k][c][f] = spec[w][c][f] exp(i phi[s][c][f]), except bins f = 0 and (even n) f = n/2,
 *   which are copied.  spec: complex128 [n_win][m][n/2+1], the rfft of every window; phi: [n_surr][m][n/2+1]; out:
 *   complex128 [n_surr][n_win][m][n/2+1] (the inverse rfft gives the phase-randomised windows).
 * hmv_null_accumulate_f64: per cell (w, i, j, b) of the tested pairs (tested: uint8 [m][m]), walks the block's
 *   surrogates in order, skips those whose fit failed (surr_bad: uint8 [n_surr][n_win]) and NaN values, and updates
 *   the running state: n_valid int32 [n_win], count / count_fwe / n_cell int32 and mean / m2 [n_win][m][m][n_bands]
 *   (zero before the first block).  count: surrogate values >= observed; count_fwe: surrogates whose maximum over the
 *   tested pairs (M [n_surr][n_win][n_bands], written) is >= observed; mean / m2: Welford in surrogate order.  No
 *   atomics: the result does not depend on how the surrogates are split into blocks.  p, p_fwe, null_mean, null_std
 *   (optional, all or none, [n_win][m][m][n_bands]): (1 + count) / (1 + n_valid), (1 + count_fwe) / (1 + n_valid), mean
 *   and sqrt(m2 / (n_cell - 1)) after this block; NaN on untested cells. */
int hmv_surrogate_shift_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* item_rec,
                            const int64_t* item_start, int64_t n_win, const int64_t* shift, int64_t n_rec, int n_surr, int m,
                            int n, int split, double* out, void* stream);
int hmv_surrogate_phase_c128(const double* spec, int64_t n_win, const double* phi, int n_surr, int m, int n, double* out,
                             void* stream);
int hmv_null_accumulate_f64(const double* observed, const double* surr, const uint8_t* surr_bad, const uint8_t* tested,
                            int64_t n_win, int n_surr, int m, int n_bands, double* M, int32_t* n_valid, int32_t* count,
                            int32_t* count_fwe, int32_t* n_cell, double* mean, double* m2, double* p, double* p_fwe,
                            double* null_mean, double* null_std, void* stream);

/* Model validation: residuals and whiteness statistics of every window's MVAR fit (csrc/validate.hip).  Beyond the
 * reference, which computes the residual covariance (ar_coeff, src/mtmvar.py:119) but never the residuals; definitions
 * after Luetkepohl, New Introduction to Multiple Time Series Analysis, section 4.4.3; Hosking 1980; Li & McLeod 1981.
 * For a window X (m x n), coefficients A_k = ar[:, :, k-1] (k = 1..p), N = n - p and h tested lags:
 *     E        = X[:, p:] - sum_k A_k X[:, p-k : n-k]                 (m x N; column c is the residual at sample p + c)
 *     C_l      = E[:, :N-l] E[:, l:]^T / N,  l = 0..h                  (K1's estimator: biased, residuals not demeaned)
 *     s_l      = || L^-1 C_l L^-T ||_F^2,  C_0 = L L^T,  l = 1..h
 *     Q_BP     = N sum_l s_l;   Q_LM = Q_BP + m^2 h (h+1) / (2N);   Q_H = N^2 sum_l s_l / (N - l)
 *     r_l[i,j] = C_l[i,j] / sqrt(C_0[i,i] C_0[j,j]);   acf_count = #{(l,i,j): |r_l[i,j]| > acf_thr}
 *     q_ch[i]  = N (N+2) sum_l r_l[i,i]^2 / (N - l)
 * The degrees of freedom (m^2 (h - q) with q the window's model order) and the chi-square tails are the caller's.
 * hmv_residuals_f64: E[item][c][t] for c < m, t < n - p;  E: [n_items][m][ldE], ldE >= n - p; columns >= n - p are not
 *   written.  Products in a fixed order (lags ascending, then source channel ascending): the bits of a window's residuals
 *   do not depend on the batch.  workspace: hmv_residuals_workspace_bytes(chunk_items, m, p) bytes for any chunk_items >= 1
 *   (the coefficients re-ordered once per item into the operand order; the call walks the items in chunks of what fits).
 * hmv_whiteness_f64: the statistics from C [n_items][h+1][MP][MP] (hmv_lagcov_f64 over the residuals as n_items
 *   recordings of N samples, p = h).  s [items][h], q [items][3] (BP, LM, H), q_ch [items][m], acf_count int32 [items], info
 *   int32 [items]: a non-positive Cholesky pivot of C_0 at column c sets info = c + 1, NaN statistics and acf_count = -1.
 *   Fixed reduction trees, no atomics: run-to-run bit-identical.
 * hmv_model_validation_f64: the three stages, `chunk` items at a time so E and C stay bounded.  resid_cov (optional):
 *   [items][MP][MP] = C_0;  E_out (optional): [n_items][m][ldE].  workspace:
 *   hmv_model_validation_workspace_bytes(chunk, m, n, p, h) bytes (-1 for bad arguments).
 * Refused before any launch: channel count (-1), p outside 1..HMV_MAX_ORDER (-2), h outside 1..HMV_MAX_ORDER (-6),
 *   n - p <= h (-3; hmv_residuals_f64: n <= p, hmv_whiteness_f64: N <= h), null required pointer (-4), workspace too small
 *   (-7), ldE < n - p (-8). */
int64_t hmv_residuals_workspace_bytes(int64_t chunk_items, int m, int p);
int hmv_residuals_f64(const double* x, int64_t rec_stride, int64_t ld,
                      const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                      int m, int n, int p, const double* ar, double* E, int64_t ldE,
                      void* workspace, int64_t workspace_bytes, void* stream);
int hmv_whiteness_f64(const double* C, int64_t n_items, int m, int N, int h, double acf_thr,
                      double* s, double* q, double* q_ch, int32_t* acf_count, int32_t* info, void* stream);
int64_t hmv_model_validation_workspace_bytes(int64_t chunk, int m, int n, int p, int h);
int hmv_model_validation_f64(const double* x, int64_t rec_stride, int64_t ld,
                             const int64_t* item_rec, const int64_t* item_start, int64_t n_items,
                             int m, int n, int p, const double* ar, int h, double acf_thr,
                             double* s, double* q, double* q_ch, int32_t* acf_count, int32_t* info,
                             double* resid_cov, double* E_out, int64_t ldE,
                             void* workspace, int64_t workspace_bytes, int64_t chunk, void* stream);

/* Anti-aliased integer-factor FIR decimation of recordings (csrc/decimate.hip): the first stage of "decimate before
 * fitting".  Replaces scipy.signal.decimate(x, q, ftype='fir', zero_phase=True) as MultimodalData._decimate_signals calls
 * it (src/data_structures.py:792) and scipy.signal.resample_poly(signal, up=1, down=q) of _downsample_signal
 * (src/eeg_alpha_ibi_ffdtf.py:404), which are one operation with different taps (firwin(20 q + 1, 1 / q) under a Hamming
 * window / a Kaiser window with beta = 5):
 *     y[r][c][k] = sum_{j=0}^{n_taps-1} h[j] * x[r][c][k*q + H - j],    H = (n_taps - 1) / 2,    k = 0 .. ceil(T / q) - 1,
 * samples outside [0, T) counting as zero.  x: [n_rec][m][ld] (T samples used, addressed through rec_stride and ld as
 * everywhere), h: [n_taps] device array (any taps; symmetry is neither required nor used), y: [n_rec][m][y_ld] through
 * y_rec_stride, columns >= ceil(T / q) are not written.  Rows are independent: m has no upper limit here.
 * float64; every output is one chain of FMAs over the taps in ascending j starting from +0.0, so its bits depend on its
 * own taps and samples only -- not on the tile, the row, the batch or the strides -- and a NaN at sample s reaches exactly
 * the outputs with |k q - s| <= H.  The reference's forward / backward fill of gaps (src/data_structures.py:779-797) is not
 * part of this call.
 * hmv_decimate_out_len: ceil(T / q); -1 for T < 1 or q outside 2..HMV_MAX_DECIMATE.
 * hmv_decimate_tile: outputs per workgroup for these q and n_taps (1024, 512 or 256; -1 for arguments the call refuses).
 * Refused before any launch: q outside 2..HMV_MAX_DECIMATE (-1), n_taps even or outside 3..HMV_MAX_DECIMATE_TAPS (-2),
 *   T < 1, n_rec < 0 or m < 1 (-3), T > 2^40 (-7), a null pointer (-4), ld < T (-5), y_ld < ceil(T / q) (-6).  n_rec = 0
 *   launches nothing and returns 0. */
#define HMV_MAX_DECIMATE 32
#define HMV_MAX_DECIMATE_TAPS 641      /* 20 * HMV_MAX_DECIMATE + 1 */
int64_t hmv_decimate_out_len(int64_t T, int q);
int hmv_decimate_tile(int q, int n_taps);
int hmv_decimate_fir_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m, int q,
                         const double* h, int n_taps, double* y, int64_t y_rec_stride, int64_t y_ld, void* stream);

/* Phase synchrony of analytic signals per window (csrc/phase_sync.hip): PLV, ciPLV, coherence and imaginary coherence.
 * The reference forms the analytic signal on the host (sosfiltfilt, then hilbert: src/eeg_alpha_ibi_ffdtf.py:271-365,
 * src/warsaw_pilot_data.py:269-283); here it is eeg_io.band_response / Engine.analytic_signal, and this entry is the
 * per-window statistic.  z: [n_rec][m][ld] complex128 as interleaved (re, im) doubles, 16-byte aligned, T samples used;
 * rec_stride and ld are counted in COMPLEX elements.  Item i is the window of n samples of recording item_rec[i] that
 * starts at item_start[i] (device arrays; keeping start + n <= T is the caller's -- a sample outside the recording is
 * read as zero, never from memory).  With channels i, j < m:
 *     mode HMV_PHASE_UNIT:  u_i[t] = z_i[t] / |z_i[t]|   (0 where |z_i[t]| == 0)
 *     mode HMV_PHASE_RAW:   u_i[t] = z_i[t]
 *     C_ij = sum_t u_i[t] conj(u_j[t]):   Re C_ij = sum re_i re_j + im_i im_j,   Im C_ij = sum im_i re_j - re_i im_j
 *     UNIT:  R_ij = C_ij / n                   mag = |R| (PLV)         lagged = ciPLV
 *     RAW:   R_ij = C_ij / sqrt(C_ii C_jj)     mag = |R| (coherence)   lagged = |Im R| (imaginary coherence)
 *     ciPLV = den > 0 ? min(1, |Im R| / sqrt(den)) : 0,   den = 1 - (Re R)^2
 *     diagonal: Im R = 0; mag = 1 and lagged = 0 where the channel has a non-zero sample in the window.
 * coherency (optional): [n_items][2][m][m], the planes Re R and Im R; mag, lagged (optional): [n_items][m][m]; unpadded.
 * info int32 [n_items]: 0 fine; 1 a non-finite sample in the window's m channels (read off the diagonal of C): every
 *   output of the item is NaN; 2 (RAW only) a channel of zero power: its row and column are NaN, the rest is valid.
 * float64 on v_mfma_f64_4x4x4_4b_f64.  Every sum runs over the samples ascending in k-steps of 4 from the window start:
 * an item's bits depend on its own samples only, not on the batch, the item order, the strides or the padded channel
 * count.  No atomics.  Element (r, c) is formed from C[min(r,c)][max(r,c)]: mag and lagged are exactly symmetric, Im R
 * exactly antisymmetric.  In UNIT mode scaling a channel of z by a power of two changes no bit (while |z|^2 stays in the
 * normal range).
 * Refused before any launch: channel count outside 1..HMV_MAX_CHANNELS (-1), n < 1 or n > T (-2), T < 1, n_rec < 0 or
 *   n_items < 0 (-3), more than 2^31 - 1 items (-10), mode outside 0..1 (-7), all three outputs null (-9), ld < T (-5),
 *   rec_stride < m * ld (-6), and with n_items > 0 a null z, item table or info (-4) or a z that is not 16-byte aligned
 *   (-8).  n_items = 0 launches nothing and returns 0. */
#define HMV_PHASE_UNIT 0
#define HMV_PHASE_RAW  1
int hmv_phase_sync_c128(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m,
                        const int64_t* item_rec, const int64_t* item_start, int64_t n_items, int n, int mode,
                        double* coherency, double* mag, double* lagged, int32_t* info, void* stream);
/* The pairs form of hmv_phase_sync_c128, for the null tests of the inter-brain cells: item `it` is the m x n block whose
 * channels c < split are z[rec_a[it]][c][item_start[it] + t] and whose channels c >= split are
 * z[rec_b[it]][c][(item_start[it] + shift_b[it] + t) mod T], t = 0..n-1 (shift_b = NULL: 0).  Because the analytic signal is
 * a circular filter of the recording, this is the window of the recording whose second participant was shifted by shift_b
 * samples (rec_b = rec_a), or of the pseudo dyad A of rec_a with B of rec_b (shift 0), and no such recording is written.
 * z, rec_stride, ld, T, n_rec, m, n, mode and the definitions of mag and lagged as above; rec_a, rec_b, item_start, shift_b
 * are device arrays [n_items] whose contents the caller has checked (rec in 0..n_rec-1, 0 <= start, start + n <= T, shift
 * in 0..T-1).  A side of an item whose entries would address outside its recording is read as zeros, never from memory.
 * Only the cross cells (r < split <= c, and their mirror) are computed: the tiles of the full form that hold one, with its
 * products in its order, so a cross cell has the bits hmv_phase_sync_c128 gives for the same block written out as one
 * recording.  RAW mode also computes the diagonal tiles, for C_ii and C_jj with those same bits.
 * values: [n_items][m][m][val_stride] doubles, the layout hmv_null_accumulate_f64 reads (val_stride its n_bands).  mag goes
 *   to column col_mag and lagged to column col_lagged of every cell of the item; a column of -1: that output is not wanted.
 *   (r, c) and (c, r) of a cross pair get the same bits; in the written columns every untested cell (both indices on one
 *   side of split, the diagonal included) gets NaN; the other columns are not touched.  There is no coherency output.
 * info int32 [n_items]: as above and, for an item whose entries are valid, the value hmv_phase_sync_c128 reports on the
 *   written-out block.  1: a non-finite sample in any of the m channels as read (B through its shift) -- every written
 *   value of the item is NaN; read off the diagonal of C in RAW mode and off the staged phasors in UNIT mode, which has no
 *   diagonal tile.  2 (RAW only): a channel of zero power; its row and column are NaN, the rest is valid.
 * No atomics; every sum runs over the samples ascending in k-steps of 4 from the window start; an item's bits depend on its
 * own samples only.
 * Refused before any launch: channel count outside 1..HMV_MAX_CHANNELS (-1), n < 1 or n > T (-2), T < 1, n_rec < 0 or
 *   n_items < 0 (-3), more than 2^31 - 1 items (-10), mode outside 0..1 (-7), split outside 1..m-1 (-11), val_stride < 1, a
 *   column outside -1..val_stride-1, both columns -1 or both columns equal (-12), ld < T (-5), rec_stride < m * ld (-6), and
 *   with n_items > 0 a null z, rec_a, rec_b, item_start, values or info (-4) or a z that is not 16-byte aligned (-8).
 *   n_items = 0 launches nothing and returns 0. */
int hmv_phase_sync_pairs_c128(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m, int split,
                              const int64_t* rec_a, const int64_t* rec_b, const int64_t* item_start, const int64_t* shift_b,
                              int64_t n_items, int n, int mode, double* values, int val_stride, int col_mag, int col_lagged,
                              int32_t* info, void* stream);

/* The phase-lag family of analytic signals per window (csrc/phase_lag.hip): the phase-lag index (PLI; Stam, Nolte &
 * Daffertshofer 2007, Hum Brain Mapp 28:1178), the weighted PLI and the debiased squared weighted PLI (Vinck, Oostenveld,
 * van Wingerden, Battaglia & Pennartz 2011, NeuroImage 55:1548).  THIS IS NOT A FUNCTION OF THE REFERENCE, which has no
 * phase-lag measure; it is here because zero-lag mixing (common reference, volume conduction, a shared artefact) cannot
 * raise these measures, while it raises PLV and coherence.
 * z, rec_stride, ld, T, n_rec, m, item_rec, item_start, n_items, n as for hmv_phase_sync_c128: item `it` is the window
 * z[item_rec[it]][c][item_start[it] + t], t = 0..n-1, a sample past T read as zero, never from memory.  No normalisation:
 * the measures use z itself.  For channels i != j:
 *     x[t]  = rn( rn(im_i[t] re_j[t]) - rn(re_i[t] im_j[t]) )   = Im(z_i conj z_j): two rounded products and one
 *                                                                 subtraction, never contracted into an FMA
 *     P = #{t : x[t] > 0}   N = #{t : x[t] < 0}   S = sum x[t]   A = sum |x[t]|   Q = sum x[t]^2
 *     pli   = |P - N| / n
 *     wpli  = |S| / A                      NaN where A == 0
 *     dwpli = (S^2 - Q) / (A^2 - Q)        NaN where A^2 - Q <= 0 (n = 1, or one non-zero sample); may be slightly
 *                                          negative, not clamped
 *     diagonal: 0 for all three.
 * The unfused x is deliberate: NumPy computes the same x bit for bit, so P and N and with them PLI are exactly
 * reproducible, and two identical or power-of-two-proportional channels give x = 0 exactly (PLI 0, wPLI NaN) where a fused
 * form would leave rounding residue of random sign.  S, A and Q are summed over t ascending from the window start, one
 * term after the other (Q by one FMA per term): the bits of cell (i, j) depend on the n samples of channels i and j only --
 * not on the batch, the item index, the other channels, m or split.  Each pair is computed once and mirrored: the three
 * outputs are symmetric bit for bit.  S and A run in the same order, so |S| <= A holds in floating point and wpli lies in
 * [0, 1] exactly.  A power-of-two scaling of a channel changes no bit (no over- or underflow assumed).
 * split = 0: all pairs.  1 <= split <= m-1: only the inter-brain pairs (i < split <= j) are computed, with the bits the
 *   split = 0 call gives them; every other off-diagonal cell is NaN.
 * pli, wpli, dwpli: [n_items][m][m], unpadded; any may be NULL, not all three.  Nothing else is written.
 * info int32 [n_items]: 1 a non-finite sample in any of the m channels of the window (flagged while staging): everything
 *   of the item is NaN; 2 some computed off-diagonal pair has A == 0 (a flat channel, duplicated channels): those cells
 *   have pli = 0 and wpli = dwpli = NaN, the rest is valid; 0 otherwise.
 * float64 VALU, no atomics.
 * Refused before any launch: channel count outside 1..HMV_MAX_CHANNELS (-1), n < 1 or n > T (-2), T < 1, n_rec < 0 or
 *   n_items < 0 (-3), more than 2^31 - 1 items (-10), split outside 0..m-1 (-11), all three outputs null (-9), ld < T (-5),
 *   rec_stride < m * ld (-6), and with n_items > 0 a null z, item table or info (-4) or a z that is not 16-byte aligned
 *   (-8).  n_items = 0 launches nothing and returns 0. */
int hmv_phase_lag_c128(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m, int split,
                       const int64_t* item_rec, const int64_t* item_start, int64_t n_items, int n,
                       double* pli, double* wpli, double* dwpli, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYPERMVAR_H */
