// Internal launch interface between the C-ABI (capi.hip) and the kernels.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hmv {

// ---- tuning knobs (capi.hip; include/hypermvar.h hmv_set_tuning).  Read by the launchers, never by kernels.
long long tuning(int key);

// ---- K1 lag covariance ------------------------------------------------------------------------
struct LagcovArgs {
  const double* x;          // [n_rec][m][ld]  (channel-major, sample-contiguous)
  long long rec_stride;     // doubles between recordings
  long long ld;             // doubles between channels
  const long long* item_rec;    // [n_items] recording index of each window (device)
  const long long* item_start;  // [n_items] first sample of each window (device)
  long long n_items;
  int m, n, p;              // channels, window length, model order
  double* R;                // [n_items][p+1][MP][MP]
  // hop-block mode (blocks != 0): item b is the block of `n` (= hop) samples starting at blk_first + b * n of ONE
  // recording x (item_rec / item_start unused); lagged partners beyond the block are read up to the end of the
  // recording (blk_T samples), the sums are left unscaled and the padding is left zero: R = partial sums Q_l(b).
  int blocks;
  long long blk_first, blk_T;
};
int launch_lagcov(const LagcovArgs& a, int m_pad, hipStream_t st);
// windows of k consecutive hop blocks from the block sums: R[w][l] = (sum_{j<k} Q[w+j][l] - C_l(w)) / n
struct LagcombArgs {
  const double* Q;          // [n_win + k - 1][p+1][MP][MP]
  const double* x;          // the recording: [m][ld]
  long long ld, first, hop, T;
  long long n_win;
  int k, m, p;
  double* R;                // [n_win][p+1][MP][MP]
};
int launch_lagcomb(const LagcombArgs& a, int m_pad, hipStream_t st);
// K1 of an event-locked ensemble (lagcov_ensemble.hip): trials (trial_rec, trial_start) in groups (CSR group_ptr), item =
// (group, offset from every trial start of the group); R = the mean over the group's trials of the window's lag
// covariances.  Every index array lives on the device.
struct LagcovEnsArgs {
  const double* x;          // [n_rec][m][ld]
  long long rec_stride, ld;
  long long T;              // samples per recording (shared form: lagged partners past it count as zero)
  const long long* trial_rec;     // [n_trials]
  const long long* trial_start;   // [n_trials]
  const long long* group_ptr;     // [n_groups + 1]
  const long long* item_group;    // [n_items]  } direct form only, of the items of THIS launch
  const long long* item_offset;   // [n_items]  }
  long long n_items;        // items of this launch
  int m, n, p;
  double* R;                // [n_items][p+1][MP][MP]
  // shared-overlap form: the items of this launch are it0 .. it0 + n_items - 1 of the grid item = g * nwin + w, window w
  // at offset w * hop, n = k * hop
  long long it0, nwin, hop;
  int k;
  double* Q;                // scratch, lagcov_ensemble_q_tiles() * (p+1) * MP * MP doubles
  // second trial table (launch_lagcov_ensemble_split only; direct form): trial step e reads the channels >= split from
  // trial (trial_rec_b[e], trial_start_b[e]), indexed through the same group_ptr
  const long long* trial_rec_b;   // [n_trials]
  const long long* trial_start_b; // [n_trials]
  int split;                // 1 .. m - 1
  // optional, both or neither: the within-participant elements are copied from R_base[item_base[item]], not computed
  const double* R_base;     // [n_base][p+1][MP][MP]
  const long long* item_base;     // [n_items], of the items of THIS launch
};
bool lagcov_ensemble_shared_ok(int n, long long hop, int p, int max_k);      // does the shared form take this grid?
long long lagcov_ensemble_q_tiles(long long n_items, long long nwin, int k);  // in stacks of (p+1) tiles
int launch_lagcov_ensemble(const LagcovEnsArgs& a, int m_pad, bool shared, hipStream_t st);
int launch_lagcov_ensemble_split(const LagcovEnsArgs& a, int m_pad, hipStream_t st);   // direct form, two trial tables
// K1 for pairs of recordings (lagcov_ensemble.hip, lagcov_pairs_kernel): item `it` is the window of n samples starting at
// item_start[it], its channels < split read from recording rec_a[it] and its channels >= split from recording rec_b[it].
// lagcov_kernel's mapping, chunks and order of products; optionally the two within-participant blocks are copied from two
// different base stacks and only the cross elements are computed.
struct LagcovPairsArgs {
  const double* x;          // [n_rec][m][ld]
  long long rec_stride, ld;
  const long long* rec_a;       // [n_items]  } of the items of THIS launch (device)
  const long long* rec_b;       // [n_items]  }
  const long long* item_start;  // [n_items]  }
  long long n_items;
  int m, n, p, split;       // split: 1 .. m - 1
  double* R;                // [n_items][p+1][MP][MP]
  // optional, all three or none: elements with both indices < split are copied from R_base[base_a[it]], elements with both
  // indices >= split (padding included) from R_base[base_b[it]]
  const double* R_base;     // [n_base][p+1][MP][MP]
  const long long* base_a;  // [n_items], of the items of THIS launch
  const long long* base_b;  // [n_items]
};
int launch_lagcov_pairs(const LagcovPairsArgs& a, int m_pad, hipStream_t st);
// K1 as a weighted sum over trials (lagcov_mix.hip): item k * n_win + w of the whole call is mix row k at window w,
// R = scale[k] * sum_e W[k][e] * Rt[e][w], trials ascending; the padding is written, not read.
struct LagcovMixArgs {
  const double* Rt;         // [n_trials][n_win][p+1][MP][MP], 16-byte aligned
  const double* W;          // [n_mix][n_trials]
  const double* scale;      // [n_mix], or null for 1
  long long n_trials, n_win;
  long long it0, n_items;   // the items of THIS launch: it0 .. it0 + n_items - 1 (may start or end inside a row)
  int m, m_pad, p;
  double* R;                // [n_items][p+1][MP][MP] of the items of this launch, 16-byte aligned
};
int launch_lagcov_mix(const LagcovMixArgs& a, hipStream_t st);

// ---- K2 Yule-Walker solve (block LDL^T of the block-Toeplitz normal equations) ------------------
struct YwArgs {
  const double* R;          // [n_items][p+1][MP][MP]
  long long n_items;
  int m, p;
  double* ws;               // [n_items][ws_tiles(p)][MP][MP] scratch
  double* ar;               // [n_items][MP][MP][p]   (row, col, lag) -- lag fastest
  double* V;                // [n_items][MP][MP]
  double* Vq_logdet;        // optional [n_items][p]: log det V_q for q = 1..p (model-order criterion)
  int* info;                // [n_items]
  int tiled;                // block LDL^T forms (yw_solve.hip): 0: one workgroup per window, one launch;  1: one workgroup
                            // per tile, p + 2 launches;  -1: no form asked for -- the block Levinson-Whittle recursion
                            // (yw_lwr.hip) unless HMV_TUNE_YW_FORM says otherwise
  int only_guarded;         // internal: the one-launch LDL^T kernel re-solves only the windows the recursion flagged
  // per-window order (one-launch LDL^T kernel only; nullptr: the uniform order p).  Window `item` is solved at order[item]
  // <= p from the first order[item] + 1 lag blocks of its [p+1]-strided R, in its ws_tiles(p)-strided scratch, and its
  // [MP][MP][p] coefficients are written with the lags >= order[item] as +0.0.
  const int* order;
  // internal (fused sliding path -- capi.hip, sliding_k2 where the plan says from_tiles --, default recursion only): the
  // recursion does not write `ar`; the model stays in the final A generation's tiles of `ws` ([k][row][col] at tile
  // (p & 1) * p), where the packing kernel of K3 reads it.  Windows re-solved by the LDL^T kernel still get their `ar`
  // (their scratch is overwritten), flagged by the guard word.
  int no_emit;
  // pivoted fallback (HMV_FLAG_YW_PIVOTED): behind the solver above, the windows it left with info != 0 are solved again
  // by the dense LU with partial pivoting (yw_lu.hip), which overwrites their ar, V and info and sets their route word to 2
  int pivoted;
};
// automatic model order (yw_auto.hip only; a struct of its own so that the fixed-order kernels' arguments stay as they
// were): YwArgs::p is the largest order tried, criterion of order q = log det Vf_q + crit_c * q * m^2 / n
// (crit_c = 2: AIC, 2 log log n: HQ, log n: SC)
struct YwAutoArgs {
  int n;                    // window length
  double crit_c;
  int* order_out;           // [n_items] selected order, 0 for a failed window
  double* crit_out;         // optional [n_items][p]
};
long long yw_ws_tiles(int p);
// Which LDL^T form a batch takes where none is asked for: the launch chain (true) or one launch (false).  One launch per
// batch is the low-latency form (small batches, small tiles).  At 64 channels and hundreds of windows both forms are
// bound by the same HBM traffic (~14 MB of tile operands per window, far more than any cache holds for a resident
// batch) and the launch chain, whose every launch streams with the whole chip, is the faster one: 2.0 ms against 2.26 ms
// for 599 windows (profiles/r02_ab_notes.md).  The one rule for launch_yw, the fused sliding step's chunks and the
// restricted fits of block Granger causality (each block by its own padded size).
inline bool yw_chain_by_shape(int m_pad, long long n_items) { return m_pad == 64 && n_items >= 128; }
int launch_yw(const YwArgs& a, int m_pad, hipStream_t st);
int launch_yw_lwr(const YwArgs& a, int m_pad, hipStream_t st);
// yw_lu.hip: the LU over every window (all != 0) or over the windows whose info is not zero; the route word (the last int
// of a window's scratch: 0 recursion, 1 LDL^T, 2 LU) set for a whole batch, and copied out
int launch_yw_lu(const YwArgs& a, int m_pad, int all, hipStream_t st);
int launch_yw_route_set(double* ws, long long n_items, int m_pad, int p, int value, hipStream_t st);
int launch_yw_routes(const double* ws, long long n_items, int m_pad, int p, int* route, hipStream_t st);
// how many workgroups (= windows) of the default recursion one compute unit holds at once, from the runtime; 0: unknown
int yw_lwr_occupancy(int m_pad);
int launch_yw_lwr2(const YwArgs& a, int m_pad, hipStream_t st);
// K2 with on-device order selection: the recursion to order p with criterion, first arg-min and snapshot, then the LDL^T
// re-solve of the guarded windows at their own orders
int launch_yw_auto(const YwArgs& a, const YwAutoArgs& s, int m_pad, hipStream_t st);
// internal: the one-launch LDL^T kernel over the windows flagged in the scratch, at order[item] (yw_solve.hip)
int launch_yw_guarded(const YwArgs& a, int m_pad, hipStream_t st);

// ---- K3 transfer matrix inverse ---------------------------------------------------------------
struct TfArgs {
  const double* ar;         // [n_items][MP][MP][p]  (reference layout; read by the packing kernel only)
  const double* arx;        // scratch, tf_workspace_doubles(): the same coefficients in K3's register order
  const double* tw;         // [F][p][2]
  const double* Zin;        // general inverse only: complex [n_items][F][MP][MP] (ar / arx / tw unused)
  double* detph;            // general inverse only, optional: [n_items*F][2] det / |det| incl. interchange sign
  double* P;                // optional [n_items][F][MP][MP]
  double* rowsum;           // required with P: [n_items][F][MP]
  double* H;                // optional complex [n_items][F][MP][MP]
  double* A;                // optional complex [n_items][F][MP][MP]
  int* info;                // [n_items*F]
  long long n_items;
  int F, p, m;
  double tau;               // pivot threshold: 1.0 = LAPACK partial pivoting
  // ffDTF normalisation inside K3 (hot path only; ff == nullptr: off).  Items < fuse_items publish their |H|^2
  // row-major; row i of item w < tail0 is normalised in-kernel by a workgroup of item w + lag, the rows of items
  // tail0 .. fuse_items - 1 (the last `lag` of the batch) by norm_missed_kernel right behind K3; the caller runs K4
  // on the items >= fuse_items (none on the hot path).
  double* ff;               // [n_items][m][m][F]
  double* den;              // [n_items][MP]
  int* wcount;              // [n_items] arrival counters          } one block of 2 * n_items + 1 ints that the
  int* ready;               // [n_items] denominators are in place  } launcher zeroes, followed by the list
  int* missed;              // [1 + fuse_items * MP] count, rows     } of rows left to norm_missed_kernel
  long long fuse_items;
  int lag;                  // (tail0 = max(0, fuse_items - lag): no field of its own -- the hand-scheduled K3 has no SGPR to spare)
  // reduced product (hot path, in-kernel normalisation only; bands == nullptr: off): instead of the ffDTF array the row
  // workers write its band sums, bands[item][i][j][b] = sum_{band_lo[b] <= f < band_hi[b]} ffdtf[item][i][j][f]
  // (the arithmetic of band_sums_stream_kernel, ffdtf_norm.hip: same partial sums, same tree, same bits); ff is unused
  double* bands;            // [n_items][m][m][nb]
  const int* band_lo;       // [nb] device
  const int* band_hi;       // [nb] device
  int nb;
  unsigned long long* stamps;   // diagnostic builds (-DHMV_STAMP) only: [wave][8] phase cycle sums; else null
  // K3 of one batch in two launches (launch_tf_inv with a TfSplit): workgroup b of a launch is (item, frequency)
  // item0 * F + b of the batch.  Every array, n_items, fuse_items and lag stay those of the whole batch.
  int item0;
};
// K3 of one batch in two launches on `st`: items [0, c0), then -- once `join` has happened (the event behind whatever
// produces the model of the items >= c0 on another stream) -- items [c0, n_items).  One protocol: one memset ahead of the
// first launch, the second launch's first workgroups normalise the first launch's last windows (complete by stream
// order), one set of tail windows, one norm_missed_kernel.  `joined` comes back true once `st` waits for `join`.
struct TfSplit {
  long long c0 = 0;
  hipEvent_t join = nullptr;
  bool joined = false;
};
int launch_twiddles(const double* freqs, int F, double fs, int p, double* tw, hipStream_t st);
// yw_ws (optional): K2's scratch of the same items, left by a recursion that did not emit (YwArgs::no_emit).  The packing
// kernel then takes window `item` from its final A generation's tiles, or from `ar` if its guard word says that the LDL^T
// re-solve wrote it.
int launch_tf_inv(const TfArgs& a, int m_pad, hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                  const double* yw_ws = nullptr, TfSplit* split = nullptr);
int launch_cinv(const TfArgs& a, int m_pad, hipStream_t st);
long long tf_workspace_doubles(long long n_items, int m_pad, int p);
int tf_band_max_F(int m_pad);

// ---- K4 ffDTF normalisation + layout transposes -------------------------------------------------
struct NormArgs {
  const double* P;          // [n_items][F][MP][MP]
  const double* rowsum;     // [n_items][F][MP]
  double* den;              // [n_items][MP] scratch/out: sum_f rowsum
  double* out;              // [n_items][m][m][F]
  long long n_items;
  int F, m, m_pad;
  int normalise;            // 1: ffDTF, 0: plain |H|^2 (dtf_multivariate)
};
int launch_ffdtf_norm(const NormArgs& a, hipStream_t st);

int launch_trial_mean(const double* in, double* out, long long n, int trials, hipStream_t st);
int launch_ddtf(const double* ff, const double* kappa, double* out, long long n, hipStream_t st);
int launch_band_sums(const double* in, const int* lo, const int* hi, double* out, long long rows, int F, int nb,
                     hipStream_t st);

// complex [n_items][F][MP][MP] -> complex [n_items][m][m][F]
int launch_transpose_c128(const double* in, double* out, long long n_items, int F, int m, int m_pad, hipStream_t st);

// ---- K5 spectra S(f) = H V H^T (plain transpose) ---------------------------------------------------
struct SpecArgs {
  const double* H;          // complex [n_items][F][MP][MP]
  const double* V;          // [n_items][MP][MP]
  double* S;                // complex [n_items][F][MP][MP] (kernel-natural), or
  double* S_mmf;            // complex [n_items][m][m][F], the reference's array layout, written by the kernel itself
  long long n_items;
  int F, m;
  int sym;                  // 1: V is symmetric (this library's own fit) -- with S_mmf only the upper triangle is computed
};
int launch_spectra(const SpecArgs& a, int m_pad, hipStream_t st);

// ---- measures on top of K3 / K5 (connect.hip) -----------------------------------------------------------
int launch_pack_c128(const double* in, double* out, long long n_items, int F, int m, int m_pad, hipStream_t st);
int launch_pcoh(const double* Sinv, const double* detph, double* out, long long n_items, int F, int m, int m_pad, hipStream_t st);
int launch_gpdc(const double* A, const double* V, double* out, long long n_items, int F, int m, int m_pad, hipStream_t st);

// ---- sliding-window dDTF / GPDC (sliding_conn.hip) --------------------------------------------------------------
struct DdtfArgs {
  const double* ar;         // [n_items][MP][MP][p]   K2
  const double* V;          // [n_items][MP][MP]      K2 (symmetric)
  int* info_yw;             // [n_items]: set to -(column + 1) where V is not positive definite (and was 0)
  double* B;                // scratch [n_items][p+1][MP][MP]: L^-1 A_k
  double* G;                // scratch [n_items][2p+1][MP][MP]: coefficients of W(f) = A^T V^-1 A
  const double* freqs;      // [F] device
  double fs;
  const double* ff;         // [n_items][m][m][F]     ffDTF of K3's fused path
  double* out;              // [n_items][m][m][F]     dDTF (may be ff)
  long long n_items;
  int F, m, p;
};
int launch_ddtf_sliding(const DdtfArgs& a, int m_pad, hipStream_t st);
// ddtf_factor_kernel on its own: B [item][p+1][MP][MP] = L^-1 A_k with V = L L^T; info_yw as DdtfArgs
int launch_ddtf_factor(const double* ar, const double* V, int* info_yw, double* B, long long n_items, int m, int m_pad, int p,
                       hipStream_t st);
int launch_gpdc_sliding(const double* ar, const double* V, const double* tw, double* out, long long n_items, int F, int m,
                        int m_pad, int p, hipStream_t st);

// ---- block Granger causality between the channels < split and the channels >= split (block_gc.hip) -------------------
// the two restricted lag-covariance stacks, each in the MP layout of its own block size, with K1's padding
int launch_bgc_gather(const double* R, double* Ra, double* Rb, long long n_items, int m, int m_pad, int p, int split,
                      hipStream_t st);
// The one layout rule of the stage, for the workspace layout and both launchers: the blocks' own MP (padded to 16, as
// hmv_pad) and NSP, the larger of the two, the row length of C and D.  1 <= split <= m - 1 <= 63 is the caller's check.
struct BgcPads {
  int mpa, mpb, nsp;
};
inline BgcPads bgc_pads(int m, int split) {
  const int mpa = ((split + 15) / 16) * 16, mpb = ((m - split + 15) / 16) * 16;
  return BgcPads{mpa, mpb, mpa > mpb ? mpa : mpb};
}
// The time-domain part of the stage: where the restricted fits come from and where the values go.  All null: no such part.
struct BgcRed {
  // the restricted fits' residual covariances and K2 infos ...
  const double* VrA;        // [n_items][MPa][MPa]
  const double* VrB;        // [n_items][MPb][MPb]
  const int* info_rA;       // [n_items]
  const int* info_rB;       // [n_items]
  // ... or (red_base != nullptr, the four above unused) their log-determinants and infos as an earlier call left them in
  // red_out / info_red: block A's from row base_a[item], column 0, block B's from row base_b[item], column 1
  const double* red_base;   // [n_base][2]
  const int* info_red_base; // [n_base][2]
  const long long* base_a;  // [n_items]
  const long long* base_b;  // [n_items]
  double* time;             // [n_items][4]
  int* info_red;            // [n_items][2]
  double* red_out;          // [n_items][2] or null: (ln det Sr_AA, ln det Sr_BB) as the time values use them
};
struct BgcArgs {
  const double* ar;         // [n_items][MP][MP][p]   K2
  const double* V;          // [n_items][MP][MP]      K2 (symmetric)
  int* info_yw;             // [n_items]: set to -(column + 1) where V, one of its diagonal blocks or a Schur complement
                            // Sigma_{s|d} is not positive definite (and the entry was 0); column counted in V
  double* B;                // scratch [n_items][p+1][MP][MP]
  double* C;                // scratch [n_items][2][p+1][NSP][NSP]: coefficients of W_ss(f), per direction
  double* D;                // scratch [n_items][2][p+1][NSP][NSP]: coefficients of At_ss(f), per direction
  double* cst;              // scratch [n_items][2]: ln det Sigma_{s|d}
  const double* tw;         // [F][p][2]
  double* out;              // [n_items][2][F]: 0 = A -> B, 1 = B -> A
  int* info_gc;             // [n_items*F]
  BgcRed red;               // time domain (VrA and red_base null: none of it)
  int want;                 // bit 0 spectral, bit 1 time; 0: spectral, and time where `red` has a source.  Without bit 0
                            // only V, info_yw and `red` are used (bgc_time_kernel alone), without bit 1 `red` is ignored
  long long n_items;
  int F, m, p, split;
};
int launch_bgc(const BgcArgs& a, int m_pad, hipStream_t st);

// ---- multitaper PSD (psd.hip; hipFFT for the transforms) -------------------------------------------------
long long psd_workspace_bytes(long long ch_chunk, long long n, int K);
int launch_psd(const double* x, long long n_ch, long long n, long long ld, const double* tapers, const double* w, int K,
               long long lo, long long hi, double* psd, void* workspace, long long ch_chunk, hipStream_t st);

// ---- DPSS tapers (dpss.hip; hipFFT for the concentration ratios) -------------------------------------------------
long long dpss_workspace_bytes(long long M, int K, int sym);
int launch_dpss(long long M, double NW, int K, int sym, double* tapers, double* ratios, void* workspace, hipStream_t st);

// ---- FAD decomposition of univariate AR models (fad.hip) ------------------------------------------------------------
struct FadArgs {
  int from_fit;             // 1: fit from samples first (fad_fit_kernel), 0: decompose the given coefficients
  // fit: series s = item * m + ch is channel ch of window `item` (addressing as LagcovArgs)
  const double* x;
  long long rec_stride, ld;
  const long long* item_rec;
  const long long* item_start;
  long long n_series;
  int m, n;
  int pmax;                 // row length of every [series][pmax] array (decomposition only: the order p)
  int order;                // fit: 0 = automatic (criterion `crit`: 0 AIC, 1 HQ, 2 SC), else the fixed order
  int crit;
  double fs, imag_tol;
  int pair_conjugates;
  int* order_out;           // [S] (fit only)
  double* crit_out;         // [S][pmax] optional (fit only)
  double* ar;               // [S][pmax]: written by the fit, read by the decomposition
  double* noise;            // [S] (fit only)
  double* poles;            // complex [S][pmax]
  double* C;                // complex [S][pmax]
  double* alpha;            // complex [S][pmax]
  double* freq, *beta, *bw, *phi, *B;   // [S][pmax]
  unsigned char* osc;       // [S][pmax]
  int* paired;              // [S][pmax]
  int* n_paired;            // [S]
  int* info;                // [S]
};
int launch_fad(const FadArgs& a, hipStream_t st);

// ---- surrogate significance (surrogate.hip) ---------------------------------------------------------------------
int launch_surrogate_shift(const double* x, long long rec_stride, long long ld, long long T, const long long* item_rec,
                           const long long* item_start, long long n_win, const long long* shift, long long n_rec, int n_surr,
                           int m, int n, int split, double* out, hipStream_t st);
int launch_surrogate_phase(const double* spec, long long n_win, const double* phi, int n_surr, int m, int n, double* out,
                           hipStream_t st);
struct NullAccArgs {
  const double* obs;          // [n_win][m][m][nb]
  const double* surr;         // [n_surr][n_win][m][m][nb]
  const unsigned char* bad;   // [n_surr][n_win]: the surrogate's fit failed
  const unsigned char* tested;  // [m][m]
  long long n_win;
  int n_surr, m, nb;
  double* M;                  // [n_surr][n_win][nb] out
  int* n_valid;               // [n_win]            running state
  int* cnt, *cnt_fwe, *n_cell;  // [n_win][m][m][nb]  running state
  double* mean, *m2;          // [n_win][m][m][nb]  running state
  double* p, *p_fwe, *null_mean, *null_std;   // [n_win][m][m][nb] out, optional (all or none)
};
int launch_null_accumulate(const NullAccArgs& a, hipStream_t st);

// ---- model validation: residuals and whiteness statistics (validate.hip) ----------------------------------------
struct ResidArgs {
  const double* x;          // [n_rec][m][ld]; windows addressed as LagcovArgs
  long long rec_stride, ld;
  const long long* item_rec;
  const long long* item_start;
  long long n_items;
  int m, n, p;
  const double* ar;         // [n_items][MP][MP][p]  (K2's layout; read by the packing kernel only)
  double* arp;              // scratch, resid_pack_doubles(): the coefficients in the A-operand order of resid_kernel
  double* E;                // [n_items][m][ldE], columns 0 .. n - p - 1 written
  long long ldE;
};
long long resid_pack_doubles(long long n_items, int m_pad, int p);
int launch_residuals(const ResidArgs& a, int m_pad, hipStream_t st);
// item_rec[i] = i, item_start[i] = 0: the residuals of a chunk as n recordings for launch_lagcov
int launch_iota_items(long long* item_rec, long long* item_start, long long n, hipStream_t st);
struct WhiteArgs {
  const double* C;          // [n_items][h+1][MP][MP]
  long long n_items;
  int m, N, h;
  double acf_thr;
  double* s;                // [n_items][h]
  double* q;                // [n_items][3]
  double* q_ch;             // [n_items][m]
  int* acf_count;           // [n_items]
  int* info;                // [n_items]
  double* resid_cov;        // optional [n_items][MP][MP]: a copy of C_0
};
int launch_whiteness(const WhiteArgs& a, int m_pad, hipStream_t st);

// ---- FIR decimation of recordings (decimate.hip) ------------------------------------------------------------------
struct DecimateArgs {
  const double* x;          // [n_rec][m][ld], T samples used
  long long rec_stride, ld, T, n_rec;
  int m, q;
  const double* h;          // [n_taps]
  int n_taps;
  double* y;                // [n_rec][m][y_ld], ceil(T / q) samples written
  long long y_rec_stride, y_ld;
};
int decimate_tile(int q, int n_taps);      // outputs per workgroup
int launch_decimate(const DecimateArgs& a, hipStream_t st);

// ---- phase synchrony of analytic signals (phase_sync.hip) ---------------------------------------------------------
struct PhaseSyncArgs {
  const double2* z;         // [n_rec][m][ld] complex (re, im), strides in complex elements; T samples used
  long long rec_stride, ld, T, n_rec;
  const long long* item_rec;    // [n_items] (device)
  const long long* item_start;  // [n_items] (device)
  long long n_items;
  int m, n, mode;           // channels, window length, HMV_PHASE_UNIT / HMV_PHASE_RAW
  double* coherency;        // optional [n_items][2][m][m]
  double* mag;              // optional [n_items][m][m]
  double* lagged;           // optional [n_items][m][m]
  int* info;                // [n_items]
};
int launch_phase_sync(const PhaseSyncArgs& a, int m_pad, hipStream_t st);
// the pairs form: channels < split of recording rec_a[it] against channels >= split of recording rec_b[it], read
// shift_b[it] samples later modulo T; the cross cells only, written into columns of a [n_items][m][m][val_stride] buffer
struct PhasePairsArgs {
  const double2* z;         // as PhaseSyncArgs
  long long rec_stride, ld, T, n_rec;
  const long long* rec_a;       // [n_items] (device)
  const long long* rec_b;       // [n_items] (device)
  const long long* item_start;  // [n_items] (device)
  const long long* shift_b;     // optional [n_items] (device), in 0..T-1; null: 0
  long long n_items;
  int m, n, mode, split;
  double* values;           // [n_items][m][m][val_stride]
  int val_stride, col_mag, col_lagged;    // a column of -1: not wanted
  int* info;                // [n_items]
};
int launch_phase_sync_pairs(const PhasePairsArgs& a, int m_pad, hipStream_t st);

// ---- phase-lag family of analytic signals: PLI, wPLI, debiased squared wPLI (phase_lag.hip) ------------------------
struct PhaseLagArgs {
  const double2* z;         // as PhaseSyncArgs
  long long rec_stride, ld, T, n_rec;
  const long long* item_rec;    // [n_items] (device)
  const long long* item_start;  // [n_items] (device)
  long long n_items;
  int m, n, split;          // channels, window length, 0 = all pairs / 1..m-1 = the pairs i < split <= j only
  double* pli;              // optional [n_items][m][m]
  double* wpli;             // optional [n_items][m][m]
  double* dwpli;            // optional [n_items][m][m]
  int* info;                // [n_items]
};
int launch_phase_lag(const PhaseLagArgs& a, int m_pad, hipStream_t st);

}  // namespace hmv
