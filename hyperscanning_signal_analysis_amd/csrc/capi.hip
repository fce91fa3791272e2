// C ABI of libhypermvar.so -- argument checking and launch sequencing only; see include/hypermvar.h.
#include "../../include/hypermvar.h"
#include "hmv_kernels.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
thread_local char g_err[256] = "";

int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
// a refusal in the words of the entry `who`: the one place where "<entry>: <what is wrong>" is put together
int refuse(const char* who, int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s: %s", who, msg);
  return code;
}
int pad_of(int m) { return (m < 1 || m > HMV_MAX_CHANNELS) ? -1 : ((m + 15) / 16) * 16; }
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// Tuning knobs: the environment is parsed once, at load time, with range checks; hmv_set_tuning overrides.
constexpr int N_TUNE = 7;
struct TuneRange { long long lo, hi; };
constexpr TuneRange kTuneRange[N_TUNE] = {{0, 0}, {0, 1 << 20}, {0, 3}, {0, 2}, {0, 5}, {0, 140000}, {-1, 1 << 20}};
long long env_knob(const char* name, int key) {
  const char* e = getenv(name);
  if (!e || !*e) return 0;
  char* end = nullptr;
  const long long v = strtoll(e, &end, 10);
  if (end == e || *end != 0 || v < kTuneRange[key].lo || v > kTuneRange[key].hi) {
    fprintf(stderr, "hypermvar: ignoring %s=%s (not an integer in %lld..%lld)\n", name, e, kTuneRange[key].lo,
            kTuneRange[key].hi);
    return 0;
  }
  return v;
}
std::atomic<long long> g_tune[N_TUNE] = {{0}, {env_knob("HYPERMVAR_NORM_LAG", 1)}, {env_knob("HYPERMVAR_LAG_GROUP", 2)},
                                         {env_knob("HYPERMVAR_K3_FORM", 3)}, {env_knob("HYPERMVAR_YW_FORM", 4)},
                                         {env_knob("HYPERMVAR_K3_LDS_PAD", 5)}, {env_knob("HYPERMVAR_K3_SPLIT", 6)}};
}  // namespace

namespace hmv {
long long tuning(int key) { return (key >= 1 && key < N_TUNE) ? g_tune[key].load(std::memory_order_relaxed) : -1; }
}

#ifdef HMV_STAMP
// Diagnostic build only (never shipped, not in include/hypermvar.h): where K3 writes its phase stamps.
static unsigned long long* g_tf_stamps = nullptr;
extern "C" void hmv_debug_set_tf_stamps(void* p) { g_tf_stamps = static_cast<unsigned long long*>(p); }
#endif

extern "C" {

int hmv_version(void) { return HMV_VERSION; }
const char* hmv_last_error(void) { return g_err; }
int hmv_pad(int m) { return pad_of(m); }

int hmv_set_tuning(int key, int64_t value) {
  if (key < 1 || key >= N_TUNE) return fail(-1, "hmv_set_tuning: unknown key");
  if (value < kTuneRange[key].lo || value > kTuneRange[key].hi) return fail(-1, "hmv_set_tuning: value out of range");
  g_tune[key].store(value, std::memory_order_relaxed);
  return 0;
}
int64_t hmv_get_tuning(int key) { return hmv::tuning(key); }

int64_t hmv_yw_workspace_doubles(int m, int p) {
  const int mp = pad_of(m);
  if (mp < 0 || p < 1 || p > HMV_MAX_ORDER) return -1;
  return hmv::yw_ws_tiles(p) * (int64_t)mp * mp;
}

int hmv_lagcov_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                   const int64_t* item_start, int64_t n_items, int m, int n, int p, double* R, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_lagcov_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_lagcov_f64: model order must be in 1..32");
  if (n <= p) return fail(-3, "hmv_lagcov_f64: window shorter than the model order");
  if (!x || !item_rec || !item_start || !R || n_items < 0) return fail(-4, "hmv_lagcov_f64: null pointer");
  hmv::LagcovArgs a{};
  a.x = x; a.rec_stride = rec_stride; a.ld = ld;
  a.item_rec = reinterpret_cast<const long long*>(item_rec);
  a.item_start = reinterpret_cast<const long long*>(item_start);
  a.n_items = n_items; a.m = m; a.n = n; a.p = p; a.R = R;
  return hmv::launch_lagcov(a, mp, S(stream));
}

int64_t hmv_lagcov_regular_workspace_doubles(int64_t n_win, int m, int n, int64_t hop, int p) {
  const int mp = pad_of(m);
  if (mp < 0 || n_win < 0 || hop < 1 || n < 1 || n % hop != 0 || p < 0) return -1;
  return (n_win + n / hop - 1) * (int64_t)(p + 1) * mp * mp;
}

int hmv_lagcov_regular_f64(const double* x, int64_t ld, int64_t T, int64_t first, int64_t hop, int64_t n_win, int m,
                           int n, int p, double* R, double* workspace, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_lagcov_regular_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_lagcov_regular_f64: model order must be in 1..32");
  if (n <= p) return fail(-3, "hmv_lagcov_regular_f64: window shorter than the model order");
  if (!x || !R || !workspace || n_win < 0) return fail(-4, "hmv_lagcov_regular_f64: null pointer");
  if (hop < 1 || n % hop != 0 || hop <= p)
    return fail(-5, "hmv_lagcov_regular_f64: the window must be a whole number of hops and a hop longer than the order");
  if (first < 0 || ld < T || (n_win > 0 && first + (n_win - 1) * hop + n > T))
    return fail(-6, "hmv_lagcov_regular_f64: windows do not lie inside the recording");
  if (n_win == 0) return 0;
  const int k = (int)(n / hop);
  hmv::LagcovArgs a{};
  a.x = x; a.rec_stride = 0; a.ld = ld; a.item_rec = nullptr; a.item_start = nullptr;
  a.n_items = n_win + k - 1; a.m = m; a.n = (int)hop; a.p = p; a.R = workspace;
  a.blocks = 1; a.blk_first = first; a.blk_T = T;
  int rc = hmv::launch_lagcov(a, mp, S(stream));
  if (rc) return rc;
  hmv::LagcombArgs c{};
  c.Q = workspace; c.x = x; c.ld = ld; c.first = first; c.hop = hop; c.T = T; c.n_win = n_win; c.k = k; c.m = m; c.p = p;
  c.R = R;
  return hmv::launch_lagcomb(c, mp, S(stream));
}

// ---- K1 of an event-locked ensemble (lagcov_ensemble.hip) -------------------------------------------------------
namespace {
// Which form of the ensemble K1 runs: the shared-overlap form where the declared grid allows it (whole hops, 2..32 hops
// per window, a hop longer than the order, a hop block and its lags within one LDS fill), else the direct form.
bool ens_shared_form(int n, int p, int64_t grid_hop, int64_t flags) {
  return grid_hop > 0 && !(flags & HMV_FLAG_DIRECT_LAGCOV) &&
         hmv::lagcov_ensemble_shared_ok(n, grid_hop, p, HMV_MAX_HOPS_ENSEMBLE);
}
bool ens_grid_ok(int64_t n_items, int64_t n_groups, int n, int64_t ld, int64_t T, int64_t grid_hop, int64_t grid_nwin) {
  return grid_hop > 0 && grid_nwin >= 1 && n_items == n_groups * grid_nwin && (grid_nwin - 1) * grid_hop + n <= T && ld >= T;
}
int64_t ens_q_tiles(int64_t n_items, int n, int p, int64_t grid_hop, int64_t grid_nwin) {
  if (grid_hop <= 0 || grid_nwin < 1 || !ens_shared_form(n, p, grid_hop, 0)) return 0;
  return hmv::lagcov_ensemble_q_tiles(n_items, grid_nwin, (int)(n / grid_hop));
}
// The samples and the two per-item tables of a K1 call, as a stage entry or sliding_impl received them: item_rec /
// item_start, for an ensemble item_group / item_offset, for pairs rec_a / item_start.
struct K1In {
  const double* x;
  int64_t rec_stride, ld;
  const int64_t* item_a;
  const int64_t* item_b;
  int m, n, p;
};
const long long* ll(const int64_t* v) { return reinterpret_cast<const long long*>(v); }
// An event-locked ensemble in place of single windows (hmv_sliding_ensemble_f64): item_rec / item_start of sliding_impl
// then carry item_group / item_offset, grid_hop / grid_nwin describe the offsets, and only K1 differs.
struct EnsDesc {
  const int64_t* trial_rec;
  const int64_t* trial_start;
  const int64_t* group_ptr;
  int64_t n_groups, T;
  // hmv_sliding_ensemble_split_f64 only: the second trial table, the first channel read through it, and the stacks the
  // within-participant elements are copied from (lagcov_ens_split_kernel; always the direct form)
  const int64_t* trial_rec_b = nullptr;
  const int64_t* trial_start_b = nullptr;
  int split = 0;
  const double* R_base = nullptr;
  const int64_t* item_base = nullptr;
};
// K1's arguments for the items i0 .. i0 + c - 1 of the call.  Q: the scratch of the shared-overlap form on the grid
// (hop, nwin), or null for the direct form.
hmv::LagcovEnsArgs ens_args(const K1In& in, const EnsDesc& e, int64_t i0, int64_t c, double* R, double* Q, int64_t hop,
                            int64_t nwin) {
  hmv::LagcovEnsArgs a{};
  a.x = in.x; a.rec_stride = in.rec_stride; a.ld = in.ld; a.T = e.T;
  a.trial_rec = ll(e.trial_rec); a.trial_start = ll(e.trial_start); a.group_ptr = ll(e.group_ptr);
  a.item_group = ll(in.item_a + i0); a.item_offset = ll(in.item_b + i0);
  a.n_items = c; a.m = in.m; a.n = in.n; a.p = in.p; a.R = R;
  if (Q) { a.it0 = i0; a.nwin = nwin; a.hop = hop; a.k = (int)(in.n / hop); a.Q = Q; }
  if (e.split) {
    a.trial_rec_b = ll(e.trial_rec_b); a.trial_start_b = ll(e.trial_start_b);
    a.split = e.split; a.R_base = e.R_base;
    a.item_base = e.item_base ? ll(e.item_base + i0) : nullptr;
  }
  return a;
}
}  // namespace

int64_t hmv_lagcov_ensemble_workspace_doubles(int64_t n_items, int m, int n, int p, int64_t grid_hop, int64_t grid_nwin) {
  const int mp = pad_of(m);
  if (mp < 0 || n_items < 0 || p < 1 || p > HMV_MAX_ORDER || n <= p || grid_hop < 0 || grid_nwin < 0) return -1;
  return ens_q_tiles(n_items, n, p, grid_hop, grid_nwin) * (int64_t)(p + 1) * mp * mp;
}

int hmv_lagcov_ensemble_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* trial_rec,
                            const int64_t* trial_start, const int64_t* group_ptr, int64_t n_groups,
                            const int64_t* item_group, const int64_t* item_offset, int64_t n_items, int m, int n, int p,
                            double* R, double* workspace, int64_t workspace_doubles, int64_t grid_hop, int64_t grid_nwin,
                            int64_t flags, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_lagcov_ensemble_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_lagcov_ensemble_f64: model order must be in 1..32");
  if (n <= p) return fail(-3, "hmv_lagcov_ensemble_f64: window shorter than the model order");
  if (!x || !trial_rec || !trial_start || !group_ptr || !item_group || !item_offset || !R || n_items < 0)
    return fail(-4, "hmv_lagcov_ensemble_f64: null pointer");
  if (n_groups < 1) return fail(-10, "hmv_lagcov_ensemble_f64: n_groups must be >= 1");
  if (grid_hop != 0 && !ens_grid_ok(n_items, n_groups, n, ld, T, grid_hop, grid_nwin))
    return fail(-9, "hmv_lagcov_ensemble_f64: inconsistent regular window grid");
  const bool shared = ens_shared_form(n, p, grid_hop, flags);
  if (shared) {
    const int64_t need = ens_q_tiles(n_items, n, p, grid_hop, grid_nwin) * (int64_t)(p + 1) * mp * mp;
    if (!workspace || workspace_doubles < need) return fail(-7, "hmv_lagcov_ensemble_f64: workspace too small");
  }
  const EnsDesc ens{trial_rec, trial_start, group_ptr, n_groups, T};
  const K1In in{x, rec_stride, ld, item_group, item_offset, m, n, p};
  return hmv::launch_lagcov_ensemble(ens_args(in, ens, 0, n_items, R, shared ? workspace : nullptr, grid_hop, grid_nwin), mp,
                                     shared, S(stream));
}

namespace {
// what the two split entries refuse about their five extra arguments; 0 when they are fine
int ens_split_check(const char* who, int m, const int64_t* trial_rec_b, const int64_t* trial_start_b, int split,
                    const double* R_base, const int64_t* item_base) {
  if (split < 1 || split >= m) return refuse(who, -5, "split must be in 1..m-1");
  if (!trial_rec_b || !trial_start_b) return refuse(who, -4, "null pointer (second trial table)");
  if ((R_base != nullptr) != (item_base != nullptr)) return refuse(who, -4, "R_base and item_base go together");
  return 0;
}
}  // namespace

int hmv_lagcov_ensemble_split_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* trial_rec,
                                  const int64_t* trial_start, const int64_t* group_ptr, int64_t n_groups,
                                  const int64_t* item_group, const int64_t* item_offset, int64_t n_items, int m, int n, int p,
                                  double* R, const int64_t* trial_rec_b, const int64_t* trial_start_b, int split,
                                  const double* R_base, const int64_t* item_base, int64_t flags, void* stream) {
  (void)flags;                                           // the direct form is the only one: nothing to choose
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_lagcov_ensemble_split_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_lagcov_ensemble_split_f64: model order must be in 1..32");
  if (n <= p) return fail(-3, "hmv_lagcov_ensemble_split_f64: window shorter than the model order");
  if (!x || !trial_rec || !trial_start || !group_ptr || !item_group || !item_offset || !R || n_items < 0)
    return fail(-4, "hmv_lagcov_ensemble_split_f64: null pointer");
  if (n_groups < 1) return fail(-10, "hmv_lagcov_ensemble_split_f64: n_groups must be >= 1");
  if (int rc = ens_split_check("hmv_lagcov_ensemble_split_f64", m, trial_rec_b, trial_start_b, split, R_base, item_base))
    return rc;
  EnsDesc ens{trial_rec, trial_start, group_ptr, n_groups, T};
  ens.trial_rec_b = trial_rec_b; ens.trial_start_b = trial_start_b; ens.split = split;
  ens.R_base = R_base; ens.item_base = item_base;
  const K1In in{x, rec_stride, ld, item_group, item_offset, m, n, p};
  return hmv::launch_lagcov_ensemble_split(ens_args(in, ens, 0, n_items, R, nullptr, 0, 0), mp, S(stream));
}

// ---- K1 for pairs of recordings (lagcov_ensemble.hip, lagcov_pairs_kernel) ---------------------------------------------
namespace {
// what the two pair entries refuse about their extra arguments; 0 when they are fine
int pairs_check(const char* who, int m, const int64_t* rec_b, int split, const double* R_base, const int64_t* base_a,
                const int64_t* base_b) {
  if (split < 1 || split >= m) return refuse(who, -5, "split must be in 1..m-1");
  if (!rec_b) return refuse(who, -4, "null pointer (rec_b)");
  if ((R_base != nullptr) != (base_a != nullptr) || (R_base != nullptr) != (base_b != nullptr))
    return refuse(who, -4, "R_base, base_a and base_b go together");
  return 0;
}
// Pairs of recordings in place of single windows (hmv_sliding_pairs_f64): item_rec / item_start of sliding_impl carry
// rec_a / item_start, the channels >= split are read from recording rec_b, and only K1 differs (lagcov_pairs_kernel).
struct PairDesc {
  const int64_t* rec_b;
  int split;
  const double* R_base;
  const int64_t* base_a;
  const int64_t* base_b;
};
// K1's arguments for the items i0 .. i0 + c - 1 of the call
hmv::LagcovPairsArgs pairs_args(const K1In& in, const PairDesc& d, int64_t i0, int64_t c, double* R) {
  hmv::LagcovPairsArgs a{};
  a.x = in.x; a.rec_stride = in.rec_stride; a.ld = in.ld;
  a.rec_a = ll(in.item_a + i0); a.rec_b = ll(d.rec_b + i0); a.item_start = ll(in.item_b + i0);
  a.n_items = c; a.m = in.m; a.n = in.n; a.p = in.p; a.split = d.split; a.R = R;
  a.R_base = d.R_base;
  a.base_a = d.R_base ? ll(d.base_a + i0) : nullptr;
  a.base_b = d.R_base ? ll(d.base_b + i0) : nullptr;
  return a;
}
}  // namespace

int hmv_lagcov_pairs_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* rec_a,
                         const int64_t* rec_b, const int64_t* item_start, int64_t n_items, int m, int n, int p, int split,
                         double* R, const double* R_base, const int64_t* base_a, const int64_t* base_b, int64_t flags,
                         void* stream) {
  (void)flags;                                           // the direct form is the only one: nothing to choose
  (void)T;                                               // the caller has checked the windows against it
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_lagcov_pairs_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_lagcov_pairs_f64: model order must be in 1..32");
  if (n <= p) return fail(-3, "hmv_lagcov_pairs_f64: window shorter than the model order");
  if (!x || !rec_a || !item_start || !R || n_items < 0) return fail(-4, "hmv_lagcov_pairs_f64: null pointer");
  if (int rc = pairs_check("hmv_lagcov_pairs_f64", m, rec_b, split, R_base, base_a, base_b)) return rc;
  const PairDesc pairs{rec_b, split, R_base, base_a, base_b};
  const K1In in{x, rec_stride, ld, rec_a, item_start, m, n, p};
  return hmv::launch_lagcov_pairs(pairs_args(in, pairs, 0, n_items, R), mp, S(stream));
}

namespace {
// K2's arguments as every caller in this file builds them: the solver form and the pivoted fallback from the caller's flags
hmv::YwArgs yw_args(const double* R, int64_t n_items, int m, int p, double* ws, double* ar, double* V, int32_t* info,
                    int64_t flags) {
  hmv::YwArgs a{};
  a.R = R; a.n_items = n_items; a.m = m; a.p = p; a.ws = ws; a.ar = ar; a.V = V; a.info = info;
  a.tiled = (flags & HMV_FLAG_YW_TILED) ? 1 : ((flags & HMV_FLAG_YW_ONE_LAUNCH) ? 0 : -1);
  a.pivoted = (flags & HMV_FLAG_YW_PIVOTED) ? 1 : 0;
  return a;
}
}  // namespace

int hmv_yw_solve_f64(const double* R, int64_t n_items, int m, int p, double* ws, double* ar, double* V,
                     double* vq_logdet, int32_t* info, int64_t flags, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_yw_solve_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_yw_solve_f64: model order must be in 1..32");
  if (!R || !ws || !ar || !V || !info || n_items < 0) return fail(-4, "hmv_yw_solve_f64: null pointer");
  if (vq_logdet && ((flags & HMV_FLAG_YW_PIVOTED) || hmv::tuning(HMV_TUNE_YW_FORM) == 5))
    return fail(-6, "hmv_yw_solve_f64: the pivoted LU gives no criterion curve (vq_logdet must be NULL)");
  hmv::YwArgs a = yw_args(R, n_items, m, p, ws, ar, V, info, flags);
  a.Vq_logdet = vq_logdet;
  return hmv::launch_yw(a, mp, S(stream));
}

namespace {
// c of the criterion's penalty c q m^2 / n (mtmvar.py:580-587); crit as in hmv_fad_f64: 0 AIC, 1 HQ, 2 SC
double crit_factor(int crit, int n) {
  return crit == 0 ? 2.0 : (crit == 1 ? 2.0 * log(log((double)n)) : log((double)n));
}
// the selection half of launch_yw_auto's arguments (the flags that would choose another solver are refused before)
hmv::YwAutoArgs yw_auto_args(int n, int crit, int32_t* order_out, double* crit_out) {
  hmv::YwAutoArgs sel{};
  sel.n = n; sel.crit_c = crit_factor(crit, n); sel.order_out = order_out; sel.crit_out = crit_out;
  return sel;
}
}  // namespace

int hmv_yw_solve_auto_f64(const double* R, int64_t n_items, int m, int pmax, int n, int crit, double* ws, double* ar,
                          double* V, int32_t* order_out, double* crit_out, double* vq_logdet, int32_t* info, int64_t flags,
                          void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_yw_solve_auto_f64: channel count must be in 1..64");
  if (pmax < 1 || pmax > HMV_MAX_ORDER) return fail(-2, "hmv_yw_solve_auto_f64: largest model order must be in 1..32");
  if (n <= pmax) return fail(-3, "hmv_yw_solve_auto_f64: window shorter than the largest model order");
  if (crit < 0 || crit > 2) return fail(-5, "hmv_yw_solve_auto_f64: criterion must be 0 (AIC), 1 (HQ) or 2 (SC)");
  if (flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH))
    return fail(-6, "hmv_yw_solve_auto_f64: the LDL^T forms of K2 have no automatic order");
  if (flags & HMV_FLAG_YW_PIVOTED)
    return fail(-6, "hmv_yw_solve_auto_f64: the pivoted LU has no automatic order (no criterion curve)");
  if (!R || !ws || !ar || !V || !order_out || !info || n_items < 0) return fail(-4, "hmv_yw_solve_auto_f64: null pointer");
  hmv::YwArgs a = yw_args(R, n_items, m, pmax, ws, ar, V, info, flags);
  a.Vq_logdet = vq_logdet;
  return hmv::launch_yw_auto(a, yw_auto_args(n, crit, order_out, crit_out), mp, S(stream));
}

int hmv_yw_routes_i32(const double* ws, int64_t n_items, int m, int p, int32_t* route, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_yw_routes_i32: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_yw_routes_i32: model order must be in 1..32");
  if (!ws || !route || n_items < 0) return fail(-4, "hmv_yw_routes_i32: null pointer");
  return hmv::launch_yw_routes(ws, n_items, mp, p, reinterpret_cast<int*>(route), S(stream));
}

int hmv_twiddles_f64(const double* freqs, int F, double fs, int p, double* tw, void* stream) {
  if (!freqs || !tw || F < 0 || p < 1) return fail(-4, "hmv_twiddles_f64: bad argument");
  if (F == 0) return 0;
  return hmv::launch_twiddles(freqs, F, fs, p, tw, S(stream));
}

int64_t hmv_tf_workspace_doubles(int64_t n_items, int m, int p) {
  const int mp = pad_of(m);
  if (mp < 0 || p < 1 || n_items < 0) return -1;
  return (int64_t)hmv::tf_workspace_doubles(n_items, mp, p);
}

int hmv_tf_f64(const double* ar, int64_t n_items, int m, int p, const double* tw, int F, double* P,
               double* rowsum, double* H, double* A, int32_t* info, double pivot_tau, double* ws,
               void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_tf_f64: channel count must be in 1..64");
  if (p < 1) return fail(-2, "hmv_tf_f64: model order must be >= 1");
  if (!ar || !tw || !info || !ws || n_items < 0 || F < 0) return fail(-4, "hmv_tf_f64: null pointer");
  if ((P == nullptr) != (rowsum == nullptr)) return fail(-5, "hmv_tf_f64: P and rowsum go together");
  if (!(pivot_tau > 0.0) || pivot_tau > 1.0) return fail(-6, "hmv_tf_f64: pivot_tau must be in (0, 1]");
  hmv::TfArgs a{};
  a.ar = ar; a.arx = ws; a.tw = tw; a.Zin = nullptr; a.detph = nullptr; a.P = P; a.rowsum = rowsum; a.H = H; a.A = A; a.info = info;
  a.n_items = n_items; a.F = F; a.p = p; a.m = m; a.tau = pivot_tau;
  a.stamps = nullptr;
#ifdef HMV_STAMP
  a.stamps = g_tf_stamps;
#endif
  return hmv::launch_tf_inv(a, mp, S(stream));
}

int hmv_ffdtf_norm_f64(const double* P, const double* rowsum, double* den, double* out, int64_t n_items,
                       int F, int m, int normalise, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_ffdtf_norm_f64: channel count must be in 1..64");
  if (!P || !out || (normalise && (!rowsum || !den))) return fail(-4, "hmv_ffdtf_norm_f64: null pointer");
  hmv::NormArgs a;
  a.P = P; a.rowsum = rowsum; a.den = den; a.out = out; a.n_items = n_items; a.F = F; a.m = m; a.m_pad = mp;
  a.normalise = normalise;
  return hmv::launch_ffdtf_norm(a, S(stream));
}

int hmv_transpose_c128(const double* in, double* out, int64_t n_items, int F, int m, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_transpose_c128: channel count must be in 1..64");
  if (!in || !out) return fail(-4, "hmv_transpose_c128: null pointer");
  return hmv::launch_transpose_c128(in, out, n_items, F, m, mp, S(stream));
}

int hmv_spectra_f64(const double* H, const double* V, double* Sout, int64_t n_items, int m, int F, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_spectra_f64: channel count must be in 1..64");
  if (!H || !V || !Sout) return fail(-4, "hmv_spectra_f64: null pointer");
  hmv::SpecArgs a;
  a.H = H; a.V = V; a.S = Sout; a.S_mmf = nullptr; a.n_items = n_items; a.F = F; a.m = m; a.sym = 0;
  return hmv::launch_spectra(a, mp, S(stream));
}

int hmv_spectra_mmf_f64(const double* H, const double* V, double* Sout, int64_t n_items, int m, int F, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_spectra_mmf_f64: channel count must be in 1..64");
  if (!H || !V || !Sout) return fail(-4, "hmv_spectra_mmf_f64: null pointer");
  hmv::SpecArgs a;
  a.H = H; a.V = V; a.S = nullptr; a.S_mmf = Sout; a.n_items = n_items; a.F = F; a.m = m; a.sym = 0;
  return hmv::launch_spectra(a, mp, S(stream));
}

int hmv_pack_c128(const double* in, double* out, int64_t n_items, int F, int m, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_pack_c128: channel count must be in 1..64");
  if (!in || !out || n_items < 0 || F < 0) return fail(-4, "hmv_pack_c128: null pointer");
  return hmv::launch_pack_c128(in, out, n_items, F, m, mp, S(stream));
}

int hmv_cinv_c128(const double* Z, int64_t n_items, int m, int F, double* Zinv, double* detph, int32_t* info,
                  double pivot_tau, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_cinv_c128: channel count must be in 1..64");
  if (!Z || !Zinv || !info || n_items < 0 || F < 0) return fail(-4, "hmv_cinv_c128: null pointer");
  if (!(pivot_tau > 0.0) || pivot_tau > 1.0) return fail(-6, "hmv_cinv_c128: pivot_tau must be in (0, 1]");
  hmv::TfArgs a{};
  a.ar = nullptr; a.arx = nullptr; a.tw = nullptr; a.Zin = Z; a.detph = detph; a.P = nullptr; a.rowsum = nullptr;
  a.H = Zinv; a.A = nullptr; a.info = info; a.n_items = n_items; a.F = F; a.p = 0; a.m = m; a.tau = pivot_tau;
  a.stamps = nullptr;
  return hmv::launch_cinv(a, mp, S(stream));
}

int hmv_partial_coherence_c128(const double* Sinv, const double* detph, double* kappa, int64_t n_items, int m, int F,
                               void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_partial_coherence_c128: channel count must be in 1..64");
  if (!Sinv || !detph || !kappa || n_items < 0 || F < 0) return fail(-4, "hmv_partial_coherence_c128: null pointer");
  return hmv::launch_pcoh(Sinv, detph, kappa, n_items, F, m, mp, S(stream));
}

int hmv_gpdc_f64(const double* A, const double* V, double* G, int64_t n_items, int m, int F, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_gpdc_f64: channel count must be in 1..64");
  if (!A || !V || !G || n_items < 0 || F < 0) return fail(-4, "hmv_gpdc_f64: null pointer");
  return hmv::launch_gpdc(A, V, G, n_items, F, m, mp, S(stream));
}

int hmv_trial_mean_f64(const double* R_trials, int64_t n_trials, int m, int p, double* R_mean, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_trial_mean_f64: channel count must be in 1..64");
  if (!R_trials || !R_mean || n_trials < 1 || n_trials > 0x7fffffff || p < 0)
    return fail(-4, "hmv_trial_mean_f64: bad argument");
  return hmv::launch_trial_mean(R_trials, R_mean, (long long)(p + 1) * mp * mp, (int)n_trials, S(stream));
}

int hmv_ddtf_f64(const double* ffdtf, const double* kappa, double* ddtf, int64_t n_items, int m, int F, void* stream) {
  if (!ffdtf || !kappa || !ddtf || n_items < 0 || m < 1 || F < 0) return fail(-4, "hmv_ddtf_f64: bad argument");
  return hmv::launch_ddtf(ffdtf, kappa, ddtf, (long long)n_items * m * m * F, S(stream));
}

int hmv_band_sums_f64(const double* ffdtf, int64_t n_rows, int F, const int32_t* bin_lo, const int32_t* bin_hi,
                      int n_bands, double* out, void* stream) {
  if (!ffdtf || !bin_lo || !bin_hi || !out || n_rows < 0 || F < 1 || n_bands < 0)
    return fail(-4, "hmv_band_sums_f64: bad argument");
  return hmv::launch_band_sums(ffdtf, bin_lo, bin_hi, out, n_rows, F, n_bands, S(stream));
}

int64_t hmv_psd_workspace_bytes(int64_t ch_chunk, int64_t n_times, int n_tapers) {
  if (ch_chunk < 1 || n_times < 2 || n_tapers < 1) return -1;
  return (int64_t)hmv::psd_workspace_bytes(ch_chunk, n_times, n_tapers);
}

int hmv_psd_multitaper_f64(const double* x, int64_t n_ch, int64_t n_times, int64_t ld, const double* tapers,
                           const double* weights, int n_tapers, int64_t bin_lo, int64_t bin_hi, double* psd,
                           void* workspace, int64_t workspace_bytes, int64_t ch_chunk, void* stream) {
  if (!x || !tapers || !weights || !psd || !workspace) return fail(-4, "hmv_psd_multitaper_f64: null pointer");
  if (n_ch < 0 || n_times < 2 || n_times > 0x7fffffff || n_tapers < 1 || ch_chunk < 1 || ld < n_times)
    return fail(-2, "hmv_psd_multitaper_f64: bad size");
  if (bin_lo < 0 || bin_hi < bin_lo || bin_hi > n_times / 2) return fail(-3, "hmv_psd_multitaper_f64: bad frequency bins");
  if (workspace_bytes < hmv::psd_workspace_bytes(ch_chunk, n_times, n_tapers))
    return fail(-7, "hmv_psd_multitaper_f64: workspace too small");
  const int rc = hmv::launch_psd(x, n_ch, n_times, ld, tapers, weights, n_tapers, bin_lo, bin_hi, psd, workspace, ch_chunk,
                                 S(stream));
  if (rc <= -20) return fail(rc, "hmv_psd_multitaper_f64: hipFFT plan / execution failed");
  return rc;
}

int64_t hmv_dpss_workspace_bytes(int64_t n_times, int k_max, int sym) {
  if (n_times < 2 || k_max < 1 || k_max > n_times) return -1;
  return (int64_t)hmv::dpss_workspace_bytes(n_times, k_max, sym != 0);
}

int hmv_dpss_f64(int64_t n_times, double half_nbw, int k_max, int sym, double* tapers, double* ratios, void* workspace,
                 int64_t workspace_bytes, void* stream) {
  if (!tapers || !workspace) return fail(-4, "hmv_dpss_f64: null pointer");
  if (n_times < 2 || n_times > 0x3fffffff || k_max < 1 || k_max > n_times)
    return fail(-2, "hmv_dpss_f64: bad size");
  if (!(half_nbw > 0.0) || half_nbw >= 0.5 * (double)n_times)
    return fail(-3, "hmv_dpss_f64: the time-half-bandwidth product must lie in (0, n_times / 2)");
  if (workspace_bytes < hmv::dpss_workspace_bytes(n_times, k_max, sym != 0)) return fail(-7, "hmv_dpss_f64: workspace too small");
  const int rc = hmv::launch_dpss(n_times, half_nbw, k_max, sym != 0, tapers, ratios, workspace, S(stream));
  if (rc <= -20) return fail(rc, "hmv_dpss_f64: hipFFT plan / execution failed");
  if (rc < 0) return fail(rc, "hmv_dpss_f64: bad argument");
  return rc;
}

// ---- K3 with the ffDTF normalisation folded in ------------------------------------------------------
namespace {
struct TfFfWs {
  size_t off_arx, off_P, off_rowsum, off_cnt, off_tail, total;
};
int64_t norm_lag_items(int mp, int F);
// `bands`: the reduced-product form also needs the full-resolution rows of the last `lag` windows of a batch (the ones the
// separate K4 pass normalises) for a moment, before their band sums are taken
TfFfWs tf_ff_layout(int64_t n, int mp, int p, int F, bool bands = false) {
  TfFfWs w;
  size_t o = 0;
  const size_t t = (size_t)mp * mp;
  w.off_arx = o;    o += align256(sizeof(double) * hmv::tf_workspace_doubles(n, mp, p));
  w.off_P = o;      o += align256(sizeof(double) * n * F * t);
  w.off_rowsum = o; o += align256(sizeof(double) * n * F * mp);
  w.off_cnt = o;    o += align256(sizeof(int) * (2 * n + 1 + n * mp));     // wcount, ready, missed (TfArgs)
  w.off_tail = o;
  if (bands) {
    const int64_t lag = norm_lag_items(mp, F);
    o += align256(sizeof(double) * (size_t)(n < lag ? n : lag) * F * t);
  }
  w.total = o;
  return w;
}
// Rows of window w are normalised inside K3 by workgroups of window w + lag, and the last `lag` windows of a batch
// by the separate K4 pass.  lag = six times the number of windows the chip holds at once (resident workgroups /
// F): at the north-star shape (4 windows resident) lag 8 left a third of the rows unfinished when they came up,
// 16 a tenth, 24 none (profiles/r02_norm_lag_sweep.txt).  A row that comes up too early is not waited for (it goes
// to norm_missed_kernel), so this only tunes speed.
int64_t norm_lag_items(int mp, int F) {
  const int64_t slots = (mp == 64 || mp == 48) ? 1024 : (mp == 32 ? 2048 : 5120);
  int64_t lag = (6 * slots + F - 1) / (F < 1 ? 1 : F);
  if (const int64_t t = hmv::tuning(HMV_TUNE_NORM_LAG)) lag = t;        // hmv_set_tuning: experiments and tests
  return lag < 8 ? 8 : lag;
}
}  // namespace

int64_t hmv_tf_ffdtf_workspace_bytes(int64_t n_items, int m, int p, int F) {
  const int mp = pad_of(m);
  if (mp < 0 || n_items < 0 || p < 1 || F < 1) return -1;
  return (int64_t)tf_ff_layout(n_items, mp, p, F).total;
}

namespace {
// ffdtf != NULL: the full array.  band_out != NULL: its band sums only (see hmv_tf_ffdtf_bands_f64).
// yw_ws (fused sliding path only): K2's scratch, where a recursion that did not emit left the model (launch_tf_inv).
int tf_ffdtf_impl(const char* who, const double* ar, int64_t n_items, int m, int p, const double* tw, int F, double* ffdtf,
                  double* band_out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* den, double* H,
                  int32_t* info, double pivot_tau, void* workspace, int64_t workspace_bytes, int64_t flags,
                  void* ev_k3_start, void* ev_k3_stop, void* stream, const double* yw_ws = nullptr,
                  hmv::TfSplit* k3_split = nullptr) {
  auto failw = [&](int code, const char* msg) { return refuse(who, code, msg); };
  const int mp = pad_of(m);
  const bool bands = (band_out != nullptr);
  if (mp < 0) return failw(-1, "channel count must be in 1..64");
  if (p < 1) return failw(-2, "model order must be >= 1");
  if (n_items == 0) return 0;
  if (!ar || !tw || (!ffdtf && !bands) || !den || !info || !workspace || n_items < 0 || F < 1)
    return failw(-4, "null pointer / empty grid");
  if (!(pivot_tau > 0.0) || pivot_tau > 1.0) return failw(-6, "pivot_tau must be in (0, 1]");
  if (bands) {
    if (!bin_lo || !bin_hi || n_bands < 1) return failw(-4, "band bins missing");
    if (F % 32 != 0 || F > hmv::tf_band_max_F(mp) || (flags & HMV_FLAG_UNFUSED_NORM))
      return failw(-10, "in-kernel band sums need F % 32 == 0, F within the row worker's LDS block and the fused normalisation");
  }
  const TfFfWs w = tf_ff_layout(n_items, mp, p, F, bands);
  if ((int64_t)w.total > workspace_bytes) return failw(-7, "workspace too small");
  char* base = static_cast<char*>(workspace);
  const size_t t = (size_t)mp * mp;
  hmv::TfArgs a{};
  a.ar = ar; a.arx = reinterpret_cast<double*>(base + w.off_arx); a.tw = tw;
  a.P = reinterpret_cast<double*>(base + w.off_P); a.rowsum = reinterpret_cast<double*>(base + w.off_rowsum);
  a.H = H;
  a.info = info; a.n_items = n_items; a.F = F; a.p = p; a.m = m; a.tau = pivot_tau;
  // the in-kernel normaliser moves 16 bytes per lane: whole 16-frequency lines of a 16-byte aligned output
  const bool fused = bands || (!(flags & HMV_FLAG_UNFUSED_NORM) && (F % 16 == 0) && (reinterpret_cast<uintptr_t>(ffdtf) % 16 == 0));
  // Every window is published and normalised by this launch: row i of window w < n - lag by a workgroup of window w + lag
  // inside K3, the rows of the last `lag` windows (and any row that came up before its window was complete) by
  // norm_missed_kernel right behind it -- the separate K4 pass over a second layout of |H|^2 is for the unfused form only.
  const int64_t lag = norm_lag_items(mp, F);
  const int64_t n_fused = fused ? n_items : 0;
  if (n_fused > 0) {
    a.ff = bands ? nullptr : ffdtf; a.den = den; a.fuse_items = n_fused; a.lag = (int)lag;
    if (bands) {
      a.bands = band_out; a.band_lo = reinterpret_cast<const int*>(bin_lo); a.band_hi = reinterpret_cast<const int*>(bin_hi);
      a.nb = n_bands;
    }
    a.wcount = reinterpret_cast<int*>(base + w.off_cnt);
    a.ready = a.wcount + n_items;
    a.missed = a.ready + n_items;
  }
#ifdef HMV_STAMP
  a.stamps = g_tf_stamps;
#endif
  hipStream_t st = S(stream);
  int rc = hmv::launch_tf_inv(a, mp, st, reinterpret_cast<hipEvent_t>(ev_k3_start), reinterpret_cast<hipEvent_t>(ev_k3_stop),
                              yw_ws, k3_split);
  if (rc) return rc;
  if (n_fused < n_items) {
    const int64_t n_tail = n_items - n_fused;
    double* tail = bands ? reinterpret_cast<double*>(base + w.off_tail) : ffdtf + (size_t)n_fused * m * m * F;
    rc = hmv_ffdtf_norm_f64(a.P + (size_t)n_fused * F * t, a.rowsum + (size_t)n_fused * F * mp, den + (size_t)n_fused * mp,
                            tail, n_tail, F, m, 1, stream);
    if (!rc && bands)
      rc = hmv::launch_band_sums(tail, reinterpret_cast<const int*>(bin_lo), reinterpret_cast<const int*>(bin_hi),
                                 band_out + (size_t)n_fused * m * m * n_bands, n_tail * (long long)m * m, F, n_bands, st);
  }
  return rc;
}
}  // namespace

int64_t hmv_tf_ffdtf_bands_workspace_bytes(int64_t n_items, int m, int p, int F) {
  const int mp = pad_of(m);
  if (mp < 0 || n_items < 0 || p < 1 || F < 1) return -1;
  return (int64_t)tf_ff_layout(n_items, mp, p, F, true).total;
}

int hmv_tf_ffdtf_f64(const double* ar, int64_t n_items, int m, int p, const double* tw, int F, double* ffdtf,
                     double* den, double* H, int32_t* info, double pivot_tau, void* workspace, int64_t workspace_bytes,
                     int64_t flags, void* ev_k3_start, void* ev_k3_stop, void* stream) {
  return tf_ffdtf_impl("hmv_tf_ffdtf_f64", ar, n_items, m, p, tw, F, ffdtf, nullptr, nullptr, nullptr, 0, den, H, info,
                       pivot_tau, workspace, workspace_bytes, flags, ev_k3_start, ev_k3_stop, stream);
}

int hmv_tf_ffdtf_bands_f64(const double* ar, int64_t n_items, int m, int p, const double* tw, int F, double* band_out,
                           const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* den, int32_t* info,
                           double pivot_tau, void* workspace, int64_t workspace_bytes, int64_t flags, void* ev_k3_start,
                           void* ev_k3_stop, void* stream) {
  if (!band_out) return fail(-4, "hmv_tf_ffdtf_bands_f64: null pointer / empty grid");
  return tf_ffdtf_impl("hmv_tf_ffdtf_bands_f64", ar, n_items, m, p, tw, F, nullptr, band_out, bin_lo, bin_hi, n_bands, den,
                       nullptr, info, pivot_tau, workspace, workspace_bytes, flags, ev_k3_start, ev_k3_stop, stream);
}

// ---- fused sliding-window path ----------------------------------------------------------------------
namespace {
// what the fused call computes on top of K1 / K2: ffDTF (K3), dDTF (K3 + sliding_conn.hip), GPDC (sliding_conn.hip only)
// (MEAS_BGC, block Granger causality, is internal to hmv_sliding_block_gc_f64: not one of the public HMV_MEASURE_* codes,
// its output is not an (m, m, F) array)
enum Measure { MEAS_FFDTF = 0, MEAS_DDTF = 1, MEAS_GPDC = 2, MEAS_BGC = 3 };
struct SlidingWs {
  size_t off_R, off_Q, off_ws, off_ar, off_V, off_tf, off_den, off_tw, off_H, off_B, off_G, off_full, total;
};
// `bands` with dDTF / GPDC: the chunk's full array passes through scratch (off_full) before its band sums are taken
// q_tiles >= 0: the hop-block scratch of the ensemble K1 (in stacks of p + 1 tiles) instead of the single-trial one
SlidingWs sliding_layout(int64_t chunk, int mp, int p, int F, bool bands = false, bool spectra = false, int measure = MEAS_FFDTF,
                         int64_t q_tiles = -1) {
  SlidingWs w;
  size_t o = 0;
  const size_t t = (size_t)mp * mp;
  w.off_R = o;      o += align256(sizeof(double) * chunk * (p + 1) * t);
  w.off_Q = o;      o += align256(sizeof(double) * (q_tiles >= 0 ? q_tiles : chunk + HMV_MAX_HOPS_PER_WINDOW - 1) * (p + 1) * t);   // hop-block sums
  w.off_ws = o;     o += align256(sizeof(double) * chunk * hmv::yw_ws_tiles(p) * t);
  w.off_ar = o;     o += align256(sizeof(double) * chunk * t * p);
  w.off_V = o;      o += align256(sizeof(double) * chunk * t);
  w.off_tf = o;
  if (measure == MEAS_FFDTF || measure == MEAS_DDTF) o += tf_ff_layout(chunk, mp, p, F, bands && measure == MEAS_FFDTF).total;
  w.off_den = o;    o += align256(sizeof(double) * chunk * mp);
  w.off_tw = o;     o += align256(sizeof(double) * F * p * 2);
  w.off_H = o;
  if (spectra) o += align256(sizeof(double) * 2 * chunk * F * t);       // H (complex) of one chunk, between K3 and K5
  w.off_B = o;
  if (measure == MEAS_DDTF) o += align256(sizeof(double) * chunk * (p + 1) * t);
  w.off_G = o;
  if (measure == MEAS_DDTF) o += align256(sizeof(double) * chunk * (2 * p + 1) * t);
  w.off_full = o;
  if ((measure == MEAS_DDTF || measure == MEAS_GPDC) && bands) o += align256(sizeof(double) * chunk * (mp * mp) * F);
  w.total = o;
  return w;
}
// What block Granger causality adds behind the shared front (K1 / K2 scratch, twiddles): the stage's own scratch, the two
// restricted lag-covariance stacks and fits, and (band form) the chunk's full spectral array.  `front` = where it starts.
struct BgcWs {
  size_t off_B, off_C, off_D, off_cst, off_Ra, off_Rb, off_arr, off_Vra, off_Vrb, off_ir, off_full, total;
};
// spectral false: the time-domain values alone (want = time of hmv_sliding_block_gc_pairs_f64), none of the stage's scratch
BgcWs bgc_layout(size_t front, int64_t chunk, int m, int p, int F, int split, bool bands, bool time, bool spectral = true) {
  BgcWs w;
  size_t o = front;
  const hmv::BgcPads pd = hmv::bgc_pads(m, split);
  const size_t mp = (size_t)pad_of(m), mpa = (size_t)pd.mpa, mpb = (size_t)pd.mpb, nsp = (size_t)pd.nsp, pp = (size_t)p + 1;
  w.off_B = o;      if (spectral) o += align256(sizeof(double) * chunk * pp * mp * mp);
  w.off_C = o;      if (spectral) o += align256(sizeof(double) * chunk * 2 * pp * nsp * nsp);
  w.off_D = o;      if (spectral) o += align256(sizeof(double) * chunk * 2 * pp * nsp * nsp);
  w.off_cst = o;    if (spectral) o += align256(sizeof(double) * chunk * 2);
  w.off_Ra = o;     if (time) o += align256(sizeof(double) * chunk * pp * mpa * mpa);
  w.off_Rb = o;     if (time) o += align256(sizeof(double) * chunk * pp * mpb * mpb);
  w.off_arr = o;    if (time) o += align256(sizeof(double) * chunk * nsp * nsp * p);
  w.off_Vra = o;    if (time) o += align256(sizeof(double) * chunk * mpa * mpa);
  w.off_Vrb = o;    if (time) o += align256(sizeof(double) * chunk * mpb * mpb);
  w.off_ir = o;     if (time) o += align256(sizeof(int32_t) * chunk * 2);
  w.off_full = o;   if (bands) o += align256(sizeof(double) * chunk * 2 * F);
  w.total = o;
  return w;
}
// The range checks every hmv_sliding_*_workspace_bytes shares, then the layout's size; -1 for sizes no entry accepts.
int64_t sliding_bytes(int64_t chunk, int m, int p, int F, int n_bands = 0, bool spectra = false, int measure = MEAS_FFDTF,
                      int64_t q_tiles = -1) {
  const int mp = pad_of(m);
  if (mp < 0 || chunk < 1 || p < 1 || p > HMV_MAX_ORDER || F < 1 || n_bands < 0 || measure < MEAS_FFDTF ||
      measure > MEAS_GPDC)
    return -1;
  return (int64_t)sliding_layout(chunk, mp, p, F, n_bands > 0, spectra, measure, q_tiles).total;
}
// Fork / join events of the two-stream K2 split, and the early fork behind K1's first block range (sliding_front): created
// once per (host thread, device), not per call.
struct ForkJoin {
  hipEvent_t fork = nullptr, join = nullptr, front = nullptr;
};
ForkJoin* fork_join_events() {
  constexpr int MAXDEV = 64;
  thread_local ForkJoin tl[MAXDEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;
  ForkJoin& e = tl[dev];
  if (!e.fork) {
    if (hipEventCreateWithFlags(&e.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&e.front, hipEventDisableTiming) != hipSuccess) return nullptr;
  }
  return &e;
}
// Where a chunk of c windows is handed from K2 to K3 in two parts (HMV_TUNE_K3_SPLIT), or 0 for one part.  K2 runs one
// workgroup per window, all of them resident at once while c < occupancy * CUs, and lasts as long as the fullest compute
// unit's windows take: with k = c / CUs full rounds and r = c % CUs windows over, r units carry k + 1 windows and the others
// wait for them.  The r windows over are then solved on the second stream while K3 starts on the first c0 = c - r.  Chunks of
// several rounds (k >= occupancy) are not split, nor are chunks whose first part is shorter than K3's normalisation lag.
// CUs and occupancy come from the runtime, once per (host thread, device, padded size).
// Where the chunk's K1 can be cut at the same point (`can_front`: sliding_front), a chunk of more than one and fewer than
// `occupancy` rounds is split after its first round instead, c0 = CUs: K2's first round then runs beside the rest of K1, and
// most of K2's second part is done before K3 arrives (profiles/front_overlap_notes.md).  A tuning value of
// HMV_K3_SPLIT_NO_FRONT + n means n without the K1 cut.
struct SplitPoint {
  int64_t c0;                                       // 0: one part
  bool front;                                       // K1 is cut at c0 too
};
SplitPoint k3_split_point(int64_t c, int mp, int64_t lag, bool can_front) {
  int64_t t = hmv::tuning(HMV_TUNE_K3_SPLIT);
  if (t < 0) return {};
  if (t >= HMV_K3_SPLIT_NO_FRONT) {
    t -= HMV_K3_SPLIT_NO_FRONT;
    can_front = false;
  }
  int64_t c0 = t;
  if (t == 0) {
    constexpr int MAXDEV = 64;
    struct Shape { int cus = 0, occ[4] = {0, 0, 0, 0}; };
    thread_local Shape tl[MAXDEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV || mp < 16 || mp > 64) return {};
    Shape& d = tl[dev];
    int& occ = d.occ[mp / 16 - 1];
    if (d.cus == 0 && hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) d.cus = -1;
    if (occ == 0 && (occ = hmv::yw_lwr_occupancy(mp)) == 0) occ = -1;
    if (d.cus < 1 || occ < 1) {
      (void)hipGetLastError();                           // (a failed query must not surface as a later launch's error)
      return {};
    }
    const int64_t k = c / d.cus, r = c % d.cus;
    if (can_front && c > d.cus && k < occ && d.cus >= lag) return {d.cus, true};
    if (k < 1 || k >= occ || r == 0) return {};
    c0 = c - r;
    can_front = false;
  }
  return (c0 >= lag && c0 < c) ? SplitPoint{c0, can_front} : SplitPoint{};
}
}  // namespace

int64_t hmv_sliding_workspace_bytes(int64_t chunk, int m, int p, int F) { return sliding_bytes(chunk, m, p, F); }

namespace {
// A weighted sum over the trials of a per-trial stack in place of single windows (hmv_sliding_mix_f64): item k * n_win + w
// is mix row k at window w, there are no samples and no item tables, and only K1 differs (lagcov_mix_kernel).
struct MixDesc {
  const double* Rt;
  const double* W;
  const double* scale;
  int64_t n_trials, n_win, n_mix;
};
// Block Granger causality in place of an (m, m, F) measure (hmv_sliding_block_gc_f64): K1 and K2 as for every entry, then
// the two restricted fits from the same lag covariances and the kernels of block_gc.hip; there is no K3.
struct BgcDesc {
  int split;
  double* time;                                     // [n_items][4]
  int32_t* info_red;                                // [n_items][2]
  int32_t* info_gc;                                 // [n_items*F]
  // hmv_sliding_block_gc_pairs_f64 only (with SlidingArgs::pairs, whose base_a / base_b index red_base too)
  int want = 3;                                     // bit 0 spectral, bit 1 time
  double* red_out = nullptr;                        // [n_items][2]
  const double* red_base = nullptr;                 // [n_base][2]
  const int32_t* info_red_base = nullptr;           // [n_base][2]
};
// Everything the driver is told, in the groups the ABI passes it in; an entry hands each group over whole.
struct Items {                                      // the samples and the windows (ensemble: item_group / item_offset in
  const double* x;                                  // place of item_rec / item_start, pairs: rec_a / item_start; mix: none)
  int64_t rec_stride, ld;
  const int64_t* item_rec;
  const int64_t* item_start;
  int64_t n_items;
  int m, n, p;                                      // (p: the largest order tried where the order is automatic)
};
struct Grid { int64_t hop, first, nwin, T; };       // the declared regular grid; hop = 0: none
struct Spectral { const double* freqs; int F; double fs; };
struct Output {
  double* out;                                      // the full (m, m, F) arrays, or (bands) their band sums
  const int32_t* bin_lo;
  const int32_t* bin_hi;
  int n_bands;
  bool bands;                                       // decided by `output` below, nowhere else
  double* S_out;                                    // the spectra beside the full ffDTF, or null
};
// n_bands > 0 means band sums; hmv_sliding_ffdtf_bands_f64 has no other form, whatever its n_bands
Output output(double* out, const int32_t* bin_lo = nullptr, const int32_t* bin_hi = nullptr, int n_bands = 0,
              bool bands_only = false, double* S_out = nullptr) {
  return {out, bin_lo, bin_hi, n_bands, bands_only || n_bands > 0, S_out};
}
struct FitOut {
  double* ar_out;
  double* V_out;
  int32_t* info_yw;
  int32_t* info_tf;
  double pivot_tau;
};
struct Run {
  void* workspace;
  int64_t workspace_bytes, chunk, flags;
  void* stream;
  void* aux_stream;
  void* ev_k3_start;
  void* ev_k3_stop;
};
struct OrderSel {                                   // crit >= 0: automatic order, with order_out (and crit_out)
  int crit = -1;
  int32_t* order_out = nullptr;
  double* crit_out = nullptr;
};
struct SlidingArgs {
  const char* who;                                  // the entry's own name, for hmv_last_error()
  int measure;
  Items it;
  Grid grid;
  Spectral spec;
  Output o;
  FitOut fit;
  Run run;
  OrderSel sel = {};
  const EnsDesc* ens = nullptr;
  const PairDesc* pairs = nullptr;
  const MixDesc* mix = nullptr;
  const BgcDesc* bgc = nullptr;                     // measure == MEAS_BGC: `o` carries the spectral output
};

// ---- what the entries refuse ahead of the driver, once each
// The measure-coded entries (auto, ensemble, pairs, mix): measure, n_bands and S_out -- the criterion between them where
// the order is automatic --, and what an accepted GPDC does to the fit outputs: it inverts nothing, so it has neither
// info_tf nor a pivot threshold.
int measure_request(const char* who, int measure, int n_bands, const double* S_out, FitOut& fit, int crit = 0) {
  if (measure < HMV_MEASURE_FFDTF || measure > HMV_MEASURE_GPDC)
    return refuse(who, -4, "measure must be HMV_MEASURE_FFDTF, _DDTF or _GPDC");
  if (crit < 0 || crit > 2) return refuse(who, -5, "criterion must be 0 (AIC), 1 (HQ) or 2 (SC)");
  if (n_bands < 0) return refuse(who, -4, "n_bands must be >= 0");
  if (S_out && (measure != HMV_MEASURE_FFDTF || n_bands != 0))
    return refuse(who, -4, "spectra come with the full ffDTF only");
  if (measure == HMV_MEASURE_GPDC) { fit.info_tf = nullptr; fit.pivot_tau = 1.0; }
  return 0;
}
// a missing output of a batch that is not empty
int need_output(const char* who, const void* out, int64_t n_items) {
  return (!out && n_items != 0) ? refuse(who, -4, "null pointer / empty grid") : 0;
}
// The same for the entries that refuse something of their own ahead of it (ensemble, pairs, mix): only where the driver's
// size checks would pass, so that a bad size is still refused first, as at the other entries.
int need_output_after_sizes(const char* who, const Items& it, const void* out) {
  const bool sizes_ok = pad_of(it.m) >= 0 && it.p >= 1 && it.p <= HMV_MAX_ORDER && it.n > it.p;
  return sizes_ok ? need_output(who, out, it.n_items) : 0;
}
// n_bands = -1 to a measure-coded sizer: the full ffDTF together with S_out (one chunk of H passes through the workspace
// between K3 and K5)
int64_t measure_bytes(int measure, int64_t chunk, int m, int p, int F, int n_bands, int64_t q_tiles) {
  const bool spectra = (n_bands == -1 && measure == HMV_MEASURE_FFDTF);
  return sliding_bytes(chunk, m, p, F, spectra ? 0 : n_bands, spectra, measure, q_tiles);
}

// ---- the second stream: all of its uses fork and join through this
// fork: st1 may start once what st0 holds is done.  join: st0 takes up again behind st1, so that the caller's stream never
// runs ahead of work this call put on the second stream; a join that cannot be expressed as an event is made on the host.
struct TwoStreams {
  hipStream_t st0 = nullptr, st1 = nullptr;
  ForkJoin* ev = nullptr;
  int fork(hipEvent_t at) const {                   // nonzero: nothing may be put on st1
    const int hrc = (int)hipEventRecord(at, st0);
    return hrc ? hrc : (int)hipStreamWaitEvent(st1, at, 0);
  }
  int fork() const { return fork(ev->fork); }
  int fork_front() const { return fork(ev->front); }   // the early fork, behind K1's first part (sliding_front)
  int record_join() const {
    const int hrc = (int)hipEventRecord(ev->join, st1);
    if (hrc) (void)hipStreamSynchronize(st1);
    return hrc;
  }
  int wait_join(hipEvent_t join) const {
    const int hrc = (int)hipStreamWaitEvent(st0, join, 0);
    if (hrc) (void)hipStreamSynchronize(st1);
    return hrc;
  }
  int join() const {
    const int hrc = record_join();
    return hrc ? hrc : wait_join(ev->join);
  }
  // the K2 -> K3 hand-over in two parts: st0 joins st1 unless K3's launcher already made it wait between its two launches
  void finish(hmv::TfSplit& sp) const {
    if (sp.join && !sp.joined) (void)wait_join(sp.join);
    sp.joined = true;
  }
};

// ---- the plan of a call: every refusal, in order, and everything that does not change from chunk to chunk
struct SlidingPlan {
  bool empty = false;                               // n_items == 0: nothing to do, nothing more was checked
  int mp = 0;
  size_t t = 0, ws_item = 0;                        // doubles per tile; K2 scratch doubles per window
  bool automatic = false, bands = false, k3_bands = false, bgc_spec = false, bgc_time = false;
  bool regular = false, ens_shared = false;         // K1: hop blocks shared between the windows of a declared grid
  bool ldl = false, from_tiles = false;             // K2: an LDL^T form; a recursion that leaves the model in its tiles
  bool half_split = false, k3_split = false;        // what the second stream may be used for
  TwoStreams fj;
  SlidingWs w{};
  BgcWs gw{};
  char* base = nullptr;
  double *R = nullptr, *Qb = nullptr, *ws = nullptr, *ar = nullptr, *V = nullptr, *den = nullptr, *tw = nullptr;
  void* tfws = nullptr;
  int64_t tfws_bytes = 0;
  double* at(size_t off) const { return reinterpret_cast<double*>(base + off); }        // a double array of the workspace
  // The caller's flags as K2 takes them for `cnt` windows of padded size mpx: where the plan has an LDL^T form, the launch
  // chain if it is asked for or chosen by shape, else the one launch
  int64_t yw_flags(int64_t flags, int mpx, int64_t cnt) const {
    const int64_t forms = HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH;
    const bool chain =
        (flags & HMV_FLAG_YW_TILED) || (ldl && !(flags & HMV_FLAG_YW_ONE_LAUNCH) && hmv::yw_chain_by_shape(mpx, cnt));
    return (flags & ~forms) | (ldl ? (chain ? HMV_FLAG_YW_TILED : HMV_FLAG_YW_ONE_LAUNCH) : 0);
  }
};
int sliding_plan(const SlidingArgs& a, SlidingPlan& pl) {
  const Items& it = a.it;
  const int64_t flags = a.run.flags;
  auto fail = [&](int code, const char* msg) { return refuse(a.who, code, msg); };
  // crit >= 0: automatic order (hmv_sliding_auto_f64) -- p is the largest order tried, K1 sums p + 1 lags, K2 selects every
  // window's order and leaves its coefficients zero-padded to p lags, and every later stage runs at p on those (the
  // added terms of A(f) = I - sum_k ar_k tw_k are exact zeros)
  pl.automatic = a.sel.crit >= 0;
  pl.bands = a.o.bands;
  pl.mp = pad_of(it.m);
  if (pl.mp < 0) return fail(-1, "channel count must be in 1..64");
  if (it.p < 1 || it.p > HMV_MAX_ORDER) return fail(-2, "model order must be in 1..32");
  if (it.n <= it.p) return fail(-3, "window shorter than the model order");
  if (pl.automatic && a.sel.crit > 2) return fail(-5, "criterion must be 0 (AIC), 1 (HQ) or 2 (SC)");
  if (pl.automatic && (flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH)))
    return fail(-6, "the LDL^T forms of K2 have no automatic order");
  if (pl.automatic && (flags & HMV_FLAG_YW_PIVOTED))
    return fail(-6, "the pivoted LU has no automatic order (no criterion curve)");
  if (a.mix && (a.mix->n_trials < 1 || a.mix->n_win < 1 || a.mix->n_mix < 1))
    return fail(-10, "n_trials, n_win and n_mix must be >= 1");
  if (it.n_items == 0) {                                           // empty batch: nothing to do, nothing to check
    pl.empty = true;
    return 0;
  }
  if (pl.automatic && !a.sel.order_out) return fail(-4, "null pointer / empty grid");
  if (a.mix ? (!a.mix->Rt || !a.mix->W || reinterpret_cast<uintptr_t>(a.mix->Rt) % 16 != 0)
            : (!it.x || !it.item_rec || !it.item_start))
    return fail(-4, "null pointer / empty grid");
  pl.bgc_spec = !a.bgc || (a.bgc->want & 1);                       // (time alone: no frequencies)
  pl.bgc_time = a.bgc && (a.bgc->want & 2);
  if ((pl.bgc_spec && (!a.spec.freqs || !a.o.out || a.spec.F < 1)) || !a.fit.info_yw ||
      (!a.fit.info_tf && (a.measure == MEAS_FFDTF || a.measure == MEAS_DDTF)) || !a.run.workspace || a.run.chunk < 1)
    return fail(-4, "null pointer / empty grid");
  if (pl.bands && (!a.o.bin_lo || !a.o.bin_hi || a.o.n_bands < 1)) return fail(-4, "band bins missing");
  if (a.ens) {
    if (!a.ens->trial_rec || !a.ens->trial_start || !a.ens->group_ptr) return fail(-4, "null pointer / empty grid");
    if (a.ens->n_groups < 1) return fail(-10, "n_groups must be >= 1");
    if (a.grid.hop != 0 && !ens_grid_ok(it.n_items, a.ens->n_groups, it.n, it.ld, a.ens->T, a.grid.hop, a.grid.nwin))
      return fail(-9, "inconsistent regular window grid");
    pl.ens_shared = !a.ens->split && ens_shared_form(it.n, it.p, a.grid.hop, flags);
  }
  const int64_t chunk = a.run.chunk;
  pl.w = sliding_layout(chunk, pl.mp, it.p, a.spec.F, pl.bands, a.o.S_out != nullptr, a.measure,
                        a.ens ? (pl.ens_shared ? ens_q_tiles(chunk, it.n, it.p, a.grid.hop, a.grid.nwin) : 0)
                              : ((a.pairs || a.mix) ? 0 : -1));
  if (a.bgc) pl.gw = bgc_layout(pl.w.total, chunk, it.m, it.p, a.spec.F, a.bgc->split, pl.bands, pl.bgc_time, pl.bgc_spec);
  if ((int64_t)(a.bgc ? pl.gw.total : pl.w.total) > a.run.workspace_bytes) return fail(-7, "workspace too small");
  // Regular grid (the caller vouches: item = rec * grid.nwin + w starts at grid.first + w * grid.hop of recording rec,
  // recordings are grid.T samples long): K1 sums every hop block once and assembles the windows from the blocks.
  pl.regular = !a.ens && !a.pairs && !a.mix && a.grid.hop > 0 && !(flags & HMV_FLAG_DIRECT_LAGCOV);
  if (pl.regular) {
    const Grid& g = a.grid;
    if (g.nwin < 1 || g.first < 0 || it.n_items % g.nwin != 0 || g.first + (g.nwin - 1) * g.hop + it.n > g.T || it.ld < g.T)
      return fail(-9, "inconsistent regular window grid");
    pl.regular = (it.n % g.hop == 0) && (it.n / g.hop >= 2) && (it.n / g.hop <= HMV_MAX_HOPS_PER_WINDOW) && g.hop > it.p;
  }
  // K2: the Levinson-Whittle recursion unless an LDL^T form is asked for (or HMV_TUNE_YW_FORM = 1, which picks the LDL^T
  // form by batch shape: hmv::yw_chain_by_shape).  Nobody but K3's packing kernel reads the model when the caller does not
  // ask for it and the measure is the ffDTF: the default recursion then leaves it in its scratch tiles, which the packing
  // kernel reads directly (windows that the conditioning guard hands to the LDL^T re-solve come through `ar` as before).
  const int64_t yw_form = hmv::tuning(HMV_TUNE_YW_FORM);
  pl.ldl = (flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH)) || yw_form == 1;
  pl.from_tiles = !pl.automatic && !a.fit.ar_out && !pl.ldl && (yw_form == 0 || yw_form == 2) && a.measure == MEAS_FFDTF;
  // Second stream, first use (the LDL^T launch chain only): that form of K2 is a chain of ~25 launches of at most a few
  // workgroups per window that cannot fill the chip; it runs as two half-batches, one per stream, whose launches
  // interleave on the device (fork after K1, join before K3).  The one-launch forms need none of this.  Chunk pipelining
  // (K1/K2 of chunk c+1 under K3 of chunk c) was measured and does NOT work: K3 holds every wave slot and starves the
  // other stream.
  // Second use, by the default form (k3_split_point, profiles/k3_split_notes.md): the work put beside K3 is the few windows
  // of the SAME chunk that K2's last, partly filled round would make the whole chip wait for, and it is placed before K3
  // arrives -- forked behind K2's first part, with only the light packing kernel between the fork and K3, so its
  // workgroups land on an almost empty chip and K3 fills in around them.  It is zero-sum in chip time like the others;
  // what it removes is the idle tail of K2 from the critical path.  Only where nobody but K3's packing kernel reads the
  // model (from_tiles) and no output beyond the ffDTF is asked for.
  // Third use, where the second applies and the chunk's K1 can be cut at the split point (front_cut_ok, sliding_front;
  // profiles/front_overlap_notes.md): the second stream forks earlier, behind K1 of the first part's hop blocks, and runs the
  // rest of K1, its lagcomb and K2's second part.  K1 is bound by the matrix pipe and K2 by the latency of its chain, and
  // K3 is not there yet, so this overlap is not zero-sum; K3 starts behind K2's first part alone, as in the second use.
  pl.fj.st0 = S(a.run.stream);
  pl.fj.st1 = S(a.run.aux_stream);
  const bool two = (a.run.aux_stream && a.run.aux_stream != a.run.stream);
  pl.half_split = two && !(flags & HMV_FLAG_YW_ONE_LAUNCH);
  pl.k3_split = two && !pl.automatic && a.measure == MEAS_FFDTF && !a.o.S_out && !a.fit.ar_out && !a.fit.V_out &&
                !(flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH));
  if (pl.half_split || pl.k3_split) {
    pl.fj.ev = fork_join_events();
    if (!pl.fj.ev) return fail(-8, "cannot create fork/join events");
  }
  pl.t = (size_t)pl.mp * pl.mp;
  pl.base = static_cast<char*>(a.run.workspace);
  pl.R = pl.at(pl.w.off_R);
  pl.Qb = pl.at(pl.w.off_Q);
  pl.ws = pl.at(pl.w.off_ws);
  pl.ar = pl.at(pl.w.off_ar);
  pl.V = pl.at(pl.w.off_V);
  pl.tfws = pl.base + pl.w.off_tf;
  pl.den = pl.at(pl.w.off_den);
  pl.tw = pl.at(pl.w.off_tw);
  pl.k3_bands = pl.bands && a.measure == MEAS_FFDTF;
  pl.tfws_bytes = (int64_t)tf_ff_layout(chunk, pl.mp, it.p, a.spec.F, pl.k3_bands).total;
  pl.ws_item = (size_t)hmv_yw_workspace_doubles(it.m, it.p);
  return 0;
}

// the windows i0 .. i0 + c - 1 of the call, and where their model goes: the caller's arrays or the workspace
struct Chunk {
  int64_t i0, c;
  double* ar;
  double* V;
  bool last;
};

// ---- K1 of a chunk into pl.R, on st0: whichever form the entry's descriptors and the grid call for
int sliding_k1(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch) {
  const Items& it = a.it;
  const int64_t i0 = ch.i0, c = ch.c;
  hipStream_t st = pl.fj.st0;
  const K1In in{it.x, it.rec_stride, it.ld, it.item_rec, it.item_start, it.m, it.n, it.p};
  if (a.ens) {
    const hmv::LagcovEnsArgs ea = ens_args(in, *a.ens, i0, c, pl.R, pl.ens_shared ? pl.Qb : nullptr, a.grid.hop, a.grid.nwin);
    return a.ens->split ? hmv::launch_lagcov_ensemble_split(ea, pl.mp, st)
                        : hmv::launch_lagcov_ensemble(ea, pl.mp, pl.ens_shared, st);
  }
  if (a.pairs) return hmv::launch_lagcov_pairs(pairs_args(in, *a.pairs, i0, c, pl.R), pl.mp, st);
  if (a.mix) {
    hmv::LagcovMixArgs ma{};
    ma.Rt = a.mix->Rt; ma.W = a.mix->W; ma.scale = a.mix->scale; ma.n_trials = a.mix->n_trials; ma.n_win = a.mix->n_win;
    ma.it0 = i0; ma.n_items = c; ma.m = it.m; ma.m_pad = pl.mp; ma.p = it.p; ma.R = pl.R;
    return hmv::launch_lagcov_mix(ma, st);
  }
  if (!pl.regular)
    return hmv_lagcov_f64(it.x, it.rec_stride, it.ld, it.item_rec + i0, it.item_start + i0, c, it.m, it.n, it.p, pl.R, st);
  // items i0 .. i0+c-1 as runs of consecutive windows of one recording each (item = rec * grid.nwin + w)
  const Grid& g = a.grid;
  const size_t stack = (size_t)(it.p + 1) * pl.t;
  int rc = 0;
  for (int64_t k = i0; k < i0 + c && rc == 0;) {
    const int64_t rec = k / g.nwin, w0 = k - rec * g.nwin;
    const int64_t run = ((g.nwin - w0) < (i0 + c - k)) ? (g.nwin - w0) : (i0 + c - k);
    rc = hmv_lagcov_regular_f64(it.x + rec * it.rec_stride, it.ld, g.T, g.first + w0 * g.hop, g.hop, run, it.m, it.n, it.p,
                                pl.R + (size_t)(k - i0) * stack, pl.Qb, st);
    k += run;
  }
  return rc;
}

// K2's arguments for the windows k0 .. k0 + cnt - 1 of a chunk
hmv::YwArgs k2_part(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch, int64_t k0, int64_t cnt, int64_t yw_flags) {
  const Items& it = a.it;
  return yw_args(pl.R + (size_t)k0 * (it.p + 1) * pl.t, cnt, it.m, it.p, pl.ws + (size_t)k0 * pl.ws_item,
                 ch.ar + (size_t)k0 * pl.t * it.p, ch.V + (size_t)k0 * pl.t, a.fit.info_yw + ch.i0 + k0, yw_flags);
}

// ---- where a chunk's K2 -> K3 hand-over is split, and whether its K1 is cut there too
// K1 can be cut where it is the direct form over single windows, or one run of sliding_k1's loop over a regular grid
// (the chunk lies inside one recording); every other K1 (ensembles, pairs, mix) is one piece.
bool front_cut_ok(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch) {
  if (a.ens || a.pairs || a.mix) return false;
  return !pl.regular || ch.i0 % a.grid.nwin + ch.c <= a.grid.nwin;
}
SplitPoint sliding_split(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch) {
  if (!pl.k3_split || !pl.from_tiles) return {};
  return k3_split_point(ch.c, pl.mp, norm_lag_items(pl.mp, a.spec.F), front_cut_ok(a, pl, ch));
}

// ---- K1 and K2 of a chunk cut at c0, the second parts on the second stream from the start (front_cut_ok).
//   st0: K1 of the windows [0, c0)  |event|  lagcomb [0, c0)   K2 [0, c0)                       -> K3's first launch
//   st1:                            |wait |  K1 of the rest    lagcomb [c0, c)   K2 [c0, c)  |join| -> K3's second launch
// On a regular grid of k hops per window K1 is the block sums: the first part sums the hop blocks [0, c0 + k - 1), the
// second [c0 + k - 1, c + k - 1), each into its own range of Q; lagcomb of the windows from c0 on reads the last k - 1
// blocks of the first part, hence the event.  Every block, window and byte is computed by the launch arguments that
// sliding_k1 / sliding_k2 would give it, by one writer.  sp comes back as from sliding_k2.
int sliding_front(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch, int64_t c0, hmv::TfSplit& sp) {
  const Items& it = a.it;
  const Grid& g = a.grid;
  const TwoStreams& fj = pl.fj;
  const int64_t i0 = ch.i0, c = ch.c;
  const size_t stack = (size_t)(it.p + 1) * pl.t;
  const int k = pl.regular ? (int)(it.n / g.hop) : 1;
  const int64_t rec = pl.regular ? i0 / g.nwin : 0;
  const double* x = it.x + rec * it.rec_stride;                      // (regular grid: the chunk's recording)
  const int64_t first = pl.regular ? g.first + (i0 - rec * g.nwin) * g.hop : 0;
  // K1 of the windows [k0, k1) without the blocks that the windows before k0 have summed
  auto sums = [&](int64_t k0, int64_t k1, hipStream_t st) {
    if (!pl.regular)
      return hmv_lagcov_f64(it.x, it.rec_stride, it.ld, it.item_rec + i0 + k0, it.item_start + i0 + k0, k1 - k0, it.m, it.n,
                            it.p, pl.R + (size_t)k0 * stack, st);
    const int64_t b0 = k0 ? k0 + k - 1 : 0;
    hmv::LagcovArgs la{};
    la.x = x; la.ld = it.ld; la.n_items = k1 + k - 1 - b0; la.m = it.m; la.n = (int)g.hop; la.p = it.p;
    la.R = pl.Qb + (size_t)b0 * stack;
    la.blocks = 1; la.blk_first = first + b0 * g.hop; la.blk_T = g.T;
    return hmv::launch_lagcov(la, pl.mp, st);
  };
  auto comb = [&](int64_t k0, int64_t k1, hipStream_t st) {
    if (!pl.regular) return 0;
    hmv::LagcombArgs ca{};
    ca.Q = pl.Qb + (size_t)k0 * stack; ca.x = x; ca.ld = it.ld; ca.first = first + k0 * g.hop; ca.hop = g.hop; ca.T = g.T;
    ca.n_win = k1 - k0; ca.k = k; ca.m = it.m; ca.p = it.p; ca.R = pl.R + (size_t)k0 * stack;
    return hmv::launch_lagcomb(ca, pl.mp, st);
  };
  auto solve = [&](int64_t k0, int64_t k1, hipStream_t st) {
    hmv::YwArgs ya = k2_part(a, pl, ch, k0, k1 - k0, a.run.flags);
    ya.no_emit = 1;
    return hmv::launch_yw(ya, pl.mp, st);
  };
  sp = hmv::TfSplit{};
  int rc = sums(0, c0, fj.st0);
  if (rc) return rc;
  if (const int hrc = fj.fork_front()) return hrc;
  rc = sums(c0, c, fj.st1);
  if (!rc) rc = comb(c0, c, fj.st1);
  if (!rc) rc = solve(c0, c, fj.st1);
  if (const int hrc = fj.record_join()) return rc ? rc : hrc;        // (joined on the host)
  sp.c0 = c0;                                                        // from here on TwoStreams::finish joins on every path
  sp.join = fj.ev->join;
  if (!rc) rc = comb(0, c0, fj.st0);
  if (!rc) rc = solve(0, c0, fj.st0);
  return rc;
}

// ---- K2 of a chunk, in one of three forms.  s0: where the K2 -> K3 hand-over is split (sliding_split), 0 for one part; sp
// comes back describing that hand-over, if one was set up.
int sliding_k2(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch, int64_t s0, hmv::TfSplit& sp) {
  const Items& it = a.it;
  const int64_t flags = a.run.flags, c = ch.c;
  const int mp = pl.mp;
  const TwoStreams& fj = pl.fj;
  auto part = [&](int64_t k0, int64_t cnt, int64_t yw_flags) { return k2_part(a, pl, ch, k0, cnt, yw_flags); };
  sp = hmv::TfSplit{};
  if (pl.automatic)                                  // the recursion to order p with the selection (flags: none of K2's)
    return hmv::launch_yw_auto(part(0, c, flags),
                               yw_auto_args(it.n, a.sel.crit, a.sel.order_out + ch.i0,
                                            a.sel.crit_out ? a.sel.crit_out + (size_t)ch.i0 * it.p : nullptr), mp, fj.st0);
  if (!pl.from_tiles) {
    // An LDL^T form (or the recursion, where somebody reads the model): the launch chain where it is asked for or chosen
    // by shape, and then, given a second stream and 16 windows, as two half-batches
    const int64_t yw_flags = pl.yw_flags(flags, mp, c);
    const int64_t c0 = (pl.half_split && (yw_flags & HMV_FLAG_YW_TILED) && c >= 16) ? (c + 1) / 2 : c;
    if (c0 < c) {
      if (const int hrc = fj.fork()) return hrc;
      int rc = hmv::launch_yw(part(c0, c - c0, yw_flags), mp, fj.st1);
      const int hrc = fj.join();
      if (!rc) rc = hrc;
      if (rc) return rc;
    }
    return hmv::launch_yw(part(0, c0, yw_flags), mp, fj.st0);
  }
  // The recursion that does not emit.  With a split point, the remainder windows go to the second stream, forked behind the
  // first part (they never share a compute unit with it); the join is waited for inside K3's launcher, between its two
  // launches, or by TwoStreams::finish on every path that did not get that far.
  hmv::YwArgs ya = part(0, s0 ? s0 : c, flags);
  ya.no_emit = 1;
  int rc = hmv::launch_yw(ya, mp, fj.st0);
  if (rc || !s0) return rc;
  if (const int hrc = fj.fork()) return hrc;
  hmv::YwArgs yb = part(s0, c - s0, flags);
  yb.no_emit = 1;
  rc = hmv::launch_yw(yb, mp, fj.st1);
  if (const int hrc = fj.record_join()) return rc ? rc : hrc;      // (joined on the host: one K3 launch)
  sp.c0 = s0;
  sp.join = fj.ev->join;
  return rc;
}

// ---- the block Granger stage of a chunk: gather, the two restricted fits, launch_bgc, band sums
int sliding_bgc(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch) {
  const Items& it = a.it;
  const BgcDesc& g = *a.bgc;
  const BgcWs& gw = pl.gw;
  const int64_t i0 = ch.i0, c = ch.c, flags = a.run.flags;
  hipStream_t st0 = pl.fj.st0;
  const int na = g.split, nb2 = it.m - na, F = a.spec.F;
  int rc = 0;
  hmv::BgcArgs ga{};
  ga.want = g.want;
  if (pl.bgc_time) {
    ga.red.time = g.time + (size_t)i0 * 4; ga.red.info_red = g.info_red + (size_t)i0 * 2;
    ga.red.red_out = g.red_out ? g.red_out + (size_t)i0 * 2 : nullptr;
  }
  if (pl.bgc_time && g.red_base) {
    // both restricted fits are those of observed windows (a pair changes the cross blocks only): their log-determinants
    // and infos come from the table, and nothing is gathered or solved
    ga.red.red_base = g.red_base; ga.red.info_red_base = g.info_red_base;
    ga.red.base_a = ll(a.pairs->base_a + i0); ga.red.base_b = ll(a.pairs->base_b + i0);
  } else if (pl.bgc_time) {
    // K2 on the gathered blocks of the same lag covariances, in the scratch the full fit has left, in the form the
    // caller's flags / HMV_TUNE_YW_FORM choose for the full fit -- the launch chain by each block's own padded size
    double* Ra = pl.at(gw.off_Ra);
    double* Rb = pl.at(gw.off_Rb);
    double* arr = pl.at(gw.off_arr);
    double* VrA = pl.at(gw.off_Vra);
    double* VrB = pl.at(gw.off_Vrb);
    int32_t* ir = reinterpret_cast<int32_t*>(pl.base + gw.off_ir);
    ga.red.VrA = VrA; ga.red.VrB = VrB;
    ga.red.info_rA = ir; ga.red.info_rB = ir + c;
    auto fit = [&](const double* Rx, int nx, double* Vx, int32_t* info) {
      const int mpx = pad_of(nx);
      return hmv::launch_yw(yw_args(Rx, c, nx, it.p, pl.ws, arr, Vx, info, pl.yw_flags(flags, mpx, c)), mpx, st0);
    };
    rc = hmv::launch_bgc_gather(pl.R, Ra, Rb, c, it.m, pl.mp, it.p, na, st0);
    if (!rc) rc = fit(Ra, na, VrA, ir);
    if (!rc) rc = fit(Rb, nb2, VrB, ir + c);
  }
  // the stage's full array goes to the output, or (band form) to scratch ahead of its band sums
  double* spec_c = !pl.bgc_spec ? nullptr : pl.bands ? pl.at(gw.off_full) : a.o.out + (size_t)i0 * 2 * F;
  ga.ar = ch.ar; ga.V = ch.V; ga.info_yw = a.fit.info_yw + i0;
  if (pl.bgc_spec) {
    ga.B = pl.at(gw.off_B); ga.C = pl.at(gw.off_C);
    ga.D = pl.at(gw.off_D); ga.cst = pl.at(gw.off_cst);
    ga.tw = pl.tw; ga.out = spec_c; ga.info_gc = g.info_gc + (size_t)i0 * F;
  }
  ga.n_items = c; ga.F = F; ga.m = it.m; ga.p = it.p; ga.split = na;
  if (!rc) rc = hmv::launch_bgc(ga, pl.mp, st0);
  if (!rc && pl.bgc_spec && pl.bands)
    rc = hmv::launch_band_sums(spec_c, reinterpret_cast<const int*>(a.o.bin_lo), reinterpret_cast<const int*>(a.o.bin_hi),
                               a.o.out + (size_t)i0 * 2 * a.o.n_bands, c * 2, F, a.o.n_bands, st0);
  return rc;
}

// ---- the measure stage of a chunk: GPDC or K3's ffDTF, then dDTF, band sums, spectra
int sliding_measure(const SlidingArgs& a, const SlidingPlan& pl, const Chunk& ch, hmv::TfSplit& sp) {
  const Items& it = a.it;
  const Output& o = a.o;
  const int64_t i0 = ch.i0, c = ch.c;
  const int F = a.spec.F, m = it.m;
  hipStream_t st0 = pl.fj.st0;
  const int* lo = reinterpret_cast<const int*>(o.bin_lo);
  const int* hi = reinterpret_cast<const int*>(o.bin_hi);
  double* Hc = o.S_out ? pl.at(pl.w.off_H) : nullptr;
  double* out_c = o.out + (size_t)i0 * m * m * (pl.bands ? o.n_bands : F);
  // dDTF / GPDC: the chunk's full array goes to the output, or (band form) to scratch ahead of its band sums;
  // ffDTF: K3 writes the output itself, the full array or (k3_bands) its band sums
  double* full_c = pl.k3_bands ? nullptr : (pl.bands ? pl.at(pl.w.off_full) : out_c);
  int rc;
  if (a.measure == MEAS_GPDC)
    rc = hmv::launch_gpdc_sliding(ch.ar, ch.V, pl.tw, full_c, c, F, m, pl.mp, it.p, st0);
  else
    rc = tf_ffdtf_impl(a.who, ch.ar, c, m, it.p, pl.tw, F, full_c, pl.k3_bands ? out_c : nullptr, o.bin_lo, o.bin_hi,
                       o.n_bands, pl.den, Hc, a.fit.info_tf + (size_t)i0 * F, a.fit.pivot_tau, pl.tfws, pl.tfws_bytes,
                       a.run.flags,
                       ch.last ? a.run.ev_k3_start : nullptr, ch.last ? a.run.ev_k3_stop : nullptr, st0,
                       pl.from_tiles ? pl.ws : nullptr, &sp);
  if (!rc && a.measure == MEAS_DDTF) {     // |kappa| from W(f) = A^T V^-1 A, multiplied into K3's ffDTF in place
    hmv::DdtfArgs da{};
    da.ar = ch.ar; da.V = ch.V; da.info_yw = a.fit.info_yw + i0;
    da.B = pl.at(pl.w.off_B); da.G = pl.at(pl.w.off_G);
    da.freqs = a.spec.freqs; da.fs = a.spec.fs; da.ff = full_c; da.out = full_c;
    da.n_items = c; da.F = F; da.m = m; da.p = it.p;
    rc = hmv::launch_ddtf_sliding(da, pl.mp, st0);
  }
  if (!rc && pl.bands && !pl.k3_bands)
    rc = hmv::launch_band_sums(full_c, lo, hi, out_c, c * (long long)m * m, F, o.n_bands, st0);
  if (!rc && o.S_out) {        // K5 from the same inverses and the same fit; V is this library's own (symmetric) estimate
    hmv::SpecArgs sa;
    sa.H = Hc; sa.V = ch.V; sa.S = nullptr; sa.S_mmf = o.S_out + (size_t)i0 * m * m * F * 2;
    sa.n_items = c; sa.F = F; sa.m = m; sa.sym = 1;
    rc = hmv::launch_spectra(sa, pl.mp, st0);
  }
  return rc;
}

// ---- the driver of the twelve fused entries: plan, twiddles, then per chunk K1, K2, the measure or block stage, join
int sliding_impl(const SlidingArgs& a) {
  SlidingPlan pl;
  int rc = sliding_plan(a, pl);
  if (rc || pl.empty) return rc;
  if (pl.bgc_spec) rc = hmv_twiddles_f64(a.spec.freqs, a.spec.F, a.spec.fs, a.it.p, pl.tw, a.run.stream);
  const int64_t n = a.it.n_items, chunk = a.run.chunk;
  hmv::TfSplit sp{};                         // the chunk's K2 -> K3 hand-over in two parts, if any
  for (int64_t i0 = 0; i0 < n && rc == 0; i0 += chunk) {
    const Chunk ch{i0, n - i0 < chunk ? n - i0 : chunk, a.fit.ar_out ? a.fit.ar_out + (size_t)i0 * pl.t * a.it.p : pl.ar,
                   a.fit.V_out ? a.fit.V_out + (size_t)i0 * pl.t : pl.V, i0 + chunk >= n};
    const SplitPoint s = sliding_split(a, pl, ch);
    if (s.front) {
      rc = sliding_front(a, pl, ch, s.c0, sp);
    } else {
      rc = sliding_k1(a, pl, ch);
      if (!rc) rc = sliding_k2(a, pl, ch, s.c0, sp);
    }
    if (!rc) rc = a.measure == MEAS_BGC ? sliding_bgc(a, pl, ch) : sliding_measure(a, pl, ch, sp);
    pl.fj.finish(sp);                        // (K3's launcher did not get to its second part, or the chunk ended on an error)
  }
  return rc;
}
}  // namespace

int64_t hmv_sliding_bands_workspace_bytes(int64_t chunk, int m, int p, int F) { return sliding_bytes(chunk, m, p, F, 1); }

int hmv_sliding_ffdtf_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                          const int64_t* item_start, int64_t n_items, int m, int n, int p,
                          const double* freqs, int F, double fs, double* ffdtf, double* ar_out, double* V_out,
                          int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes,
                          int64_t chunk, double pivot_tau, int64_t flags, int64_t grid_hop, int64_t grid_first,
                          int64_t grid_nwin, int64_t grid_T, void* ev_k3_start, void* ev_k3_stop, void* stream,
                          void* aux_stream) {
  return sliding_impl({"hmv_sliding_ffdtf_f64", MEAS_FFDTF, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, p},
                       {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs}, output(ffdtf),
                       {ar_out, V_out, info_yw, info_tf, pivot_tau},
                       {workspace, workspace_bytes, chunk, flags, stream, aux_stream, ev_k3_start, ev_k3_stop}});
}

int hmv_sliding_ffdtf_bands_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                                const int64_t* item_start, int64_t n_items, int m, int n, int p,
                                const double* freqs, int F, double fs, double* band_out, const int32_t* bin_lo,
                                const int32_t* bin_hi, int n_bands, double* ar_out, double* V_out,
                                int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes,
                                int64_t chunk, double pivot_tau, int64_t flags, int64_t grid_hop, int64_t grid_first,
                                int64_t grid_nwin, int64_t grid_T, void* ev_k3_start, void* ev_k3_stop, void* stream,
                                void* aux_stream) {
  const char* who = "hmv_sliding_ffdtf_bands_f64";
  if (int rc = need_output(who, band_out, n_items)) return rc;
  return sliding_impl({who, MEAS_FFDTF, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, p},
                       {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs},
                       output(band_out, bin_lo, bin_hi, n_bands, true), {ar_out, V_out, info_yw, info_tf, pivot_tau},
                       {workspace, workspace_bytes, chunk, flags, stream, aux_stream, ev_k3_start, ev_k3_stop}});
}

int64_t hmv_sliding_spectra_workspace_bytes(int64_t chunk, int m, int p, int F) {
  return sliding_bytes(chunk, m, p, F, 0, true);
}

int hmv_sliding_ffdtf_spectra_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                                  const int64_t* item_start, int64_t n_items, int m, int n, int p,
                                  const double* freqs, int F, double fs, double* ffdtf, double* S_out, double* ar_out,
                                  double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace,
                                  int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                                  int64_t grid_hop, int64_t grid_first, int64_t grid_nwin, int64_t grid_T, void* stream,
                                  void* aux_stream) {
  const char* who = "hmv_sliding_ffdtf_spectra_f64";
  if (int rc = need_output(who, S_out, n_items)) return rc;
  return sliding_impl({who, MEAS_FFDTF, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, p},
                       {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs},
                       output(ffdtf, nullptr, nullptr, 0, false, S_out), {ar_out, V_out, info_yw, info_tf, pivot_tau},
                       {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr}});
}

// ---- sliding-window dDTF / GPDC (sliding_conn.hip) ------------------------------------------------------
// direct_dtf (/root/reference/src/mtmvar.py:341-385) and gen_partial_directed_coherence (mtmvar.py:388-468) of every
// window; n_bands = 0: the full (m, m, F) arrays, n_bands >= 1: their band sums.
int64_t hmv_sliding_ddtf_workspace_bytes(int64_t chunk, int m, int p, int F, int n_bands) {
  return sliding_bytes(chunk, m, p, F, n_bands, false, MEAS_DDTF);
}

namespace {
// what the two entries share: GPDC comes without info_tf and without a pivot threshold (it inverts nothing)
int sliding_conn_entry(const char* who, int measure, const Items& it, const Grid& grid, const Spectral& spec, double* out,
                       const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, const FitOut& fit, const Run& run) {
  if (n_bands < 0) return refuse(who, -4, "n_bands must be >= 0");
  if (int rc = need_output(who, out, it.n_items)) return rc;
  return sliding_impl({who, measure, it, grid, spec, output(out, bin_lo, bin_hi, n_bands), fit, run});
}
}  // namespace

int hmv_sliding_ddtf_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                         const int64_t* item_start, int64_t n_items, int m, int n, int p, const double* freqs, int F,
                         double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace,
                         int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags, int64_t grid_hop,
                         int64_t grid_first, int64_t grid_nwin, int64_t grid_T, void* stream, void* aux_stream) {
  return sliding_conn_entry("hmv_sliding_ddtf_f64", MEAS_DDTF, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, p},
                            {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs}, out, bin_lo, bin_hi, n_bands,
                            {ar_out, V_out, info_yw, info_tf, pivot_tau},
                            {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr});
}

int64_t hmv_sliding_gpdc_workspace_bytes(int64_t chunk, int m, int p, int F, int n_bands) {
  return sliding_bytes(chunk, m, p, F, n_bands, false, MEAS_GPDC);
}

int hmv_sliding_gpdc_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                         const int64_t* item_start, int64_t n_items, int m, int n, int p, const double* freqs, int F,
                         double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* ar_out, double* V_out, int32_t* info_yw, void* workspace, int64_t workspace_bytes,
                         int64_t chunk, int64_t flags, int64_t grid_hop, int64_t grid_first, int64_t grid_nwin,
                         int64_t grid_T, void* stream, void* aux_stream) {
  return sliding_conn_entry("hmv_sliding_gpdc_f64", MEAS_GPDC, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, p},
                            {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs}, out, bin_lo, bin_hi, n_bands,
                            {ar_out, V_out, info_yw, nullptr, 1.0},
                            {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr});
}

// ---- block Granger causality (block_gc.hip) ----------------------------------------------------------------------
namespace {
// the checks the three block Granger entries share; 0 or the refusal
int bgc_check(const char* who, int m, int p, int split, int F) {
  if (pad_of(m) < 0) return refuse(who, -1, "channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return refuse(who, -2, "model order must be in 1..32");
  if (split < 1 || split > m - 1) return refuse(who, -11, "split must be in 1..m-1 (both blocks need a channel)");
  if (F < 1) return refuse(who, -12, "the frequency grid is empty (F must be >= 1)");
  return 0;
}
}  // namespace

int64_t hmv_block_gc_workspace_bytes(int64_t n_items, int m, int p, int split, int F) {
  if (pad_of(m) < 0 || n_items < 1 || p < 1 || p > HMV_MAX_ORDER || split < 1 || split > m - 1 || F < 1) return -1;
  return (int64_t)bgc_layout(align256(sizeof(double) * F * p * 2), n_items, m, p, F, split, false, false).total;
}

int hmv_block_gc_f64(const double* ar, const double* V, int64_t n_items, int m, int p, int split, const double* freqs, int F,
                     double fs, double* spectral, int32_t* info_v, int32_t* info_gc, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  if (int rc = bgc_check("hmv_block_gc_f64", m, p, split, F)) return rc;
  if (n_items < 0) return fail(-4, "hmv_block_gc_f64: n_items must be >= 0");
  if (n_items == 0) return 0;
  if (!spectral) return fail(-13, "hmv_block_gc_f64: the spectral output is a null pointer");
  if (!ar || !V || !freqs || !info_v || !info_gc || !workspace) return fail(-4, "hmv_block_gc_f64: null pointer");
  const size_t front = align256(sizeof(double) * F * p * 2);
  const BgcWs gw = bgc_layout(front, n_items, m, p, F, split, false, false);
  if ((int64_t)gw.total > workspace_bytes) return fail(-7, "hmv_block_gc_f64: workspace too small");
  char* base = static_cast<char*>(workspace);
  double* tw = reinterpret_cast<double*>(base);
  int rc = hmv_twiddles_f64(freqs, F, fs, p, tw, stream);
  if (rc) return rc;
  rc = (int)hipMemsetAsync(info_v, 0, sizeof(int32_t) * n_items, S(stream));
  if (rc) return rc;
  hmv::BgcArgs ga{};
  ga.ar = ar; ga.V = V; ga.info_yw = info_v;
  ga.B = reinterpret_cast<double*>(base + gw.off_B); ga.C = reinterpret_cast<double*>(base + gw.off_C);
  ga.D = reinterpret_cast<double*>(base + gw.off_D); ga.cst = reinterpret_cast<double*>(base + gw.off_cst);
  ga.tw = tw; ga.out = spectral; ga.info_gc = info_gc;
  ga.n_items = n_items; ga.F = F; ga.m = m; ga.p = p; ga.split = split;
  return hmv::launch_bgc(ga, pad_of(m), S(stream));
}

int64_t hmv_block_gc_sliding_workspace_bytes(int64_t chunk, int m, int p, int split, int F, int n_bands) {
  const int mp = pad_of(m);
  if (mp < 0 || chunk < 1 || p < 1 || p > HMV_MAX_ORDER || split < 1 || split > m - 1 || F < 1 || n_bands < 0) return -1;
  const SlidingWs w = sliding_layout(chunk, mp, p, F, n_bands > 0, false, MEAS_BGC);
  return (int64_t)bgc_layout(w.total, chunk, m, p, F, split, n_bands > 0, true).total;
}

int hmv_sliding_block_gc_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                             const int64_t* item_start, int64_t n_items, int m, int n, int p, int split,
                             const double* freqs, int F, double fs, double* spectral, const int32_t* bin_lo,
                             const int32_t* bin_hi, int n_bands, double* time, double* ar_out, double* V_out,
                             int32_t* info_yw, int32_t* info_red, int32_t* info_gc, void* workspace,
                             int64_t workspace_bytes, int64_t chunk, int64_t flags, int64_t grid_hop, int64_t grid_first,
                             int64_t grid_nwin, int64_t grid_T, void* stream) {
  const char* who = "hmv_sliding_block_gc_f64";
  if (int rc = bgc_check(who, m, p, split, F)) return rc;
  if (n <= p) return refuse(who, -3, "window shorter than the model order");
  if (n_items < 0) return refuse(who, -4, "n_items must be >= 0");
  if (n_bands < 0) return refuse(who, -14, "n_bands must be >= 0");
  if (n_items != 0 && !spectral) return refuse(who, -13, "the spectral output is a null pointer");
  if (n_items != 0 && (!time || !info_red || !info_gc)) return refuse(who, -4, "null pointer / empty grid");
  const BgcDesc g{split, time, info_red, info_gc};
  SlidingArgs a{who, MEAS_BGC, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, p},
                {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs}, output(spectral, bin_lo, bin_hi, n_bands),
                {ar_out, V_out, info_yw, nullptr, 1.0},
                {workspace, workspace_bytes, chunk, flags, stream, nullptr, nullptr, nullptr}};
  a.bgc = &g;
  return sliding_impl(a);
}

// ---- block Granger causality of pairs of recordings: the pair K1 in front of the stage (its surrogate tests) -----------
int64_t hmv_block_gc_pairs_workspace_bytes(int64_t chunk, int m, int n, int p, int split, int F, int n_bands, int want) {
  const int mp = pad_of(m);
  if (mp < 0 || chunk < 1 || p < 1 || p > HMV_MAX_ORDER || n <= p || split < 1 || split > m - 1 || want < 1 || want > 3) return -1;
  if ((want & 1) && (F < 1 || n_bands < 0)) return -1;
  const bool bands = (want & 1) && n_bands > 0;
  if (!(want & 1)) F = 0;                                // time alone takes no frequency grid
  const SlidingWs w = sliding_layout(chunk, mp, p, F, bands, false, MEAS_BGC, 0);
  return (int64_t)bgc_layout(w.total, chunk, m, p, F, split, bands, (want & 2) != 0, (want & 1) != 0).total;
}

int hmv_sliding_block_gc_pairs_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* rec_a,
                                   const int64_t* rec_b, const int64_t* item_start, int64_t n_items, int m, int n, int p,
                                   int split, const double* freqs, int F, double fs, double* spectral, const int32_t* bin_lo,
                                   const int32_t* bin_hi, int n_bands, double* time, double* ar_out, double* V_out,
                                   int32_t* info_yw, int32_t* info_red, int32_t* info_gc, void* workspace,
                                   int64_t workspace_bytes, int64_t chunk, int64_t flags, const double* R_base,
                                   const int64_t* base_a, const int64_t* base_b, int want, double* red_out,
                                   const double* red_base, const int32_t* info_red_base, void* stream) {
  const char* who = "hmv_sliding_block_gc_pairs_f64";
  (void)T;                                               // the caller has checked the windows against it
  if (want < 1 || want > 3) return refuse(who, -15, "want must be 1 (spectral), 2 (time) or 3 (both)");
  const bool spec = want & 1, timed = want & 2;
  if (int rc = bgc_check(who, m, p, split, spec ? F : 1)) return rc;
  if (n <= p) return refuse(who, -3, "window shorter than the model order");
  if (n_items < 0) return refuse(who, -4, "n_items must be >= 0");
  if (spec && n_bands < 0) return refuse(who, -14, "n_bands must be >= 0");
  if (int rc = pairs_check(who, m, rec_b, split, R_base, base_a, base_b)) return rc;
  if ((red_base != nullptr) != (info_red_base != nullptr)) return refuse(who, -4, "red_base and info_red_base go together");
  if (red_base && !R_base) return refuse(who, -4, "red_base needs R_base, base_a and base_b (its rows are theirs)");
  if (n_items != 0 && spec && !spectral) return refuse(who, -13, "the spectral output is a null pointer");
  if (n_items != 0 && ((spec && !info_gc) || (timed && (!time || !info_red))))
    return refuse(who, -4, "null pointer / empty grid");
  const PairDesc pairs{rec_b, split, R_base, base_a, base_b};
  BgcDesc g{split, time, info_red, info_gc};
  g.want = want;
  if (timed) { g.red_out = red_out; g.red_base = red_base; g.info_red_base = info_red_base; }
  // (time alone: neither a frequency grid nor a spectral output)
  SlidingArgs a{who, MEAS_BGC, {x, rec_stride, ld, rec_a, item_start, n_items, m, n, p}, {0, 0, 0, 0},
                spec ? Spectral{freqs, F, fs} : Spectral{nullptr, 0, fs},
                spec ? output(spectral, bin_lo, bin_hi, n_bands) : output(nullptr), {ar_out, V_out, info_yw, nullptr, 1.0},
                {workspace, workspace_bytes, chunk, flags, stream, nullptr, nullptr, nullptr}};
  a.bgc = &g;
  a.pairs = &pairs;
  return sliding_impl(a);
}

// ---- automatic model order (yw_auto.hip): mvar_criterion (mtmvar.py:551-601) per window inside the fused call -------
int64_t hmv_sliding_auto_workspace_bytes(int measure, int64_t chunk, int m, int pmax, int F, int n_bands) {
  return measure_bytes(measure, chunk, m, pmax, F, n_bands, -1);
}

int hmv_sliding_auto_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                         const int64_t* item_start, int64_t n_items, int m, int n, int pmax, int crit, const double* freqs,
                         int F, double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* S_out, double* ar_out, double* V_out, int32_t* order_out, double* crit_out,
                         int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes, int64_t chunk,
                         double pivot_tau, int64_t flags, int64_t grid_hop, int64_t grid_first, int64_t grid_nwin,
                         int64_t grid_T, void* stream, void* aux_stream) {
  const char* who = "hmv_sliding_auto_f64";
  FitOut fit{ar_out, V_out, info_yw, info_tf, pivot_tau};
  if (int rc = measure_request(who, measure, n_bands, S_out, fit, crit)) return rc;
  if (int rc = need_output(who, out, n_items)) return rc;
  SlidingArgs a{who, measure, {x, rec_stride, ld, item_rec, item_start, n_items, m, n, pmax},
                {grid_hop, grid_first, grid_nwin, grid_T}, {freqs, F, fs},
                output(out, bin_lo, bin_hi, n_bands, false, S_out), fit,
                {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr}};
  a.sel = {crit, order_out, crit_out};
  return sliding_impl(a);
}

// ---- event-locked ensembles: the fused path with the trial-averaged K1 (lagcov_ensemble.hip) ----------------------------
int64_t hmv_sliding_ensemble_workspace_bytes(int measure, int64_t chunk, int m, int n, int p, int F, int n_bands,
                                             int64_t grid_hop, int64_t grid_nwin) {
  if (n <= p || grid_hop < 0 || grid_nwin < 0) return -1;
  // (ens_q_tiles sees chunk, m and p before sliding_bytes range-checks them: it guards every division itself)
  return measure_bytes(measure, chunk, m, p, F, n_bands, ens_q_tiles(chunk, n, p, grid_hop, grid_nwin));
}

namespace {
// The entries whose K1 is not the single-trial one (ensemble, ensemble split, pairs, mix): measure-coded, no declared grid
// but the ensemble's own two numbers, no K3 events.  `a` comes with its items, spectral request and run filled in.
int sliding_k1_entry(SlidingArgs a, int measure, double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                     double* S_out, FitOut fit) {
  if (int rc = measure_request(a.who, measure, n_bands, S_out, fit)) return rc;
  if (int rc = need_output_after_sizes(a.who, a.it, out)) return rc;
  a.measure = measure;
  a.o = output(out, bin_lo, bin_hi, n_bands, false, S_out);
  a.fit = fit;
  return sliding_impl(a);
}
}  // namespace

int hmv_sliding_ensemble_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                             const int64_t* trial_rec, const int64_t* trial_start, const int64_t* group_ptr,
                             int64_t n_groups, const int64_t* item_group, const int64_t* item_offset, int64_t n_items,
                             int m, int n, int p, const double* freqs, int F, double fs, double* out,
                             const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out, double* ar_out,
                             double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes,
                             int64_t chunk, double pivot_tau, int64_t flags, int64_t grid_hop, int64_t grid_nwin,
                             void* stream, void* aux_stream) {
  const EnsDesc ens{trial_rec, trial_start, group_ptr, n_groups, T};
  SlidingArgs a{"hmv_sliding_ensemble_f64", MEAS_FFDTF, {x, rec_stride, ld, item_group, item_offset, n_items, m, n, p},
                {grid_hop, 0, grid_nwin, T}, {freqs, F, fs}, {}, {},
                {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr}};
  a.ens = &ens;
  return sliding_k1_entry(a, measure, out, bin_lo, bin_hi, n_bands, S_out, {ar_out, V_out, info_yw, info_tf, pivot_tau});
}

int hmv_sliding_ensemble_split_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, int64_t T,
                                   const int64_t* trial_rec, const int64_t* trial_start, const int64_t* group_ptr,
                                   int64_t n_groups, const int64_t* item_group, const int64_t* item_offset, int64_t n_items,
                                   int m, int n, int p, const double* freqs, int F, double fs, double* out,
                                   const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out, double* ar_out,
                                   double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace,
                                   int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                                   const int64_t* trial_rec_b, const int64_t* trial_start_b, int split, const double* R_base,
                                   const int64_t* item_base, void* stream, void* aux_stream) {
  const char* who = "hmv_sliding_ensemble_split_f64";
  if (pad_of(m) >= 0)                                    // (a bad channel count is the driver's -1)
    if (int rc = ens_split_check(who, m, trial_rec_b, trial_start_b, split, R_base, item_base)) return rc;
  EnsDesc ens{trial_rec, trial_start, group_ptr, n_groups, T};
  ens.trial_rec_b = trial_rec_b; ens.trial_start_b = trial_start_b; ens.split = split; ens.R_base = R_base;
  ens.item_base = item_base;
  SlidingArgs a{who, MEAS_FFDTF, {x, rec_stride, ld, item_group, item_offset, n_items, m, n, p}, {0, 0, 0, T}, {freqs, F, fs},
                {}, {}, {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr}};
  a.ens = &ens;
  return sliding_k1_entry(a, measure, out, bin_lo, bin_hi, n_bands, S_out, {ar_out, V_out, info_yw, info_tf, pivot_tau});
}

// ---- pairs of recordings: the fused path with the pair K1 (pseudo-dyad surrogates) -------------------------------------
int64_t hmv_pairs_workspace_bytes(int measure, int64_t chunk, int m, int n, int p, int F, int n_bands) {
  if (n <= p) return -1;
  return measure_bytes(measure, chunk, m, p, F, n_bands, 0);
}

int hmv_sliding_pairs_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* rec_a,
                          const int64_t* rec_b, const int64_t* item_start, int64_t n_items, int m, int n, int p,
                          const double* freqs, int F, double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi,
                          int n_bands, double* S_out, double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                          void* workspace, int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags, int split,
                          const double* R_base, const int64_t* base_a, const int64_t* base_b, void* stream,
                          void* aux_stream) {
  const char* who = "hmv_sliding_pairs_f64";
  (void)T;                                               // the caller has checked the windows against it
  if (pad_of(m) >= 0)                                    // (a bad channel count is the driver's -1)
    if (int rc = pairs_check(who, m, rec_b, split, R_base, base_a, base_b)) return rc;
  const PairDesc pairs{rec_b, split, R_base, base_a, base_b};
  SlidingArgs a{who, MEAS_FFDTF, {x, rec_stride, ld, rec_a, item_start, n_items, m, n, p}, {0, 0, 0, 0}, {freqs, F, fs},
                {}, {}, {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr}};
  a.pairs = &pairs;
  return sliding_k1_entry(a, measure, out, bin_lo, bin_hi, n_bands, S_out, {ar_out, V_out, info_yw, info_tf, pivot_tau});
}

// ---- weighted trial sums: the fused path with the mix K1 (label permutations of the condition contrast) ----------------
int hmv_lagcov_mix_f64(const double* Rt, int64_t n_trials, int64_t n_win, const double* W, const double* scale,
                       int64_t n_mix, int m, int p, double* R, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_lagcov_mix_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_lagcov_mix_f64: model order must be in 1..32");
  if (n_trials < 1 || n_win < 1 || n_mix < 1) return fail(-10, "hmv_lagcov_mix_f64: n_trials, n_win and n_mix must be >= 1");
  if (!Rt || !W || !R || reinterpret_cast<uintptr_t>(Rt) % 16 != 0 || reinterpret_cast<uintptr_t>(R) % 16 != 0)
    return fail(-4, "hmv_lagcov_mix_f64: null or misaligned pointer");
  hmv::LagcovMixArgs ma{};
  ma.Rt = Rt; ma.W = W; ma.scale = scale; ma.n_trials = n_trials; ma.n_win = n_win;
  ma.it0 = 0; ma.n_items = n_mix * n_win; ma.m = m; ma.m_pad = mp; ma.p = p; ma.R = R;
  return hmv::launch_lagcov_mix(ma, S(stream));
}

int64_t hmv_mix_workspace_bytes(int measure, int64_t chunk, int m, int p, int F, int n_bands) {
  return measure_bytes(measure, chunk, m, p, F, n_bands, 0);
}

int hmv_sliding_mix_f64(int measure, const double* Rt, int64_t n_trials, int64_t n_win, const double* W, const double* scale,
                        int64_t n_mix, int m, int n, int p, const double* freqs, int F, double fs, double* out,
                        const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out, double* ar_out,
                        double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes,
                        int64_t chunk, double pivot_tau, int64_t flags, void* stream, void* aux_stream) {
  // (bad sizes: an empty batch as far as the entry's own check goes; the driver refuses them in their turn)
  const bool sizes_ok = n_trials >= 1 && n_win >= 1 && n_mix >= 1;
  const MixDesc mix{Rt, W, scale, n_trials, n_win, n_mix};
  SlidingArgs a{"hmv_sliding_mix_f64", MEAS_FFDTF, {nullptr, 0, 0, nullptr, nullptr, sizes_ok ? n_mix * n_win : 0, m, n, p},
                {0, 0, 0, 0}, {freqs, F, fs}, {}, {},
                {workspace, workspace_bytes, chunk, flags, stream, aux_stream, nullptr, nullptr}};
  a.mix = &mix;
  return sliding_k1_entry(a, measure, out, bin_lo, bin_hi, n_bands, S_out, {ar_out, V_out, info_yw, info_tf, pivot_tau});
}

int64_t hmv_fad_workspace_bytes(int64_t n_series, int pmax) {
  return (n_series < 0 || pmax < 1 || pmax > HMV_MAX_ORDER) ? -1 : 0;
}

int hmv_fad_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec, const int64_t* item_start,
                int64_t n_items, int m, int n, int pmax, int order, int crit, double fs, double imag_tol,
                int pair_conjugates, int32_t* order_out, double* crit_out, double* ar, double* noise_variance,
                double* poles, double* C, double* alpha, double* freq, double* beta, double* bandwidth, double* phi,
                double* B, uint8_t* osc_mask, int32_t* paired, int32_t* n_paired, int32_t* info, void* stream) {
  if (m < 1 || m > HMV_MAX_CHANNELS) return fail(-1, "hmv_fad_f64: channel count must be in 1..64");
  if (pmax < 1 || pmax > HMV_MAX_ORDER) return fail(-2, "hmv_fad_f64: maximum model order must be in 1..32");
  if (n <= pmax) return fail(-3, "hmv_fad_f64: series shorter than the model order");
  if (!x || !item_rec || !item_start || !order_out || !ar || !noise_variance || !poles || !C || !alpha || !freq ||
      !beta || !bandwidth || !phi || !B || !osc_mask || !paired || !n_paired || !info || n_items < 0)
    return fail(-4, "hmv_fad_f64: null pointer");
  if (crit < 0 || crit > 2) return fail(-5, "hmv_fad_f64: criterion must be 0 (AIC), 1 (HQ) or 2 (SC)");
  if (order < 0 || order > pmax) return fail(-6, "hmv_fad_f64: model order must be 0 (automatic) or in 1..pmax");
  hmv::FadArgs a{};
  a.from_fit = 1;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld;
  a.item_rec = reinterpret_cast<const long long*>(item_rec);
  a.item_start = reinterpret_cast<const long long*>(item_start);
  a.n_series = n_items * m; a.m = m; a.n = n; a.pmax = pmax; a.order = order; a.crit = crit;
  a.fs = fs; a.imag_tol = imag_tol; a.pair_conjugates = pair_conjugates != 0;
  a.order_out = order_out; a.crit_out = crit_out; a.ar = ar; a.noise = noise_variance;
  a.poles = poles; a.C = C; a.alpha = alpha; a.freq = freq; a.beta = beta; a.bw = bandwidth; a.phi = phi; a.B = B;
  a.osc = osc_mask; a.paired = paired; a.n_paired = n_paired; a.info = info;
  return hmv::launch_fad(a, S(stream));
}

int hmv_fad_decompose_f64(const double* ar, int64_t n_series, int p, double fs, double imag_tol, int pair_conjugates,
                          double* poles, double* C, double* alpha, double* freq, double* beta, double* bandwidth,
                          double* phi, double* B, uint8_t* osc_mask, int32_t* paired, int32_t* n_paired, int32_t* info,
                          void* stream) {
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_fad_decompose_f64: model order must be in 1..32");
  if (!ar || !poles || !C || !alpha || !freq || !beta || !bandwidth || !phi || !B || !osc_mask || !paired ||
      !n_paired || !info || n_series < 0)
    return fail(-4, "hmv_fad_decompose_f64: null pointer");
  hmv::FadArgs a{};
  a.from_fit = 0;
  a.n_series = n_series; a.pmax = p;
  a.fs = fs; a.imag_tol = imag_tol; a.pair_conjugates = pair_conjugates != 0;
  a.ar = const_cast<double*>(ar);
  a.poles = poles; a.C = C; a.alpha = alpha; a.freq = freq; a.beta = beta; a.bw = bandwidth; a.phi = phi; a.B = B;
  a.osc = osc_mask; a.paired = paired; a.n_paired = n_paired; a.info = info;
  return hmv::launch_fad(a, S(stream));
}

// ---- surrogate significance (surrogate.hip) --------------------------------------------------------------------
int hmv_surrogate_shift_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, const int64_t* item_rec,
                            const int64_t* item_start, int64_t n_win, const int64_t* shift, int64_t n_rec, int n_surr, int m,
                            int n, int split, double* out, void* stream) {
  if (m < 1 || m > HMV_MAX_CHANNELS) return fail(-1, "hmv_surrogate_shift_f64: channel count must be in 1..64");
  if (n < 2 || n > T) return fail(-3, "hmv_surrogate_shift_f64: window length must be in 2..T");
  if (split < 1 || split >= m) return fail(-5, "hmv_surrogate_shift_f64: split must be in 1..m-1");
  if (n_surr < 1) return fail(-6, "hmv_surrogate_shift_f64: surrogate count must be >= 1");
  if (n_win < 0 || n_rec < 1) return fail(-4, "hmv_surrogate_shift_f64: bad window / recording count");
  if (n_win == 0) return 0;
  if (!x || !item_rec || !item_start || !shift || !out) return fail(-4, "hmv_surrogate_shift_f64: null pointer");
  return hmv::launch_surrogate_shift(x, rec_stride, ld, T, reinterpret_cast<const long long*>(item_rec),
                                     reinterpret_cast<const long long*>(item_start), n_win,
                                     reinterpret_cast<const long long*>(shift), n_rec, n_surr, m, n, split, out, S(stream));
}

int hmv_surrogate_phase_c128(const double* spec, int64_t n_win, const double* phi, int n_surr, int m, int n, double* out,
                             void* stream) {
  if (m < 1 || m > HMV_MAX_CHANNELS) return fail(-1, "hmv_surrogate_phase_c128: channel count must be in 1..64");
  if (n < 2) return fail(-3, "hmv_surrogate_phase_c128: window length must be >= 2");
  if (n_surr < 1) return fail(-6, "hmv_surrogate_phase_c128: surrogate count must be >= 1");
  if (n_win < 0) return fail(-4, "hmv_surrogate_phase_c128: bad window count");
  if (n_win == 0) return 0;
  if (!spec || !phi || !out) return fail(-4, "hmv_surrogate_phase_c128: null pointer");
  return hmv::launch_surrogate_phase(spec, n_win, phi, n_surr, m, n, out, S(stream));
}

int hmv_null_accumulate_f64(const double* observed, const double* surr, const uint8_t* surr_bad, const uint8_t* tested,
                            int64_t n_win, int n_surr, int m, int n_bands, double* M, int32_t* n_valid, int32_t* count,
                            int32_t* count_fwe, int32_t* n_cell, double* mean, double* m2, double* p, double* p_fwe,
                            double* null_mean, double* null_std, void* stream) {
  if (m < 1 || m > HMV_MAX_CHANNELS) return fail(-1, "hmv_null_accumulate_f64: channel count must be in 1..64");
  if (n_bands < 1) return fail(-2, "hmv_null_accumulate_f64: band count must be >= 1");
  if (n_surr < 1) return fail(-6, "hmv_null_accumulate_f64: surrogate count must be >= 1");
  if (n_win < 0) return fail(-4, "hmv_null_accumulate_f64: bad window count");
  const int fin = (p != nullptr) + (p_fwe != nullptr) + (null_mean != nullptr) + (null_std != nullptr);
  if (fin != 0 && fin != 4) return fail(-7, "hmv_null_accumulate_f64: p, p_fwe, null_mean and null_std go together");
  if (n_win == 0) return 0;
  if (!observed || !surr || !surr_bad || !tested || !M || !n_valid || !count || !count_fwe || !n_cell || !mean || !m2)
    return fail(-4, "hmv_null_accumulate_f64: null pointer");
  hmv::NullAccArgs a{};
  a.obs = observed; a.surr = surr; a.bad = surr_bad; a.tested = tested;
  a.n_win = n_win; a.n_surr = n_surr; a.m = m; a.nb = n_bands;
  a.M = M; a.n_valid = n_valid; a.cnt = count; a.cnt_fwe = count_fwe; a.n_cell = n_cell; a.mean = mean; a.m2 = m2;
  a.p = p; a.p_fwe = p_fwe; a.null_mean = null_mean; a.null_std = null_std;
  return hmv::launch_null_accumulate(a, S(stream));
}

// ---- model validation (validate.hip) ---------------------------------------------------------------------------
namespace {
// workspace of hmv_model_validation_f64 for a chunk: packed coefficients | E | C | item_rec, item_start of the residuals
struct ValidationLayout {
  size_t arp, E, C, idx, total;
  int64_t ldE;
};
ValidationLayout validation_layout(int64_t chunk, int mp, int m, int n, int p, int h) {
  ValidationLayout L{};
  L.ldE = ((int64_t)(n - p) + 3) & ~int64_t(3);
  size_t off = 0;
  L.arp = off; off += align256(sizeof(double) * (size_t)hmv::resid_pack_doubles(chunk, mp, p));
  L.E = off;   off += align256(sizeof(double) * (size_t)chunk * m * L.ldE);
  L.C = off;   off += align256(sizeof(double) * (size_t)chunk * (h + 1) * mp * mp);
  L.idx = off; off += align256(sizeof(int64_t) * 2 * (size_t)chunk);
  L.total = off;
  return L;
}
}  // namespace

int64_t hmv_residuals_workspace_bytes(int64_t chunk_items, int m, int p) {
  const int mp = pad_of(m);
  if (mp < 0 || p < 1 || p > HMV_MAX_ORDER || chunk_items < 1) return -1;
  return (int64_t)sizeof(double) * hmv::resid_pack_doubles(chunk_items, mp, p);
}

int hmv_residuals_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec, const int64_t* item_start,
                      int64_t n_items, int m, int n, int p, const double* ar, double* E, int64_t ldE, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_residuals_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_residuals_f64: model order must be in 1..32");
  if (n <= p) return fail(-3, "hmv_residuals_f64: window shorter than the model order");
  if (!x || !item_rec || !item_start || !ar || !E || !workspace || n_items < 0)
    return fail(-4, "hmv_residuals_f64: null pointer");
  const int64_t per_item = hmv_residuals_workspace_bytes(1, m, p);
  if (workspace_bytes < per_item) return fail(-7, "hmv_residuals_f64: workspace too small");
  if (ldE < n - p) return fail(-8, "hmv_residuals_f64: ldE is smaller than n - p");
  const int64_t chunk = workspace_bytes / per_item;
  for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
    hmv::ResidArgs a{};
    a.x = x; a.rec_stride = rec_stride; a.ld = ld;
    a.item_rec = reinterpret_cast<const long long*>(item_rec) + i0;
    a.item_start = reinterpret_cast<const long long*>(item_start) + i0;
    a.n_items = n_items - i0 < chunk ? n_items - i0 : chunk;
    a.m = m; a.n = n; a.p = p;
    a.ar = ar + (size_t)i0 * mp * mp * p;
    a.arp = static_cast<double*>(workspace);
    a.E = E + (size_t)i0 * m * ldE; a.ldE = ldE;
    const int rc = hmv::launch_residuals(a, mp, S(stream));
    if (rc) return rc;
  }
  return 0;
}

int hmv_whiteness_f64(const double* C, int64_t n_items, int m, int N, int h, double acf_thr, double* s, double* q,
                      double* q_ch, int32_t* acf_count, int32_t* info, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_whiteness_f64: channel count must be in 1..64");
  if (h < 1 || h > HMV_MAX_ORDER) return fail(-6, "hmv_whiteness_f64: number of tested lags must be in 1..32");
  if (N <= h) return fail(-3, "hmv_whiteness_f64: no more residuals than tested lags");
  if (!C || !s || !q || !q_ch || !acf_count || !info || n_items < 0) return fail(-4, "hmv_whiteness_f64: null pointer");
  hmv::WhiteArgs a{};
  a.C = C; a.n_items = n_items; a.m = m; a.N = N; a.h = h; a.acf_thr = acf_thr;
  a.s = s; a.q = q; a.q_ch = q_ch; a.acf_count = acf_count; a.info = info;
  return hmv::launch_whiteness(a, mp, S(stream));
}

int64_t hmv_model_validation_workspace_bytes(int64_t chunk, int m, int n, int p, int h) {
  const int mp = pad_of(m);
  if (mp < 0 || p < 1 || p > HMV_MAX_ORDER || h < 1 || h > HMV_MAX_ORDER || (int64_t)n - p <= h || chunk < 1) return -1;
  return (int64_t)validation_layout(chunk, mp, m, n, p, h).total;
}

int hmv_model_validation_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                             const int64_t* item_start, int64_t n_items, int m, int n, int p, const double* ar, int h,
                             double acf_thr, double* s, double* q, double* q_ch, int32_t* acf_count, int32_t* info,
                             double* resid_cov, double* E_out, int64_t ldE, void* workspace, int64_t workspace_bytes,
                             int64_t chunk, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_model_validation_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_model_validation_f64: model order must be in 1..32");
  if (h < 1 || h > HMV_MAX_ORDER) return fail(-6, "hmv_model_validation_f64: number of tested lags must be in 1..32");
  if ((int64_t)n - p <= h) return fail(-3, "hmv_model_validation_f64: no more residuals than tested lags");
  if (!x || !item_rec || !item_start || !ar || !s || !q || !q_ch || !acf_count || !info || !workspace || n_items < 0)
    return fail(-4, "hmv_model_validation_f64: null pointer");
  if (chunk < 1 || workspace_bytes < hmv_model_validation_workspace_bytes(chunk, m, n, p, h))
    return fail(-7, "hmv_model_validation_f64: workspace too small");
  if (E_out && ldE < n - p) return fail(-8, "hmv_model_validation_f64: ldE is smaller than n - p");
  const ValidationLayout L = validation_layout(chunk, mp, m, n, p, h);
  char* ws = static_cast<char*>(workspace);
  const int N = n - p;
  long long* rec_e = reinterpret_cast<long long*>(ws + L.idx);
  long long* start_e = rec_e + chunk;
  for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
    const int64_t cnt = n_items - i0 < chunk ? n_items - i0 : chunk;
    hmv::ResidArgs r{};
    r.x = x; r.rec_stride = rec_stride; r.ld = ld;
    r.item_rec = reinterpret_cast<const long long*>(item_rec) + i0;
    r.item_start = reinterpret_cast<const long long*>(item_start) + i0;
    r.n_items = cnt; r.m = m; r.n = n; r.p = p;
    r.ar = ar + (size_t)i0 * mp * mp * p;
    r.arp = reinterpret_cast<double*>(ws + L.arp);
    r.E = E_out ? E_out + (size_t)i0 * m * ldE : reinterpret_cast<double*>(ws + L.E);
    r.ldE = E_out ? ldE : L.ldE;
    int rc = hmv::launch_residuals(r, mp, S(stream));
    if (rc) return rc;
    // K1 over the residuals: `cnt` recordings of N samples, h lags
    rc = hmv::launch_iota_items(rec_e, start_e, cnt, S(stream));
    if (rc) return rc;
    hmv::LagcovArgs c{};
    c.x = r.E; c.rec_stride = (long long)m * r.ldE; c.ld = r.ldE; c.item_rec = rec_e; c.item_start = start_e;
    c.n_items = cnt; c.m = m; c.n = N; c.p = h; c.R = reinterpret_cast<double*>(ws + L.C);
    rc = hmv::launch_lagcov(c, mp, S(stream));
    if (rc) return rc;
    hmv::WhiteArgs w{};
    w.C = c.R; w.n_items = cnt; w.m = m; w.N = N; w.h = h; w.acf_thr = acf_thr;
    w.s = s + (size_t)i0 * h; w.q = q + (size_t)i0 * 3; w.q_ch = q_ch + (size_t)i0 * m;
    w.acf_count = acf_count + i0; w.info = info + i0;
    w.resid_cov = resid_cov ? resid_cov + (size_t)i0 * mp * mp : nullptr;
    rc = hmv::launch_whiteness(w, mp, S(stream));
    if (rc) return rc;
  }
  return 0;
}

// ---- FIR decimation of recordings (decimate.hip) ------------------------------------------------------------------
int64_t hmv_decimate_out_len(int64_t T, int q) {
  if (T < 1 || q < 2 || q > HMV_MAX_DECIMATE) return -1;
  return (T + q - 1) / q;
}

int hmv_decimate_tile(int q, int n_taps) {
  if (q < 2 || q > HMV_MAX_DECIMATE || n_taps < 3 || n_taps > HMV_MAX_DECIMATE_TAPS || n_taps % 2 == 0) return -1;
  return hmv::decimate_tile(q, n_taps);
}

int hmv_decimate_fir_f64(const double* x, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m, int q,
                         const double* h, int n_taps, double* y, int64_t y_rec_stride, int64_t y_ld, void* stream) {
  if (q < 2 || q > HMV_MAX_DECIMATE) return fail(-1, "hmv_decimate_fir_f64: decimation factor must be in 2..32");
  if (n_taps < 3 || n_taps > HMV_MAX_DECIMATE_TAPS || n_taps % 2 == 0)
    return fail(-2, "hmv_decimate_fir_f64: the number of taps must be odd and in 3..641");
  if (T < 1 || n_rec < 0 || m < 1) return fail(-3, "hmv_decimate_fir_f64: bad sample / recording / channel count");
  if (T > (int64_t(1) << 40)) return fail(-7, "hmv_decimate_fir_f64: recordings longer than 2^40 samples are not supported");
  if (n_rec == 0) return 0;
  if (!x || !h || !y) return fail(-4, "hmv_decimate_fir_f64: null pointer");
  if (ld < T) return fail(-5, "hmv_decimate_fir_f64: ld is smaller than T");
  if (y_ld < hmv_decimate_out_len(T, q)) return fail(-6, "hmv_decimate_fir_f64: y_ld is smaller than ceil(T / q)");
  hmv::DecimateArgs a{};
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.T = T; a.n_rec = n_rec; a.m = m; a.q = q;
  a.h = h; a.n_taps = n_taps; a.y = y; a.y_rec_stride = y_rec_stride; a.y_ld = y_ld;
  return hmv::launch_decimate(a, S(stream));
}

// ---- phase synchrony and phase-lag family of analytic signals (phase_sync.hip, phase_lag.hip) ----------------------------
namespace {
// What the three phase entries refuse, in the order they refuse it: phase_head, the entry's own arguments, phase_layout,
// the empty batch (0, with whatever pointers), phase_tail.  Each returns 0 when its arguments are fine.
int phase_head(const char* who, int64_t T, int64_t n_rec, int m, int64_t n_items, int n) {
  if (pad_of(m) < 0) return refuse(who, -1, "channel count must be in 1..64");
  if (T < 1 || n_rec < 0 || n_items < 0) return refuse(who, -3, "bad sample / recording / item count");
  if (n_items > 0x7fffffffLL) return refuse(who, -10, "more than 2^31 - 1 items in one call");
  if (n < 1 || n > T) return refuse(who, -2, "window length must be in 1..T");
  return 0;
}
int phase_mode(const char* who, int mode) {
  if (mode == HMV_PHASE_UNIT || mode == HMV_PHASE_RAW) return 0;
  return refuse(who, -7, "mode must be HMV_PHASE_UNIT (0) or HMV_PHASE_RAW (1)");
}
int phase_layout(const char* who, int64_t rec_stride, int64_t ld, int64_t T, int m) {
  if (ld < T) return refuse(who, -5, "ld is smaller than T");
  if (ld > INT64_MAX / m || rec_stride < (int64_t)m * ld) return refuse(who, -6, "rec_stride is smaller than m * ld");
  return 0;
}
int phase_tail(const char* who, const double* z, bool pointers) {
  if (!z || !pointers) return refuse(who, -4, "null pointer");
  if (reinterpret_cast<uintptr_t>(z) % 16) return refuse(who, -8, "z is not 16-byte aligned");
  return 0;
}
// the head that PhaseSyncArgs, PhasePairsArgs and PhaseLagArgs have in common (a template: not of C linkage)
extern "C++" template <class Args>
Args phase_args(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int64_t n_items, int m, int n,
                int32_t* info) {
  Args a{};
  a.z = reinterpret_cast<const double2*>(z); a.rec_stride = rec_stride; a.ld = ld; a.T = T; a.n_rec = n_rec;
  a.n_items = n_items; a.m = m; a.n = n; a.info = info;
  return a;
}
}  // namespace

int hmv_phase_sync_c128(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m,
                        const int64_t* item_rec, const int64_t* item_start, int64_t n_items, int n, int mode,
                        double* coherency, double* mag, double* lagged, int32_t* info, void* stream) {
  const char* who = "hmv_phase_sync_c128";
  if (int rc = phase_head(who, T, n_rec, m, n_items, n)) return rc;
  if (int rc = phase_mode(who, mode)) return rc;
  if (!coherency && !mag && !lagged) return refuse(who, -9, "no output requested (coherency, mag, lagged all null)");
  if (int rc = phase_layout(who, rec_stride, ld, T, m)) return rc;
  if (n_items == 0) return 0;
  if (int rc = phase_tail(who, z, item_rec && item_start && info)) return rc;
  auto a = phase_args<hmv::PhaseSyncArgs>(z, rec_stride, ld, T, n_rec, n_items, m, n, info);
  a.item_rec = ll(item_rec); a.item_start = ll(item_start); a.mode = mode;
  a.coherency = coherency; a.mag = mag; a.lagged = lagged;
  return hmv::launch_phase_sync(a, pad_of(m), S(stream));
}

int hmv_phase_sync_pairs_c128(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m, int split,
                              const int64_t* rec_a, const int64_t* rec_b, const int64_t* item_start, const int64_t* shift_b,
                              int64_t n_items, int n, int mode, double* values, int val_stride, int col_mag, int col_lagged,
                              int32_t* info, void* stream) {
  const char* who = "hmv_phase_sync_pairs_c128";
  if (int rc = phase_head(who, T, n_rec, m, n_items, n)) return rc;
  if (int rc = phase_mode(who, mode)) return rc;
  if (split < 1 || split > m - 1) return refuse(who, -11, "split must be in 1..m-1");
  if (val_stride < 1 || col_mag < -1 || col_mag >= val_stride || col_lagged < -1 || col_lagged >= val_stride ||
      col_mag == col_lagged)        // equal columns: both -1 (no output) or one column asked to hold two values
    return refuse(who, -12, "val_stride must be >= 1 and col_mag, col_lagged two different columns in -1..val_stride-1, not "
                            "both -1");
  if (int rc = phase_layout(who, rec_stride, ld, T, m)) return rc;
  if (n_items == 0) return 0;
  if (int rc = phase_tail(who, z, rec_a && rec_b && item_start && values && info)) return rc;
  auto a = phase_args<hmv::PhasePairsArgs>(z, rec_stride, ld, T, n_rec, n_items, m, n, info);
  a.rec_a = ll(rec_a); a.rec_b = ll(rec_b); a.item_start = ll(item_start); a.shift_b = ll(shift_b);
  a.mode = mode; a.split = split;
  a.values = values; a.val_stride = val_stride; a.col_mag = col_mag; a.col_lagged = col_lagged;
  return hmv::launch_phase_sync_pairs(a, pad_of(m), S(stream));
}

int hmv_phase_lag_c128(const double* z, int64_t rec_stride, int64_t ld, int64_t T, int64_t n_rec, int m, int split,
                       const int64_t* item_rec, const int64_t* item_start, int64_t n_items, int n, double* pli, double* wpli,
                       double* dwpli, int32_t* info, void* stream) {
  const char* who = "hmv_phase_lag_c128";
  if (int rc = phase_head(who, T, n_rec, m, n_items, n)) return rc;
  if (split < 0 || split > m - 1) return refuse(who, -11, "split must be in 0..m-1 (0: all pairs)");
  if (!pli && !wpli && !dwpli) return refuse(who, -9, "no output requested (pli, wpli, dwpli all null)");
  if (int rc = phase_layout(who, rec_stride, ld, T, m)) return rc;
  if (n_items == 0) return 0;
  if (int rc = phase_tail(who, z, item_rec && item_start && info)) return rc;
  auto a = phase_args<hmv::PhaseLagArgs>(z, rec_stride, ld, T, n_rec, n_items, m, n, info);
  a.item_rec = ll(item_rec); a.item_start = ll(item_start); a.split = split;
  a.pli = pli; a.wpli = wpli; a.dwpli = dwpli;
  return hmv::launch_phase_lag(a, pad_of(m), S(stream));
}

}  // extern "C"
