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
  char buf[160];
  const char* msg = nullptr;
  int code = -4;
  if (split < 1 || split >= m) { code = -5; msg = "split must be in 1..m-1"; }
  else if (!trial_rec_b || !trial_start_b) msg = "null pointer (second trial table)";
  else if ((R_base != nullptr) != (item_base != nullptr)) msg = "R_base and item_base go together";
  if (!msg) return 0;
  snprintf(buf, sizeof(buf), "%s: %s", who, msg);
  return fail(code, buf);
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
  char buf[160];
  const char* msg = nullptr;
  int code = -4;
  if (split < 1 || split >= m) { code = -5; msg = "split must be in 1..m-1"; }
  else if (!rec_b) msg = "null pointer (rec_b)";
  else if ((R_base != nullptr) != (base_a != nullptr) || (R_base != nullptr) != (base_b != nullptr))
    msg = "R_base, base_a and base_b go together";
  if (!msg) return 0;
  snprintf(buf, sizeof(buf), "%s: %s", who, msg);
  return fail(code, buf);
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

int hmv_yw_solve_f64(const double* R, int64_t n_items, int m, int p, double* ws, double* ar, double* V,
                     double* vq_logdet, int32_t* info, int64_t flags, void* stream) {
  const int mp = pad_of(m);
  if (mp < 0) return fail(-1, "hmv_yw_solve_f64: channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return fail(-2, "hmv_yw_solve_f64: model order must be in 1..32");
  if (!R || !ws || !ar || !V || !info || n_items < 0) return fail(-4, "hmv_yw_solve_f64: null pointer");
  if (vq_logdet && ((flags & HMV_FLAG_YW_PIVOTED) || hmv::tuning(HMV_TUNE_YW_FORM) == 5))
    return fail(-6, "hmv_yw_solve_f64: the pivoted LU gives no criterion curve (vq_logdet must be NULL)");
  hmv::YwArgs a{};
  a.R = R; a.n_items = n_items; a.m = m; a.p = p; a.ws = ws; a.ar = ar; a.V = V;
  a.Vq_logdet = vq_logdet; a.info = info; a.tiled = (flags & HMV_FLAG_YW_TILED) ? 1 : ((flags & HMV_FLAG_YW_ONE_LAUNCH) ? 0 : -1);
  a.pivoted = (flags & HMV_FLAG_YW_PIVOTED) ? 1 : 0;
  return hmv::launch_yw(a, mp, S(stream));
}

namespace {
// c of the criterion's penalty c q m^2 / n (mtmvar.py:580-587); crit as in hmv_fad_f64: 0 AIC, 1 HQ, 2 SC
double crit_factor(int crit, int n) {
  return crit == 0 ? 2.0 : (crit == 1 ? 2.0 * log(log((double)n)) : log((double)n));
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
  hmv::YwArgs a{};
  a.R = R; a.n_items = n_items; a.m = m; a.p = pmax; a.ws = ws; a.ar = ar; a.V = V; a.Vq_logdet = vq_logdet; a.info = info;
  a.tiled = -1;
  hmv::YwAutoArgs sel{};
  sel.n = n; sel.crit_c = crit_factor(crit, n); sel.order_out = order_out; sel.crit_out = crit_out;
  return hmv::launch_yw_auto(a, sel, mp, S(stream));
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
  auto failw = [&](int code, const char* msg) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, msg);
    return fail(code, buf);
  };
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
// Fork / join events of the two-stream K2 split: created once per (host thread, device), not per call.
struct ForkJoin {
  hipEvent_t fork = nullptr, join = nullptr;
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
  }
  return &e;
}
// Where a chunk of c windows is handed from K2 to K3 in two parts (HMV_TUNE_K3_SPLIT), or 0 for one part.  K2 runs one
// workgroup per window, all of them resident at once while c < occupancy * CUs, and lasts as long as the fullest compute
// unit's windows take: with k = c / CUs full rounds and r = c % CUs windows over, r units carry k + 1 windows and the others
// wait for them.  The r windows over are then solved on the second stream while K3 starts on the first c0 = c - r.  Chunks of
// several rounds (k >= occupancy) are not split, nor are chunks whose first part is shorter than K3's normalisation lag.
// CUs and occupancy come from the runtime, once per (host thread, device, padded size).
int64_t k3_split_point(int64_t c, int mp, int64_t lag) {
  const int64_t t = hmv::tuning(HMV_TUNE_K3_SPLIT);
  int64_t c0 = t;
  if (t < 0) return 0;
  if (t == 0) {
    constexpr int MAXDEV = 64;
    struct Shape { int cus = 0, occ[4] = {0, 0, 0, 0}; };
    thread_local Shape tl[MAXDEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV || mp < 16 || mp > 64) return 0;
    Shape& d = tl[dev];
    int& occ = d.occ[mp / 16 - 1];
    if (d.cus == 0 && hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) d.cus = -1;
    if (occ == 0 && (occ = hmv::yw_lwr_occupancy(mp)) == 0) occ = -1;
    if (d.cus < 1 || occ < 1) {
      (void)hipGetLastError();                           // (a failed query must not surface as a later launch's error)
      return 0;
    }
    const int64_t k = c / d.cus, r = c % d.cus;
    if (k < 1 || k >= occ || r == 0) return 0;
    c0 = c - r;
  }
  return (c0 >= lag && c0 < c) ? c0 : 0;
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
// Everything sliding_impl is told, by name; a field left alone means "not asked for".  The exported entries below fill in
// what they have.  `ffdtf` receives the full (m, m, F) arrays, `band_out` (with bin_lo / bin_hi / n_bands) the band sums.
struct SlidingArgs {
  const char* who;                                  // the entry's own name, for hmv_last_error()
  const double* x = nullptr;
  int64_t rec_stride = 0, ld = 0;
  const int64_t* item_rec = nullptr;                // (ensemble: item_group)
  const int64_t* item_start = nullptr;              // (ensemble: item_offset)
  int64_t n_items = 0;
  int m = 0, n = 0, p = 0;
  const double* freqs = nullptr;
  int F = 0;
  double fs = 0.0;
  double* ffdtf = nullptr;
  double* band_out = nullptr;
  const int32_t* bin_lo = nullptr;
  const int32_t* bin_hi = nullptr;
  int n_bands = 0;
  double* S_out = nullptr;
  double* ar_out = nullptr;
  double* V_out = nullptr;
  int32_t* info_yw = nullptr;
  int32_t* info_tf = nullptr;
  void* workspace = nullptr;
  int64_t workspace_bytes = 0, chunk = 0;
  double pivot_tau = 1.0;
  int64_t flags = 0, grid_hop = 0, grid_first = 0, grid_nwin = 0, grid_T = 0;
  void* ev_k3_start = nullptr;
  void* ev_k3_stop = nullptr;
  void* stream = nullptr;
  void* aux_stream = nullptr;
  int measure = MEAS_FFDTF;
  int crit = -1;                                    // >= 0: automatic order, with order_out (and crit_out)
  int32_t* order_out = nullptr;
  double* crit_out = nullptr;
  const EnsDesc* ens = nullptr;
  const PairDesc* pairs = nullptr;
  const MixDesc* mix = nullptr;
  const BgcDesc* bgc = nullptr;                     // measure == MEAS_BGC: `ffdtf` / `band_out` carry the spectral output
};
// K1 of the chunk i0 .. i0 + c - 1 into R, on st: whichever form the entry's descriptors and the grid call for
int sliding_k1(const SlidingArgs& a, int mp, bool ens_shared, bool regular, int64_t i0, int64_t c, double* R, double* Qb,
               hipStream_t st) {
  const K1In in{a.x, a.rec_stride, a.ld, a.item_rec, a.item_start, a.m, a.n, a.p};
  if (a.ens) {
    const hmv::LagcovEnsArgs ea = ens_args(in, *a.ens, i0, c, R, ens_shared ? Qb : nullptr, a.grid_hop, a.grid_nwin);
    return a.ens->split ? hmv::launch_lagcov_ensemble_split(ea, mp, st) : hmv::launch_lagcov_ensemble(ea, mp, ens_shared, st);
  }
  if (a.pairs) return hmv::launch_lagcov_pairs(pairs_args(in, *a.pairs, i0, c, R), mp, st);
  if (a.mix) {
    hmv::LagcovMixArgs ma{};
    ma.Rt = a.mix->Rt; ma.W = a.mix->W; ma.scale = a.mix->scale; ma.n_trials = a.mix->n_trials; ma.n_win = a.mix->n_win;
    ma.it0 = i0; ma.n_items = c; ma.m = a.m; ma.m_pad = mp; ma.p = a.p; ma.R = R;
    return hmv::launch_lagcov_mix(ma, st);
  }
  if (!regular) return hmv_lagcov_f64(a.x, a.rec_stride, a.ld, a.item_rec + i0, a.item_start + i0, c, a.m, a.n, a.p, R, st);
  // items i0 .. i0+c-1 as runs of consecutive windows of one recording each (item = rec * grid_nwin + w)
  const size_t stack = (size_t)(a.p + 1) * mp * mp;
  int rc = 0;
  for (int64_t it = i0; it < i0 + c && rc == 0;) {
    const int64_t rec = it / a.grid_nwin, w0 = it - rec * a.grid_nwin;
    const int64_t run = ((a.grid_nwin - w0) < (i0 + c - it)) ? (a.grid_nwin - w0) : (i0 + c - it);
    rc = hmv_lagcov_regular_f64(a.x + rec * a.rec_stride, a.ld, a.grid_T, a.grid_first + w0 * a.grid_hop, a.grid_hop, run,
                                a.m, a.n, a.p, R + (size_t)(it - i0) * stack, Qb, st);
    it += run;
  }
  return rc;
}
int sliding_impl(const SlidingArgs& a) {
  // crit >= 0: automatic order (hmv_sliding_auto_f64) -- p is the largest order tried, K1 sums p + 1 lags, K2 selects every
  // window's order and leaves its coefficients zero-padded to p lags, and every later stage runs at p on those (the
  // added terms of A(f) = I - sum_k ar_k tw_k are exact zeros)
  const bool automatic = a.crit >= 0;
  const bool bands = (a.band_out != nullptr);
  auto fail = [&](int code, const char* msg) {
    const char* own = strchr(msg, ':');             // messages below are written "hmv_sliding_ffdtf_f64: ..."
    char buf[220];
    snprintf(buf, sizeof(buf), "%s%s", a.who, own ? own : msg);
    return ::fail(code, buf);
  };
  const int mp = pad_of(a.m);
  if (mp < 0) return fail(-1, "hmv_sliding_ffdtf_f64: channel count must be in 1..64");
  if (a.p < 1 || a.p > HMV_MAX_ORDER) return fail(-2, "hmv_sliding_ffdtf_f64: model order must be in 1..32");
  if (a.n <= a.p) return fail(-3, "hmv_sliding_ffdtf_f64: window shorter than the model order");
  if (automatic && a.crit > 2) return fail(-5, "hmv_sliding_ffdtf_f64: criterion must be 0 (AIC), 1 (HQ) or 2 (SC)");
  if (automatic && (a.flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH)))
    return fail(-6, "hmv_sliding_ffdtf_f64: the LDL^T forms of K2 have no automatic order");
  if (automatic && (a.flags & HMV_FLAG_YW_PIVOTED))
    return fail(-6, "hmv_sliding_ffdtf_f64: the pivoted LU has no automatic order (no criterion curve)");
  if (a.mix && (a.mix->n_trials < 1 || a.mix->n_win < 1 || a.mix->n_mix < 1))
    return fail(-10, "hmv_sliding_ffdtf_f64: n_trials, n_win and n_mix must be >= 1");
  if (a.n_items == 0) return 0;                                    // empty batch: nothing to do, nothing to check
  if (automatic && !a.order_out) return fail(-4, "hmv_sliding_ffdtf_f64: null pointer / empty grid");
  if (a.mix ? (!a.mix->Rt || !a.mix->W || reinterpret_cast<uintptr_t>(a.mix->Rt) % 16 != 0)
            : (!a.x || !a.item_rec || !a.item_start))
    return fail(-4, "hmv_sliding_ffdtf_f64: null pointer / empty grid");
  const bool bgc_spec = !a.bgc || (a.bgc->want & 1), bgc_time = a.bgc && (a.bgc->want & 2);   // (time alone: no frequencies)
  if ((bgc_spec && (!a.freqs || (!a.ffdtf && !bands) || a.F < 1)) || !a.info_yw ||
      (!a.info_tf && (a.measure == MEAS_FFDTF || a.measure == MEAS_DDTF)) || !a.workspace || a.chunk < 1)
    return fail(-4, "hmv_sliding_ffdtf_f64: null pointer / empty grid");
  if (bands && (!a.bin_lo || !a.bin_hi || a.n_bands < 1)) return fail(-4, "hmv_sliding_ffdtf_f64: band bins missing");
  bool ens_shared = false;
  if (a.ens) {
    if (!a.ens->trial_rec || !a.ens->trial_start || !a.ens->group_ptr)
      return fail(-4, "hmv_sliding_ffdtf_f64: null pointer / empty grid");
    if (a.ens->n_groups < 1) return fail(-10, "hmv_sliding_ffdtf_f64: n_groups must be >= 1");
    if (a.grid_hop != 0 && !ens_grid_ok(a.n_items, a.ens->n_groups, a.n, a.ld, a.ens->T, a.grid_hop, a.grid_nwin))
      return fail(-9, "hmv_sliding_ffdtf_f64: inconsistent regular window grid");
    ens_shared = !a.ens->split && ens_shared_form(a.n, a.p, a.grid_hop, a.flags);
  }
  const SlidingWs w = sliding_layout(a.chunk, mp, a.p, a.F, bands, a.S_out != nullptr, a.measure,
                                     a.ens ? (ens_shared ? ens_q_tiles(a.chunk, a.n, a.p, a.grid_hop, a.grid_nwin) : 0)
                                           : ((a.pairs || a.mix) ? 0 : -1));
  BgcWs gw{};
  if (a.bgc) gw = bgc_layout(w.total, a.chunk, a.m, a.p, a.F, a.bgc->split, bands, bgc_time, bgc_spec);
  if ((int64_t)(a.bgc ? gw.total : w.total) > a.workspace_bytes) return fail(-7, "hmv_sliding_ffdtf_f64: workspace too small");
  // Regular grid (the caller vouches: item = rec * grid_nwin + w starts at grid_first + w * grid_hop of recording rec,
  // recordings are grid_T samples long): K1 sums every hop block once and assembles the windows from the blocks.
  bool regular = !a.ens && !a.pairs && !a.mix && a.grid_hop > 0 && !(a.flags & HMV_FLAG_DIRECT_LAGCOV);
  if (regular) {
    if (a.grid_nwin < 1 || a.grid_first < 0 || a.n_items % a.grid_nwin != 0 ||
        a.grid_first + (a.grid_nwin - 1) * a.grid_hop + a.n > a.grid_T || a.ld < a.grid_T)
      return fail(-9, "hmv_sliding_ffdtf_f64: inconsistent regular window grid");
    regular = (a.n % a.grid_hop == 0) && (a.n / a.grid_hop >= 2) && (a.n / a.grid_hop <= HMV_MAX_HOPS_PER_WINDOW) &&
              a.grid_hop > a.p;
  }
  // Second stream (HMV_FLAG_YW_TILED only): the tile-per-workgroup form of K2 is a chain of ~25 launches of at
  // most a few workgroups per window that cannot fill the chip; it runs as two half-batches, one per stream,
  // whose launches interleave on the device (fork after K1, join before K3).  The default one-launch form of K2
  // needs none of this.  Chunk pipelining (K1/K2 of chunk c+1 under K3 of chunk c) was measured and does NOT
  // work: K3 holds every wave slot and starves the other stream.
  // What the default form does with the second stream is a different thing (k3_split_point, profiles/k3_split_notes.md):
  // the work put beside K3 is the few windows of the SAME chunk that K2's last, partly filled round would make the whole
  // chip wait for, and it is placed before K3 arrives -- forked behind K2's first part, with only the light packing kernel
  // between the fork and K3, so its workgroups land on an almost empty chip and K3 fills in around them.  It is zero-sum
  // in chip time like the others; what it removes is the idle tail of K2 from the critical path.  Only where nobody but
  // K3's packing kernel reads the model (from_tiles below) and no output beyond the ffDTF is asked for.
  hipStream_t st0 = S(a.stream), st1 = S(a.aux_stream);
  const bool two = (a.aux_stream && a.aux_stream != a.stream);
  const bool split = two && !(a.flags & HMV_FLAG_YW_ONE_LAUNCH);
  const bool k3_split = two && !automatic && a.measure == MEAS_FFDTF && !a.S_out && !a.ar_out && !a.V_out &&
                        !(a.flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH));
  ForkJoin* fj = nullptr;
  if (split || k3_split) {
    fj = fork_join_events();
    if (!fj) return fail(-8, "hmv_sliding_ffdtf_f64: cannot create fork/join events");
  }
  int rc = 0;
  const size_t t = (size_t)mp * mp;
  const int64_t n_chunks = (a.n_items + a.chunk - 1) / a.chunk;
  char* base = static_cast<char*>(a.workspace);
  double* R = reinterpret_cast<double*>(base + w.off_R);
  double* Qb = reinterpret_cast<double*>(base + w.off_Q);
  double* ws = reinterpret_cast<double*>(base + w.off_ws);
  double* ar = reinterpret_cast<double*>(base + w.off_ar);
  double* V = reinterpret_cast<double*>(base + w.off_V);
  void* tfws = base + w.off_tf;
  double* den = reinterpret_cast<double*>(base + w.off_den);
  double* tw = reinterpret_cast<double*>(base + w.off_tw);
  const bool k3_bands = bands && a.measure == MEAS_FFDTF;
  const int64_t tfws_bytes = (int64_t)tf_ff_layout(a.chunk, mp, a.p, a.F, k3_bands).total;
  if (bgc_spec) rc = hmv_twiddles_f64(a.freqs, a.F, a.fs, a.p, tw, st0);
  const size_t ws_item = (size_t)hmv_yw_workspace_doubles(a.m, a.p);
  hmv::TfSplit sp{};                         // the chunk's K2 -> K3 hand-over in two parts, if any
  auto join_k3_split = [&]() {               // st0 joins st1 unless K3's launcher already made it wait
    if (sp.join && !sp.joined)
      if (hipStreamWaitEvent(st0, sp.join, 0) != hipSuccess) (void)hipStreamSynchronize(st1);
    sp.joined = true;
  };
  for (int64_t ci = 0; ci < n_chunks && rc == 0; ++ci) {
    const int64_t i0 = ci * a.chunk;
    const int64_t c = (a.n_items - i0 < a.chunk) ? (a.n_items - i0) : a.chunk;
    double* ar_c = a.ar_out ? a.ar_out + (size_t)i0 * t * a.p : ar;
    double* V_c = a.V_out ? a.V_out + (size_t)i0 * t : V;
    rc = sliding_k1(a, mp, ens_shared, regular, i0, c, R, Qb, st0);
    if (rc) break;
    if (automatic) {
      hmv::YwArgs ya{};
      ya.R = R; ya.n_items = c; ya.m = a.m; ya.p = a.p; ya.ws = ws; ya.ar = ar_c; ya.V = V_c; ya.info = a.info_yw + i0;
      ya.tiled = -1;
      hmv::YwAutoArgs sel{};
      sel.n = a.n; sel.crit_c = crit_factor(a.crit, a.n); sel.order_out = a.order_out + i0;
      sel.crit_out = a.crit_out ? a.crit_out + (size_t)i0 * a.p : nullptr;
      rc = hmv::launch_yw_auto(ya, sel, mp, st0);
      if (rc) break;
    }
    // the tiled form of K2 (asked for, or chosen for a large 64-channel chunk) as two half-batches
    // K2: the Levinson-Whittle recursion unless an LDL^T form is asked for (or HMV_TUNE_YW_FORM = 1, which picks the
    // LDL^T form by batch shape as before: the launch chain for large 64-channel chunks)
    const bool ldl = (a.flags & (HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH)) || hmv::tuning(HMV_TUNE_YW_FORM) == 1;
    const bool tiled = (a.flags & HMV_FLAG_YW_TILED) || (ldl && !(a.flags & HMV_FLAG_YW_ONE_LAUNCH) && mp == 64 && c >= 128);
    const int64_t yw_flags = (a.flags & ~(int64_t)(HMV_FLAG_YW_TILED | HMV_FLAG_YW_ONE_LAUNCH)) |
                             (ldl ? (tiled ? HMV_FLAG_YW_TILED : HMV_FLAG_YW_ONE_LAUNCH) : 0);
    const int64_t c0 = (split && tiled && c >= 16) ? (c + 1) / 2 : c, c1 = c - c0;
    if (c1 > 0 && !automatic) {
      // fork: st1 may start once K1 is done.  Whatever happens on st1 afterwards, st0 joins it again before this call
      // returns, so that the caller's stream never runs ahead of work this call put on the second stream.
      int hrc = (int)hipEventRecord(fj->fork, st0);
      if (!hrc) hrc = (int)hipStreamWaitEvent(st1, fj->fork, 0);
      if (hrc) { rc = hrc; break; }                      // nothing was put on st1
      rc = hmv_yw_solve_f64(R + (size_t)c0 * (a.p + 1) * t, c1, a.m, a.p, ws + (size_t)c0 * ws_item,
                            ar_c + (size_t)c0 * t * a.p, V_c + (size_t)c0 * t, nullptr, a.info_yw + i0 + c0, yw_flags, st1);
      hrc = (int)hipEventRecord(fj->join, st1);
      if (!hrc) hrc = (int)hipStreamWaitEvent(st0, fj->join, 0);
      if (hrc) {                                         // cannot express the join as an event: join on the host
        (void)hipStreamSynchronize(st1);
        if (!rc) rc = hrc;
      }
      if (rc) break;
    }
    // Nobody but K3's packing kernel reads the model when the caller does not ask for it and the measure is the ffDTF:
    // the default recursion then leaves it in its scratch tiles, which the packing kernel reads directly (windows that
    // the conditioning guard hands to the LDL^T re-solve come through `ar` as before).
    const int64_t yw_form = hmv::tuning(HMV_TUNE_YW_FORM);
    const bool from_tiles = !automatic && !a.ar_out && !ldl && (yw_form == 0 || yw_form == 2) && a.measure == MEAS_FFDTF;
    sp = hmv::TfSplit{};
    if (!automatic && from_tiles) {
      const int64_t s0 = k3_split ? k3_split_point(c, mp, norm_lag_items(mp, a.F)) : 0;
      hmv::YwArgs ya{};
      ya.R = R; ya.n_items = s0 ? s0 : c0; ya.m = a.m; ya.p = a.p; ya.ws = ws; ya.ar = ar_c; ya.V = V_c; ya.info = a.info_yw + i0;
      ya.tiled = -1; ya.no_emit = 1; ya.pivoted = (a.flags & HMV_FLAG_YW_PIVOTED) ? 1 : 0;
      rc = hmv::launch_yw(ya, mp, st0);
      if (!rc && s0) {
        // fork behind K2's first part (the remainder never shares a compute unit with it); the join is waited for inside
        // K3's launcher, between its two launches, or below on every path that did not get that far
        int hrc = (int)hipEventRecord(fj->fork, st0);
        if (!hrc) hrc = (int)hipStreamWaitEvent(st1, fj->fork, 0);
        if (hrc) { rc = hrc; break; }                    // nothing was put on st1
        hmv::YwArgs yb = ya;
        yb.R = R + (size_t)s0 * (a.p + 1) * t; yb.n_items = c - s0; yb.ws = ws + (size_t)s0 * ws_item;
        yb.ar = ar_c + (size_t)s0 * t * a.p; yb.V = V_c + (size_t)s0 * t; yb.info = a.info_yw + i0 + s0;
        rc = hmv::launch_yw(yb, mp, st1);
        hrc = (int)hipEventRecord(fj->join, st1);
        if (hrc) {                                       // cannot express the join as an event: join on the host, one K3 launch
          (void)hipStreamSynchronize(st1);
          if (!rc) rc = hrc;
        } else {
          sp.c0 = s0; sp.join = fj->join;
        }
      }
    } else if (!automatic) {
      rc = hmv_yw_solve_f64(R, c0, a.m, a.p, ws, ar_c, V_c, nullptr, a.info_yw + i0, yw_flags, st0);
    }
    if (rc) break;
    const bool last = (ci == n_chunks - 1);
    double* Hc = a.S_out ? reinterpret_cast<double*>(base + w.off_H) : nullptr;
    // dDTF / GPDC: the chunk's full array goes to the output, or (band form) to scratch ahead of its band sums
    double* full_c = (a.measure == MEAS_FFDTF || a.measure == MEAS_BGC) ? nullptr
                     : bands ? reinterpret_cast<double*>(base + w.off_full) : a.ffdtf + (size_t)i0 * a.m * a.m * a.F;
    if (a.measure == MEAS_BGC) {
      // the two restricted fits (K2 on the gathered blocks of the same lag covariances, in the scratch the full fit has
      // left, in the form the caller's flags / HMV_TUNE_YW_FORM choose for the full fit -- the launch chain by each
      // block's own padded size), then the stage; its full array goes to the output or (band form) to scratch ahead of
      // its band sums
      const int na = a.bgc->split, nb2 = a.m - na;
      hmv::BgcArgs ga{};
      ga.want = a.bgc->want;
      if (bgc_time) {
        ga.red.time = a.bgc->time + (size_t)i0 * 4; ga.red.info_red = a.bgc->info_red + (size_t)i0 * 2;
        ga.red.red_out = a.bgc->red_out ? a.bgc->red_out + (size_t)i0 * 2 : nullptr;
      }
      if (bgc_time && a.bgc->red_base) {
        // both restricted fits are those of observed windows (a pair changes the cross blocks only): their log-determinants
        // and infos come from the table, and nothing is gathered or solved
        ga.red.red_base = a.bgc->red_base; ga.red.info_red_base = a.bgc->info_red_base;
        ga.red.base_a = ll(a.pairs->base_a + i0); ga.red.base_b = ll(a.pairs->base_b + i0);
      } else if (bgc_time) {
        double* Ra = reinterpret_cast<double*>(base + gw.off_Ra);
        double* Rb = reinterpret_cast<double*>(base + gw.off_Rb);
        double* arr = reinterpret_cast<double*>(base + gw.off_arr);
        int32_t* ir = reinterpret_cast<int32_t*>(base + gw.off_ir);
        ga.red.VrA = reinterpret_cast<double*>(base + gw.off_Vra); ga.red.VrB = reinterpret_cast<double*>(base + gw.off_Vrb);
        ga.red.info_rA = ir; ga.red.info_rB = ir + c;
        auto red_flags = [&](int nx) {
          const bool chain = (a.flags & HMV_FLAG_YW_TILED) ||
                             (ldl && !(a.flags & HMV_FLAG_YW_ONE_LAUNCH) && pad_of(nx) == 64 && c >= 128);
          return (int64_t)(ldl ? (chain ? HMV_FLAG_YW_TILED : HMV_FLAG_YW_ONE_LAUNCH) : 0) | (a.flags & HMV_FLAG_YW_PIVOTED);
        };
        rc = hmv::launch_bgc_gather(R, Ra, Rb, c, a.m, mp, a.p, na, st0);
        if (!rc)
          rc = hmv_yw_solve_f64(Ra, c, na, a.p, ws, arr, const_cast<double*>(ga.red.VrA), nullptr, ir, red_flags(na), st0);
        if (!rc)
          rc = hmv_yw_solve_f64(Rb, c, nb2, a.p, ws, arr, const_cast<double*>(ga.red.VrB), nullptr, ir + c, red_flags(nb2),
                                st0);
      }
      double* spec_c = !bgc_spec ? nullptr
                       : bands   ? reinterpret_cast<double*>(base + gw.off_full) : a.ffdtf + (size_t)i0 * 2 * a.F;
      ga.ar = ar_c; ga.V = V_c; ga.info_yw = a.info_yw + i0;
      if (bgc_spec) {
        ga.B = reinterpret_cast<double*>(base + gw.off_B); ga.C = reinterpret_cast<double*>(base + gw.off_C);
        ga.D = reinterpret_cast<double*>(base + gw.off_D); ga.cst = reinterpret_cast<double*>(base + gw.off_cst);
        ga.tw = tw; ga.out = spec_c; ga.info_gc = a.bgc->info_gc + (size_t)i0 * a.F;
      }
      ga.n_items = c; ga.F = a.F; ga.m = a.m; ga.p = a.p; ga.split = na;
      if (!rc) rc = hmv::launch_bgc(ga, mp, st0);
      if (!rc && bgc_spec && bands)
        rc = hmv::launch_band_sums(spec_c, reinterpret_cast<const int*>(a.bin_lo), reinterpret_cast<const int*>(a.bin_hi),
                                   a.band_out + (size_t)i0 * 2 * a.n_bands, c * 2, a.F, a.n_bands, st0);
    } else if (a.measure == MEAS_GPDC) {
      rc = hmv::launch_gpdc_sliding(ar_c, V_c, tw, full_c, c, a.F, a.m, mp, a.p, st0);
    } else {
      rc = tf_ffdtf_impl(a.who, ar_c, c, a.m, a.p, tw, a.F,
                         k3_bands ? nullptr : (full_c ? full_c : a.ffdtf + (size_t)i0 * a.m * a.m * a.F),
                         k3_bands ? a.band_out + (size_t)i0 * a.m * a.m * a.n_bands : nullptr, a.bin_lo, a.bin_hi,
                         a.n_bands, den, Hc, a.info_tf + (size_t)i0 * a.F, a.pivot_tau, tfws, tfws_bytes, a.flags,
                         last ? a.ev_k3_start : nullptr, last ? a.ev_k3_stop : nullptr, st0, from_tiles ? ws : nullptr, &sp);
    }
    join_k3_split();                         // (K3's launcher did not get to its second part)
    if (!rc && a.measure == MEAS_DDTF) {     // |kappa| from W(f) = A^T V^-1 A, multiplied into K3's ffDTF in place
      hmv::DdtfArgs da{};
      da.ar = ar_c; da.V = V_c; da.info_yw = a.info_yw + i0;
      da.B = reinterpret_cast<double*>(base + w.off_B); da.G = reinterpret_cast<double*>(base + w.off_G);
      da.freqs = a.freqs; da.fs = a.fs; da.ff = full_c; da.out = full_c;
      da.n_items = c; da.F = a.F; da.m = a.m; da.p = a.p;
      rc = hmv::launch_ddtf_sliding(da, mp, st0);
    }
    if (!rc && (a.measure == MEAS_DDTF || a.measure == MEAS_GPDC) && bands)
      rc = hmv::launch_band_sums(full_c, reinterpret_cast<const int*>(a.bin_lo), reinterpret_cast<const int*>(a.bin_hi),
                                 a.band_out + (size_t)i0 * a.m * a.m * a.n_bands, c * (long long)a.m * a.m, a.F,
                                 a.n_bands, st0);
    if (!rc && a.S_out) {      // K5 from the same inverses and the same fit; V is this library's own (symmetric) estimate
      hmv::SpecArgs sa;
      sa.H = Hc; sa.V = V_c; sa.S = nullptr; sa.S_mmf = a.S_out + (size_t)i0 * a.m * a.m * a.F * 2;
      sa.n_items = c; sa.F = a.F; sa.m = a.m; sa.sym = 1;
      rc = hmv::launch_spectra(sa, mp, st0);
    }
  }
  join_k3_split();                           // a chunk that ended on an error between the fork and K3
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
  SlidingArgs a{"hmv_sliding_ffdtf_f64"};
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  a.ffdtf = ffdtf;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.ev_k3_start = ev_k3_start; a.ev_k3_stop = ev_k3_stop;
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
}

int hmv_sliding_ffdtf_bands_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                                const int64_t* item_start, int64_t n_items, int m, int n, int p,
                                const double* freqs, int F, double fs, double* band_out, const int32_t* bin_lo,
                                const int32_t* bin_hi, int n_bands, double* ar_out, double* V_out,
                                int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes,
                                int64_t chunk, double pivot_tau, int64_t flags, int64_t grid_hop, int64_t grid_first,
                                int64_t grid_nwin, int64_t grid_T, void* ev_k3_start, void* ev_k3_stop, void* stream,
                                void* aux_stream) {
  if (!band_out && n_items != 0) return fail(-4, "hmv_sliding_ffdtf_bands_f64: null pointer / empty grid");
  SlidingArgs a{"hmv_sliding_ffdtf_bands_f64"};
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  a.band_out = band_out; a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.ev_k3_start = ev_k3_start; a.ev_k3_stop = ev_k3_stop;
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
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
  if (!S_out && n_items != 0) return fail(-4, "hmv_sliding_ffdtf_spectra_f64: null pointer / empty grid");
  SlidingArgs a{"hmv_sliding_ffdtf_spectra_f64"};
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  a.ffdtf = ffdtf; a.S_out = S_out;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
}

// ---- sliding-window dDTF / GPDC (sliding_conn.hip) ------------------------------------------------------
// direct_dtf (/root/reference/src/mtmvar.py:341-385) and gen_partial_directed_coherence (mtmvar.py:388-468) of every
// window; n_bands = 0: the full (m, m, F) arrays, n_bands >= 1: their band sums.
int64_t hmv_sliding_ddtf_workspace_bytes(int64_t chunk, int m, int p, int F, int n_bands) {
  return sliding_bytes(chunk, m, p, F, n_bands, false, MEAS_DDTF);
}

int hmv_sliding_ddtf_f64(const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                         const int64_t* item_start, int64_t n_items, int m, int n, int p, const double* freqs, int F,
                         double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace,
                         int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags, int64_t grid_hop,
                         int64_t grid_first, int64_t grid_nwin, int64_t grid_T, void* stream, void* aux_stream) {
  if (n_bands < 0) return fail(-4, "hmv_sliding_ddtf_f64: n_bands must be >= 0");
  if (!out && n_items != 0) return fail(-4, "hmv_sliding_ddtf_f64: null pointer / empty grid");
  SlidingArgs a{"hmv_sliding_ddtf_f64"};
  a.measure = MEAS_DDTF;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = out; else a.ffdtf = out;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
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
  if (n_bands < 0) return fail(-4, "hmv_sliding_gpdc_f64: n_bands must be >= 0");
  if (!out && n_items != 0) return fail(-4, "hmv_sliding_gpdc_f64: null pointer / empty grid");
  SlidingArgs a{"hmv_sliding_gpdc_f64"};
  a.measure = MEAS_GPDC;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = out; else a.ffdtf = out;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.flags = flags;
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
}

// ---- block Granger causality (block_gc.hip) ----------------------------------------------------------------------
namespace {
// the checks the three block Granger entries share; 0 or the refusal
int bgc_check(const char* who, int m, int p, int split, int F) {
  char buf[200];
  auto refuse = [&](int code, const char* msg) {
    snprintf(buf, sizeof(buf), "%s: %s", who, msg);
    return fail(code, buf);
  };
  if (pad_of(m) < 0) return refuse(-1, "channel count must be in 1..64");
  if (p < 1 || p > HMV_MAX_ORDER) return refuse(-2, "model order must be in 1..32");
  if (split < 1 || split > m - 1) return refuse(-11, "split must be in 1..m-1 (both blocks need a channel)");
  if (F < 1) return refuse(-12, "the frequency grid is empty (F must be >= 1)");
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
  if (n <= p) return fail(-3, "hmv_sliding_block_gc_f64: window shorter than the model order");
  if (n_items < 0) return fail(-4, "hmv_sliding_block_gc_f64: n_items must be >= 0");
  if (n_bands < 0) return fail(-14, "hmv_sliding_block_gc_f64: n_bands must be >= 0");
  if (n_items != 0 && !spectral) return fail(-13, "hmv_sliding_block_gc_f64: the spectral output is a null pointer");
  if (n_items != 0 && (!time || !info_red || !info_gc)) return fail(-4, "hmv_sliding_block_gc_f64: null pointer / empty grid");
  BgcDesc g{split, time, info_red, info_gc};
  SlidingArgs a{who};
  a.measure = MEAS_BGC; a.bgc = &g;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = spectral; else a.ffdtf = spectral;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.flags = flags;
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.stream = stream;
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
  if (want < 1 || want > 3)
    return fail(-15, "hmv_sliding_block_gc_pairs_f64: want must be 1 (spectral), 2 (time) or 3 (both)");
  const bool spec = want & 1, timed = want & 2;
  if (int rc = bgc_check(who, m, p, split, spec ? F : 1)) return rc;
  if (n <= p) return fail(-3, "hmv_sliding_block_gc_pairs_f64: window shorter than the model order");
  if (n_items < 0) return fail(-4, "hmv_sliding_block_gc_pairs_f64: n_items must be >= 0");
  if (spec && n_bands < 0) return fail(-14, "hmv_sliding_block_gc_pairs_f64: n_bands must be >= 0");
  if (int rc = pairs_check(who, m, rec_b, split, R_base, base_a, base_b)) return rc;
  if ((red_base != nullptr) != (info_red_base != nullptr))
    return fail(-4, "hmv_sliding_block_gc_pairs_f64: red_base and info_red_base go together");
  if (red_base && !R_base)
    return fail(-4, "hmv_sliding_block_gc_pairs_f64: red_base needs R_base, base_a and base_b (its rows are theirs)");
  if (n_items != 0 && spec && !spectral) return fail(-13, "hmv_sliding_block_gc_pairs_f64: the spectral output is a null pointer");
  if (n_items != 0 && ((spec && !info_gc) || (timed && (!time || !info_red))))
    return fail(-4, "hmv_sliding_block_gc_pairs_f64: null pointer / empty grid");
  const PairDesc pairs{rec_b, split, R_base, base_a, base_b};
  BgcDesc g{split, time, info_red, info_gc};
  g.want = want;
  if (timed) { g.red_out = red_out; g.red_base = red_base; g.info_red_base = info_red_base; }
  SlidingArgs a{who};
  a.measure = MEAS_BGC; a.bgc = &g; a.pairs = &pairs;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = rec_a; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.fs = fs;
  if (spec) {
    a.freqs = freqs; a.F = F;
    if (n_bands > 0) a.band_out = spectral; else a.ffdtf = spectral;
    a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands;
  }
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.flags = flags;
  a.stream = stream;
  return sliding_impl(a);
}

// ---- automatic model order (yw_auto.hip): mvar_criterion (mtmvar.py:551-601) per window inside the fused call -------
int64_t hmv_sliding_auto_workspace_bytes(int measure, int64_t chunk, int m, int pmax, int F, int n_bands) {
  // n_bands = -1: the full ffDTF together with S_out (one chunk of H passes through the workspace between K3 and K5)
  const bool spectra = (n_bands == -1 && measure == HMV_MEASURE_FFDTF);
  return sliding_bytes(chunk, m, pmax, F, spectra ? 0 : n_bands, spectra, measure);
}

int hmv_sliding_auto_f64(int measure, const double* x, int64_t rec_stride, int64_t ld, const int64_t* item_rec,
                         const int64_t* item_start, int64_t n_items, int m, int n, int pmax, int crit, const double* freqs,
                         int F, double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi, int n_bands,
                         double* S_out, double* ar_out, double* V_out, int32_t* order_out, double* crit_out,
                         int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes, int64_t chunk,
                         double pivot_tau, int64_t flags, int64_t grid_hop, int64_t grid_first, int64_t grid_nwin,
                         int64_t grid_T, void* stream, void* aux_stream) {
  if (measure < HMV_MEASURE_FFDTF || measure > HMV_MEASURE_GPDC)
    return fail(-4, "hmv_sliding_auto_f64: measure must be HMV_MEASURE_FFDTF, _DDTF or _GPDC");
  if (crit < 0 || crit > 2) return fail(-5, "hmv_sliding_auto_f64: criterion must be 0 (AIC), 1 (HQ) or 2 (SC)");
  if (n_bands < 0) return fail(-4, "hmv_sliding_auto_f64: n_bands must be >= 0");
  if (S_out && (measure != HMV_MEASURE_FFDTF || n_bands != 0))
    return fail(-4, "hmv_sliding_auto_f64: spectra come with the full ffDTF only");
  if (!out && n_items != 0) return fail(-4, "hmv_sliding_auto_f64: null pointer / empty grid");
  SlidingArgs a{"hmv_sliding_auto_f64"};
  a.measure = measure; a.crit = crit; a.order_out = order_out; a.crit_out = crit_out;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_rec; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = pmax; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = out; else a.ffdtf = out;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands; a.S_out = S_out;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  if (measure == HMV_MEASURE_GPDC) { a.info_tf = nullptr; a.pivot_tau = 1.0; }
  a.grid_hop = grid_hop; a.grid_first = grid_first; a.grid_nwin = grid_nwin; a.grid_T = grid_T;
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
}

// ---- event-locked ensembles: the fused path with the trial-averaged K1 (lagcov_ensemble.hip) ----------------------------
int64_t hmv_sliding_ensemble_workspace_bytes(int measure, int64_t chunk, int m, int n, int p, int F, int n_bands,
                                             int64_t grid_hop, int64_t grid_nwin) {
  // n_bands = -1: the full ffDTF together with S_out, as hmv_sliding_auto_workspace_bytes
  const bool spectra = (n_bands == -1 && measure == HMV_MEASURE_FFDTF);
  if (n <= p || grid_hop < 0 || grid_nwin < 0) return -1;
  // (ens_q_tiles sees chunk, m and p before sliding_bytes range-checks them: it guards every division itself)
  const int64_t q_tiles = ens_q_tiles(chunk, n, p, grid_hop, grid_nwin);
  return sliding_bytes(chunk, m, p, F, spectra ? 0 : n_bands, spectra, measure, q_tiles);
}

namespace {
int sliding_ensemble_entry(const char* who, int measure, const double* x, int64_t rec_stride, int64_t ld, const EnsDesc& ens,
                           const int64_t* item_group, const int64_t* item_offset, int64_t n_items, int m, int n, int p,
                           const double* freqs, int F, double fs, double* out, const int32_t* bin_lo, const int32_t* bin_hi,
                           int n_bands, double* S_out, double* ar_out, double* V_out, int32_t* info_yw, int32_t* info_tf,
                           void* workspace, int64_t workspace_bytes, int64_t chunk, double pivot_tau, int64_t flags,
                           int64_t grid_hop, int64_t grid_nwin, void* stream, void* aux_stream) {
  auto refuse = [&](const char* msg) {
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, msg);
    return fail(-4, buf);
  };
  if (measure < HMV_MEASURE_FFDTF || measure > HMV_MEASURE_GPDC)
    return refuse("measure must be HMV_MEASURE_FFDTF, _DDTF or _GPDC");
  if (n_bands < 0) return refuse("n_bands must be >= 0");
  if (S_out && (measure != HMV_MEASURE_FFDTF || n_bands != 0)) return refuse("spectra come with the full ffDTF only");
  const int mp = pad_of(m);                              // ahead of the pointer checks, in the order of the other entries
  if (mp >= 0 && p >= 1 && p <= HMV_MAX_ORDER && n > p && !out && n_items != 0) return refuse("null pointer / empty grid");
  SlidingArgs a{who};
  a.measure = measure; a.ens = &ens;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = item_group; a.item_start = item_offset; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = out; else a.ffdtf = out;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands; a.S_out = S_out;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  if (measure == HMV_MEASURE_GPDC) { a.info_tf = nullptr; a.pivot_tau = 1.0; }
  a.grid_hop = grid_hop; a.grid_nwin = grid_nwin; a.grid_T = ens.T;
  a.stream = stream; a.aux_stream = aux_stream;
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
  return sliding_ensemble_entry("hmv_sliding_ensemble_f64", measure, x, rec_stride, ld, ens, item_group, item_offset, n_items, m,
                                n, p, freqs, F, fs, out, bin_lo, bin_hi, n_bands, S_out, ar_out, V_out, info_yw, info_tf,
                                workspace, workspace_bytes, chunk, pivot_tau, flags, grid_hop, grid_nwin, stream, aux_stream);
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
  if (pad_of(m) >= 0)                                    // (a bad channel count is sliding_impl's -1)
    if (int rc = ens_split_check("hmv_sliding_ensemble_split_f64", m, trial_rec_b, trial_start_b, split, R_base, item_base))
      return rc;
  EnsDesc ens{trial_rec, trial_start, group_ptr, n_groups, T};
  ens.trial_rec_b = trial_rec_b; ens.trial_start_b = trial_start_b; ens.split = split; ens.R_base = R_base;
  ens.item_base = item_base;
  return sliding_ensemble_entry("hmv_sliding_ensemble_split_f64", measure, x, rec_stride, ld, ens, item_group, item_offset,
                                n_items, m, n, p, freqs, F, fs, out, bin_lo, bin_hi, n_bands, S_out, ar_out, V_out, info_yw,
                                info_tf, workspace, workspace_bytes, chunk, pivot_tau, flags, 0, 0, stream, aux_stream);
}

// ---- pairs of recordings: the fused path with the pair K1 (pseudo-dyad surrogates) -------------------------------------
int64_t hmv_pairs_workspace_bytes(int measure, int64_t chunk, int m, int n, int p, int F, int n_bands) {
  // n_bands = -1: the full ffDTF together with S_out, as hmv_sliding_auto_workspace_bytes
  const bool spectra = (n_bands == -1 && measure == HMV_MEASURE_FFDTF);
  if (n <= p) return -1;
  return sliding_bytes(chunk, m, p, F, spectra ? 0 : n_bands, spectra, measure, 0);
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
  if (pad_of(m) >= 0)                                    // (a bad channel count is sliding_impl's -1)
    if (int rc = pairs_check(who, m, rec_b, split, R_base, base_a, base_b)) return rc;
  if (measure < HMV_MEASURE_FFDTF || measure > HMV_MEASURE_GPDC)
    return fail(-4, "hmv_sliding_pairs_f64: measure must be HMV_MEASURE_FFDTF, _DDTF or _GPDC");
  if (n_bands < 0) return fail(-4, "hmv_sliding_pairs_f64: n_bands must be >= 0");
  if (S_out && (measure != HMV_MEASURE_FFDTF || n_bands != 0))
    return fail(-4, "hmv_sliding_pairs_f64: spectra come with the full ffDTF only");
  if (pad_of(m) >= 0 && p >= 1 && p <= HMV_MAX_ORDER && n > p && !out && n_items != 0)
    return fail(-4, "hmv_sliding_pairs_f64: null pointer / empty grid");
  const PairDesc pairs{rec_b, split, R_base, base_a, base_b};
  SlidingArgs a{who};
  a.measure = measure; a.pairs = &pairs;
  a.x = x; a.rec_stride = rec_stride; a.ld = ld; a.item_rec = rec_a; a.item_start = item_start; a.n_items = n_items;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = out; else a.ffdtf = out;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands; a.S_out = S_out;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  if (measure == HMV_MEASURE_GPDC) { a.info_tf = nullptr; a.pivot_tau = 1.0; }
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
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
  // n_bands = -1: the full ffDTF together with S_out, as hmv_sliding_auto_workspace_bytes
  const bool spectra = (n_bands == -1 && measure == HMV_MEASURE_FFDTF);
  return sliding_bytes(chunk, m, p, F, spectra ? 0 : n_bands, spectra, measure, 0);
}

int hmv_sliding_mix_f64(int measure, const double* Rt, int64_t n_trials, int64_t n_win, const double* W, const double* scale,
                        int64_t n_mix, int m, int n, int p, const double* freqs, int F, double fs, double* out,
                        const int32_t* bin_lo, const int32_t* bin_hi, int n_bands, double* S_out, double* ar_out,
                        double* V_out, int32_t* info_yw, int32_t* info_tf, void* workspace, int64_t workspace_bytes,
                        int64_t chunk, double pivot_tau, int64_t flags, void* stream, void* aux_stream) {
  const char* who = "hmv_sliding_mix_f64";
  if (measure < HMV_MEASURE_FFDTF || measure > HMV_MEASURE_GPDC)
    return fail(-4, "hmv_sliding_mix_f64: measure must be HMV_MEASURE_FFDTF, _DDTF or _GPDC");
  if (n_bands < 0) return fail(-4, "hmv_sliding_mix_f64: n_bands must be >= 0");
  if (S_out && (measure != HMV_MEASURE_FFDTF || n_bands != 0))
    return fail(-4, "hmv_sliding_mix_f64: spectra come with the full ffDTF only");
  const bool sizes_ok = n_trials >= 1 && n_win >= 1 && n_mix >= 1;
  if (pad_of(m) >= 0 && p >= 1 && p <= HMV_MAX_ORDER && n > p && sizes_ok && !out)
    return fail(-4, "hmv_sliding_mix_f64: null pointer / empty grid");
  const MixDesc mix{Rt, W, scale, n_trials, n_win, n_mix};
  SlidingArgs a{who};
  a.measure = measure; a.mix = &mix;
  a.n_items = sizes_ok ? n_mix * n_win : 0;
  a.m = m; a.n = n; a.p = p; a.freqs = freqs; a.F = F; a.fs = fs;
  if (n_bands > 0) a.band_out = out; else a.ffdtf = out;
  a.bin_lo = bin_lo; a.bin_hi = bin_hi; a.n_bands = n_bands; a.S_out = S_out;
  a.ar_out = ar_out; a.V_out = V_out; a.info_yw = info_yw; a.info_tf = info_tf;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.chunk = chunk; a.pivot_tau = pivot_tau; a.flags = flags;
  if (measure == HMV_MEASURE_GPDC) { a.info_tf = nullptr; a.pivot_tau = 1.0; }
  a.stream = stream; a.aux_stream = aux_stream;
  return sliding_impl(a);
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

}  // extern "C"
