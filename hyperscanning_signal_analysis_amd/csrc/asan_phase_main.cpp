// Stand-alone driver of the host code (argument checks) of hmv_phase_sync_c128, hmv_phase_sync_pairs_c128 and
// hmv_phase_lag_c128 for the host-sanitized twin of the library: `make -C csrc asan-phase` builds it with AddressSanitizer +
// UBSan against libhypermvar_asan.so and runs it.  Every pointer is a fake non-zero address: each call must be refused (or be
// an empty batch) before any of them is read and before anything is launched, so the program needs no GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/hypermvar.h"

enum : unsigned { SYNC = 1, PAIRS = 2, LAG = 4, ALL = 7 };
static const char* const names[] = {"hmv_phase_sync_c128: ", "hmv_phase_sync_pairs_c128: ", "hmv_phase_lag_c128: "};

template <class T> static T* fake() { return reinterpret_cast<T*>(0x1000); }

// A good call of every entry: the arguments the three share, then each entry's own.
struct Call {
  const double* z = fake<const double>();
  int64_t rec_stride = 8000, ld = 1000, T = 1000, n_rec = 2;
  int m = 8;
  const int64_t* item_rec = fake<const int64_t>();                      // sync, lag
  const int64_t* item_start = fake<const int64_t>();
  int64_t n_items = 5;
  int n = 100, mode = HMV_PHASE_UNIT;                                   // mode: sync, pairs
  int32_t* info = fake<int32_t>();
  double *coherency = fake<double>(), *mag = fake<double>(), *lagged = fake<double>();          // sync
  int pairs_split = 4, val_stride = 4, col_mag = 0, col_lagged = 1;                             // pairs
  const int64_t *rec_a = fake<const int64_t>(), *rec_b = fake<const int64_t>(), *shift_b = fake<const int64_t>();
  double* values = fake<double>();
  int lag_split = 0;                                                                            // lag
  double *pli = fake<double>(), *wpli = fake<double>(), *dwpli = fake<double>();
  int run(unsigned entry) const {
    if (entry == SYNC)
      return hmv_phase_sync_c128(z, rec_stride, ld, T, n_rec, m, item_rec, item_start, n_items, n, mode, coherency, mag, lagged,
                                 info, nullptr);
    if (entry == PAIRS)
      return hmv_phase_sync_pairs_c128(z, rec_stride, ld, T, n_rec, m, pairs_split, rec_a, rec_b, item_start, shift_b, n_items, n,
                                       mode, values, val_stride, col_mag, col_lagged, info, nullptr);
    return hmv_phase_lag_c128(z, rec_stride, ld, T, n_rec, m, lag_split, item_rec, item_start, n_items, n, pli, wpli, dwpli, info,
                              nullptr);
  }
};

static void null_inputs(Call& c) {
  c.z = nullptr; c.item_rec = c.item_start = c.rec_a = c.rec_b = c.shift_b = nullptr; c.values = nullptr; c.info = nullptr;
}

struct Case {
  unsigned on;                       // the entries the case is run against
  void (*set)(Call&);
  int want;
  const char* text;                  // part of the refusal's text; null where the call succeeds
  const char* what;
};

static const Case cases[] = {
    // what the three entries share
    {ALL, [](Call& c) { c.m = 0; }, -1, "channel count", "m = 0"},
    {ALL, [](Call& c) { c.m = 65; c.rec_stride = 65000; }, -1, "channel count", "m = 65"},
    {ALL, [](Call& c) { c.n = 0; }, -2, "window length", "n = 0"},
    {ALL, [](Call& c) { c.n = 1001; }, -2, "window length", "n > T"},
    {ALL, [](Call& c) { c.T = 0; c.ld = 0; }, -3, "count", "T = 0"},
    {ALL, [](Call& c) { c.n_rec = -1; }, -3, "count", "n_rec < 0"},
    {ALL, [](Call& c) { c.n_items = -1; }, -3, "count", "n_items < 0"},
    {ALL, [](Call& c) { c.n_items = int64_t(1) << 31; }, -10, "items", "2^31 items"},
    {ALL, [](Call& c) { c.z = nullptr; }, -4, "null pointer", "null z"},
    {ALL, [](Call& c) { c.item_start = nullptr; }, -4, "null pointer", "null item_start"},
    {ALL, [](Call& c) { c.info = nullptr; }, -4, "null pointer", "null info"},
    {ALL, [](Call& c) { c.z = reinterpret_cast<const double*>(0x1008); }, -8, "16-byte aligned", "misaligned z"},
    {ALL, [](Call& c) { c.ld = 999; }, -5, "ld is smaller", "ld < T"},
    {ALL, [](Call& c) { c.rec_stride = 7999; }, -6, "rec_stride is smaller", "rec_stride < m * ld"},
    {ALL, [](Call& c) { c.ld = int64_t(1) << 58; c.rec_stride = INT64_MAX; c.m = 64; c.pairs_split = 32; }, -6,
     "rec_stride is smaller", "huge ld"},
    {ALL, [](Call& c) { c.n_items = 0; }, 0, nullptr, "empty batch"},
    {ALL, [](Call& c) { c.n_items = 0; null_inputs(c); }, 0, nullptr, "empty batch, null pointers"},
    // the item table of the two full forms, the mode of the two synchrony entries
    {SYNC | LAG, [](Call& c) { c.item_rec = nullptr; }, -4, "null pointer", "null item_rec"},
    {SYNC | PAIRS, [](Call& c) { c.mode = 2; }, -7, "mode", "mode = 2"},
    {SYNC | PAIRS, [](Call& c) { c.mode = -1; }, -7, "mode", "mode = -1"},
    // hmv_phase_sync_c128
    {SYNC, [](Call& c) { c.coherency = c.mag = c.lagged = nullptr; }, -9, "no output", "no output"},
    {SYNC, [](Call& c) { c.n_items = 0; c.mode = 3; }, -7, "mode", "empty batch, bad mode"},
    // hmv_phase_sync_pairs_c128
    {PAIRS, [](Call& c) { c.rec_a = nullptr; }, -4, "null pointer", "null rec_a"},
    {PAIRS, [](Call& c) { c.rec_b = nullptr; }, -4, "null pointer", "null rec_b"},
    {PAIRS, [](Call& c) { c.values = nullptr; }, -4, "null pointer", "null values"},
    {PAIRS, [](Call& c) { c.pairs_split = 0; }, -11, "split", "split = 0"},
    {PAIRS, [](Call& c) { c.pairs_split = 8; }, -11, "split", "split = m"},
    {PAIRS, [](Call& c) { c.m = 1; c.pairs_split = 1; }, -11, "split", "m = 1"},
    {PAIRS, [](Call& c) { c.val_stride = 0; }, -12, "val_stride", "val_stride = 0"},
    {PAIRS, [](Call& c) { c.col_mag = 4; }, -12, "val_stride", "col_mag = val_stride"},
    {PAIRS, [](Call& c) { c.col_lagged = -2; }, -12, "val_stride", "col_lagged = -2"},
    {PAIRS, [](Call& c) { c.col_mag = -1; c.col_lagged = -1; }, -12, "val_stride", "no column"},
    {PAIRS, [](Call& c) { c.col_mag = 2; c.col_lagged = 2; }, -12, "val_stride", "equal columns"},
    {PAIRS, [](Call& c) { c.n_items = 0; c.pairs_split = 9; }, -11, "split", "empty batch, bad split"},
    {PAIRS, [](Call& c) { c.n_items = 0; c.col_mag = -1; c.val_stride = 1; c.col_lagged = 0; }, 0, nullptr, "one column"},
    // hmv_phase_lag_c128
    {LAG, [](Call& c) { c.pli = c.wpli = c.dwpli = nullptr; }, -9, "no output", "no output"},
    {LAG, [](Call& c) { c.lag_split = -1; }, -11, "split", "split = -1"},
    {LAG, [](Call& c) { c.lag_split = 8; }, -11, "split", "split = m"},
    {LAG, [](Call& c) { c.m = 1; c.lag_split = 1; }, -11, "split", "m = 1, split = 1"},
    {LAG, [](Call& c) { c.n_items = 0; c.lag_split = 7; }, 0, nullptr, "empty batch, split = m - 1"},
    {LAG, [](Call& c) { c.n_items = 0; c.m = 1; }, 0, nullptr, "empty batch, one channel"},
    {LAG, [](Call& c) { c.n_items = 0; c.lag_split = 9; }, -11, "split", "empty batch, bad split"},
    {LAG, [](Call& c) { c.n_items = 0; c.pli = nullptr; c.dwpli = nullptr; }, 0, nullptr, "one output"},
};

static int failures = 0;
static void expect(const char* entry, int got, int want, const char* text, const char* what) {
  const char* err = hmv_last_error();
  if (got != want || (text && (!strstr(err, text) || strncmp(err, entry, strlen(entry)) != 0))) {
    printf("FAIL %s%s: got %d (%s), want %d (%s)\n", entry, what, got, err, want, text ? text : "");
    ++failures;
  }
}

int main() {
  int ran[3] = {0, 0, 0};
  for (int e = 0; e < 3; ++e)
    for (const Case& k : cases)
      if (k.on & (1u << e)) {
        Call c;
        k.set(c);
        expect(names[e], c.run(1u << e), k.want, k.text, k.what);
        ++ran[e];
      }
  if (failures) printf("asan phase driver: %d failure(s)\n", failures);
  else printf("asan phase driver ok (%d + %d + %d cases)\n", ran[0], ran[1], ran[2]);
  return failures ? 1 : 0;
}
