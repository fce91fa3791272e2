// Stand-alone driver of the host code (argument checks) of hmv_phase_lag_c128 for the host-sanitized twin of the library:
// `make -C csrc asan-phase-lag` builds it with AddressSanitizer + UBSan against libhypermvar_asan.so and runs it.  Every
// pointer is a fake non-zero address: each call must be refused (or be an empty batch) before any of them is read and
// before anything is launched, so the program needs no GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/hypermvar.h"

static int failures = 0;
static const char* entry = "hmv_phase_lag_c128: ";
static void expect(int got, int want, const char* text, const char* what) {
  const char* err = hmv_last_error();
  if (got != want || (text && (!strstr(err, text) || strncmp(err, entry, strlen(entry)) != 0))) {
    printf("FAIL %s%s: got %d (%s), want %d (%s)\n", entry, what, got, err, want, text ? text : "");
    ++failures;
  }
}

struct Call {
  const double* z = reinterpret_cast<const double*>(0x1000);
  int64_t rec_stride = 8000, ld = 1000, T = 1000, n_rec = 2;
  int m = 8, split = 0;
  const int64_t* item_rec = reinterpret_cast<const int64_t*>(0x1000);
  const int64_t* item_start = reinterpret_cast<const int64_t*>(0x1000);
  int64_t n_items = 5;
  int n = 100;
  double* pli = reinterpret_cast<double*>(0x1000);
  double* wpli = reinterpret_cast<double*>(0x1000);
  double* dwpli = reinterpret_cast<double*>(0x1000);
  int32_t* info = reinterpret_cast<int32_t*>(0x1000);
  int run() const {
    return hmv_phase_lag_c128(z, rec_stride, ld, T, n_rec, m, split, item_rec, item_start, n_items, n, pli, wpli, dwpli, info,
                              nullptr);
  }
};

int main() {
  Call c;
  c = Call(); c.m = 0; expect(c.run(), -1, "channel count", "m = 0");
  c = Call(); c.m = 65; c.rec_stride = 65000; expect(c.run(), -1, "channel count", "m = 65");
  c = Call(); c.n = 0; expect(c.run(), -2, "window length", "n = 0");
  c = Call(); c.n = 1001; expect(c.run(), -2, "window length", "n > T");
  c = Call(); c.T = 0; c.ld = 0; expect(c.run(), -3, "count", "T = 0");
  c = Call(); c.n_rec = -1; expect(c.run(), -3, "count", "n_rec < 0");
  c = Call(); c.n_items = -1; expect(c.run(), -3, "count", "n_items < 0");
  c = Call(); c.n_items = int64_t(1) << 31; expect(c.run(), -10, "items", "2^31 items");
  c = Call(); c.z = nullptr; expect(c.run(), -4, "null pointer", "null z");
  c = Call(); c.item_rec = nullptr; expect(c.run(), -4, "null pointer", "null item_rec");
  c = Call(); c.item_start = nullptr; expect(c.run(), -4, "null pointer", "null item_start");
  c = Call(); c.info = nullptr; expect(c.run(), -4, "null pointer", "null info");
  c = Call(); c.z = reinterpret_cast<const double*>(0x1008); expect(c.run(), -8, "16-byte aligned", "misaligned z");
  c = Call(); c.ld = 999; expect(c.run(), -5, "ld is smaller", "ld < T");
  c = Call(); c.rec_stride = 7999; expect(c.run(), -6, "rec_stride is smaller", "rec_stride < m * ld");
  c = Call(); c.ld = int64_t(1) << 58; c.rec_stride = INT64_MAX; c.m = 64; expect(c.run(), -6, "rec_stride is smaller", "huge ld");
  c = Call(); c.pli = nullptr; c.wpli = nullptr; c.dwpli = nullptr; expect(c.run(), -9, "no output", "no output");
  c = Call(); c.split = -1; expect(c.run(), -11, "split", "split = -1");
  c = Call(); c.split = 8; expect(c.run(), -11, "split", "split = m");
  c = Call(); c.m = 1; c.split = 1; expect(c.run(), -11, "split", "m = 1, split = 1");
  c = Call(); c.n_items = 0; expect(c.run(), 0, nullptr, "empty batch");
  c = Call(); c.n_items = 0; c.z = nullptr; c.item_rec = nullptr; c.item_start = nullptr; c.info = nullptr;
  expect(c.run(), 0, nullptr, "empty batch, null pointers");
  c = Call(); c.n_items = 0; c.split = 7; expect(c.run(), 0, nullptr, "empty batch, split = m - 1");
  c = Call(); c.n_items = 0; c.m = 1; expect(c.run(), 0, nullptr, "empty batch, one channel");
  c = Call(); c.n_items = 0; c.split = 9; expect(c.run(), -11, "split", "empty batch, bad split");
  c = Call(); c.n_items = 0; c.pli = nullptr; c.dwpli = nullptr; expect(c.run(), 0, nullptr, "one output");
  printf(failures ? "asan phase_lag driver: %d failure(s)\n" : "asan phase_lag driver ok\n", failures);
  return failures ? 1 : 0;
}
