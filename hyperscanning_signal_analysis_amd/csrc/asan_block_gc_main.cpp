// Stand-alone driver of the block Granger entries' host code (argument checks, workspace layout) for the host-sanitized
// twin of the library: `make -C csrc asan-block-gc` builds it with AddressSanitizer + UBSan against libhypermvar_asan.so
// and runs it.  Every pointer is a fake non-zero address: each call must be refused (or be an empty batch) before any of
// them is read and before anything is launched, so the program needs no GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/hypermvar.h"

static int failures = 0;
static void expect(int got, int want, const char* text, const char* what) {
  const char* err = hmv_last_error();
  if (got != want || (text && !strstr(err, text))) {
    printf("FAIL %s: got %d (%s), want %d (%s)\n", what, got, err, want, text ? text : "");
    ++failures;
  }
}

int main() {
  double* P = reinterpret_cast<double*>(0x1000);
  int64_t* I = reinterpret_cast<int64_t*>(0x1000);
  int32_t* J = reinterpret_cast<int32_t*>(0x1000);
  void* W = reinterpret_cast<void*>(0x1000);
  const int64_t big = int64_t(1) << 40;
  auto sliding = [&](int m, int n, int p, int split, int F, int n_bands, double* spectral, int64_t ws, int64_t chunk,
                     int64_t n_items) {
    return hmv_sliding_block_gc_f64(P, 0, 100, I, I, n_items, m, n, p, split, P, F, 100.0, spectral, J, J, n_bands, P, nullptr,
                                    nullptr, J, J, J, W, ws, chunk, 0, 0, 0, 0, 100, nullptr);
  };
  const int64_t need = hmv_block_gc_sliding_workspace_bytes(4, 8, 4, 3, 16, 0);
  if (need <= 0) { printf("FAIL workspace size %lld\n", (long long)need); ++failures; }
  expect(sliding(8, 100, 4, 0, 16, 0, P, big, 4, 1), -11, "split", "split = 0");
  expect(sliding(8, 100, 4, 8, 16, 0, P, big, 4, 1), -11, "split", "split = m");
  expect(sliding(65, 100, 4, 3, 16, 0, P, big, 4, 1), -1, "channel count", "m = 65");
  expect(sliding(8, 100, 0, 3, 16, 0, P, big, 4, 1), -2, "model order", "p = 0");
  expect(sliding(8, 100, 33, 3, 16, 0, P, big, 4, 1), -2, "model order", "p = 33");
  expect(sliding(8, 4, 4, 3, 16, 0, P, big, 4, 1), -3, "window shorter", "n <= p");
  expect(sliding(8, 100, 4, 3, 0, 0, P, big, 4, 1), -12, "frequency grid", "F = 0");
  expect(sliding(8, 100, 4, 3, 16, -1, P, big, 4, 1), -14, "n_bands", "n_bands < 0");
  expect(sliding(8, 100, 4, 3, 16, 0, nullptr, big, 4, 1), -13, "spectral output", "null output");
  expect(sliding(8, 100, 4, 3, 16, 0, P, need - 1, 4, 1), -7, "workspace too small", "workspace one byte short");
  expect(sliding(8, 100, 4, 3, 16, 0, P, big, 0, 1), -4, "null pointer", "chunk = 0");
  expect(sliding(8, 100, 4, 3, 16, 0, nullptr, 0, 4, 0), 0, nullptr, "empty batch");
  expect(sliding(8, 100, 4, 3, 16, 0, P, big, 4, -1), -4, "n_items", "n_items < 0");
  for (int m = 2; m <= 64; ++m)                                   // every layout the workspace function can be asked for
    for (int split = 1; split < m; split += (m > 8 ? 7 : 1))
      for (int nb = 0; nb <= 5; nb += 5)
        if (hmv_block_gc_sliding_workspace_bytes(3, m, 8, split, 32, nb) <= hmv_block_gc_sliding_workspace_bytes(2, m, 8, split, 32, nb)) {
          printf("FAIL workspace not monotone at m=%d split=%d\n", m, split);
          ++failures;
        }
  const int64_t need_s = hmv_block_gc_workspace_bytes(1, 8, 4, 3, 16);
  auto stage = [&](int m, int p, int split, int F, double* spectral, int64_t ws, int64_t n_items) {
    return hmv_block_gc_f64(P, P, n_items, m, p, split, P, F, 100.0, spectral, J, J, W, ws, nullptr);
  };
  expect(stage(8, 4, 0, 16, P, big, 1), -11, "split", "stage split = 0");
  expect(stage(65, 4, 3, 16, P, big, 1), -1, "channel count", "stage m = 65");
  expect(stage(8, 33, 3, 16, P, big, 1), -2, "model order", "stage p = 33");
  expect(stage(8, 4, 3, 0, P, big, 1), -12, "frequency grid", "stage F = 0");
  expect(stage(8, 4, 3, 16, nullptr, big, 1), -13, "spectral output", "stage null output");
  expect(stage(8, 4, 3, 16, P, need_s - 1, 1), -7, "workspace too small", "stage workspace one byte short");
  expect(stage(8, 4, 3, 16, nullptr, 0, 0), 0, nullptr, "stage empty batch");
  expect(stage(8, 4, 3, 16, P, big, -1), -4, "n_items", "stage n_items < 0");
  if (hmv_block_gc_workspace_bytes(1, 8, 4, 8, 16) != -1 || hmv_block_gc_sliding_workspace_bytes(1, 8, 4, 0, 16, 0) != -1) {
    printf("FAIL bad sizes accepted\n");
    ++failures;
  }
  printf(failures ? "asan block_gc driver: %d failure(s)\n" : "asan block_gc driver ok\n", failures);
  return failures ? 1 : 0;
}
