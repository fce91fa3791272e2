// Anti-aliased integer-factor FIR decimation of recordings (hmv_decimate_fir_f64).
//
//   y[r][c][k] = sum_{j=0}^{n_taps-1} h[j] * x[r][c][k*q + H - j],   H = (n_taps - 1) / 2,   k = 0 .. ceil(T/q) - 1,
// samples outside [0, T) counting as zero: scipy.signal.decimate(ftype='fir', zero_phase=True) and
// scipy.signal.resample_poly(x, 1, q) with their own taps.
//
//   decimate_kernel<R>   one workgroup of 256 lanes per tile of 256 R consecutive outputs of one row.
//     1. the n_taps taps and the (TILE - 1) q + 2H + 1 input samples the tile reads are staged in LDS, the samples with
//        coalesced 8-byte loads (lane t takes tile samples t, t + 256, ...), zero outside the recording;
//     2. lane t produces outputs t, t + 256, .., t + 256 (R - 1) of the tile, each as ONE chain of FMAs over the taps in
//        ascending j, starting from +0.0: the bits of an output depend on its n_taps (tap, sample) pairs alone -- not on
//        R, the tile, the row or the batch.  A tap read is shared by the lane's R chains.
//   LDS layout: POLYPHASE.  Tile sample u (u = 0 is input sample k0 q - H) lives at [u mod q][u div q], rows of L
//     doubles.  Output k of the tile reads, for tap j, u = k q + e with e = 2H - j: row e mod q (wave-uniform), column
//     k + e div q -- the 32 lanes that one ds_read_b64 pass serves read 32 neighbouring doubles, all 64 banks once.  In
//     the plain layout they would read at a stride of q doubles and collide gcd(q, 32) ways: 2-way at q = 2, 4-way at the
//     q = 4 this exists for, 32-way at q = 32.  The price is paid once per sample on the write side, where neighbouring
//     lanes scatter over the q rows; L is made odd so that those rows start on different banks.
// No atomics, no workspace, no hand-off between workgroups.
#include "../../include/hypermvar.h"
#include "hmv_common.h"
#include "hmv_kernels.h"

namespace hmv {

namespace {
constexpr int DEC_THREADS = 256;
constexpr int DEC_STAGE = 8;
constexpr int DEC_LDS_BYTES = 80 * 1024;       // two workgroups per CU at the largest shape (q = 32, 641 taps: 76 KB)

// row length of the polyphase image for a tile of `tile` outputs, odd
__host__ __device__ inline int dec_row_len(int tile, int q, int n_taps) {
  const long long count = (long long)(tile - 1) * q + n_taps;        // (tile - 1) q + 2H + 1
  return (int)((count + q - 1) / q) | 1;
}
inline size_t dec_lds_bytes(int tile, int q, int n_taps) {
  return sizeof(double) * ((size_t)q * dec_row_len(tile, q, n_taps) + n_taps);
}
}  // namespace

// outputs per workgroup: the largest of 1024 / 512 / 256 whose image fits DEC_LDS_BYTES
int decimate_tile(int q, int n_taps) {
  for (int r = 4; r > 1; r >>= 1)
    if (dec_lds_bytes(DEC_THREADS * r, q, n_taps) <= (size_t)DEC_LDS_BYTES) return DEC_THREADS * r;
  return DEC_THREADS;
}

// grid: (tiles, rows of this launch); block 256; dynamic LDS dec_lds_bytes(256 R, q, n_taps).
template <int R>
__global__ void __launch_bounds__(DEC_THREADS) decimate_kernel(const double* __restrict__ x, long long rec_stride, long long ld,
                                                               long long T, int m, int q, const double* __restrict__ h,
                                                               int n_taps, double* __restrict__ y, long long y_rec_stride,
                                                               long long y_ld, long long T_out, long long row0) {
  extern __shared__ double lds[];
  constexpr int TILE = DEC_THREADS * R;
  const int t = threadIdx.x;
  const int L = dec_row_len(TILE, q, n_taps);
  double* xs = lds;                                  // [q][L]
  double* hs = lds + (size_t)q * L;                  // [n_taps]
  const long long row = row0 + blockIdx.y;           // rec * m + channel
  const long long rec = row / m;
  const int c = (int)(row - rec * m);
  const double* xr = x + rec * rec_stride + (long long)c * ld;
  double* yr = y + rec * y_rec_stride + (long long)c * y_ld;
  const long long k0 = (long long)blockIdx.x * TILE;
  const int twoH = n_taps - 1;
  const long long s0 = k0 * q - twoH / 2;            // input sample of tile sample u = 0
  const long long k_left = T_out - k0;               // outputs of this tile that exist (>= 1)
  const int n_out = k_left < TILE ? (int)k_left : TILE;
  const int count = (n_out - 1) * q + n_taps;        // tile samples that an existing output reads

  for (int j = t; j < n_taps; j += DEC_THREADS) hs[j] = h[j];
  {
    int ph = t % q, dv = t / q;                      // u = dv q + ph, advanced by 256 per step without a division
    const int dph = DEC_THREADS % q, ddv = DEC_THREADS / q;
    // DEC_STAGE loads in flight per lane before the first of them is written to LDS
    for (int u0 = t; u0 < count; u0 += DEC_THREADS * DEC_STAGE) {
      double v[DEC_STAGE];
#pragma unroll
      for (int i = 0; i < DEC_STAGE; ++i) {
        const int u = u0 + DEC_THREADS * i;
        const long long s = s0 + u;
        v[i] = (u < count && s >= 0 && s < T) ? xr[s] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < DEC_STAGE; ++i) {
        if (u0 + DEC_THREADS * i < count) xs[ph * L + dv] = v[i];
        ph += dph; dv += ddv;
        if (ph >= q) { ph -= q; ++dv; }
      }
    }
  }
  __syncthreads();

  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0;
  // tile samples past `count` are not staged: lanes whose output does not exist read column 0 instead (and store nothing)
  int col[R];
#pragma unroll
  for (int r = 0; r < R; ++r) col[r] = (t + DEC_THREADS * r < n_out) ? t + DEC_THREADS * r : 0;
  int ph = twoH % q, dv = twoH / q;                  // e = 2H - j = dv q + ph, walked downwards (wave-uniform)
  for (int j = 0; j < n_taps; ++j) {
    const double hj = hs[j];
    const double* xrow = xs + ph * L + dv;
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = fma(hj, xrow[col[r]], acc[r]);
    if (ph == 0) { ph = q - 1; --dv; } else { --ph; }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (t + DEC_THREADS * r < n_out) yr[k0 + t + DEC_THREADS * r] = acc[r];
}

template <int R>
static int launch_decimate_r(const DecimateArgs& a, long long T_out, hipStream_t st) {
  constexpr int TILE = DEC_THREADS * R;
  const size_t lds = dec_lds_bytes(TILE, a.q, a.n_taps);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&decimate_kernel<R>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, DEC_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
  }
  const long long tiles = (T_out + TILE - 1) / TILE;
  const long long rows = a.n_rec * a.m;
  for (long long r0 = 0; r0 < rows; r0 += 65535) {
    const long long nr = rows - r0 < 65535 ? rows - r0 : 65535;
    hipLaunchKernelGGL(decimate_kernel<R>, dim3((unsigned)tiles, (unsigned)nr), dim3(DEC_THREADS), lds, st, a.x, a.rec_stride,
                       a.ld, a.T, a.m, a.q, a.h, a.n_taps, a.y, a.y_rec_stride, a.y_ld, T_out, r0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

int launch_decimate(const DecimateArgs& a, hipStream_t st) {
  if (a.n_rec == 0) return 0;
  const long long T_out = (a.T + a.q - 1) / a.q;
  switch (decimate_tile(a.q, a.n_taps) / DEC_THREADS) {
    case 4: return launch_decimate_r<4>(a, T_out, st);
    case 2: return launch_decimate_r<2>(a, T_out, st);
    default: return launch_decimate_r<1>(a, T_out, st);
  }
}

}  // namespace hmv
