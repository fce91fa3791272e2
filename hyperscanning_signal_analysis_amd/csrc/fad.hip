// FAD (frequency-amplitude-damping) decomposition of univariate AR models, batched over series.
//
// Replaces fad_decomposition (/root/reference/src/mtmvar.py:607-757): order selection as mvar_criterion at m = 1
// (:551-601), the fit of ar_coeff / count_corr (:35-123), and the partial-fraction expansion of
// scipy.signal.residuez([1], [1, -a_1, .., -a_p]) with its default grouping (tol = 1e-3, rtype 'avg').
//
// Two kernels, one 64-lane workgroup (= one wave) per series, every intermediate in LDS or in registers with
// compile-time indices (no scratch):
//   fad_fit_kernel        stage A: r_0..r_P, biased (1/n), not demeaned -- lane l sums the products of samples
//                         t = l (mod 64) through a 96-sample LDS window, one xor-butterfly per lag (the same
//                         association in every lane, so all lanes hold the same bits);
//                         stage B: Levinson-Durbin to P (lane j holds a_j), V_k = r_0 - a^(k) . r_{1..k} at every
//                         order, criterion curve, first arg-min, coefficients of the chosen order from an LDS history.
//   fad_decompose_kernel  stage C: roots of z^p - a_1 z^(p-1) - .. - a_p by Aberth-Ehrlich iteration (lane j owns
//                         root j, simultaneous updates), then real-root snapping and conjugate symmetrisation
//                         (a root is real when its own mirror image is nearer than every other root's; a mutual
//                         nearest-mirror pair becomes an exact conjugate pair);
//                         stage D: grouping within tol (connected components; bit 2 when a component is wider than
//                         tol), sort by |z| (+Im first on ties), residues, FAD parameters, paired index list.
#include "hmv_common.h"
#include "hmv_kernels.h"

namespace hmv {

constexpr int FAD_P = 32;              // HMV_MAX_ORDER
constexpr int FAD_MAXIT = 500;         // Aberth sweeps before a series is reported as not converged (info bit 1)
constexpr double FAD_GROUP_TOL = 1e-3; // residuez's default tol
constexpr double FAD_EPS = 2.220446049250313e-16;

__device__ __forceinline__ double wave_sum(double v) {
  const int l = lane_id();
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += shfl_f64(v, l ^ m);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  const int l = lane_id();
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmax(v, shfl_f64(v, l ^ m));
  return v;
}

struct cplx { double re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cplx cdiv(cplx a, cplx b) {     // Smith's algorithm (no overflow for moderate operands)
  if (fabs(b.re) >= fabs(b.im)) {
    const double r = b.im / b.re, d = b.re + b.im * r;
    return {(a.re + a.im * r) / d, (a.im - a.re * r) / d};
  }
  const double r = b.re / b.im, d = b.im + b.re * r;
  return {(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}

// ---- stages A + B -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) fad_fit_kernel(FadArgs a) {
  __shared__ double xs[64 + FAD_P];
  __shared__ double rs[FAD_P + 1];
  __shared__ double hist[FAD_P * FAD_P];   // a^(k)_j at [k-1][j-1]
  __shared__ double Vh[FAD_P + 1], cr[FAD_P];
  const int l = lane_id();
  const long long s = blockIdx.x;
  const long long item = s / a.m;
  const int ch = (int)(s - item * a.m);
  const double* x = a.x + a.item_rec[item] * a.rec_stride + (long long)ch * a.ld + a.item_start[item];
  const int n = a.n;
  const int K = a.order > 0 ? a.order : a.pmax;   // Levinson depth

  double acc[FAD_P + 1];
#pragma unroll
  for (int k = 0; k <= FAD_P; ++k) acc[k] = 0.0;
  for (int t0 = 0; t0 < n; t0 += 64) {
    const double v0 = t0 + l < n ? x[t0 + l] : 0.0;
    const double v1 = (l < FAD_P && t0 + 64 + l < n) ? x[t0 + 64 + l] : 0.0;
    __syncthreads();
    xs[l] = v0;
    if (l < FAD_P) xs[64 + l] = v1;
    __syncthreads();
    const double xv = xs[l];
    static_for<FAD_P + 1>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      if (k <= K) acc[k] = __builtin_fma(xv, xs[l + k], acc[k]);
    });
  }
  const double inv_n = 1.0 / (double)n;            // count_corr's corr_scale = 1 / n, multiplied
  static_for<FAD_P + 1>([&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    if (k <= K) {
      const double v = wave_sum(acc[k]);
      if (l == 0) rs[k] = v * inv_n;
    }
  });
  __syncthreads();

  // Levinson-Durbin on the symmetric Toeplitz system of ar_coeff at m = 1; lane j (1..k) holds a_j
  const double r0 = rs[0];
  const double cc = a.crit == 0 ? 2.0 : (a.crit == 1 ? 2.0 * log(log((double)n)) : log((double)n));
  bool bad = !(r0 > 0.0) || !isfinite(r0);
  double aj = 0.0, V = r0;
  const int lr = l < FAD_P ? l : FAD_P;
  for (int k = 1; k <= K && !bad; ++k) {
    const bool old = l >= 1 && l < k;
    const double sacc = wave_sum(old ? aj * rs[old ? k - l : 0] : 0.0);
    const double kk = (rs[k] - sacc) / V;
    const double amir = shfl_f64(aj, old ? k - l : l);
    aj = old ? __builtin_fma(-kk, amir, aj) : (l == k ? kk : aj);
    const bool cur = l >= 1 && l <= k;
    V = r0 - wave_sum(cur ? aj * rs[lr] : 0.0);
    if (cur) hist[(k - 1) * FAD_P + l - 1] = aj;
    if (l == 0) {
      Vh[k] = V;
      cr[k - 1] = log(V) + cc * k / n;            // log det V_k + c p m^2 / n  (mvar_criterion at m = 1)
    }
    if (!(V > 0.0) || !isfinite(V) || !isfinite(kk)) bad = true;   // V is the same in every lane: uniform
  }
  __syncthreads();
  int p = a.order;
  if (!bad && p == 0) {                             // first arg-min of the criterion curve
    double best = cr[0];
    p = 1;
    for (int k = 2; k <= a.pmax; ++k)
      if (cr[k - 1] < best) { best = cr[k - 1]; p = k; }
  }
  const double nan = __builtin_nan("");
  const long long so = s * a.pmax;
  if (l < a.pmax) {
    const double h = hist[(p > 0 ? p - 1 : 0) * FAD_P + l];
    a.ar[so + l] = (!bad && l < p) ? h : nan;
    if (a.crit_out) a.crit_out[so + l] = (!bad && a.order == 0) ? cr[l] : nan;
  }
  if (l == 0) {
    a.noise[s] = bad ? nan : Vh[p > 0 ? p : 0];
    a.order_out[s] = bad && a.order == 0 ? 0 : p;
    a.info[s] = bad ? 1 : 0;
  }
}

// ---- stages C + D -----------------------------------------------------------------------------------------
__device__ __forceinline__ void fad_write_nan(const FadArgs& a, long long s, int l) {
  const double nan = __builtin_nan("");
  const long long q = s * a.pmax + l;
  if (l < a.pmax) {
    a.poles[2 * q] = nan; a.poles[2 * q + 1] = nan;
    a.C[2 * q] = nan; a.C[2 * q + 1] = nan;
    a.alpha[2 * q] = nan; a.alpha[2 * q + 1] = nan;
    a.freq[q] = nan; a.beta[q] = nan; a.bw[q] = nan; a.phi[q] = nan; a.B[q] = nan;
    a.osc[q] = 0;
    a.paired[q] = -1;
  }
  if (l == 0) a.n_paired[s] = 0;
}

__global__ void __launch_bounds__(64) fad_decompose_kernel(FadArgs a) {
  __shared__ double cf[FAD_P + 1];                 // monic polynomial: cf[k] multiplies z^(p-k); cf[0] = 1
  __shared__ double zr[FAD_P], zi[FAD_P];          // current roots
  __shared__ int lab[FAD_P], part[FAD_P], mul[FAD_P];
  __shared__ double ur[FAD_P], ui[FAD_P];          // grouped poles, expanded and sorted (residuez's order)
  __shared__ double gr[FAD_P], gi[FAD_P];          // series scratch of repeated poles
  __shared__ double Cr[FAD_P], Ci[FAD_P];          // residues, same order as ur / ui
  __shared__ double fq[FAD_P];
  __shared__ int sel[FAD_P];
  const int l = lane_id();
  const long long s = blockIdx.x;
  const int P = a.pmax;
  int info = 0, p = P;
  if (a.from_fit) {
    info = uni(a.info[s]);
    p = uni(a.order_out[s]);
  }
  if ((info & 1) || p < 1) {                        // fit breakdown: nothing to decompose
    fad_write_nan(a, s, l);
    return;
  }
  const double av = l < p ? a.ar[s * P + l] : 0.0;
  if (l < p) cf[l + 1] = -av;
  if (l == 0) cf[0] = 1.0;
  const bool finite_in = __all(isfinite(av));
  __syncthreads();

  // ---- stage C: Aberth-Ehrlich ---------------------------------------------------------------------------
  const double rho0 = wave_max(l < p ? pow(fabs(av), 1.0 / (l + 1)) : 0.0);   // max_k |c_k|^(1/k)
  const double rho = rho0 > 0.0 ? rho0 : 1.0;
  const double th = 6.283185307179586 * l / p + 0.4;
  cplx z = {rho * cos(th), rho * sin(th)};
  bool done = l >= p || !finite_in;
  int it = 0;
  for (; it < FAD_MAXIT; ++it) {
    if (l < FAD_P) { zr[l] = z.re; zi[l] = z.im; }
    __syncthreads();
    if (!done) {
      cplx pv = {1.0, 0.0}, dv = {0.0, 0.0};
      const double az = sqrt(z.re * z.re + z.im * z.im);
      double eb = 1.0;
      for (int k = 1; k <= p; ++k) {
        dv = cmul(dv, z); dv.re += pv.re; dv.im += pv.im;
        pv = cmul(pv, z); pv.re += cf[k];
        eb = eb * az + fabs(cf[k]);
      }
      if (sqrt(pv.re * pv.re + pv.im * pv.im) <= 4.0 * (p + 1) * FAD_EPS * eb) {
        done = true;                                // |p(z)| at the rounding level of its evaluation
      } else {
        const cplx N = cdiv(pv, dv);
        cplx S = {0.0, 0.0};
        for (int k = 0; k < p; ++k) {
          if (k == l) continue;
          const cplx d = {z.re - zr[k], z.im - zi[k]};
          const double dd = d.re * d.re + d.im * d.im;
          S.re += d.re / dd; S.im -= d.im / dd;
        }
        const cplx NS = cmul(N, S);
        const cplx w = cdiv(N, {1.0 - NS.re, -NS.im});
        z = csub(z, w);
        if (!(sqrt(w.re * w.re + w.im * w.im) > 4.0 * FAD_EPS * sqrt(z.re * z.re + z.im * z.im))) done = true;
      }
    }
    __syncthreads();
    if (__all(done)) break;
  }
  if (l < FAD_P) { zr[l] = z.re; zi[l] = z.im; }
  __syncthreads();
  bool fail = it >= FAD_MAXIT || !finite_in || !__all(l >= p || (isfinite(z.re) && isfinite(z.im)));

  // real / conjugate-pair structure: nearest mirror image
  if (l < p) {
    double dmin = __builtin_inf();
    int kmin = -1;
    for (int k = 0; k < p; ++k) {
      if (k == l) continue;
      const double d = hypot(zr[k] - z.re, zi[k] + z.im);
      if (d < dmin) { dmin = d; kmin = k; }
    }
    part[l] = 2.0 * fabs(z.im) <= dmin ? -1 : kmin;
  }
  __syncthreads();
  if (l < p) {
    int pk = part[l];
    if (pk >= 0 && part[pk] != l) pk = -1;
    if (pk < 0) {                                   // real root: one real Newton step if it reduces |p|
      const double x0 = z.re;
      double pv = 1.0, dv = 0.0;
      for (int k = 1; k <= p; ++k) { dv = dv * x0 + pv; pv = pv * x0 + cf[k]; }
      const double x1 = x0 - pv / dv;
      double pv1 = 1.0;
      for (int k = 1; k <= p; ++k) pv1 = pv1 * x1 + cf[k];
      z = {(isfinite(x1) && fabs(pv1) < fabs(pv)) ? x1 : x0, 0.0};
    } else {
      const bool upper = zi[l] > zi[pk] || (zi[l] == zi[pk] && l < pk);
      const int iu = upper ? l : pk, iw = upper ? pk : l;
      const double re = (zr[l] + zr[pk]) * 0.5;
      const double im = (zi[iu] - zi[iw]) * 0.5;
      z = {re, upper ? im : -im};
    }
  }
  __syncthreads();
  if (l < FAD_P) { zr[l] = z.re; zi[l] = z.im; }
  __syncthreads();

  // ---- stage D: grouping (residuez: unique_roots(tol = 1e-3, rtype = 'avg')) -------------------------------
  unsigned adj = 0;
  if (l < p)
    for (int k = 0; k < p; ++k)
      if (hypot(zr[k] - z.re, zi[k] - z.im) <= FAD_GROUP_TOL) adj |= 1u << k;
  int L = l;
  for (;;) {                                        // connected components: smallest index of the component
    if (l < FAD_P) lab[l] = L;
    __syncthreads();
    int Ln = L;
    for (unsigned b = adj; b; b &= b - 1) Ln = min(Ln, lab[__builtin_ctz(b)]);
    __syncthreads();
    const bool ch = Ln != L;
    L = Ln;
    if (!__any(ch)) break;
  }
  if (l < FAD_P) lab[l] = L;
  __syncthreads();
  int mult = 0;
  bool wide = false;
  cplx u = {0.0, 0.0};
  const bool leader = l < p && L == l;
  if (leader) {
    for (int k = 0; k < p; ++k)
      if (lab[k] == l) {
        ++mult;
        u.re += zr[k]; u.im += zi[k];
        for (int q = 0; q < p; ++q)
          if (lab[q] == l && hypot(zr[k] - zr[q], zi[k] - zi[q]) > FAD_GROUP_TOL) wide = true;
      }
    const double inv = 1.0 / mult;
    u = {u.re * inv, u.im * inv};
    mul[l] = mult;
    ur[l] = u.re; ui[l] = u.im;
  } else if (l < FAD_P) {
    mul[l] = 0;
  }
  if (__any(wide)) info |= 4;
  __syncthreads();
  // sort the unique poles by |z| (+Im first on ties, then index), expand by multiplicity
  int start = 0;
  const double mag = hypot(u.re, u.im);
  if (leader) {
    for (int k = 0; k < p; ++k) {
      if (mul[k] == 0 || k == l) continue;
      const double mk = hypot(ur[k], ui[k]);
      if (mk < mag || (mk == mag && (ui[k] > u.im || (ui[k] == u.im && k < l)))) start += mul[k];
    }
  }
  __syncthreads();
  // residues: simple pole C = prod_{k != j} (u_j / (u_j - u_k))^{m_k};  repeated pole of multiplicity m: the
  // coefficients g_0..g_{m-1} of prod_k (alpha_k + beta_k s)^{-m_k} in s = 1 - u z^-1 (alpha_k = 1 - u_k / u,
  // beta_k = u_k / u) give the terms r_i / (1 - u z^-1)^i with r_i = g_{m-i}, i = 1..m, ascending in power
  if (leader) {
    if (mult == 1) {
      cplx c = {1.0, 0.0};
      for (int k = 0; k < p; ++k) {
        if (mul[k] == 0 || k == l) continue;
        const cplx f = cdiv(u, {u.re - ur[k], u.im - ui[k]});
        for (int r = 0; r < mul[k]; ++r) c = cmul(c, f);
      }
      Cr[start] = c.re; Ci[start] = c.im;
    } else {
      for (int q = 0; q < mult; ++q) { gr[start + q] = q == 0 ? 1.0 : 0.0; gi[start + q] = 0.0; }
      for (int k = 0; k < p; ++k) {
        if (mul[k] == 0 || k == l) continue;
        const cplx be = cdiv({ur[k], ui[k]}, u);
        const cplx al = {1.0 - be.re, -be.im};
        for (int r = 0; r < mul[k]; ++r) {
          cplx prev = {0.0, 0.0};
          for (int q = 0; q < mult; ++q) {
            const cplx bp = cmul(be, prev);
            prev = cdiv({gr[start + q] - bp.re, gi[start + q] - bp.im}, al);
            gr[start + q] = prev.re; gi[start + q] = prev.im;
          }
        }
      }
      for (int i = 1; i <= mult; ++i) { Cr[start + i - 1] = gr[start + mult - i]; Ci[start + i - 1] = gi[start + mult - i]; }
    }
  }
  __syncthreads();
  if (leader)
    for (int q = 0; q < mult; ++q) { ur[start + q] = u.re; ui[start + q] = u.im; }
  // (a leader's own slot l is read only by itself above; the expanded writes go after the barrier)
  __syncthreads();

  if (fail) {
    fad_write_nan(a, s, l);
    if (l == 0) a.info[s] = info | 2;
    return;
  }
  // ---- FAD parameters of every (expanded) pole ----------------------------------------------------------------
  const double fs_eff = 1.0 / (1.0 / a.fs);        // alpha = log(z) / dt with dt = 1 / fs
  const double twopi = 6.283185307179586;
  const long long q = s * P + l;
  bool pick = false;
  double fhz = 0.0;
  if (l < p) {
    const double pr = ur[l], pi = ui[l], cre = Cr[l], cim = Ci[l];
    const double are = log(hypot(pr, pi)) * fs_eff, aim = atan2(pi, pr) * fs_eff;
    fhz = aim / twopi;
    a.poles[2 * q] = pr; a.poles[2 * q + 1] = pi;
    a.C[2 * q] = cre; a.C[2 * q + 1] = cim;
    a.alpha[2 * q] = are; a.alpha[2 * q + 1] = aim;
    a.freq[q] = fhz;
    a.beta[q] = -are;
    a.bw[q] = -are / twopi;
    a.phi[q] = atan2(cim, cre);
    a.B[q] = 2.0 * hypot(cre, cim);
    a.osc[q] = fabs(pi) > a.imag_tol;
    pick = a.pair_conjugates ? pi > a.imag_tol : fabs(pi) > a.imag_tol;
  } else if (l < P) {
    const double nan = __builtin_nan("");
    a.poles[2 * q] = nan; a.poles[2 * q + 1] = nan;
    a.C[2 * q] = nan; a.C[2 * q + 1] = nan;
    a.alpha[2 * q] = nan; a.alpha[2 * q + 1] = nan;
    a.freq[q] = nan; a.beta[q] = nan; a.bw[q] = nan; a.phi[q] = nan; a.B[q] = nan;
    a.osc[q] = 0;
  }
  if (l < FAD_P) { sel[l] = pick; fq[l] = fhz; }
  __syncthreads();
  // paired components: the +Im poles sorted by frequency (pair_conjugates), else every oscillatory pole in order
  const int cnt = __popcll(__ballot(pick));
  if (pick) {
    int r = 0;
    for (int k = 0; k < p; ++k)
      if (sel[k] && k != l && (a.pair_conjugates ? (fq[k] < fhz || (fq[k] == fhz && k < l)) : k < l)) ++r;
    a.paired[s * P + r] = l;
  }
  if (l >= cnt && l < P) a.paired[s * P + l] = -1;
  if (l == 0) {
    a.n_paired[s] = cnt;
    a.info[s] = info;
  }
}

int launch_fad(const FadArgs& a, hipStream_t st) {
  if (a.n_series == 0) return 0;
  if (a.pmax < 1 || a.pmax > FAD_P) return -2;
  if (a.from_fit) {
    hipLaunchKernelGGL(fad_fit_kernel, dim3((unsigned)a.n_series), dim3(64), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(fad_decompose_kernel, dim3((unsigned)a.n_series), dim3(64), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace hmv
