// Remaining preprocess/signal steps behind the same run(data, params) plugin ABI:
// per-channel z-score (whole recording or a baseline interval), common-average re-reference and
// rolling z-score.  HBM-bound reductions; statistics are accumulated in fp64.
#include "tonal_common.h"

namespace tl {

template <typename T>
__device__ __forceinline__ double ldd(const void* p, long long i) { return (double)reinterpret_cast<const T*>(p)[i]; }

__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int off = blockDim.x / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

// stats[c] = (mean, population std) of x[c][t0:t1]  (numpy: mean, then mean of squared deviations)
template <typename T>
__global__ __launch_bounds__(256) void row_stats_kernel(const void* __restrict__ x, double* __restrict__ stats, long long Tn,
                                                        long long t0, long long t1) {
  __shared__ double red[256];
  const long long base = (long long)blockIdx.x * Tn;
  double s = 0.0;
  for (long long t = t0 + threadIdx.x; t < t1; t += blockDim.x) s += ldd<T>(x, base + t);
  const double mean = block_sum(s, red) / (double)(t1 - t0);
  double q = 0.0;
  for (long long t = t0 + threadIdx.x; t < t1; t += blockDim.x) {
    const double d = ldd<T>(x, base + t) - mean;
    q += d * d;
  }
  const double var = block_sum(q, red) / (double)(t1 - t0);
  if (threadIdx.x == 0) {
    stats[2 * blockIdx.x] = mean;
    stats[2 * blockIdx.x + 1] = sqrt(var);
  }
}

// y[c][t] = (x[c][t] - mean[c]) / std[c]; NaN results -> 0 when zero_nans
template <typename T>
__global__ __launch_bounds__(256) void row_normalise_kernel(const void* __restrict__ x, const double* __restrict__ stats,
                                                            T* __restrict__ y, long long total, long long Tn, int zero_nans) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long c = i / Tn;
    double v = (ldd<T>(x, i) - stats[2 * c]) / stats[2 * c + 1];
    if (zero_nans && v != v) v = 0.0;
    y[i] = (T)v;
  }
}

// y[c][t] = x[c][t] - mean_{c in include} x[c][t]
template <typename T>
__global__ __launch_bounds__(256) void car_kernel(const void* __restrict__ x, const int* __restrict__ include, T* __restrict__ y,
                                                  int C, long long Tn, int n_inc) {
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < Tn; t += (long long)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < C; ++c)
      if (include[c]) s += ldd<T>(x, (long long)c * Tn + t);
    const double m = s / (double)n_inc;
    for (int c = 0; c < C; ++c) y[(long long)c * Tn + t] = (T)(ldd<T>(x, (long long)c * Tn + t) - m);
  }
}

// pandas rolling(window=W, min_periods=1): mean and sample std (ddof=1) over the non-NaN values of
// x[c][max(0,t-W+1) .. t]; z = (x - mean)/std.  Two-pass per output on an LDS-staged window: the block's RZ_TB
// outputs read the RZ_TB + W - 1 samples x[c][t0-W+1 .. t0+RZ_TB-1].  When those exceed one LDS tile (RZ_CHUNK
// samples) they stream through it chunk by chunk, once per pass; each output still adds its window in time order, so
// the result does not depend on whether its window was resident or streamed.
// Like pandas, a window whose non-NaN values are all equal has mean = that value and std 0 exactly, so z = 0/0 = NaN;
// the plain sum leaves s/n an ulp off a non-dyadic constant and would turn a flat stretch into +-sqrt((n-1)/n).  Such a
// window has every deviation equal to x[t] - mean, i.e. q == n (x[t] - mean)^2 up to the rounding of the sum; only
// outputs that meet that test (rare off a flat stretch) scan their window a third time to compare every value with x[t].
constexpr int RZ_TB = 256;
constexpr int RZ_CHUNK = 8192;                                   // 64 KiB of fp64
template <typename T>
__device__ __forceinline__ void rz_stage(const void* __restrict__ x, double* xs, long long row, long long Tn, long long src0,
                                         int len, double nan) {
  for (int j = threadIdx.x; j < len; j += blockDim.x) {
    const long long src = src0 + j;
    xs[j] = (src >= 0 && src < Tn) ? ldd<T>(x, row + src) : nan;
  }
}
// f(v) on window samples in time order.  The trip counts are block-uniform so that the loops stay scalar (and unrolled):
// rz_each walks a resident window p[0 .. W); rz_each_in_chunk walks the part of output i's window that lies in the chunk
// of tile positions [c0, c0 + len) staged in xs, over a window-offset range that covers every lane of the block.
template <typename F>
__device__ __forceinline__ void rz_each(const double* p, int W, F f) {
  for (int k = 0; k < W; ++k) f(p[k]);
}
template <typename F>
__device__ __forceinline__ void rz_each_in_chunk(const double* xs, int i, int c0, int len, int W, F f) {
  const int kb = c0 - (RZ_TB - 1) > 0 ? c0 - (RZ_TB - 1) : 0, ke = c0 + len < W ? c0 + len : W;
  for (int k = kb; k < ke; ++k) {
    const int j = i + k - c0;
    if (j >= 0 && j < len) f(xs[j]);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void rolling_zscore_kernel(const void* __restrict__ x, double* __restrict__ y, long long Tn,
                                                             int W, int zero_nans) {
  extern __shared__ __attribute__((aligned(16))) double xs[];     // [min(RZ_TB + W - 1, RZ_CHUNK)]
  const int c = blockIdx.y;
  const long long row = (long long)c * Tn;
  const long long t0 = (long long)blockIdx.x * RZ_TB;
  const long long src0 = t0 - (W - 1);
  const int win = RZ_TB + W - 1;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int i = threadIdx.x;                                     // window of this output: tile positions [i, i + W)
  const long long t = t0 + i;
  const double xv = t < Tn ? ldd<T>(x, row + t) : nan;
  double s = 0.0, q = 0.0, mean = nan;
  int n = 0;
  bool need, flat = true;
  auto add = [&](double v) {
    if (v == v) {
      s += v;
      ++n;
    }
  };
  auto sq = [&](double v) {
    if (v == v) q += (v - mean) * (v - mean);
  };
  auto same = [&](double v) { flat = flat && !(v == v && v != xv); };
  if (win <= RZ_CHUNK) {                                         // the whole window resident in LDS
    rz_stage<T>(x, xs, row, Tn, src0, win, nan);
    __syncthreads();
    if (t >= Tn) return;
    rz_each(xs + i, W, add);
    mean = s / n;
    need = n >= 2;
    if (need) rz_each(xs + i, W, sq);
    const double d = xv - mean;
    if (need && fabs(q - n * d * d) <= 1e-6 * q)
      rz_each(xs + i, W, same);
    else
      flat = false;
  } else {
    for (int c0 = 0; c0 < win; c0 += RZ_CHUNK) {
      const int len = win - c0 < RZ_CHUNK ? win - c0 : RZ_CHUNK;
      if (c0 > 0) __syncthreads();
      rz_stage<T>(x, xs, row, Tn, src0 + c0, len, nan);
      __syncthreads();
      rz_each_in_chunk(xs, i, c0, len, W, add);
    }
    mean = s / n;
    need = t < Tn && n >= 2;
    const double d = xv - mean;
    for (int pass = 0; pass < 2; ++pass) {                       // q, then (where flagged) the flat test
      const bool act = pass == 0 ? need : (need && fabs(q - n * d * d) <= 1e-6 * q);
      if (pass == 1 && !act) flat = false;
      if (!__syncthreads_or(act)) break;
      for (int c0 = 0; c0 < win; c0 += RZ_CHUNK) {
        const int len = win - c0 < RZ_CHUNK ? win - c0 : RZ_CHUNK;
        __syncthreads();
        rz_stage<T>(x, xs, row, Tn, src0 + c0, len, nan);
        __syncthreads();
        if (!act) continue;
        if (pass == 0)
          rz_each_in_chunk(xs, i, c0, len, W, sq);
        else
          rz_each_in_chunk(xs, i, c0, len, W, same);
      }
    }
    if (t >= Tn) return;
  }
  double out = nan;
  if (need && !flat) out = (xv - mean) / sqrt(q / (n - 1));
  if (zero_nans && out != out) out = 0.0;
  y[row + t] = out;
}

// The same quantity in O(1) per output (tl_rolling_zscore_blocked): the window's count, sum S1 and sum of
// squares S2 - the sums as (hi, lo) pairs, so that n S2 - S1^2 survives its cancellation - plus its minimum and maximum, which
// decide pandas' flat-window rule exactly.  With W >= RZ_TB every window of output tile j (samples t0 .. t0 + 255) is the
// union of three parts, nothing subtracted:
//   (a) the tile's prefix up to the output                             - a forward scan over the tile;
//   (b) the whole tiles k0 .. j-1, k0 = ceil((t0 + 256 - W) / 256)      - rows of the per-tile table rz_tile_moments wrote;
//   (c) the head: the L <= 510 samples from t0 - W + 1 up to tile k0   - output i takes head[i .. L): a backward scan over
//       head[0 .. 256) plus all of head[256 .. L).
// Lane i starts its partial with head[256 + i] and adds the table rows k0 + i, k0 + i + 256, ... in that order; one scan over
// the partials gives the part M every output of the tile shares.  Output i: ((c_i + M) + a_i).  The order of every sum is
// fixed by the lane and wave numbers alone: two runs give the same bits.  Samples before t = 0 or past T and NaN samples
// enter as the identity and are never dereferenced.  tests/rolling_blocked_ref.py restates all of this in NumPy.
struct RzMom {
  int n;
  double s1h, s1l, s2h, s2l, mn, mx;
};
__device__ __forceinline__ void rz_two_sum(double a, double b, double& s, double& e) {   // a + b = s + e exactly
  s = __dadd_rn(a, b);
  const double bv = __dsub_rn(s, a);
  e = __dadd_rn(__dsub_rn(a, __dsub_rn(s, bv)), __dsub_rn(b, bv));
}
__device__ __forceinline__ void rz_fast_two_sum(double a, double b, double& s, double& e) {   // the same for |a| >= |b|
  s = __dadd_rn(a, b);
  e = __dsub_rn(b, __dsub_rn(s, a));
}
__device__ __forceinline__ void rz_dd_add(double ah, double al, double bh, double bl, double& h, double& l) {
  double s, e, t, f, s2, e2;
  rz_two_sum(ah, bh, s, e);
  rz_two_sum(al, bl, t, f);
  rz_fast_two_sum(s, __dadd_rn(e, t), s2, e2);
  rz_fast_two_sum(s2, __dadd_rn(e2, f), h, l);
}
// (a b) + c as a pair: a b exactly by fma, the low-order term c added to its error.  Every product of this route is an
// rz_mul: it rounds on its own whatever contraction the file is compiled with (the additions are __dadd_rn / __dsub_rn).
__device__ __forceinline__ double rz_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ void rz_prod_plus(double a, double b, double c, double& h, double& l) {
  const double p = rz_mul(a, b);
  const double e = __fma_rn(a, b, -p);
  rz_fast_two_sum(p, __dadd_rn(e, c), h, l);
}
__device__ __forceinline__ RzMom rz_identity() {
  return {0, 0.0, 0.0, 0.0, 0.0, __longlong_as_double(0x7ff0000000000000LL), __longlong_as_double(0xfff0000000000000LL)};
}
__device__ __forceinline__ RzMom rz_sample(double v) {
  if (v != v) return rz_identity();
  RzMom m = {1, v, 0.0, 0.0, 0.0, v, v};
  rz_prod_plus(v, v, 0.0, m.s2h, m.s2l);
  return m;
}
template <typename T>
__device__ __forceinline__ RzMom rz_load(const void* __restrict__ x, long long row, long long Tn, long long t) {
  return (t >= 0 && t < Tn) ? rz_sample(ldd<T>(x, row + t)) : rz_identity();
}
__device__ __forceinline__ RzMom rz_combine(const RzMom& a, const RzMom& b) {   // a's samples, then b's
  RzMom r;
  r.n = a.n + b.n;
  rz_dd_add(a.s1h, a.s1l, b.s1h, b.s1l, r.s1h, r.s1l);
  rz_dd_add(a.s2h, a.s2l, b.s2h, b.s2l, r.s2h, r.s2l);
  r.mn = fmin(a.mn, b.mn);
  r.mx = fmax(a.mx, b.mx);
  return r;
}
template <bool REV>
__device__ __forceinline__ RzMom rz_shfl(const RzMom& m, int off) {
  RzMom r;
#define RZ_SH(f) r.f = REV ? __shfl_down(m.f, off) : __shfl_up(m.f, off)
  RZ_SH(n); RZ_SH(s1h); RZ_SH(s1l); RZ_SH(s2h); RZ_SH(s2l); RZ_SH(mn); RZ_SH(mx);
#undef RZ_SH
  return r;
}
__device__ __forceinline__ void rz_put(double* p, const RzMom& m) {
  p[0] = (double)m.n; p[1] = m.s1h; p[2] = m.s1l; p[3] = m.s2h; p[4] = m.s2l; p[5] = m.mn; p[6] = m.mx; p[7] = 0.0;
}
__device__ __forceinline__ RzMom rz_get(const double* p) { return {(int)p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }
// Inclusive scan over the block's 256 lanes in lane order (REV: from lane 255 down): Hillis-Steele inside each 64-lane
// wave, then the totals of the waves before (REV: after) this one, added nearest wave last, go in front.  red: [4][8].
template <bool REV>
__device__ __forceinline__ RzMom rz_block_scan(RzMom m, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const RzMom o = rz_shfl<REV>(m, off);
    if (REV ? lane + off < 64 : lane >= off) m = REV ? rz_combine(m, o) : rz_combine(o, m);
  }
  __syncthreads();                                               // red may still be read from the scan before
  if (lane == (REV ? 0 : 63)) rz_put(red + 8 * wave, m);
  __syncthreads();
  if (REV) {
    if (wave < 3) {
      RzMom p = rz_get(red + 8 * 3);
      for (int w = 2; w > wave; --w) p = rz_combine(rz_get(red + 8 * w), p);
      m = rz_combine(m, p);
    }
  } else if (wave > 0) {
    RzMom p = rz_get(red);
    for (int w = 1; w < wave; ++w) p = rz_combine(p, rz_get(red + 8 * w));
    m = rz_combine(p, m);
  }
  return m;
}

// work[c][j][0..8) = (count, S1 hi, S1 lo, S2 hi, S2 lo, min, max, 0) of tile j of channel c
template <typename T>
__global__ __launch_bounds__(256) void rz_tile_moments(const void* __restrict__ x, double* __restrict__ work, long long Tn) {
  __shared__ double red[32];
  const long long row = (long long)blockIdx.y * Tn;
  const RzMom m = rz_block_scan<false>(rz_load<T>(x, row, Tn, (long long)blockIdx.x * RZ_TB + threadIdx.x), red);
  if (threadIdx.x == RZ_TB - 1) rz_put(work + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 8, m);
}

template <typename T>
__global__ __launch_bounds__(256) void rolling_zscore_blocked_kernel(const void* __restrict__ x, const double* __restrict__ work,
                                                                     double* __restrict__ y, long long Tn, int W, int zero_nans) {
  __shared__ double red[32];
  __shared__ double shared_m[8];
  const long long row = (long long)blockIdx.y * Tn;
  const int j = blockIdx.x, i = threadIdx.x;
  const long long t0 = (long long)j * RZ_TB, t = t0 + i;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double xv = t < Tn ? ldd<T>(x, row + t) : nan;
  const RzMom a = rz_block_scan<false>(rz_sample(xv), red);                        // (a)
  // W >= 256, so k0 <= j; a head that lies before t = 0 altogether is empty
  const long long k0u = (t0 + RZ_TB - W + (RZ_TB - 1)) >> 8;                       // ceil: the numerator is > -2^31
  const int k0 = t0 + RZ_TB - W > 0 ? (int)k0u : 0;
  const long long h0 = t0 - W + 1;
  const int L = t0 + RZ_TB - W > 0 ? (int)((long long)k0 * RZ_TB - h0) : 0;
  RzMom c = rz_block_scan<true>(i < L ? rz_load<T>(x, row, Tn, h0 + i) : rz_identity(), red);   // (c), head[i .. 256)
  RzMom p = RZ_TB + i < L ? rz_load<T>(x, row, Tn, h0 + RZ_TB + i) : rz_identity();
  const double* tab = work + (long long)blockIdx.y * gridDim.x * 8;
  for (int k = k0 + i; k < j; k += RZ_TB) p = rz_combine(p, rz_get(tab + (long long)k * 8));   // (b)
  p = rz_block_scan<false>(p, red);
  if (i == RZ_TB - 1) rz_put(shared_m, p);
  __syncthreads();
  if (t >= Tn) return;
  const RzMom w = rz_combine(rz_combine(c, rz_get(shared_m)), a);
  double out = nan;
  if (xv == xv && w.n >= 2 && w.mn != w.mx) {
    const double n = (double)w.n;
    double ah, al, bh, bl, qh, ql, dh, dl;
    rz_prod_plus(n, w.s2h, rz_mul(n, w.s2l), ah, al);                              // n S2
    rz_prod_plus(w.s1h, w.s1h, rz_mul(2.0, rz_mul(w.s1h, w.s1l)), bh, bl);         // S1^2
    rz_dd_add(ah, al, -bh, -bl, qh, ql);                                           // n q = n S2 - S1^2
    rz_prod_plus(n, xv, 0.0, ah, al);                                              // n x_t
    rz_dd_add(ah, al, -w.s1h, -w.s1l, dh, dl);                                     // n d = n x_t - S1
    out = (__dadd_rn(dh, dl) / n) / sqrt((__dadd_rn(qh, ql) / n) / (double)(w.n - 1));
  }
  if (zero_nans && out != out) out = 0.0;
  y[row + t] = out;
}


// mean and population std (np.std) of the n_seg consecutive segments of L samples from s0 on, per channel
// (utils/diagnostics.py segment_mean_std).  Two-pass: the mean, then the sum of (x - mean)^2 over the same samples - never
// E[x^2] - mean^2, so a DC level costs nothing.  One wave per (channel, segment) up to L = 512, one workgroup beyond; the
// samples stay in registers (eight a thread) up to L = 512 resp. 2048 and are read a second time, from L2, beyond.  A wave
// adds by an xor butterfly, a workgroup adds its four wave sums in wave order: the same bits on every run.
constexpr int SM_REG = 8, SM_WAVE_L = 64 * SM_REG;
__device__ __forceinline__ double sm_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
template <typename T, bool BLOCK>
__global__ __launch_bounds__(256) void segment_moments_kernel(const void* __restrict__ x, long long row_stride,
                                                              double* __restrict__ mean, double* __restrict__ sd, long long s0,
                                                              long long L, long long n_seg, long long total) {
  __shared__ double red[2][4];
  constexpr int NT = BLOCK ? 256 : 64;
  const int t = BLOCK ? (int)threadIdx.x : (int)(threadIdx.x & 63), wave = threadIdx.x >> 6;
  const long long item = BLOCK ? (long long)blockIdx.x : blockIdx.x * 4LL + wave;
  const bool live = item < total;                                  // BLOCK: always
  const long long c = live ? item / n_seg : 0, g = live ? item - c * n_seg : 0;
  const long long base = c * row_stride + s0 + g * L;
  const long long len = live ? L : 0;
  const bool in_regs = L <= (long long)NT * SM_REG;                // uniform
  double v[SM_REG], s = 0.0;
  if (in_regs) {
#pragma unroll
    for (int u = 0; u < SM_REG; ++u) {
      const int i = t + u * NT;
      v[u] = i < len ? ldd<T>(x, base + i) : 0.0;
      s += v[u];
    }
  } else {
    for (long long i = t; i < len; i += NT) s += ldd<T>(x, base + i);
  }
  s = sm_wave_sum(s);
  if (BLOCK) {
    if ((threadIdx.x & 63) == 0) red[0][wave] = s;
    __syncthreads();
    s = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  }
  const double mu = s / (double)L;
  double q = 0.0;
  if (in_regs) {
#pragma unroll
    for (int u = 0; u < SM_REG; ++u) {
      const double d = v[u] - mu;
      if (t + u * NT < len) q = fma(d, d, q);
    }
  } else {
    for (long long i = t; i < len; i += NT) {
      const double d = ldd<T>(x, base + i) - mu;
      q = fma(d, d, q);
    }
  }
  q = sm_wave_sum(q);
  if (BLOCK) {
    if ((threadIdx.x & 63) == 0) red[1][wave] = q;
    __syncthreads();
    q = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
  if (live && t == 0) {
    mean[item] = mu;
    sd[item] = sqrt(q / (double)L);
  }
}

// ------------------------------------------------------------------------------------------
// FFT resampling (scipy.signal.resample as used by preprocess/signal/downsample.py:21-27): the DFT of
// an arbitrary length n is evaluated with Bluestein's chirp-z identity on a power-of-two Stockham
// FFT (fp64, complex interleaved, batched over channels).  Chirps, their spectra and the twiddle
// table are coefficient data prepared by the host.
// ------------------------------------------------------------------------------------------
struct c64 { double re, im; };
__device__ __forceinline__ c64 cmul(c64 a, c64 b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ c64 cconj(c64 a) { return {a.re, -a.im}; }

// one radix-2 Stockham pass: out[j0] = a + w b, out[j0 + ns] = a - w b
__global__ __launch_bounds__(256) void fft_pass_kernel(const c64* __restrict__ in, c64* __restrict__ out,
                                                       const c64* __restrict__ tw, long long total_half, int m2, int ns,
                                                       int inverse) {
  const int half = m2 >> 1;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total_half; i += (long long)gridDim.x * blockDim.x) {
    const long long c = i / half;
    const int j = (int)(i % half);
    const int k = j & (ns - 1);
    c64 w = tw[(long long)k * (half / ns)];                 // exp(-2 pi i k / (2 ns))
    if (inverse) w.im = -w.im;
    const c64 a = in[c * m2 + j];
    const c64 b = cmul(in[c * m2 + j + half], w);
    const int j0 = ((j - k) << 1) + k;
    out[c * m2 + j0] = {a.re + b.re, a.im + b.im};
    out[c * m2 + j0 + ns] = {a.re - b.re, a.im - b.im};
  }
}

// a[c][j] = x[c][j] * conj(w[j]) for j < n, 0 up to m2
template <typename T>
__global__ __launch_bounds__(256) void rs_prep_kernel(const void* __restrict__ x, const c64* __restrict__ w, c64* __restrict__ a,
                                                      long long total, int n, int m2) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(i % m2);
    const long long c = i / m2;
    c64 v = {0.0, 0.0};
    if (j < n) {
      const double xv = ldd<T>(x, c * n + j);
      v = {xv * w[j].re, -xv * w[j].im};
    }
    a[i] = v;
  }
}
// A[c][m] *= Bf[m]
__global__ __launch_bounds__(256) void rs_cmul_kernel(c64* __restrict__ A, const c64* __restrict__ Bf, long long total, int m2) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    A[i] = cmul(A[i], Bf[i % m2]);
}
// Spectrum hand-over.  c1 (c, m2a) holds the chirp-convolved forward transform (un-normalised inverse
// FFT, scale 1/m2a folded in here): X[k] = conj(w1[k]) c1[k] / m2a, k < nx.  Build the half-spectrum Y
// of scipy.signal.resample (copy up to the smaller Nyquist; double / halve the shared Nyquist bin),
// extend it Hermitian-ly as irfft does, and emit a2[k] = conj(Yc[k]) conj(w2[k]) padded to m2b.
__global__ __launch_bounds__(256) void rs_spec_kernel(const c64* __restrict__ c1, const c64* __restrict__ w1,
                                                      const c64* __restrict__ w2, c64* __restrict__ a2, long long total,
                                                      int nx, int num, int m2a, int m2b) {
  const int N = nx < num ? nx : num;
  const int nyq = N / 2 + 1;
  const double inv = 1.0 / (double)m2a;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % m2b);
    const long long c = i / m2b;
    c64 v = {0.0, 0.0};
    if (k < num) {
      const int kk = (k <= num / 2) ? k : num - k;          // index into the half spectrum Y
      c64 y = {0.0, 0.0};
      if (kk < nyq) {
        const c64 cx = c1[c * m2a + kk];
        y = cmul(cconj(w1[kk]), cx);
        y.re *= inv;
        y.im *= inv;
        if (N % 2 == 0 && kk == N / 2) {
          const double f = (num < nx) ? 2.0 : ((nx < num) ? 0.5 : 1.0);
          y.re *= f;
          y.im *= f;
        }
      }
      if (kk == 0 || (num % 2 == 0 && kk == num / 2)) y.im = 0.0;      // C2R ignores these imaginary parts
      const c64 yc = (k <= num / 2) ? y : cconj(y);
      v = cmul(cconj(yc), cconj(w2[k]));
    }
    a2[i] = v;
  }
}
// y[c][m] = Re(conj(w2[m]) c2[m]) / (m2b * nx)      (ifft = conj(DFT(conj .))/num, times num/nx)
template <typename T>
__global__ __launch_bounds__(256) void rs_out_kernel(const c64* __restrict__ c2, const c64* __restrict__ w2, T* __restrict__ y,
                                                     long long total, int num, int m2b, double scale) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i % num);
    const long long c = i / num;
    const c64 d = cmul(cconj(w2[m]), c2[c * m2b + m]);
    y[i] = (T)(d.re * scale);
  }
}

// ------------------------------------------------------------------------------------------
// DFT-domain Gaussian Hilbert bank (frequency_filter.py:155-184 taken literally): X = DFT(x); per band
// z_b = IDFT(X . K_b), K_b = H_b x analytic multiplier (real, host coefficient data); y = mean_b |z_b| or Re z_b.
// Arbitrary recording length through Bluestein on the Stockham passes above.  This is the path for bands whose
// time-domain kernels are too long for tl_gauss_envelope's LDS window (low bands at a raw recording rate).
// ------------------------------------------------------------------------------------------
// X[c][k] = conj(w[k]) c1[c][k] / m2, k < n   (c1 = chirp-convolved forward transform, un-normalised)
__global__ __launch_bounds__(256) void hb_spec_kernel(const c64* __restrict__ c1, const c64* __restrict__ w, c64* __restrict__ X,
                                                      long long total, int n, int m2) {
  const double inv = 1.0 / (double)m2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % n);
    const long long c = i / n;
    c64 v = cmul(cconj(w[k]), c1[c * m2 + k]);
    X[i] = {v.re * inv, v.im * inv};
  }
}
// a[c][k] = conj(X[c][k] K[k]) conj(w[k]) for k < n, 0 up to m2: Bluestein input of DFT(conj(Z)), Z = X K
__global__ __launch_bounds__(256) void hb_band_prep_kernel(const c64* __restrict__ X, const double* __restrict__ K,
                                                           const c64* __restrict__ w, c64* __restrict__ a, long long total,
                                                           int n, int m2) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % m2);
    const long long c = i / m2;
    c64 v = {0.0, 0.0};
    if (k < n) {
      const c64 x = X[c * n + k];
      const double kk = K[k];
      v = cmul(c64{x.re * kk, -x.im * kk}, cconj(w[k]));
    }
    a[i] = v;
  }
}
// d = conj(w[t]) c2[c][t] / m2 = DFT(conj Z)[t]; z[t] = conj(d) / n.  y (+)= (|d| or Re d) * scale
__global__ __launch_bounds__(256) void hb_accum_kernel(const c64* __restrict__ c2, const c64* __restrict__ w, double* __restrict__ y,
                                                       long long total, int n, int m2, double scale, int envelope, int first) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i % n);
    const long long c = i / n;
    const c64 d = cmul(cconj(w[t]), c2[c * m2 + t]);
    const double v = (envelope ? sqrt(d.re * d.re + d.im * d.im) : d.re) * scale;
    y[i] = first ? v : y[i] + v;
  }
}

static inline unsigned sgrid(long long total) {
  long long g = (total + 255) / 256;
  if (g < 1) g = 1;
  if (g > 8192) g = 8192;
  return (unsigned)g;
}

}  // namespace tl
using namespace tl;

extern "C" int tl_row_zscore(const void* x, int is_f64, void* y, double* stats, int C, int64_t T, int64_t t0, int64_t t1,
                             int zero_nans, void* stream) {
  TL_REQUIRE(x && y && stats && C > 0 && T > 0, "row_zscore: bad arguments");
  TL_REQUIRE(t0 >= 0 && t1 <= T && t0 < t1, "row_zscore: statistics interval out of bounds");
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)C * T;
  if (is_f64) {
    hipLaunchKernelGGL((row_stats_kernel<double>), dim3(C), dim3(256), 0, st, x, stats, (long long)T, (long long)t0, (long long)t1);
    hipLaunchKernelGGL((row_normalise_kernel<double>), dim3(sgrid(total)), dim3(256), 0, st, x, stats, (double*)y, total, (long long)T, zero_nans);
  } else {
    hipLaunchKernelGGL((row_stats_kernel<float>), dim3(C), dim3(256), 0, st, x, stats, (long long)T, (long long)t0, (long long)t1);
    hipLaunchKernelGGL((row_normalise_kernel<float>), dim3(sgrid(total)), dim3(256), 0, st, x, stats, (float*)y, total, (long long)T, zero_nans);
  }
  return check_launch("row_zscore");
}

extern "C" int tl_car(const void* x, int is_f64, const int32_t* include, void* y, int C, int64_t T, int n_inc, void* stream) {
  TL_REQUIRE(x && include && y && C > 0 && T > 0 && n_inc > 0, "car: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    hipLaunchKernelGGL((car_kernel<double>), dim3(sgrid(T)), dim3(256), 0, st, x, include, (double*)y, C, (long long)T, n_inc);
  else
    hipLaunchKernelGGL((car_kernel<float>), dim3(sgrid(T)), dim3(256), 0, st, x, include, (float*)y, C, (long long)T, n_inc);
  return check_launch("car");
}

extern "C" int tl_rolling_zscore(const void* x, int is_f64, double* y, int C, int64_t T, int window, int zero_nans, void* stream) {
  TL_REQUIRE(x && y && C > 0 && C <= 65535 && T > 0, "rolling_zscore: bad arguments");
  TL_REQUIRE(window > 1, "rolling_zscore: window_size must be greater than 1.");
  TL_REQUIRE(T <= INT32_MAX - RZ_TB, "rolling_zscore: recording too long");
  // a window wider than the recording holds the same samples as one of length T (the rest lies before t = 0)
  const int W = window < T ? window : (int)T;
  const size_t lds = (size_t)(RZ_TB + W - 1 < RZ_CHUNK ? RZ_TB + W - 1 : RZ_CHUNK) * sizeof(double);
  dim3 grid((unsigned)((T + RZ_TB - 1) / RZ_TB), (unsigned)C);
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    hipLaunchKernelGGL((rolling_zscore_kernel<double>), grid, dim3(256), lds, st, x, y, (long long)T, W, zero_nans);
  else
    hipLaunchKernelGGL((rolling_zscore_kernel<float>), grid, dim3(256), lds, st, x, y, (long long)T, W, zero_nans);
  return check_launch("rolling_zscore");
}

extern "C" int tl_rolling_zscore_blocked(const void* x, int is_f64, double* y, double* work, int64_t work_elems, int C, int64_t T,
                                         int window, int zero_nans, void* stream) {
  TL_REQUIRE(x && y && work, "rolling_zscore_blocked: null pointer");
  TL_REQUIRE(C > 0 && C <= 65535 && T > 0, "rolling_zscore_blocked: C must lie in [1, 65535] and T must be positive");
  TL_REQUIRE(window > 1, "rolling_zscore_blocked: window_size must be greater than 1.");
  TL_REQUIRE(T <= INT32_MAX - RZ_TB, "rolling_zscore_blocked: recording too long");
  const int W = window < T ? window : (int)T;                    // as in tl_rolling_zscore
  TL_REQUIRE(W >= RZ_TB, "rolling_zscore_blocked: min(window, T) = %d is below %d; such windows run on the window kernel "
             "(tl_rolling_zscore)", W, RZ_TB);
  const int64_t tiles = (T + RZ_TB - 1) / RZ_TB;
  TL_REQUIRE(work_elems >= 8 * (int64_t)C * tiles, "rolling_zscore_blocked: the workspace holds %lld doubles, 8 * C * "
             "ceil(T / 256) = %lld are needed", (long long)work_elems, (long long)(8 * (int64_t)C * tiles));
  dim3 grid((unsigned)tiles, (unsigned)C);
  hipStream_t st = (hipStream_t)stream;
  if (is_f64) {
    hipLaunchKernelGGL((rz_tile_moments<double>), grid, dim3(256), 0, st, x, work, (long long)T);
    hipLaunchKernelGGL((rolling_zscore_blocked_kernel<double>), grid, dim3(256), 0, st, x, work, y, (long long)T, W, zero_nans);
  } else {
    hipLaunchKernelGGL((rz_tile_moments<float>), grid, dim3(256), 0, st, x, work, (long long)T);
    hipLaunchKernelGGL((rolling_zscore_blocked_kernel<float>), grid, dim3(256), 0, st, x, work, y, (long long)T, W, zero_nans);
  }
  return check_launch("rolling_zscore_blocked");
}

extern "C" int tl_segment_moments(const void* x, int x_is_f64, int64_t row_stride, double* mean, double* std, int C, int64_t T,
                                  int64_t s0, int64_t L, int64_t n_seg, void* stream) {
  TL_REQUIRE(x && mean && std, "segment_moments: null pointer");
  TL_REQUIRE(C >= 1 && T >= 1 && T <= (1LL << 40) && row_stride >= T, "segment_moments: C and T must be at least 1 and "
             "row_stride >= T");
  TL_REQUIRE(s0 >= 0 && L >= 1 && n_seg >= 1, "segment_moments: s0 >= 0, L >= 1 and n_seg >= 1 are required (got %lld, %lld, "
             "%lld)", (long long)s0, (long long)L, (long long)n_seg);
  TL_REQUIRE(s0 <= T && n_seg <= (T - s0) / L, "segment_moments: s0 + n_seg * L = %lld + %lld * %lld runs past T = %lld",
             (long long)s0, (long long)n_seg, (long long)L, (long long)T);
  const long long total = (long long)C * n_seg;
  TL_REQUIRE(total <= 0x7fffffffLL, "segment_moments: too many segments for one launch");
  hipStream_t st = (hipStream_t)stream;
#define SM_LAUNCH(TIN)                                                                                                  \
  if (L <= SM_WAVE_L)                                                                                                   \
    hipLaunchKernelGGL((segment_moments_kernel<TIN, false>), dim3((unsigned)((total + 3) / 4)), dim3(256), 0, st, x,         \
                       (long long)row_stride, mean, std, (long long)s0, (long long)L, (long long)n_seg, total);               \
  else                                                                                                                  \
    hipLaunchKernelGGL((segment_moments_kernel<TIN, true>), dim3((unsigned)total), dim3(256), 0, st, x, (long long)row_stride, \
                       mean, std, (long long)s0, (long long)L, (long long)n_seg, total)
  if (x_is_f64) {
    SM_LAUNCH(double);
  } else {
    SM_LAUNCH(float);
  }
#undef SM_LAUNCH
  return check_launch("segment_moments");
}

// in-place power-of-two FFT of `buf` (C, m2) complex128 with scratch `tmp`; result ends in `buf`
static int fft_pow2(tl::c64* buf, tl::c64* tmp, const tl::c64* tw, int C, int m2, int inverse, hipStream_t st) {
  tl::c64* in = buf;
  tl::c64* out = tmp;
  const long long total_half = (long long)C * (m2 / 2);
  for (int ns = 1; ns < m2; ns <<= 1) {
    hipLaunchKernelGGL(tl::fft_pass_kernel, dim3(sgrid(total_half)), dim3(256), 0, st, in, out, tw, total_half, m2, ns, inverse);
    tl::c64* t = in; in = out; out = t;
  }
  if (in != buf && hipMemcpyAsync(buf, in, sizeof(tl::c64) * (size_t)C * m2, hipMemcpyDeviceToDevice, st) != hipSuccess)
  {
    tl::set_error("fft_pow2: device copy failed");
    return -1;
  }
  return check_launch("fft_pow2");
}

extern "C" int tl_fft_resample(const void* x, int is_f64, void* y, int C, int64_t nx, int64_t num, const double* w1,
                               const double* bf1, const double* tw1, int m2a, const double* w2, const double* bf2,
                               const double* tw2, int m2b, double* work, void* stream) {
  TL_REQUIRE(x && y && w1 && bf1 && tw1 && w2 && bf2 && tw2 && work, "fft_resample: null pointer");
  TL_REQUIRE(C > 0 && nx > 1 && num > 0, "fft_resample: bad sizes");
  TL_REQUIRE(m2a >= 2 * nx - 1 && (m2a & (m2a - 1)) == 0 && m2b >= 2 * num - 1 && (m2b & (m2b - 1)) == 0,
             "fft_resample: m2a/m2b must be powers of two >= 2n-1");
  hipStream_t st = (hipStream_t)stream;
  const int mmax = m2a > m2b ? m2a : m2b;
  tl::c64* A = reinterpret_cast<tl::c64*>(work);                 // (C, mmax)
  tl::c64* T = A + (size_t)C * mmax;                              // scratch (C, mmax)
  tl::c64* A2 = T + (size_t)C * mmax;                             // (C, m2b)
  const tl::c64* W1 = reinterpret_cast<const tl::c64*>(w1);
  const tl::c64* W2 = reinterpret_cast<const tl::c64*>(w2);
  const long long ta = (long long)C * m2a, tb = (long long)C * m2b;
  if (is_f64)
    hipLaunchKernelGGL((tl::rs_prep_kernel<double>), dim3(sgrid(ta)), dim3(256), 0, st, x, W1, A, ta, (int)nx, m2a);
  else
    hipLaunchKernelGGL((tl::rs_prep_kernel<float>), dim3(sgrid(ta)), dim3(256), 0, st, x, W1, A, ta, (int)nx, m2a);
  int rc = fft_pow2(A, T, reinterpret_cast<const tl::c64*>(tw1), C, m2a, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(tl::rs_cmul_kernel, dim3(sgrid(ta)), dim3(256), 0, st, A, reinterpret_cast<const tl::c64*>(bf1), ta, m2a);
  rc = fft_pow2(A, T, reinterpret_cast<const tl::c64*>(tw1), C, m2a, 1, st);
  if (rc) return rc;
  hipLaunchKernelGGL(tl::rs_spec_kernel, dim3(sgrid(tb)), dim3(256), 0, st, A, W1, W2, A2, tb, (int)nx, (int)num, m2a, m2b);
  rc = fft_pow2(A2, T, reinterpret_cast<const tl::c64*>(tw2), C, m2b, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(tl::rs_cmul_kernel, dim3(sgrid(tb)), dim3(256), 0, st, A2, reinterpret_cast<const tl::c64*>(bf2), tb, m2b);
  rc = fft_pow2(A2, T, reinterpret_cast<const tl::c64*>(tw2), C, m2b, 1, st);
  if (rc) return rc;
  const long long to = (long long)C * num;
  const double scale = 1.0 / ((double)m2b * (double)nx);
  if (is_f64)
    hipLaunchKernelGGL((tl::rs_out_kernel<double>), dim3(sgrid(to)), dim3(256), 0, st, A2, W2, (double*)y, to, (int)num, m2b, scale);
  else
    hipLaunchKernelGGL((tl::rs_out_kernel<float>), dim3(sgrid(to)), dim3(256), 0, st, A2, W2, (float*)y, to, (int)num, m2b, scale);
  return check_launch("fft_resample");
}

extern "C" int tl_hilbert_fft(const void* x, int is_f64, double* y, int C, int64_t T, const double* kernels, int nb,
                              const double* w, const double* bf, const double* tw, int m2, int envelope, double* work,
                              void* stream) {
  TL_REQUIRE(x && y && kernels && w && bf && tw && work, "hilbert_fft: null pointer");
  TL_REQUIRE(C > 0 && T > 1 && nb > 0, "hilbert_fft: bad sizes");
  TL_REQUIRE(m2 >= 2 * T - 1 && (m2 & (m2 - 1)) == 0, "hilbert_fft: m2 must be a power of two >= 2T-1");
  TL_REQUIRE(T < (1LL << 30), "hilbert_fft: recording too long");
  hipStream_t st = (hipStream_t)stream;
  tl::c64* A = reinterpret_cast<tl::c64*>(work);                 // (C, m2)
  tl::c64* Tm = A + (size_t)C * m2;                              // scratch (C, m2)
  tl::c64* X = Tm + (size_t)C * m2;                              // (C, T) spectrum
  const tl::c64* W = reinterpret_cast<const tl::c64*>(w);
  const tl::c64* BF = reinterpret_cast<const tl::c64*>(bf);
  const tl::c64* TW = reinterpret_cast<const tl::c64*>(tw);
  const long long ta = (long long)C * m2, tx = (long long)C * T;
  const int n = (int)T;
  if (is_f64)
    hipLaunchKernelGGL((tl::rs_prep_kernel<double>), dim3(sgrid(ta)), dim3(256), 0, st, x, W, A, ta, n, m2);
  else
    hipLaunchKernelGGL((tl::rs_prep_kernel<float>), dim3(sgrid(ta)), dim3(256), 0, st, x, W, A, ta, n, m2);
  int rc = fft_pow2(A, Tm, TW, C, m2, 0, st);
  if (rc) return rc;
  hipLaunchKernelGGL(tl::rs_cmul_kernel, dim3(sgrid(ta)), dim3(256), 0, st, A, BF, ta, m2);
  rc = fft_pow2(A, Tm, TW, C, m2, 1, st);
  if (rc) return rc;
  hipLaunchKernelGGL(tl::hb_spec_kernel, dim3(sgrid(tx)), dim3(256), 0, st, A, W, X, tx, n, m2);
  const double scale = 1.0 / ((double)m2 * (double)T * (double)nb);
  for (int b = 0; b < nb; ++b) {
    hipLaunchKernelGGL(tl::hb_band_prep_kernel, dim3(sgrid(ta)), dim3(256), 0, st, X, kernels + (size_t)b * T, W, A, ta, n, m2);
    rc = fft_pow2(A, Tm, TW, C, m2, 0, st);
    if (rc) return rc;
    hipLaunchKernelGGL(tl::rs_cmul_kernel, dim3(sgrid(ta)), dim3(256), 0, st, A, BF, ta, m2);
    rc = fft_pow2(A, Tm, TW, C, m2, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(tl::hb_accum_kernel, dim3(sgrid(tx)), dim3(256), 0, st, A, W, y, tx, n, m2, scale, envelope, b == 0 ? 1 : 0);
  }
  return check_launch("hilbert_fft");
}
