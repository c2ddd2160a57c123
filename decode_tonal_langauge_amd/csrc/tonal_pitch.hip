// F0 tracking of a batch of clips: the YIN estimator (de Cheveigne & Kawahara 2002) with the steps of librosa 0.10's `yin`
// (pad_mode='constant'), one workgroup per frame, fp64 throughout (utils/audio.py yin_f0 is the host statement).
//
// The difference function is the DIRECT sum d[tau] = sum_j (x[j] - x[j + tau])^2: every term is non-negative, so the sum has a
// relative error bound of (W + 2) u in any order.  The FFT form E(0) + E(tau) - 2 r(tau) cancels exactly where d -> 0, at the
// period of a voiced frame; it is not used, and neither is an f64-MFMA Toeplitz product, which is the same form.
#include "tonal_common.h"
#include <float.h>
#include <limits.h>

namespace tl {

#define YIN_THREADS 256
#define YIN_MAX_FRAME 4096
#define YIN_TILE 4                      // lags a lane carries through one sweep over the window

// d[tau] for the R lags tau0 + 256 r of this lane: x[j] is one broadcast read per step, x[j + tau] is consecutive across the
// lanes (8-byte reads, conflict-free).  A lag past pmax reads lag pmax instead (in bounds) and is not stored.
template <int R>
__device__ __forceinline__ void yin_diff_sweep(const double* __restrict__ xs, double* __restrict__ d, int W, int tau0, int pmax) {
  const double* p[R];
  double acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int tau = tau0 + YIN_THREADS * r;
    p[r] = xs + (tau <= pmax ? tau : pmax);
    acc[r] = 0.0;
  }
#pragma unroll 4
  for (int j = 0; j < W; ++j) {
    const double xj = xs[j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double df = xj - p[r][j];
      acc[r] = fma(df, df, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int tau = tau0 + YIN_THREADS * r;
    if (tau <= pmax) d[tau] = acc[r];
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid: N * n_frames blocks of 256 threads; dynamic LDS: frame_length + max_period + 1 doubles
template <typename TIN>
__global__ __launch_bounds__(YIN_THREADS) void yin_f0_kernel(const TIN* __restrict__ audio, long long row_stride, double* __restrict__ f0,
                                                             double* __restrict__ aper, int32_t* __restrict__ pidx,
                                                             double* __restrict__ rms, double* __restrict__ cmnd, long long S,
                                                             int frame_length, int W, int hop, int pad, int pmin, int pmax,
                                                             double threshold, double sr, long long n_frames) {
  extern __shared__ __attribute__((aligned(16))) double yin_lds[];
  __shared__ double s_red[YIN_THREADS / 64];
  __shared__ int s_first[YIN_THREADS / 64];
  __shared__ int s_arg[YIN_THREADS / 64];
  double* xs = yin_lds;                         // the frame
  double* d = yin_lds + frame_length;           // d[0 .. pmax], then the CMND in place at d[pmin + i]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long frame = blockIdx.x;
  const long long n = frame / n_frames, f = frame - n * n_frames;
  const TIN* row = audio + n * row_stride;
  const long long start = f * hop - pad;

  // the frame, zero outside [0, S): the centre padding is an index check
  double sq = 0.0;
  for (int k = tid; k < frame_length; k += YIN_THREADS) {
    const long long s = start + k;
    const double v = (s >= 0 && s < S) ? (double)row[s] : 0.0;
    xs[k] = v;
    if (k < W) sq = fma(v, v, sq);
  }
  sq = wave_sum(sq);
  if (lane == 0) s_red[wave] = sq;
  __syncthreads();
  const double sumsq = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);

  // 1. difference function, lags 1 .. pmax (d[0] is never read)
  for (int base = 1; base <= pmax; base += YIN_THREADS * YIN_TILE) {
    const int groups = (pmax - base) / YIN_THREADS + 1;          // lag groups of 256 left, block-uniform
    const int tau0 = base + tid;
    if (groups >= 4) yin_diff_sweep<4>(xs, d, W, tau0, pmax);
    else if (groups == 3) yin_diff_sweep<3>(xs, d, W, tau0, pmax);
    else if (groups == 2) yin_diff_sweep<2>(xs, d, W, tau0, pmax);
    else yin_diff_sweep<1>(xs, d, W, tau0, pmax);
  }
  __syncthreads();

  // 2. + 3. running sum over the lags as a block scan (a lane owns `chunk` consecutive lags), CMND written over d
  const int chunk = (pmax + YIN_THREADS - 1) / YIN_THREADS;
  const int lo = 1 + tid * chunk;
  const int hi = lo + chunk < pmax + 1 ? lo + chunk : pmax + 1;
  double own = 0.0;
  for (int tau = lo; tau < hi; ++tau) own += d[tau];
  double incl = own;                                              // inclusive scan of the lane totals inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();                                                // s_red was read above by every thread
  if (lane == 63) s_red[wave] = incl;
  __syncthreads();
  // the exclusive prefix by additions alone (never incl - own): every partial sum is a sum of non-negative terms, so the
  // gamma_n bound holds whatever the order
  double before = __shfl_up(incl, 1, 64);
  if (lane == 0) before = 0.0;
  double waves_before = 0.0;
  for (int w = 0; w < wave; ++w) waves_before += s_red[w];
  double run = before + waves_before;
  for (int tau = lo; tau < hi; ++tau) {
    const double dt = d[tau];
    run += dt;
    if (tau >= pmin) d[tau] = dt / (run / (double)tau + DBL_MIN);
  }
  __syncthreads();

  // 4. + 5. the first trough below the threshold, else the lowest index of the global minimum
  const double* c = d + pmin;
  const int nc = pmax - pmin + 1;
  int first = INT_MAX, arg = INT_MAX;
  double best = INFINITY;
  for (int i = tid; i < nc; i += YIN_THREADS) {
    const double ci = c[i];
    bool trough = false;
    if (i == 0) trough = ci < c[1];
    else if (i < nc - 1) trough = ci < c[i - 1] && ci <= c[i + 1];
    if (trough && ci < threshold && i < first) first = i;
    if (ci < best) { best = ci; arg = i; }                        // i rises within a lane: the lowest index of a tie stays
    if (cmnd) cmnd[frame * nc + i] = ci;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int of = __shfl_down(first, o, 64);
    const double ob = __shfl_down(best, o, 64);
    const int oa = __shfl_down(arg, o, 64);
    first = of < first ? of : first;
    if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (lane == 0) { s_first[wave] = first; s_red[wave] = best; s_arg[wave] = arg; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < YIN_THREADS / 64; ++w) {
      first = s_first[w] < first ? s_first[w] : first;
      if (s_red[w] < best || (s_red[w] == best && s_arg[w] < arg)) { best = s_red[w]; arg = s_arg[w]; }
    }
    int i = first != INT_MAX ? first : arg;
    if (i < 0 || i >= nc) i = 0;                                  // a frame of NaN compares false everywhere
    // 6. parabolic shift on the three values around the pick
    double shift = 0.0;
    if (i > 0 && i < nc - 1) {
      const double a = c[i + 1] + c[i - 1] - 2.0 * c[i];
      const double b = (c[i + 1] - c[i - 1]) / 2.0;
      if (fabs(b) < fabs(a)) shift = -b / a;
    }
    f0[frame] = sr / ((double)(pmin + i) + shift);
    aper[frame] = c[i];
    pidx[frame] = i;
    rms[frame] = sqrt(sumsq / (double)W);
  }
}

}  // namespace tl
using namespace tl;

extern "C" int tl_yin_f0(const void* audio, int audio_is_f64, int64_t row_stride, double* f0, double* aperiodicity,
                         int32_t* period_index, double* rms, double* cmnd, int N, int64_t S, int frame_length, int win_length,
                         int hop, int center, int min_period, int max_period, double threshold, double sr, int64_t n_frames,
                         void* stream) {
  TL_REQUIRE(audio && f0 && aperiodicity && period_index && rms, "yin_f0: null pointer");
  TL_REQUIRE(N >= 1 && S >= 1, "yin_f0: N and S must be at least 1 (got %d, %lld)", N, (long long)S);
  TL_REQUIRE(win_length >= 1 && win_length < frame_length && frame_length <= YIN_MAX_FRAME,
             "yin_f0: 1 <= win_length < frame_length <= %d is required (got win_length %d, frame_length %d)", YIN_MAX_FRAME,
             win_length, frame_length);
  TL_REQUIRE(hop >= 1, "yin_f0: hop must be at least 1 (got %d)", hop);
  TL_REQUIRE(min_period >= 1 && min_period + 1 <= max_period && max_period <= frame_length - win_length - 1,
             "yin_f0: 1 <= min_period, min_period + 1 <= max_period <= frame_length - win_length - 1 = %d is required (got "
             "min_period %d, max_period %d)", frame_length - win_length - 1, min_period, max_period);
  TL_REQUIRE(threshold > 0.0, "yin_f0: threshold must be positive");
  TL_REQUIRE(sr > 0.0, "yin_f0: sr must be positive");
  TL_REQUIRE(center || S >= frame_length, "yin_f0: a clip of %lld samples is shorter than frame_length = %d (center = 0)",
             (long long)S, frame_length);
  const int64_t expect = center ? 1 + S / hop : 1 + (S - frame_length) / hop;
  TL_REQUIRE(n_frames == expect, "yin_f0: n_frames = %lld, but S, hop and center give %lld", (long long)n_frames,
             (long long)expect);
  TL_REQUIRE(N == 1 || row_stride >= S, "yin_f0: row_stride = %lld is below S = %lld", (long long)row_stride, (long long)S);
  const long long blocks = (long long)N * n_frames;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "yin_f0: too many frames for one launch");
  const size_t lds = (size_t)(frame_length + max_period + 1) * sizeof(double);
  const void* fn = audio_is_f64 ? reinterpret_cast<const void*>(yin_f0_kernel<double>)
                                : reinterpret_cast<const void*>(yin_f0_kernel<float>);
  if (lds + 256 > 64 * 1024) {      // with the static words more than 64 KB of the CU's 160 KB: raise the per-block limit once
    static thread_local int raised_on[2] = {-1, -1};
    int devid = 0;
    (void)hipGetDevice(&devid);
    if (raised_on[audio_is_f64 != 0] != devid) {
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * YIN_MAX_FRAME * (int)sizeof(double));
      if (e != hipSuccess) {
        set_error("yin_f0: cannot raise the dynamic LDS limit for frame_length %d: %s", frame_length, hipGetErrorString(e));
        return TL_ELAUNCH;
      }
      raised_on[audio_is_f64 != 0] = devid;
    }
  }
  const int pad = center ? frame_length / 2 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (audio_is_f64)
    hipLaunchKernelGGL((yin_f0_kernel<double>), dim3((unsigned)blocks), dim3(YIN_THREADS), lds, st, (const double*)audio,
                       (long long)row_stride, f0, aperiodicity, period_index, rms, cmnd, (long long)S, frame_length, win_length, hop,
                       pad, min_period, max_period, threshold, sr, (long long)n_frames);
  else
    hipLaunchKernelGGL((yin_f0_kernel<float>), dim3((unsigned)blocks), dim3(YIN_THREADS), lds, st, (const float*)audio,
                       (long long)row_stride, f0, aperiodicity, period_index, rms, cmnd, (long long)S, frame_length, win_length, hop,
                       pad, min_period, max_period, threshold, sr, (long long)n_frames);
  return check_launch("yin_f0");
}
