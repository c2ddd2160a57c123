// Mel-spectrogram targets of a batch of trials (utils/audio.py: audio_to_mel = STFT -> |.|^power -> mel bank -> dB, one
// NumPy call per trial on the host).  Two launches for the whole (N, S) batch, all arithmetic fp64, float32 only at the
// final store; see include/tonal_hip.h for the contracts.
//
// tl_mel_power: a workgroup of 256 threads holds 1024 complex points in LDS = 1024 / M frames of M = n_fft / 2 points each
// (one frame at n_fft 2048, eight at 256), so a thread always owns four points of one frame and every size runs the same
// code with full waves.  Per frame:
//   gather   z[m] = w[2m] x[2m] + i w[2m+1] x[2m+1] straight from the audio row (centre padding = an index test, no padded
//            copy); a thread loads the four points j + r M/4 its first butterfly needs, so the frame never goes through LDS;
//   FFT_M    Stockham autosort, radix 4 (plus one radix-2 pass when log2 M is odd), ping-pong between two LDS images,
//            twiddles from one full-circle table W_nfft^i (W_{4 Ns}^{rk} = W_nfft^{rk nfft / 4 Ns}), all loaded up front;
//   unpack   X[k] = E[k] + W_nfft^k O[k],  E = (Z[k] + conj Z[M-k]) / 2,  O = (Z[k] - conj Z[M-k]) / 2i,  k = 0..M,
//            and |X|^2 (or |X|) goes to the LDS image the last pass has finished reading;
//   mel      band m touches bins [first, last) only: four lanes per (frame, band) stride over the run and add up through
//            two shuffles - the dense n_mels x (M + 1) product would be 97 % zeros at 80 bands;
//   max      the workgroup's largest value -> one vector atomic max per workgroup on the bit pattern of rowmax[n] (the values
//            are non-negative doubles, whose order is the order of their bit patterns; max is order-independent).
// LDS: 4 images of 1024 + 64 doubles = 34 KB -> four workgroups per CU.  The index padding d + (d >> 4) takes the stride-4
// stores of the first pass off each other's banks (a 16-lane store group then covers 16 different bank pairs).
#include "tonal_common.h"
#include <math.h>

namespace tl {

constexpr int MEL_PTS = 1024, MEL_Q = MEL_PTS / 4, MEL_PAD = MEL_PTS + (MEL_PTS >> 4);
__device__ __forceinline__ int mel_idx(int d) { return d + (d >> 4); }
typedef double mel_d2 __attribute__((ext_vector_type(2)));

template <typename T>
__device__ __forceinline__ double mel_ld(const void* p, long long i) { return (double)static_cast<const T*>(p)[i]; }

// forward radix-4 butterfly: y[r] = sum_q x[q] (-i)^(rq)
__device__ __forceinline__ void mel_bfly(const double (&xr)[4], const double (&xi)[4], double (&yr)[4], double (&yi)[4]) {
  const double t0r = xr[0] + xr[2], t0i = xi[0] + xi[2], t1r = xr[0] - xr[2], t1i = xi[0] - xi[2];
  const double t2r = xr[1] + xr[3], t2i = xi[1] + xi[3];
  const double t3r = xi[1] - xi[3], t3i = xr[3] - xr[1];     // (x1 - x3) * (-i)
  yr[0] = t0r + t2r; yi[0] = t0i + t2i;
  yr[1] = t1r + t3r; yi[1] = t1i + t3i;
  yr[2] = t0r - t2r; yi[2] = t0i - t2i;
  yr[3] = t1r - t3r; yi[3] = t1i - t3i;
}

// bands (n_mels, 3) int32: first bin, one past the last bin, offset of the band's first weight in `weights`
template <typename TIN, int LOG2M>
__global__ __launch_bounds__(MEL_Q) void mel_power_kernel(const void* __restrict__ audio, long long row_stride, long long S,
                                                          const mel_d2* __restrict__ window, const mel_d2* __restrict__ tw,
                                                          const int32_t* __restrict__ bands, const double* __restrict__ weights,
                                                          int n_weights, double* __restrict__ mel, double* __restrict__ rowmax,
                                                          int blocks_per_trial, long long n_frames, int hop, int center,
                                                          int power, int n_mels) {
  constexpr int M = 1 << LOG2M, NFFT = 2 * M, F = MEL_PTS / M, Q = M / 4, NS4 = LOG2M / 2, HAS2 = LOG2M & 1;
  constexpr int FIN = HAS2 ? (NS4 & 1) : ((NS4 - 1) & 1);    // the image that holds the transform
  __shared__ __attribute__((aligned(16))) double lds[4 * MEL_PAD];
  __shared__ double wmax[MEL_Q / 64];
  double* re[2] = {lds, lds + 2 * MEL_PAD};
  double* im[2] = {lds + MEL_PAD, lds + 3 * MEL_PAD};
  const int tid = threadIdx.x, fl = tid >> (LOG2M - 2), j = tid & (Q - 1), fbase = fl * M;
  const long long n = blockIdx.x / blocks_per_trial;
  const long long frame0 = (long long)(blockIdx.x % blocks_per_trial) * F;
  const long long frame = frame0 + fl;
  const long long start = frame * hop - (center ? M : 0);
  const long long row = n * row_stride;

  // the thread's twiddles of every pass, requested before the first barrier: one memory latency instead of one per pass
  mel_d2 twr[NS4][3], tw2[2];
#pragma unroll
  for (int st = 1; st < NS4; ++st)
#pragma unroll
    for (int r = 1; r < 4; ++r) twr[st][r - 1] = tw[r * (j & ((1 << (2 * st)) - 1)) * (NFFT >> (2 * st + 2))];
  if (HAS2) {
    tw2[0] = tw[2 * j];
    tw2[1] = tw[2 * (j + Q)];
  }
  // ---- gather + window + first pass (Ns = 1, no twiddles) straight from registers
  double xr[4], xi[4], yr[4], yi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * Q;
    const long long s0 = start + 2 * m, s1 = s0 + 1;
    const mel_d2 w = window[m];
    xr[r] = (frame < n_frames && s0 >= 0 && s0 < S) ? mel_ld<TIN>(audio, row + s0) * w[0] : 0.0;
    xi[r] = (frame < n_frames && s1 >= 0 && s1 < S) ? mel_ld<TIN>(audio, row + s1) * w[1] : 0.0;
  }
  mel_bfly(xr, xi, yr, yi);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    re[0][mel_idx(fbase + 4 * j + r)] = yr[r];
    im[0][mel_idx(fbase + 4 * j + r)] = yi[r];
  }
  __syncthreads();
  // ---- the other radix-4 passes: butterfly j reads j + r M/4 and writes (j / Ns) 4 Ns + (j % Ns) + r Ns
#pragma unroll
  for (int st = 1; st < NS4; ++st) {
    const int src = (st - 1) & 1, dst = st & 1, Ns = 1 << (2 * st), k = j & (Ns - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      xr[r] = re[src][mel_idx(fbase + j + r * Q)];
      xi[r] = im[src][mel_idx(fbase + j + r * Q)];
    }
#pragma unroll
    for (int r = 1; r < 4; ++r) {
      const mel_d2 w = twr[st][r - 1];                       // W_{4 Ns}^{rk} = W_nfft^{rk nfft / 4 Ns} as (cos, -sin)
      const double tr = fma(-xi[r], w[1], xr[r] * w[0]), ti = fma(xr[r], w[1], xi[r] * w[0]);
      xr[r] = tr;
      xi[r] = ti;
    }
    mel_bfly(xr, xi, yr, yi);
    const int j0 = ((j >> (2 * st)) << (2 * st + 2)) + k;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      re[dst][mel_idx(fbase + j0 + r * Ns)] = yr[r];
      im[dst][mel_idx(fbase + j0 + r * Ns)] = yi[r];
    }
    __syncthreads();
  }
  // ---- odd log2 M: one radix-2 pass (Ns = M / 2), two butterflies per thread
  if (HAS2) {
    constexpr int src = (NS4 - 1) & 1, dst = NS4 & 1, H = M / 2;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int jj = j + u * Q;
      const double ar = re[src][mel_idx(fbase + jj)], ai = im[src][mel_idx(fbase + jj)];
      const double br = re[src][mel_idx(fbase + jj + H)], bi = im[src][mel_idx(fbase + jj + H)];
      const mel_d2 w = tw2[u];                               // W_M^jj
      const double tr = fma(-bi, w[1], br * w[0]), ti = fma(br, w[1], bi * w[0]);
      re[dst][mel_idx(fbase + jj)] = ar + tr;
      im[dst][mel_idx(fbase + jj)] = ai + ti;
      re[dst][mel_idx(fbase + jj + H)] = ar - tr;
      im[dst][mel_idx(fbase + jj + H)] = ai - ti;
    }
    __syncthreads();
  }
  // ---- unpack to the M + 1 bins of the real transform, |X|^power into the image nobody reads any more
  double* pw = re[FIN ^ 1];                                  // [F][M + 1], F (M + 1) <= 1032 doubles
  for (int k = j; k <= M; k += Q) {
    const int ka = k & (M - 1), kb = (M - k) & (M - 1);
    const double ar = re[FIN][mel_idx(fbase + ka)], ai = im[FIN][mel_idx(fbase + ka)];
    const double cr = re[FIN][mel_idx(fbase + kb)], ci = im[FIN][mel_idx(fbase + kb)];
    const double er = 0.5 * (ar + cr), ei = 0.5 * (ai - ci);
    const double orr = 0.5 * (ai + ci), oi = -0.5 * (ar - cr);
    const mel_d2 w = tw[k];
    const double Xr = er + fma(-oi, w[1], orr * w[0]), Xi = ei + fma(orr, w[1], oi * w[0]);
    const double p2 = fma(Xr, Xr, Xi * Xi);
    pw[fl * (M + 1) + k] = power == 2 ? p2 : sqrt(p2);
  }
  __syncthreads();
  // ---- mel bank: four lanes per (frame, band); every lane runs every trip so the shuffles see whole groups
  const int sub = tid & 3, total = F * n_mels;
  double lmax = 0.0;
  for (int it = 0; it * (MEL_Q / 4) < total; ++it) {
    const int item = it * (MEL_Q / 4) + (tid >> 2);
    const bool live = item < total;
    const int f2 = live ? item / n_mels : 0, m = live ? item - f2 * n_mels : 0;
    const int first = bands[3 * m], last = bands[3 * m + 1], off = bands[3 * m + 2];
    // a table that points outside the spectrum or the weights poisons the band instead of reading out of bounds
    const bool sane = first >= 0 && first <= last && last <= M + 1 && off >= 0 && (long long)off + (last - first) <= n_weights;
    double acc = 0.0;
    // eight weights in flight per trip (a run is up to ~90 bins at 80 bands: three trips, not twenty-two dependent loads); the
    // padding terms are fma(0, 0, acc) = acc, so the sum is the plain in-order one
    if (live && sane)
      for (int k0 = first + sub; k0 < last; k0 += 32) {
        double wv[8], pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + 4 * u;
          wv[u] = k < last ? weights[off + k - first] : 0.0;
          pv[u] = k < last ? pw[f2 * (M + 1) + k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = fma(wv[u], pv[u], acc);
      }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if (!sane) acc = __builtin_nan("");
    if (live && sub == 0 && frame0 + f2 < n_frames) {
      mel[(n * n_mels + m) * n_frames + frame0 + f2] = acc;
      lmax = fmax(lmax, acc);
    }
  }
  // ---- the trial's maximum
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) lmax = fmax(lmax, __shfl_xor(lmax, d));
  if ((tid & 63) == 0) wmax[tid >> 6] = lmax;
  __syncthreads();
  if (tid == 0) {
    double v = wmax[0];
#pragma unroll
    for (int w = 1; w < MEL_Q / 64; ++w) v = fmax(v, wmax[w]);
    atomicMax(reinterpret_cast<unsigned long long*>(rowmax + n), (unsigned long long)__double_as_longlong(v));
  }
}

// power_to_db(S, ref=np.max) of one trial, top_db = 80: the largest dB value of a trial is that of its maximum, ref - ref
__global__ __launch_bounds__(256) void mel_finish_kernel(const double* __restrict__ mel, const double* __restrict__ rowmax,
                                                         float* __restrict__ out, long long per_trial, long long total,
                                                         int in_db) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  double v = mel[i];
  if (in_db) {
    const double ref = 10.0 * log10(fmax(1e-10, rowmax[i / per_trial]));
    const double db = 10.0 * log10(fmax(1e-10, v)) - ref;
    const double floor_db = (ref - ref) - 80.0;
    v = db < floor_db ? floor_db : db;                       // np.maximum: NaN stays NaN
  }
  out[i] = (float)v;
}

}  // namespace tl
using namespace tl;

static int mel_log2m(int n_fft) {
  switch (n_fft) {
    case 256: return 7;
    case 512: return 8;
    case 1024: return 9;
    case 2048: return 10;
    default: return 0;
  }
}

extern "C" int tl_mel_power(const void* audio, int audio_is_f64, int64_t row_stride, const double* window, const double* tw,
                            const int32_t* bands, const double* weights, int n_weights, double* mel, double* rowmax, int N,
                            int64_t S, int n_fft, int win_length, int hop, int center, int power, int n_mels, int64_t n_frames,
                            void* stream) {
  TL_REQUIRE(audio && window && tw && bands && weights && mel && rowmax, "mel_power: null pointer");
  const int log2m = mel_log2m(n_fft);
  TL_REQUIRE(log2m, "mel_power: n_fft must be one of 256, 512, 1024, 2048 (got %d)", n_fft);
  TL_REQUIRE(win_length >= 1 && win_length <= n_fft, "mel_power: win_length must lie in [1, n_fft] (got %d)", win_length);
  TL_REQUIRE(hop >= 1, "mel_power: hop must be at least 1 (got %d)", hop);
  TL_REQUIRE(power == 1 || power == 2, "mel_power: power must be 1 or 2 (got %d)", power);
  TL_REQUIRE(n_mels >= 1 && n_mels <= 65536, "mel_power: n_mels must lie in [1, 65536] (got %d)", n_mels);
  TL_REQUIRE(center == 0 || center == 1, "mel_power: center must be 0 or 1");
  TL_REQUIRE(N >= 1 && S >= 1 && S <= (1LL << 40) && row_stride >= S, "mel_power: N and S must be at least 1 and row_stride >= S");
  TL_REQUIRE(n_weights >= 0, "mel_power: n_weights must not be negative");
  const long long padded = (long long)S + (center ? n_fft : 0);
  TL_REQUIRE(padded >= n_fft, "mel_power: S = %lld samples are shorter than n_fft = %d", (long long)S, n_fft);
  const long long want = 1 + (padded - n_fft) / hop;
  TL_REQUIRE(n_frames == want, "mel_power: n_frames = %lld disagrees with S, n_fft, hop and center (%lld)", (long long)n_frames, want);
  const int fpb = tl::MEL_PTS / (n_fft / 2);
  const long long bpt = (n_frames + fpb - 1) / fpb;
  TL_REQUIRE(bpt * N <= 0x7fffffffLL, "mel_power: too many frames for one launch");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(rowmax, 0, sizeof(double) * (size_t)N, st) != hipSuccess) {
    (void)hipGetLastError();
    tl::set_error("mel_power: clearing rowmax failed");
    return TL_ELAUNCH;
  }
  const mel_d2* w2 = reinterpret_cast<const mel_d2*>(window);
  const mel_d2* t2 = reinterpret_cast<const mel_d2*>(tw);
  dim3 grid((unsigned)(bpt * N));
#define MEL_LAUNCH(TIN, L2M)                                                                                            \
  hipLaunchKernelGGL((mel_power_kernel<TIN, L2M>), grid, dim3(MEL_Q), 0, st, audio, (long long)row_stride, (long long)S, w2, t2,  \
                     bands, weights, n_weights, mel, rowmax, (int)bpt, (long long)n_frames, hop, center, power, n_mels)
#define MEL_SIZES(TIN)                                                                                                  \
  switch (log2m) {                                                                                                      \
    case 7: MEL_LAUNCH(TIN, 7); break;                                                                                  \
    case 8: MEL_LAUNCH(TIN, 8); break;                                                                                  \
    case 9: MEL_LAUNCH(TIN, 9); break;                                                                                  \
    default: MEL_LAUNCH(TIN, 10); break;                                                                                \
  }
  if (audio_is_f64) {
    MEL_SIZES(double)
  } else {
    MEL_SIZES(float)
  }
#undef MEL_SIZES
#undef MEL_LAUNCH
  return check_launch("mel_power");
}

extern "C" int tl_mel_finish(const double* mel, const double* rowmax, float* out, int N, int n_mels, int64_t n_frames, int in_db,
                             void* stream) {
  TL_REQUIRE(mel && rowmax && out, "mel_finish: null pointer");
  TL_REQUIRE(N >= 1, "mel_finish: N must be at least 1 (got %d)", N);
  TL_REQUIRE(n_mels >= 1, "mel_finish: n_mels must be at least 1 (got %d)", n_mels);
  TL_REQUIRE(n_frames >= 1, "mel_finish: n_frames must be at least 1 (got %lld)", (long long)n_frames);
  TL_REQUIRE(in_db == 0 || in_db == 1, "mel_finish: in_db must be 0 or 1");
  const long long per = (long long)n_mels * n_frames;
  TL_REQUIRE(per / n_mels == n_frames && per <= 0x7fffffffffffLL / N, "mel_finish: output too large");
  const long long total = per * N, blocks = (total + 255) / 256;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "mel_finish: output too large for one launch");
  hipLaunchKernelGGL(mel_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mel, rowmax, out, per, total,
                     in_db);
  return check_launch("mel_finish");
}
