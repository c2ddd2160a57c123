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
//
// Every kernel of this file that transforms frames (mel_power, gl_synth, gl_analyse, welch_accum) is built from the same pieces,
// each stated once: MelFrames (the workgroup's frame set-up: LDS images, fl, j, fbase, twiddles; mel_fft and mel_unpack_bin on
// them) and mel_band_sane (the band-run check, also of mel_invert).  On the host MelArgs holds the checks the entries share
// (n_fft -> log2 M, win_length, hop, frames per workgroup, the 2^31 launch cap) and mel_dispatch picks the instantiation by size
// (mel_by_type the sample type, where the rows have one).  The windowed gather of mel_power and gl_analyse stays written out in both: as one function over a sample
// callable the compiler fused a different product of the first butterfly into its fma in gl_analyse, and bits changed.
//
// The way back (utils/audio.py mel_to_audio_batch) is further down: tl_mel_invert (mel -> linear spectrum by FISTA, the whole
// solve in LDS and registers) and Griffin-Lim as tl_gl_synth / tl_gl_analyse / tl_gl_overlap_add, whose inverse and forward
// transforms are the mel_fft below (the inverse runs it on the conjugate).
#include "tonal_common.h"
#include <math.h>
#include <type_traits>

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

// ---- the M-point transform every kernel of this file shares (the inverse runs it on the conjugate)
// the LDS image that holds the transform after the last pass
constexpr int mel_fin(int log2m) { return (log2m & 1) ? ((log2m / 2) & 1) : ((log2m / 2 - 1) & 1); }

// the thread's twiddles of every pass, requested before the first barrier: one memory latency instead of one per pass
template <int LOG2M>
struct MelTwiddles {
  mel_d2 r4[LOG2M / 2][3], r2[2];
};

template <int LOG2M>
__device__ __forceinline__ void mel_load_twiddles(const mel_d2* __restrict__ tw, int j, MelTwiddles<LOG2M>& t) {
  constexpr int M = 1 << LOG2M, NFFT = 2 * M, Q = M / 4, NS4 = LOG2M / 2, HAS2 = LOG2M & 1;
#pragma unroll
  for (int st = 1; st < NS4; ++st)
#pragma unroll
    for (int r = 1; r < 4; ++r) t.r4[st][r - 1] = tw[r * (j & ((1 << (2 * st)) - 1)) * (NFFT >> (2 * st + 2))];
  if (HAS2) {
    t.r2[0] = tw[2 * j];
    t.r2[1] = tw[2 * (j + Q)];
  }
}

// FFT_M of the frame at fbase: the thread brings the points j + r M/4 in registers (the first pass, Ns = 1, has no twiddles and
// never goes through LDS); the transform lands in natural order in image FIN of re / im; ends on a barrier
template <int LOG2M>
__device__ __forceinline__ void mel_fft(double (&xr)[4], double (&xi)[4], const MelTwiddles<LOG2M>& t, double* const (&re)[2],
                                        double* const (&im)[2], int j, int fbase) {
  constexpr int M = 1 << LOG2M, Q = M / 4, NS4 = LOG2M / 2, HAS2 = LOG2M & 1;
  double yr[4], yi[4];
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
      const mel_d2 w = t.r4[st][r - 1];                      // W_{4 Ns}^{rk} = W_nfft^{rk nfft / 4 Ns} as (cos, -sin)
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
      const mel_d2 w = t.r2[u];                              // W_M^jj
      const double tr = fma(-bi, w[1], br * w[0]), ti = fma(br, w[1], bi * w[0]);
      re[dst][mel_idx(fbase + jj)] = ar + tr;
      im[dst][mel_idx(fbase + jj)] = ai + ti;
      re[dst][mel_idx(fbase + jj + H)] = ar - tr;
      im[dst][mel_idx(fbase + jj + H)] = ai - ti;
    }
    __syncthreads();
  }
}

// bin k = 0..M of the real transform from the packed one Z: X[k] = E[k] + W_nfft^k O[k], E = (Z[k] + conj Z[M-k]) / 2,
// O = (Z[k] - conj Z[M-k]) / 2i
template <int LOG2M>
__device__ __forceinline__ void mel_unpack_bin(const double* zr, const double* zi, const mel_d2* __restrict__ tw, int fbase, int k,
                                               double& Xr, double& Xi) {
  constexpr int M = 1 << LOG2M;
  const int ka = k & (M - 1), kb = (M - k) & (M - 1);
  const double ar = zr[mel_idx(fbase + ka)], ai = zi[mel_idx(fbase + ka)];
  const double cr = zr[mel_idx(fbase + kb)], ci = zi[mel_idx(fbase + kb)];
  const double er = 0.5 * (ar + cr), ei = 0.5 * (ai - ci);
  const double orr = 0.5 * (ai + ci), oi = -0.5 * (ar - cr);
  const mel_d2 w = tw[k];
  Xr = er + fma(-oi, w[1], orr * w[0]);
  Xi = ei + fma(orr, w[1], oi * w[0]);
}

// ---- the set-up of the four frame kernels (mel_power, gl_synth, gl_analyse, welch_accum): thread tid of the MEL_Q owns the points
// j + r M/4 of frame fl of the workgroup's F = MEL_PTS / M, whose points start at fbase in the ping-pong images re[] / im[] laid
// over the kernel's own `__shared__ double lds[4 * MEL_PAD]`; the thread's twiddles are requested here.  Which frames of which
// row a workgroup holds (blockIdx) is each kernel's own business
template <int LOG2M>
struct MelFrames {
  static constexpr int M = 1 << LOG2M, F = MEL_PTS / M, Q = M / 4, FIN = mel_fin(LOG2M);
  double* re[2];
  double* im[2];
  int tid, fl, j, fbase;
  MelTwiddles<LOG2M> twd;
  __device__ __forceinline__ explicit MelFrames(double* lds)
      : re{lds, lds + 2 * MEL_PAD}, im{lds + MEL_PAD, lds + 3 * MEL_PAD}, tid(threadIdx.x), fl(tid >> (LOG2M - 2)),
        j(tid & (Q - 1)), fbase(fl * M) {}
  __device__ __forceinline__ void load_twiddles(const mel_d2* tw) { mel_load_twiddles<LOG2M>(tw, j, twd); }
  __device__ __forceinline__ void fft(double (&xr)[4], double (&xi)[4]) const { mel_fft<LOG2M>(xr, xi, twd, re, im, j, fbase); }
  __device__ __forceinline__ void unpack_bin(const mel_d2* tw, int k, double& Xr, double& Xi) const {
    mel_unpack_bin<LOG2M>(re[FIN], im[FIN], tw, fbase, k, Xr, Xi);
  }
};

// a band's run [first, last) lies within the nb bins and its weights within the table; the kernels poison a band whose run does
// not instead of reading out of bounds
__device__ __forceinline__ bool mel_band_sane(int first, int last, int off, int nb, int n_weights) {
  return first >= 0 && first <= last && last <= nb && off >= 0 && (long long)off + (last - first) <= n_weights;
}

// bands (n_mels, 3) int32: first bin, one past the last bin, offset of the band's first weight in `weights`
template <typename TIN, int LOG2M>
__global__ __launch_bounds__(MEL_Q) void mel_power_kernel(const void* __restrict__ audio, long long row_stride, long long S,
                                                          const mel_d2* __restrict__ window, const mel_d2* __restrict__ tw,
                                                          const int32_t* __restrict__ bands, const double* __restrict__ weights,
                                                          int n_weights, double* __restrict__ mel, double* __restrict__ rowmax,
                                                          int blocks_per_trial, long long n_frames, int hop, int center,
                                                          int power, int n_mels) {
  using Fr = MelFrames<LOG2M>;
  constexpr int M = Fr::M, F = Fr::F, Q = Fr::Q, FIN = Fr::FIN;
  __shared__ __attribute__((aligned(16))) double lds[4 * MEL_PAD];
  __shared__ double wmax[MEL_Q / 64];
  Fr fr(lds);
  const int tid = fr.tid, fl = fr.fl, j = fr.j;
  const long long n = blockIdx.x / blocks_per_trial;
  const long long frame0 = (long long)(blockIdx.x % blocks_per_trial) * F;
  const long long frame = frame0 + fl;
  const long long start = frame * hop - (center ? M : 0);
  const long long row = n * row_stride;

  fr.load_twiddles(tw);
  // ---- gather + window + first pass (Ns = 1, no twiddles) straight from registers
  double xr[4], xi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * Q;
    const long long s0 = start + 2 * m, s1 = s0 + 1;
    const mel_d2 w = window[m];
    xr[r] = (frame < n_frames && s0 >= 0 && s0 < S) ? mel_ld<TIN>(audio, row + s0) * w[0] : 0.0;
    xi[r] = (frame < n_frames && s1 >= 0 && s1 < S) ? mel_ld<TIN>(audio, row + s1) * w[1] : 0.0;
  }
  fr.fft(xr, xi);
  // ---- unpack to the M + 1 bins of the real transform, |X|^power into the image nobody reads any more
  double* pw = fr.re[FIN ^ 1];                               // [F][M + 1], F (M + 1) <= 1032 doubles
  for (int k = j; k <= M; k += Q) {
    double Xr, Xi;
    fr.unpack_bin(tw, k, Xr, Xi);
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
    const bool sane = mel_band_sane(first, last, off, M + 1, n_weights);
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


// ---------------------------------------------------------------------------------------------- mel -> linear spectrum
// min_{x >= 0} ||fb x - p||^2 per frame by FISTA (utils/audio.py mel_to_linear states it): 1024 / M frames per workgroup as
// above.  Per iteration r = fb z - p is a reduction per (frame, band) over the band's run, four lanes each, and the gradient
// fb^T r of a bin needs the at most two bands that cover it (bin_bands / bin_weights), so it is two multiplies per bin:
// no search, no atomics.  z, r, p, the band table and the weights stay in LDS and x in registers for the whole solve; global
// memory is read before the first iteration and written after the last, but for the iteration's momentum factor.
constexpr int INV_MAX_MELS = 256, INV_MAX_WEIGHTS = 2 * (MEL_PTS + 1), INV_BINS = 5;   // 5 * 256 threads >= 1032 bins

template <int LOG2M>
__global__ __launch_bounds__(MEL_Q) void mel_invert_kernel(const double* __restrict__ p, const int32_t* __restrict__ bands,
                                                           const double* __restrict__ weights, int n_weights,
                                                           const int32_t* __restrict__ bin_bands,
                                                           const double* __restrict__ bin_weights,
                                                           const double* __restrict__ momentum, double* __restrict__ out,
                                                           int blocks_per_trial, long long n_frames, int n_mels, int iters,
                                                           double step, int power) {
  // utils/audio.py bank_operators writes out the order of every sum and rounds every product and sum on its own; with no
  // fused multiply-add here the kernel returns the bits of mel_to_linear
#pragma clang fp contract(off)
  constexpr int M = 1 << LOG2M, F = MEL_PTS / M, NB = M + 1;
  __shared__ double zs[F * NB], rs[F * INV_MAX_MELS], ps[F * INV_MAX_MELS], ws[INV_MAX_WEIGHTS];
  __shared__ int32_t bs[3 * INV_MAX_MELS];
  const int tid = threadIdx.x, sub = tid & 3, total = F * n_mels;
  const long long n = blockIdx.x / blocks_per_trial;
  const long long frame0 = (long long)(blockIdx.x % blocks_per_trial) * F;

  for (int i = tid; i < total; i += MEL_Q) {
    const int f = i / n_mels, m = i - f * n_mels;
    ps[i] = frame0 + f < n_frames ? p[(n * n_mels + m) * n_frames + frame0 + f] : 0.0;
  }
  for (int i = tid; i < n_weights; i += MEL_Q) ws[i] = weights[i];
  // a run that leaves the spectrum or the weights is emptied here and its band comes out NaN: nothing reads out of bounds
  bool bad = false;
  for (int m = tid; m < n_mels; m += MEL_Q) {
    const int first = bands[3 * m], last = bands[3 * m + 1], off = bands[3 * m + 2];
    const bool sane = mel_band_sane(first, last, off, NB, n_weights);
    bs[3 * m] = sane ? first : 0;
    bs[3 * m + 1] = sane ? last : 0;
    bs[3 * m + 2] = sane ? off : 0;
    bad |= !sane;
  }
  // the thread's bins: flat index tid + i * 256 over (frame, bin)
  double x[INV_BINS], z[INV_BINS], gw[INV_BINS][2];
  int gb[INV_BINS][2];
#pragma unroll
  for (int i = 0; i < INV_BINS; ++i) {
    const int idx = tid + i * MEL_Q, f = idx / NB, k = idx - f * NB;
    x[i] = z[i] = 0.0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int b = idx < F * NB ? bin_bands[2 * k + u] : -1;
      gw[i][u] = b >= 0 && b < n_mels ? bin_weights[2 * k + u] : 0.0;
      gb[i][u] = b >= 0 && b < n_mels ? f * n_mels + b : 0;
      bad |= b >= n_mels;
    }
    if (idx < F * NB) zs[idx] = 0.0;
  }
  __syncthreads();

  double beta = momentum[0];
  for (int it = 0; it < iters; ++it) {
    const double beta_next = momentum[min(it + 1, iters - 1)];   // one uniform 8-byte load, a whole iteration ahead of its use
    // ---- r = fb z - p: every lane runs every trip so the shuffles see whole groups
    for (int trip = 0; trip * (MEL_Q / 4) < total; ++trip) {
      const int item = trip * (MEL_Q / 4) + (tid >> 2);
      const bool live = item < total;
      const int f = live ? item / n_mels : 0, m = live ? item - f * n_mels : 0;
      const int first = bs[3 * m], last = bs[3 * m + 1], off = bs[3 * m + 2];
      double acc = 0.0;
      if (live)
        for (int k = first + sub; k < last; k += 4) acc = acc + ws[off + k - first] * zs[f * NB + k];
      acc += __shfl_xor(acc, 1);                             // (s0 + s1) + (s2 + s3)
      acc += __shfl_xor(acc, 2);
      if (live && sub == 0) rs[item] = acc - ps[item];
    }
    __syncthreads();
    // ---- x+ = max(z - step fb^T r, 0),  z+ = x+ + beta (x+ - x)
#pragma unroll
    for (int i = 0; i < INV_BINS; ++i) {
      const int idx = tid + i * MEL_Q;
      const double g = gw[i][0] * rs[gb[i][0]] + gw[i][1] * rs[gb[i][1]];
      const double x_new = fmax(z[i] - step * g, 0.0);
      z[i] = x_new + beta * (x_new - x[i]);
      x[i] = x_new;
      if (idx < F * NB) zs[idx] = z[i];
    }
    beta = beta_next;
    __syncthreads();
  }
  bad = __syncthreads_or(bad);
#pragma unroll
  for (int i = 0; i < INV_BINS; ++i) {
    const int idx = tid + i * MEL_Q, f = idx / NB, k = idx - f * NB;
    if (idx < F * NB && frame0 + f < n_frames)
      out[(n * NB + k) * n_frames + frame0 + f] = bad ? __builtin_nan("") : (power == 2 ? sqrt(x[i]) : x[i]);
  }
}

// ---------------------------------------------------------------------------------------------- Griffin-Lim
// One iteration = gl_synth_kernel (spectrum -> windowed frames) + gl_analyse_kernel (frames -> overlap-added signal ->
// spectrum -> new phases); utils/audio.py griffinlim / istft / stft state it.  Both hold 1024 / M frames per workgroup as
// mel_power_kernel does.  The overlap-add is a gather: sample q of the signal is the sum, frame by frame in rising order as
// the host adds them, of the at most ceil(n_fft / hop) frames that cover it, over the window-square sum - no atomics, and the
// same bits on every run.

// sample q of the overlap-added signal of one trial, q counted from the start of frame 0 (the centre trim not yet applied)
template <int NFFT>
__device__ __forceinline__ double gl_sample(const double* __restrict__ fr, const double* __restrict__ wsum, long long q,
                                            long long n_frames, int hop) {
  const long long t0 = q >= NFFT ? (q - NFFT) / hop + 1 : 0, t1 = min(n_frames - 1, q / hop);
  double acc = 0.0;
  for (long long t = t0; t <= t1; ++t) acc += fr[t * NFFT + (q - t * hop)];
  const double w = wsum[q];
  return w > 1.1754943508222875e-38 ? acc / w : acc;        // istft: wsum > np.finfo(np.float32).tiny
}

// frames (N, T, n_fft) = irfft(mag * angles) * window.  The inverse real transform is the packed one run backwards:
// Z[k] = E[k] + i O[k], E = (X[k] + conj X[M-k]) / 2, O = (X[k] - conj X[M-k]) / 2 * conj W_nfft^k, z = IFFT_M(Z) =
// conj(FFT_M(conj Z)) / M, x[2m] = Re z[m], x[2m+1] = Im z[m].  mag is (N, T, M + 1), angles (T, M + 1) complex shared by all
// trials (angle_stride 0) or (N, T, M + 1)
template <int LOG2M>
__global__ __launch_bounds__(MEL_Q) void gl_synth_kernel(const double* __restrict__ mag, const mel_d2* __restrict__ angles,
                                                         long long angle_stride, const mel_d2* __restrict__ window,
                                                         const mel_d2* __restrict__ tw, mel_d2* __restrict__ frames,
                                                         int blocks_per_trial, long long n_frames) {
  using Fr = MelFrames<LOG2M>;
  constexpr int M = Fr::M, F = Fr::F, Q = Fr::Q, FIN = Fr::FIN;
  __shared__ __attribute__((aligned(16))) double lds[4 * MEL_PAD];
  Fr fr(lds);
  const int fl = fr.fl, j = fr.j, fbase = fr.fbase;
  const long long n = blockIdx.x / blocks_per_trial;
  const long long frame = (long long)(blockIdx.x % blocks_per_trial) * F + fl;
  const bool live = frame < n_frames;
  const double* mg = mag + (n * n_frames + frame) * (M + 1);
  const mel_d2* an = angles + n * angle_stride + frame * (M + 1);

  fr.load_twiddles(tw);
  double xr[4], xi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * Q, mc = M - m;
    double ar = 0.0, ai = 0.0, cr = 0.0, ci = 0.0;
    if (live) {
      const double ma = mg[m], mb = mg[mc];
      const mel_d2 pa = an[m], pb = an[mc];
      ar = ma * pa[0];
      ai = m == 0 ? 0.0 : ma * pa[1];                        // irfft reads the real parts of X[0] and X[M] only
      cr = mb * pb[0];
      ci = m == 0 ? 0.0 : mb * pb[1];
    }
    const double er = 0.5 * (ar + cr), ei = 0.5 * (ai - ci), dr = 0.5 * (ar - cr), di = 0.5 * (ai + ci);
    const mel_d2 w = tw[m];                                  // (cos, -sin): conj W^m = (w0, -w1)
    const double orr = fma(di, w[1], dr * w[0]), oi = fma(-dr, w[1], di * w[0]);
    xr[r] = er - oi;                                         // conj Z, Z = E + i O
    xi[r] = -(ei + orr);
  }
  fr.fft(xr, xi);
  if (live) {
    constexpr double inv_m = 1.0 / M;
    mel_d2* dst = frames + (n * n_frames + frame) * M;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = j + r * Q;
      const mel_d2 w = window[m];
      mel_d2 v;
      v[0] = fr.re[FIN][mel_idx(fbase + m)] * inv_m * w[0];
      v[1] = -fr.im[FIN][mel_idx(fbase + m)] * inv_m * w[1];
      dst[m] = v;
    }
  }
}

// frames -> signal (samples [M, M + length) of the overlap-add) -> stft with n_fft / 2 zeros on both sides -> rebuilt;
// angles = rebuilt - coef * tprev (rebuilt alone on the first iteration), angles /= |angles| + 1e-16, tprev = rebuilt.
// Frames from re_frames = 1 + length / hop on are past the rebuilt signal: zero
template <int LOG2M>
__global__ __launch_bounds__(MEL_Q) void gl_analyse_kernel(const double* __restrict__ frames, const double* __restrict__ wsum,
                                                           const mel_d2* __restrict__ window, const mel_d2* __restrict__ tw,
                                                           mel_d2* __restrict__ angles, mel_d2* __restrict__ tprev,
                                                           int blocks_per_trial, long long n_frames, long long length,
                                                           long long re_frames, int hop, double coef, int first) {
  using Fr = MelFrames<LOG2M>;
  constexpr int M = Fr::M, NFFT = 2 * M, F = Fr::F, Q = Fr::Q;
  __shared__ __attribute__((aligned(16))) double lds[4 * MEL_PAD];
  Fr fr(lds);
  const int j = fr.j;
  const long long n = blockIdx.x / blocks_per_trial;
  const long long frame = (long long)(blockIdx.x % blocks_per_trial) * F + fr.fl;
  const bool live = frame < n_frames && frame < re_frames;
  const long long start = frame * hop - M;
  const double* trial = frames + n * n_frames * NFFT;

  fr.load_twiddles(tw);
  double xr[4], xi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * Q;
    const long long s0 = start + 2 * m, s1 = s0 + 1;
    const mel_d2 w = window[m];
    xr[r] = (live && s0 >= 0 && s0 < length) ? gl_sample<NFFT>(trial, wsum, s0 + M, n_frames, hop) * w[0] : 0.0;
    xi[r] = (live && s1 >= 0 && s1 < length) ? gl_sample<NFFT>(trial, wsum, s1 + M, n_frames, hop) * w[1] : 0.0;
  }
  fr.fft(xr, xi);
  if (frame < n_frames)
    for (int k = j; k <= M; k += Q) {
      double Xr, Xi;
      fr.unpack_bin(tw, k, Xr, Xi);
      if (k == 0 || k == M) Xi = 0.0;                        // exactly real, as rfft returns them
      const long long idx = (n * n_frames + frame) * (M + 1) + k;
      double ar = Xr, ai = Xi;
      if (!first) {
        const mel_d2 pv = tprev[idx];
        ar = Xr - coef * pv[0];
        ai = Xi - coef * pv[1];
      }
      const double d = sqrt(ar * ar + ai * ai) + 1e-16;
      mel_d2 a, x;
      a[0] = ar / d;
      a[1] = ai / d;
      x[0] = Xr;
      x[1] = Xi;
      angles[idx] = a;
      tprev[idx] = x;
    }
}

// out (N, length) = samples [M, M + length) of the overlap-add of frames (N, T, n_fft)
template <int NFFT>
__global__ __launch_bounds__(256) void gl_overlap_add_kernel(const double* __restrict__ frames, const double* __restrict__ wsum,
                                                             double* __restrict__ out, long long n_frames, long long length,
                                                             int hop) {
  const long long s = blockIdx.x * 256LL + threadIdx.x, n = blockIdx.y;
  if (s < length) out[n * length + s] = gl_sample<NFFT>(frames + n * n_frames * NFFT, wsum, s + NFFT / 2, n_frames, hop);
}

// ---------------------------------------------------------------------------------------------- Welch PSD
// scipy.signal.welch(axis=1, average='mean') of every row of a (C, T) recording (utils/diagnostics.py welch_psd): the
// segments of one channel are the frames of mel_power_kernel, but nothing is written per frame - a workgroup owns one
// (channel, slab of consecutive segments), walks the slab F segments a trip and keeps |X|^2 of its own bins in registers.
//   gather   the thread's eight samples 2m, 2m + 1 (m = j + r M/4) straight from the row; offsets >= nperseg (the zero padding
//            up to n_fft) and offsets past T are never read;
//   detrend  constant: the mean of the segment's nperseg live samples is a reduction over the frame's Q = M/4 threads - an
//            xor butterfly where a frame fits a wave (Q <= 64), else per-wave sums through LDS added in wave order; every
//            thread of the frame ends with the same bits.  The raw samples stay in registers;
//   FFT      mel_fft, then the next trip's samples are requested, then mel_unpack_bin and acc += Xr^2 + Xi^2;
//   slab     after the last trip the F lanes are added through LDS in lane order -> work (C, n_slabs, M + 1).
// No atomics; the order of every sum is fixed by thread and slab numbers, so two runs give the same bits.
template <typename TIN, int Q>
__device__ __forceinline__ void welch_gather(const void* __restrict__ x, long long row, long long T, long long seg,
                                             long long seg_end, int step, int nperseg, int j, double (&raw)[8]) {
  const bool live = seg < seg_end;
  const long long start = seg * step;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 2 * (j + r * Q);
    raw[2 * r] = (live && o < nperseg && start + o < T) ? mel_ld<TIN>(x, row + start + o) : 0.0;
    raw[2 * r + 1] = (live && o + 1 < nperseg && start + o + 1 < T) ? mel_ld<TIN>(x, row + start + o + 1) : 0.0;
  }
}

template <typename TIN, int LOG2M>
__global__ __launch_bounds__(MEL_Q) void welch_accum_kernel(const void* __restrict__ x, long long row_stride, long long T,
                                                            const mel_d2* __restrict__ window, const mel_d2* __restrict__ tw,
                                                            double* __restrict__ work, long long n_seg, int trips, int nperseg,
                                                            int step, int detrend) {
  using Fr = MelFrames<LOG2M>;
  constexpr int M = Fr::M, F = Fr::F, Q = Fr::Q, NB = M + 1;
  __shared__ __attribute__((aligned(16))) double lds[4 * MEL_PAD];
  __shared__ double wsum[MEL_Q / 64];
  Fr fr(lds);
  const int tid = fr.tid, fl = fr.fl, j = fr.j;
  const long long row = (long long)blockIdx.y * row_stride;
  const long long seg0 = (long long)blockIdx.x * trips * F;             // an absent slab (seg0 >= n_seg) writes zeros
  const long long seg_end = seg0 + (long long)trips * F < n_seg ? seg0 + (long long)trips * F : n_seg;

  fr.load_twiddles(tw);
  mel_d2 wv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) wv[r] = window[j + r * Q];
  double raw[8], acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  welch_gather<TIN, Q>(x, row, T, seg0 + fl, seg_end, step, nperseg, j, raw);
  for (int trip = 0; trip < trips; ++trip) {
    double mean = 0.0;
    if (detrend) {                                                       // block-uniform
      double s = ((raw[0] + raw[1]) + (raw[2] + raw[3])) + ((raw[4] + raw[5]) + (raw[6] + raw[7]));
      if (Q <= 64) {
#pragma unroll
        for (int d = Q / 2; d >= 1; d >>= 1) s += __shfl_xor(s, d);
      } else {
        constexpr int WPF = Q > 64 ? Q / 64 : 1;                         // waves per frame
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
        if ((tid & 63) == 0) wsum[tid >> 6] = s;
        __syncthreads();                                                 // the next write is behind the barriers of mel_fft
        const int w0 = (tid >> 6) / WPF * WPF;
        s = wsum[w0];
#pragma unroll
        for (int u = 1; u < WPF; ++u) s += wsum[w0 + u];
      }
      mean = s / (double)nperseg;
    }
    double xr[4], xi[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 2 * (j + r * Q);
      xr[r] = o < nperseg ? (raw[2 * r] - mean) * wv[r][0] : 0.0;
      xi[r] = o + 1 < nperseg ? (raw[2 * r + 1] - mean) * wv[r][1] : 0.0;
    }
    fr.fft(xr, xi);
    // the next trip's samples are on their way while this one is unpacked (past the last trip: seg >= seg_end, no load)
    welch_gather<TIN, Q>(x, row, T, seg0 + (long long)(trip + 1) * F + fl, trip + 1 < trips ? seg_end : 0, step, nperseg, j, raw);
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int k = j + u * Q;
      if (k <= M) {                                                      // u = 4: bin M, thread j = 0 only
        double Xr, Xi;
        fr.unpack_bin(tw, k, Xr, Xi);
        acc[u] += fma(Xr, Xr, Xi * Xi);
      }
    }
    __syncthreads();                                                     // the next first pass overwrites image 0
  }
  // ---- the F frame lanes, in lane order
  double* pw = lds;                                                      // [F][M + 1], F (M + 1) <= 1032 doubles
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    const int k = j + u * Q;
    if (k <= M) pw[fl * NB + k] = acc[u];
  }
  __syncthreads();
  double* dst = work + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * NB;
  for (int k = tid; k < NB; k += MEL_Q) {
    double s = pw[k];
#pragma unroll
    for (int f = 1; f < F; ++f) s += pw[f * NB + k];
    dst[k] = s;
  }
}

// psd[c][k] = (sum of the slabs in order) / n_seg * scale, doubled but at DC and Nyquist (one-sided)
__global__ __launch_bounds__(256) void welch_finish_kernel(const double* __restrict__ work, double* __restrict__ psd, long long total,
                                                           int nb, int n_slabs, double n_seg, double scale) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i >= total) return;
  const long long c = i / nb;
  const int k = (int)(i - c * nb);
  const double* p = work + c * n_slabs * nb + k;
  double s = p[0];
  for (int sl = 1; sl < n_slabs; ++sl) s += p[(long long)sl * nb];
  s = s / n_seg * scale;
  psd[i] = (k == 0 || k == nb - 1) ? s : 2.0 * s;
}


}  // namespace tl
using namespace tl;

static const mel_d2* mel_d2_ptr(const double* p) { return reinterpret_cast<const mel_d2*>(p); }
static mel_d2* mel_d2_ptr(double* p) { return reinterpret_cast<mel_d2*>(p); }

// ---- what the entries check in common, each fault refused in `who`'s name with the one text it has
struct MelArgs {
  const char* who;
  int log2m = 0, fpb = 0;                                    // log2 (n_fft / 2); frames per workgroup
  long long bpt = 0;                                         // workgroups per trial

  int size(int n_fft) {
    log2m = n_fft == 256 ? 7 : n_fft == 512 ? 8 : n_fft == 1024 ? 9 : n_fft == 2048 ? 10 : 0;
    TL_REQUIRE(log2m, "%s: n_fft must be one of 256, 512, 1024, 2048 (got %d)", who, n_fft);
    fpb = tl::MEL_PTS / (n_fft / 2);
    return TL_OK;
  }
  int window(int n_fft, int win_length, int hop) const {
    TL_REQUIRE(win_length >= 1 && win_length <= n_fft, "%s: win_length must lie in [1, n_fft] (got %d)", who, win_length);
    TL_REQUIRE(hop >= 1, "%s: hop must be at least 1 (got %d)", who, hop);
    return TL_OK;
  }
  // after size(): N trials of n_frames frames in one launch.  The 2^40 test is the inverse entries'; mel_power has bounded S
  // and checked n_frames against it before it comes here, and at 2^40 frames the launch cap refuses in the same words
  int frames(int N, int64_t n_frames) {
    bpt = ((long long)n_frames + fpb - 1) / fpb;
    TL_REQUIRE(n_frames <= (1LL << 40) && bpt * N <= 0x7fffffffLL, "%s: too many frames for one launch", who);
    return TL_OK;
  }
  int inverse(int N, int n_fft, int64_t n_frames) {          // what the four entries of the way back begin with
    if (size(n_fft)) return TL_EINVAL;
    TL_REQUIRE(N >= 1 && n_frames >= 1, "%s: N and n_frames must be at least 1 (got %d, %lld)", who, N, (long long)n_frames);
    return frames(N, n_frames);
  }
  // what istft keeps of n_frames frames after the centre trim: at most n_fft / 2 + hop (n_frames - 1) samples
  int signal(int n_fft, int win_length, int hop, int64_t n_frames, int64_t length) const {
    if (window(n_fft, win_length, hop)) return TL_EINVAL;
    TL_REQUIRE(hop <= win_length, "%s: hop = %d > win_length = %d leaves gaps in the window-square sum", who, hop, win_length);
    const long long most = n_fft / 2 + (long long)hop * (n_frames - 1);
    TL_REQUIRE(length >= 1 && length <= most, "%s: length = %lld disagrees with n_frames = %lld, n_fft and hop (1 .. %lld)", who,
               (long long)length, (long long)n_frames, most);
    return TL_OK;
  }
};

// launch(size) with log2m as a std::integral_constant; the two entries that read float32 or float64 rows pick the sample type
// inside their launch with mel_by_type
template <typename Launch>
static void mel_dispatch(int log2m, Launch launch) {
  switch (log2m) {
    case 7: launch(std::integral_constant<int, 7>()); break;
    case 8: launch(std::integral_constant<int, 8>()); break;
    case 9: launch(std::integral_constant<int, 9>()); break;
    default: launch(std::integral_constant<int, 10>()); break;
  }
}

template <typename Launch>
static void mel_by_type(int is_f64, Launch launch) {
  is_f64 ? launch(double()) : launch(float());
}

extern "C" int tl_mel_power(const void* audio, int audio_is_f64, int64_t row_stride, const double* window, const double* tw,
                            const int32_t* bands, const double* weights, int n_weights, double* mel, double* rowmax, int N,
                            int64_t S, int n_fft, int win_length, int hop, int center, int power, int n_mels, int64_t n_frames,
                            void* stream) {
  TL_REQUIRE(audio && window && tw && bands && weights && mel && rowmax, "mel_power: null pointer");
  MelArgs a{"mel_power"};
  if (a.size(n_fft) || a.window(n_fft, win_length, hop)) return TL_EINVAL;
  TL_REQUIRE(power == 1 || power == 2, "mel_power: power must be 1 or 2 (got %d)", power);
  TL_REQUIRE(n_mels >= 1 && n_mels <= 65536, "mel_power: n_mels must lie in [1, 65536] (got %d)", n_mels);
  TL_REQUIRE(center == 0 || center == 1, "mel_power: center must be 0 or 1");
  TL_REQUIRE(N >= 1 && S >= 1 && S <= (1LL << 40) && row_stride >= S, "mel_power: N and S must be at least 1 and row_stride >= S");
  TL_REQUIRE(n_weights >= 0, "mel_power: n_weights must not be negative");
  const long long padded = (long long)S + (center ? n_fft : 0);
  TL_REQUIRE(padded >= n_fft, "mel_power: S = %lld samples are shorter than n_fft = %d", (long long)S, n_fft);
  const long long want = 1 + (padded - n_fft) / hop;
  TL_REQUIRE(n_frames == want, "mel_power: n_frames = %lld disagrees with S, n_fft, hop and center (%lld)", (long long)n_frames, want);
  if (a.frames(N, n_frames)) return TL_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(rowmax, 0, sizeof(double) * (size_t)N, st) != hipSuccess) {
    (void)hipGetLastError();
    tl::set_error("mel_power: clearing rowmax failed");
    return TL_ELAUNCH;
  }
  mel_dispatch(a.log2m, [&](auto size) {
    mel_by_type(audio_is_f64, [&](auto sample) {
      hipLaunchKernelGGL((mel_power_kernel<decltype(sample), decltype(size)::value>), dim3((unsigned)(a.bpt * N)), dim3(MEL_Q), 0,
                         st, audio, (long long)row_stride, (long long)S, mel_d2_ptr(window), mel_d2_ptr(tw), bands, weights,
                         n_weights, mel, rowmax, (int)a.bpt, (long long)n_frames, hop, center, power, n_mels);
    });
  });
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

extern "C" int tl_welch_psd(const void* x, int x_is_f64, int64_t row_stride, const double* window, const double* tw, double* work,
                            int64_t work_elems, double* psd, int C, int64_t T, int n_fft, int nperseg, int noverlap, int detrend,
                            double scale, int64_t n_seg, int n_slabs, void* stream) {
  TL_REQUIRE(x && window && tw && work && psd, "welch_psd: null pointer");
  MelArgs a{"welch_psd"};
  if (a.size(n_fft)) return TL_EINVAL;
  TL_REQUIRE(nperseg >= 2 && nperseg <= n_fft, "welch_psd: nperseg must lie in [2, n_fft] (got %d)", nperseg);
  TL_REQUIRE(noverlap >= 0 && nperseg - noverlap >= 1, "welch_psd: step = nperseg - noverlap must be at least 1 and noverlap "
             "not negative (got nperseg %d, noverlap %d)", nperseg, noverlap);
  TL_REQUIRE(detrend == 0 || detrend == 1, "welch_psd: detrend must be 0 (none) or 1 (constant)");
  TL_REQUIRE(C >= 1 && C <= 65535, "welch_psd: C must lie in [1, 65535] (got %d)", C);
  TL_REQUIRE(T >= nperseg && T <= (1LL << 40) && row_stride >= T, "welch_psd: T = %lld must lie in [nperseg, 2^40] and "
             "row_stride >= T", (long long)T);
  const int step = nperseg - noverlap;
  const long long want = ((long long)T - noverlap) / step;
  TL_REQUIRE(n_seg == want, "welch_psd: n_seg = %lld disagrees with T, nperseg and noverlap (%lld)", (long long)n_seg, want);
  const int fpb = a.fpb, nb = n_fft / 2 + 1;
  const long long all_trips = (want + fpb - 1) / fpb;
  TL_REQUIRE(n_slabs >= 1 && n_slabs <= 0x7fffffff / nb, "welch_psd: n_slabs must be at least 1 (got %d)", n_slabs);
  TL_REQUIRE(work_elems >= (int64_t)C * n_slabs * nb, "welch_psd: the workspace holds %lld doubles, C * n_slabs * (n_fft / 2 + 1) "
             "= %lld are needed", (long long)work_elems, (long long)((int64_t)C * n_slabs * nb));
  const long long trips = (all_trips + n_slabs - 1) / n_slabs;
  TL_REQUIRE(trips <= 0x7fffffffLL / fpb, "welch_psd: too many segments per slab");
  hipStream_t st = (hipStream_t)stream;
  mel_dispatch(a.log2m, [&](auto size) {
    mel_by_type(x_is_f64, [&](auto sample) {
      hipLaunchKernelGGL((welch_accum_kernel<decltype(sample), decltype(size)::value>), dim3((unsigned)n_slabs, (unsigned)C),
                         dim3(MEL_Q), 0, st, x, (long long)row_stride, (long long)T, mel_d2_ptr(window), mel_d2_ptr(tw), work,
                         (long long)n_seg, (int)trips, nperseg, step, detrend);
    });
  });
  const long long total = (long long)C * nb;
  hipLaunchKernelGGL(welch_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, work, psd, total, nb, n_slabs,
                     (double)n_seg, scale);
  return check_launch("welch_psd");
}

extern "C" int tl_mel_invert(const double* mel_power, const int32_t* bands, const double* weights, int n_weights,
                             const int32_t* bin_bands, const double* bin_weights, const double* momentum, double* out, int N,
                             int n_fft, int n_mels, int64_t n_frames, int nnls_iter, double step, int power, void* stream) {
  TL_REQUIRE(mel_power && bands && weights && bin_bands && bin_weights && momentum && out, "mel_invert: null pointer");
  MelArgs a{"mel_invert"};
  if (a.inverse(N, n_fft, n_frames)) return TL_EINVAL;
  TL_REQUIRE(n_mels >= 1 && n_mels <= tl::INV_MAX_MELS, "mel_invert: n_mels must lie in [1, %d] (got %d)", tl::INV_MAX_MELS, n_mels);
  TL_REQUIRE(n_weights >= 0 && n_weights <= n_fft + 2,
             "mel_invert: n_weights must lie in [0, n_fft + 2]: at most two bands cover a bin (got %d)", n_weights);
  TL_REQUIRE(nnls_iter >= 1, "mel_invert: nnls_iter must be at least 1 (got %d)", nnls_iter);
  TL_REQUIRE(step > 0.0 && step < INFINITY, "mel_invert: step must be positive and finite");
  TL_REQUIRE(power == 1 || power == 2, "mel_invert: power must be 1 or 2 (got %d)", power);
  mel_dispatch(a.log2m, [&](auto size) {
    hipLaunchKernelGGL((mel_invert_kernel<decltype(size)::value>), dim3((unsigned)(a.bpt * N)), dim3(MEL_Q), 0, (hipStream_t)stream,
                       mel_power, bands, weights, n_weights, bin_bands, bin_weights, momentum, out, (int)a.bpt,
                       (long long)n_frames, n_mels, nnls_iter, step, power);
  });
  return check_launch("mel_invert");
}

extern "C" int tl_gl_synth(const double* mag, const double* angles, int angles_shared, const double* window, const double* tw,
                           double* frames, int N, int n_fft, int64_t n_frames, void* stream) {
  TL_REQUIRE(mag && angles && window && tw && frames, "gl_synth: null pointer");
  MelArgs a{"gl_synth"};
  if (a.inverse(N, n_fft, n_frames)) return TL_EINVAL;
  TL_REQUIRE(angles_shared == 0 || angles_shared == 1, "gl_synth: angles_shared must be 0 or 1");
  const long long stride = angles_shared ? 0 : (long long)n_frames * (n_fft / 2 + 1);
  mel_dispatch(a.log2m, [&](auto size) {
    hipLaunchKernelGGL((gl_synth_kernel<decltype(size)::value>), dim3((unsigned)(a.bpt * N)), dim3(MEL_Q), 0, (hipStream_t)stream,
                       mag, mel_d2_ptr(angles), stride, mel_d2_ptr(window), mel_d2_ptr(tw), mel_d2_ptr(frames), (int)a.bpt,
                       (long long)n_frames);
  });
  return check_launch("gl_synth");
}

extern "C" int tl_gl_analyse(const double* frames, const double* wsum, const double* window, const double* tw, double* angles,
                             double* tprev, int N, int n_fft, int win_length, int hop, int64_t n_frames, int64_t length,
                             double momentum, int first, void* stream) {
  TL_REQUIRE(frames && wsum && window && tw && angles && tprev, "gl_analyse: null pointer");
  MelArgs a{"gl_analyse"};
  if (a.inverse(N, n_fft, n_frames) || a.signal(n_fft, win_length, hop, n_frames, length)) return TL_EINVAL;
  TL_REQUIRE(momentum >= 0.0 && momentum < INFINITY, "gl_analyse: momentum must be finite and not negative");
  TL_REQUIRE(first == 0 || first == 1, "gl_analyse: first must be 0 or 1");
  const double coef = momentum / (1.0 + momentum);
  const long long re_frames = 1 + length / hop;
  mel_dispatch(a.log2m, [&](auto size) {
    hipLaunchKernelGGL((gl_analyse_kernel<decltype(size)::value>), dim3((unsigned)(a.bpt * N)), dim3(MEL_Q), 0, (hipStream_t)stream,
                       frames, wsum, mel_d2_ptr(window), mel_d2_ptr(tw), mel_d2_ptr(angles), mel_d2_ptr(tprev), (int)a.bpt,
                       (long long)n_frames, (long long)length, re_frames, hop, coef, first);
  });
  return check_launch("gl_analyse");
}

extern "C" int tl_gl_overlap_add(const double* frames, const double* wsum, double* out, int N, int n_fft, int win_length, int hop,
                                 int64_t n_frames, int64_t length, void* stream) {
  TL_REQUIRE(frames && wsum && out, "gl_overlap_add: null pointer");
  MelArgs a{"gl_overlap_add"};
  if (a.inverse(N, n_fft, n_frames) || a.signal(n_fft, win_length, hop, n_frames, length)) return TL_EINVAL;
  TL_REQUIRE(N <= 65535, "gl_overlap_add: at most 65535 trials per launch (got %d)", N);
  const long long blocks = ((long long)length + 255) / 256;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "gl_overlap_add: length too large for one launch");
  mel_dispatch(a.log2m, [&](auto size) {
    hipLaunchKernelGGL((gl_overlap_add_kernel<(2 << decltype(size)::value)>), dim3((unsigned)blocks, (unsigned)N), dim3(256), 0,
                       (hipStream_t)stream, frames, wsum, out, (long long)n_frames, (long long)length, hop);
  });
  return check_launch("gl_overlap_add");
}
