// Channel selection: one-way ANOVA at every (channel, timepoint) column, and the longest significant run per channel
// (reference channel_selection/active.py:58-76, discriminative.py:171-180, utils.py:4-30 - scipy.stats.f_oneway in a Python
// loop over channels).  An (n_samples, C, T) recording is C*T independent columns, each reduced over the samples: one
// streaming pass.  All arithmetic is fp64; see include/tonal_hip.h for the contracts.
#include "tonal_common.h"
#include <math.h>

namespace tl {

// ------------------------------------------------------------------------------------------
// per-group column sums.  A lane owns a column (loads coalesce along cols) and walks the group's index list, which is
// wave-uniform, MOM_UNROLL rows in flight.  One group per launch keeps one accumulator pair in registers (an accumulator
// array indexed by label would be a dynamic register index, i.e. scratch).  The sums are taken of x - shift[col]: scipy
// subtracts the overall mean before it squares, and raw sums of a recording with mean 1e4 and unit variance lose 8 digits
// in ss_within.
// ------------------------------------------------------------------------------------------
#define MOM_UNROLL 8

template <typename T>
__global__ __launch_bounds__(256) void group_moments_kernel(const T* __restrict__ x, const T* __restrict__ shift,
                                                            const int32_t* __restrict__ idx, int n, long long n_rows,
                                                            long long cols, int chunk, double* __restrict__ sum,
                                                            double* __restrict__ sumsq) {
  const long long col = blockIdx.x * 256LL + threadIdx.x;
  if (col >= cols) return;
  const int s = blockIdx.y;
  const int i0 = s * chunk;
  const int i1 = i0 + chunk < n ? i0 + chunk : n;
  const double sh = (double)shift[col];
  const double bad = __builtin_nan("");
  double a = 0.0, q = 0.0;
  int i = i0;
  for (; i + MOM_UNROLL <= i1; i += MOM_UNROLL) {
    double v[MOM_UNROLL];
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      const long long r = idx[i + u];
      v[u] = (r >= 0 && r < n_rows) ? (double)x[r * cols + col] : bad;       // the test is wave-uniform
    }
#pragma unroll
    for (int u = 0; u < MOM_UNROLL; ++u) {
      const double d = v[u] - sh;
      a += d;
      q = fma(d, d, q);
    }
  }
  for (; i < i1; ++i) {
    const long long r = idx[i];
    const double d = ((r >= 0 && r < n_rows) ? (double)x[r * cols + col] : bad) - sh;
    a += d;
    q = fma(d, d, q);
  }
  sum[(long long)s * cols + col] = a;
  sumsq[(long long)s * cols + col] = q;
}

// ------------------------------------------------------------------------------------------
// F survival function: p = I_x(a, b), a = dfw/2, b = dfb/2, x = dfw/(dfw + dfb F), y = 1 - x formed by the caller as
// dfb F/(dfw + dfb F) (1.0 - x would lose y below 1e-16 and every digit of a p close to 1).
// ------------------------------------------------------------------------------------------
// Stirling's correction lgamma(z) - ((z - 1/2) log z - z + log(2 pi)/2); the truncation is below 1e-16 for z >= 16
__host__ __device__ inline double stirling_corr(double z) {
  const double r = 1.0 / z, r2 = r * r;
  return r * (1.0 / 12 - r2 * (1.0 / 360 - r2 * (1.0 / 1260 - r2 * (1.0 / 1680 - r2 * (1.0 / 1188 - r2 * (691.0 / 360360))))));
}
// log B(a, b) = lgamma(a) + lgamma(b) - lgamma(a + b).  With dfw/2 in the hundreds the three terms are near 1e3 and cancel
// to a few units, which would cost three digits of p; for max(a, b) >= 16 the difference lgamma(hi) - lgamma(hi + lo) is
// taken analytically from Stirling's series instead.
__host__ __device__ inline double log_beta(double a, double b) {
  const double lo = a < b ? a : b, hi = a < b ? b : a;
  if (hi < 16.0) return lgamma(a) + lgamma(b) - lgamma(a + b);
  return lgamma(lo) - (hi - 0.5) * log1p(lo / hi) - lo * log(hi + lo) + lo + (stirling_corr(hi) - stirling_corr(hi + lo));
}
// continued fraction of the incomplete beta function, modified Lentz; converges fast for x < (a + 1)/(a + b + 2)
__host__ __device__ inline double beta_cf(double a, double b, double x) {
  const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 2000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 2e-16) break;
  }
  return h;
}
// the prefactor x^a y^b / B(a, b) is built in log space: a p of 1e-80 and below keeps its relative accuracy
__host__ __device__ inline double f_survival(double F, double dfb, double dfw) {
  if (F != F || dfb <= 0.0 || dfw <= 0.0 || F < 0.0) return __builtin_nan("");
  const double den = dfw + dfb * F;
  if (den > 1.7e308) return 0.0;                  // F = inf (ssw = 0 under ssb > 0), or dfb F overflows
  if (F == 0.0) return 1.0;
  const double a = 0.5 * dfw, b = 0.5 * dfb, x = dfw / den, y = dfb * F / den;
  const double pre = exp(a * log(x) + b * log(y) - log_beta(a, b));
  if (x < (a + 1.0) / (a + b + 2.0)) return pre * beta_cf(a, b, x) / a;
  return 1.0 - pre * beta_cf(b, a, y) / b;
}

struct AnovaCounts { int32_t n[64]; };

// sum / sumsq (k, splits, cols): the split slabs of a group are added here.  With S_g, Q_g the shifted sums of group g,
// ssb = sum_g n_g (S_g/n_g - S/N)^2 and ssw = sum_g (Q_g - S_g^2/n_g) - both invariant under the shift; the group sums are
// read twice rather than kept in an array indexed by g (a dynamic register index).
__device__ __forceinline__ void group_ss(const double* __restrict__ sum, const double* __restrict__ sumsq, const AnovaCounts& cnt,
                                         int k, int splits, long long cols, long long N, long long col, double& ssb, double& ssw) {
  double S = 0.0;
  for (int g = 0; g < k; ++g)
    for (int s = 0; s < splits; ++s) S += sum[((long long)g * splits + s) * cols + col];
  const double mean = S / (double)N;
  ssb = 0.0;
  ssw = 0.0;
  for (int g = 0; g < k; ++g) {
    double Sg = 0.0, Qg = 0.0;
    for (int s = 0; s < splits; ++s) {
      Sg += sum[((long long)g * splits + s) * cols + col];
      Qg += sumsq[((long long)g * splits + s) * cols + col];
    }
    const double ng = (double)cnt.n[g], mg = Sg / ng, d = mg - mean;
    ssb = fma(ng * d, d, ssb);
    ssw += Qg - Sg * mg;
  }
}

// a statistic of group_finalize_kernel: (stat, pv) of a column from its (ssb, ssw), left as they come in (NaN) where undefined
struct AnovaF {
  static __device__ __forceinline__ void eval(double ssb, double ssw, long long N, int k, double& stat, double& pv) {
    const double dfb = (double)(k - 1), dfw = (double)(N - k);
    if (N > k) {
      stat = (ssb / dfb) / (ssw / dfw);
      pv = f_survival(stat, dfb, dfw);
    }
  }
};

// ------------------------------------------------------------------------------------------
// Kruskal-Wallis: with its tie correction H is the ANOVA decomposition of the midranks, H = (N - 1) ssb / (ssb + ssw), and
// p = Q(a, x), a = (k - 1)/2, x = H/2, the regularised upper incomplete gamma function (the chi-square tail): the series of
// P below a + 1, the continued fraction of Q (modified Lentz) from there on.  The prefactor x^a e^-x / Gamma(a) is the product
// of exp(-x), whose argument is exact, and exp(a log x - lgamma(a)), whose argument stays below 210 for a <= 31.5 and every
// x that exp(-x) survives: a p of 1e-100 carries the rounding of an argument of a few units, not of one near -230.
// ------------------------------------------------------------------------------------------
__host__ __device__ inline double chi2_survival(double H, double df) {
  if (H != H || df <= 0.0 || H < 0.0) return __builtin_nan("");
  if (H == 0.0) return 1.0;
  const double a = 0.5 * df, x = 0.5 * H;
  const double pre = exp(-x) * exp(fma(a, log(x), -lgamma(a)));
  if (x < a + 1.0) {
    double ap = a, del = 1.0 / a, s = del;
    for (int n = 1; n <= 2000; ++n) {
      ap += 1.0;
      del *= x / ap;
      s += del;
      if (del < s * 1e-17) break;
    }
    return 1.0 - pre * s;
  }
  const double tiny = 1e-300;
  double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
  for (int i = 1; i <= 2000; ++i) {
    const double an = -i * (i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < tiny) d = tiny;
    c = b + an / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) < 2e-16) break;
  }
  return pre * h;
}

// (ssb, ssw) taken of the midranks; a column of identical values has sst = 0: NaN
struct KruskalH {
  static __device__ __forceinline__ void eval(double ssb, double ssw, long long N, int k, double& stat, double& pv) {
    const double sst = ssb + ssw;
    if (sst > 0.0) {                                             // false for NaN
      stat = (double)(N - 1) * ssb / sst;
      pv = chi2_survival(stat, (double)(k - 1));
    }
  }
};

// one column per lane: Stat (AnovaF or KruskalH) turns the column's (ssb, ssw) into the statistic and its p
template <typename Stat>
__global__ __launch_bounds__(256) void group_finalize_kernel(const double* __restrict__ sum, const double* __restrict__ sumsq,
                                                       AnovaCounts cnt, int k, int splits, long long cols, long long N,
                                                       double* __restrict__ stat, double* __restrict__ p) {
  const long long col = blockIdx.x * 256LL + threadIdx.x;
  if (col >= cols) return;
  double ssb, ssw;
  group_ss(sum, sumsq, cnt, k, splits, cols, N, col, ssb, ssw);
  double s = __builtin_nan(""), pv = __builtin_nan("");
  Stat::eval(ssb, ssw, N, k, s, pv);
  stat[col] = s;
  p[col] = pv;
}

// ------------------------------------------------------------------------------------------
// midranks down the sample axis: ranks[i][col] = scipy.stats.rankdata(column col, method='average')[i].  A block owns tw
// consecutive columns and all N samples.  Every value becomes an unsigned key in the order of the values (-0.0 made +0.0 first,
// so the two tie; the sign bit flipped for a positive value, every bit for a negative one) next to its sample index; a NaN and
// the padding up to npad = the next power of two take the largest key.  The image is [position][column]: a row load is
// coalesced along the columns, and a pass of the bitonic network (rank_pass: up to three steps) touches, per lane group, tw
// consecutive words per position at ANY stride of the network - no power-of-two stride between the lanes of a group, the bank
// of a word is its column (tw >= 32; a narrower tile puts 32 / tw positions into a lane group: conflict-free while the threads
// of the group own neighbouring positions, up to 32 / tw-way in the last pass of a stage, whose threads own neighbouring runs
// of 2^M positions - the narrow tiles measured faster all the same, see below).  The
// network is not stable and need not be: tied keys get one rank.  Sorted position s then finds the ends [lo, hi) of its tie run
// (a neighbour compare; a binary search only inside a run) and writes (lo + hi + 1) / 2 to the row of its index.  A column that
// holds a NaN has the largest key at position N - 1 and gets NaN in every row.
// tw is the largest power of two <= RK_MAX_TW with npad * tw * (key bytes + 2) <= RK_TILE_BYTES, and 1 where one column takes
// more (up to RK_LDS_BYTES): four blocks of 512 threads a CU where the tile allows it - at 480 samples tw = 8 for both dtypes,
// 24 and 40 KiB.  Measured there against 80 KiB tiles and 256 or 1024 threads (float32 / float64 ms): 256 threads, 80 KiB
// 1.09 / 1.78; 1024, 80 KiB 0.92 / 1.72; 512, 80 KiB 0.86 / 1.30; 256, 40 KiB 0.90 / 1.22; 512, 40 KiB 0.89 / 1.20.
// ------------------------------------------------------------------------------------------
#define RK_THREADS 512
#define RK_MAX_N 8192                 // 8192 float64 keys with their indices are RK_LDS_BYTES at tw = 1
#define RK_LDS_BYTES 81920            // most LDS of a block: half of the 160 KiB of a CU
#define RK_TILE_BYTES 40960           // a tile of more than one column stays within a quarter
#define RK_MAX_TW 64
#define RK_LOADS 8

__device__ __forceinline__ uint32_t rank_key(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.f) v = 0.f;
  const uint32_t u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ uint64_t rank_key(double v) {
  if (v != v) return ~0ull;
  if (v == 0.0) v = 0.0;
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
}

// M consecutive steps of stage k, strides j, j/2, .., low = j >> (M - 1), in one pass over LDS: the 2^M positions
// base + a low (the M stride bits of the position free, the rest taken from g) only exchange among themselves in those steps,
// so a thread holds them in registers; one read and one write per element and one barrier where the steps alone take M.
// The direction bit k lies above every stride of its stage: one direction per thread.
template <typename K, int M>
__device__ __forceinline__ void rank_pass(K* keys, uint16_t* idx, int npad, int ltw, int k, int j, int tid) {
  constexpr int E = 1 << M;
  const int low = j >> (M - 1), st = low << ltw, items = (npad >> M) << ltw;
  for (int e = tid; e < items; e += RK_THREADS) {
    const int g = e >> ltw, base = ((g & ~(low - 1)) << M) | (g & (low - 1));
    const int a0 = (base << ltw) + (e & ((1 << ltw) - 1));
    const bool up = (base & k) == 0;
    K kv[E];
    uint16_t iv[E];
#pragma unroll
    for (int a = 0; a < E; ++a) {
      kv[a] = keys[a0 + a * st];
      iv[a] = idx[a0 + a * st];
    }
#pragma unroll
    for (int t = M - 1; t >= 0; --t)
#pragma unroll
      for (int a = 0; a < E; ++a)
        if (!(a & (1 << t))) {
          const int b = a | (1 << t);
          const bool sw = (kv[a] > kv[b]) == up;
          const K ka = kv[a];
          const uint16_t ia = iv[a];
          kv[a] = sw ? kv[b] : ka;
          kv[b] = sw ? ka : kv[b];
          iv[a] = sw ? iv[b] : ia;
          iv[b] = sw ? ia : iv[b];
        }
#pragma unroll
    for (int a = 0; a < E; ++a) {
      keys[a0 + a * st] = kv[a];
      idx[a0 + a * st] = iv[a];
    }
  }
}

template <typename T, typename K>
__global__ __launch_bounds__(RK_THREADS) void rank_columns_kernel(const T* __restrict__ x0, long long n0, const T* __restrict__ x1,
                                                                  int N, long long cols, int npad, int ltw,
                                                                  float* __restrict__ ranks) {
  extern __shared__ unsigned long long rk_lds[];
  const int tw = 1 << ltw, cmask = tw - 1, tid = threadIdx.x;
  K* keys = reinterpret_cast<K*>(rk_lds);                      // [npad][tw]
  uint16_t* idx = reinterpret_cast<uint16_t*>(keys + npad * tw);
  const long long col0 = (long long)blockIdx.x * tw;
  const K pad = ~(K)0;
  for (int e0 = tid; e0 < npad * tw; e0 += RK_LOADS * RK_THREADS) {       // RK_LOADS row segments in flight per thread
    T v[RK_LOADS];
#pragma unroll
    for (int u = 0; u < RK_LOADS; ++u) {
      const int e = e0 + u * RK_THREADS;
      const long long i = e >> ltw, col = col0 + (e & cmask);
      v[u] = (T)__builtin_nanf("");                                        // padding takes the key of a NaN
      if (i < N && col < cols) v[u] = i < n0 ? x0[i * cols + col] : x1[(i - n0) * cols + col];
    }
#pragma unroll
    for (int u = 0; u < RK_LOADS; ++u) {
      const int e = e0 + u * RK_THREADS;
      if (e < npad * tw) {
        keys[e] = rank_key(v[u]);
        idx[e] = (uint16_t)(e >> ltw);
      }
    }
  }
  for (int k = 2, steps = 1; k <= npad; k <<= 1, ++steps)      // stage k: steps of stride k/2 .. 1, three to a pass
    for (int j = k >> 1, left = steps; left > 0;) {
      __syncthreads();
      if (left >= 3) {
        rank_pass<K, 3>(keys, idx, npad, ltw, k, j, tid);
        j >>= 3;
        left -= 3;
      } else if (left == 2) {
        rank_pass<K, 2>(keys, idx, npad, ltw, k, j, tid);
        j >>= 2;
        left -= 2;
      } else {
        rank_pass<K, 1>(keys, idx, npad, ltw, k, j, tid);
        j >>= 1;
        left -= 1;
      }
    }
  __syncthreads();
  for (int e = tid; e < (N << ltw); e += RK_THREADS) {
    const int c = e & cmask, s = e >> ltw;
    const long long col = col0 + c;
    if (col >= cols) continue;
    if (keys[((N - 1) << ltw) + c] == pad) {                   // a NaN in the column: positions below N may hold padding
      ranks[(long long)s * cols + col] = __builtin_nanf("");
      continue;
    }
    const K key = keys[e];
    int lo = s, hi = s + 1;
    if (s > 0 && keys[e - tw] == key) {                        // the first position of the run, in [0, s)
      int a = 0, b = s - 1;
      while (a < b) {
        const int m = (a + b) >> 1;
        if (keys[(m << ltw) + c] < key) a = m + 1; else b = m;
      }
      lo = a;
    }
    if (hi < N && keys[e + tw] == key) {                       // one past its last position, in (s + 1, N]
      int a = s + 2, b = N;
      while (a < b) {
        const int m = (a + b) >> 1;
        if (keys[(m << ltw) + c] <= key) a = m + 1; else b = m;
      }
      hi = a;
    }
    ranks[(long long)idx[e] * cols + col] = 0.5f * (float)(lo + hi + 1);
  }
}

// ------------------------------------------------------------------------------------------
// longest run of p < thr per row: one wave per row, lane l owns elements [l chunk, (l + 1) chunk) and reduces them to
// (pre, suf, best, len) = (run at the start, run at the end, longest run, elements); segments combine associatively and an
// empty segment (all zero) is the identity, so lanes beyond T need no special case.
// The lanes of a wave read with a stride of chunk doubles - uncoalesced, and fine for what this serves: p is (C, T) of a few hundred
// timepoints, about a megabyte, read once.  For rows of many thousands of points walk the row 64 elements at a time (coalesced) with a
// per-lane carry instead of copying this layout.
// ------------------------------------------------------------------------------------------
struct RunSeg { int pre, suf, best, len, cnt; };

__device__ __forceinline__ RunSeg run_combine(const RunSeg& L, const RunSeg& R) {
  RunSeg o;
  o.pre = L.pre == L.len ? L.len + R.pre : L.pre;
  o.suf = R.suf == R.len ? R.len + L.suf : R.suf;
  const int mid = L.suf + R.pre;
  o.best = L.best > R.best ? L.best : R.best;
  o.best = o.best > mid ? o.best : mid;
  o.len = L.len + R.len;
  o.cnt = L.cnt + R.cnt;
  return o;
}

__global__ __launch_bounds__(256) void max_run_below_kernel(const double* __restrict__ p, int C, long long T, double thr,
                                                            int32_t* __restrict__ count, int32_t* __restrict__ maxrun) {
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (row >= C) return;                                        // whole waves leave: the shuffles below see 64 live lanes
  const long long chunk = (T + 63) / 64;
  long long t0 = lane * chunk, t1 = t0 + chunk;
  if (t0 > T) t0 = T;
  if (t1 > T) t1 = T;
  const double* pr = p + row * T;
  RunSeg s = {0, 0, 0, (int)(t1 - t0), 0};
  int run = 0;
  bool open = true;                                            // no element at or above thr seen yet
  for (long long t = t0; t < t1; ++t) {
    if (pr[t] < thr) {                                         // false for NaN
      ++run;
      ++s.cnt;
      if (run > s.best) s.best = run;
    } else {
      if (open) { s.pre = run; open = false; }
      run = 0;
    }
  }
  if (open) s.pre = run;
  s.suf = run;
  for (int d = 1; d < 64; d <<= 1) {
    RunSeg r;
    r.pre = __shfl_down(s.pre, d, 64);
    r.suf = __shfl_down(s.suf, d, 64);
    r.best = __shfl_down(s.best, d, 64);
    r.len = __shfl_down(s.len, d, 64);
    r.cnt = __shfl_down(s.cnt, d, 64);
    s = run_combine(s, r);                                     // exact in the lanes that are multiples of 2d; lane 0 at the end
  }
  if (lane == 0) {
    count[row] = s.cnt;
    maxrun[row] = s.best;
  }
}

// ------------------------------------------------------------------------------------------
// label-permutation test: where does the ANOVA of a RELABELLED recording pass the threshold?  A relabelling keeps the group
// sizes, so the total sum of squares and the degrees of freedom are those of the observed labelling and p < alpha' is
// sum_g S_g^2 / n_g > tau[col] (tau = theta sst + total^2 / N, formed once by the caller; S_g the shifted column sum of group
// g).  The group sums of all relabellings are one fp64 product, onehot (P k x N) times (x - shift) (N x cols), on
// v_mfma_f64_16x16x4_f64:
//   A (16 rows x 4 samples): row r = q + 4 reg is (relabelling q + 4 (reg / GR), group gbase + reg % GR) of the tile, so the GR
//     groups of a relabelling are registers of ONE lane in the f64 C/D layout (row = (lane >> 4) + 4 reg, col = lane & 15) and
//     sum_g S_g^2 / n_g needs no lane movement.  GR = 2 for two groups (8 relabellings per tile), else 4; more than GR groups
//     are further passes over the samples, each adding its groups' share.  The 0/1 operand is formed in registers from label
//     bytes held in LDS - a compare, never an index: a label >= k matches no row.
//   B (4 samples x 16 columns): the samples widened and shifted, staged through LDS from coalesced row loads, PX_KC samples a
//     stage; the next stage's loads are in flight while the MFMAs of this one run.
// A wave owns PX_MT x PX_NT tiles (every B value feeds PX_MT MFMAs, every A value PX_NT), a block 4 waves on the same columns.
// ------------------------------------------------------------------------------------------
#define PX_KC 32                 // samples per LDS stage
#define PX_CB 64                 // columns per block = 16 PX_NT
#define PX_LD 80                 // row stride of the staged samples in doubles: rows s and s + 1 fall into different bank halves
#define PX_MT 4
#define PX_NT 4

typedef double f64x4 __attribute__((ext_vector_type(4)));
struct PermWeights { double inv_n[64]; };

template <typename T, int GR>
__global__ __launch_bounds__(256) void perm_exceed_kernel(const T* __restrict__ x0, long long n0, const T* __restrict__ x1,
                                                          long long N, long long cols, const T* __restrict__ shift,
                                                          const uint8_t* __restrict__ labels, int P, int k, PermWeights wts,
                                                          const double* __restrict__ tau, uint8_t* __restrict__ exceed) {
  constexpr int PT = 16 / GR;                                  // relabellings per 16-row tile
  constexpr int PW = PX_MT * PT;                               // per wave
  constexpr int PB = 4 * PW;                                   // per block
  constexpr int LPT = PB * PX_KC / 256;                        // label bytes a thread stages
  constexpr int XPT = PX_KC * PX_CB / 256;                     // samples a thread stages
  __shared__ double xs[PX_KC * PX_LD];
  __shared__ unsigned long long ls[PB * PX_KC / 8];            // [relabelling][sample & 3][sample >> 2] bytes
  uint8_t* lsb = reinterpret_cast<uint8_t*>(ls);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npb = (P + PB - 1) / PB;
  const int pbase = (int)(blockIdx.x % (unsigned)npb) * PB;    // relabelling blocks of one column block are neighbours in the grid
  const long long col0 = (long long)(blockIdx.x / (unsigned)npb) * PX_CB;
  const int sc = tid & 63, sr = tid >> 6;                      // staged column, first staged row
  const long long scol = col0 + sc;
  const bool col_ok = scol < cols;
  const double sh = col_ok ? (double)shift[scol] : 0.0;
  const int arow = lane & 15, kq = lane >> 4;                  // A row of this lane, its sample within a 4-sample step
  const int a_rel = (arow & 3) + 4 * ((arow >> 2) / GR), a_grp = (arow >> 2) % GR;

  // staging addresses without a multiply in the loop: row i of the samples lies cols * i past (i < n0 ? x0 : x1 - n0 cols), the
  // label of relabelling p and sample i at labels + p N + i; xo / lo are those offsets for the stage being fetched
  const long long xstep = 4 * cols, x1_back = n0 * cols, lstep = 8 * N;
  const int lp0 = pbase + (tid >> 5), ls0 = tid & 31;
  T xr[XPT];
  uint8_t lr[LPT];
  auto fetch = [&](long long i0, long long xo, long long lo) {
#pragma unroll
    for (int j = 0; j < XPT; ++j) {
      const long long i = i0 + sr + 4 * j, o = xo + j * xstep;
      T v = (T)0;
      if (col_ok && i < N) v = *(i < n0 ? x0 + o : x1 + (o - x1_back));
      xr[j] = v;
    }
    const bool s_ok = i0 + ls0 < N;
#pragma unroll
    for (int j = 0; j < LPT; ++j) lr[j] = (s_ok && lp0 + 8 * j < P) ? labels[lo + j * lstep] : (uint8_t)255;
  };

  double stat[PX_MT][PX_NT][4 / GR];
#pragma unroll
  for (int m = 0; m < PX_MT; ++m)
#pragma unroll
    for (int n = 0; n < PX_NT; ++n)
#pragma unroll
      for (int j = 0; j < 4 / GR; ++j) stat[m][n][j] = 0.0;

  for (int gbase = 0; gbase < k; gbase += GR) {
    const unsigned long long gsel = gbase + a_grp < k ? (unsigned long long)(gbase + a_grp) : 0x100ull;   // 0x100: no byte equals it
    f64x4 acc[PX_MT][PX_NT];
#pragma unroll
    for (int m = 0; m < PX_MT; ++m)
#pragma unroll
      for (int n = 0; n < PX_NT; ++n) acc[m][n] = (f64x4){0.0, 0.0, 0.0, 0.0};
    long long xo = (long long)sr * cols + scol, lo = (long long)lp0 * N + ls0;
    fetch(0, xo, lo);
    for (long long i0 = 0; i0 < N; i0 += PX_KC) {
      __syncthreads();                                         // the previous stage has been read by every wave
#pragma unroll
      for (int j = 0; j < XPT; ++j) {
        const int r = sr + 4 * j;
        xs[r * PX_LD + sc] = (col_ok && i0 + r < N) ? (double)xr[j] - sh : 0.0;
      }
#pragma unroll
      for (int j = 0; j < LPT; ++j) {
        const int e = tid + 256 * j, s = e & 31;
        lsb[(e >> 5) * PX_KC + (s & 3) * 8 + (s >> 2)] = lr[j];
      }
      __syncthreads();
      xo += PX_KC * cols;
      lo += PX_KC;
      if (i0 + PX_KC < N) fetch(i0 + PX_KC, xo, lo);
      unsigned long long lw[PX_MT];                            // byte kk: the label of sample i0 + 4 kk + kq
#pragma unroll
      for (int m = 0; m < PX_MT; ++m) lw[m] = ls[(wave * PW + m * PT + a_rel) * (PX_KC / 8) + kq];
      double b[2][PX_NT];                                      // the next step's B values are read while this step's MFMAs run
#pragma unroll
      for (int n = 0; n < PX_NT; ++n) b[0][n] = xs[kq * PX_LD + n * 16 + arow];
#pragma unroll
      for (int kk = 0; kk < PX_KC / 4; ++kk) {
        if (kk + 1 < PX_KC / 4) {
#pragma unroll
          for (int n = 0; n < PX_NT; ++n) b[(kk + 1) & 1][n] = xs[(4 * (kk + 1) + kq) * PX_LD + n * 16 + arow];
        }
#pragma unroll
        for (int m = 0; m < PX_MT; ++m) {
          const double a = ((lw[m] >> (8 * kk)) & 0xffull) == gsel ? 1.0 : 0.0;
#pragma unroll
          for (int n = 0; n < PX_NT; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[kk & 1][n], acc[m][n], 0, 0, 0);
        }
      }
    }
    // C/D of the f64 form: register reg of lane l is row (l >> 4) + 4 reg, column l & 15
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int g = gbase + reg % GR;
      if (g < k) {
        const double w = wts.inv_n[g];
#pragma unroll
        for (int m = 0; m < PX_MT; ++m)
#pragma unroll
          for (int n = 0; n < PX_NT; ++n) stat[m][n][reg / GR] = fma(acc[m][n][reg] * acc[m][n][reg], w, stat[m][n][reg / GR]);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < PX_NT; ++n) {
    const long long c = col0 + n * 16 + arow;
    if (c >= cols) continue;
    const double t = tau[c];
#pragma unroll
    for (int m = 0; m < PX_MT; ++m)
#pragma unroll
      for (int j = 0; j < 4 / GR; ++j) {
        const int p = pbase + wave * PW + m * PT + kq + 4 * j;
        if (p < P) exceed[(long long)p * cols + c] = stat[m][n][j] > t ? 1 : 0;        // false for NaN
      }
  }
}

// longest run of set cells per row of a byte mask: one wave per row, 64 cells a step (coalesced); the step's cells are one
// ballot word, reduced to a RunSeg with bit operations (the same in every lane) and appended to the row's segment
__global__ __launch_bounds__(256) void perm_runs_kernel(const uint8_t* __restrict__ mask, long long rows, long long T,
                                                        int32_t* __restrict__ maxrun) {
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * 4LL + (threadIdx.x >> 6);
  if (row >= rows) return;                                     // whole waves leave
  const uint8_t* mr = mask + row * T;
  RunSeg s = {0, 0, 0, 0, 0};
  for (long long t0 = 0; t0 < T; t0 += 64) {
    const long long t = t0 + lane;
    const unsigned long long w = __ballot(t < T && mr[t] != 0);
    const int len = T - t0 < 64 ? (int)(T - t0) : 64;
    const unsigned long long nw = ~w, nwl = ~(w << (64 - len));   // cells past len are clear: nwl != 0 whenever len < 64
    RunSeg r;
    r.len = len;
    r.cnt = __popcll(w);
    r.pre = nw ? __ffsll((long long)nw) - 1 : 64;
    r.suf = nwl ? __clzll((long long)nwl) : 64;
    r.best = 0;
    for (unsigned long long v = w; v; v &= v << 1) ++r.best;
    s = run_combine(s, r);
  }
  if (lane == 0) maxrun[row] = s.best;
}

}  // namespace tl
using namespace tl;

extern "C" int tl_group_moments(const void* x, int is_f64, int64_t n_rows, int64_t cols, const int32_t* idx, int n,
                                const void* shift, int splits, double* sum, double* sumsq, void* stream) {
  TL_REQUIRE(x && idx && shift && sum && sumsq, "group_moments: null pointer");
  TL_REQUIRE(n >= 1 && n_rows >= 1 && cols >= 1, "group_moments: n, n_rows and cols must be at least 1");
  TL_REQUIRE(splits >= 1 && splits <= 1024, "group_moments: splits must lie in [1, 1024]");
  const long long blocks = (cols + 255) / 256;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "group_moments: too many columns");
  const int chunk = (n + splits - 1) / splits;
  dim3 grid((unsigned)blocks, (unsigned)splits);
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    hipLaunchKernelGGL((group_moments_kernel<double>), grid, dim3(256), 0, st, (const double*)x, (const double*)shift, idx, n,
                       (long long)n_rows, (long long)cols, chunk, sum, sumsq);
  else
    hipLaunchKernelGGL((group_moments_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (const float*)shift, idx, n,
                       (long long)n_rows, (long long)cols, chunk, sum, sumsq);
  return check_launch("group_moments");
}

template <typename Stat>
static int finalize(const char* name, const double* sum, const double* sumsq, const int32_t* counts, int k, int splits,
                    int64_t cols, double* stat, double* p, void* stream) {
  TL_REQUIRE(sum && sumsq && counts && stat && p, "%s: null pointer", name);
  TL_REQUIRE(k >= 2 && k <= 64, "%s: the number of groups k must lie in [2, 64]", name);
  TL_REQUIRE(cols >= 1, "%s: cols must be at least 1", name);
  TL_REQUIRE(splits >= 1 && splits <= 1024, "%s: splits must lie in [1, 1024]", name);
  const long long blocks = (cols + 255) / 256;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "%s: too many columns", name);
  AnovaCounts cnt = {};
  long long N = 0;
  for (int g = 0; g < k; ++g) {
    TL_REQUIRE(counts[g] >= 1, "%s: every group needs at least one sample", name);
    cnt.n[g] = counts[g];
    N += counts[g];
  }
  hipLaunchKernelGGL((group_finalize_kernel<Stat>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, sum, sumsq, cnt, k, splits,
                     (long long)cols, N, stat, p);
  return check_launch(name);
}

extern "C" int tl_anova_finalize(const double* sum, const double* sumsq, const int32_t* counts, int k, int splits, int64_t cols,
                                 double* F, double* p, void* stream) {
  return finalize<AnovaF>("anova_finalize", sum, sumsq, counts, k, splits, cols, F, p, stream);
}

extern "C" int tl_kruskal_finalize(const double* sum, const double* sumsq, const int32_t* counts, int k, int splits, int64_t cols,
                                   double* H, double* p, void* stream) {
  return finalize<KruskalH>("kruskal_finalize", sum, sumsq, counts, k, splits, cols, H, p, stream);
}

extern "C" int tl_rank_columns(const void* x0, int64_t n0, const void* x1, int64_t n1, int is_f64, int64_t cols, float* ranks,
                               void* stream) {
  TL_REQUIRE(x0 && ranks, "rank_columns: null pointer");
  TL_REQUIRE(n0 >= 1 && n1 >= 0 && (x1 || n1 == 0), "rank_columns: n0 must be at least 1, and n1 zero unless x1 is given");
  TL_REQUIRE(cols >= 1, "rank_columns: cols must be at least 1");
  TL_REQUIRE(n0 <= RK_MAX_N && n1 <= RK_MAX_N && n0 + n1 <= RK_MAX_N, "rank_columns: at most %d samples n0 + n1 (got %lld and %lld)",
             RK_MAX_N, (long long)n0, (long long)n1);
  const int N = (int)(n0 + n1);
  int npad = 2, ltw = 0;
  while (npad < N) npad <<= 1;
  const size_t per = (size_t)npad * (is_f64 ? 10 : 6);         // bytes of one column: keys and 16-bit sample indices
  while ((1 << ltw) < RK_MAX_TW && (per << (ltw + 1)) <= RK_TILE_BYTES) ++ltw;
  const long long blocks = (cols + (1 << ltw) - 1) >> ltw;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "rank_columns: too many columns");
  const size_t lds = per << ltw;
  const void* fn = is_f64 ? reinterpret_cast<const void*>(rank_columns_kernel<double, uint64_t>)
                          : reinterpret_cast<const void*>(rank_columns_kernel<float, uint32_t>);
  if (lds > 64 * 1024) {      // more than 64 KB of the CU's 160 KB: raise the per-block limit once
    static thread_local int raised_on[2] = {-1, -1};
    int devid = 0;
    (void)hipGetDevice(&devid);
    if (raised_on[is_f64 != 0] != devid) {
      hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, RK_LDS_BYTES);
      if (e != hipSuccess) {
        set_error("rank_columns: cannot raise the dynamic LDS limit for %d samples: %s", N, hipGetErrorString(e));
        return TL_ELAUNCH;
      }
      raised_on[is_f64 != 0] = devid;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (is_f64)
    hipLaunchKernelGGL((rank_columns_kernel<double, uint64_t>), dim3((unsigned)blocks), dim3(RK_THREADS), lds, st, (const double*)x0,
                       (long long)n0, (const double*)x1, N, (long long)cols, npad, ltw, ranks);
  else
    hipLaunchKernelGGL((rank_columns_kernel<float, uint32_t>), dim3((unsigned)blocks), dim3(RK_THREADS), lds, st, (const float*)x0,
                       (long long)n0, (const float*)x1, N, (long long)cols, npad, ltw, ranks);
  return check_launch("rank_columns");
}

extern "C" int tl_max_run_below(const double* p, int C, int64_t T, double thr, int32_t* count, int32_t* maxrun, void* stream) {
  TL_REQUIRE(p && count && maxrun, "max_run_below: null pointer");
  TL_REQUIRE(C >= 1 && T >= 1 && T <= 0x7fffffffLL, "max_run_below: C and T must be at least 1");
  hipLaunchKernelGGL(max_run_below_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, C, (long long)T, thr,
                     count, maxrun);
  return check_launch("max_run_below");
}

extern "C" int tl_perm_exceed(const void* x0, int64_t n0, const void* x1, int64_t n1, int is_f64, int64_t cols, const void* shift,
                              const uint8_t* labels, int P, const int32_t* counts, int k, const double* tau, uint8_t* exceed,
                              void* stream) {
  TL_REQUIRE(x0 && shift && labels && counts && tau && exceed, "perm_exceed: null pointer");
  TL_REQUIRE(n0 >= 1 && n1 >= 0 && (x1 || n1 == 0), "perm_exceed: n0 must be at least 1, and n1 zero unless x1 is given");
  TL_REQUIRE(cols >= 1 && P >= 1, "perm_exceed: cols and P must be at least 1");
  TL_REQUIRE(k >= 2 && k <= 64, "perm_exceed: the number of groups k must lie in [2, 64]");
  const long long N = (long long)n0 + n1;
  TL_REQUIRE(n0 <= 0x7fffffffLL && n1 <= 0x7fffffffLL && N <= 0x7fffffffLL, "perm_exceed: too many samples");
  PermWeights w = {};
  long long total = 0;
  for (int g = 0; g < k; ++g) {
    TL_REQUIRE(counts[g] >= 1, "perm_exceed: every group needs at least one sample");
    w.inv_n[g] = 1.0 / (double)counts[g];
    total += counts[g];
  }
  TL_REQUIRE(total == N, "perm_exceed: the group sizes must add up to n0 + n1 (got %lld and %lld)", total, N);
  const int pb = 4 * PX_MT * (k == 2 ? 8 : 4);                 // relabellings per block
  const long long blocks = ((cols + PX_CB - 1) / PX_CB) * (((long long)P + pb - 1) / pb);
  TL_REQUIRE(blocks <= 0x7fffffffLL, "perm_exceed: too many blocks (P times cols too large for one launch)");
  hipStream_t st = (hipStream_t)stream;
#define TL_PERM_LAUNCH(T, GR)                                                                                                   \
  hipLaunchKernelGGL((perm_exceed_kernel<T, GR>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x0, (long long)n0,       \
                     (const T*)x1, N, (long long)cols, (const T*)shift, labels, P, k, w, tau, exceed)
  if (is_f64) {
    if (k == 2) TL_PERM_LAUNCH(double, 2); else TL_PERM_LAUNCH(double, 4);
  } else {
    if (k == 2) TL_PERM_LAUNCH(float, 2); else TL_PERM_LAUNCH(float, 4);
  }
#undef TL_PERM_LAUNCH
  return check_launch("perm_exceed");
}

extern "C" int tl_perm_runs(const uint8_t* mask, int64_t rows, int64_t T, int32_t* maxrun, void* stream) {
  TL_REQUIRE(mask && maxrun, "perm_runs: null pointer");
  TL_REQUIRE(rows >= 1 && T >= 1 && T <= 0x7fffffffLL, "perm_runs: rows and T must be at least 1");
  const long long blocks = (rows + 3) / 4;
  TL_REQUIRE(blocks <= 0x7fffffffLL, "perm_runs: too many rows");
  hipLaunchKernelGGL(perm_runs_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mask, (long long)rows,
                     (long long)T, maxrun);
  return check_launch("perm_runs");
}
