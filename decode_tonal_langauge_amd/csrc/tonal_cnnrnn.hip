// Training kernels of CNNRNNClassifier (reference models/deep_classifiers.py:158-343 under the loop of
// models/classifier_trainer.py:72-89) that the shared conv / GEMM / head kernels do not cover (gfx950):
//   lstm_train_step_kernel   one LSTM step that KEEPS h, c and the activated gates (sibling of lstm_step_fused_kernel)
//   lstm_bptt_step_kernel    one BPTT step: dh = dgates_{t+1} . W_hh on the matrix cores, the cell backward in the epilogue
//   pool3_fwd / pool3_bwd    MaxPool2d((3,1)) + Dropout behind the un-pooled 256-channel stage, straight into / out of the
//                            second LSTM's input matrix (the reference's raw view, :309-315)
//   conv1_dgrad_kernel       input gradient of the C_in = 1 first stage (block 2 reads the first LSTM's output)
// No atomics anywhere: every sum has one owner and a fixed order, the same inputs give the same bits.
#include "tonal_common.h"
#include <math.h>

namespace tl {

constexpr int LT_NKS = 8;        // K slices of a step's recurrent product, one wave each

// ------------------------------------------------------------------------------------------
// Forward step.  Tiling of the inference kernel: a workgroup owns 32 batch rows x 8 hidden units = 32 gate columns of the
// unit-major recurrent weight wp (row 4 u + g), 8 interleaved K slices (one per wave) summed through LDS by the cell
// epilogue; thread tid < 256 owns the cell (row tid / 8, unit tid % 8).  What differs: h_in / h_out are rows t - 1 / t of the
// kept series hs (no ping-pong), c is read from cs[t - 1] and written to cs[t], and the activated gates go to act[t]
// (gate-major columns g * H + u, the layout of dgates and of torch's weights).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void lstm_train_step_kernel(const float* __restrict__ xp, long long xp_row_stride,
                                                                 const float* __restrict__ wp, const float* __restrict__ h_in,
                                                                 float* __restrict__ h_out, const float* __restrict__ c_in,
                                                                 float* __restrict__ c_out, float* __restrict__ act, int B, int H,
                                                                 int first) {
  __shared__ __attribute__((aligned(16))) float red[LT_NKS * 32 * 32];
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  const int lr = lane & 31, kh = lane >> 5;
  const int row0 = blockIdx.y * 32;
  const int u0 = blockIdx.x * 8;
  const int rloc = tid >> 3, ucell = tid & 7;
  const bool cell = tid < 256 && row0 + rloc < B;
  float xg[4] = {0.f, 0.f, 0.f, 0.f}, cprev = 0.f;
  if (cell) {
    const float* x = xp + (long long)(row0 + rloc) * xp_row_stride + (u0 + ucell);
#pragma unroll
    for (int g = 0; g < 4; ++g) xg[g] = x[(long long)g * H];
    if (!first) cprev = c_in[(long long)(row0 + rloc) * H + u0 + ucell];
  }
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  if (!first) {
    int row = row0 + lr;
    row = row < B ? row : B - 1;                         // clamped rows are never written
    const float* ap = h_in + (long long)row * H + 4 * kh;
    const float* bp = wp + (long long)(4 * u0 + lr) * H + 4 * kh;
    const int nchunk = H >> 3;                           // host-checked: H % 8 == 0
    for (int kc = ks; kc < nchunk; kc += LT_NKS) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ap + kc * 8);
      const f32x4 b = *reinterpret_cast<const f32x4*>(bp + kc * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
    }
  }
  float* mine = red + ks * 1024;                         // [32 rows][32 gate columns]
#pragma unroll
  for (int e = 0; e < 16; ++e) mine[((e & 3) + 8 * (e >> 2) + 4 * kh) * 32 + lr] = acc[e];
  __syncthreads();
  if (cell) {
    f32x4 pre = {0.f, 0.f, 0.f, 0.f};
    if (!first) {
#pragma unroll
      for (int z = 0; z < LT_NKS; ++z) pre += *reinterpret_cast<const f32x4*>(red + z * 1024 + rloc * 32 + 4 * ucell);
    }
    const float ig = sigmoidf_(pre[0] + xg[0]), fg = sigmoidf_(pre[1] + xg[1]), gg = tanhf(pre[2] + xg[2]),
                og = sigmoidf_(pre[3] + xg[3]);
    const long long i = (long long)(row0 + rloc) * H + u0 + ucell;
    const float cn = fg * cprev + ig * gg;               // cprev = 0 on the first step
    c_out[i] = cn;
    h_out[i] = og * tanhf(cn);
    float* a = act + (long long)(row0 + rloc) * 4 * H + u0 + ucell;
    a[0] = ig;
    a[H] = fg;
    a[2LL * H] = gg;
    a[3LL * H] = og;
  }
}

// ------------------------------------------------------------------------------------------
// BPTT step t.  A workgroup owns 32 batch rows x 32 hidden units: dh[row][u] = sum_n dgates_{t+1}[row][n] whT[u][n] over the
// K = 4 H gate rows (whT = W_hh^T, row u contiguous over n: a tile's 32 units are the MFMA columns), 8 interleaved K slices,
// one per wave, summed through LDS.  Epilogue: thread tid owns the cells (row tid / 32, unit tid % 32) and (16 + tid / 32,
// tid % 32) - consecutive lanes, consecutive units - reads the unit's four stored gates, c_t, c_{t-1}, adds dh_last on the
// last step, carries dc in place and writes dgates[t] (and its transposed copy, column t * B + row).
// A pad unit (zero weights, zero dh_last column) has c = 0, dh = 0, dc = 0: every product below is exactly 0.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void lstm_bptt_step_kernel(const float* __restrict__ dg_next, const float* __restrict__ whT,
                                                                const float* __restrict__ dh_last, const float* __restrict__ act,
                                                                const float* __restrict__ c, const float* __restrict__ c_prev,
                                                                float* __restrict__ dc, float* __restrict__ dgates,
                                                                float* __restrict__ dgates_t, long long ldt, int B, int H) {
  __shared__ __attribute__((aligned(16))) float red[LT_NKS * 32 * 32];
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  const int lr = lane & 31, kh = lane >> 5;
  const int row0 = blockIdx.y * 32;
  const int u0 = blockIdx.x * 32;
  const long long K = 4LL * H;
  if (dg_next != nullptr) {                              // (grid-uniform: null on the last step, whose dh is dh_last alone)
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    int row = row0 + lr, unit = u0 + lr;
    row = row < B ? row : B - 1;                         // clamped rows / units are never written
    unit = unit < H ? unit : H - 1;
    const float* ap = dg_next + (long long)row * K + 4 * kh;
    const float* bp = whT + (long long)unit * K + 4 * kh;
    const int nchunk = H >> 1;                           // 4 H / 8
    for (int kc = ks; kc < nchunk; kc += LT_NKS) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ap + kc * 8);
      const f32x4 b = *reinterpret_cast<const f32x4*>(bp + kc * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
    }
    float* mine = red + ks * 1024;                       // [32 rows][32 units]
#pragma unroll
    for (int e = 0; e < 16; ++e) mine[((e & 3) + 8 * (e >> 2) + 4 * kh) * 32 + lr] = acc[e];
    __syncthreads();
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int rloc = (tid >> 5) + 16 * half, ul = tid & 31;
    const int row = row0 + rloc, u = u0 + ul;
    if (row >= B || u >= H) continue;
    const long long i = (long long)row * H + u;
    float dht = dh_last != nullptr ? dh_last[i] : 0.f;
    if (dg_next != nullptr) {
      float s = 0.f;
#pragma unroll
      for (int z = 0; z < LT_NKS; ++z) s += red[z * 1024 + rloc * 32 + ul];
      dht += s;
    }
    const long long ab = (long long)row * K + u;
    const float ig = act[ab], fg = act[ab + H], gg = act[ab + 2LL * H], og = act[ab + 3LL * H];
    const float tc = tanhf(c[i]);
    const float dog = dht * tc;
    float dcv = dht * og * (1.f - tc * tc);
    if (dh_last == nullptr) dcv += dc[i];                // (dh_last is given on the last step only: nothing carried yet)
    const float cp = c_prev != nullptr ? c_prev[i] : 0.f;
    const float d_i = dcv * gg * ig * (1.f - ig);
    const float d_f = dcv * cp * fg * (1.f - fg);
    const float d_g = dcv * ig * (1.f - gg * gg);
    const float d_o = dog * og * (1.f - og);
    dgates[ab] = d_i;
    dgates[ab + H] = d_f;
    dgates[ab + 2LL * H] = d_g;
    dgates[ab + 3LL * H] = d_o;
    if (dgates_t != nullptr) {
      dgates_t[(long long)u * ldt + row] = d_i;
      dgates_t[((long long)H + u) * ldt + row] = d_f;
      dgates_t[(2LL * H + u) * ldt + row] = d_g;
      dgates_t[(3LL * H + u) * ldt + row] = d_o;
    }
    dc[i] = dcv * fg;
  }
}

// ------------------------------------------------------------------------------------------
// MaxPool2d((3,1)) + Dropout.  Y rows [seq * Tp + t][ldy], sequences branch-major: the B * w1 LSTM-branch columns (seq =
// b * w1 + j), then the B * Cn electrode columns.  Element (b, ch, s, w) of the contiguous (B, C, tq, W) activation
// (w = j, or w1 + electrode: torch.cat((x1, x), dim=3)) has flat offset f = (ch * tq + s) * W + w inside its batch element,
// and the reference's raw view hands the second LSTM row f / (C W), column f % (C W) of that element: X row b * rs_b +
// (f / (C W)) * rs_t.  The keep decision is tl_dropout_scale's at the element's position in the (seq, s, ch) buffer of the
// forward-only engine.  One thread per (seq, s, ch), ch fastest: the row reads are coalesced.
// ------------------------------------------------------------------------------------------
struct pool3_geom {
  long long nseq;
  int B, w1, Cn, C, Tp, tq, ldy;
  long long rs_b, rs_t;
  float p, inv_keep;
  uint64_t seed;
  // data-parallel shard: what a local sequence number is short of the sequence's number in the GLOBAL batch's branch-major
  // order, per branch ((b0 + b) * w1 + j, and B_global * w1 + (b0 + b) * Cn + e); both 0 for a whole batch
  long long kseq_lstm, kseq_el;
};

// position of element (seq, s, ch) in the (seq, s, ch) buffer of the global batch: the index of the keep decision
__device__ __forceinline__ uint64_t pool3_keep_index(const pool3_geom& g, long long seq, int s, int ch) {
  const long long gseq = seq + (seq < (long long)g.B * g.w1 ? g.kseq_lstm : g.kseq_el);
  return (uint64_t)((gseq * g.tq + s) * g.C + ch);
}

__device__ __forceinline__ long long pool3_x_index(const pool3_geom& g, long long seq, int s, int ch) {
  const long long nb = (long long)g.B * g.w1;
  long long b;
  int w;
  if (seq < nb) {
    b = seq / g.w1;
    w = (int)(seq - b * g.w1);
  } else {
    const long long q = seq - nb;
    b = q / g.Cn;
    w = g.w1 + (int)(q - b * g.Cn);
  }
  const int W = g.w1 + g.Cn;
  const long long rowlen = (long long)g.C * W;
  const long long f = ((long long)ch * g.tq + s) * W + w;
  const long long r = f / rowlen;
  return (b * g.rs_b + r * g.rs_t) * rowlen + (f - r * rowlen);
}

__device__ __forceinline__ int first_max3(float v0, float v1, float v2) {
  int arg = 0;
  float m = v0;
  if (v1 > m) { m = v1; arg = 1; }
  if (v2 > m) arg = 2;
  return arg;
}

__global__ __launch_bounds__(256) void pool3_fwd_kernel(const float* __restrict__ Y, float* __restrict__ X, pool3_geom g) {
  const long long total = g.nseq * g.tq * g.C;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % g.C);
    const long long r = i / g.C;
    const int s = (int)(r % g.tq);
    const long long seq = r / g.tq;
    const float* y = Y + (seq * g.Tp + 3LL * s) * g.ldy + ch;
    const float v0 = y[0], v1 = y[g.ldy], v2 = y[2LL * g.ldy];
    const int arg = first_max3(v0, v1, v2);
    float m = arg == 0 ? v0 : (arg == 1 ? v1 : v2);
    if (g.p > 0.f) m = u01(g.seed, pool3_keep_index(g, seq, s, ch)) >= g.p ? m * g.inv_keep : 0.f;
    X[pool3_x_index(g, seq, s, ch)] = m;
  }
}

// dZ[seq * Tp + 3 s + arg][ch] = dX * keep / (1 - p) * LeakyReLU'(Y at the arg-max), zero in the other two rows of the triple,
// in rows t >= 3 tq and in the pad rows of the sequence: one thread per (seq, row triple, ch) writes its three rows.
__global__ __launch_bounds__(256) void pool3_bwd_kernel(const float* __restrict__ Y, const float* __restrict__ dX,
                                                        float* __restrict__ dZ, int lddz, float slope, pool3_geom g) {
  const int ntri = (g.Tp + 2) / 3;
  const long long total = g.nseq * ntri * g.C;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % g.C);
    const long long r = i / g.C;
    const int s = (int)(r % ntri);
    const long long seq = r / ntri;
    float out[3] = {0.f, 0.f, 0.f};
    if (s < g.tq) {
      const float* y = Y + (seq * g.Tp + 3LL * s) * g.ldy + ch;
      const float v0 = y[0], v1 = y[g.ldy], v2 = y[2LL * g.ldy];
      const int arg = first_max3(v0, v1, v2);
      const float m = arg == 0 ? v0 : (arg == 1 ? v1 : v2);
      float d = dX[pool3_x_index(g, seq, s, ch)];
      if (g.p > 0.f) d = u01(g.seed, pool3_keep_index(g, seq, s, ch)) >= g.p ? d * g.inv_keep : 0.f;
      d *= m > 0.f ? 1.f : slope;
#pragma unroll
      for (int a = 0; a < 3; ++a) out[a] = a == arg ? d : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (3 * s + a < g.Tp) dZ[(seq * g.Tp + 3LL * s + a) * lddz + ch] = out[a];
  }
}

// ------------------------------------------------------------------------------------------
// Input gradient of the first stage (C_in = 1): dx[seq][2 t + a + j] = sum over (t, j) reaching the sample of
// sum_c G1[seq * Tp + t][c] w[c][j], a = the arg-max bit of (t, c).  One workgroup owns a whole sequence.  A wave streams a
// row of G1 (lane l owns channels 256 i + 4 l .. + 3, i < C1 / 256; their taps sit in registers), splits the row's sum by
// arg-max bit and reduces the 2 KT sums across its lanes (xor butterfly: every lane ends with the same bits); per chunk of 64
// rows the sums go to LDS, and after a barrier thread u gathers the (t, a, j) that reach sample u in a fixed order into the
// sequence's dx image in LDS.  Output sample u of sequence (o, i) = (seq / n_inner, seq % n_inner) goes to
// out[o * stride_outer + u * stride_t + i * stride_inner] (the first LSTM's h1[b][t * w1 + j] for (b, j)).
// ------------------------------------------------------------------------------------------
constexpr int CD_ROWS = 64;
constexpr int CD_MAXKT = 8;

template <int KT, int NQ>
__global__ __launch_bounds__(256) void conv1_dgrad_kernel(const float* __restrict__ G, const uint32_t* __restrict__ bits,
                                                          const float* __restrict__ w, float* __restrict__ out, int T, int Tp,
                                                          int Tout, int n_inner, long long stride_outer, long long stride_t,
                                                          long long stride_inner) {
  constexpr int C1 = NQ * 256;
  extern __shared__ __attribute__((aligned(16))) float dxs[];                   // [T]
  __shared__ float sums[CD_ROWS][2][CD_MAXKT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long seq = blockIdx.x;
  for (int u = tid; u < T; u += 256) dxs[u] = 0.f;
  float wv[NQ][4][KT];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < KT; ++j) wv[q][e][j] = w[(long long)(q * 256 + 4 * lane + e) * KT + j];
  for (int t0 = 0; t0 < Tout; t0 += CD_ROWS) {
    const int nt = Tout - t0 < CD_ROWS ? Tout - t0 : CD_ROWS;
    for (int tl = wave; tl < nt; tl += 4) {
      const long long row = seq * Tp + t0 + tl;
      float acc[2][KT];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[a][j] = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(G + row * C1 + q * 256 + 4 * lane);
        const uint32_t wb = bits[row * (C1 >> 5) + q * 8 + (lane >> 3)] >> ((4 * lane) & 31);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool odd = (wb >> e) & 1u;
          const float g0 = odd ? 0.f : g[e], g1 = odd ? g[e] : 0.f;
#pragma unroll
          for (int j = 0; j < KT; ++j) {
            acc[0][j] = fmaf(g0, wv[q][e][j], acc[0][j]);
            acc[1][j] = fmaf(g1, wv[q][e][j], acc[1][j]);
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < KT; ++j) {
          float v = acc[a][j];
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
          if (lane == 0) sums[tl][a][j] = v;
        }
    }
    __syncthreads();
    // samples this chunk reaches: u in [2 t0, 2 (t0 + nt) + KT - 1)
    const int ulo = 2 * t0, uhi = 2 * (t0 + nt) + KT - 1 < T ? 2 * (t0 + nt) + KT - 1 : T;
    for (int u = ulo + tid; u < uhi; u += 256) {
      float v = dxs[u];
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        const int r = u - j - 2 * t0;                    // = 2 tl + a
        if (r >= 0 && (r >> 1) < nt) v += sums[r >> 1][r & 1][j];
      }
      dxs[u] = v;
    }
    __syncthreads();
  }
  __syncthreads();
  const long long o = seq / n_inner, in = seq - o * n_inner;
  for (int u = tid; u < T; u += 256) out[o * stride_outer + u * stride_t + in * stride_inner] = dxs[u];
}

}  // namespace tl

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" int tl_lstm_train_seq(const float* xp, int64_t xp_row_stride, int64_t xp_step_stride, const float* wp, float* hs,
                                 float* cs, float* act, int B, int H, int T, void* stream) {
  using namespace tl;
  TL_REQUIRE(xp && wp && hs && cs && act, "lstm_train_seq: null pointer");
  TL_REQUIRE(B > 0 && H > 0 && T >= 1, "lstm_train_seq: B, H > 0 and T >= 1 needed");
  TL_REQUIRE(H % 8 == 0, "lstm_train_seq: hidden width must be a multiple of 8 (pad the packed weights)");
  TL_REQUIRE(xp_row_stride >= 4LL * H && xp_step_stride >= 4LL * H, "lstm_train_seq: xp row / step stride shorter than 4 H");
  TL_REQUIRE((((uintptr_t)wp | (uintptr_t)hs) & 15) == 0, "lstm_train_seq: wp and hs must be 16-byte aligned");
  dim3 grid((unsigned)(H / 8), (unsigned)((B + 31) / 32));
  TL_REQUIRE(grid.y <= 65535u, "lstm_train_seq: batch too large");
  const long long bh = (long long)B * H;
  for (int t = 0; t < T; ++t)
    hipLaunchKernelGGL(lstm_train_step_kernel, grid, dim3(512), 0, (hipStream_t)stream, xp + (long long)t * xp_step_stride,
                       (long long)xp_row_stride, wp, hs + (t > 0 ? (t - 1) * bh : 0), hs + t * bh, cs + (t > 0 ? (t - 1) * bh : 0),
                       cs + t * bh, act + t * 4 * bh, B, H, t == 0 ? 1 : 0);
  return check_launch("lstm_train_seq");
}

extern "C" int tl_lstm_bptt_seq(const float* whT, const float* dh_last, const float* act, const float* cs, float* dc, float* dgates,
                                float* dgates_t, int64_t ldt, int B, int H, int T, void* stream) {
  using namespace tl;
  TL_REQUIRE(whT && dh_last && act && cs && dc && dgates, "lstm_bptt_seq: null pointer");
  TL_REQUIRE(B > 0 && H > 0 && T >= 1, "lstm_bptt_seq: B, H > 0 and T >= 1 needed");
  TL_REQUIRE(H % 8 == 0, "lstm_bptt_seq: hidden width must be a multiple of 8 (pad the packed weights)");
  TL_REQUIRE(!dgates_t || ldt >= (int64_t)T * B, "lstm_bptt_seq: the transposed copy needs ldt >= T * B");
  TL_REQUIRE((((uintptr_t)whT | (uintptr_t)dgates) & 15) == 0, "lstm_bptt_seq: whT and dgates must be 16-byte aligned");
  dim3 grid((unsigned)((H + 31) / 32), (unsigned)((B + 31) / 32));
  TL_REQUIRE(grid.y <= 65535u, "lstm_bptt_seq: batch too large");
  const long long bh = (long long)B * H;
  for (int t = T - 1; t >= 0; --t)
    hipLaunchKernelGGL(lstm_bptt_step_kernel, grid, dim3(512), 0, (hipStream_t)stream,
                       t == T - 1 ? (const float*)nullptr : dgates + (t + 1) * 4 * bh, whT, t == T - 1 ? dh_last : (const float*)nullptr,
                       act + t * 4 * bh, cs + t * bh, t > 0 ? cs + (t - 1) * bh : (const float*)nullptr, dc, dgates + t * 4 * bh,
                       dgates_t ? dgates_t + (long long)t * B : (float*)nullptr, (long long)ldt, B, H);
  return check_launch("lstm_bptt_seq");
}

static int pool3_geom_check(tl::pool3_geom& g, const char* what, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int64_t rs_b,
                            int64_t rs_t, float p, uint64_t seed, int b0, int B_global) {
  TL_REQUIRE(b0 >= 0 && B_global >= 1 && (long long)b0 + B <= B_global, "%s: rows [%d, %d + %d) outside the global batch of %d", what,
             b0, b0, B, B_global);
  TL_REQUIRE(B > 0 && w1 >= 0 && Cn >= 0 && w1 + Cn > 0 && C > 0, "%s: bad sizes", what);
  TL_REQUIRE(tq >= 1 && 3LL * tq <= Tp, "%s: 1 <= tq and 3 tq <= Tp needed (%d, %d)", what, tq, Tp);
  TL_REQUIRE(ldy >= C, "%s: row stride %d shorter than the %d channels", what, ldy, C);
  TL_REQUIRE(rs_b >= 1 && rs_t >= 1, "%s: row strides of the LSTM input must be positive", what);
  TL_REQUIRE(p >= 0.f && p < 1.f, "%s: p must be in [0, 1)", what);
  g.nseq = (long long)B * (w1 + Cn);
  TL_REQUIRE(g.nseq * Tp * (long long)ldy < (1LL << 40), "%s: too many rows", what);
  g.B = B; g.w1 = w1; g.Cn = Cn; g.C = C; g.Tp = Tp; g.tq = tq; g.ldy = ldy;
  g.rs_b = rs_b; g.rs_t = rs_t;
  g.p = p; g.inv_keep = 1.0f / (1.0f - p); g.seed = seed;
  g.kseq_lstm = (long long)b0 * w1;
  g.kseq_el = (long long)(B_global - B) * w1 + (long long)b0 * Cn;
  TL_REQUIRE((long long)B_global * (w1 + Cn) * tq * (long long)C < (1LL << 62), "%s: global batch too large", what);
  return TL_OK;
}

static unsigned pool3_blocks(long long total) {
  long long nb = (total + 255) / 256;
  return (unsigned)(nb > 65536 ? 65536 : nb);
}

static int pool3_fwd_launch(const char* what, const float* Y, float* X, int B, int w1, int Cn, int C, int Tp, int tq, int ldy,
                            int64_t rs_b, int64_t rs_t, float p, uint64_t seed, int b0, int B_global, void* stream) {
  using namespace tl;
  TL_REQUIRE(Y && X, "%s: null pointer", what);
  pool3_geom g;
  if (int rc = pool3_geom_check(g, what, B, w1, Cn, C, Tp, tq, ldy, rs_b, rs_t, p, seed, b0, B_global)) return rc;
  hipLaunchKernelGGL(pool3_fwd_kernel, dim3(pool3_blocks(g.nseq * tq * C)), dim3(256), 0, (hipStream_t)stream, Y, X, g);
  return check_launch(what);
}

static int pool3_bwd_launch(const char* what, const float* Y, const float* dX, float* dZ, int B, int w1, int Cn, int C, int Tp, int tq,
                            int ldy, int lddz, int64_t rs_b, int64_t rs_t, float p, uint64_t seed, float slope, int b0,
                            int B_global, void* stream) {
  using namespace tl;
  TL_REQUIRE(Y && dX && dZ, "%s: null pointer", what);
  TL_REQUIRE(lddz >= C, "%s: row stride %d of dZ shorter than the %d channels", what, lddz, C);
  pool3_geom g;
  if (int rc = pool3_geom_check(g, what, B, w1, Cn, C, Tp, tq, ldy, rs_b, rs_t, p, seed, b0, B_global)) return rc;
  hipLaunchKernelGGL(pool3_bwd_kernel, dim3(pool3_blocks(g.nseq * ((Tp + 2) / 3) * C)), dim3(256), 0, (hipStream_t)stream, Y, dX, dZ,
                     lddz, slope, g);
  return check_launch(what);
}

extern "C" int tl_pool3_fwd(const float* Y, float* X, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int64_t rs_b,
                            int64_t rs_t, float p, uint64_t seed, void* stream) {
  return pool3_fwd_launch("pool3_fwd", Y, X, B, w1, Cn, C, Tp, tq, ldy, rs_b, rs_t, p, seed, 0, B, stream);
}

extern "C" int tl_pool3_bwd(const float* Y, const float* dX, float* dZ, int B, int w1, int Cn, int C, int Tp, int tq, int ldy,
                            int lddz, int64_t rs_b, int64_t rs_t, float p, uint64_t seed, float slope, void* stream) {
  return pool3_bwd_launch("pool3_bwd", Y, dX, dZ, B, w1, Cn, C, Tp, tq, ldy, lddz, rs_b, rs_t, p, seed, slope, 0, B, stream);
}

// The same two kernels on rows [b0, b0 + B) of a global batch of B_global: X / dZ addressing stays local, the keep decision is the
// global batch's (a shard draws its rows of the single-process mask).
extern "C" int tl_pool3_fwd_shard(const float* Y, float* X, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int64_t rs_b,
                                  int64_t rs_t, float p, uint64_t seed, int b0, int B_global, void* stream) {
  return pool3_fwd_launch("pool3_fwd_shard", Y, X, B, w1, Cn, C, Tp, tq, ldy, rs_b, rs_t, p, seed, b0, B_global, stream);
}

extern "C" int tl_pool3_bwd_shard(const float* Y, const float* dX, float* dZ, int B, int w1, int Cn, int C, int Tp, int tq, int ldy,
                                  int lddz, int64_t rs_b, int64_t rs_t, float p, uint64_t seed, float slope, int b0, int B_global,
                                  void* stream) {
  return pool3_bwd_launch("pool3_bwd_shard", Y, dX, dZ, B, w1, Cn, C, Tp, tq, ldy, lddz, rs_b, rs_t, p, seed, slope, b0, B_global,
                          stream);
}

extern "C" int tl_conv1_dgrad(const float* G, const uint32_t* bits, const float* w, float* dx, int64_t S, int T, int ktaps, int C1,
                              int Tp, int Tout, int n_inner, int64_t stride_outer, int64_t stride_t, int64_t stride_inner,
                              void* stream) {
  using namespace tl;
  TL_REQUIRE(G && bits && w && dx, "conv1_dgrad: null pointer");
  TL_REQUIRE(S > 0 && S < (1LL << 31), "conv1_dgrad: bad S");
  // one instantiation: the first stage of CNNRNNClassifier, the only caller (the kernel is a template over both)
  TL_REQUIRE(ktaps == 7, "conv1_dgrad: ktaps must be 7");
  TL_REQUIRE(C1 == 1024, "conv1_dgrad: C1 must be 1024");
  TL_REQUIRE(Tout >= 0 && Tout <= Tp && 2 * Tout + ktaps - 1 <= T, "conv1_dgrad: Tout/Tp/T inconsistent (%d,%d,%d)", Tout, Tp, T);
  TL_REQUIRE((size_t)T * 4 <= 64 * 1024, "conv1_dgrad: T too large for the LDS image");
  TL_REQUIRE(n_inner >= 1 && stride_t >= 1, "conv1_dgrad: bad output map");
  TL_REQUIRE(((uintptr_t)G & 15) == 0, "conv1_dgrad: G must be 16-byte aligned");
  hipLaunchKernelGGL((conv1_dgrad_kernel<7, 4>), dim3((unsigned)S), dim3(256), (size_t)T * 4, (hipStream_t)stream, G, bits, w, dx, T,
                     Tp, Tout, n_inner, (long long)stride_outer, (long long)stride_t, (long long)stride_inner);
  return check_launch("conv1_dgrad");
}
