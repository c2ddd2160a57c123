// Winograd F(6,3) on pre-transformed operands (round 4): the V-form kernels of tonal_wino43v.hip with HEXES in place of
// quads - 8 products per 6 conv rows instead of 6 per 4 (0.444 of the direct convolution's multiplies against 0.5).
//
// conv2 / conv3 of the ECoG stack (models/synthesis_models.py:91-97) and their backward are 80 % of the train step and
// run on the fp32 matrix pipe at 0.77 - 0.83 of its peak: what is left is the amount of matrix work itself.  The numerics
// of the form were cleared first (oracle/winograd_f63_gate.py: per stage 8.5e-7 relative L2 against fp64, the 30-step
// trajectory of golden G14 1.9e-6 from the reference's - the same noise floor as F(4,3)).  Interpolation points
// 0, +-1, +-2, +-1/2, inf; the matrices are the exact Cook-Toom construction of that script.
//
// Layouts.  A sequence holds Tp rows, Tp a multiple of 6 (of 12 where the pooled output feeds another F(6,3) stage).
// Hex H of a sequence = its rows 6 H .. 6 H + 7 (rows past the sequence taken as zero), eight transforms, ldv channels
// (a multiple of 8); zero hexes appended to whole 128-hex tiles.  Vd the same for the un-pooled dZ rows 6 H - 2 .. 6 H + 5.
// V is stored in the PAIR layout V[hex / 2][ldv / 8][8 transforms][hex % 2][8 channels] (8 ldv floats per hex, like
// [hex][8][ldv]): what one LDS-DMA piece of the NT kernel fetches - an 8-channel chunk of one transform of 32 hexes - is
// then 16 runs of 64 B, and a piece of the weight-gradient kernel (64 channels of four (transform, hex) rows) 16 runs of
// 64 B as well.  (With channels last an NT piece is 32 runs of 32 B, a quarter of a cache line each: measured 4.2 of 41.5
// ms at conv2 forward - the 8-deep K-steps that three stages in 160 KB of LDS allow make the runs that short.)  The taps
// are stored chunk-major for the same reason: U[K / 8][8 transforms][rows][8] - a piece is 1 KB contiguous.
//
//   tl_wino63_weights       w (O, I, 3, 1) -> forward taps [8][O][ld_f], input-gradient taps [8][I][ld_d] (flipped)
//   tl_wino63_weights_y     ... -> the taps of an input gradient that runs on Y = A dz (un-flipped, contracted over C_out)
//   tl_conv3_wino63v_nt     M_i[hex][n] = sum_k V_i[hex][k] U_i[n][k], i < 8: batched NT GEMM, both operands by LDS-DMA
//                           into three 8-deep stages, epilogues of tonal_wino63_epi.h
//   tl_wino63_v_fixup       second half of the V-writing forward epilogue
//   tl_conv3_wino63v_tn     weight gradient slab_i[c_in][c_out] = sum_hexes V_i (x) Y_i, Y = A dy; also writes Vd
//   tl_wino63_wgrad_finalize  dW = G^T (sum of slabs)
//   tl_conv1_fwd_v6         first stage (C_in = 1) writing V of its pooled output in hex form
#include "tonal_common.h"
#include "tonal_wino43_epi.h"
#include "tonal_wino43v_epi.h"
#include "tonal_wino63_epi.h"
#include "tonal_wino63_kloop.h"
#include <type_traits>

namespace tl {

typedef __attribute__((address_space(3))) void lds_void6_t;
__device__ __forceinline__ void dma16h(__amdgpu_buffer_rsrc_t rs, char* lds_dst, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void6_t*)lds_dst, 16, voff, soff, 0, 0);
}

// A raw buffer resource as four scalar words (what __builtin_amdgcn_make_buffer_rsrc builds: base, stride 0, num_records =
// bytes, flags) - as a plain vector it can be an "s" operand of the K-loop asm statements (tonal_wino63_kloop.h)
typedef int v6_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v6_i32x4 v6_rsrc_words(const void* base, long long bytes) {
  const unsigned long long a = (unsigned long long)base;
  const long long n = bytes < 0 ? 0 : (bytes < 0x7fffffffLL ? bytes : 0x7fffffffLL);
  return v6_i32x4{(int)(unsigned)a, (int)(unsigned)((a >> 32) & 0xffffu), (int)n, 0x00020000};
}

// float offset of (hex, transform i, channel c) in the pair layout; kc8 = ldv / 8
__device__ __forceinline__ long long v6_at(long long hex, int i, int c, int kc8) {
  return ((((hex >> 1) * kc8 + (c >> 3)) * 8 + i) * 2 + (hex & 1)) * 8 + (c & 7);
}

// ------------------------------------------------------------------------------------------
// Tap transforms U = G g,  G = [-1 0 0; -2/9 (1 1 1); -2/9 (1 -1 1); 1/90 (1 2 4); 1/90 (1 -2 4); 1/45 (32 16 8);
// 1/45 (32 -16 8); 0 0 1]
// ------------------------------------------------------------------------------------------
__global__ void wino63_weights_kernel(const float* __restrict__ w, float* __restrict__ fwd, float* __restrict__ dgr, int O,
                                      int I, int ld_f, int ld_d, int flip) {
  const long long n_f = (long long)O * ld_f, n_d = (long long)I * ld_d;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // element (transform t, row r of R, reduction index k) of a chunk-major tap set: ((k / 8 * 8 + t) * R + r) * 8 + k % 8
  auto emit = [](float* dst, int R, int r, int k, float g0, float g1, float g2) {
    float* d0 = dst + (((long long)(k >> 3) * 8) * R + r) * 8 + (k & 7);
    const long long n = (long long)R * 8;
    const float s = g0 + g2;
    d0[0] = -g0;
    d0[n] = (-2.f / 9.f) * (s + g1);
    d0[2 * n] = (-2.f / 9.f) * (s - g1);
    const float a = fmaf(4.f, g2, g0), b = 2.f * g1;
    d0[3 * n] = (1.f / 90.f) * (a + b);
    d0[4 * n] = (1.f / 90.f) * (a - b);
    const float c = fmaf(4.f, g0, g2), d = 2.f * g1;
    d0[5 * n] = (8.f / 45.f) * (c + d);
    d0[6 * n] = (8.f / 45.f) * (c - d);
    d0[7 * n] = g2;
  };
  if (fwd != nullptr && idx < n_f) {
    const int o = (int)(idx / ld_f), i = (int)(idx % ld_f);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (i < I) {
      const float* s = w + ((long long)o * I + i) * 3;
      g0 = s[0], g1 = s[1], g2 = s[2];
    }
    emit(fwd, O, o, i, g0, g1, g2);
  }
  if (dgr != nullptr && idx < n_d) {
    const int i = (int)(idx / ld_d), o = (int)(idx % ld_d);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (o < O) {
      const float* s = w + ((long long)o * I + i) * 3;
      if (flip) g0 = s[2], g1 = s[1], g2 = s[0];          // flipped taps (the Vd form of the input gradient)
      else g0 = s[0], g1 = s[1], g2 = s[2];               // as they are (its Y form: tl_wino63_weights_y)
    }
    emit(dgr, I, i, o, g0, g1, g2);
  }
}

// dW (O, I, 3) = G^T M from the reduced transforms red[8][I][ld]
__global__ void wino63_wgrad_finalize_kernel(const float* __restrict__ red, float* __restrict__ gw, int O, int I, int ld) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)O * I) return;
  const int i = (int)(idx / O), o = (int)(idx % O);
  const long long plane = (long long)I * ld;
  const float* s = red + (long long)i * ld + o;
  float m[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) m[t] = s[t * plane];
  const float a12 = m[1] + m[2], s12 = m[1] - m[2], a34 = m[3] + m[4], s34 = m[3] - m[4], a56 = m[5] + m[6], s56 = m[5] - m[6];
  float* d = gw + ((long long)o * I + i) * 3;
  d[0] = -m[0] - (2.f / 9.f) * a12 + (1.f / 90.f) * a34 + (32.f / 45.f) * a56;
  d[1] = -(2.f / 9.f) * s12 + (1.f / 45.f) * s34 + (16.f / 45.f) * s56;
  d[2] = -(2.f / 9.f) * a12 + (2.f / 45.f) * a34 + (8.f / 45.f) * a56 + m[7];
}

// Taps of a 7-tap (k,1) convolution as three F(6,3) segments (taps 3 s .. 3 s + 2 of segment s, missing ones zero), chunk-major
// over the concatenated reduction index k = s I + i: fwd[3 I / 8][8 transforms][O][8]
__global__ void wino63_weights7_kernel(const float* __restrict__ w, float* __restrict__ fwd, int O, int I, int taps) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 3LL * O * I) return;
  const int k = (int)(idx % (3LL * I)), o = (int)(idx / (3LL * I));
  const int seg = k / I, i = k - seg * I;
  const float* s = w + ((long long)o * I + i) * taps + 3 * seg;
  const float g0 = 3 * seg < taps ? s[0] : 0.f, g1 = 3 * seg + 1 < taps ? s[1] : 0.f, g2 = 3 * seg + 2 < taps ? s[2] : 0.f;
  float* d0 = fwd + (((long long)(k >> 3) * 8) * O + o) * 8 + (k & 7);
  const long long n = (long long)O * 8;
  const float sm = g0 + g2;
  d0[0] = -g0;
  d0[n] = (-2.f / 9.f) * (sm + g1);
  d0[2 * n] = (-2.f / 9.f) * (sm - g1);
  const float a = fmaf(4.f, g2, g0), b = 2.f * g1;
  d0[3 * n] = (1.f / 90.f) * (a + b);
  d0[4 * n] = (1.f / 90.f) * (a - b);
  const float c = fmaf(4.f, g0, g2), d = 2.f * g1;
  d0[5 * n] = (8.f / 45.f) * (c + d);
  d0[6 * n] = (8.f / 45.f) * (c - d);
  d0[7 * n] = g2;
}

// Rows P[seq * Tp + t][C] -> V0 = B^T (rows 6 h .. 6 h + 7) and V1 = B^T (rows 6 h + 3 .. 6 h + 10) of every hex, pair layout:
// the operands of tl_conv7_wino63v_nt.  Rows from Tvalid on (and past the sequence) enter as zeros.  Thread = 4 channels x one
// hex, lanes ordered (8-channel chunk, hex of the pair, half chunk) like wino63_unpool_yvd_kernel: whole 64-byte runs.
// shift (tl_wino63_xform2s): the rows enter moved down by `shift` inside their sequence - row t as row t + shift, zeros in front.
__global__ __launch_bounds__(256, 4) void wino63_xform2_kernel(const float* __restrict__ P, float* __restrict__ V0, float* __restrict__ V1,
                                                             long long nhex, int hps, int Tp, int Tvalid, int C, int ldp, int ldv,
                                                             int shift) {
  const int tpp = C >> 1;                                    // threads per hex pair
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long pair = idx / tpp;
  const int tl_ = (int)(idx - pair * tpp);
  const int half = tl_ & 1, hpar = (tl_ >> 1) & 1, kc = tl_ >> 2;
  const int c = 8 * kc + 4 * half;
  const long long hg = 2 * pair + hpar;
  if (hg >= nhex) return;
  const long long seq = hg / hps;
  const int hs = (int)(hg - seq * hps);
  const float* src = P + (seq * Tp + 6LL * hs) * (long long)ldp + c;
  f32x4 d[11];
#pragma unroll
  for (int j = 0; j < 11; ++j) {
    d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t = 6 * hs + j - shift;
    if (t >= 0 && t < Tvalid) d[j] = *reinterpret_cast<const f32x4*>(src + (long long)(j - shift) * ldp);
  }
  f32x4 o0[8], o1[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float a[8], b[8], va[8], vb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = d[j][k];
      b[j] = d[j + 3][k];
    }
    wino63_bt(a, va);
    wino63_bt(b, vb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o0[j][k] = va[j];
      o1[j][k] = vb[j];
    }
  }
  const long long at = v6_at(hg, 0, c, ldv >> 3);
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(V0 + at + 16 * j) = o0[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(V1 + at + 16 * j) = o1[j];
}

// Gradient rows dz[seq * Tp + t][C] of a stage WITHOUT a pool -> Y = A dz (rows 6 h .. 6 h + 5) of every hex, pair layout: the
// second operand of tl_conv3_wino63v_tn with loader 3 for the three segments of a 7-tap weight gradient.  Rows from Tvalid on
// enter as zeros.  Planes and their arithmetic are wino63_unpool_yvd_kernel's (plane 1 = the sum of the six rows); threads as above.
__global__ __launch_bounds__(256, 4) void wino63_ydz_kernel(const float* __restrict__ G, float* __restrict__ Y, long long nhex, int hps,
                                                          int Tp, int Tvalid, int C, int ldg, int ldv) {
  const int tpp = C >> 1;                                    // threads per hex pair
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long pair = idx / tpp;
  const int tl_ = (int)(idx - pair * tpp);
  const int half = tl_ & 1, hpar = (tl_ >> 1) & 1, kc = tl_ >> 2;
  const int c = 8 * kc + 4 * half;
  const long long hg = 2 * pair + hpar;
  if (hg >= nhex) return;
  const long long seq = hg / hps;
  const int hs = (int)(hg - seq * hps);
  const float* src = G + (seq * Tp + 6LL * hs) * (long long)ldg + c;
  f32x4 d[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (6 * hs + j < Tvalid) d[j] = *reinterpret_cast<const f32x4*>(src + (long long)j * ldg);
  }
  f32x4 oy[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d6[6] = {d[0][k], d[1][k], d[2][k], d[3][k], d[4][k], d[5][k]};
    const float ev1 = (d6[0] + d6[2]) + d6[4], od1 = (d6[1] + d6[3]) + d6[5];
    const float ev2 = fmaf(16.f, d6[4], fmaf(4.f, d6[2], d6[0])), od2 = fmaf(32.f, d6[5], fmaf(8.f, d6[3], 2.f * d6[1]));
    const float ev3 = fmaf(0.0625f, d6[4], fmaf(0.25f, d6[2], d6[0])), od3 = fmaf(0.03125f, d6[5], fmaf(0.125f, d6[3], 0.5f * d6[1]));
    const float y[8] = {d6[0], ev1 + od1, ev1 - od1, ev2 + od2, ev2 - od2, ev3 + od3, ev3 - od3, d6[5]};
#pragma unroll
    for (int j = 0; j < 8; ++j) oy[j][k] = y[j];
  }
  const long long at = v6_at(hg, 0, c, ldv >> 3);
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(Y + at + 16 * j) = oy[j];
}

// ------------------------------------------------------------------------------------------
// Second half of the V-writing forward epilogue (tonal_wino63_epi.h, POOLV): the last output hex of every 128-hex tile
// (64 next-stage hexes) needs pooled rows 6, 7 from the next tile.  The tile left rows 0..5 raw in the hex's transform
// slots 0..5 and every tile stored its first two pooled rows to vhalo; thread = (tile, 4 channels).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void wino63_v_fixup_kernel(float* __restrict__ V, const float* __restrict__ halo, long long hexes,
                                                              long long tiles, int Tq, int C, int ldv) {
  const int c4n = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= tiles * c4n) return;
  const long long t = idx / c4n;
  const int c = (int)(idx - t * c4n) * 4;
  const long long q = t * 64 + 63;
  if (q >= hexes) return;
  float* v = V + v6_at(q, 0, c, ldv >> 3);                  // transform j of these four channels: v + 16 j
  f32x4 d[8];
#pragma unroll
  for (int j = 0; j < 6; ++j) d[j] = *reinterpret_cast<const f32x4*>(v + 16 * j);
  const int tq = (int)((6 * q) % Tq);
  if (tq + 6 < Tq && t + 1 < tiles) {
    d[6] = *reinterpret_cast<const f32x4*>(halo + ((t + 1) * 2) * (long long)C + c);
    d[7] = *reinterpret_cast<const f32x4*>(halo + ((t + 1) * 2 + 1) * (long long)C + c);
  } else {
    d[6] = d[7] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 o[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float dd[8], vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) dd[j] = d[j][k];
    wino63_bt(dd, vv);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j][k] = vv[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(v + 16 * j) = o[j];
}

// ------------------------------------------------------------------------------------------
// NT kernel on V.  Workgroup: 8 waves as 4 (hexes) x 2 (columns); block tile 128 hexes (768 conv rows) x 64 columns;
// wave tile 32 hexes x 32 columns x 8 transforms = 128 accumulator registers.  A K-step is 8 channels: A stage
// [8][128 hexes][32 B] = 32 KB, B stage [8][64 columns][32 B] = 16 KB; THREE stages = 144 KB (a 16-deep stage would be 96 KB:
// two do not fit), filled two steps ahead by 48 LDS-DMA pieces (32 rows x 32 B each), 6 per wave - the same 0.19 pieces
// per MFMA as the F(4,3) kernel.  Per wave and K-step: 16 ds_read_b128 + 32 MFMAs; the fragments are held as two half-sets
// (transforms 0-3, 4-7: 32 registers each), the second one carried across the closing barrier.
// LDS rows are 32 B: bank conflicts of the fragment reads are removed by swapping the two 16-byte chunks of the rows with
// bit 3 set (applied to the per-lane SOURCE address of the LDS-DMA and to the fragment read).
// ------------------------------------------------------------------------------------------
constexpr int V6_BH = 128, V6_BN = 64, V6_BK = 8;
constexpr int V6_ROWB = V6_BK * 4;                       // bytes per LDS row (32)
constexpr int V6_A_BYTES = 8 * V6_BH * V6_ROWB;          // 32768
constexpr int V6_B_BYTES = 8 * V6_BN * V6_ROWB;          // 16384
constexpr int V6_STAGE = V6_A_BYTES + V6_B_BYTES;        // 49152
constexpr int V6_ROWS = 6 * V6_BH;                       // conv rows per tile (768)

template <int EPI>
__global__ __launch_bounds__(512, 2) void wino63v_nt_kernel(const tl_nt_params p) {
  __shared__ __attribute__((aligned(1024))) char lds[3 * V6_STAGE + ((EPI == W_EPI_POOLV || EPI == W_EPI_MASKY || EPI == W_EPI_GY) ? 4096 : (EPI == W_EPI_C1W || EPI == W6_EPI_C1W_Y) ? 16384 : 0)];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;

  const int ntn = (p.N + V6_BN - 1) / V6_BN;
  const long long ntm = (p.M + V6_ROWS - 1) / V6_ROWS;
  const long long nwg = ntm * ntn;
  // EPI == LRELU: a SEVEN-tap convolution as three 3-tap segments summed in the transform domain (tl_conv7_wino63v_nt): the K
  // loop runs over 3 K channels - segment 0 = V0 (A), hex H; segment 1 = V1 (aux: the transform of the rows shifted by 3);
  // segment 2 = V0 again, hex H + 1 (rows shifted by 6 ARE the next hex) - against taps [3 K / 8][8][N][8]
  // (W6_EPI_MASK7 / _MASK7F, tl_conv7_wino63v_dgrad_nt: the same K loop under the MASK epilogue - the input gradient of such a
  // convolution is a 7-tap convolution of the gradient rows moved down six rows, tl_wino63_xform2s)
  constexpr bool SEG3 = EPI == W_EPI_LRELU || EPI == W6_EPI_MASK7 || EPI == W6_EPI_MASK7F;
  // EPI == GY (tl_conv1_wino63v_dgrad_nt): transforms 6, 7 of both operands are zero - the six-batch K loop (V6K6_*: half-set H =
  // transforms 4, 5; 24 MFMAs per K-step), and waves 6, 7 fetch through empty resources (their planes are never read)
  constexpr bool SIX = EPI == W_EPI_GY || EPI == W6_EPI_GY_Y;
  const int kseg = p.K / V6_BK;                            // K-steps per segment (host-checked: K % 8 == 0)
  const int nsteps = SEG3 ? 3 * kseg : kseg;               // host-checked: >= 5
  // Accumulators and fragments live in FIXED registers (tonal_wino63_kloop.h: v0 - v127, v128 - v191): every K-step is one asm
  // statement tied to them, the epilogues read `acc` where the last statement left it.
  f32x16 acc[8];
  f32x4 faL[4], fbL[4], faH[4], fbH[4];

  // ---- LDS-DMA plan.  Piece = 32 rows x 32 B; lane -> (row = lane >> 1, physical chunk = lane & 1); the source chunk
  // is the swizzled one, chunk ^ ((row >> 3) & 1).  Wave w fetches transform w: its four 32-hex blocks of A and its two
  // 32-column blocks of B: LDS destinations (wave w, piece t) = stage + (w 128 + 32 t) 32 B for A, + 32 KB + (w 64 + 32 t) 32 B
  // for B - M0 of the first piece of each kind, + 1 KB per further piece.
  const int prow = lane >> 1;
  const int src_chunk = (lane & 1) ^ ((lane >> 4) & 1);
  const v6_i32x4 rsB = v6_rsrc_words(p.Bw, (SIX && wave >= 6) ? 0 : 8LL * p.N * p.ldb * 4);
  const unsigned lds0 = (unsigned)(unsigned long long)(lds_void6_t*)lds;        // LDS byte address of the first stage
  const unsigned dst_a0 = lds0 + (unsigned)(wave * V6_BH * V6_ROWB);
  const unsigned dst_b0 = lds0 + (unsigned)(V6_A_BYTES + wave * V6_BN * V6_ROWB);
  // LDS row rho = 8 g + 4 lh' + j' of a wave's 32 (the MFMA row whose results lane half lh' holds in accumulator elements
  // 4 g + j') takes hex 16 lh' + 4 g + j': a lane owns 16 consecutive hexes (tonal_wino63_epi.h)
  const int hex_of_row = (prow & 3) | ((prow >> 3) << 2) | (((prow >> 2) & 1) << 4);
  // sources: V in the pair layout (K-step s = its 8-channel chunk s: + 512 B), taps chunk-major (+ 256 N bytes per step)
  const int kc8 = p.lda >> 3;
  // compact-M mode (tl_nt_params.a_hps_extra = x > 0; host-checked: 16 computed hexes per sequence): V stores 16 + x hexes per
  // sequence, hex c of a tile lies at storage hex c + (c / 16) x - a per-lane constant like the offsets themselves - and a
  // tile (eight sequences) starts 8 (16 + x) hexes behind the one before.  x = 0: the offsets and the tile step as they were.
  const int hx = p.a_hps_extra;
  unsigned avoff[4], bv_lane[2];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = t * 32 + hex_of_row;
    avoff[t] = (unsigned)(v6_at(c + (c >> 4) * hx, wave, src_chunk * 4, kc8) * 4);
  }
  unsigned avoff1[4];                                      // the same pieces one hex on (SEG3, third segment)
#pragma unroll
  for (int t = 0; t < 4; ++t) avoff1[t] = SEG3 ? (unsigned)(v6_at(t * 32 + hex_of_row + 1, wave, src_chunk * 4, kc8) * 4) : avoff[t];
#pragma unroll
  for (int t = 0; t < 2; ++t) bv_lane[t] = (unsigned)((((long long)wave * p.N + t * 32 + prow) * 8 + src_chunk * 4) * 4);
  const unsigned b_step = (unsigned)p.N * 256u;

  // A workgroup walks the tiles blockIdx.x, + gridDim.x, ... (one workgroup per CU, a multiple of 8: a tile sequence stays
  // on one XCD).  V holds whole 128-hex tiles (host-checked): the per-lane source offsets of the A pieces never change.
  struct tile_t {
    long long tm, R0;
    int n0;
    v6_i32x4 rsA, rsA1;
    unsigned bvoff[2];
  };
  const long long a_tile_bytes = (long long)(V6_BH + 8 * hx) * 8 * p.lda * 4, a_total_bytes = p.A_rows * 8LL * p.lda * 4;
  auto place = [&](tile_t& t, long long tm, int tn) {
    t.tm = tm;
    t.R0 = tm * V6_ROWS;
    t.n0 = tn * V6_BN;
    const long long ab = tm * a_tile_bytes;
    t.rsA = v6_rsrc_words(reinterpret_cast<const char*>(p.A) + ab, (SIX && wave >= 6) ? 0 : a_total_bytes - ab);
    t.rsA1 = SEG3 ? v6_rsrc_words(reinterpret_cast<const char*>(p.aux) + ab, a_total_bytes - ab) : t.rsA;
    if (t.n0 + V6_BN <= p.N) {
      const unsigned nb4 = (unsigned)t.n0 * 32u;
#pragma unroll
      for (int k = 0; k < 2; ++k) t.bvoff[k] = bv_lane[k] + nb4;
    } else {                                               // column tile past the edge: clamped columns (masked by the epilogue)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        int n = t.n0 + k * 32 + prow;
        if (n > p.N - 1) n = p.N - 1;
        t.bvoff[k] = (unsigned)((((long long)wave * p.N + n) * 8 + src_chunk * 4) * 4);
      }
    }
  };
  tile_t cur;
  {
    long long bid = blockIdx.x;
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    place(cur, bid / ntn, (int)(bid % ntn));
  }
  // next tile without divisions: with a persistent launch of 8 k workgroups the XCD-aware remap sends tile sequence
  // blockIdx.x + j gridDim.x to b' + j gridDim.x / 8, so (tm, tn) advance by a fixed pair with a carry
  const int walk = (int)(gridDim.x >> 3), walk_q = walk / ntn, walk_r = walk - walk_q * ntn;
  auto advance = [&](const tile_t& c) -> tile_t {
    tile_t t = c;
    int tn = c.n0 / V6_BN + walk_r;
    long long tm = c.tm + walk_q;
    if (tn >= ntn) {
      tn -= ntn;
      ++tm;
    }
    place(t, tm, tn);
    return t;
  };
  auto next3 = [](int s) { return s == 2 ? 0 : s + 1; };

  // ---- fragment reads: row r of a plane, logical chunk lh -> r * 32 + ((lh ^ ((r >> 3) & 1)) << 4)
  const int cphys = (lh ^ ((lr >> 3) & 1)) << 4;
  const unsigned a_row = lds0 + (unsigned)((wm * 32 + lr) * V6_ROWB + cphys);
  const unsigned b_row = lds0 + (unsigned)((wn * 32 + lr) * V6_ROWB + cphys);     // (+ 32 KB: in the instructions' offsets)
  int stg = 0;                                             // stage of the K-step about to run (rolls on across tiles)

  // The operands every K-step statement shares.  `step`: the K-step whose six pieces it issues (into stage `dst`); `wimm`: the
  // closing wait of the first step as an immediate.
  // where the six pieces of a K-step come from: resource and per-lane offsets of the A pieces, scalar offsets of both kinds
  struct dma_src {
    v6_i32x4 ra;
    unsigned va[4], vb[2], sa, sb;
  };
  auto src_of = [&](const tile_t& t, int step) {
    dma_src d;
    int ks = step;
    if constexpr (SEG3) {                                  // (selects, no branches: see the K loop below)
      const int seg = (step >= kseg ? 1 : 0) + (step >= 2 * kseg ? 1 : 0);
      ks = step - seg * kseg;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        d.ra[k] = seg == 1 ? t.rsA1[k] : t.rsA[k];
        d.va[k] = seg == 2 ? avoff1[k] : avoff[k];
      }
    } else {
      d.ra = t.rsA;
#pragma unroll
      for (int k = 0; k < 4; ++k) d.va[k] = avoff[k];
    }
    d.vb[0] = t.bvoff[0];
    d.vb[1] = t.bvoff[1];
    // (wave-uniform by construction; said explicitly: an "s" operand the compiler believes divergent is handed over in a VGPR)
#pragma unroll
    for (int k = 0; k < 4; ++k) d.ra[k] = __builtin_amdgcn_readfirstlane(d.ra[k]);
    d.sa = (unsigned)__builtin_amdgcn_readfirstlane(ks * 512);
    d.sb = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)step * b_step));
    return d;
  };
#define V6K_INPUTS(src, dst, wimm)                                                                                             \
  [a] "v"(a_row + (unsigned)stg * (unsigned)V6_STAGE), [b] "v"(b_row + (unsigned)stg * (unsigned)V6_STAGE),                    \
      [va0] "v"((src).va[0]), [va1] "v"((src).va[1]), [va2] "v"((src).va[2]), [va3] "v"((src).va[3]), [vb0] "v"((src).vb[0]), \
      [vb1] "v"((src).vb[1]), [ra] "s"((src).ra), [rb] "s"(rsB), [m0a] "s"(dst_a0 + (unsigned)(dst) * (unsigned)V6_STAGE),     \
      [m0b] "s"(dst_b0 + (unsigned)(dst) * (unsigned)V6_STAGE), [sa] "s"((src).sa), [sb] "s"((src).sb), [w] "n"(wimm)
  // (clobbers: the statements advance M0 with s_add_u32, which writes SCC - a compare the compiler placed in front of a
  // statement must not be consumed behind it.  M0 is written inside the statements and named as a clobber too, so that an
  // M0 initialisation the compiler makes for a consumer of its own is never assumed to survive one of them;
  // clang remarks that M0 is a reserved register - the clobber is recorded all the same and the generated code is unchanged,
  // profiles/r05_kernel_resources.md - hence the diagnostic pragma)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define V6K_STMT_R(REGS, TEXT, tl_, step, dst, wimm)                                                                     \
  do {                                                                                                                   \
    const dma_src src_ = src_of(tl_, step);                                                                              \
    asm volatile(TEXT : REGS(acc, faL, fbL, faH, fbH) : V6K_INPUTS(src_, dst, wimm) : "memory", "scc", "m0");                  \
  } while (0)
#define V6K_STMT(TEXT, tl_, step, dst, wimm) V6K_STMT_R(V6K_REGS, TEXT, tl_, step, dst, wimm)
  // the six LDS-DMA pieces of K-step `step` of tile tl_ into stage `dst` (no MFMAs, no vector operands: the first two stages
  // of a tile, issued in front of the epilogue of the tile before - which must not see fragments or accumulators as live)
  auto issue = [&](const tile_t& tl_, int step, int dst) {
    const dma_src src_ = src_of(tl_, step);
    asm volatile(V6K_ISSUE : : V6K_INPUTS(src_, dst, 0) : "memory", "scc", "m0");
  };
  // The reads of H between L's MFMAs: one per MFMA in the first half of L's window, so that the last eight MFMAs cover their
  // latency behind the barrier - for the conv2 launches (POOLV, fused conv1 gradient: -0.5 / -0.4 ms, same-call A/B, twice);
  // the instantiations of conv3 (POOL, MASKY) measured +0.2 ms with it and keep one read per two MFMAs
  constexpr bool early = EPI == W_EPI_POOLV || EPI == W_EPI_C1W || EPI == W6_EPI_C1W_Y;
  constexpr int NST = v6_stores<EPI>();
  constexpr int first_n = NST + 6 > 63 ? 63 : NST + 6;
  constexpr int first_wait = (first_n & 15) | (7 << 4) | (0 << 8) | ((first_n >> 4) << 14);       // vmcnt(n) lgkmcnt(0)

  // the first tile's first two stages
  issue(cur, 0, 0);
  issue(cur, 1, 1);
  __builtin_amdgcn_s_waitcnt(0x0f70);                       // vmcnt(0)
  for (long long vb = blockIdx.x; vb < nwg; vb += gridDim.x) {
    // stage stg of this tile has landed (waited for at the end of the tile in front), every wave is past that epilogue
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // What the epilogue reads from global memory is requested in front of the LAST K-step (tonal_wino43v.hip)
    auto prefetch = [&] {
      if constexpr (EPI == W_EPI_POOL || EPI == W_EPI_POOLV || EPI == W_EPI_LRELU) return v5_prefetch_pool(p, cur.n0, wn, lr);
      else if constexpr (EPI == W_EPI_MASK || EPI == W6_EPI_MASK7) return v6_prefetch_mask(p, cur.R0, cur.n0, wm, wn, lr, lh);
      else if constexpr (EPI == W6_EPI_MASK7F) return v6_pre_mask{{0u, 0u, 0u}};      // (float rows: read by the epilogue itself)
      else if constexpr (EPI == W_EPI_MASKY || EPI == W6_EPI_MASKY_Y) return v6_prefetch_masky(p, cur.R0, cur.n0, wm, wn, lr, lh);
      else if constexpr (EPI == W_EPI_GY || EPI == W6_EPI_GY_Y) return v6_prefetch_masky<true>(p, cur.R0, cur.n0, wm, wn, lr, lh);
      else if constexpr (EPI == W6_EPI_MASKY_SEQ) return v6_prefetch_masky_seq(p, cur.tm, cur.n0, wm, wn, lr, lh);
      else return v6_prefetch_c1w(p, cur.R0, cur.n0, wm, wn, lr, lh);
    };
    decltype(prefetch()) pre;
    // ---- K loop.  Step 0 has no carried half-set (its L starts accumulators 0-3 from zero, its H is read and runs in step
    // 1, which starts 4-7 from zero); a step issues the pieces of the step two ahead into the stage released by the barrier in
    // front of it; the pieces of step 1 went out in front of the previous tile's epilogue: between them and step 0's pieces
    // sit that epilogue's stores, which the closing wait of step 0 leaves in flight (first_wait).
    // (V6K_RUN: the statement of one K-step in the form this instantiation runs - six-batch, early or late fragment reads)
#define V6K_RUN(KIND, RSFX, tl_, step, dst, wimm)                                                                              \
  do {                                                                                                                         \
    if constexpr (SIX) V6K_STMT_R(V6K6_REGS##RSFX, V6K6_##KIND##_L, tl_, step, dst, wimm);                                     \
    else if constexpr (early) V6K_STMT_R(V6K_REGS##RSFX, V6K_##KIND##_E, tl_, step, dst, wimm);                                \
    else V6K_STMT_R(V6K_REGS##RSFX, V6K_##KIND##_L, tl_, step, dst, wimm);                                                     \
  } while (0)
    if constexpr (SIX) V6K_STMT_R(V6K6_REGS_FIRST, V6K6_FIRST, cur, 2, stg == 0 ? 2 : stg - 1, first_wait);
    else V6K_STMT_R(V6K_REGS_FIRST, V6K_FIRST, cur, 2, stg == 0 ? 2 : stg - 1, first_wait);
    stg = next3(stg);
    // (straight-line control flow between the statements - nsteps >= 5 is host-checked, the steady-state loop runs at least
    // once: across a branch with two successors the allocator moves the pinned values out of their registers and back)
    V6K_RUN(STEP1, _STEP1, cur, 3, stg == 0 ? 2 : stg - 1, 0);
    stg = next3(stg);
    {
      int s = 2;
      do {
        V6K_RUN(NORM, , cur, s + 2, stg == 0 ? 2 : stg - 1, 0);
        stg = next3(stg);
      } while (++s + 2 < nsteps);
    }
    V6K_RUN(PRELAST, , cur, 0, 0, 0);
    stg = next3(stg);
    pre = prefetch();
    V6K_RUN(LAST, , cur, 0, 0, 0);
    stg = next3(stg);
#undef V6K_RUN

    // The first two K-steps of the next tile go into the two stages that are NOT the last step's: stg (read in step
    // nsteps - 3) and stg + 1 (step nsteps - 2) - every wave is past the barrier that closed step nsteps - 2.  The last
    // step's stage (stg + 2) is still being read by slower waves; it is the epilogue's scratch behind a barrier.
    const tile_t done = cur;
    const long long nb = vb + gridDim.x;
    const int last_stage = stg == 0 ? 2 : stg - 1;
    // the prefetched words have landed (requested a K-step ago; nothing else is in flight)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    if (nb < nwg) {
      cur = advance(cur);
      issue(cur, 0, stg);
      issue(cur, 1, next3(stg));
    }
    __builtin_amdgcn_sched_barrier(0);
    float* scratch = reinterpret_cast<float*>(lds + last_stage * V6_STAGE);
    (void)scratch;
    const bool full = done.R0 + V6_ROWS <= p.M && done.n0 + V6_BN <= p.N;
    if constexpr (EPI == W_EPI_POOL) {
      if (full) v6_epilogue_pool<false, true>(p, acc, pre, nullptr, done.R0, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_pool<false, false>(p, acc, pre, nullptr, done.R0, done.n0, wm, wn, lr, lh, done.tm);
    } else if constexpr (EPI == W_EPI_POOLV) {
      float* xch = reinterpret_cast<float*>(lds + 3 * V6_STAGE);
      if (full) v6_epilogue_pool<true, true>(p, acc, pre, xch, done.R0, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_pool<true, false>(p, acc, pre, xch, done.R0, done.n0, wm, wn, lr, lh, done.tm);
    } else if constexpr (EPI == W_EPI_LRELU) {
      if (full) v6_epilogue_lrelu<true>(p, acc, pre, done.R0, done.n0, wm, wn, lr, lh);
      else v6_epilogue_lrelu<false>(p, acc, pre, done.R0, done.n0, wm, wn, lr, lh);
    } else if constexpr (EPI == W_EPI_MASK || EPI == W6_EPI_MASK7) {
      if (full) v6_epilogue_mask<true>(p, acc, pre, done.R0, done.n0, wm, wn, lr, lh);
      else v6_epilogue_mask<false>(p, acc, pre, done.R0, done.n0, wm, wn, lr, lh);
    } else if constexpr (EPI == W6_EPI_MASK7F) {
      if (full) v6_epilogue_mask<true, true>(p, acc, pre, done.R0, done.n0, wm, wn, lr, lh);
      else v6_epilogue_mask<false, true>(p, acc, pre, done.R0, done.n0, wm, wn, lr, lh);
    } else if constexpr (EPI == W_EPI_MASKY) {
      float* xch = reinterpret_cast<float*>(lds + 3 * V6_STAGE);
      if (full) v6_epilogue_masky<true>(p, acc, pre, xch, done.R0, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_masky<false>(p, acc, pre, xch, done.R0, done.n0, wm, wn, lr, lh, done.tm);
    } else if constexpr (EPI == W6_EPI_MASKY_Y) {
      if (full) v6_epilogue_masky<true, false, false>(p, acc, pre, nullptr, done.R0, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_masky<false, false, false>(p, acc, pre, nullptr, done.R0, done.n0, wm, wn, lr, lh, done.tm);
    } else if constexpr (EPI == W_EPI_GY) {
      float* xch = reinterpret_cast<float*>(lds + 3 * V6_STAGE);
      if (full) v6_epilogue_masky<true, true>(p, acc, pre, xch, done.R0, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_masky<false, true>(p, acc, pre, xch, done.R0, done.n0, wm, wn, lr, lh, done.tm);
    } else if constexpr (EPI == W6_EPI_GY_Y) {
      if (full) v6_epilogue_masky<true, true, false>(p, acc, pre, nullptr, done.R0, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_masky<false, true, false>(p, acc, pre, nullptr, done.R0, done.n0, wm, wn, lr, lh, done.tm);
    } else if constexpr (EPI == W6_EPI_MASKY_SEQ) {
      if (full) v6_epilogue_masky_seq<true>(p, acc, pre, done.n0, wm, wn, lr, lh, done.tm);
      else v6_epilogue_masky_seq<false>(p, acc, pre, done.n0, wm, wn, lr, lh, done.tm);
    } else {
      v6_epilogue_c1w<EPI == W6_EPI_C1W_Y>(p, acc, pre, reinterpret_cast<float*>(lds + 3 * V6_STAGE) + wave * 512, scratch, done.R0,
                                           done.n0, wm, wn, lr, lh, done.tm);
    }
    {
      // The next tile's first stage (issued in front of the epilogue) has landed; its second stage and the epilogue's own
      // stores need not: vmcnt counts in issue order (6 bits)
      constexpr int n = NST + 6 > 63 ? 63 : NST + 6;
      __builtin_amdgcn_s_waitcnt((n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14));
    }
  }
#pragma clang diagnostic pop
}



// ------------------------------------------------------------------------------------------
// Weight gradient on V, 128 (C_in) x 64 (C_out) tile, 8 waves, one workgroup per CU: wino43v_tn8_kernel with hexes.
// A K-step is SIX hexes (36 conv rows; three k-slices of two hexes): the V tile [8][6 hexes][64 channels] is exactly the
// 12 KB of the F(4,3) kernel's [6][8 quads][64], so ring, pieces (3 per wave), swizzle and fragment reads keep their
// shape; 24 MFMAs per wave and K-step as before, for 36 rows instead of 32.
//   * V: LDS-DMA, 4-slot ring, three steps ahead;
//   * the pooled gradient rows of a hex (3 h .. 3 h + 3: its own three and the first of the next hex - the row in front of
//     a hex, which Vd needs, is row 2 of the piece in front) by LDS-DMA, waves 0-5 one hex each, four steps ahead, 6-slot
//     ring; their arg-max words as one 4-byte-per-lane piece (waves 6, 7: the same one).  The gradient and its words live
//     in the row layout [seq * g_tp + t'] of the stage's OUTPUT (tl_tn_params.g_tp; 0: Tp / 2): a lane follows its hex
//     through the sequences with two counters;
//   * Y side: wave w < 6 owns hex w of the step, a lane one channel; the word pair of a pooled row is the lane mask of
//     the un-pool select; Y = A dy (8 values) to LDS, Vd = B^T (dZ rows 6 h - 2 .. 6 h + 5) transposed over groups of four
//     lanes and stored as two 16-byte buffer stores per lane, the C_in-tile workgroups of a (split, C_out tile) taking turns.
// ------------------------------------------------------------------------------------------
constexpr int T6_BN = 64, T6_H = 6;
constexpr int T6_PLANE = T6_H * 64;                       // floats per transform plane (384)
constexpr int T6_TILE = 8 * T6_PLANE;                     // floats per operand tile (12 KB)
constexpr int T6_NA = 4, T6_NG = 6;
constexpr int T6_GW = T6_H * 4 * 64;                      // floats of gradient rows per raw slot (6 hexes x 4 rows x 64)
constexpr int T6_GT = T6_GW + 64;                         // + 6 x 4 rows x 2 words (48 of 64 four-byte lanes)

template <bool WVD>
__global__ __launch_bounds__(512, 1) void wino63v_tn_kernel(const tl_tn_params p, int mtn) {
  constexpr int NA = T6_NA, NG = T6_NG, GW = T6_GW, GT = T6_GT;
  __shared__ __attribute__((aligned(1024))) float lds[(NA * 2 + 2) * T6_TILE + NG * GT];
  float* As = lds;                               // [4][2][8][6][64]  V ring (two 64-channel half-tiles)
  float* Bs = lds + NA * 2 * T6_TILE;            // [2][8][6][64]     Y
  float* Gs = Bs + 2 * T6_TILE;                  // [6]{[6 hexes][4 rows][64], [6][4][2 words]}
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
  const int ntn = p.Ndim / T6_BN;
  const long long tiles = (long long)mtn * ntn;
  const long long nwg = tiles * p.splitk;
  long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  {
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const int z = __builtin_amdgcn_readfirstlane((int)(bid / tiles));
  const int tt = __builtin_amdgcn_readfirstlane((int)(bid % tiles));
  const int mi = __builtin_amdgcn_readfirstlane(tt / ntn);                          // C_in tile of this workgroup
  const int m0 = mi * 128, n0 = __builtin_amdgcn_readfirstlane((tt % ntn) * T6_BN);

  const long long hexes_all = p.Krows / 6;
  const long long ksteps_all = (hexes_all + T6_H - 1) / T6_H;
  const long long per = __builtin_amdgcn_readfirstlane((int)((ksteps_all + p.splitk - 1) / p.splitk));
  const long long ks_begin = z * per;
  long long ks_end = ks_begin + per;
  if (ks_end > ksteps_all) ks_end = ksteps_all;
  const int nsteps = ks_end > ks_begin ? (int)(ks_end - ks_begin) : 0;

  f32x16 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  // ---- V by LDS-DMA: piece 3 wave + t -> half-tile pc / 12, rows 4 (pc % 12) .. + 3 of its 48 ([transform][hex] order);
  // lane -> (row offset lane >> 4, physical 16-byte chunk lane & 15); odd hexes: halves swapped = source chunk ^ 8
  const long long v_h0 = ks_begin * T6_H;                           // first hex of this split
  // (V in the pair layout: v_h0 is even, a K-step is three pairs; the channel tile enters through the chunk index)
  const int kc8 = p.lda >> 3;
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.A + v_h0 * 8 * (long long)p.lda), 0, clip31((p.A_rows - v_h0) * 8 * (long long)p.lda * 4), 0x00020000);
  unsigned vvoff[3], vdst[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int half = (wave * 3 + t) / 12, pc = (wave * 3 + t) % 12;
    const int rho = 4 * pc + (lane >> 4), i = rho / 6, hx = rho % 6;
    const int chunk = (lane & 15) ^ ((hx & 1) << 3);
    vvoff[t] = (unsigned)(v6_at(hx, i, m0 + half * 64 + chunk * 4, kc8) * 4);
    vdst[t] = (unsigned)((half * T6_TILE + pc * 256) * 4);
  }
  const unsigned v_step = (unsigned)(T6_H * 8 * p.lda * 4);         // bytes per K-step (host-checked to fit)
  auto issue_v = [&](int step) {
    char* base = reinterpret_cast<char*>(As) + (step & (NA - 1)) * (2 * T6_TILE * 4);
    const unsigned soff = (unsigned)step * v_step;          // (in the per-lane offset: that one is range-checked)
#pragma unroll
    for (int t = 0; t < 3; ++t) dma16h(rsV, base + vdst[t], vvoff[t] + soff, 0u);
  };
  // ---- raw pooled gradient rows and arg-max words by LDS-DMA.  A lane follows ITS hex of the step (waves 0-5: hex `wave`;
  // waves 6, 7: hex lane >> 3 for the word piece) through the G row layout: hs = hex index inside its sequence, goff = G
  // row of the hex's first pooled row relative to the first hex of the split.
  const int Tq = p.Tp >> 1, hps = p.Tp / 6;                        // pooled rows / hexes per sequence (hex layout)
  const int g_tp = p.g_tp > 0 ? p.g_tp : Tq;
  const bool wpiece = wave >= 6;
  const int myhex = wpiece ? (lane >> 3) : wave;                    // (lanes >= 48 of a word piece: never fetched)
  const long long seq0 = v_h0 / hps;
  const int hs0 = (int)(v_h0 - seq0 * hps);
  const long long g_r0 = seq0 * g_tp + 3LL * hs0;                   // G row of the split's first hex
  int g_hs = hs0 + myhex, g_off = 3 * myhex;
  while (g_hs >= hps) {
    g_hs -= hps;
    g_off += g_tp - Tq;
  }
  const int ldw4 = p.ld_bbits * 4;
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(
      wpiece ? (void*)(p.bbits + g_r0 * (long long)p.ld_bbits + (n0 >> 5)) : (void*)(p.B + g_r0 * (long long)p.ldb + n0), 0,
      wpiece ? clip31((p.B_rows - g_r0) * (long long)ldw4 - (long long)(n0 >> 5) * 4)
             : clip31((p.B_rows - g_r0) * (long long)p.ldb * 4 - (long long)n0 * 4),
      0x00020000);
  const unsigned g_lane = wpiece ? (unsigned)(((lane >> 1) & 3) * ldw4 + (lane & 1) * 4)
                                 : (unsigned)(((lane >> 4) * (long long)p.ldb + (lane & 15) * 4) * 4);
  const unsigned g_row4 = wpiece ? (unsigned)ldw4 : (unsigned)(p.ldb * 4);
  const unsigned gdst = wpiece ? (unsigned)(GW * 4) : (unsigned)(wave * 256 * 4);
  const bool g_live = !wpiece || lane < 48;
  auto issue_g = [&](int slot) {                                    // the piece of the NEXT step in line; advances the counters
    const unsigned voff = g_live ? (unsigned)g_off * g_row4 + g_lane : 0xfffffff0u;
    if (wpiece) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsG, (lds_void6_t*)(reinterpret_cast<char*>(Gs) + slot * (GT * 4) + gdst), 4, voff, 0u, 0, 0);
    else dma16h(rsG, reinterpret_cast<char*>(Gs) + slot * (GT * 4) + gdst, voff, 0u);
    g_hs += T6_H;
    g_off += 3 * T6_H;
    while (g_hs >= hps) {
      g_hs -= hps;
      g_off += g_tp - Tq;
    }
  };
  auto next6 = [](int v) { return v == NG - 1 ? 0 : v + 1; };

  // ---- Y side: wave w < 6 = hex w of the K-step, lane = channel ----
  constexpr bool write_vd = WVD;
  const bool ywave = wave < T6_H;
  const int sw = lane ^ ((wave & 1) << 5);                  // swizzled channel position inside the 64-wide row
  int tq = __builtin_amdgcn_readfirstlane((int)((6 * (v_h0 + (ywave ? wave : 0))) % p.Tp));   // first conv row of the NEXT hex to transform
  const int dstep = __builtin_amdgcn_readfirstlane((6 * T6_H) % p.Tp);
  float bsum = 0.f;
  // Vd in the pair layout (ld_vd / 8 chunks): a lane stores four channels of transforms lane & 3 and 4 + (lane & 3)
  const int kcd = write_vd ? (p.ld_vd >> 3) : 1;
  const unsigned vd_pstride = (unsigned)(16 * p.ld_vd * 4);          // bytes per hex pair
  const long long vd_hexes = ((hexes_all + 1) >> 1) << 1;
  const __amdgpu_buffer_rsrc_t rsVd = __builtin_amdgcn_make_buffer_rsrc(
      write_vd ? (void*)(p.vd + v_h0 * 8 * (long long)p.ld_vd) : (void*)p.slab, 0,
      write_vd ? clip31((vd_hexes - v_h0) * 8 * (long long)p.ld_vd * 4) : 0, 0x00020000);
  const unsigned vdA_lane = (unsigned)(v6_at(0, lane & 3, n0 + (lane & ~3), kcd) * 4);
  const unsigned vdB_lane = vdA_lane + 4u * 64u;
  const int nhex = (int)hexes_all, h_first = (int)v_h0;
  const int h_end = h_first + nsteps * T6_H;
  const int hs_lim = nhex < h_end ? nhex : h_end;           // hexes of this split that exist
  struct y_in {
    float g[3];
    unsigned long long mo[3], me[3];
    int tq;               // time index of the hex's first conv row
  };
  struct y_out {
    float d[6];           // dZ rows 6 h .. 6 h + 5
  };
  auto uni = [](unsigned long long v) -> unsigned long long {   // a wave-uniform value out of vector registers
    return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |
           ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32);
  };
  const int wy = ywave ? wave : 0;                          // (waves 6, 7 run the same code on hex 0's data with all-zero masks)
  auto fetch_y = [&](int sd, int slot, y_in& y) {
    const int h = h_first + sd * T6_H + wy;
    const int live = ywave & (h < hs_lim);
    const float* gs = Gs + slot * GT;
    const unsigned long long* ws = reinterpret_cast<const unsigned long long*>(gs + GW) + wy * 4;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      y.g[r] = gs[wy * 256 + r * 64 + lane];
      const unsigned long long w = uni(ws[r]);
      const int v = live & (tq + 2 * r < p.Tvalid);
      y.mo[r] = v ? w : 0ull;
      y.me[r] = v ? ~w : 0ull;
    }
    y.tq = tq;
    tq += dstep;
    if (tq >= p.Tp) tq -= p.Tp;
  };
  auto compute_y = [&](int sd, const y_in& y) -> y_out {
    y_out u;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u.d[2 * r] = selm0(y.me[r], y.g[r]);
      u.d[2 * r + 1] = selm0(y.mo[r], y.g[r]);
    }
    const float ev1 = (u.d[0] + u.d[2]) + u.d[4], od1 = (u.d[1] + u.d[3]) + u.d[5];
    const float ev2 = fmaf(16.f, u.d[4], fmaf(4.f, u.d[2], u.d[0])), od2 = fmaf(32.f, u.d[5], fmaf(8.f, u.d[3], 2.f * u.d[1]));
    const float ev3 = fmaf(0.0625f, u.d[4], fmaf(0.25f, u.d[2], u.d[0])), od3 = fmaf(0.03125f, u.d[5], fmaf(0.125f, u.d[3], 0.5f * u.d[1]));
    float o[8];
    o[0] = u.d[0];
    o[1] = ev1 + od1;
    o[2] = ev1 - od1;
    o[3] = ev2 + od2;
    o[4] = ev2 - od2;
    o[5] = ev3 + od3;
    o[6] = ev3 - od3;
    o[7] = u.d[5];
    bsum += o[1];
    if (ywave) {
      float* dst = Bs + (sd & 1) * T6_TILE + wave * 64 + sw;
#pragma unroll
      for (int i = 0; i < 8; ++i) dst[i * T6_PLANE] = o[i];
    }
    return u;
  };
  typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
  // Vd of the hexes of step sd.  gp / wp: the pooled row in front of the hex (conv rows 6 h - 2, 6 h - 1) and its word pair
  auto vd_part = [&](int sd, int tqc, const y_out& u, float gp, unsigned long long wp) {
    const int h = h_first + sd * T6_H + wy;
    const int vp = ywave & (tqc >= 2) & (tqc - 2 < p.Tvalid) & (h < hs_lim);
    float d[8], v[8];
    d[1] = selm0(vp ? wp : 0ull, gp);
    d[0] = selm0(vp ? ~wp : 0ull, gp);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[2 + k] = u.d[k];
    wino63_bt(d, v);
    // two 4 x 4 transposes over the lanes of a group (register n of lane r <- register r of lane n)
    const bool odd = lane & 1, hi = lane & 2;
    auto xch = [](float x, auto CTRL) -> float {
      return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), decltype(CTRL)::value, 0xf, 0xf, true));
    };
    using X1 = std::integral_constant<int, 0xB1>;         // quad_perm [1,0,3,2]
    using X2 = std::integral_constant<int, 0x4E>;         // quad_perm [2,3,0,1]
    auto stage = [&](float& a, float& b, bool up, auto CTRL) {
      const float r = xch(up ? a : b, CTRL);
      a = up ? r : a;
      b = up ? b : r;
    };
#pragma unroll
    for (int g4 = 0; g4 < 8; g4 += 4) {
      stage(v[g4 + 0], v[g4 + 1], odd, X1{});
      stage(v[g4 + 2], v[g4 + 3], odd, X1{});
      stage(v[g4 + 0], v[g4 + 2], hi, X2{});
      stage(v[g4 + 1], v[g4 + 3], hi, X2{});
    }
    const f32x4 va4 = {v[0], v[1], v[2], v[3]};
    const f32x4 vb4 = {v[4], v[5], v[6], v[7]};
    const bool ok = ywave && h < hs_lim;
    const unsigned hoff = (unsigned)((h - h_first) >> 1) * vd_pstride + (unsigned)((h - h_first) & 1) * 32u;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, va4), rsVd, ok ? hoff + vdA_lane : 0xfffffff0u, 0u, 2);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, vb4), rsVd, ok ? hoff + vdB_lane : 0xfffffff0u, 0u, 2);
  };
  // the row in front of this wave's hex at step sd: row 2 of the piece in front (hex wave - 1; for wave 0 the last hex
  // of the previous step, still in the ring)
  auto front_row = [&](int slot, int pslot, float& gp, unsigned long long& wp) {
    const int s_ = wy > 0 ? slot : pslot, hx = wy > 0 ? wy - 1 : T6_H - 1;
    gp = Gs[s_ * GT + hx * 256 + 128 + lane];
    wp = uni(reinterpret_cast<const unsigned long long*>(Gs + s_ * GT + GW)[hx * 4 + 2]);
  };

  // ---- MFMA side: k-slice sl of a K-step = hexes 2 sl (lanes 0-31) and 2 sl + 1 (lanes 32-63) ----
  const int a_off = (wm >> 1) * T6_TILE + lh * 64 + (((wm & 1) * 32 + lr) ^ (lh << 5));
  const int b_off = lh * 64 + ((wn * 32 + lr) ^ (lh << 5));
  float fa0[8], fb0[8], fa1[8], fb1[8], fac[8], fbc[8];     // slices 0, 1 of a step; slice 2, carried
  auto load_frag = [&](float (&fa)[8], float (&fb)[8], int abuf, int bbuf, int sl) {
    const float* a_s = As + abuf * (2 * T6_TILE) + sl * 128 + a_off;
    const float* b_s = Bs + bbuf * T6_TILE + sl * 128 + b_off;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      fa[i] = a_s[i * T6_PLANE];
      fb[i] = b_s[i * T6_PLANE];
    }
  };
  auto mfma8 = [&](const float (&fa)[8], const float (&fb)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[i], acc[i], 0, 0, 0);
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) fac[i] = fbc[i] = 0.f;

  {   // (also for an empty split: every access is clamped by its resource, the masks are all zero)
    issue_v(0);
    issue_v(1);
    issue_v(2);
    issue_g(0);
    issue_g(1);
    issue_g(2);
    issue_g(3);
    // the pooled row in front of the split's first hex (wave 0 only needs it, for Vd; everyone loads it - uniform code)
    float gp0 = 0.f;
    unsigned long long wp0 = 0ull;
    if (write_vd && hs0 > 0) {
      const long long pr = g_r0 - 1;                          // same sequence as the first hex (hs0 > 0)
      if (pr < p.B_rows) {
        gp0 = p.B[pr * (long long)p.ldb + n0 + lane];
        const uint32_t* wsrc = p.bbits + pr * (long long)p.ld_bbits + (n0 >> 5);
        wp0 = (unsigned long long)wsrc[0] | ((unsigned long long)wsrc[1] << 32);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    {
      y_in y0;
      fetch_y(0, 0, y0);
      const y_out u0 = compute_y(0, y0);
      if (write_vd && mi == 0) {
        float gp;
        unsigned long long wp;
        front_row(0, NG - 1, gp, wp);                         // (wave 0 reads an unwritten slot here: replaced below)
        if (wave == 0) {
          gp = gp0;
          wp = uni(wp0);
        }
        vd_part(0, y0.tq, u0, gp, wp);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  int slot1 = 1, slot4 = 4;                                 // ring slots of steps s + 1 and s + 4
  int turn = mtn > 1 ? 1 : 0;                               // (s + 1) % mtn: whose turn it is to write Vd for step s + 1
  for (int s = 0; s < nsteps; ++s) {
    const int abuf = s & (NA - 1), bbuf = s & 1;
    const int slot0 = slot1 == 0 ? NG - 1 : slot1 - 1;
    __builtin_amdgcn_sched_barrier(0);
    issue_v(s + 3);
    issue_g(slot4);
    load_frag(fa0, fb0, abuf, bbuf, 0);
    mfma8(fac, fbc);                                        // slice 2 of the previous step
    load_frag(fa1, fb1, abuf, bbuf, 1);
    mfma8(fa0, fb0);
    __builtin_amdgcn_sched_barrier(0);
    // second half: the transform of step s + 1 beside the MFMAs of slice 1
    load_frag(fac, fbc, abuf, bbuf, 2);
    if (ywave) {                                            // (wave-uniform: waves 6, 7 own no hex)
      y_in yn;
      fetch_y(s + 1, slot1, yn);
      const y_out un = compute_y(s + 1, yn);
      if constexpr (write_vd) {
        if (turn == mi && s + 1 < nsteps) {
          float gp;
          unsigned long long wp;
          front_row(slot1, slot0, gp, wp);
          vd_part(s + 1, yn.tq, un, gp, wp);
        }
      }
    }
    if constexpr (write_vd) turn = turn + 1 == mtn ? 0 : turn + 1;
    mfma8(fa1, fb1);
    __builtin_amdgcn_sched_barrier(0);                      // (the closing wait would be hoisted over these MFMAs)
    // everything issued up to step s - 2 has landed: V(s + 1), G(s + 2).  In flight: the 4 pieces of this step and of the
    // one before (a Vd store among them only makes the wait reach further back)
    __builtin_amdgcn_s_waitcnt(0x0078);                           // vmcnt(8) lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    slot1 = next6(slot1);
    slot4 = next6(slot4);
  }
  mfma8(fac, fbc);

  if (p.colsum != nullptr && m0 == 0) {
    __syncthreads();
    float* red = lds;
    red[wave * 64 + lane] = ywave ? bsum : 0.f;
    __syncthreads();
    if (tid < 64) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < T6_H; ++q) t += red[q * 64 + tid];
      p.colsum[(long long)z * p.Ndim + n0 + tid] = t;
    }
  }
  float* out = p.slab + (long long)z * p.slab_stride;
  const int col = n0 + wn * 32 + lr;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      out[((long long)i * p.Mdim + m) * (long long)p.ldc + col] = acc[i][e];
    }
}

// ------------------------------------------------------------------------------------------
// The same weight gradient with the eight transforms split over TWO workgroups: tile 256 (C_in) x 64 (C_out) x FOUR
// transforms.  What bounds the kernel above is the Y side - every workgroup of a (split, C_out tile) rebuilds the whole
// Y = A dy tile, and on gfx950 that vector work displaces matrix work one for one (measured: 9.8 of 46.0 ms at conv2).
// Here a workgroup builds only the four Y planes of its transforms for the same 24 MFMAs per wave and K-step: the
// un-pool selects are shared, the output arithmetic halves, the Y stores halve, the B fragments halve (12 reads per
// slice instead of 16); V tile, rings and pieces keep their sizes ([4][6 hexes][256 channels] = the 24 KB of [8][6][128]).
// Selected where C_in is a multiple of 256.  Same k order per accumulator as the kernel above: bit-identical results.
// ------------------------------------------------------------------------------------------
template <bool WVD>
__global__ __launch_bounds__(512, 1) void wino63v_tn4_kernel(const tl_tn_params p, int mtn) {
  constexpr int NA = T6_NA, NG = T6_NG, GW = T6_GW, GT = T6_GT;
  constexpr int QT = 4 * T6_PLANE;               // floats per quarter-tile of V / per Y tile: [4 transforms][6 hexes][64]
  __shared__ __attribute__((aligned(1024))) float lds[(NA * 4 + 2) * QT + NG * GT + 2 * QT];
  float* As = lds;                               // [4][4][4][6][64]  V ring (four 64-channel quarter-tiles, four transforms)
  float* Bs = lds + NA * 4 * QT;                 // [2][4][6][64]     Y
  float* Gs = Bs + 2 * QT;                       // [6]{[6 hexes][4 rows][64], [6][4][2 words]}
  float* Ydummy = Gs + NG * GT;                  // where waves 6, 7 (no hex of their own) put their Y: no branch in the K-step
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
  const int ntn = p.Ndim / T6_BN;
  const long long tiles = 2LL * mtn * ntn;        // (transform half, C_in tile, C_out tile)
  const long long nwg = tiles * p.splitk;
  long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  {
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const int z = __builtin_amdgcn_readfirstlane((int)(bid / tiles));
  const int tt = __builtin_amdgcn_readfirstlane((int)(bid % tiles));
  // (the workgroups of one (split, C_out tile) are neighbours: they share the gradient rows through the L2 and take turns at Vd)
  const int mi = __builtin_amdgcn_readfirstlane(tt % (2 * mtn));                    // slot among them: 2 x C_in tile + transform half
  const int th = mi & 1, i0 = 4 * th;                                               // this workgroup's transforms: i0 .. i0 + 3
  const int m0 = (mi >> 1) * 256, n0 = __builtin_amdgcn_readfirstlane((tt / (2 * mtn)) * T6_BN);
  const int nslots = 2 * mtn;

  const long long hexes_all = p.Krows / 6;
  const long long ksteps_all = (hexes_all + T6_H - 1) / T6_H;
  const long long per = __builtin_amdgcn_readfirstlane((int)((ksteps_all + p.splitk - 1) / p.splitk));
  const long long ks_begin = z * per;
  long long ks_end = ks_begin + per;
  if (ks_end > ksteps_all) ks_end = ksteps_all;
  const int nsteps = ks_end > ks_begin ? (int)(ks_end - ks_begin) : 0;

  f32x16 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  // ---- V by LDS-DMA: piece 3 wave + t -> quarter-tile pc / 6, rows 4 (pc % 6) .. + 3 of its 24 ([transform][hex] order);
  // lane -> (row offset lane >> 4, physical 16-byte chunk lane & 15); odd hexes: halves swapped = source chunk ^ 8
  const long long v_h0 = ks_begin * T6_H;                           // first hex of this split
  // (V in the pair layout: v_h0 is even, a K-step is three pairs; the channel tile enters through the chunk index)
  const int kc8 = p.lda >> 3;
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.A + v_h0 * 8 * (long long)p.lda), 0, clip31((p.A_rows - v_h0) * 8 * (long long)p.lda * 4), 0x00020000);
  unsigned vvoff[3], vdst[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int quarter = (wave * 3 + t) / 6, pc = (wave * 3 + t) % 6;
    const int rho = 4 * pc + (lane >> 4), i = rho / 6, hx = rho % 6;
    const int chunk = (lane & 15) ^ ((hx & 1) << 3);
    vvoff[t] = (unsigned)(v6_at(hx, i0 + i, m0 + quarter * 64 + chunk * 4, kc8) * 4);
    vdst[t] = (unsigned)((quarter * QT + pc * 256) * 4);
  }
  const unsigned v_step = (unsigned)(T6_H * 8 * p.lda * 4);         // bytes per K-step (host-checked to fit)
  auto issue_v = [&](int step) {
    char* base = reinterpret_cast<char*>(As) + (step & (NA - 1)) * (4 * QT * 4);
    const unsigned soff = (unsigned)step * v_step;          // (in the per-lane offset: that one is range-checked)
#pragma unroll
    for (int t = 0; t < 3; ++t) dma16h(rsV, base + vdst[t], vvoff[t] + soff, 0u);
  };
  // ---- raw pooled gradient rows and arg-max words by LDS-DMA.  A lane follows ITS hex of the step (waves 0-5: hex `wave`;
  // waves 6, 7: hex lane >> 3 for the word piece) through the G row layout: hs = hex index inside its sequence, goff = G
  // row of the hex's first pooled row relative to the first hex of the split.
  const int Tq = p.Tp >> 1, hps = p.Tp / 6;                        // pooled rows / hexes per sequence (hex layout)
  const int g_tp = p.g_tp > 0 ? p.g_tp : Tq;
  const bool wpiece = wave >= 6;
  const int myhex = wpiece ? (lane >> 3) : wave;                    // (lanes >= 48 of a word piece: never fetched)
  const long long seq0 = v_h0 / hps;
  const int hs0 = (int)(v_h0 - seq0 * hps);
  const long long g_r0 = seq0 * g_tp + 3LL * hs0;                   // G row of the split's first hex
  int g_hs = hs0 + myhex, g_off = 3 * myhex;
  while (g_hs >= hps) {
    g_hs -= hps;
    g_off += g_tp - Tq;
  }
  const int ldw4 = p.ld_bbits * 4;
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(
      wpiece ? (void*)(p.bbits + g_r0 * (long long)p.ld_bbits + (n0 >> 5)) : (void*)(p.B + g_r0 * (long long)p.ldb + n0), 0,
      wpiece ? clip31((p.B_rows - g_r0) * (long long)ldw4 - (long long)(n0 >> 5) * 4)
             : clip31((p.B_rows - g_r0) * (long long)p.ldb * 4 - (long long)n0 * 4),
      0x00020000);
  const unsigned g_lane = wpiece ? (unsigned)(((lane >> 1) & 3) * ldw4 + (lane & 1) * 4)
                                 : (unsigned)(((lane >> 4) * (long long)p.ldb + (lane & 15) * 4) * 4);
  const unsigned g_row4 = wpiece ? (unsigned)ldw4 : (unsigned)(p.ldb * 4);
  const unsigned gdst = wpiece ? (unsigned)(GW * 4) : (unsigned)(wave * 256 * 4);
  const bool g_live = !wpiece || lane < 48;
  auto issue_g = [&](int slot) {                                    // the piece of the NEXT step in line; advances the counters
    const unsigned voff = g_live ? (unsigned)g_off * g_row4 + g_lane : 0xfffffff0u;
    if (wpiece) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsG, (lds_void6_t*)(reinterpret_cast<char*>(Gs) + slot * (GT * 4) + gdst), 4, voff, 0u, 0, 0);
    else dma16h(rsG, reinterpret_cast<char*>(Gs) + slot * (GT * 4) + gdst, voff, 0u);
    g_hs += T6_H;
    g_off += 3 * T6_H;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                           // (no loop: a branch would cut the K-step into basic blocks)
      const bool wrap = g_hs >= hps;
      g_hs -= wrap ? hps : 0;
      g_off += wrap ? g_tp - Tq : 0;
    }
  };
  auto next6 = [](int v) { return v == NG - 1 ? 0 : v + 1; };

  // ---- Y side: wave w < 6 = hex w of the K-step, lane = channel ----
  constexpr bool write_vd = WVD;
  const bool ywave = wave < T6_H;
  const int sw = lane ^ ((wave & 1) << 5);                  // swizzled channel position inside the 64-wide row
  int tq = __builtin_amdgcn_readfirstlane((int)((6 * (v_h0 + (ywave ? wave : 0))) % p.Tp));   // first conv row of the NEXT hex to transform
  const int dstep = __builtin_amdgcn_readfirstlane((6 * T6_H) % p.Tp);
  float bsum = 0.f;
  // Vd in the pair layout (ld_vd / 8 chunks): a lane stores four channels of transforms lane & 3 and 4 + (lane & 3)
  const int kcd = write_vd ? (p.ld_vd >> 3) : 1;
  const unsigned vd_pstride = (unsigned)(16 * p.ld_vd * 4);          // bytes per hex pair
  const long long vd_hexes = ((hexes_all + 1) >> 1) << 1;
  const __amdgpu_buffer_rsrc_t rsVd = __builtin_amdgcn_make_buffer_rsrc(
      write_vd ? (void*)(p.vd + v_h0 * 8 * (long long)p.ld_vd) : (void*)p.slab, 0,
      write_vd ? clip31((vd_hexes - v_h0) * 8 * (long long)p.ld_vd * 4) : 0, 0x00020000);
  const unsigned vdA_lane = (unsigned)(v6_at(0, lane & 3, n0 + (lane & ~3), kcd) * 4);
  const unsigned vdB_lane = vdA_lane + 4u * 64u;
  const int nhex = (int)hexes_all, h_first = (int)v_h0;
  const int h_end = h_first + nsteps * T6_H;
  const int hs_lim = nhex < h_end ? nhex : h_end;           // hexes of this split that exist
  struct y_in {
    float g[3];
    unsigned long long mo[3], me[3];
    int tq;               // time index of the hex's first conv row
  };
  struct y_out {
    float d[6];           // dZ rows 6 h .. 6 h + 5
  };
  auto uni = [](unsigned long long v) -> unsigned long long {   // a wave-uniform value out of vector registers
    return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |
           ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32);
  };
  const int wy = ywave ? wave : 0;                          // (waves 6, 7 run the same code on hex 0's data with all-zero masks)
  struct y_raw {
    float g[3];
    unsigned long long w[3];
  };
  auto fetch_raw = [&](int slot, y_raw& r) {                 // the LDS reads of a hex: issued early in the K-step
    const float* gs = Gs + slot * GT;
    const unsigned long long* ws = reinterpret_cast<const unsigned long long*>(gs + GW) + wy * 4;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      r.g[q] = gs[wy * 256 + q * 64 + lane];
      r.w[q] = ws[q];
    }
  };
  auto masks_y = [&](int sd, const y_raw& r, y_in& y) {
    const int h = h_first + sd * T6_H + wy;
    const int live = ywave & (h < hs_lim);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      y.g[q] = r.g[q];
      const unsigned long long w = uni(r.w[q]);
      const int v = live & (tq + 2 * q < p.Tvalid);
      y.mo[q] = v ? w : 0ull;
      y.me[q] = v ? ~w : 0ull;
    }
    y.tq = tq;
    tq += dstep;
    tq -= tq >= p.Tp ? p.Tp : 0;
  };
  auto fetch_y = [&](int sd, int slot, y_in& y) {
    y_raw r;
    fetch_raw(slot, r);
    masks_y(sd, r, y);
  };
  auto compute_y = [&](int sd, const y_in& y) -> y_out {
    y_out u;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      u.d[2 * r] = selm0(y.me[r], y.g[r]);
      u.d[2 * r + 1] = selm0(y.mo[r], y.g[r]);
    }
    const float ev2 = fmaf(16.f, u.d[4], fmaf(4.f, u.d[2], u.d[0])), od2 = fmaf(32.f, u.d[5], fmaf(8.f, u.d[3], 2.f * u.d[1]));
    float o[4];
    if (th == 0) {                                          // (wave-uniform) transforms 0..3
      const float ev1 = (u.d[0] + u.d[2]) + u.d[4], od1 = (u.d[1] + u.d[3]) + u.d[5];
      o[0] = u.d[0];
      o[1] = ev1 + od1;
      o[2] = ev1 - od1;
      o[3] = ev2 + od2;
      bsum += o[1];
    } else {                                                // transforms 4..7
      const float ev3 = fmaf(0.0625f, u.d[4], fmaf(0.25f, u.d[2], u.d[0])), od3 = fmaf(0.03125f, u.d[5], fmaf(0.125f, u.d[3], 0.5f * u.d[1]));
      o[0] = ev2 - od2;
      o[1] = ev3 + od3;
      o[2] = ev3 - od3;
      o[3] = u.d[5];
    }
    {
      float* dst = (ywave ? Bs + (sd & 1) * QT + wave * 64 : Ydummy + (wave - T6_H) * 64) + sw;
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[i * T6_PLANE] = o[i];
    }
    return u;
  };
  typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
  // Vd of the hexes of step sd.  gp / wp: the pooled row in front of the hex (conv rows 6 h - 2, 6 h - 1) and its word pair
  auto vd_part = [&](int sd, int tqc, const y_out& u, float gp, unsigned long long wp) {
    const int h = h_first + sd * T6_H + wy;
    const int vp = ywave & (tqc >= 2) & (tqc - 2 < p.Tvalid) & (h < hs_lim);
    float d[8], v[8];
    d[1] = selm0(vp ? wp : 0ull, gp);
    d[0] = selm0(vp ? ~wp : 0ull, gp);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[2 + k] = u.d[k];
    wino63_bt(d, v);
    // two 4 x 4 transposes over the lanes of a group (register n of lane r <- register r of lane n)
    const bool odd = lane & 1, hi = lane & 2;
    auto xch = [](float x, auto CTRL) -> float {
      return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), decltype(CTRL)::value, 0xf, 0xf, true));
    };
    using X1 = std::integral_constant<int, 0xB1>;         // quad_perm [1,0,3,2]
    using X2 = std::integral_constant<int, 0x4E>;         // quad_perm [2,3,0,1]
    auto stage = [&](float& a, float& b, bool up, auto CTRL) {
      const float r = xch(up ? a : b, CTRL);
      a = up ? r : a;
      b = up ? b : r;
    };
#pragma unroll
    for (int g4 = 0; g4 < 8; g4 += 4) {
      stage(v[g4 + 0], v[g4 + 1], odd, X1{});
      stage(v[g4 + 2], v[g4 + 3], odd, X1{});
      stage(v[g4 + 0], v[g4 + 2], hi, X2{});
      stage(v[g4 + 1], v[g4 + 3], hi, X2{});
    }
    const f32x4 va4 = {v[0], v[1], v[2], v[3]};
    const f32x4 vb4 = {v[4], v[5], v[6], v[7]};
    const bool ok = ywave && h < hs_lim;
    const unsigned hoff = (unsigned)((h - h_first) >> 1) * vd_pstride + (unsigned)((h - h_first) & 1) * 32u;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, va4), rsVd, ok ? hoff + vdA_lane : 0xfffffff0u, 0u, 2);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32, vb4), rsVd, ok ? hoff + vdB_lane : 0xfffffff0u, 0u, 2);
  };
  // the row in front of this wave's hex at step sd: row 2 of the piece in front (hex wave - 1; for wave 0 the last hex
  // of the previous step, still in the ring)
  auto front_row = [&](int slot, int pslot, float& gp, unsigned long long& wp) {
    const int s_ = wy > 0 ? slot : pslot, hx = wy > 0 ? wy - 1 : T6_H - 1;
    gp = Gs[s_ * GT + hx * 256 + 128 + lane];
    wp = uni(reinterpret_cast<const unsigned long long*>(Gs + s_ * GT + GW)[hx * 4 + 2]);
  };

  // ---- MFMA side: k-slice sl of a K-step = hexes 2 sl (lanes 0-31) and 2 sl + 1 (lanes 32-63) ----
  // wave (wm, wn): C_in rows m0 + 64 wm + {0..31, 32..63} (quarter-tile wm of V) x C_out columns n0 + 32 wn ..; accumulator
  // 4 r + t = (row tile r, transform i0 + t)
  const int a_off0 = wm * QT + lh * 64 + (lr ^ (lh << 5)), a_off1 = wm * QT + lh * 64 + ((32 + lr) ^ (lh << 5));
  const int b_off = lh * 64 + ((wn * 32 + lr) ^ (lh << 5));
  float fa0[8], fb0[4], fa1[8], fb1[4], fac[8], fbc[4];     // slices 0, 1 of a step; slice 2, carried
  auto load_frag = [&](float (&fa)[8], float (&fb)[4], int abuf, int bbuf, int sl) {
    const float* a_s = As + abuf * (4 * QT) + sl * 128;
    const float* b_s = Bs + bbuf * QT + sl * 128 + b_off;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      fa[t] = a_s[a_off0 + t * T6_PLANE];
      fa[4 + t] = a_s[a_off1 + t * T6_PLANE];
      fb[t] = b_s[t * T6_PLANE];
    }
  };
  auto mfma8 = [&](const float (&fa)[8], const float (&fb)[4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[i & 3], acc[i], 0, 0, 0);
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) fac[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) fbc[i] = 0.f;

  {   // (also for an empty split: every access is clamped by its resource, the masks are all zero)
    issue_v(0);
    issue_v(1);
    issue_v(2);
    issue_g(0);
    issue_g(1);
    issue_g(2);
    issue_g(3);
    // the pooled row in front of the split's first hex (wave 0 only needs it, for Vd; everyone loads it - uniform code)
    float gp0 = 0.f;
    unsigned long long wp0 = 0ull;
    if (write_vd && hs0 > 0) {
      const long long pr = g_r0 - 1;                          // same sequence as the first hex (hs0 > 0)
      if (pr < p.B_rows) {
        gp0 = p.B[pr * (long long)p.ldb + n0 + lane];
        const uint32_t* wsrc = p.bbits + pr * (long long)p.ld_bbits + (n0 >> 5);
        wp0 = (unsigned long long)wsrc[0] | ((unsigned long long)wsrc[1] << 32);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    {
      y_in y0;
      fetch_y(0, 0, y0);
      const y_out u0 = compute_y(0, y0);
      if (write_vd && mi == 0) {
        float gp;
        unsigned long long wp;
        front_row(0, NG - 1, gp, wp);                         // (wave 0 reads an unwritten slot here: replaced below)
        if (wave == 0) {
          gp = gp0;
          wp = uni(wp0);
        }
        vd_part(0, y0.tq, u0, gp, wp);
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0070);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  int slot1 = 1, slot4 = 4;                                 // ring slots of steps s + 1 and s + 4
  int turn = 1;                                             // (s + 1) % nslots: whose turn it is to write Vd for step s + 1
  for (int s = 0; s < nsteps; ++s) {
    const int abuf = s & (NA - 1), bbuf = s & 1;
    const int slot0 = slot1 == 0 ? NG - 1 : slot1 - 1;
    __builtin_amdgcn_sched_barrier(0);
    // first half: the pieces of steps s + 3 / s + 4 go out, the raw gradient rows and words of step s + 1 are read from
    // the ring (they return under the 16 MFMAs), the carried slice and slice 0 run
    issue_v(s + 3);
    issue_g(slot4);
    y_raw yr;
    fetch_raw(slot1, yr);
    load_frag(fa0, fb0, abuf, bbuf, 0);
    mfma8(fac, fbc);                                        // slice 2 of the previous step
    load_frag(fa1, fb1, abuf, bbuf, 1);
    mfma8(fa0, fb0);
    // (0x008 MFMA, 0x010 vector memory, 0x100 LDS read, 0x002 VALU, 0x200 LDS write)
    __builtin_amdgcn_sched_group_barrier(0x100, 6 + 6, 0);   // raw rows / words, fragments of slice 0
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if (t < 4) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
      if (t >= 4 && t < 10) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // second half: the transform of step s + 1 between the MFMAs of slice 1 (no branch: waves 6, 7 run it on zero masks)
    load_frag(fac, fbc, abuf, bbuf, 2);
    y_in yn;
    y_out un = {};
    masks_y(s + 1, yr, yn);
    un = compute_y(s + 1, yn);
    mfma8(fa1, fb1);
    __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
      if (t >= 6) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (write_vd) {
      if (ywave && turn == mi && s + 1 < nsteps) {                             // (wave-uniform; every nslots-th step)
        float gp;
        unsigned long long wp;
        front_row(slot1, slot0, gp, wp);
        vd_part(s + 1, yn.tq, un, gp, wp);
      }
      turn = turn + 1 == nslots ? 0 : turn + 1;
    }
    // everything issued up to step s - 2 has landed: V(s + 1), G(s + 2).  In flight: the 4 pieces of this step and of the
    // one before (a Vd store among them only makes the wait reach further back)
    __builtin_amdgcn_s_waitcnt(0x0078);                           // vmcnt(8) lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    slot1 = next6(slot1);
    slot4 = next6(slot4);
  }
  mfma8(fac, fbc);

  if (p.colsum != nullptr && mi == 0) {
    __syncthreads();
    float* red = lds;
    red[wave * 64 + lane] = ywave ? bsum : 0.f;
    __syncthreads();
    if (tid < 64) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < T6_H; ++q) t += red[q * 64 + tid];
      p.colsum[(long long)z * p.Ndim + n0 + tid] = t;
    }
  }
  float* out = p.slab + (long long)z * p.slab_stride;
  const int col = n0 + wn * 32 + lr;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m0 + wm * 64 + (i >> 2) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      out[((long long)(i0 + (i & 3)) * p.Mdim + m) * (long long)p.ldc + col] = acc[i][e];
    }
}

// ------------------------------------------------------------------------------------------
// Second half of the Y / Vd-writing input-gradient epilogue (tonal_wino63_epi.h, MASKY): the first hex of every tile (256
// hexes of the stage below) needs the pooled row in front of it, which the tile in front owns.  The tile left its six rows
// raw in transform slots 2..7 and every tile stored its last pooled row (un-pooled: even, odd) to vhalo.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void wino63_vd_fixup_kernel(float* __restrict__ Vd, const float* __restrict__ halo, long long hexes,
                                                               long long tiles, int hps, int C, int ldv) {
  const int c4n = C >> 2;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= tiles * c4n) return;
  const long long t = idx / c4n;
  const int c = (int)(idx - t * c4n) * 4;
  const long long q = t * 256;
  if (q >= hexes) return;
  float* v = Vd + v6_at(q, 0, c, ldv >> 3);
  f32x4 d[8];
#pragma unroll
  for (int j = 2; j < 8; ++j) d[j] = *reinterpret_cast<const f32x4*>(v + 16 * j);
  if (t > 0 && (q % hps) != 0) {
    d[0] = *reinterpret_cast<const f32x4*>(halo + ((t - 1) * 2) * (long long)C + c);
    d[1] = *reinterpret_cast<const f32x4*>(halo + ((t - 1) * 2 + 1) * (long long)C + c);
  } else {
    d[0] = d[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  f32x4 o[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float dd[8], vv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) dd[j] = d[j][k];
    wino63_bt(dd, vv);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j][k] = vv[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(v + 16 * j) = o[j];
}

// ------------------------------------------------------------------------------------------
// Weight gradient with BOTH operands pre-transformed (loader 3): slab_i[c_in][c_out] = sum_hexes V_i (x) Y_i, Y written by
// the MASKY epilogue of the stage above.  wino63v_tn4_kernel (tile 256 x 64 x 4 transforms, 8 waves) without its Y side: V
// and Y tiles of a K-step (six hexes) arrive by LDS-DMA into two 4-slot rings, three steps ahead (three V pieces per wave,
// one Y piece for waves 0-5); the K-step is 18 ds_read2st64_b32 + 24 MFMAs per wave and nothing else.  colsum (the bias
// gradient of the stage = the column sums of Y plane 1 = the sum of dz over a hex) is added up by wave 0 of slot 0.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void wino63v_tn4y_kernel(const tl_tn_params p, int mtn) {
  constexpr int NA = 4;
  constexpr int QT = 4 * T6_PLANE;               // floats per quarter-tile of V / per Y tile: [4 transforms][6 hexes][64]
  __shared__ __attribute__((aligned(1024))) float lds[NA * 4 * QT + NA * QT + 256];
  float* As = lds;                               // [4][4][4][6][64]  V ring
  float* Ys = lds + NA * 4 * QT;                 // [4][4][6][64]     Y ring   (+ 1 KB: where waves 6, 7 aim their empty piece)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
  // s_setprio 1 for waves 4-7 (the younger half): +0.5 ms here, noise in wino63v_nt_kernel, r04_kernel_notes.md
  const int ntn = p.Ndim / T6_BN;
  const long long tiles = 2LL * mtn * ntn;
  const long long nwg = tiles * p.splitk;
  long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  {
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const int z = __builtin_amdgcn_readfirstlane((int)(bid / tiles));
  const int tt = __builtin_amdgcn_readfirstlane((int)(bid % tiles));
  const int mi = __builtin_amdgcn_readfirstlane(tt % (2 * mtn));
  const int th = mi & 1, i0 = 4 * th;
  const int m0 = (mi >> 1) * 256, n0 = __builtin_amdgcn_readfirstlane((tt / (2 * mtn)) * T6_BN);
  const long long hexes_all = p.Krows / 6;
  const long long ksteps_all = (hexes_all + T6_H - 1) / T6_H;
  const long long per = __builtin_amdgcn_readfirstlane((int)((ksteps_all + p.splitk - 1) / p.splitk));
  const long long ks_begin = z * per;
  long long ks_end = ks_begin + per;
  if (ks_end > ksteps_all) ks_end = ksteps_all;
  const int nsteps = ks_end > ks_begin ? (int)(ks_end - ks_begin) : 0;

  f32x16 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  const long long v_h0 = ks_begin * T6_H;
  const int kc8 = p.lda >> 3, kcy = p.ldb >> 3;
  const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.A + v_h0 * 8 * (long long)p.lda), 0, clip31((p.A_rows - v_h0) * 8 * (long long)p.lda * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.B + v_h0 * 8 * (long long)p.ldb), 0, clip31((p.B_rows - v_h0) * 8 * (long long)p.ldb * 4), 0x00020000);
  unsigned vvoff[3], vdst[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int quarter = (wave * 3 + t) / 6, pc = (wave * 3 + t) % 6;
    const int rho = 4 * pc + (lane >> 4), i = rho / 6, hx = rho % 6;
    const int chunk = (lane & 15) ^ ((hx & 1) << 3);
    vvoff[t] = (unsigned)(v6_at(hx + p.a_hex, i0 + i, m0 + quarter * 64 + chunk * 4, kc8) * 4);   // (a_hex: tl_tn_params)
    vdst[t] = (unsigned)((quarter * QT + pc * 256) * 4);
  }
  // the Y piece of wave w < 6: rows 4 w .. 4 w + 3 of the tile's 24 ([transform][hex] order), like a quarter-tile of V
  const bool ypiece = wave < T6_H;
  unsigned yvoff;
  {
    const int rho = 4 * (ypiece ? wave : 0) + (lane >> 4), i = rho / 6, hx = rho % 6;
    const int chunk = (lane & 15) ^ ((hx & 1) << 3);
    yvoff = (unsigned)(v6_at(hx, i0 + i, n0 + chunk * 4, kcy) * 4);
  }
  const unsigned v_step = (unsigned)(T6_H * 8 * p.lda * 4), y_step = (unsigned)(T6_H * 8 * p.ldb * 4);
  auto issue = [&](int step) {
    char* vb = reinterpret_cast<char*>(As) + (step & (NA - 1)) * (4 * QT * 4);
    const unsigned soff = (unsigned)step * v_step;            // (in the per-lane offset: that one is range-checked)
#pragma unroll
    for (int t = 0; t < 3; ++t) dma16h(rsV, vb + vdst[t], vvoff[t] + soff, 0u);
    // (waves 6, 7: an empty piece - offset past the resource - into the spare KB behind the ring: one operation per wave)
    char* yb = reinterpret_cast<char*>(Ys) + (ypiece ? ((step & (NA - 1)) * QT + wave * 256) * 4 : NA * QT * 4);
    dma16h(rsY, yb, ypiece ? yvoff + (unsigned)step * y_step : 0xfffffff0u, 0u);
  };
  const int a_off0 = wm * QT + lh * 64 + (lr ^ (lh << 5)), a_off1 = wm * QT + lh * 64 + ((32 + lr) ^ (lh << 5));
  const int b_off = lh * 64 + ((wn * 32 + lr) ^ (lh << 5));
  float fa0[8], fb0[4], fa1[8], fb1[4], fac[8], fbc[4];     // slices 0, 1 of a step; slice 2, carried
  auto load_frag = [&](float (&fa)[8], float (&fb)[4], int buf, int sl) {
    const float* a_s = As + buf * (4 * QT) + sl * 128;
    const float* b_s = Ys + buf * QT + sl * 128 + b_off;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      fa[t] = a_s[a_off0 + t * T6_PLANE];
      fa[4 + t] = a_s[a_off1 + t * T6_PLANE];
      fb[t] = b_s[t * T6_PLANE];
    }
  };
  auto mfma8 = [&](const float (&fa)[8], const float (&fb)[4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[i & 3], acc[i], 0, 0, 0);
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) fac[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) fbc[i] = 0.f;
  const bool summer = p.colsum != nullptr && mi == 0 && wave == 0;    // (slot 0 holds transform 1: Y plane 1 = the sum of a hex's dz)
  float bsum = 0.f;
  issue(0);
  issue(1);
  issue(2);
  __builtin_amdgcn_s_waitcnt(0x0078);                         // vmcnt(8): step 0 has landed
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & (NA - 1);
    __builtin_amdgcn_sched_barrier(0);
    issue(s + 3);
    load_frag(fa0, fb0, buf, 0);
    mfma8(fac, fbc);                                        // slice 2 of the previous step
    load_frag(fa1, fb1, buf, 1);
    mfma8(fa0, fb0);
    load_frag(fac, fbc, buf, 2);
    mfma8(fa1, fb1);
    // (0x008 MFMA, 0x010 vector memory, 0x100 LDS read): the reads of slice 0 first, one piece behind each of the first MFMAs,
    // the reads of slices 1 and 2 between the others
    __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
    for (int t = 0; t < 24; ++t) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if (t < 4) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
      if (t >= 4 && t < 16) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (summer) {
      const float* y1 = Ys + buf * QT + T6_PLANE;
#pragma unroll
      for (int hx = 0; hx < T6_H; ++hx) bsum += y1[hx * 64 + (lane ^ ((hx & 1) << 5))];
    }
    // everything issued up to step s + 1 has landed; the 4 pieces of steps s + 2 and s + 3 may fly
    __builtin_amdgcn_s_waitcnt(0x0078);                           // vmcnt(8) lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  mfma8(fac, fbc);
  if (summer) p.colsum[(long long)z * p.Ndim + n0 + lane] = bsum;
  float* out = p.slab + (long long)z * p.slab_stride;
  const int col = n0 + wn * 32 + lr;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = m0 + wm * 64 + (i >> 2) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      out[((long long)(i0 + (i & 3)) * p.Mdim + m) * (long long)p.ldc + col] = acc[i][e];
    }
}

// ------------------------------------------------------------------------------------------
// (G, arg-max bits) -> Y = A dz and Vd = B^T (dz rows 6 h - 2 .. 6 h + 5) of a pooled 3-tap stage, as a kernel of its own:
// the operands of the stage's transform-free weight gradient (tl_conv3_wino63v_tn, loader 3) and of its input gradient, for
// a stage whose gradient rows come from a kernel that has no Y-producing epilogue (conv3 of the reference stack: G3 comes
// out of the one-tap GEMM of stage 4).  Thread = 4 channels x one hex, lanes ordered (8-channel chunk, hex of the pair, half
// chunk) as in conv1_fwd_vh_kernel: four adjacent lanes write the 64-byte run of a transform, two transforms one line.
// HBM-write bound: 2 x 2.67 x the bytes of G.  G / bits rows in the layout [seq * g_tp + t'].
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void wino63_unpool_yvd_kernel(const float* __restrict__ G, const uint32_t* __restrict__ bits,
                                                                 float* __restrict__ Y, float* __restrict__ Vd, long long nhex,
                                                                 long long g_rows, int hps, int g_tp, int Tvalid, int C, int ldg,
                                                                 int ld_bits, int ldv) {
  const int tpp = C >> 1;                                    // threads per hex pair
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long pair = idx / tpp;
  const int tl_ = (int)(idx - pair * tpp);
  const int half = tl_ & 1, hpar = (tl_ >> 1) & 1, kc = tl_ >> 2;
  const int c = 8 * kc + 4 * half;
  const long long hg = 2 * pair + hpar;
  if (hg >= nhex) return;
  const long long seq = hg / hps;
  const int hs = (int)(hg - seq * hps);
  const long long row0 = seq * g_tp + 3LL * hs;               // G row of the hex's first pooled row
  float dz[8][4];                                             // un-pooled rows 6 h - 2 .. 6 h + 5, four channels
#pragma unroll
  for (int r = -1; r < 3; ++r) {
    const long long row = row0 + r;
    const bool ok = (r >= 0 || hs > 0) && 6 * hs + 2 * r < Tvalid && row >= 0 && row < g_rows;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    uint32_t w = 0;
    if (ok) {
      g = *reinterpret_cast<const f32x4*>(G + row * (long long)ldg + c);
      w = bits[row * (long long)ld_bits + (c >> 5)] >> (c & 31);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool odd = (w >> k) & 1u;
      dz[2 * (r + 1)][k] = odd ? 0.f : g[k];
      dz[2 * (r + 1) + 1][k] = odd ? g[k] : 0.f;
    }
  }
  f32x4 oy[8], ov[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float d[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = dz[j][k];
    wino63_bt(d, v);
    const float* d6 = d + 2;
    const float ev1 = (d6[0] + d6[2]) + d6[4], od1 = (d6[1] + d6[3]) + d6[5];
    const float ev2 = fmaf(16.f, d6[4], fmaf(4.f, d6[2], d6[0])), od2 = fmaf(32.f, d6[5], fmaf(8.f, d6[3], 2.f * d6[1]));
    const float ev3 = fmaf(0.0625f, d6[4], fmaf(0.25f, d6[2], d6[0])), od3 = fmaf(0.03125f, d6[5], fmaf(0.125f, d6[3], 0.5f * d6[1]));
    const float y[8] = {d6[0], ev1 + od1, ev1 - od1, ev2 + od2, ev2 - od2, ev3 + od3, ev3 - od3, d6[5]};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      oy[j][k] = y[j];
      ov[j][k] = v[j];
    }
  }
  const long long at = v6_at(hg, 0, c, ldv >> 3);
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(Y + at + 16 * j) = oy[j];
#pragma unroll
  for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(Vd + at + 16 * j) = ov[j];
}

// ------------------------------------------------------------------------------------------
// Round 5: the input gradient of a ONE-tap pooled stage whose input comes out of a pooled 3-tap F(6,3) stage (conv4 of the
// reference stack, models/synthesis_models.py:99-101) on the NT63 kernel, so that its epilogue can hand that stage the operands of
// its backward pass (Y, Vd: epilogue 7) instead of gradient rows which a kernel of its own (wino63_unpool_yvd_kernel: 21.7 GB)
// then has to un-pool and transform.  The eight batched GEMMs of the kernel take the SIX rows of a hex: A[hex H][slot i < 6] =
// un-pooled gradient row 6 H + i of the one-tap stage (row geometry [seq * Tp + t], the hexes of the 3-tap stage below: three of
// its pooled rows each, two of its hexes per hex here), slots 6, 7 zero, against the same taps W^T in every slot.
//   wino63_unpool_rows6_kernel: (G rows [seq * g_tp + t / 2], arg-max bits) -> A, pair layout; thread = 4 channels x one hex,
//   lanes ordered like wino63_unpool_yvd_kernel (64-byte runs); slots 6, 7 are written (zeros) only when `pad` is set.
//   wino63_weights1_kernel: w (O, I) -> taps [ldb / 8][8][I][8], slot t < 6: w[o][n], slots 6, 7 and o >= O: zero.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void wino63_unpool_rows6_kernel(const float* __restrict__ G, const uint32_t* __restrict__ bits,
                                                                   float* __restrict__ A, long long nhex, long long rows,
                                                                   long long g_rows, int Tp, int g_tp, int Tvalid, int C, int ldg,
                                                                   int ld_bits, int lda, int pad) {
  const int tpp = C >> 1;                                    // threads per hex pair
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long pair = idx / tpp;
  const int tl_ = (int)(idx - pair * tpp);
  const int half = tl_ & 1, hpar = (tl_ >> 1) & 1, kc = tl_ >> 2;
  const int c = 8 * kc + 4 * half;
  const long long hg = 2 * pair + hpar;
  if (hg >= nhex) return;
  float* dst = A + v6_at(hg, 0, c, lda >> 3);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const long long R = 6 * hg + i;
    f32x4 v = zero;
    if (R < rows) {
      const long long seq = R / Tp;
      const int t = (int)(R - seq * Tp);
      const long long row = seq * g_tp + (t >> 1);
      if (t < Tvalid && row < g_rows) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(G + row * (long long)ldg + c);
        const uint32_t w = bits[row * (long long)ld_bits + (c >> 5)] >> (c & 31);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (int)((w >> k) & 1u) == (t & 1) ? g[k] : 0.f;
      }
    }
    *reinterpret_cast<f32x4*>(dst + 16 * i) = v;
  }
  if (pad) {
    *reinterpret_cast<f32x4*>(dst + 16 * 6) = zero;
    *reinterpret_cast<f32x4*>(dst + 16 * 7) = zero;
  }
}

__global__ void wino63_weights1_kernel(const float* __restrict__ w, float* __restrict__ out, int O, int I, int ldb) {
  const long long n_all = (long long)ldb * 8 * I;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_all) return;
  const int k8 = (int)(idx & 7);
  const long long q = idx >> 3;
  const int n = (int)(q % I);
  const long long q2 = q / I;
  const int t = (int)(q2 & 7);
  const int o = (int)(q2 >> 3) * 8 + k8;
  out[idx] = (t < 6 && o < O) ? w[(long long)o * I + n] : 0.f;
}

// ------------------------------------------------------------------------------------------
// conv1 (C_in = 1) + LeakyReLU + max-pool writing V of its pooled output in HEX form, pair layout (conv1_fwd_vq_kernel of
// tonal_misc.hip with six rows per unit).  HBM-write bound, so the thread mapping follows the layout: four adjacent lanes
// = (one 8-channel chunk) x (the two hexes of a pair) write the 64-byte run of a transform, two transforms = one cache line;
// a thread walks the hexes of ONE parity of its sequence and computes all eight rows of each (the halo rows are three
// MACs per element from the LDS-resident signal).  (The first version - a thread = 4 channels x consecutive hexes, 32-byte
// runs half a KB apart, non-temporal - ran at 0.65 TB/s: 27.9 ms for the 18 GB of V1.)
// ------------------------------------------------------------------------------------------
constexpr int C1_MAXKT = 8;
template <int KT>
__global__ __launch_bounds__(256) void conv1_fwd_vh_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ P,
                                                           float* __restrict__ V, uint32_t* __restrict__ bits,
                                                           uint32_t* __restrict__ sign, long long S, int T, int C1,
                                                           int Tp, int Tout, float slope) {
  constexpr int kt = KT;                         // (a run-time tap count cost 547 scalar branches in the row loop)
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const long long seq = blockIdx.x;
  for (int i = threadIdx.x; i < T; i += blockDim.x) xs[i] = x[seq * T + i];
  __syncthreads();
  const int tpp = C1 >> 1;                       // threads per hex pair: (C1 / 8 chunks) x 2 hexes x 2 halves of a chunk
  const int ppp = 256 / tpp;                     // hex pairs per pass (1 for C1 = 512)
  const int tl_ = threadIdx.x % tpp, psub = threadIdx.x / tpp;
  const int half = tl_ & 1, hpar = (tl_ >> 1) & 1, kc = tl_ >> 2;
  const int o = 8 * kc + 4 * half;               // first of this thread's four channels
  float wv[4][KT], bv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    bv[c] = b[o + c];
#pragma unroll
    for (int j = 0; j < KT; ++j) wv[c][j] = w[(o + c) * kt + j];
  }
  // position of the four channels inside their 32-channel word: the eight lanes of a word differ in lane bits 0, 2, 3
  const int sh = 4 * (2 * (kc & 3) + half);
  const int Th = Tp / 6;
  auto row = [&](int pr, bool live, f32x4& out, uint32_t& wb, uint32_t& ws) {
    out = f32x4{0.f, 0.f, 0.f, 0.f};
    uint32_t nib = 0, nsg = 0;
    if (live && pr < Tout) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float z0 = 0.f, z1 = 0.f;
#pragma unroll
        for (int jj = 0; jj < KT; ++jj) {
          z0 = fmaf(wv[c][jj], xs[2 * pr + jj], z0);
          z1 = fmaf(wv[c][jj], xs[2 * pr + 1 + jj], z1);
        }
        const float y0 = lrelu(z0 + bv[c], slope), y1 = lrelu(z1 + bv[c], slope);
        const bool sel = y1 > y0;
        const float v = sel ? y1 : y0;
        out[c] = v;
        nib |= (sel ? 1u : 0u) << c;
        nsg |= (v > 0.f ? 1u : 0u) << c;
      }
    }
    // OR over the eight lanes of the word (lane bits 0, 2, 3) with DPP operands: neighbour of the quad pair, then the row
    // rotated by 4 and by 8
    auto or8 = [](uint32_t v) {
      v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);      // quad_perm [1, 0, 3, 2]
      v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xf, 0xf, false);     // row_ror 4
      v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, false);     // row_ror 8
      return v;
    };
    wb = or8(nib << sh);
    ws = or8(nsg << sh);
  };
  // global hex index seq * Th + q; a thread takes those whose parity is hpar (its slot inside the pair)
  const long long h0 = seq * Th;
  const int q0 = (int)((hpar - h0) & 1) + 2 * psub;
  const int trips = (Th + 2 * ppp - 1) / (2 * ppp) + 1;          // (uniform over the block: the shuffles need every lane)
  const bool word_writer = sh == 0;
  for (int i = 0; i < trips; ++i) {
    const int q = q0 + 2 * ppp * i;
    const bool live = q < Th;
    f32x4 d[8];
    uint32_t wb[8], ws[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row(6 * q + j, live && 6 * q + j < Tp, d[j], wb[j], ws[j]);
    if (live) {
      const long long row0 = seq * Tp + 6 * q;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (P != nullptr) *reinterpret_cast<f32x4*>(P + (row0 + j) * C1 + o) = d[j];
        if (word_writer) {
          bits[(row0 + j) * (C1 >> 5) + (o >> 5)] = wb[j];
          if (sign != nullptr) sign[(row0 + j) * (C1 >> 5) + (o >> 5)] = ws[j];
        }
      }
      f32x4 ov[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float dd[8], vv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) dd[j] = d[j][k];
        wino63_bt(dd, vv);
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[j][k] = vv[j];
      }
      float* dst = V + v6_at(h0 + q, 0, o, C1 >> 3);          // (pair layout: transform j of these four channels at + 16 j)
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(dst + 16 * j) = ov[j];
    }
  }
}

}  // namespace tl

extern "C" int tl_wino63_weights(const float* w, float* fwd, float* dgr, int O, int I, int ld_f, int ld_d, void* stream) {
  using namespace tl;
  TL_REQUIRE(w != nullptr && (fwd != nullptr || dgr != nullptr), "wino63_weights: null pointer");
  TL_REQUIRE(O > 0 && I > 0, "wino63_weights: bad sizes");
  TL_REQUIRE((fwd == nullptr || (ld_f >= I && ld_f % 8 == 0)) && (dgr == nullptr || (ld_d >= O && ld_d % 8 == 0)),
             "wino63_weights: leading dimensions must cover the reduction length and be multiples of 8");
  const long long nf = (long long)O * ld_f, nd = (long long)I * ld_d;
  const long long n = nf > nd ? nf : nd;
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_weights: too large");
  hipLaunchKernelGGL(wino63_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, fwd, dgr, O,
                     I, ld_f, ld_d, 1);
  return check_launch("wino63_weights");
}

// Taps of the input gradient that runs on Y = A dz (epilogue 4 with row_shift 0): U = G g of the taps as they are, chunk-major over
// the reduction index C_out like the flipped set of tl_wino63_weights: [ld_d / 8][8 transforms][I rows][8]
extern "C" int tl_wino63_weights_y(const float* w, float* dgy, int O, int I, int ld_d, void* stream) {
  using namespace tl;
  TL_REQUIRE(w != nullptr && dgy != nullptr, "wino63_weights_y: null pointer");
  TL_REQUIRE(O > 0 && I > 0 && ld_d >= O && ld_d % 8 == 0, "wino63_weights_y: O, I > 0 and ld_d %% 8 == 0, ld_d >= O needed");
  const long long n = (long long)I * ld_d;
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_weights_y: too large");
  hipLaunchKernelGGL(wino63_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     (float*)nullptr, dgy, O, I, 0, ld_d, 0);
  return check_launch("wino63_weights_y");
}

extern "C" int tl_wino63_wgrad_finalize(const float* red, float* gw, int O, int I, int ld, void* stream) {
  using namespace tl;
  TL_REQUIRE(red && gw && O > 0 && I > 0 && ld >= O, "wino63_wgrad_finalize: bad arguments");
  const long long n = (long long)O * I;
  hipLaunchKernelGGL(wino63_wgrad_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, red, gw,
                     O, I, ld);
  return check_launch("wino63_wgrad_finalize");
}

extern "C" int tl_wino63_v_fixup(float* V, const float* vhalo, int64_t hexes, int64_t tiles, int Tq, int C, int ldv, void* stream) {
  using namespace tl;
  TL_REQUIRE(V && vhalo, "wino63_v_fixup: null pointer");
  TL_REQUIRE(hexes > 0 && tiles > 0 && Tq > 0 && Tq % 6 == 0, "wino63_v_fixup: hexes, tiles > 0 and Tq %% 6 == 0 needed");
  TL_REQUIRE(C > 0 && C % 4 == 0 && ldv >= C && ldv % 8 == 0, "wino63_v_fixup: C %% 4 and ldv %% 8 needed");
  const long long n = (long long)tiles * (C / 4);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_v_fixup: grid too large");
  hipLaunchKernelGGL(wino63_v_fixup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, V, vhalo,
                     (long long)hexes, (long long)tiles, Tq, C, ldv);
  return check_launch("wino63_v_fixup");
}

extern "C" int tl_wino63_vd_fixup(float* Vd, const float* vhalo, int64_t hexes, int64_t tiles, int hexes_per_seq, int C, int ldv,
                                  void* stream) {
  using namespace tl;
  TL_REQUIRE(Vd && vhalo, "wino63_vd_fixup: null pointer");
  TL_REQUIRE(hexes > 0 && tiles > 0 && hexes_per_seq > 0, "wino63_vd_fixup: hexes, tiles, hexes per sequence > 0 needed");
  TL_REQUIRE(C > 0 && C % 4 == 0 && ldv >= C && ldv % 8 == 0, "wino63_vd_fixup: C %% 4 and ldv %% 8 needed");
  const long long n = (long long)tiles * (C / 4);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_vd_fixup: grid too large");
  hipLaunchKernelGGL(wino63_vd_fixup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Vd, vhalo,
                     (long long)hexes, (long long)tiles, hexes_per_seq, C, ldv);
  return check_launch("wino63_vd_fixup");
}

extern "C" int tl_wino63_unpool_yvd(const float* G, const uint32_t* bits, float* Y, float* Vd, int64_t conv_rows, int64_t g_rows,
                                    int Tp, int g_tp, int Tvalid, int C, int ldg, int ld_bits, int ldv, void* stream) {
  using namespace tl;
  TL_REQUIRE(G && bits && Y && Vd, "wino63_unpool_yvd: null pointer");
  TL_REQUIRE(Tp > 0 && Tp % 6 == 0 && conv_rows > 0 && conv_rows % Tp == 0 && Tvalid % 2 == 0 && Tvalid <= Tp,
             "wino63_unpool_yvd: Tp %% 6 == 0, whole sequences, an even Tvalid <= Tp needed");
  TL_REQUIRE(g_tp > 0 && 2 * g_tp >= Tvalid && g_rows >= (conv_rows / Tp) * (long long)g_tp, "wino63_unpool_yvd: G holds fewer rows than sequences x g_tp");
  TL_REQUIRE(C > 0 && C % 8 == 0 && ldg >= C && ldg % 4 == 0 && ldv >= C && ldv % 8 == 0 && ld_bits * 32 >= C,
             "wino63_unpool_yvd: C %% 8, ldg %% 4, ldv %% 8 needed, bits row must cover C");
  const long long nhex = conv_rows / 6;
  const long long n = ((nhex + 1) / 2) * (C / 2);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_unpool_yvd: grid too large");
  hipLaunchKernelGGL(wino63_unpool_yvd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, bits, Y, Vd,
                     nhex, (long long)g_rows, Tp / 6, g_tp, Tvalid, C, ldg, ld_bits, ldv);
  return check_launch("wino63_unpool_yvd");
}

// ---- the CNN-RNN classifier's 7-tap convolutions on the F(6,3) NT kernel (reference models/deep_classifiers.py:250-256) ----
extern "C" int tl_wino63_weights7(const float* w, float* fwd, int O, int I, int taps, void* stream) {
  using namespace tl;
  TL_REQUIRE(w && fwd && O > 0 && I > 0 && I % 8 == 0 && taps >= 7 && taps <= 9, "wino63_weights7: I %% 8 == 0 and 7..9 taps needed");
  const long long n = 3LL * O * I;
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_weights7: grid too large");
  hipLaunchKernelGGL(wino63_weights7_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, fwd, O, I, taps);
  return check_launch("wino63_weights7");
}

extern "C" int tl_wino63_xform2(const float* P, float* V0, float* V1, int64_t rows, int Tp, int Tvalid, int C, int ldp, int ldv,
                                void* stream) {
  using namespace tl;
  TL_REQUIRE(P && V0 && V1, "wino63_xform2: null pointer");
  TL_REQUIRE(Tp > 0 && Tp % 6 == 0 && rows > 0 && rows % Tp == 0 && Tvalid >= 0 && Tvalid <= Tp, "wino63_xform2: Tp %% 6 == 0, whole sequences, Tvalid <= Tp needed");
  TL_REQUIRE(C > 0 && C % 8 == 0 && ldp >= C && ldp % 4 == 0 && ldv >= C && ldv % 8 == 0, "wino63_xform2: C %% 8, ldp %% 4, ldv %% 8 needed");
  const long long nhex = rows / 6;
  const long long n = ((nhex + 1) / 2) * (C / 2);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_xform2: grid too large");
  hipLaunchKernelGGL(wino63_xform2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, V0, V1, nhex,
                     Tp / 6, Tp, Tvalid, C, ldp, ldv, 0);
  return check_launch("wino63_xform2");
}

// ---- the backward of those 7-tap stages (TONAL_KERNELS conv7=wino63bwd; include/tonal_hip.h states the algebra) ----
extern "C" int tl_wino63_xform2s(const float* P, float* V0, float* V1, int64_t rows, int Tp, int Tvalid, int shift, int C, int ldp,
                                 int ldv, void* stream) {
  using namespace tl;
  TL_REQUIRE(P && V0 && V1, "wino63_xform2s: null pointer");
  TL_REQUIRE(Tp > 0 && Tp % 6 == 0 && rows > 0 && rows % Tp == 0 && Tvalid >= 0 && Tvalid <= Tp, "wino63_xform2s: Tp %% 6 == 0, whole sequences, Tvalid <= Tp needed");
  TL_REQUIRE(shift >= 0 && shift <= 6, "wino63_xform2s: shift must lie in 0..6");
  TL_REQUIRE(C > 0 && C % 8 == 0 && ldp >= C && ldp % 4 == 0 && ldv >= C && ldv % 8 == 0, "wino63_xform2s: C %% 8, ldp %% 4, ldv %% 8 needed");
  const long long nhex = rows / 6;
  const long long n = ((nhex + 1) / 2) * (C / 2);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_xform2s: grid too large");
  hipLaunchKernelGGL(wino63_xform2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, V0, V1, nhex,
                     Tp / 6, Tp, Tvalid, C, ldp, ldv, shift);
  return check_launch("wino63_xform2s");
}

extern "C" int tl_wino63_ydz(const float* G, float* Y, int64_t rows, int Tp, int Tvalid, int C, int ldg, int ldv, void* stream) {
  using namespace tl;
  TL_REQUIRE(G && Y, "wino63_ydz: null pointer");
  TL_REQUIRE(Tp > 0 && Tp % 6 == 0 && rows > 0 && rows % Tp == 0 && Tvalid >= 0 && Tvalid <= Tp, "wino63_ydz: Tp %% 6 == 0, whole sequences, Tvalid <= Tp needed");
  TL_REQUIRE(C > 0 && C % 8 == 0 && ldg >= C && ldg % 4 == 0 && ldv >= C && ldv % 8 == 0, "wino63_ydz: C %% 8, ldg %% 4, ldv %% 8 needed");
  const long long nhex = rows / 6;
  const long long n = ((nhex + 1) / 2) * (C / 2);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_ydz: grid too large");
  hipLaunchKernelGGL(wino63_ydz_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, Y, nhex, Tp / 6, Tp,
                     Tvalid, C, ldg, ldv);
  return check_launch("wino63_ydz");
}

// out[R][n] = LeakyReLU(sum_{j < 7..9} sum_k w[n][k][j] x[R + j][k] + bias[n]) from A = V0, aux = V1 (tl_wino63_xform2 of x) and
// Bw = tl_wino63_weights7: K = input channels (per segment), ldb >= 3 K
extern "C" int tl_conv7_wino63v_nt(const tl_nt_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "conv7_wino63: null params");
  const tl_nt_params& p = *pp;
  TL_REQUIRE(p.A && p.aux && p.Bw && p.out, "conv7_wino63: null V0 (A) / V1 (aux) / Bw / out");
  TL_REQUIRE(p.loader == W_LOAD_V && p.epilogue == W_EPI_LRELU && p.row_shift == 0 && p.splitk <= 1,
             "conv7_wino63: loader 2 (pre-transformed operands), LRELU epilogue, row_shift 0, no split-K");
  TL_REQUIRE(p.J >= 7 && p.J <= 9, "conv7_wino63: 7..9 taps (three segments)");
  TL_REQUIRE(p.M > 0 && p.M % 6 == 0 && p.N > 0 && p.N % 32 == 0 && p.K >= 16 && p.K % 8 == 0, "conv7_wino63: M %% 6, N %% 32, K %% 8, K >= 16 needed");
  TL_REQUIRE(p.lda >= p.K && p.lda % 8 == 0 && p.ldb >= 3 * p.K && p.ldb % 8 == 0 && p.ldo >= p.N, "conv7_wino63: bad leading dimensions");
  TL_REQUIRE(p.A_rows % 2 == 0 && p.Tp > 0 && p.Tp % 6 == 0 && p.M % p.Tp == 0, "conv7_wino63: V holds hex pairs; Tp %% 6, whole sequences");
  TL_REQUIRE(8LL * p.N * p.ldb * 4 < (1LL << 31), "conv7_wino63: tap set larger than a buffer resource");
  TL_REQUIRE(128LL * 8 * p.lda * 4 + 4LL * p.K < (1LL << 31) && p.M + V6_ROWS < (1LL << 31), "conv7_wino63: tile span / M too large");
  TL_REQUIRE(p.slope >= 0.f && p.slope <= 1.f, "conv7_wino63: LeakyReLU slope must lie in [0, 1]");
  const long long ntm = (p.M + V6_ROWS - 1) / V6_ROWS;
  const long long nwg = ntm * ((p.N + V6_BN - 1) / V6_BN);
  TL_REQUIRE(nwg < (1LL << 31), "conv7_wino63: grid too large");
  TL_REQUIRE(p.A_rows >= ntm * V6_BH, "conv7_wino63: V0 / V1 must hold whole 128-hex tiles (pad them with zero hexes)");
  TL_REQUIRE(p.a_hps_extra == 0, "conv7_wino63: no compact-M mode (a_hps_extra must be 0)");
  const long long ngrid = nwg < 256 ? nwg : 256;
  hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_LRELU>), dim3((unsigned)ngrid), dim3(512), 0, (hipStream_t)stream, p);
  return check_launch("conv7_wino63");
}

// out[R][n] = (sum_{j < 7} sum_k Bw-taps[n][k][j] dzs[R + j][k]) * LeakyReLU'(stage input at [R][n]) from A = V0, aux = V1
// (tl_wino63_xform2s of dz with shift 6) and Bw = tl_wino63_weights7 of the flipped, transposed weight: K = C_out, N = C_in
extern "C" int tl_conv7_wino63v_dgrad_nt(const tl_nt_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "conv7_wino63_dgrad: null params");
  const tl_nt_params& p = *pp;
  TL_REQUIRE(p.A && p.aux && p.Bw && p.out, "conv7_wino63_dgrad: null V0 (A) / V1 (aux) / Bw / out");
  TL_REQUIRE(p.loader == W_LOAD_V && p.epilogue == W_EPI_MASK && p.row_shift == 0 && p.splitk <= 1,
             "conv7_wino63_dgrad: loader 2 (pre-transformed operands), MASK epilogue, row_shift 0 (the rows are moved by the transform), no split-K");
  TL_REQUIRE((p.auxbits != nullptr) != (p.mask != nullptr), "conv7_wino63_dgrad: exactly one mask source - auxbits (sign words) or mask (float rows)");
  TL_REQUIRE(p.J == 7, "conv7_wino63_dgrad: 7 taps");
  TL_REQUIRE(p.M > 0 && p.M % 6 == 0 && p.N > 0 && p.N % 32 == 0 && p.K >= 16 && p.K % 8 == 0, "conv7_wino63_dgrad: M %% 6, N %% 32, K %% 8, K >= 16 needed");
  TL_REQUIRE(p.lda >= p.K && p.lda % 8 == 0 && p.ldb >= 3 * p.K && p.ldb % 8 == 0 && p.ldo >= p.N, "conv7_wino63_dgrad: bad leading dimensions");
  TL_REQUIRE(p.auxbits == nullptr || p.ld_auxbits * 32 >= p.N, "conv7_wino63_dgrad: ld_auxbits too small");
  TL_REQUIRE(p.mask == nullptr || p.ld_mask >= p.N, "conv7_wino63_dgrad: ld_mask too small");
  TL_REQUIRE(p.A_rows % 2 == 0 && p.Tp > 0 && p.Tp % 6 == 0 && p.M % p.Tp == 0, "conv7_wino63_dgrad: V holds hex pairs; Tp %% 6, whole sequences");
  TL_REQUIRE(8LL * p.N * p.ldb * 4 < (1LL << 31), "conv7_wino63_dgrad: tap set larger than a buffer resource");
  TL_REQUIRE(128LL * 8 * p.lda * 4 + 4LL * p.K < (1LL << 31) && p.M + V6_ROWS < (1LL << 31), "conv7_wino63_dgrad: tile span / M too large");
  TL_REQUIRE(192LL * (p.ldo > p.ld_mask ? p.ldo : p.ld_mask) * 4 < (1LL << 31), "conv7_wino63_dgrad: ldo / ld_mask too large");
  TL_REQUIRE(p.slope >= 0.f && p.slope <= 1.f, "conv7_wino63_dgrad: LeakyReLU slope must lie in [0, 1]");
  const long long ntm = (p.M + V6_ROWS - 1) / V6_ROWS;
  const long long nwg = ntm * ((p.N + V6_BN - 1) / V6_BN);
  TL_REQUIRE(nwg < (1LL << 31), "conv7_wino63_dgrad: grid too large");
  TL_REQUIRE(p.A_rows >= ntm * V6_BH, "conv7_wino63_dgrad: V0 / V1 must hold whole 128-hex tiles (pad them with zero hexes)");
  TL_REQUIRE(p.a_hps_extra == 0, "conv7_wino63_dgrad: no compact-M mode (a_hps_extra must be 0)");
  const long long ngrid = nwg < 256 ? nwg : 256;
  if (p.auxbits != nullptr) hipLaunchKernelGGL((wino63v_nt_kernel<W6_EPI_MASK7>), dim3((unsigned)ngrid), dim3(512), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((wino63v_nt_kernel<W6_EPI_MASK7F>), dim3((unsigned)ngrid), dim3(512), 0, (hipStream_t)stream, p);
  return check_launch("conv7_wino63_dgrad");
}

// NT passes on a pre-transformed operand: A = V[hex][8][lda], A_rows = hexes in V (whole 128-hex tiles), M = output rows
// (6 per hex).  Forward: V of the stage input, POOL / POOLV epilogue.  Input gradient: Vd (written by tl_conv3_wino63v_tn),
// taps = the flipped / transposed set, MASK or fused-conv1-weight-gradient epilogue.  Epilogue 6 (MASKY) writes Y (and, with
// vout2 / vhalo, Vd) of the stage below instead of rows; epilogue 4 with row_shift 0 takes that Y as its operand:
//   dd[rows 6 H .. 6 H + 7] = B [sum_cout (G g)_i . (A dz)_i], the transposition of the forward form (tonal_wino63_epi.h).
extern "C" int tl_wino63_nt_tile_rows(void) { return tl::V6_ROWS; }

extern "C" int tl_conv3_wino63v_nt(const tl_nt_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "wino63v_nt: null params");
  const tl_nt_params& p = *pp;
  TL_REQUIRE(p.A && p.Bw && (p.out || p.epilogue == W_EPI_C1W || p.epilogue == W_EPI_POOLV || p.epilogue == W_EPI_MASKY), "wino63v_nt: null V/Bw/out");
  TL_REQUIRE(p.loader == W_LOAD_V, "wino63v_nt: loader 2 (pre-transformed operand) only");
  TL_REQUIRE(p.J == 3 && p.splitk <= 1, "wino63v_nt: 3 taps, no split-K");
  TL_REQUIRE(p.M > 0 && p.M % 6 == 0 && p.N > 0 && p.K >= 40 && p.K % 8 == 0, "wino63v_nt: M %% 6, K %% 8, K >= 40 needed");
  TL_REQUIRE(p.lda >= p.K && p.ldb >= p.K && p.lda % 8 == 0 && p.ldb % 8 == 0, "wino63v_nt: bad leading dimensions (multiples of 8)");
  TL_REQUIRE(p.A_rows % 2 == 0, "wino63v_nt: V holds hex pairs");
  TL_REQUIRE(p.Tp > 0 && p.Tp % 6 == 0 && p.M % p.Tp == 0, "wino63v_nt: Tp must be a positive multiple of 6, M whole sequences");
  TL_REQUIRE(8LL * p.N * p.ldb * 4 < (1LL << 31), "wino63v_nt: tap set larger than a buffer resource");
  TL_REQUIRE(128LL * 8 * p.lda * 4 + 4LL * p.K < (1LL << 31), "wino63v_nt: tile span too large");
  const long long ntm = (p.M + V6_ROWS - 1) / V6_ROWS;
  const long long nwg = ntm * ((p.N + V6_BN - 1) / V6_BN);
  TL_REQUIRE(nwg < (1LL << 31), "wino63v_nt: grid too large");
  TL_REQUIRE(p.N % 32 == 0 && p.M + V6_ROWS < (1LL << 31), "wino63v_nt: N %% 32 == 0 and M < 2^31 - 768 needed");
  TL_REQUIRE(p.slope >= 0.f && p.slope <= 1.f, "wino63v_nt: LeakyReLU slope must lie in [0, 1]");
  if (p.a_hps_extra != 0) {
    // compact-M mode: M / Tp / Tvalid are the computed geometry, V stores a_hps_extra more hexes per sequence
    TL_REQUIRE(p.a_hps_extra > 0 && p.a_hps_extra <= 16, "wino63v_nt: compact M: a_hps_extra must lie in [0, 16]");
    TL_REQUIRE(p.epilogue == W_EPI_POOL || p.epilogue == W_EPI_MASKY, "wino63v_nt: compact M: POOL epilogue or epilogue 6 only");
    TL_REQUIRE(V6_BH % (p.Tp / 6) == 0, "wino63v_nt: compact M: tiles must start on sequence boundaries (128 %% (Tp / 6) == 0)");
    TL_REQUIRE(p.Tp == 96, "wino63v_nt: compact M: 16 computed hexes per sequence (Tp == 96) needed - a lane owns one sequence");
    TL_REQUIRE((128LL + 8 * p.a_hps_extra) * 8 * p.lda * 4 + 4LL * p.K < (1LL << 31), "wino63v_nt: compact M: tile span too large");
    TL_REQUIRE(p.A_rows >= ntm * 8 * (16 + p.a_hps_extra),
               "wino63v_nt: compact M: V must hold 8 (16 + a_hps_extra) hexes for every tile (pad it with zero hexes)");
  } else {
    TL_REQUIRE(p.A_rows >= ntm * V6_BH, "wino63v_nt: V must hold whole 128-hex tiles (pad it with zero hexes)");
  }
  hipStream_t st = (hipStream_t)stream;
  const long long ngrid = nwg < 256 ? nwg : 256;          // one workgroup per CU (144 - 160 KB of LDS each)
  if (p.epilogue == W_EPI_POOL) {
    TL_REQUIRE(p.row_shift == 0 && p.out && p.ldo >= p.N, "wino63v_nt: forward needs row_shift 0 and an output");
    TL_REQUIRE(p.obits != nullptr && p.Tvalid % 2 == 0 && p.Tvalid <= p.Tp, "wino63v_nt: POOL needs obits and an even Tvalid");
    TL_REQUIRE(p.ld_obits * 32 >= p.N, "wino63v_nt: POOL: ld_obits too small");
    TL_REQUIRE(p.out_tp >= 0 && (p.out_tp == 0 || 2 * p.out_tp >= p.Tvalid), "wino63v_nt: out_tp must cover the valid pooled rows");
    const long long orows = (p.M / p.Tp) * (long long)(p.out_tp > 0 ? p.out_tp : p.Tp / 2);
    TL_REQUIRE(orows * (long long)p.ldo * 4 < (1LL << 40), "wino63v_nt: output too large");
    hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_POOL>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
  } else if (p.epilogue == W_EPI_POOLV) {
    TL_REQUIRE(p.row_shift == 0 && (p.out == nullptr || p.ldo >= p.N), "wino63v_nt: forward needs row_shift 0");
    TL_REQUIRE(p.obits != nullptr && p.Tvalid % 2 == 0 && p.Tvalid <= p.Tp, "wino63v_nt: POOLV needs obits and an even Tvalid");
    TL_REQUIRE(p.ld_obits * 32 >= p.N && p.Tp % 12 == 0, "wino63v_nt: POOLV needs Tp %% 12 == 0 (output hexes inside one sequence)");
    TL_REQUIRE(p.vout && p.vhalo && p.ld_vout >= p.N && p.ld_vout % 8 == 0 && p.vout_quads >= p.M / 12 && p.vout_quads % 2 == 0,
               "wino63v_nt: POOLV needs vout (>= M / 12 hexes, whole pairs, ld_vout %% 8 == 0) and vhalo");
    TL_REQUIRE(64LL * 8 * p.ld_vout * 4 < (1LL << 31), "wino63v_nt: ld_vout too large");
    hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_POOLV>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
  } else if (p.epilogue == W_EPI_MASK) {
    TL_REQUIRE(p.row_shift == -2 && p.ldo >= p.N, "wino63v_nt: input gradient needs row_shift -2");
    TL_REQUIRE(p.auxbits != nullptr, "wino63v_nt: MASK needs auxbits (the sign bits of the stage input)");
    hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_MASK>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
  } else if (p.epilogue == W_EPI_MASKY && p.a_hps_extra != 0) {
    // whole-sequence tiles: the operand is Y of the stage (row_shift 0, taps of tl_wino63_weights_y), Y of the stage below is all
    // that is written; the bit arrays and vout count 6 / 2 (16 + a_hps_extra) rows / hexes per sequence
    const long long hps2 = 2LL * (16 + p.a_hps_extra);
    TL_REQUIRE(p.row_shift == 0 && p.auxbits != nullptr && p.abits != nullptr, "wino63v_nt: epilogue 6, compact M: needs row_shift 0 (operand Y), auxbits and abits");
    TL_REQUIRE(p.ld_abits * 32 >= p.N && p.ld_auxbits * 32 >= p.N && p.Tvalid_in >= 0 && p.Tvalid_in % 2 == 0 && p.Tvalid_in <= 2 * (p.Tp + 2),
               "wino63v_nt: epilogue 6, compact M: bad abits / auxbits / Tvalid_in (at most 2 (Tp + 2))");
    TL_REQUIRE(p.vout && p.ld_vout >= p.N && p.ld_vout % 8 == 0 && p.vout_quads >= (p.M / p.Tp) * hps2 && p.vout_quads % 2 == 0,
               "wino63v_nt: epilogue 6, compact M: needs vout (>= 2 (16 + a_hps_extra) hexes per sequence, whole pairs, ld_vout %% 8 == 0)");
    TL_REQUIRE(p.vout2 == nullptr && p.vhalo == nullptr, "wino63v_nt: epilogue 6, compact M: writes Y only (no vout2 / vhalo)");
    TL_REQUIRE(128LL * 8 * p.ld_vout * 4 < (1LL << 31), "wino63v_nt: ld_vout too large");
    hipLaunchKernelGGL((wino63v_nt_kernel<W6_EPI_MASKY_SEQ>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
  } else if (p.epilogue == W_EPI_MASKY) {
    TL_REQUIRE(p.row_shift == -2 && p.auxbits != nullptr && p.abits != nullptr, "wino63v_nt: epilogue 6 needs row_shift -2, auxbits and abits");
    TL_REQUIRE(p.ld_abits * 32 >= p.N && p.Tvalid_in % 2 == 0 && p.Tvalid_in <= 2 * p.Tp, "wino63v_nt: epilogue 6: bad abits / Tvalid_in");
    TL_REQUIRE(p.vout && p.ld_vout >= p.N && p.ld_vout % 8 == 0 && p.vout_quads >= p.M / 3 && p.vout_quads % 2 == 0,
               "wino63v_nt: epilogue 6 needs vout (>= M / 3 hexes, whole pairs, ld_vout %% 8 == 0)");
    TL_REQUIRE((p.vout2 == nullptr) == (p.vhalo == nullptr), "wino63v_nt: epilogue 6 takes vout2 and vhalo together (Y and Vd) or neither (Y only)");
    TL_REQUIRE(128LL * 8 * p.ld_vout * 4 < (1LL << 31), "wino63v_nt: ld_vout too large");
    // without vout2 / vhalo: Y only (the stage below runs its input gradient on Y); its fix-up pass has nothing to do then
    if (p.vout2 != nullptr) hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_MASKY>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
    else hipLaunchKernelGGL((wino63v_nt_kernel<W6_EPI_MASKY_Y>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
  } else if (p.epilogue == W_EPI_C1W) {
    // row_shift -2: A = Vd (B^T of the un-pooled gradient rows 6 H - 2 .. 6 H + 5), flipped taps; row_shift 0: A = Y (A dz of
    // rows 6 H .. 6 H + 5), taps of tl_wino63_weights_y - hex H yields rows 6 H .. 6 H + 7
    TL_REQUIRE(p.row_shift == -2 || p.row_shift == 0, "wino63v_nt: epilogue 4 needs row_shift -2 (operand Vd) or 0 (operand Y)");
    TL_REQUIRE(p.auxbits && p.c1x && p.c1bits && p.c1partial, "wino63v_nt: epilogue 4 needs auxbits, c1x, c1bits, c1partial");
    TL_REQUIRE(p.c1kt >= 1 && p.c1kt <= 3 && p.c1T >= 2 * p.Tvalid + 2, "wino63v_nt: epilogue 4: 1..3 taps, c1T >= 2*Tvalid + 2");
    TL_REQUIRE(p.Tvalid >= 0 && p.Tvalid <= p.Tp, "wino63v_nt: epilogue 4: Tvalid must lie in [0, Tp]");
    if (p.row_shift == -2) hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_C1W>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
    else hipLaunchKernelGGL((wino63v_nt_kernel<W6_EPI_C1W_Y>), dim3((unsigned)ngrid), dim3(512), 0, st, p);
  } else {
    set_error("wino63v_nt: unsupported epilogue %d", p.epilogue);
    return TL_EINVAL;
  }
  return check_launch("wino63v_nt");
}

// Input gradient of a one-tap pooled stage on the NT63 kernel, epilogue 7 (kernel comment above wino63_unpool_rows6_kernel)
extern "C" int tl_wino63_unpool_rows6(const float* G, const uint32_t* bits, float* A, int64_t rows, int64_t g_rows, int Tp, int g_tp,
                                      int Tvalid, int C, int ldg, int ld_bits, int lda, int pad, void* stream) {
  using namespace tl;
  TL_REQUIRE(G && bits && A, "wino63_unpool_rows6: null pointer");
  TL_REQUIRE(rows > 0 && Tp > 0 && rows % Tp == 0 && Tvalid > 0 && Tvalid <= Tp, "wino63_unpool_rows6: whole sequences of Tp rows, 0 < Tvalid <= Tp needed");
  TL_REQUIRE(g_tp > 0 && 2 * g_tp >= Tvalid && g_rows >= (rows / Tp) * (long long)g_tp, "wino63_unpool_rows6: G holds fewer rows than sequences x g_tp");
  TL_REQUIRE(C > 0 && C % 8 == 0 && ldg >= C && ldg % 4 == 0 && lda >= C && lda % 8 == 0 && ld_bits * 32 >= C,
             "wino63_unpool_rows6: C %% 8, ldg %% 4, lda %% 8 needed, bits row must cover C");
  const long long nhex = (rows + 5) / 6;
  const long long n = (nhex + 1) / 2 * (C >> 1);
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_unpool_rows6: grid too large");
  hipLaunchKernelGGL(wino63_unpool_rows6_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G, bits, A,
                     nhex, (long long)rows, (long long)g_rows, Tp, g_tp, Tvalid, C, ldg, ld_bits, lda, pad);
  return check_launch("wino63_unpool_rows6");
}

extern "C" int tl_wino63_weights1(const float* w, float* taps, int O, int I, int ldb, void* stream) {
  using namespace tl;
  TL_REQUIRE(w && taps && O > 0 && I > 0 && ldb >= O && ldb % 8 == 0, "wino63_weights1: w, taps, O, I > 0 and ldb %% 8 == 0, ldb >= O needed");
  const long long n = (long long)ldb * 8 * I;
  TL_REQUIRE((n + 255) / 256 < (1LL << 31), "wino63_weights1: too large");
  hipLaunchKernelGGL(wino63_weights1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, taps, O, I, ldb);
  return check_launch("wino63_weights1");
}

extern "C" int tl_conv1_wino63v_dgrad_nt(const tl_nt_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "conv1_wino63v_dgrad_nt: null params");
  const tl_nt_params& p = *pp;
  TL_REQUIRE(p.A && p.Bw, "conv1_wino63v_dgrad_nt: null A / taps");
  TL_REQUIRE(p.loader == W_LOAD_V && p.epilogue == W_EPI_GY && p.J == 1 && p.row_shift == 0 && p.splitk <= 1,
             "conv1_wino63v_dgrad_nt: loader 2, epilogue 7, one tap, row_shift 0, no split-K");
  TL_REQUIRE(p.M > 0 && p.N > 0 && p.K >= 40 && p.K % 8 == 0, "conv1_wino63v_dgrad_nt: K %% 8, K >= 40 needed");
  TL_REQUIRE(p.Tp > 0 && p.Tp % 3 == 0 && p.M % p.Tp == 0, "conv1_wino63v_dgrad_nt: Tp (rows per sequence) must be a multiple of 3, M whole sequences");
  TL_REQUIRE(p.lda >= p.K && p.ldb >= p.K && p.lda % 8 == 0 && p.ldb % 8 == 0, "conv1_wino63v_dgrad_nt: bad leading dimensions (multiples of 8)");
  TL_REQUIRE(p.A_rows % 2 == 0, "conv1_wino63v_dgrad_nt: A holds hex pairs");
  TL_REQUIRE(8LL * p.N * p.ldb * 4 < (1LL << 31), "conv1_wino63v_dgrad_nt: tap set larger than a buffer resource");
  TL_REQUIRE(128LL * 8 * p.lda * 4 + 4LL * p.K < (1LL << 31), "conv1_wino63v_dgrad_nt: tile span too large");
  const long long ntm = (p.M + V6_ROWS - 1) / V6_ROWS;
  const long long nwg = ntm * ((p.N + V6_BN - 1) / V6_BN);
  TL_REQUIRE(nwg < (1LL << 31), "conv1_wino63v_dgrad_nt: grid too large");
  TL_REQUIRE(p.N % 32 == 0 && p.M + V6_ROWS < (1LL << 31), "conv1_wino63v_dgrad_nt: N %% 32 == 0 and M < 2^31 - 768 needed");
  TL_REQUIRE(p.slope >= 0.f && p.slope <= 1.f, "conv1_wino63v_dgrad_nt: LeakyReLU slope must lie in [0, 1]");
  TL_REQUIRE(p.A_rows >= ntm * V6_BH, "conv1_wino63v_dgrad_nt: A must hold whole 128-hex tiles (pad it with zero hexes)");
  TL_REQUIRE(p.a_hps_extra == 0, "conv1_wino63v_dgrad_nt: no compact-M mode (a_hps_extra must be 0)");
  TL_REQUIRE(p.auxbits != nullptr && p.abits != nullptr, "conv1_wino63v_dgrad_nt: needs auxbits (sign) and abits (arg-max) of the stage below");
  TL_REQUIRE(p.out_tp > 0 && p.out_tp <= p.Tp && 2 * p.out_tp >= p.Tvalid_in, "conv1_wino63v_dgrad_nt: out_tp = rows per sequence of the bit arrays (0 < out_tp <= Tp, covering Tvalid_in / 2)");
  TL_REQUIRE(p.ld_abits * 32 >= p.N && p.ld_auxbits * 32 >= p.N && p.Tvalid_in % 2 == 0 && p.Tvalid_in <= 2 * p.Tp, "conv1_wino63v_dgrad_nt: bad abits / auxbits / Tvalid_in");
  TL_REQUIRE(p.vout && p.ld_vout >= p.N && p.ld_vout % 8 == 0 && p.vout_quads >= p.M / 3 && p.vout_quads % 2 == 0,
             "conv1_wino63v_dgrad_nt: needs vout (>= M / 3 hexes, whole pairs, ld_vout %% 8 == 0)");
  TL_REQUIRE((p.vout2 == nullptr) == (p.vhalo == nullptr),
             "conv1_wino63v_dgrad_nt: takes vout2 and vhalo together (Y and Vd) or neither (Y only: the stage below runs its input gradient on Y)");
  TL_REQUIRE(128LL * 8 * p.ld_vout * 4 < (1LL << 31), "conv1_wino63v_dgrad_nt: ld_vout too large");
  const long long ngrid = nwg < 256 ? nwg : 256;
  if (p.vout2 != nullptr) hipLaunchKernelGGL((wino63v_nt_kernel<W_EPI_GY>), dim3((unsigned)ngrid), dim3(512), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((wino63v_nt_kernel<W6_EPI_GY_Y>), dim3((unsigned)ngrid), dim3(512), 0, (hipStream_t)stream, p);
  return check_launch("conv1_wino63v_dgrad_nt");
}

// weight gradient on V: A = V[hex][8][lda], A_rows = hexes held by V (a whole number of 6-hex K-steps)
extern "C" int tl_conv3_wino63v_tn(const tl_tn_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "wino63v_tn: null params");
  tl_tn_params p = *pp;
  if (p.splitk < 1) p.splitk = 1;
  if (p.loader == 3) {
    // both operands pre-transformed: B = Y[hex][8][ldb] (pair layout) from the MASKY epilogue of the stage above
    TL_REQUIRE(p.A && p.B && p.slab, "wino63v_tn: null V/Y/slab");
    TL_REQUIRE(p.J == 3 && p.Tp > 0 && p.Tp % 6 == 0 && p.Krows > 0 && p.Krows % p.Tp == 0, "wino63v_tn: loader 3: bad Tp / Krows");
    TL_REQUIRE(p.Krows + 64 < (1LL << 31), "wino63v_tn: more than 2^31 reduction rows");
    TL_REQUIRE(p.Mdim % 256 == 0 && p.Ndim % 64 == 0 && p.lda % 8 == 0 && p.ldb % 8 == 0 && p.lda >= p.Mdim && p.ldb >= p.Ndim &&
               p.ldc >= p.Ndim, "wino63v_tn: loader 3 needs Mdim %% 256, Ndim %% 64, lda / ldb %% 8");
    TL_REQUIRE(p.A_rows % 2 == 0 && p.B_rows % 2 == 0 && p.vd == nullptr, "wino63v_tn: loader 3: whole hex pairs in V and Y, no Vd");
    TL_REQUIRE(p.a_hex == 0 || p.a_hex == 1, "wino63v_tn: loader 3: a_hex must be 0 or 1");
    TL_REQUIRE(p.splitk <= 65535 && (p.splitk == 1 || p.slab_stride >= 8LL * p.Mdim * p.ldc), "wino63v_tn: bad splitk / slab_stride");
    const long long ks = (p.Krows / 6 + T6_H - 1) / T6_H;
    TL_REQUIRE(p.A_rows >= ks * T6_H && p.B_rows >= ks * T6_H, "wino63v_tn: V and Y must hold whole 6-hex K-steps (pad with zero hexes)");
    const long long per3 = (ks + p.splitk - 1) / p.splitk;
    TL_REQUIRE((per3 + 4) * (long long)T6_H * 8 * p.lda * 4 < (1LL << 31) && (per3 + 4) * (long long)T6_H * 8 * p.ldb * 4 < (1LL << 31),
               "wino63v_tn: a reduction split spans more than 2 GB of V or Y: raise splitk");
    const int ntm3 = p.Mdim / 256;
    hipLaunchKernelGGL(wino63v_tn4y_kernel, dim3((unsigned)(2 * ntm3 * (p.Ndim / T6_BN)), (unsigned)p.splitk, 1), dim3(512), 0,
                       (hipStream_t)stream, p, ntm3);
    return check_launch("wino63v_tn (both operands pre-transformed)");
  }
  TL_REQUIRE(p.A && p.B && p.slab && p.bbits, "wino63v_tn: null V/B/bbits/slab");
  TL_REQUIRE(p.a_hex == 0, "wino63v_tn: a_hex needs loader 3 (both operands pre-transformed)");
  TL_REQUIRE(p.J == 3 && p.loader == 1, "wino63v_tn: 3 taps, UNPOOL loader (1) or pre-transformed Y (3)");
  TL_REQUIRE(p.Tp > 0 && p.Tp % 6 == 0 && p.Tvalid % 2 == 0 && p.Tvalid <= p.Tp, "wino63v_tn: Tp %% 6 == 0 and an even Tvalid <= Tp needed");
  TL_REQUIRE(p.Krows > 0 && p.Krows % p.Tp == 0 && p.Mdim > 0 && p.Ndim > 0, "wino63v_tn: bad sizes (Krows must be whole sequences)");
  TL_REQUIRE(p.Krows + 64 < (1LL << 31), "wino63v_tn: more than 2^31 reduction rows");
  TL_REQUIRE(p.Mdim % 128 == 0 && p.Ndim % 64 == 0 && p.lda % 8 == 0 && p.ldb % 4 == 0 && p.A_rows % 2 == 0,
             "wino63v_tn: Mdim %% 128, Ndim %% 64, lda %% 8, ldb %% 4, whole hex pairs in V needed");
  TL_REQUIRE(p.lda >= p.Mdim && p.ldb >= p.Ndim && p.ldc >= p.Ndim, "wino63v_tn: leading dimension too small");
  TL_REQUIRE(p.ld_bbits * 32 >= p.Ndim && p.ld_bbits % 2 == 0, "wino63v_tn: bbits row too short / odd");
  TL_REQUIRE(p.splitk <= 65535, "wino63v_tn: splitk too large");
  TL_REQUIRE(p.splitk == 1 || p.slab_stride >= 8LL * p.Mdim * p.ldc, "wino63v_tn: slab_stride smaller than 8*Mdim*ldc");
  const int g_tp = p.g_tp > 0 ? p.g_tp : p.Tp / 2;
  TL_REQUIRE(2 * g_tp >= p.Tvalid, "wino63v_tn: g_tp must cover the valid pooled rows");
  TL_REQUIRE(p.B_rows >= (p.Krows / p.Tp) * (long long)g_tp && p.B_rows < (1LL << 30), "wino63v_tn: G holds fewer rows than sequences x g_tp");
  const long long ksteps_all = (p.Krows / 6 + T6_H - 1) / T6_H;
  TL_REQUIRE(p.A_rows >= (ksteps_all + 3) * T6_H, "wino63v_tn: V must hold whole 6-hex K-steps and three more (pad it with zero hexes)");
  const long long per = (ksteps_all + p.splitk - 1) / p.splitk;
  TL_REQUIRE((per + 4) * (long long)T6_H * 8 * p.lda * 4 < (1LL << 31), "wino63v_tn: a reduction split spans more than 2 GB of V: raise splitk");
  TL_REQUIRE((per + 6) * 3LL * T6_H * p.ldb * 4 < (1LL << 31), "wino63v_tn: a reduction split spans more than 2 GB of G: raise splitk");
  TL_REQUIRE(p.vd == nullptr || (p.ld_vd >= p.Ndim && p.ld_vd % 8 == 0), "wino63v_tn: ld_vd must cover Ndim (multiple of 8)");
  TL_REQUIRE(p.vd == nullptr || (per + 4) * (long long)T6_H * 8 * p.ld_vd * 4 < (1LL << 31), "wino63v_tn: a reduction split spans more than 2 GB of Vd: raise splitk");
  const int ntn = p.Ndim / T6_BN;
  hipStream_t st = (hipStream_t)stream;
  // C_in a multiple of 256: the kernel that splits the eight transforms over two workgroups (bm = 128 asks for the other one)
  TL_REQUIRE(p.bm == 0 || p.bm == 128 || (p.bm == 256 && p.Mdim % 256 == 0 && p.Tp >= 12),
             "wino63v_tn: bm must be 0, 128, or 256 with Mdim %% 256 == 0 and Tp >= 12");
  if (p.bm == 256 || (p.bm == 0 && p.Mdim % 256 == 0 && p.Tp >= 12)) {
    const int ntm = p.Mdim / 256;
    const dim3 grid((unsigned)(2 * ntm * ntn), (unsigned)p.splitk, 1);
    if (p.vd != nullptr) hipLaunchKernelGGL((wino63v_tn4_kernel<true>), grid, dim3(512), 0, st, p, ntm);
    else hipLaunchKernelGGL((wino63v_tn4_kernel<false>), grid, dim3(512), 0, st, p, ntm);
    return check_launch("wino63v_tn (4 transforms per workgroup)");
  }
  const int ntm = p.Mdim / 128;
  const dim3 grid((unsigned)(ntm * ntn), (unsigned)p.splitk, 1);
  if (p.vd != nullptr) hipLaunchKernelGGL((wino63v_tn_kernel<true>), grid, dim3(512), 0, st, p, ntm);
  else hipLaunchKernelGGL((wino63v_tn_kernel<false>), grid, dim3(512), 0, st, p, ntm);
  return check_launch("wino63v_tn");
}

extern "C" int tl_conv1_fwd_v6(const float* x, const float* w, const float* b, float* P, float* V, uint32_t* bits, uint32_t* sign,
                               int64_t S, int T, int ktaps, int C1, int Tp, int Tout, float slope, void* stream) {
  using namespace tl;
  TL_REQUIRE(x && w && b && V && bits, "conv1_fwd_v6: null pointer");
  TL_REQUIRE(S > 0 && S < (1LL << 31) && T > 0, "conv1_fwd_v6: bad sizes");
  TL_REQUIRE(ktaps >= 1 && ktaps <= C1_MAXKT, "conv1_fwd_v6: ktaps must be 1..%d", C1_MAXKT);
  TL_REQUIRE(C1 % 128 == 0 && C1 <= 1024 && (C1 & (C1 - 1)) == 0, "conv1_fwd_v6: C1 must be 128, 256, 512 or 1024");
  TL_REQUIRE(Tp > 0 && Tp % 6 == 0, "conv1_fwd_v6: Tp must be a multiple of 6");
  TL_REQUIRE(Tout >= 0 && Tout <= Tp && 2 * Tout + ktaps - 1 <= T, "conv1_fwd_v6: Tout/Tp/T inconsistent (%d,%d,%d)", Tout, Tp, T);
  TL_REQUIRE((size_t)T * 4 <= 64 * 1024, "conv1_fwd_v6: T too large for the LDS window");
#define TL_C1V_LAUNCH(KT_)                                                                                                   \
  case KT_:                                                                                                                  \
    hipLaunchKernelGGL(conv1_fwd_vh_kernel<KT_>, dim3((unsigned)S), dim3(256), (size_t)T * 4, (hipStream_t)stream, x, w, b, P, V, \
                       bits, sign, (long long)S, T, C1, Tp, Tout, slope);                                                    \
    break;
  switch (ktaps) {                               // the tap count is a template parameter: straight-line row arithmetic
    TL_C1V_LAUNCH(1) TL_C1V_LAUNCH(2) TL_C1V_LAUNCH(3) TL_C1V_LAUNCH(4) TL_C1V_LAUNCH(5) TL_C1V_LAUNCH(6) TL_C1V_LAUNCH(7)
    TL_C1V_LAUNCH(8)
  }
#undef TL_C1V_LAUNCH
  return check_launch("conv1_fwd_v6");
}
