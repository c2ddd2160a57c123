// fp32 MFMA implicit-GEMM kernels for gfx950 (MI355X): windowed NT (forward / input-gradient
// of the (k,1) convolutions, Linear, LSTM h.W_hh^T) and windowed TN (weight gradients).
//
// Both use v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD).  A single accumulator chain
// already issues back to back (64-cycle issue = 64-cycle dependent latency), so the design
// effort goes into keeping the matrix pipe fed: register-staged global loads issued one K-step
// ahead, LDS double buffering with one barrier per K-step, 2 workgroups (8 waves) per CU.
#include "tonal_common.h"
#include <stdlib.h>

namespace tl {

constexpr int BN = 128;   // column tile
constexpr int BK = 32;    // K depth of one LDS stage
constexpr int LDS_LD = BK + 4;   // 36 floats = 144 B rows: conflict-free ds_read_b128 (9 odd)

enum { LOAD_DIRECT = 0, LOAD_UNPOOL = 1 };
enum { EPI_STORE = 0, EPI_LRELU = 1, EPI_POOL = 2, EPI_MASK = 3 };

// ------------------------------------------------------------------------------------------
// NT window kernel
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// shared epilogue of the NT kernels.  C/D map of 32x32x2: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
// ------------------------------------------------------------------------------------------
template <int EPI, int MI, int NI>
__device__ __forceinline__ void nt_epilogue(const tl_nt_params& p, f32x16 (&acc)[MI][NI], long long R0, int n0, int wm,
                                            int wn, int lr, int lh, int z) {
  // C/D map of 32x32x2: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int col = n0 + wn * (NI * 32) + ni * 32 + lr;
      const bool colok = col < p.N;
      const long long rbase = R0 + wm * (MI * 32) + mi * 32;
      if constexpr (EPI == EPI_POOL) {
        const float bv = (colok && p.bias) ? p.bias[col] : 0.f;
        int tq = (int)((rbase + 4 * lh) % p.Tp);              // time index of row rbase + 4 lh; rows below step by 2 / 8
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const long long Rq = rbase + 8 * q + 4 * lh;        // even conv row of this lane's 4 rows
          if (q > 0) {
            tq += 8;
            while (tq >= p.Tp) tq -= p.Tp;
          }
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float y0 = lrelu(acc[mi][ni][4 * q + 2 * e] + bv, p.slope);
            const float y1 = lrelu(acc[mi][ni][4 * q + 2 * e + 1] + bv, p.slope);
            const bool rowok = (Rq + 2 * e) < p.M;              // Tp, Tvalid even: the pair shares validity
            int te = tq + 2 * e;
            if (te >= p.Tp) te -= p.Tp;
            const bool valid_e = rowok && te < p.Tvalid;
            const bool sel = valid_e && colok && (y1 > y0);
            const float o = valid_e ? (sel ? y1 : y0) : 0.f;
            const long long prow = (Rq >> 1) + e;
            if (rowok && colok) p.out[prow * (long long)p.ldo + col] = o;
            const unsigned long long m = __ballot(sel);
            const unsigned long long ms = __ballot(o > 0.f);
            if (lr == 0 && rowok && (n0 + wn * (NI * 32) + ni * 32) < p.N) {
              const long long at = prow * (long long)p.ld_obits + ((n0 + wn * (NI * 32) + ni * 32) >> 5);
              p.obits[at] = (uint32_t)(m >> (32 * lh));
              if (p.osign != nullptr) p.osign[at] = (uint32_t)(ms >> (32 * lh));
            }
          }
        }
      } else {
        float bv = 0.f;
        if constexpr (EPI == EPI_STORE || EPI == EPI_LRELU) bv = (colok && p.bias && p.splitk == 1) ? p.bias[col] : 0.f;
        float* outp = p.out + (long long)z * p.slab_stride;
        // MASK from sign bits: the 16 words this lane group needs (one per row) are fetched by lanes
        // 0..15 of each half-wave up front and read back with a shuffle - no dependent load per row
        uint32_t sword = 0;
        if constexpr (EPI == EPI_MASK) {
          if (p.auxbits != nullptr) {
            const int es = lr & 15;
            const long long Rs = rbase + (es & 3) + 8 * (es >> 2) + 4 * lh;
            const int cb = n0 + wn * (NI * 32) + ni * 32;
            if (Rs < p.M && cb < p.N) sword = p.auxbits[Rs * (long long)p.ld_auxbits + (cb >> 5)];
          }
        }
        // MASK from the stage input itself (no sign words: the 1x1 stack): all 16 values of the tile are requested before the
        // first store - behind a store the compiler may not move a load that could alias it, and one dependent load per row
        // (16 round trips per 32 x 32 tile) made this epilogue the longest part of a short-K launch
        float ax[16];
        if constexpr (EPI == EPI_MASK) {
          if (p.auxbits == nullptr) {
            // (through a buffer resource like the stores below: rows from M on and columns from N on read 0)
            const long long ab = (p.M - rbase) * (long long)p.ldaux * 4;
            const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(p.aux + rbase * (long long)p.ldaux), 0, (int)(ab <= 0 ? 0 : (ab < 0x7fffffffLL ? ab : 0x7fffffffLL)), 0x00020000);
            const unsigned lda4 = (unsigned)p.ldaux * 4u;
            const unsigned xo0 = colok ? (unsigned)(4 * lh) * lda4 + (unsigned)col * 4u : 0x80000000u;
#pragma unroll
            for (int e = 0; e < 16; ++e)
              ax[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsX, xo0 + (unsigned)((e & 3) + 8 * (e >> 2)) * lda4, 0u, 0));
          }
        }
        // stores through a buffer resource over the rows of this 32-row tile that exist (rows from M on are past its end and
        // dropped by the range check; a lane whose column is past N carries an offset no resource reaches): one 32-bit add per
        // store instead of a 64-bit address and a branch
        const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(outp + rbase * (long long)p.ldo), 0,
            (int)((p.M - rbase) <= 0 ? 0 : ((p.M - rbase) * (long long)p.ldo * 4 < 0x7fffffffLL ? (p.M - rbase) * (long long)p.ldo * 4 : 0x7fffffffLL)),
            0x00020000);
        const unsigned ldo4 = (unsigned)p.ldo * 4u;
        const unsigned vo0 = colok ? (unsigned)(4 * lh) * ldo4 + (unsigned)col * 4u : 0x80000000u;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          uint32_t word = 0;
          if constexpr (EPI == EPI_MASK) word = __shfl(sword, e + 32 * lh);
          float v = acc[mi][ni][e] + bv;
          if constexpr (EPI == EPI_LRELU) v = lrelu(v, p.slope);
          if constexpr (EPI == EPI_MASK) {
            bool pos;
            if (p.auxbits != nullptr)
              pos = (word >> lr) & 1u;
            else
              pos = ax[e] > 0.f;
            v = pos ? v : v * p.slope;
          }
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsO, vo0 + (unsigned)((e & 3) + 8 * (e >> 2)) * ldo4, 0u, 0);
        }
      }
    }
  }
}

// BM = 256 runs 8 waves (512 threads, 4 x 2): the per-thread staging work per MFMA halves, which is
// what limits the 128-row variant (scripts/mfma_ablate.hip); BM = 32 is the skinny-M streaming form.
template <int BM>
struct nt_cfg {
  static constexpr int NTHR = (BM == 256) ? 512 : 256;
  static constexpr int WM = (BM == 256) ? 4 : ((BM == 128) ? 2 : 1);   // waves along M
  static constexpr int WN = (NTHR / 64) / WM;                            // waves along N
};

// Each NT kernel body is a file of statements (tonal_gemm_nt_*_body.h) included into two __global__ functions: the single
// launch (tl_gemm_nt_window) and the group launch (tl_gemm_nt_window_group: member blockIdx.z works on pointers moved by its
// strides), so a member's tile runs the arithmetic of the single launch's tile in its order.  Text, not a __device__ function:
// inlined from a function the single kernels came out with other registers and another schedule than they had.
struct nt_group {
  long long s_A, s_Bw, s_bias, s_out;   // member strides, elements
  const int32_t* active;                // M words or null; 0: the member's workgroups return at once
  long long s_aux;                      // ... of aux (the MASK epilogue of tl_gemm_nt_window_group_fc)
};

// member blockIdx.z's parameters; false: the member is masked out (uniform over the workgroup - before any load or barrier)
__device__ __forceinline__ bool nt_member(tl_nt_params& p, const nt_group& g) {
  const int mem = blockIdx.z;
  if (g.active != nullptr && g.active[mem] == 0) return false;
  p.A += mem * g.s_A;
  p.Bw += mem * g.s_Bw;
  if (p.bias != nullptr) p.bias += mem * g.s_bias;
  if (p.aux != nullptr) p.aux += mem * g.s_aux;
  p.out += mem * g.s_out;
  return true;
}

template <int BM, int LOADER, int EPI>
__global__ __launch_bounds__(nt_cfg<BM>::NTHR, 2) void nt_window_kernel(const tl_nt_params p) {
#include "tonal_gemm_nt_window_body.h"
}

template <int BM, int LOADER, int EPI>
__global__ __launch_bounds__(nt_cfg<BM>::NTHR, 2) void nt_window_group_kernel(tl_nt_params p, const nt_group g) {
  if (!nt_member(p, g)) return;
#include "tonal_gemm_nt_window_body.h"
}


// ------------------------------------------------------------------------------------------
// NT window kernel, direct-to-LDS staging (global_load_lds_dwordx4): no staging VGPRs, no ds_write.
// In the register-staged kernel the B (weight) tile costs 6-7 % and the A tile 1-6 % of the matrix
// pipe (ablation with build variants); here a K-stage is 16 deep, B lives in a 4-slot LDS ring
// (three K-steps of latency tolerance), A in 2 slots, and one counted s_waitcnt + raw s_barrier
// closes a step.  LDS rows are 64 B (unpadded, as the DMA requires a lane-linear image); the 16-B
// chunk index is XOR-swizzled with (row >> 2) & 3 on the per-lane SOURCE address and on the
// fragment read, which makes the ds_read_b128 of 16 consecutive rows conflict-free.
// Preconditions (host-checked): DIRECT loader, row_shift == 0, K % 16 == 0, no tap window past A_rows (J == 1 or A_rows >= M + J - 1).
// ------------------------------------------------------------------------------------------
constexpr int GK = 16;                 // K depth of a stage
constexpr int G_AROWS = 144;           // 130 staged rows, 9 DMA pieces of 16 rows
constexpr int G_NB = 4;                // B ring slots

// NI = 32 x 32 tiles per wave along N: 2 = the 128-column tile, 1 = a 64-column tile for N <= 64 (the last layer of the 1x1 stack,
// conv5: with the 128-column tile half of their MFMAs were masked columns)
template <int EPI, int NI>
__global__ __launch_bounds__(256, 2) void nt_glds_kernel(const tl_nt_params p) {
#include "tonal_gemm_nt_glds_body.h"
}

template <int EPI, int NI>
__global__ __launch_bounds__(256, 2) void nt_glds_group_kernel(tl_nt_params p, const nt_group g) {
  if (!nt_member(p, g)) return;
#include "tonal_gemm_nt_glds_body.h"
}

template <int EPI>
static int launch_glds(const tl_nt_params& p, hipStream_t st) {
  const bool narrow = p.N <= 64 && p.J == 1;              // one 64-column tile (the wait counts of the narrow form cover J == 1)
  const int bn = narrow ? 64 : BN;
  const long long nwg = ((p.M + 127) / 128) * ((p.N + bn - 1) / bn);
  if (nwg <= 0) return TL_OK;
  TL_REQUIRE(nwg < (1LL << 31), "nt_glds: grid too large");
  dim3 grid((unsigned)nwg, (unsigned)p.splitk, 1);
  if (narrow)
    hipLaunchKernelGGL((nt_glds_kernel<EPI, 1>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((nt_glds_kernel<EPI, 2>), grid, dim3(256), 0, st, p);
  return check_launch("nt_glds");
}

template <int BM, int LOADER, int EPI>
static int launch_nt(const tl_nt_params& p, hipStream_t st) {
  const long long ntm = (p.M + BM - 1) / BM;
  const long long ntn = (p.N + BN - 1) / BN;
  const long long nwg = ntm * ntn;
  if (nwg <= 0) return TL_OK;
  TL_REQUIRE(nwg < (1LL << 31), "nt_window: grid too large");
  dim3 grid((unsigned)nwg, (unsigned)p.splitk, 1);
  hipLaunchKernelGGL((nt_window_kernel<BM, LOADER, EPI>), grid, dim3(nt_cfg<BM>::NTHR), 0, st, p);
  return check_launch("nt_window");
}

template <int BM>
static int dispatch_nt(const tl_nt_params& p, hipStream_t st) {
  if constexpr (BM == 32) {
    if (p.loader != LOAD_DIRECT) {
      set_error("nt_window: bm = 32 supports the DIRECT loader only");
      return TL_EINVAL;
    }
  }
  if (p.loader == LOAD_DIRECT) {
    switch (p.epilogue) {
      case EPI_STORE: return launch_nt<BM, LOAD_DIRECT, EPI_STORE>(p, st);
      case EPI_LRELU: return launch_nt<BM, LOAD_DIRECT, EPI_LRELU>(p, st);
      case EPI_POOL: return launch_nt<BM, LOAD_DIRECT, EPI_POOL>(p, st);
      case EPI_MASK: return launch_nt<BM, LOAD_DIRECT, EPI_MASK>(p, st);
    }
  } else if constexpr (BM != 32) {
    switch (p.epilogue) {
      case EPI_STORE: return launch_nt<BM, LOAD_UNPOOL, EPI_STORE>(p, st);
      case EPI_MASK: return launch_nt<BM, LOAD_UNPOOL, EPI_MASK>(p, st);
    }
  }
  set_error("nt_window: unsupported loader/epilogue combination %d/%d", p.loader, p.epilogue);
  return TL_EINVAL;
}

// ------------------------------------------------------------------------------------------
// TN window kernel: slab[z][j*Mdim + m][n] = sum_R A[R + j][m] * Bz[R][n]
// LDS tiles are k-major ([BK][128 + 4]); fragments are conflict-free ds_read_b32.
// ------------------------------------------------------------------------------------------
constexpr int TN_LD = 128 + 4;

template <int LOADER>
__global__ __launch_bounds__(256, 2) void tn_window_kernel(const tl_tn_params p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * BK * TN_LD];
  float* As = lds;                        // [2][BK][TN_LD]
  float* Bs = lds + 2 * BK * TN_LD;       // [2][BK][TN_LD]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;

  const int ntm1 = (p.Mdim + 127) / 128;          // m tiles per tap
  const int ntn = (p.Ndim + 127) / 128;
  // Work item = (split z, tap j, m tile, n tile).  Every tile of one split reads the SAME rows of
  // A and B, so all tiles of a split must share an L2: blocks b and b+8 sit on one XCD, hence the
  // bijective remap that hands each XCD a contiguous run of work items (split-major).
  const long long tiles = (long long)ntm1 * ntn * p.J;
  const long long nwg = tiles * p.splitk;
  long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  {
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const int z = (int)(bid / tiles);
  int tid_tile = (int)(bid % tiles);
  const int tn = tid_tile % ntn;
  tid_tile /= ntn;
  const int tm = tid_tile % ntm1;
  const int j = tid_tile / ntm1;
  const int m0 = tm * 128, n0 = tn * 128;

  const long long ksteps_all = (p.Krows + BK - 1) / BK;
  const long long per = (ksteps_all + p.splitk - 1) / p.splitk;
  const long long ks_begin = z * per;
  long long ks_end = ks_begin + per;
  if (ks_end > ksteps_all) ks_end = ksteps_all;
  const long long nsteps = ks_end > ks_begin ? ks_end - ks_begin : 0;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  // column sums of B over this split (the bias gradient of a one-tap layer: B = the layer's output gradient): the first row
  // tile's workgroup of a (split, column tile) adds up the rows it stages anyway - no pass of its own over B
  const bool do_cs = LOADER == LOAD_DIRECT && p.colsum != nullptr && tm == 0 && j == 0;
  f32x4 cs = {0.f, 0.f, 0.f, 0.f};

  // two staging sets (P/Q): tiles are prefetched two K-steps ahead
  f32x4 raP[4], rbP[4], raQ[4], rbQ[4];
  uint32_t rnP[2], rnQ[2];
  (void)rnP; (void)rnQ;

  // Hoisted per-thread state: row pointers advance by a wave-uniform stride per K-step, column
  // validity is loop-invariant, row validity ((row % Tp) < Tvalid) is tracked incrementally.
  constexpr int NB = (LOADER == LOAD_DIRECT) ? 4 : 2;
  const int a_lim = (int)(p.A_rows < p.Krows + j ? p.A_rows : p.Krows + j);
  const int b_lim = (LOADER == LOAD_DIRECT) ? (int)(p.B_rows < p.Krows ? p.B_rows : p.Krows)
                                            : (int)(2 * p.B_rows < p.Krows ? 2 * p.B_rows : p.Krows);
  const int kbase = (int)(ks_begin * BK);
  const float* aptr[4];
  int arow[4];
  const bool amok = (m0 + (tid & 31) * 4) < p.Mdim;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (tid + i * 256) >> 5;
    arow[i] = kbase + r + j;
    aptr[i] = p.A + (long long)arow[i] * p.lda + m0 + (tid & 31) * 4;
  }
  const float* bptr[NB];
  const uint32_t* bbptr[NB];
  int brow[NB], bt[NB];
  (void)bbptr;
  const int ncol = n0 + (tid & 31) * 4;
  const bool bnok = ncol < p.Ndim;
  const int dstep = BK % p.Tp;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int r = (tid + i * 256) >> 5;
    if constexpr (LOADER == LOAD_DIRECT) {
      brow[i] = kbase + r;                              // B row
      bptr[i] = p.B + (long long)brow[i] * p.ldb + ncol;
      bbptr[i] = nullptr;
    } else {
      brow[i] = kbase + 2 * r;                          // even conv row of the pooled pair
      bptr[i] = p.B + (long long)(brow[i] >> 1) * p.ldb + ncol;
      bbptr[i] = p.bbits + (long long)(brow[i] >> 1) * p.ld_bbits + (ncol >> 5);
    }
    bt[i] = brow[i] % p.Tp;
  }
  const long long a_step = (long long)BK * p.lda;
  const long long b_step = (LOADER == LOAD_DIRECT) ? (long long)BK * p.ldb : (long long)(BK / 2) * p.ldb;
  const long long bb_step = (long long)(BK / 2) * p.ld_bbits;

  // loads the tiles of the NEXT not-yet-loaded step and advances the per-thread state
  auto load_tiles = [&](f32x4 (&ra)[4], f32x4 (&rb)[4], uint32_t (&rnib)[2], long long /*step*/) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (amok && arow[i] < a_lim) v = *reinterpret_cast<const f32x4*>(aptr[i]);
      ra[i] = v;
      aptr[i] += a_step;
      arow[i] += BK;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      uint32_t nib = 0;
      if (bnok && brow[i] < b_lim && bt[i] < p.Tvalid) {
        v = *reinterpret_cast<const f32x4*>(bptr[i]);
        if constexpr (LOADER == LOAD_UNPOOL) nib = *bbptr[i];
      }
      rb[i] = v;
      if constexpr (LOADER == LOAD_DIRECT) {
        if (do_cs) cs += v;
      }
      if constexpr (LOADER == LOAD_UNPOOL) {
        rnib[i] = nib;
        bbptr[i] += bb_step;
      }
      bptr[i] += b_step;
      brow[i] += BK;
      bt[i] += dstep;
      if (bt[i] >= p.Tp) bt[i] -= p.Tp;
    }
  };
  auto store_tiles = [&](const f32x4 (&ra)[4], const f32x4 (&rb)[4], const uint32_t (&rnib)[2], int buf) {
    float* da = As + buf * BK * TN_LD;
    float* db = Bs + buf * BK * TN_LD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256;
      const int r = idx >> 5, c4 = idx & 31;
      *reinterpret_cast<f32x4*>(da + r * TN_LD + c4 * 4) = ra[i];
    }
    if constexpr (LOADER == LOAD_DIRECT) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = tid + i * 256;
        const int r = idx >> 5, c4 = idx & 31;
        *reinterpret_cast<f32x4*>(db + r * TN_LD + c4 * 4) = rb[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int idx = tid + i * 256;
        const int pr = idx >> 5, c4 = idx & 31;
        f32x4 e, o;
        const uint32_t nibv = rnib[i] >> (ncol & 31);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool odd = (nibv >> q) & 1u;
          e[q] = odd ? 0.f : rb[i][q];
          o[q] = odd ? rb[i][q] : 0.f;
        }
        *reinterpret_cast<f32x4*>(db + (2 * pr) * TN_LD + c4 * 4) = e;
        *reinterpret_cast<f32x4*>(db + (2 * pr + 1) * TN_LD + c4 * 4) = o;
      }
    }
  };

  // same software pipeline as the NT kernel: k-groups of 8 rows (4 MFMA k-steps), fragment
  // sets F0/F1, the last group carried across the barrier, LDS stores issued mid-step
  float ta0[4][2], tb0[4][2], ta1[4][2], tb1[4][2];
  auto load_frag = [&](float (&fa)[4][2], float (&fb)[4][2], int buf, int g) {
    const float* a_s = As + buf * BK * TN_LD + (g * 8 + lh) * TN_LD + wm * 64 + lr;
    const float* b_s = Bs + buf * BK * TN_LD + (g * 8 + lh) * TN_LD + wn * 64 + lr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      fa[q][0] = a_s[q * 2 * TN_LD];
      fa[q][1] = a_s[q * 2 * TN_LD + 32];
      fb[q][0] = b_s[q * 2 * TN_LD];
      fb[q][1] = b_s[q * 2 * TN_LD + 32];
    }
  };
  auto mfma_group = [&](const float (&fa)[4][2], const float (&fb)[4][2]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][mi], fb[q][ni], acc[mi][ni], 0, 0, 0);
  };

  auto kstep = [&](long long s, f32x4 (&ra_ld)[4], f32x4 (&rb_ld)[4], uint32_t (&rn_ld)[2], const f32x4 (&ra_st)[4],
                   const f32x4 (&rb_st)[4], const uint32_t (&rn_st)[2]) {
    const int buf = (int)(s & 1);
    load_frag(ta0, tb0, buf, 0);
    if (s + 2 < nsteps) load_tiles(ra_ld, rb_ld, rn_ld, s + 2);
    if (s > 0) mfma_group(ta1, tb1);
    load_frag(ta1, tb1, buf, 1);
    mfma_group(ta0, tb0);
    load_frag(ta0, tb0, buf, 2);
    mfma_group(ta1, tb1);
    if (s + 1 < nsteps) store_tiles(ra_st, rb_st, rn_st, buf ^ 1);
    load_frag(ta1, tb1, buf, 3);
    mfma_group(ta0, tb0);
    __syncthreads();
  };

  if (nsteps > 0) {
    load_tiles(raP, rbP, rnP, 0);
    store_tiles(raP, rbP, rnP, 0);
    if (nsteps > 1) load_tiles(raQ, rbQ, rnQ, 1);
  }
  __syncthreads();
  long long s = 0;
  for (; s + 1 < nsteps; s += 2) {
    kstep(s, raP, rbP, rnP, raQ, rbQ, rnQ);
    kstep(s + 1, raQ, rbQ, rnQ, raP, rbP, rnP);
  }
  if (s < nsteps) kstep(s, raP, rbP, rnP, raQ, rbQ, rnQ);
  if (nsteps > 0) mfma_group(ta1, tb1);

  if (do_cs) {                                            // (workgroup-uniform; every LDS read of the loop is behind its last barrier)
    float* red = lds;                                     // [8 row groups][128 columns]
    *reinterpret_cast<f32x4*>(red + (tid >> 5) * 128 + (tid & 31) * 4) = cs;
    __syncthreads();
    if (tid < 128 && n0 + tid < p.Ndim) {
      float t = 0.f;
#pragma unroll
      for (int g = 0; g < 8; ++g) t += red[g * 128 + tid];
      p.colsum[(long long)z * p.Ndim + n0 + tid] = t;
    }
  }

  float* out = p.slab + (long long)z * p.slab_stride;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int col = n0 + wn * 64 + ni * 32 + lr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m < p.Mdim && col < p.Ndim)
          out[((long long)j * p.Mdim + m) * (long long)p.ldc + col] = acc[mi][ni][e];
      }
    }
}


// ------------------------------------------------------------------------------------------
// TN, all three taps per workgroup (the conv weight gradient): one staged activation tile
// (BK + 2 rows) and one staged dZ tile feed the accumulators of all 3 taps, so the staging work
// per MFMA is half that of the one-tap kernel.  Block tile 128 (C_in) x 64 (C_out), wave tile
// 64 x 32 x 3 taps = 96 accumulator registers, still 2 workgroups per CU.
// ------------------------------------------------------------------------------------------
constexpr int T3_BN = 64, T3_LDA = 128 + 4, T3_LDB = T3_BN + 4, T3_AR = BK + 2;

template <int LOADER>
__global__ __launch_bounds__(256, 2) void tn3_kernel(const tl_tn_params p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * T3_AR * T3_LDA + 2 * BK * T3_LDB];
  float* As = lds;
  float* Bs = lds + 2 * T3_AR * T3_LDA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
  const int ntm = (p.Mdim + 127) / 128, ntn = (p.Ndim + T3_BN - 1) / T3_BN;
  const long long tiles = (long long)ntm * ntn;
  const long long nwg = tiles * p.splitk;
  long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  {
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const int z = (int)(bid / tiles);
  const int tt = (int)(bid % tiles);
  const int m0 = (tt / ntn) * 128, n0 = (tt % ntn) * T3_BN;

  const long long ksteps_all = (p.Krows + BK - 1) / BK;
  const long long per = (ksteps_all + p.splitk - 1) / p.splitk;
  const long long ks_begin = z * per;
  long long ks_end = ks_begin + per;
  if (ks_end > ksteps_all) ks_end = ksteps_all;
  const long long nsteps = ks_end > ks_begin ? ks_end - ks_begin : 0;

  f32x16 acc[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  constexpr int NB = (LOADER == LOAD_DIRECT) ? 2 : 1;
  f32x4 raP[5], raQ[5], rbP[NB], rbQ[NB];
  uint32_t rnP[NB], rnQ[NB];
  (void)rnP; (void)rnQ;

  const int a_lim = (int)(p.A_rows < p.Krows + 2 ? p.A_rows : p.Krows + 2);
  const int b_lim = (LOADER == LOAD_DIRECT) ? (int)(p.B_rows < p.Krows ? p.B_rows : p.Krows)
                                            : (int)(2 * p.B_rows < p.Krows ? 2 * p.B_rows : p.Krows);
  const int kbase = (int)(ks_begin * BK);
  const float* aptr[5];
  int arow[5];
  bool aact[5];
  const bool amok = (m0 + (tid & 31) * 4) < p.Mdim;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int r = (tid + i * 256) >> 5;           // 0..39, rows >= 34 unused
    aact[i] = r < T3_AR;
    arow[i] = kbase + r;
    aptr[i] = p.A + (long long)arow[i] * p.lda + m0 + (tid & 31) * 4;
  }
  const float* bptr[NB];
  const uint32_t* bbptr[NB];
  int brow[NB], bt[NB];
  (void)bbptr;
  const int ncol = n0 + (tid & 15) * 4;
  const bool bnok = ncol < p.Ndim;
  const int dstep = BK % p.Tp;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int r = (tid + i * 256) >> 4;           // 16 float4 per 64-column row
    if constexpr (LOADER == LOAD_DIRECT) {
      brow[i] = kbase + r;
      bptr[i] = p.B + (long long)brow[i] * p.ldb + ncol;
      bbptr[i] = nullptr;
    } else {
      brow[i] = kbase + 2 * r;
      bptr[i] = p.B + (long long)(brow[i] >> 1) * p.ldb + ncol;
      bbptr[i] = p.bbits + (long long)(brow[i] >> 1) * p.ld_bbits + (ncol >> 5);
    }
    bt[i] = brow[i] % p.Tp;
  }
  const long long a_step = (long long)BK * p.lda;
  const long long b_step = (LOADER == LOAD_DIRECT) ? (long long)BK * p.ldb : (long long)(BK / 2) * p.ldb;
  const long long bb_step = (long long)(BK / 2) * p.ld_bbits;

  auto load_tiles = [&](f32x4 (&ra)[5], f32x4 (&rb)[NB], uint32_t (&rn)[NB]) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (aact[i] && amok && arow[i] < a_lim) v = *reinterpret_cast<const f32x4*>(aptr[i]);
      ra[i] = v;
      aptr[i] += a_step;
      arow[i] += BK;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      uint32_t nib = 0;
      if (bnok && brow[i] < b_lim && bt[i] < p.Tvalid) {
        v = *reinterpret_cast<const f32x4*>(bptr[i]);
        if constexpr (LOADER == LOAD_UNPOOL) nib = *bbptr[i];
      }
      rb[i] = v;
      if constexpr (LOADER == LOAD_UNPOOL) {
        rn[i] = nib;
        bbptr[i] += bb_step;
      }
      bptr[i] += b_step;
      brow[i] += BK;
      bt[i] += dstep;
      if (bt[i] >= p.Tp) bt[i] -= p.Tp;
    }
  };
  auto store_tiles = [&](const f32x4 (&ra)[5], const f32x4 (&rb)[NB], const uint32_t (&rn)[NB], int buf) {
    float* da = As + buf * T3_AR * T3_LDA;
    float* db = Bs + buf * BK * T3_LDB;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int idx = tid + i * 256;
      const int r = idx >> 5, c4 = idx & 31;
      if (r < T3_AR) *reinterpret_cast<f32x4*>(da + r * T3_LDA + c4 * 4) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + i * 256;
      const int r = idx >> 4, c4 = idx & 15;
      if constexpr (LOADER == LOAD_DIRECT) {
        *reinterpret_cast<f32x4*>(db + r * T3_LDB + c4 * 4) = rb[i];
      } else {
        f32x4 e, o;
        const uint32_t nibv = rn[i] >> (ncol & 31);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool odd = (nibv >> q) & 1u;
          e[q] = odd ? 0.f : rb[i][q];
          o[q] = odd ? rb[i][q] : 0.f;
        }
        *reinterpret_cast<f32x4*>(db + (2 * r) * T3_LDB + c4 * 4) = e;
        *reinterpret_cast<f32x4*>(db + (2 * r + 1) * T3_LDB + c4 * 4) = o;
      }
    }
  };

  // fragments of one k-group (8 rows = 4 MFMA k-steps): A needs rows lh .. lh+8 (taps 0..2)
  float fa0[10][2], fb0[4], fa1[10][2], fb1[4];
  auto load_frag = [&](float (&fa)[10][2], float (&fb)[4], int buf, int g) {
    const float* a_s = As + buf * T3_AR * T3_LDA + (g * 8 + lh) * T3_LDA + wm * 64 + lr;
    const float* b_s = Bs + buf * BK * T3_LDB + (g * 8 + lh) * T3_LDB + wn * 32 + lr;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      fa[r][0] = a_s[r * T3_LDA];
      fa[r][1] = a_s[r * T3_LDA + 32];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) fb[q] = b_s[q * 2 * T3_LDB];
  };
  auto mfma_group = [&](const float (&fa)[10][2], const float (&fb)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[j][mi] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[2 * q + j][mi], fb[q], acc[j][mi], 0, 0, 0);
  };
  auto kstep = [&](long long s, f32x4 (&ra_ld)[5], f32x4 (&rb_ld)[NB], uint32_t (&rn_ld)[NB], const f32x4 (&ra_st)[5],
                   const f32x4 (&rb_st)[NB], const uint32_t (&rn_st)[NB]) {
    const int buf = (int)(s & 1);
    load_frag(fa0, fb0, buf, 0);
    if (s + 2 < nsteps) load_tiles(ra_ld, rb_ld, rn_ld);
    if (s > 0) mfma_group(fa1, fb1);
    load_frag(fa1, fb1, buf, 1);
    mfma_group(fa0, fb0);
    load_frag(fa0, fb0, buf, 2);
    mfma_group(fa1, fb1);
    if (s + 1 < nsteps) store_tiles(ra_st, rb_st, rn_st, buf ^ 1);
    load_frag(fa1, fb1, buf, 3);
    mfma_group(fa0, fb0);
    __syncthreads();
  };

  if (nsteps > 0) {
    load_tiles(raP, rbP, rnP);
    store_tiles(raP, rbP, rnP, 0);
    if (nsteps > 1) load_tiles(raQ, rbQ, rnQ);
  }
  __syncthreads();
  long long s = 0;
  for (; s + 1 < nsteps; s += 2) {
    kstep(s, raP, rbP, rnP, raQ, rbQ, rnQ);
    kstep(s + 1, raQ, rbQ, rnQ, raP, rbP, rnP);
  }
  if (s < nsteps) kstep(s, raP, rbP, rnP, raQ, rbQ, rnQ);
  if (nsteps > 0) mfma_group(fa1, fb1);

  float* out = p.slab + (long long)z * p.slab_stride;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int col = n0 + wn * 32 + lr;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m < p.Mdim && col < p.Ndim) out[((long long)j * p.Mdim + m) * (long long)p.ldc + col] = acc[j][mi][e];
      }
    }
}

// ------------------------------------------------------------------------------------------
// TN, skinny M (<= 32 rows of output): slab[z][m][n] = sum_k A[k][m] * B[k][n].  Used for
// dh = dgates . W_hh on the few distinct label rows: B (5.4 GB) is streamed exactly once, so the
// tile is 32 x 512 with a 16-deep K stage (33 KB in flight per workgroup, 2 workgroups per CU) and
// the kernel is HBM-bound, not MFMA-bound.
// ------------------------------------------------------------------------------------------
constexpr int SK_BK = 16, SK_BN = 512, SK_LDB = SK_BN + 4, SK_LDA = 32 + 4;

__global__ __launch_bounds__(256, 2) void tn_skinny_kernel(const tl_tn_params p) {
  __shared__ __attribute__((aligned(16))) float lds[2 * SK_BK * SK_LDA + 2 * SK_BK * SK_LDB];
  float* As = lds;
  float* Bs = lds + 2 * SK_BK * SK_LDA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.x * SK_BN;
  const int z = blockIdx.y;
  const long long ksteps_all = (p.Krows + SK_BK - 1) / SK_BK;
  const long long per = (ksteps_all + p.splitk - 1) / p.splitk;
  const long long ks_begin = z * per;
  long long ks_end = ks_begin + per;
  if (ks_end > ksteps_all) ks_end = ksteps_all;
  const long long nsteps = ks_end > ks_begin ? ks_end - ks_begin : 0;

  f32x16 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
  f32x4 rb[8], ra;
  const bool mask_rows = p.Tp > 1;

  auto load_tiles = [&](long long step) {
    const long long k0 = (ks_begin + step) * SK_BK;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + i * 256;
      const int r = idx >> 7, c4 = idx & 127;
      const long long row = k0 + r;
      const int n = n0 + c4 * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      bool ok = row < p.Krows && row < p.B_rows && n < p.Ndim;
      if (mask_rows) ok = ok && (int)(row % p.Tp) < p.Tvalid;
      if (ok) v = *reinterpret_cast<const f32x4*>(p.B + row * (long long)p.ldb + n);
      rb[i] = v;
    }
    {
      const int r = (tid >> 3) & 15, c4 = tid & 7;
      const long long row = k0 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (tid < 128 && row < p.Krows && row < p.A_rows && c4 * 4 < p.Mdim)
        v = *reinterpret_cast<const f32x4*>(p.A + row * (long long)p.lda + c4 * 4);
      ra = v;
    }
  };
  auto store_tiles = [&](int buf) {
    float* db = Bs + buf * SK_BK * SK_LDB;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + i * 256;
      const int r = idx >> 7, c4 = idx & 127;
      *reinterpret_cast<f32x4*>(db + r * SK_LDB + c4 * 4) = rb[i];
    }
    if (tid < 128) {
      const int r = tid >> 3, c4 = tid & 7;
      *reinterpret_cast<f32x4*>(As + buf * SK_BK * SK_LDA + r * SK_LDA + c4 * 4) = ra;
    }
  };

  if (nsteps > 0) {
    load_tiles(0);
    store_tiles(0);
  }
  __syncthreads();
  for (long long s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    if (more) load_tiles(s + 1);
    const float* a_s = As + (s & 1) * SK_BK * SK_LDA + lh * SK_LDA + lr;
    const float* b_s = Bs + (s & 1) * SK_BK * SK_LDB + lh * SK_LDB + wave * 128 + lr;
#pragma unroll
    for (int kk = 0; kk < SK_BK / 2; ++kk) {
      const float fa = a_s[kk * 2 * SK_LDA];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, b_s[kk * 2 * SK_LDB + ni * 32], acc[ni], 0, 0, 0);
    }
    if (more) store_tiles((s + 1) & 1);
    __syncthreads();
  }
  float* out = p.slab + (long long)z * p.slab_stride;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int col = n0 + wave * 128 + ni * 32 + lr;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = (e & 3) + 8 * (e >> 2) + 4 * lh;
      if (m < p.Mdim && col < p.Ndim) out[(long long)m * p.ldc + col] = acc[ni][e];
    }
  }
}

}  // namespace tl

// the argument checks of tl_gemm_nt_window (shared with tl_gemm_nt_window_group); fills in the defaults of splitk and bm
static int nt_check(tl_nt_params& p) {
  using namespace tl;
  if (p.splitk < 1) p.splitk = 1;
  if (p.bm == 0) p.bm = 128;
  TL_REQUIRE(p.A && p.Bw && p.out, "nt_window: null A/Bw/out");
  TL_REQUIRE(p.M >= 0 && p.N > 0 && p.K > 0, "nt_window: bad M/N/K %lld/%d/%d", (long long)p.M, p.N, p.K);
  TL_REQUIRE(p.K % 4 == 0 && p.lda % 4 == 0 && p.ldb % 4 == 0, "nt_window: K, lda, ldb must be multiples of 4");
  TL_REQUIRE(p.lda >= p.K && p.ldb >= p.K, "nt_window: lda/ldb smaller than K");
  TL_REQUIRE(p.J >= 1 && p.J <= 7, "nt_window: J must be 1..7");
  TL_REQUIRE(p.row_shift == 0 || p.row_shift == -(p.J - 1), "nt_window: row_shift must be 0 or -(J-1)");
  TL_REQUIRE(p.bm == 256 || p.bm == 128 || p.bm == 32, "nt_window: bm must be 256, 128 or 32");
  TL_REQUIRE(p.Tp > 0, "nt_window: Tp must be positive");
  TL_REQUIRE(p.splitk == 1 || p.epilogue == EPI_STORE, "nt_window: split-K needs the STORE epilogue");
  TL_REQUIRE(p.splitk <= 65535, "nt_window: splitk too large");
  if (p.loader == LOAD_UNPOOL) {
    TL_REQUIRE(p.abits != nullptr, "nt_window: UNPOOL loader needs abits");
    TL_REQUIRE((p.row_shift % 2) == 0 && p.Tp % 2 == 0 && p.Tvalid_in % 2 == 0, "nt_window: UNPOOL needs even shift/Tp/Tvalid_in");
    TL_REQUIRE(p.K % 32 == 0 || p.ld_abits * 32 >= p.K, "nt_window: abits row too short");
    TL_REQUIRE(p.bm != 32, "nt_window: UNPOOL loader needs bm = 128 or 256");
  }
  if (p.epilogue == EPI_POOL) {
    TL_REQUIRE(p.obits != nullptr, "nt_window: POOL epilogue needs obits");
    TL_REQUIRE(p.Tp % 2 == 0 && p.Tvalid % 2 == 0, "nt_window: POOL needs even Tp/Tvalid");
    TL_REQUIRE(p.N % 32 == 0 && p.ld_obits * 32 >= p.N, "nt_window: POOL needs N %% 32 == 0");
  }
  if (p.epilogue == EPI_MASK) TL_REQUIRE(p.aux != nullptr || p.auxbits != nullptr, "nt_window: MASK epilogue needs aux or auxbits");
  return TL_OK;
}

// TONAL_GLDS=0 under TONAL_AB=1 selects the register-staged kernel (see tl_gemm_nt_window)
static bool nt_glds_on() {
  const char* ab = getenv("TONAL_AB");
  const char* genv = (ab != nullptr && ab[0] == '1') ? getenv("TONAL_GLDS") : nullptr;
  return genv == nullptr || genv[0] != '0';
}

// does tl_gemm_nt_window run these (checked) parameters on the direct-to-LDS kernel?
// (its DMA cannot zero-fill: a row from A_rows on is read as row A_rows - 1, which is harmless only where no output row's tap
// window reaches that far - one tap, or J - 1 rows behind row M - 1.  With fewer rows behind the end, rows M - J + 1 .. M - 1
// would take the last row's values where the contract says zero: the register-staged kernel runs those.)
static bool nt_takes_glds(const tl_nt_params& p) {
  return nt_glds_on() && p.J <= 3 && p.bm == 128 && p.loader == tl::LOAD_DIRECT && p.row_shift == 0 && (p.K % tl::GK) == 0 &&
         p.A_rows > 0 && (p.J == 1 || p.A_rows >= p.M + p.J - 1);
}

extern "C" int tl_gemm_nt_window(const tl_nt_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "nt_window: null params");
  tl_nt_params p = *pp;
  if (const int rc = nt_check(p)) return rc;
  hipStream_t st = (hipStream_t)stream;
  // Direct-to-LDS staging variant.  Round 1 measured it equal to the register-staged kernel on the conv2 forward (129.6 vs
  // 128.6 TFLOP/s) and kept the simpler one; on what is left for this entry point since the Winograd kernels took the 3-tap
  // stages - conv4 / conv5 forward, the 1x1 stack, the Linear layer - it is the faster one (train step 209.7 -> 208.9 ms,
  // same-call A/B, round 4): default on; TONAL_GLDS=0 selects the register-staged kernel (the A/B partner,
  // tests/test_gpu_parity.py holds the two against each other).
  // (an A/B switch of the test suite: honoured only under TONAL_AB=1, like the per-switch variables of _kernels.py)
  if (nt_takes_glds(p)) {
    switch (p.epilogue) {
      case EPI_STORE: return launch_glds<EPI_STORE>(p, st);
      case EPI_LRELU: return launch_glds<EPI_LRELU>(p, st);
      case EPI_POOL: return launch_glds<EPI_POOL>(p, st);
      case EPI_MASK: return launch_glds<EPI_MASK>(p, st);
    }
  }
  if (p.bm == 256) return dispatch_nt<256>(p, st);
  return p.bm == 128 ? dispatch_nt<128>(p, st) : dispatch_nt<32>(p, st);
}

// tl_gemm_nt_window for M members of equal shape - what the hidden layer of the shallow-classifier ensemble launches: a plain
// GEMM (J = 1, DIRECT, no split-K, 128-row tiles) with bias and LeakyReLU in the epilogue.  The kernel is chosen exactly as
// tl_gemm_nt_window chooses it for *pp, and its body is that kernel's: a member's bits are the single launch's.
extern "C" int tl_gemm_nt_window_group(const tl_nt_params* pp, int M, int64_t s_A, int64_t s_Bw, int64_t s_bias, int64_t s_out,
                                       const int32_t* active, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "nt_window_group: null params");
  tl_nt_params p = *pp;
  TL_REQUIRE_MEMBERS("nt_window_group", M);
  TL_REQUIRE(p.J == 1 && p.loader == LOAD_DIRECT && p.row_shift == 0,
             "nt_window_group: only the plain GEMM has a group form (J = 1, DIRECT loader, row_shift = 0; got J %d, loader %d, "
             "row_shift %d)", p.J, p.loader, p.row_shift);
  TL_REQUIRE(p.splitk <= 1, "nt_window_group: no split-K (got splitk %d)", p.splitk);
  TL_REQUIRE(p.bm == 0 || p.bm == 128, "nt_window_group: bm must be 0 or 128 (got %d)", p.bm);
  TL_REQUIRE(p.epilogue == EPI_LRELU, "nt_window_group: only the LRELU epilogue has a group form (ReLU is slope 0; got %d)", p.epilogue);
  TL_REQUIRE(p.bias != nullptr, "nt_window_group: null bias");
  TL_REQUIRE(!p.aux && !p.auxbits && !p.abits && !p.obits && !p.osign && !p.vout && !p.vout2 && !p.vhalo && !p.c1x && !p.c1bits &&
                 !p.c1partial && !p.mask,
             "nt_window_group: aux / auxbits / abits / obits / osign / vout / c1 / mask pointers have no member stride: pass null");
  if (const int rc = nt_check(p)) return rc;
  TL_REQUIRE(s_A >= 0 && s_Bw >= 0 && s_bias >= 0 && s_A % 4 == 0 && s_Bw % 4 == 0,
             "nt_window_group: the member strides of A and Bw must be non-negative multiples of 4 elements (16-byte aligned "
             "members), that of bias non-negative");
  TL_REQUIRE(M == 1 || s_out >= p.M * (int64_t)p.ldo,
             "nt_window_group: member stride of out shorter than the M x ldo elements of a member");
  hipStream_t st = (hipStream_t)stream;
  const nt_group g = {(long long)s_A, (long long)s_Bw, (long long)s_bias, (long long)s_out, active, 0};
  const bool glds = nt_takes_glds(p), narrow = glds && p.N <= 64;
  const int bn = narrow ? 64 : BN;
  const long long nwg = ((p.M + 127) / 128) * ((p.N + bn - 1) / bn);
  if (nwg <= 0) return TL_OK;
  TL_REQUIRE(nwg < (1LL << 31), "nt_window_group: grid too large");
  const dim3 grid((unsigned)nwg, 1, (unsigned)M);
  if (narrow)
    hipLaunchKernelGGL((nt_glds_group_kernel<EPI_LRELU, 1>), grid, dim3(256), 0, st, p, g);
  else if (glds)
    hipLaunchKernelGGL((nt_glds_group_kernel<EPI_LRELU, 2>), grid, dim3(256), 0, st, p, g);
  else
    hipLaunchKernelGGL((nt_window_group_kernel<128, LOAD_DIRECT, EPI_LRELU>), grid, dim3(nt_cfg<128>::NTHR), 0, st, p, g);
  return check_launch("nt_window_group");
}

// The group form of the two Linear layers of SynthesisLite and of their input gradients (_lite_ensemble_engine.py): the plain
// GEMM (J = 1, DIRECT, row_shift 0) on 32- or 128-row tiles, epilogue STORE - split-K on grid.y as in the single launch, every
// member with splitk slabs of its own - or MASK with aux at a member stride.  The kernel is chosen as tl_gemm_nt_window chooses
// it for *pp, its body is that kernel's, the member sits on grid.z.
template <int EPI>
static int launch_nt_group_fc(const tl_nt_params& p, const tl::nt_group& g, int M, hipStream_t st) {
  using namespace tl;
  const bool glds = nt_takes_glds(p), narrow = glds && p.N <= 64;
  const int bn = narrow ? 64 : BN, bm = glds ? 128 : p.bm;
  const long long nwg = ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn);
  if (nwg <= 0) return TL_OK;
  TL_REQUIRE(nwg < (1LL << 31), "nt_window_group_fc: grid too large");
  const dim3 grid((unsigned)nwg, (unsigned)p.splitk, (unsigned)M);
  if (narrow)
    hipLaunchKernelGGL((nt_glds_group_kernel<EPI, 1>), grid, dim3(256), 0, st, p, g);
  else if (glds)
    hipLaunchKernelGGL((nt_glds_group_kernel<EPI, 2>), grid, dim3(256), 0, st, p, g);
  else if (p.bm == 128)
    hipLaunchKernelGGL((nt_window_group_kernel<128, LOAD_DIRECT, EPI>), grid, dim3(nt_cfg<128>::NTHR), 0, st, p, g);
  else
    hipLaunchKernelGGL((nt_window_group_kernel<32, LOAD_DIRECT, EPI>), grid, dim3(nt_cfg<32>::NTHR), 0, st, p, g);
  return check_launch("nt_window_group_fc");
}

extern "C" int tl_gemm_nt_window_group_fc(const tl_nt_params* pp, int M, int64_t s_A, int64_t s_Bw, int64_t s_bias, int64_t s_aux,
                                          int64_t s_out, const int32_t* active, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "nt_window_group_fc: null params");
  tl_nt_params p = *pp;
  TL_REQUIRE_MEMBERS("nt_window_group_fc", M);
  TL_REQUIRE(p.J == 1 && p.loader == LOAD_DIRECT && p.row_shift == 0,
             "nt_window_group_fc: only the plain GEMM has a group form (J = 1, DIRECT loader, row_shift = 0; got J %d, loader %d, "
             "row_shift %d)", p.J, p.loader, p.row_shift);
  TL_REQUIRE(p.bm == 32 || p.bm == 128, "nt_window_group_fc: bm must be 32 or 128 (got %d)", p.bm);
  TL_REQUIRE(p.epilogue == EPI_STORE || p.epilogue == EPI_MASK,
             "nt_window_group_fc: only the STORE and MASK epilogues have this group form (got %d)", p.epilogue);
  TL_REQUIRE(!p.auxbits && !p.abits && !p.obits && !p.osign && !p.vout && !p.vout2 && !p.vhalo && !p.c1x && !p.c1bits &&
                 !p.c1partial && !p.mask && (p.epilogue == EPI_MASK || !p.aux),
             "nt_window_group_fc: auxbits / abits / obits / osign / vout / c1 / mask pointers (and aux without the MASK epilogue) "
             "have no member stride: pass null");
  TL_REQUIRE(p.epilogue != EPI_MASK || p.aux != nullptr, "nt_window_group_fc: the MASK epilogue needs aux");
  if (const int rc = nt_check(p)) return rc;
  TL_REQUIRE(s_A >= 0 && s_Bw >= 0 && s_bias >= 0 && s_aux >= 0 && s_A % 4 == 0 && s_Bw % 4 == 0,
             "nt_window_group_fc: the member strides of A and Bw must be non-negative multiples of 4 elements (16-byte aligned "
             "members), those of bias and aux non-negative");
  TL_REQUIRE(p.splitk == 1 || p.slab_stride >= p.M * (int64_t)p.ldo,
             "nt_window_group_fc: slab_stride shorter than the M x ldo elements of a slab");
  TL_REQUIRE(M == 1 || s_out >= (p.splitk > 1 ? (int64_t)p.splitk * p.slab_stride : p.M * (int64_t)p.ldo),
             "nt_window_group_fc: member stride of out shorter than a member's extent (M x ldo elements, or splitk x slab_stride)");
  const nt_group g = {(long long)s_A, (long long)s_Bw, (long long)s_bias, (long long)s_out, active, (long long)s_aux};
  hipStream_t st = (hipStream_t)stream;
  return p.epilogue == EPI_STORE ? launch_nt_group_fc<EPI_STORE>(p, g, M, st) : launch_nt_group_fc<EPI_MASK>(p, g, M, st);
}

namespace tl {
// Short reductions (a few hundred rows: the weight gradients of SynthesisLite's Linear / LSTM layers at batch 64): the MFMA
// kernels' 128 x 128 tiles leave a handful of workgroups with a short K loop of dependent latency (17 - 30 us).  Here a
// workgroup takes a 32 x 128 tile and walks the rows in chunks of 64: one round of loads per chunk (issued before the
// arithmetic of the chunk in front of it, 40 KB of LDS), plain FMAs on a 4 x 4 patch per thread, rows in order
// (deterministic); masked rows ((R % Tp) >= Tvalid) are zero-filled, not read.
constexpr int TS_K = 64, TS_M = 32, TS_N = 128;
// (the body is a file of statements included into the single and the group kernel, as with the NT kernels above)
__global__ __launch_bounds__(256) void tn_short_kernel(const tl_tn_params p) {
#include "tonal_gemm_tn_short_body.h"
}
struct tn_group {
  long long s_A, s_B, s_slab, s_colsum;   // member strides, elements
  const int32_t* active;                  // M words or null; 0: the member's workgroups return at once
};
__global__ __launch_bounds__(256) void tn_short_group_kernel(tl_tn_params p, const tn_group g) {
  const int mem = blockIdx.z;
  if (g.active != nullptr && g.active[mem] == 0) return;        // uniform over the workgroup, before any load or barrier
  p.A += mem * g.s_A;
  p.B += mem * g.s_B;
  p.slab += mem * g.s_slab;
  if (p.colsum != nullptr) p.colsum += mem * g.s_colsum;
#include "tonal_gemm_tn_short_body.h"
}
}  // namespace tl

// the shared argument checks of tl_gemm_tn_window and tl_gemm_tn_window_group; fills in the default of splitk
static int tn_check(tl_tn_params& p, const char* what) {
  using namespace tl;
  if (p.splitk < 1) p.splitk = 1;
  TL_REQUIRE(p.A && p.B && p.slab, "%s: null A/B/slab", what);
  TL_REQUIRE(p.Krows > 0 && p.Mdim > 0 && p.Ndim > 0, "%s: bad sizes", what);
  TL_REQUIRE(p.Krows + 64 < (1LL << 31), "%s: more than 2^31 reduction rows", what);
  TL_REQUIRE(p.Mdim % 4 == 0 && p.Ndim % 4 == 0 && p.lda % 4 == 0 && p.ldb % 4 == 0, "%s: dims/ld must be multiples of 4", what);
  TL_REQUIRE(p.J >= 1 && p.J <= 7, "%s: J must be 1..7", what);
  TL_REQUIRE(p.Tp > 0, "%s: Tp must be positive", what);
  TL_REQUIRE(p.splitk <= 65535, "%s: splitk too large", what);
  return TL_OK;
}
// does tl_gemm_tn_window run these (checked) parameters on the short-reduction kernel?
static bool tn_takes_short(const tl_tn_params& p) {
  return p.J == 1 && p.loader == tl::LOAD_DIRECT && p.Krows <= 8 * tl::TS_K && p.splitk <= 8 &&
         (long long)p.Mdim * p.Ndim <= (1 << 20) && (p.splitk == 1 || p.slab_stride >= (long long)p.Mdim * p.ldc) && p.ldc % 4 == 0;
}

// tl_gemm_tn_window for M members of equal shape, for the parameters the single entry sends to tn_short_kernel (the weight
// gradients of SynthesisLite's Linear / LSTM layers): that kernel's body with the member on grid.z.
extern "C" int tl_gemm_tn_window_group(const tl_tn_params* pp, int M, int64_t s_A, int64_t s_B, int64_t s_slab, int64_t s_colsum,
                                       const int32_t* active, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "tn_window_group: null params");
  tl_tn_params p = *pp;
  TL_REQUIRE_MEMBERS("tn_window_group", M);
  if (const int rc = tn_check(p, "tn_window_group")) return rc;
  TL_REQUIRE(tn_takes_short(p),
             "tn_window_group: only the short-reduction kernel has a group form (J = 1, DIRECT loader, Krows <= 512, splitk <= 8, "
             "Mdim * Ndim <= 2^20, ldc %% 4 == 0, slab_stride >= Mdim * ldc under split-K; got J %d, loader %d, Krows %lld, splitk %d, "
             "Mdim %d, Ndim %d, ldc %d)", p.J, p.loader, (long long)p.Krows, p.splitk, p.Mdim, p.Ndim, p.ldc);
  TL_REQUIRE(!p.bbits && !p.vd, "tn_window_group: bbits / vd have no member stride: pass null");
  TL_REQUIRE(p.lda >= p.Mdim && p.ldb >= p.Ndim && p.ldc >= p.Ndim, "tn_window_group: lda / ldb / ldc smaller than the row they stride");
  TL_REQUIRE(p.A_rows > 0 && p.B_rows > 0, "tn_window_group: A_rows and B_rows must be positive");
  TL_REQUIRE(s_A >= 0 && s_B >= 0 && s_A % 4 == 0 && s_B % 4 == 0 && s_slab % 4 == 0,
             "tn_window_group: the member strides of A, B and slab must be non-negative multiples of 4 elements (16-byte aligned members)");
  TL_REQUIRE(s_slab >= 0 && (M == 1 || s_slab >= (p.splitk > 1 ? (int64_t)p.splitk * p.slab_stride : (int64_t)p.Mdim * p.ldc)),
             "tn_window_group: member stride of slab shorter than a member's extent (Mdim x ldc elements, or splitk x slab_stride)");
  TL_REQUIRE(p.colsum == nullptr || (s_colsum >= 0 && (M == 1 || s_colsum >= p.Mdim)),
             "tn_window_group: member stride of colsum shorter than the Mdim elements of a member");
  const long long nwg = (long long)((p.Mdim + TS_M - 1) / TS_M) * ((p.Ndim + TS_N - 1) / TS_N);
  const tn_group g = {(long long)s_A, (long long)s_B, (long long)s_slab, (long long)s_colsum, active};
  hipLaunchKernelGGL(tn_short_group_kernel, dim3((unsigned)nwg, (unsigned)p.splitk, (unsigned)M), dim3(256), 0, (hipStream_t)stream,
                     p, g);
  return check_launch("tn_short_group");
}

extern "C" int tl_gemm_tn_window(const tl_tn_params* pp, void* stream) {
  using namespace tl;
  TL_REQUIRE(pp != nullptr, "tn_window: null params");
  tl_tn_params p = *pp;
  if (const int rc = tn_check(p, "tn_window")) return rc;
  if (p.loader == LOAD_UNPOOL) {
    TL_REQUIRE(p.bbits != nullptr, "tn_window: UNPOOL loader needs bbits");
    TL_REQUIRE(p.Tp % 2 == 0 && p.Tvalid % 2 == 0, "tn_window: UNPOOL needs even Tp/Tvalid");
    TL_REQUIRE(p.ld_bbits * 32 >= p.Ndim, "tn_window: bbits row too short");
  }
  hipStream_t st = (hipStream_t)stream;
  if (tn_takes_short(p)) {                                           // short reduction, small output: latency-bound
    const long long nwg = (long long)((p.Mdim + TS_M - 1) / TS_M) * ((p.Ndim + TS_N - 1) / TS_N);
    hipLaunchKernelGGL(tn_short_kernel, dim3((unsigned)nwg, (unsigned)p.splitk), dim3(256), 0, st, p);
    return check_launch("tn_short");
  }
  TL_REQUIRE(p.colsum == nullptr || (p.J == 1 && p.loader == LOAD_DIRECT && p.Mdim > 32),
             "tn_window: colsum comes from the short-reduction kernel (Krows <= 512, splitk <= 8, Mdim * Ndim <= 2^20) or the one-tap direct kernel (Mdim > 32)");
  if (p.Mdim <= 32 && p.J == 1 && p.loader == LOAD_DIRECT) {       // skinny-M streaming variant
    dim3 grid((unsigned)((p.Ndim + SK_BN - 1) / SK_BN), (unsigned)p.splitk, 1);
    hipLaunchKernelGGL(tn_skinny_kernel, grid, dim3(256), 0, st, p);
    return check_launch("tn_skinny");
  }
  if (p.J == 3) {                                                    // all taps per workgroup
    const long long t3 = (long long)((p.Mdim + 127) / 128) * ((p.Ndim + T3_BN - 1) / T3_BN);
    TL_REQUIRE(t3 < (1LL << 31), "tn_window: grid too large");
    dim3 grid((unsigned)t3, (unsigned)p.splitk, 1);
    if (p.loader == LOAD_DIRECT)
      hipLaunchKernelGGL((tn3_kernel<LOAD_DIRECT>), grid, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((tn3_kernel<LOAD_UNPOOL>), grid, dim3(256), 0, st, p);
    return check_launch("tn3");
  }
  const long long ntm = (p.Mdim + 127) / 128, ntn = (p.Ndim + 127) / 128;
  const long long nwg = ntm * ntn * p.J;
  TL_REQUIRE(nwg < (1LL << 31), "tn_window: grid too large");
  dim3 grid((unsigned)nwg, (unsigned)p.splitk, 1);
  if (p.loader == LOAD_DIRECT)
    hipLaunchKernelGGL((tn_window_kernel<LOAD_DIRECT>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((tn_window_kernel<LOAD_UNPOOL>), grid, dim3(256), 0, st, p);
  return check_launch("tn_window");
}

extern "C" int tl_sizeof_nt_params(void) { return (int)sizeof(tl_nt_params); }
extern "C" int tl_sizeof_tn_params(void) { return (int)sizeof(tl_tn_params); }
