// Shared by the V-form NT kernels (tonal_wino43v.hip, tonal_wino63.hip) and their epilogues (tonal_wino43v_epi.h,
// tonal_wino63_epi.h): the loader / epilogue numbering of tl_nt_params and the accumulator + block reduction of the fused
// first-stage weight gradient.  Reference arithmetic: models/synthesis_models.py:87-97 and their backward.
#pragma once
#include "tonal_common.h"

namespace tl {

enum { W_LOAD_DIRECT = 0, W_LOAD_UNPOOL = 1, W_LOAD_V = 2 };
enum { W_EPI_LRELU = 1, W_EPI_POOL = 2, W_EPI_MASK = 3, W_EPI_C1W = 4, W_EPI_POOLV = 5, W_EPI_MASKY = 6, W_EPI_GY = 7 };   // numbering of tl_nt_params.epilogue

// ------------------------------------------------------------------------------------------
// Fused first-stage weight gradient (epilogue 4).  The input gradient of conv2 is G1 = dL/dZ of conv1
// at its arg-max; conv1 has one input channel, so its weight gradient is a contraction of G1 with the
// raw signal: dW1[o][j] = sum_rows G1[row][o] * x[seq][2t + a + j].  Doing it on the accumulators
// removes the 13.4 GB store of G1 and the kernel that re-read it.
// ------------------------------------------------------------------------------------------
struct c1w_acc {
  float s[3], b;
  __device__ __forceinline__ void clear() { s[0] = s[1] = s[2] = b = 0.f; }
};
// block reduction over the row dimension: lanes lr / lr + 32 and the NWM waves that share a column;
// red: LDS [NWM][NCOL][5].  Writes c1partial[tile][j][col] for the block's NCOL columns.
template <int NWM, int NCOL>
__device__ __forceinline__ void c1w_reduce_store(const tl_nt_params& p, float* red, const c1w_acc& a, int wm, int cl,
                                                 int lh, long long tile, int col, bool colok) {
  float v[4] = {a.s[0], a.s[1], a.s[2], a.b};
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] += __shfl_xor(v[j], 32);
  if (lh == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) red[(wm * NCOL + cl) * 4 + j] = v[j];
  }
  __syncthreads();
  if (wm == 0 && lh == 0 && colok) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NWM; ++w) t += red[(w * NCOL + cl) * 4 + j];
      v[j] = t;
    }
    float* dst = p.c1partial + tile * (long long)(p.c1kt + 1) * p.N;
    for (int j = 0; j < p.c1kt; ++j) dst[(long long)j * p.N + col] = v[j];
    dst[(long long)p.c1kt * p.N + col] = v[3];
  }
  __syncthreads();
}

}  // namespace tl
