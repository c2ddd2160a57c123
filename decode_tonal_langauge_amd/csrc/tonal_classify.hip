// Classifier training (models/classifier_trainer.py:72-89: nn.CrossEntropyLoss, loss.backward() and the per-batch confusion
// matrix of the reference loop): the softmax-cross-entropy step with its statistics kept on the device, and the backward of a
// head layer with a handful of outputs.  See include/tonal_hip.h for the contracts.
#include "tonal_common.h"
#include <math.h>

namespace tl {

// ------------------------------------------------------------------------------------------
// softmax cross-entropy.  One wave per row, lane n owns logit n (N <= 64: a row is one coalesced load and one coalesced
// store); ONE workgroup of 16 waves walks the rows, wave w takes rows w, w + 16, ..  The floating-point sums therefore have a
// fixed order - a wave adds its rows in row order, the 16 partial sums meet in wave order - and the same inputs give the same
// bits.  The row arithmetic is fp64: B N exponentials are nothing next to the launch, and dlogits comes out as the rounding
// of the exact value instead of carrying an fp32 log-sum-exp.  The integer counts use vector atomics.
//   SCORES: the rows are the sigmoid outputs s = sigmoid(z) of the deep classifiers, which the reference trainer hands to
// nn.CrossEntropyLoss as they are (models/deep_classifiers.py:97-99): loss = CE(s), and the gradient written is the one with
// respect to the pre-sigmoid z, (softmax(s) - onehot) s (1 - s), with s (1 - s) formed from the stored fp32 score (a score
// saturated at 0 or 1 gives exactly 0).
// ------------------------------------------------------------------------------------------
constexpr int CE_WAVES = 16;

// arg-max rule of torch.argmax (and labels_from_scores_kernel): the first maximum, a NaN counts as the maximum
__device__ __forceinline__ bool ce_better(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

template <bool SCORES>
__global__ __launch_bounds__(CE_WAVES * 64) void ce_loss_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                float* __restrict__ dlogits, float* __restrict__ dbias,
                                                                long long* __restrict__ pred, double* loss_sum, long long* count,
                                                                unsigned long long* confusion, int32_t* err, int B, int N,
                                                                int ldl, int ldd, float grad_scale,
                                                                const int32_t* __restrict__ active, long long s_logits,
                                                                long long s_labels, long long s_dlogits, long long s_dbias,
                                                                long long s_pred, long long s_stats) {
  // member blockIdx.x of a group (tl_ce_loss_group): one workgroup per member, whose arrays lie s_* elements behind member 0's
  // (s_stats: 8-byte words, for loss_sum, count, confusion and err alike); a member whose active word is 0 writes nothing.
  // The single launch is member 0 of a group of one.
  const int mem = blockIdx.x;
  if (active != nullptr && active[mem] == 0) return;
  logits += mem * s_logits;
  if (labels != nullptr) labels += mem * s_labels;
  if (dlogits != nullptr) dlogits += mem * s_dlogits;
  if (dbias != nullptr) dbias += mem * s_dbias;
  if (pred != nullptr) pred += mem * s_pred;
  if (labels != nullptr) {
    loss_sum += mem * s_stats;
    count += mem * s_stats;
    confusion += mem * s_stats;
    err += 2 * mem * s_stats;
  }
  __shared__ double s_db[CE_WAVES][64];
  __shared__ double s_loss[CE_WAVES];
  __shared__ int s_cnt[CE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool col = lane < N;
  double db = 0.0, loss = 0.0;
  int cnt = 0;
  for (int b = wave; b < B; b += CE_WAVES) {
    const float x = col ? logits[(long long)b * ldl + lane] : 0.f;
    float bv = x;
    int bi = col ? lane : 64 + lane;                     // lanes past the row lose against every column
    if (!col) bv = -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ce_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (pred != nullptr && lane == 0) pred[b] = bi;
    if (labels == nullptr) continue;                     // prediction only (uniform)
    const long long y = labels[b];
    const bool ok = y >= 0 && y < N;                     // uniform over the wave
    const double m = (double)bv;
    const double e = col ? exp((double)x - m) : 0.0;
    double s = e;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    float g = 0.f;
    if (ok) {
      double gd = (e / s - (lane == (int)y ? 1.0 : 0.0)) * (double)grad_scale;
      if constexpr (SCORES) gd *= (double)x * (1.0 - (double)x);       // d sigmoid / dz off the stored score
      g = (float)gd;
      const double xy = (double)__shfl(x, (int)y, 64);
      loss += log(s) + m - xy;
      cnt += 1;
      if (col) db += (double)g;
      if (lane == 0) atomicAdd(&confusion[(long long)y * N + bi], 1ULL);
    } else if (lane == 0) {
      *err = 1;
    }
    if (dlogits != nullptr && lane < ldd) dlogits[(long long)b * ldd + lane] = col ? g : 0.f;
  }
  if (labels == nullptr) return;
  s_db[wave][lane] = db;
  if (lane == 0) {
    s_loss[wave] = loss;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (wave != 0) return;
  if (dbias != nullptr && col) {
    double t = 0.0;
    for (int w = 0; w < CE_WAVES; ++w) t += s_db[w][lane];
    dbias[lane] = (float)t;
  }
  if (lane == 0) {
    double t = 0.0;
    long long c = 0;
    for (int w = 0; w < CE_WAVES; ++w) {
      t += s_loss[w];
      c += s_cnt[w];
    }
    *loss_sum += t;                                      // launches on one stream are ordered: no other writer
    *count += c;
  }
}

// ------------------------------------------------------------------------------------------
// backward of a head layer z = h W^T (+ b), N <= 64 outputs over K inputs, in one pass over h.  A thread owns four
// neighbouring columns k (16-byte loads and stores, a wave covers 1 KB of a row), so dw[n][k] = sum_b dl[b][n] h[b][k],
// dh[b][k] = sum_n dl[b][n] W[n][k] and the bias gradient of the layer below are sums a thread forms alone, in row order: no
// atomics, no cross-lane traffic, the same bits every run.  One-wave workgroups: K / 4 threads is all the parallelism there
// is, and 64-thread groups spread them over the most CUs.  dlogits reaches the lanes as LDS broadcasts, HB_RB rows at a time.
// HB_NT outputs are live at once (their W columns, dw accumulators and the sums s below: 96 registers); a wider head repeats
// the row walk per HB_NT outputs - W and dw still move once, h comes from L2 on the repeats and dh is carried through its
// own storage.  The heads this serves have 2 .. 8 classes: one walk.
//   dbias_h[k] = sum_b dh[b][k] is formed as sum_n W[n][k] s[n][k] with s[n][k] = sum_b act'(h[b][k]) dl[b][n] - the same
// number, and it does not need dh: the result has the same bits whether dh is asked for or not.
// ------------------------------------------------------------------------------------------
constexpr int HB_NT = 8, HB_RB = 64;

__device__ __forceinline__ f32x4 hb_dact(const f32x4 h, int act, float slope) {
  f32x4 d = {1.f, 1.f, 1.f, 1.f};
  if (act != 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = h[q] > 0.f ? 1.f : slope;
  }
  return d;
}

__global__ __launch_bounds__(64) void head_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ h,
                                                      const float* __restrict__ W, float* dh, float* __restrict__ dbias_h,
                                                      float* __restrict__ dw, int B, int K, int N, int ldd, int act, float slope,
                                                      const int32_t* __restrict__ active, long long s_dl, long long s_h,
                                                      long long s_W, long long s_dh, long long s_dbh, long long s_dw) {
  // member blockIdx.y of a group (tl_head_bwd_act_group): its dl, h, W, dh, dbias_h and dw lie s_* elements behind member 0's; a
  // member whose active word is 0 writes nothing.  The single launch is member 0 of a group of one.
  const int mem = blockIdx.y;
  if (active != nullptr && active[mem] == 0) return;
  dl += mem * s_dl;
  h += mem * s_h;
  W += mem * s_W;
  if (dh != nullptr) dh += mem * s_dh;
  if (dbias_h != nullptr) dbias_h += mem * s_dbh;
  if (dw != nullptr) dw += mem * s_dw;
  __shared__ __attribute__((aligned(16))) float sd[HB_RB][HB_NT];
  const int K4 = K >> 2;
  const int k4 = blockIdx.x * 64 + threadIdx.x;
  const bool live = k4 < K4;
  const bool want_s = dbias_h != nullptr, need_h = dw != nullptr || act != 0;
  const int ntiles = (N + HB_NT - 1) / HB_NT;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 dbh = zero;
#pragma unroll 1
  for (int t = 0; t < ntiles; ++t) {
    const int n0 = t * HB_NT;
    const bool last = t == ntiles - 1;
    f32x4 w[HB_NT], gw[HB_NT], s[HB_NT];
#pragma unroll
    for (int j = 0; j < HB_NT; ++j) {
      w[j] = (live && n0 + j < N) ? reinterpret_cast<const f32x4*>(W)[(long long)(n0 + j) * K4 + k4] : zero;
      gw[j] = zero;
      s[j] = zero;
    }
#pragma unroll 1
    for (int b0 = 0; b0 < B; b0 += HB_RB) {
      __syncthreads();                                   // the chunk before is still being read
      for (int i = threadIdx.x; i < HB_RB * HB_NT; i += 64) {
        const int r = i / HB_NT, c = i % HB_NT;
        sd[r][c] = (b0 + r < B && n0 + c < N) ? dl[(long long)(b0 + r) * ldd + n0 + c] : 0.f;
      }
      __syncthreads();
      if (!live) continue;
      const int rows = B - b0 < HB_RB ? B - b0 : HB_RB;
#pragma unroll 4
      for (int r = 0; r < rows; ++r) {
        const long long at = (long long)(b0 + r) * K4 + k4;
        const f32x4 d0 = *reinterpret_cast<const f32x4*>(&sd[r][0]), d1 = *reinterpret_cast<const f32x4*>(&sd[r][4]);
        const float d[HB_NT] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
        f32x4 hv = zero;
        if (need_h) hv = reinterpret_cast<const f32x4*>(h)[at];
        const f32x4 da = hb_dact(hv, act, slope);
        if (dw != nullptr) {
#pragma unroll
          for (int j = 0; j < HB_NT; ++j) gw[j] += d[j] * hv;
        }
        if (want_s) {
#pragma unroll
          for (int j = 0; j < HB_NT; ++j) s[j] += d[j] * da;
        }
        if (dh != nullptr) {
          f32x4 acc = t > 0 ? reinterpret_cast<const f32x4*>(dh)[at] : zero;
#pragma unroll
          for (int j = 0; j < HB_NT; ++j) acc += d[j] * w[j];
          if (last) acc *= da;
          reinterpret_cast<f32x4*>(dh)[at] = acc;
        }
      }
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < HB_NT; ++j) {
        if (dw != nullptr && n0 + j < N) reinterpret_cast<f32x4*>(dw)[(long long)(n0 + j) * K4 + k4] = gw[j];
        dbh += w[j] * s[j];
      }
    }
  }
  if (live && want_s) reinterpret_cast<f32x4*>(dbias_h)[k4] = dbh;
}

}  // namespace tl
using namespace tl;

template <bool SCORES>
static int ce_launch(const float* logits, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred, double* loss_sum,
                     int64_t* count, int64_t* confusion, int32_t* err, int B, int N, int ldl, int ldd, float grad_scale,
                     void* stream, int M = 1, int64_t s_logits = 0, int64_t s_labels = 0, int64_t s_dlogits = 0,
                     int64_t s_dbias = 0, int64_t s_pred = 0, int64_t s_stats = 0, const int32_t* active = nullptr) {
  TL_REQUIRE(logits != nullptr, "ce_loss: null logits");
  TL_REQUIRE(labels != nullptr || pred != nullptr, "ce_loss: null labels (allowed only to get pred alone)");
  TL_REQUIRE(labels == nullptr || (loss_sum && count && confusion && err),
             "ce_loss: null loss_sum / count / confusion / err (the statistics are not optional)");
  TL_REQUIRE(labels != nullptr || (!dlogits && !dbias), "ce_loss: dlogits / dbias need labels");
  TL_REQUIRE(N >= 1 && N <= 64, "ce_loss: the number of classes N must lie in [1, 64]");
  TL_REQUIRE(B >= 1, "ce_loss: the batch B must be at least 1");
  TL_REQUIRE(ldl >= N, "ce_loss: row stride ldl of logits below N");
  TL_REQUIRE(dlogits == nullptr || (ldd >= N && ldd <= 64), "ce_loss: row stride ldd of dlogits must lie in [N, 64]");
  hipLaunchKernelGGL(ce_loss_kernel<SCORES>, dim3((unsigned)M), dim3(CE_WAVES * 64), 0, (hipStream_t)stream, logits,
                     (const long long*)labels, dlogits, dbias, (long long*)pred, loss_sum, (long long*)count,
                     (unsigned long long*)confusion, err, B, N, ldl, ldd, grad_scale, active, (long long)s_logits,
                     (long long)s_labels, (long long)s_dlogits, (long long)s_dbias, (long long)s_pred, (long long)s_stats);
  return check_launch(SCORES ? "ce_scores_loss" : "ce_loss");
}

extern "C" int tl_ce_loss(const float* logits, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred,
                          double* loss_sum, int64_t* count, int64_t* confusion, int32_t* err, int B, int N, int ldl, int ldd,
                          float grad_scale, void* stream) {
  return ce_launch<false>(logits, labels, dlogits, dbias, pred, loss_sum, count, confusion, err, B, N, ldl, ldd, grad_scale,
                          stream);
}

extern "C" int tl_ce_loss_group(const float* logits, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred,
                                double* loss_sum, int64_t* count, int64_t* confusion, int32_t* err, int M, int B, int N, int ldl,
                                int ldd, float grad_scale, int64_t s_logits, int64_t s_labels, int64_t s_dlogits, int64_t s_dbias,
                                int64_t s_pred, int64_t s_stats, const int32_t* active, void* stream) {
  TL_REQUIRE_MEMBERS("ce_loss_group", M);
  TL_REQUIRE(B >= 1 && N >= 1 && s_logits >= 0 && s_labels >= 0, "ce_loss_group: bad sizes or a negative member stride");
  // members must not share what they write: every output stride covers a member's extent
  TL_REQUIRE(M == 1 || ((!dlogits || s_dlogits >= (int64_t)B * ldd) && (!dbias || s_dbias >= N) && (!pred || s_pred >= B)),
             "ce_loss_group: member stride of dlogits / dbias / pred shorter than a member's B x ldd / N / B elements");
  TL_REQUIRE(M == 1 || !labels || s_stats >= (int64_t)N * N,
             "ce_loss_group: member stride of the statistics words shorter than the N x N confusion matrix");
  return ce_launch<false>(logits, labels, dlogits, dbias, pred, loss_sum, count, confusion, err, B, N, ldl, ldd, grad_scale,
                          stream, M, s_logits, s_labels, s_dlogits, s_dbias, s_pred, s_stats, active);
}

extern "C" int tl_ce_scores_loss(const float* scores, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred,
                                 double* loss_sum, int64_t* count, int64_t* confusion, int32_t* err, int B, int N, int ldl,
                                 int ldd, float grad_scale, void* stream) {
  return ce_launch<true>(scores, labels, dlogits, dbias, pred, loss_sum, count, confusion, err, B, N, ldl, ldd, grad_scale,
                         stream);
}

static int head_bwd_launch(const float* dlogits, const float* h, const float* W, float* dh, float* dbias_h, float* dw, int B,
                           int K, int N, int ldd, int act, float slope, void* stream, int M = 1, int64_t s_dlogits = 0,
                           int64_t s_h = 0, int64_t s_W = 0, int64_t s_dh = 0, int64_t s_dbias_h = 0, int64_t s_dw = 0,
                           const int32_t* active = nullptr) {
  TL_REQUIRE(dlogits && h && W, "head_bwd: null dlogits / h / W");
  TL_REQUIRE(dh || dbias_h || dw, "head_bwd: null dh, dbias_h and dw (nothing to compute)");
  TL_REQUIRE(N >= 1 && N <= 64, "head_bwd: the number of outputs N must lie in [1, 64]");
  TL_REQUIRE(B >= 1 && K >= 4 && K % 4 == 0, "head_bwd: B >= 1 and K a positive multiple of 4 needed (columns move as float4)");
  TL_REQUIRE(ldd >= N, "head_bwd: row stride ldd of dlogits below N");
  TL_REQUIRE(act >= 0 && act <= 2, "head_bwd: act must be 0 (none), 1 (ReLU) or 2 (LeakyReLU)");
  TL_REQUIRE((((uintptr_t)h | (uintptr_t)W | (uintptr_t)dh | (uintptr_t)dbias_h | (uintptr_t)dw) & 15) == 0,
             "head_bwd: h, W, dh, dbias_h and dw must be 16-byte aligned");
  // members must not share what they write: every output stride covers a member's extent (products of the sizes checked above)
  TL_REQUIRE(M == 1 || !dh || s_dh >= (int64_t)B * K, "head_bwd: member stride of dh shorter than the B x K elements of a member");
  TL_REQUIRE(M == 1 || !dbias_h || s_dbias_h >= K, "head_bwd: member stride of dbias_h shorter than the K elements of a member");
  TL_REQUIRE(M == 1 || !dw || s_dw >= (int64_t)N * K, "head_bwd: member stride of dw shorter than the N x K elements of a member");
  const int blocks = (K / 4 + 63) / 64;
  hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)blocks, (unsigned)M), dim3(64), 0, (hipStream_t)stream, dlogits, h, W, dh,
                     dbias_h, dw, B, K, N, ldd, act, act == 1 ? 0.f : slope, active, (long long)s_dlogits, (long long)s_h,
                     (long long)s_W, (long long)s_dh, (long long)s_dbias_h, (long long)s_dw);
  return check_launch("head_bwd");
}

extern "C" int tl_head_bwd(const float* dlogits, const float* h, const float* W, float* dh, float* dbias_h, float* dw, int B,
                           int K, int N, int ldd, int act, float slope, void* stream) {
  return head_bwd_launch(dlogits, h, W, dh, dbias_h, dw, B, K, N, ldd, act, slope, stream);
}

extern "C" int tl_head_bwd_act_group(const float* dlogits, const float* h, const float* W, float* dh, float* dbias_h, float* dw,
                                     int M, int B, int K, int N, int ldd, int act, float slope, int64_t s_dlogits, int64_t s_h,
                                     int64_t s_W, int64_t s_dh, int64_t s_dbias_h, int64_t s_dw, const int32_t* active,
                                     void* stream) {
  TL_REQUIRE_MEMBERS("head_bwd_act_group", M);
  TL_REQUIRE(s_dlogits >= 0 && s_h >= 0 && s_W >= 0 && s_dh >= 0 && s_dbias_h >= 0 && s_dw >= 0 && s_h % 4 == 0 && s_W % 4 == 0 &&
                 s_dh % 4 == 0 && s_dbias_h % 4 == 0 && s_dw % 4 == 0,
             "head_bwd_act_group: the member strides of h, W, dh, dbias_h and dw must be non-negative multiples of 4 elements "
             "(16-byte aligned members)");
  return head_bwd_launch(dlogits, h, W, dh, dbias_h, dw, B, K, N, ldd, act, slope, stream, M, s_dlogits, s_h, s_W, s_dh, s_dbias_h,
                         s_dw, active);
}

// the dw-only form (the dense route of the logistic group): tl_head_bwd_act_group without dh and dbias_h, act 0
extern "C" int tl_head_bwd_group(const float* dlogits, const float* h, const float* W, float* dw, int M, int B, int K, int N,
                                 int ldd, int64_t s_dlogits, int64_t s_h, int64_t s_W, int64_t s_dw, const int32_t* active,
                                 void* stream) {
  return tl_head_bwd_act_group(dlogits, h, W, nullptr, nullptr, dw, M, B, K, N, ldd, 0, 0.f, s_dlogits, s_h, s_W, 0, 0, s_dw, active,
                               stream);
}
