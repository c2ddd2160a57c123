// Body of tn_short_kernel / tn_short_group_kernel (tonal_gemm.hip): statements, included into both __global__ functions so
// that a member of a group launch runs the single launch's arithmetic in its order.  Reads p (tl_tn_params), blockIdx.x / .y.
  __shared__ __attribute__((aligned(16))) float As[TS_K * TS_M];
  __shared__ __attribute__((aligned(16))) float Bs[TS_K * TS_N];
  const int tid = threadIdx.x, tn = tid & 31, tm = tid >> 5;
  const int ntn = (p.Ndim + TS_N - 1) / TS_N;
  const int mt = (int)(blockIdx.x / ntn) * TS_M, nt = (int)(blockIdx.x % ntn) * TS_N;
  const int kall = (int)(p.Krows < p.A_rows ? (p.Krows < p.B_rows ? p.Krows : p.B_rows) : (p.A_rows < p.B_rows ? p.A_rows : p.B_rows));
  // reduction split blockIdx.y: rows [kb, kr) = whole 64-row chunks (slab blockIdx.y; the caller sums the splitk slabs)
  const int per = ((kall + (int)gridDim.y - 1) / (int)gridDim.y + TS_K - 1) / TS_K * TS_K;
  const int kb = (int)blockIdx.y * per;
  const int kr = kb + per < kall ? kb + per : kall;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  // a chunk: A 64 rows x 8 float4, B 64 rows x 32 float4 (Mdim, Ndim % 4 == 0: a float4 is whole or absent)
  f32x4 ra[2], rb[8];
  // (every load is issued, from a clamped address, and zeroed afterwards: predicated loads come out as one exec-masked
  // region each, with the latencies in series)
  int ta[2], tb[8];                                          // (row offset in the chunk) % Tp: the division is done once
#pragma unroll
  for (int i = 0; i < 2; ++i) ta[i] = ((tid + i * 256) >> 3) % p.Tp;
#pragma unroll
  for (int i = 0; i < 8; ++i) tb[i] = ((tid + i * 256) >> 5) % p.Tp;
  const int kstep_mod = TS_K % p.Tp;
  int r0m = kb % p.Tp;                                       // r0 % Tp of the chunk being fetched
  auto fetch = [&](int r0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + i * 256, R = r0 + (idx >> 3), c = mt + (idx & 7) * 4;
      int t = ta[i] + r0m;
      t = t >= p.Tp ? t - p.Tp : t;
      const bool ok = R < kr && t < p.Tvalid && c < p.Mdim;
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.A + (long long)(R < kall ? R : kall - 1) * p.lda + (c < p.Mdim ? c : p.Mdim - 4));
      ra[i] = ok ? v : zero;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + i * 256, R = r0 + (idx >> 5), c = nt + (idx & 31) * 4;
      int t = tb[i] + r0m;
      t = t >= p.Tp ? t - p.Tp : t;
      const bool ok = R < kr && t < p.Tvalid && c < p.Ndim;
      const f32x4 v = *reinterpret_cast<const f32x4*>(p.B + (long long)(R < kall ? R : kall - 1) * p.ldb + (c < p.Ndim ? c : p.Ndim - 4));
      rb[i] = ok ? v : zero;
    }
    r0m += kstep_mod;
    r0m = r0m >= p.Tp ? r0m - p.Tp : r0m;
  };
  f32x4 acc[4] = {zero, zero, zero, zero};
  // optional column sums of A (the bias gradient of a Linear layer rides along): the workgroups of the first column tile,
  // threads 0..31, one column each, rows in order
  const bool do_cs = p.colsum != nullptr && nt == 0 && gridDim.y == 1 && tid < TS_M;
  float csum = 0.f;
  fetch(kb);
  for (int r0 = kb; r0 < kr; r0 += TS_K) {
    __syncthreads();                                       // the chunk in front has been consumed
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(As + ((tid + i * 256) >> 3) * TS_M + ((tid + i * 256) & 7) * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4*>(Bs + ((tid + i * 256) >> 5) * TS_N + ((tid + i * 256) & 31) * 4) = rb[i];
    __syncthreads();
    if (r0 + TS_K < kr) fetch(r0 + TS_K);
    if (do_cs) {
#pragma unroll 8
      for (int R = 0; R < TS_K; ++R) csum += As[R * TS_M + tid];
    }
#pragma unroll 8
    for (int R = 0; R < TS_K; ++R) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(As + R * TS_M + tm * 4);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(Bs + R * TS_N + tn * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += av[i] * bv;
    }
  }
  const int m0 = mt + tm * 4, n0 = nt + tn * 4;
  if (m0 < p.Mdim && n0 < p.Ndim) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4*>(p.slab + (long long)blockIdx.y * p.slab_stride + (long long)(m0 + i) * p.ldc + n0) = acc[i];
  }
  if (do_cs && mt + tid < p.Mdim) p.colsum[mt + tid] = csum;
