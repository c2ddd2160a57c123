// The body of nt_window_kernel / nt_window_group_kernel (tonal_gemm.hip), included into both: statements only, in the scope of
// `template <int BM, int LOADER, int EPI>` and the kernel's parameter struct `p`.  Kept as text, not as a __device__ function: the
// single launch's kernel then compiles to the instructions it had before the group form existed.
  constexpr int NTHR = nt_cfg<BM>::NTHR;
  constexpr int WM = nt_cfg<BM>::WM;
  constexpr int WN = nt_cfg<BM>::WN;
  constexpr int MI = BM / (32 * WM);               // 32x32 tiles per wave along M
  constexpr int NI = BN / (32 * WN);
  constexpr int AROWS = BM + 6;                    // staged rows incl. the tap window (J <= 7)
  constexpr int A_F4 = (LOADER == LOAD_DIRECT) ? ((AROWS * 8 + NTHR - 1) / NTHR) : ((AROWS / 2 * 8 + NTHR - 1) / NTHR);
  constexpr int B_F4 = BN * 8 / NTHR;

  __shared__ __attribute__((aligned(16))) float lds[2 * AROWS * LDS_LD + 2 * BN * LDS_LD];
  float* As = lds;                                 // [2][AROWS][LDS_LD]
  float* Bs = lds + 2 * AROWS * LDS_LD;            // [2][BN][LDS_LD]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;

  // XCD-aware tile order: blocks b and b+8 share an XCD/L2, so give each XCD a contiguous
  // run of logical tiles; consecutive logical tiles walk N first and share the A panel.
  const int ntn = (p.N + BN - 1) / BN;
  const long long ntm = (p.M + BM - 1) / BM;
  const long long nwg = ntm * ntn;
  long long bid = blockIdx.x;
  {
    const long long q = nwg / 8, r = nwg % 8, x = bid % 8, i = bid / 8;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
  }
  const long long tm = bid / ntn;
  const int tn = (int)(bid % ntn);
  const long long R0 = tm * BM;
  const int n0 = tn * BN;
  const int J = p.J;
  const int arows_used = BM + J - 1;

  // K range (split-K only meaningful for J == 1 plain GEMMs, but handled generally)
  const int nkc_all = (p.K + BK - 1) / BK;
  const int z = blockIdx.y;
  const int kc_per = (nkc_all + p.splitk - 1) / p.splitk;
  const int kc_begin = z * kc_per;
  const int kc_end = min(nkc_all, kc_begin + kc_per);
  const int nchunks = max(0, kc_end - kc_begin);
  const int nsteps = nchunks * J;

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 ra[A_F4];          // staged A (DIRECT) or G (UNPOOL)
  uint32_t rbits[A_F4];    // UNPOOL: raw 32-bit arg word (bit set -> odd row of the pair); the
                           // nibble is extracted at LDS-store time so the load stays in flight
  f32x4 rbP[B_F4], rbQ[B_F4];    // two B staging sets: B is prefetched TWO K-steps ahead (HBM/L2 latency
                           // under full load exceeds one 64-MFMA step; measured in scripts/mfma_ablate.hip)

  const long long Abase = R0 + p.row_shift;        // first staged A row (even for UNPOOL)

  // Per-thread row pointers and validity are loop-invariant (a thread stages the same rows of
  // every K-chunk): hoist them, so a K-step issues its global loads with one 64-bit add each.
  const float* aptr[A_F4];
  const uint32_t* abptr[A_F4];
  bool aok[A_F4];
  (void)abptr;
#pragma unroll
  for (int i = 0; i < A_F4; ++i) {
    const int idx = tid + i * NTHR;
    const int r = idx >> 3, c4 = idx & 7;
    if constexpr (LOADER == LOAD_DIRECT) {
      const long long row = Abase + r;
      aok[i] = r < arows_used && row >= 0 && row < p.A_rows;
      aptr[i] = p.A + (aok[i] ? row : 0) * (long long)p.lda + c4 * 4;
      abptr[i] = nullptr;
    } else {
      const long long prow = (Abase >> 1) + r;     // Abase is even
      aok[i] = (r < (arows_used + 1) / 2) && prow >= 0 && prow < p.A_rows &&
               (int)((2 * prow) % p.Tp) < p.Tvalid_in;
      aptr[i] = p.A + (aok[i] ? prow : 0) * (long long)p.lda + c4 * 4;
      abptr[i] = p.abits + (aok[i] ? prow : 0) * (long long)p.ld_abits;
    }
  }
  const float* bptr[B_F4];
  bool bok[B_F4];
#pragma unroll
  for (int i = 0; i < B_F4; ++i) {
    const int idx = tid + i * NTHR;
    const int r = idx >> 3, c4 = idx & 7;
    bok[i] = (n0 + r) < p.N;
    bptr[i] = p.Bw + (long long)(bok[i] ? n0 + r : 0) * p.ldb + c4 * 4;
  }
  const bool ktail = (p.K % BK) != 0;             // wave-uniform: the hot shapes have K % 32 == 0
  const int kq = (tid & 7) * 4;
  const long long tap_stride = (long long)p.N * p.ldb;

  auto load_a = [&](int chunk) {
    const int kc = (kc_begin + chunk) * BK;
    const bool kok = !ktail || (kc + kq) < p.K;
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      uint32_t nib = 0;
      if (aok[i] && kok) {
        v = *reinterpret_cast<const f32x4*>(aptr[i] + kc);
        if constexpr (LOADER == LOAD_UNPOOL) nib = abptr[i][kc >> 5];
      }
      ra[i] = v;
      rbits[i] = nib;
    }
  };
  auto store_a = [&](int buf) {
    float* dst = As + buf * AROWS * LDS_LD;
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
      const int idx = tid + i * NTHR;
      const int r = idx >> 3, c4 = idx & 7;
      if constexpr (LOADER == LOAD_DIRECT) {
        if (r < AROWS) *reinterpret_cast<f32x4*>(dst + r * LDS_LD + c4 * 4) = ra[i];
      } else {
        if (r < AROWS / 2) {
          f32x4 e, o;
          const uint32_t nibv = rbits[i] >> ((c4 * 4) & 31);     // kc is a multiple of 32
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool odd = (nibv >> q) & 1u;
            e[q] = odd ? 0.f : ra[i][q];
            o[q] = odd ? ra[i][q] : 0.f;
          }
          *reinterpret_cast<f32x4*>(dst + (2 * r) * LDS_LD + c4 * 4) = e;
          *reinterpret_cast<f32x4*>(dst + (2 * r + 1) * LDS_LD + c4 * 4) = o;
        }
      }
    }
  };
  auto load_b = [&](f32x4 (&rb)[B_F4], int chunk, int j) {
    const int kc = (kc_begin + chunk) * BK;
    const bool kok = !ktail || (kc + kq) < p.K;
    const long long off = (long long)j * tap_stride + kc;     // wave-uniform
#pragma unroll
    for (int i = 0; i < B_F4; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (bok[i] && kok) v = *reinterpret_cast<const f32x4*>(bptr[i] + off);
      rb[i] = v;
    }
  };
  auto store_b = [&](const f32x4 (&rb)[B_F4], int buf) {
    float* dst = Bs + buf * BN * LDS_LD;
#pragma unroll
    for (int i = 0; i < B_F4; ++i) {
      const int idx = tid + i * NTHR;
      const int r = idx >> 3, c4 = idx & 7;
      *reinterpret_cast<f32x4*>(dst + r * LDS_LD + c4 * 4) = rb[i];
    }
  };

  // Fragment sets F0 / F1 (statically named): while the MFMAs of one 8-deep k-group run, the
  // ds_read_b128 of the next group are in flight; the last group of a K-step is carried in
  // registers ACROSS the barrier, so the matrix pipe has work the moment the barrier opens, and
  // the LDS stores of the next stage are issued mid-step (their target buffer was released at
  // the previous barrier), leaving nothing but the barrier itself at the end of a step.
  f32x4 fa0[MI], fb0[NI], fa1[MI], fb1[NI];
  auto load_frag = [&](f32x4 (&fa)[MI], f32x4 (&fb)[NI], int abuf, int bbuf, int j, int kk) {
    const float* a_s = As + abuf * AROWS * LDS_LD + (wm * (MI * 32) + lr + j) * LDS_LD + lh * 4 + kk * 8;
    const float* b_s = Bs + bbuf * BN * LDS_LD + (wn * (NI * 32) + lr) * LDS_LD + lh * 4 + kk * 8;
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const f32x4*>(a_s + i * 32 * LDS_LD);
#pragma unroll
    for (int i = 0; i < NI; ++i) fb[i] = *reinterpret_cast<const f32x4*>(b_s + i * 32 * LDS_LD);
  };
  auto mfma_group = [&](const f32x4 (&fa)[MI], const f32x4 (&fb)[NI]) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][q], fb[ni][q], acc[mi][ni], 0, 0, 0);
  };

  // One K-step.  `rb_ld` receives B(s+2); `rb_st` holds B(s+1) (loaded one step ago) and is written
  // to LDS mid-step.  A(chunk+1) is loaded at the first tap of a chunk and stored at its last tap.
  // (chunk, tap) counters advanced without divisions
  int c_cur = 0, j_cur = 0;          // step s
  int c_ld = 0, j_ld = 0;            // step s + 2 (next B tile to load)
  auto advance = [&](int& c, int& j) {
    if (++j == J) {
      j = 0;
      ++c;
    }
  };
  auto kstep = [&](int s, f32x4 (&rb_ld)[B_F4], const f32x4 (&rb_st)[B_F4]) {
    const int chunk = c_cur, j = j_cur;
    const int abuf = chunk & 1, bbuf = s & 1;
    const bool more = s + 1 < nsteps;
    const bool has_next_chunk = chunk + 1 < nchunks;
    load_frag(fa0, fb0, abuf, bbuf, j, 0);
    if (s + 2 < nsteps) load_b(rb_ld, c_ld, j_ld);
    if (j == 0 && has_next_chunk) load_a(chunk + 1);
    if (s > 0) mfma_group(fa1, fb1);             // k-group 3 of the previous step (registers)
    load_frag(fa1, fb1, abuf, bbuf, j, 1);
    mfma_group(fa0, fb0);
    load_frag(fa0, fb0, abuf, bbuf, j, 2);
    mfma_group(fa1, fb1);
    if (more) store_b(rb_st, bbuf ^ 1);
    if (j == J - 1 && has_next_chunk) store_a(abuf ^ 1);
    load_frag(fa1, fb1, abuf, bbuf, j, 3);
    mfma_group(fa0, fb0);
    advance(c_cur, j_cur);
    advance(c_ld, j_ld);
    __syncthreads();
  };

  if (nsteps > 0) {
    load_a(0);
    load_b(rbP, 0, 0);
    store_a(0);
    store_b(rbP, 0);
    advance(c_ld, j_ld);
    if (nsteps > 1) load_b(rbQ, c_ld, j_ld);
    advance(c_ld, j_ld);
  }
  __syncthreads();
  int s = 0;
  for (; s + 1 < nsteps; s += 2) {
    kstep(s, rbP, rbQ);
    kstep(s + 1, rbQ, rbP);
  }
  if (s < nsteps) kstep(s, rbP, rbQ);
  if (nsteps > 0) mfma_group(fa1, fb1);

  nt_epilogue<EPI, MI, NI>(p, acc, R0, n0, wm, wn, lr, lh, z);
