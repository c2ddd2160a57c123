// The body of nt_glds_kernel / nt_glds_group_kernel (tonal_gemm.hip), included into both: statements only, in the scope of
// `template <int EPI, int NI>` and the kernel's parameter struct `p`.  Kept as text, not as a __device__ function: the single
// launch's kernel then compiles to the instructions it had before the group form existed.
  constexpr int BM = 128, MI = 2, WN = 2, BN = 64 * NI;         // (shadows the file's 128-column constant)
  __shared__ __attribute__((aligned(16))) float lds[2 * G_AROWS * GK + G_NB * BN * GK];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 31, lh = lane >> 5;

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

  const int nkc_all = p.K / GK;
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

  // DMA piece = 16 rows x 64 B; lane -> (row = lane >> 2, physical chunk = lane & 3), and the source
  // chunk is the swizzled one: chunk ^ ((row >> 2) & 3) with row % 16 == lane >> 2
  const int prow = lane >> 2;
  const int src_chunk = (lane & 3) ^ ((lane >> 4) & 3);
  // A pieces: every wave issues 3 (pieces w, w+4 and 8); B pieces: 2 (w, w+4)
  const float* asrc[3];
  unsigned adst[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int piece = (i < 2) ? wave + 4 * i : 8;
    long long row = R0 + piece * 16 + prow;
    if (row > p.A_rows - 1) row = p.A_rows - 1;          // clamped rows only feed masked outputs
    asrc[i] = p.A + row * (long long)p.lda + src_chunk * 4;
    adst[i] = (unsigned)(piece * 16 * GK * 4);
  }
  const float* bsrc[NI];
  unsigned bdst[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int piece = wave + 4 * i;
    int n = n0 + piece * 16 + prow;
    if (n > p.N - 1) n = p.N - 1;                         // clamped columns are masked by the epilogue
    bsrc[i] = p.Bw + (long long)n * p.ldb + src_chunk * 4;
    bdst[i] = (unsigned)(piece * 16 * GK * 4);
  }
  const long long tap_stride = (long long)p.N * p.ldb;
  char* const lds_a = reinterpret_cast<char*>(lds);
  char* const lds_b = reinterpret_cast<char*>(lds) + 2 * G_AROWS * GK * 4;

  auto dma = [&](const float* g, char* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
  };
  auto issue_a = [&](int chunk) {
    const int kc = (kc_begin + chunk) * GK;
    char* base = lds_a + (chunk & 1) * (G_AROWS * GK * 4);
#pragma unroll
    for (int i = 0; i < 3; ++i) dma(asrc[i] + kc, base + adst[i]);
  };
  auto issue_b = [&](int step, int chunk, int j) {
    const long long off = (long long)j * tap_stride + (long long)(kc_begin + chunk) * GK;
    char* base = lds_b + (step & (G_NB - 1)) * (BN * GK * 4);
#pragma unroll
    for (int i = 0; i < NI; ++i) dma(bsrc[i] + off, base + bdst[i]);
  };

  // fragment read offsets (bytes): row r, logical chunk c -> r*64 + ((c ^ ((r >> 2) & 3)) * 16)
  f32x4 fa0[MI], fb0[NI], fa1[MI], fb1[NI];
  auto load_frag = [&](f32x4 (&fa)[MI], f32x4 (&fb)[NI], int abuf, int bslot, int j, int kk) {
    const int c = 2 * kk + lh;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int r = wm * 64 + i * 32 + lr + j;
      fa[i] = *reinterpret_cast<const f32x4*>(lds_a + abuf * (G_AROWS * GK * 4) + r * 64 + ((c ^ ((r >> 2) & 3)) << 4));
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = wn * (NI * 32) + i * 32 + lr;
      fb[i] = *reinterpret_cast<const f32x4*>(lds_b + bslot * (BN * GK * 4) + r * 64 + ((c ^ ((r >> 2) & 3)) << 4));
    }
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

  // ---- prologue: A(0), B(0..2) in flight; wait for A(0) and B(0)
  int c_ld = 0, j_ld = 0;
  auto advance = [&](int& c, int& j) {
    if (++j == J) {
      j = 0;
      ++c;
    }
  };
  if (nsteps > 0) {
    issue_a(0);
    issue_b(0, 0, 0);
    advance(c_ld, j_ld);
    if (nsteps > 1) issue_b(1, c_ld, j_ld);
    advance(c_ld, j_ld);
    if (nsteps > 2) issue_b(2, c_ld, j_ld);
    advance(c_ld, j_ld);
    // everything but the last two B pieces-pairs must have landed (A(0), B(0))
    if (nsteps > 2) {
      if constexpr (NI == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    } else if (nsteps > 1) {
      if constexpr (NI == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  // s_waitcnt needs an immediate: dispatch the (wave-uniform) count over the few values it takes
  auto wait_all_but = [&](int n) {
    switch (n) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
      case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };

  int c_cur = 0, j_cur = 0;
  for (int s = 0; s < nsteps; ++s) {
    const int chunk = c_cur, j = j_cur;
    const int abuf = chunk & 1, bslot = s & (G_NB - 1);
    load_frag(fa0, fb0, abuf, bslot, j, 0);
    // DMA issue order inside a step: A(chunk+1) (first tap of a chunk; its slot held chunk-1), then
    // B(s+3) (its ring slot held B(s-1), released at the last barrier)
    const bool has_next = chunk + 1 < nchunks;
    const bool lda_ = (j == 0) && has_next;
    const bool ldb = s + 3 < nsteps;
    if (lda_) issue_a(chunk + 1);
    if (ldb) issue_b(s + 3, c_ld, j_ld);
    if (s > 0) mfma_group(fa1, fb1);             // k-group 1 of the previous step (registers)
    load_frag(fa1, fb1, abuf, bslot, j, 1);
    mfma_group(fa0, fb0);
    advance(c_cur, j_cur);
    advance(c_ld, j_ld);
    if (s + 1 < nsteps) {
      // The next step reads B(s+1) and, when it opens a chunk, A(chunk+1).  vmcnt retires this
      // wave's pieces in issue order, so allow exactly the pieces issued AFTER the youngest needed
      // one to stay in flight: this step's own, B(s+2) (issued one step ago) and - when the next
      // step stays in this chunk - an A(chunk+1) issued one step ago.
      int n = (ldb ? NI : 0);                              // (NI B pieces per wave and step)
      if (J == 1) {
        // A(chunk+1) was issued this step (before B(s+3)) and is needed next step
      } else {
        n += (lda_ ? 3 : 0) + ((s + 2 < nsteps) ? NI : 0);
        if (j == 1 && j != J - 1 && has_next) n += 3;
      }
      wait_all_but(n);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }
  if (nsteps > 0) mfma_group(fa1, fb1);
  nt_epilogue<EPI, MI, NI>(p, acc, R0, n0, wm, wn, lr, lh, z);
