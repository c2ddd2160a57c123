// Device-resident batch loader: a batch of up to four tensors gathered by one index vector in ONE launch
// (data_loading/resident.py; the stock DataLoader indexes sample by sample in Python and stacks B views).
// Window extraction: n windows cut from one (C, T) recording by a table of starts in ONE launch (data_loading/epoching.py).
// See include/tonal_hip.h for the contracts.
#include "tonal_common.h"

namespace tl {

// One segment = one output tensor of the batch.  A *unit* is one contiguous copy: a whole sample (C * inner_bytes) without a
// channel list, one innermost row (inner_bytes) with one.  Units are cut into vectors of `width` bytes (16, 4 or 1: the widest
// that divides the unit and both base addresses, so that every unit of the segment starts aligned) and a thread moves
// GATHER_UNROLL vectors, all loads issued before the first store.  Consecutive lanes take consecutive vectors of the flat
// (batch row, unit, vector) index, so a row shorter than a wave's 1 KiB shares the wave with its neighbours and a segment of
// tiny rows (labels: 4 or 8 bytes each) is a handful of threads of one workgroup, not a workgroup per row.
struct gather_seg {
  const char* src;
  char* dst;
  const int32_t* chan;
  long long src_rows;      // samples in the source
  long long sample_bytes;  // C * inner_bytes
  long long unit_bytes;
  int C;
  unsigned n_unit;         // units per batch row: n_chan with a channel list, 1 without
  unsigned vec_per_unit;   // unit_bytes / width
  unsigned n_vec;          // n_idx * n_unit * vec_per_unit   (< 2^31)
  unsigned block0;         // first workgroup of the segment
  int width;
  long long dst_stride;    // bytes between the destinations of two members of a group (tl_gather_rows_group; 0 alone)
};
struct gather_args {
  gather_seg seg[4];
  int n;
};

#define GATHER_UNROLL 4
#define GATHER_PER_BLOCK (256 * GATHER_UNROLL)

// Three phases without a branch between the loads of one phase, so that each phase has GATHER_UNROLL loads in flight: the
// indices, the rows, the stores.  A thread past the end, or one whose index is out of range, reads the segment's first
// vector instead (always there: src_rows, C and inner_bytes are positive) and stores nothing.  Named variables, not arrays:
// the compiler merges the four guarded stores of an array into one block that indexes it dynamically, which puts the rows
// in scratch memory and a full wait between the loads.
#define GATHER_INDEX(u)                                                              \
  const unsigned v##u = first + u * 256;                                               \
  bool ok##u = v##u < g.n_vec;                                                       \
  const unsigned unit##u = ok##u ? v##u / g.vec_per_unit : 0u;                       \
  const unsigned off##u = ok##u ? v##u - unit##u * g.vec_per_unit : 0u;              \
  const unsigned b##u = unit##u / g.n_unit, j##u = unit##u - b##u * g.n_unit;        \
  const long long r##u = idx[b##u];                                                  \
  const int c##u = CHAN ? g.chan[j##u] : (int)j##u; /* a template argument: no branch between the loads */
#define GATHER_LOAD(u)                                                                                        \
  {                                                                                                           \
    const bool r_ok = r##u >= 0 && r##u < g.src_rows, c_ok = c##u >= 0 && c##u < g.C;                         \
    if (ok##u) bad |= (r_ok ? 0 : 1) | (c_ok ? 0 : 2);                                                        \
    ok##u = ok##u && r_ok && c_ok;                                                                            \
  }                                                                                                           \
  const long long so##u =                                                                                     \
      ok##u ? r##u * g.sample_bytes + (long long)c##u * g.unit_bytes + (long long)off##u * (long long)sizeof(V) : 0; \
  const V val##u = *reinterpret_cast<const V*>(g.src + so##u);
#define GATHER_STORE(u) \
  if (ok##u) *reinterpret_cast<V*>(dst + (long long)v##u * (long long)sizeof(V)) = val##u;

template <typename V, bool CHAN>
__device__ __forceinline__ void gather_copy(const gather_seg& g, const long long* __restrict__ idx, int* __restrict__ err,
                                            unsigned blk, char* __restrict__ dst) {
  static_assert(GATHER_UNROLL == 4, "the phases below are written out four times");
  const unsigned first = blk * GATHER_PER_BLOCK + threadIdx.x;
  int bad = 0;
  GATHER_INDEX(0) GATHER_INDEX(1) GATHER_INDEX(2) GATHER_INDEX(3)
  GATHER_LOAD(0) GATHER_LOAD(1) GATHER_LOAD(2) GATHER_LOAD(3)
  GATHER_STORE(0) GATHER_STORE(1) GATHER_STORE(2) GATHER_STORE(3)
  if (bad) atomicOr(err, bad);
}
#undef GATHER_INDEX
#undef GATHER_LOAD
#undef GATHER_STORE

// Member blockIdx.y of a group (tl_gather_rows_group) reads its own index vector, idx_stride words behind member 0's, and writes
// dst_stride bytes behind member 0's destination; a member whose active word is 0 loads and writes nothing.  The single launch
// is member 0 of a group of one.
__global__ __launch_bounds__(256) void gather_rows_kernel(gather_args a, const long long* __restrict__ idx, int* __restrict__ err,
                                                          const int32_t* __restrict__ active, long long idx_stride) {
  const int mem = blockIdx.y;
  if (active != nullptr && active[mem] == 0) return;
  idx += mem * idx_stride;
  int s = 0;
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (i < a.n && blockIdx.x >= a.seg[i].block0) s = i;
  const gather_seg& g = a.seg[s];
  const unsigned blk = blockIdx.x - g.block0;
  const bool chan = g.chan != nullptr;
  char* dst = g.dst + mem * g.dst_stride;
  if (g.width == 16) {
    if (chan) gather_copy<uint4, true>(g, idx, err, blk, dst); else gather_copy<uint4, false>(g, idx, err, blk, dst);
  } else if (g.width == 4) {
    if (chan) gather_copy<uint32_t, true>(g, idx, err, blk, dst); else gather_copy<uint32_t, false>(g, idx, err, blk, dst);
  } else {
    if (chan) gather_copy<uint8_t, true>(g, idx, err, blk, dst); else gather_copy<uint8_t, false>(g, idx, err, blk, dst);
  }
}

// ---- tl_extract_windows: dst[i][c][:] = src[c][starts[i] : starts[i] + L] -----------------------------------------------------------
// A window starts at an arbitrary sample, so every (window, channel) row has its own source alignment and no width above
// the element's holds for all of them: one element per lane per copy, WINDOW_UNROLL copies per thread, all loads issued
// before the first store (gather_copy's phases).  Lanes run along the flat (window, channel, sample) index: a row shorter
// than a wave shares it with the next row, and the destination is written front to back in whole cache lines.
// The flat index is 64-bit; it is divided once per thread (the workgroup's first element, uniform) and once more in 32 bits,
// and a thread's further copies, 256 elements apart, advance (window, channel, sample) by the host's split of 256.
struct window_args {
  const char* src;
  char* dst;
  long long C, T, ld_src, L;
  unsigned long long total;  // n * C * L elements
  unsigned q256, r256;       // 256 = q256 * L + r256
  unsigned qC, rC;           // q256 = qC * C + rC
};

#define WINDOW_UNROLL 8
#define WINDOW_PER_BLOCK (256 * WINDOW_UNROLL)

// a thread past the end reads starts[0], a thread of a bad window src[0] (both there: n, C, T >= 1); neither stores
#define WINDOW_INDEX(u)                                                             \
  const unsigned long long v##u = first + u * 256ull;                               \
  bool ok##u = v##u < a.total;                                                      \
  const unsigned i##u = ok##u ? i : 0u, c##u = c, j##u = j;                         \
  {                                                                                 \
    j += a.r256;                                                                    \
    const unsigned carry = j >= L ? 1u : 0u;                                        \
    j -= carry ? L : 0u;                                                            \
    c += a.rC + carry;                                                              \
    const unsigned wrap = c >= C ? 1u : 0u;                                         \
    c -= wrap ? C : 0u;                                                             \
    i += a.qC + wrap;                                                               \
  }                                                                                 \
  const long long s##u = starts[i##u];
#define WINDOW_LOAD(u)                                                              \
  {                                                                                 \
    const bool s_ok = s##u >= 0 && s##u <= a.T - a.L;                               \
    if (ok##u && !s_ok) bad = 2;                                                    \
    ok##u = ok##u && s_ok;                                                          \
  }                                                                                 \
  const long long so##u = ok##u ? (long long)c##u * a.ld_src + s##u + (long long)j##u : 0; \
  const E val##u = src[so##u];
#define WINDOW_STORE(u) \
  if (ok##u) dst[v##u] = val##u;

template <typename E>
__global__ __launch_bounds__(256) void extract_windows_kernel(window_args a, const long long* __restrict__ starts,
                                                              int* __restrict__ err) {
  static_assert(WINDOW_UNROLL == 8, "the phases below are written out eight times");
  const E* __restrict__ src = reinterpret_cast<const E*>(a.src);
  E* __restrict__ dst = reinterpret_cast<E*>(a.dst);
  const unsigned L = (unsigned)a.L, C = (unsigned)a.C;              // both below 2^30 (host check)
  const unsigned long long base = (unsigned long long)blockIdx.x * WINDOW_PER_BLOCK;
  const unsigned long long row0 = base / (unsigned long long)a.L;    // uniform: rows (window, channel) before the workgroup
  const unsigned o = (unsigned)(base - row0 * (unsigned long long)a.L) + threadIdx.x;   // < L + 256
  const unsigned dq = o / L;
  const unsigned row = (unsigned)row0 + dq;                         // n * C < 2^31
  unsigned j = o - dq * L, i = row / C;
  unsigned c = row - i * C;
  const unsigned long long first = base + threadIdx.x;
  int bad = 0;
  WINDOW_INDEX(0) WINDOW_INDEX(1) WINDOW_INDEX(2) WINDOW_INDEX(3) WINDOW_INDEX(4) WINDOW_INDEX(5) WINDOW_INDEX(6) WINDOW_INDEX(7)
  WINDOW_LOAD(0) WINDOW_LOAD(1) WINDOW_LOAD(2) WINDOW_LOAD(3) WINDOW_LOAD(4) WINDOW_LOAD(5) WINDOW_LOAD(6) WINDOW_LOAD(7)
  WINDOW_STORE(0) WINDOW_STORE(1) WINDOW_STORE(2) WINDOW_STORE(3) WINDOW_STORE(4) WINDOW_STORE(5) WINDOW_STORE(6) WINDOW_STORE(7)
  if (bad) atomicOr(err, bad);
}
#undef WINDOW_INDEX
#undef WINDOW_LOAD
#undef WINDOW_STORE

}  // namespace tl

using namespace tl;

// dst_stride null: the single launch (M = 1)
static int gather_launch(const void* const* src, void* const* dst, const int64_t* dst_stride, const int64_t* src_rows,
                         const int64_t* C, const int64_t* inner_bytes, const int32_t* const* chan, const int64_t* n_chan, int n_seg,
                         const int64_t* idx, int64_t idx_stride, int64_t n_idx, int M, const int32_t* active, int32_t* err,
                         void* stream) {
  TL_REQUIRE(n_seg >= 1 && n_seg <= 4, "gather_rows: 1 to 4 segments per launch, at most 4 (got %d)", n_seg);
  TL_REQUIRE(src && dst && src_rows && C && inner_bytes && chan && n_chan, "gather_rows: null table");
  TL_REQUIRE(idx && err, "gather_rows: null index vector or error word");
  TL_REQUIRE(n_idx > 0 && n_idx < (1LL << 31), "gather_rows: n_idx must be in [1, 2^31) (got %lld)", (long long)n_idx);
  gather_args a;
  a.n = n_seg;
  unsigned long long blocks = 0;
  for (int i = 0; i < 4; ++i) {
    gather_seg& g = a.seg[i];
    if (i >= n_seg) {
      g = gather_seg{};
      g.block0 = 0xffffffffu;
      continue;
    }
    TL_REQUIRE(src[i] && dst[i], "gather_rows: null tensor in segment %d", i);
    TL_REQUIRE(src_rows[i] > 0 && C[i] > 0 && inner_bytes[i] > 0 && n_chan[i] >= 0,
               "gather_rows: segment %d: src_rows, C and inner_bytes must be positive, n_chan non-negative", i);
    TL_REQUIRE(n_chan[i] == 0 || chan[i], "gather_rows: segment %d: n_chan = %lld with a null chan", i, (long long)n_chan[i]);
    TL_REQUIRE(!chan[i] || n_chan[i] > 0, "gather_rows: segment %d: a channel list needs n_chan > 0", i);
    TL_REQUIRE(C[i] < (1LL << 31) && inner_bytes[i] < (1LL << 31) && n_chan[i] < (1LL << 31),
               "gather_rows: segment %d: C, n_chan or inner_bytes too large", i);
    g.src = (const char*)src[i];
    g.dst = (char*)dst[i];
    g.chan = chan[i];
    g.src_rows = src_rows[i];
    g.C = (int)C[i];
    g.sample_bytes = C[i] * inner_bytes[i];
    g.unit_bytes = chan[i] ? inner_bytes[i] : g.sample_bytes;
    g.n_unit = chan[i] ? (unsigned)n_chan[i] : 1u;
    g.dst_stride = dst_stride ? dst_stride[i] : 0;
    const uintptr_t al = (uintptr_t)g.src | (uintptr_t)g.dst | (uintptr_t)g.unit_bytes | (uintptr_t)g.dst_stride;
    g.width = (al & 15) == 0 ? 16 : (al & 3) == 0 ? 4 : 1;
    const long long vpu = g.unit_bytes / g.width;
    // n_idx, n_unit, C and inner_bytes are below 2^31: every product below fits 64 bits when taken one factor at a time
    TL_REQUIRE(vpu < (1LL << 31) && (long long)g.n_unit * vpu < (1LL << 31) && n_idx * ((long long)g.n_unit * vpu) < (1LL << 31),
               "gather_rows: segment %d: more than 2^31 vectors of %d bytes in one batch", i, g.width);
    g.vec_per_unit = (unsigned)vpu;
    g.n_vec = (unsigned)(n_idx * (long long)g.n_unit * vpu);
    g.block0 = (unsigned)blocks;
    blocks += (g.n_vec + (unsigned long long)GATHER_PER_BLOCK - 1) / GATHER_PER_BLOCK;
    TL_REQUIRE(blocks < (1ULL << 31), "gather_rows: too many workgroups");
    TL_REQUIRE(M == 1 || g.dst_stride >= n_idx * (long long)g.n_unit * g.unit_bytes,
               "gather_rows_group: segment %d: member stride of dst shorter than the bytes of a member's batch", i);
  }
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)blocks, (unsigned)M), dim3(256), 0, (hipStream_t)stream, a,
                     (const long long*)idx, (int*)err, active, (long long)idx_stride);
  return check_launch("gather_rows");
}

extern "C" int tl_gather_rows(const void* const* src, void* const* dst, const int64_t* src_rows, const int64_t* C,
                              const int64_t* inner_bytes, const int32_t* const* chan, const int64_t* n_chan, int n_seg,
                              const int64_t* idx, int64_t n_idx, int32_t* err, void* stream) {
  return gather_launch(src, dst, nullptr, src_rows, C, inner_bytes, chan, n_chan, n_seg, idx, 0, n_idx, 1, nullptr, err, stream);
}

extern "C" int tl_gather_rows_group(const void* const* src, void* const* dst, const int64_t* dst_stride, const int64_t* src_rows,
                                    const int64_t* C, const int64_t* inner_bytes, const int32_t* const* chan,
                                    const int64_t* n_chan, int n_seg, const int64_t* idx, int64_t idx_stride, int64_t n_idx, int M,
                                    const int32_t* active, int32_t* err, void* stream) {
  TL_REQUIRE_MEMBERS("gather_rows_group", M);
  TL_REQUIRE(dst_stride != nullptr, "gather_rows_group: null table of member strides");
  TL_REQUIRE(M == 1 || idx_stride >= n_idx, "gather_rows_group: member stride of idx shorter than the n_idx indices of a batch");
  for (int i = 0; i < n_seg && i < 4; ++i)
    TL_REQUIRE(dst_stride[i] >= 0, "gather_rows_group: segment %d: negative member stride", i);
  return gather_launch(src, dst, dst_stride, src_rows, C, inner_bytes, chan, n_chan, n_seg, idx, idx_stride, n_idx, M, active, err,
                       stream);
}

extern "C" int tl_extract_windows(const void* src, int64_t C, int64_t T, int64_t ld_src, const int64_t* starts, int64_t n,
                                  int64_t L, int elem_bytes, void* dst, int32_t* err, void* stream) {
  TL_REQUIRE(n >= 0, "extract_windows: n must not be negative (got %lld)", (long long)n);
  TL_REQUIRE(C >= 1 && T >= 1 && L >= 1, "extract_windows: C, T and L must be positive (got %lld, %lld, %lld)", (long long)C,
             (long long)T, (long long)L);
  TL_REQUIRE(ld_src >= T, "extract_windows: row stride %lld shorter than the %lld samples of a row", (long long)ld_src,
             (long long)T);
  TL_REQUIRE(L <= T, "extract_windows: window length %lld exceeds the %lld samples of the recording", (long long)L,
             (long long)T);
  TL_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8,
             "extract_windows: elem_bytes must be 1, 2, 4 or 8 (got %d)", elem_bytes);
  if (n == 0) return TL_OK;
  TL_REQUIRE(src && starts && dst && err, "extract_windows: null src, starts, dst or error word");
  TL_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & (uintptr_t)(elem_bytes - 1)) == 0,
             "extract_windows: src and dst must be aligned to the %d bytes of an element", elem_bytes);
  TL_REQUIRE(((uintptr_t)starts & 7) == 0 && ((uintptr_t)err & 3) == 0, "extract_windows: misaligned starts or error word");
  TL_REQUIRE(L < (1LL << 30) && C < (1LL << 30) && n < (1LL << 31) && n * C < (1LL << 31),
             "extract_windows: L and C must be below 2^30 and n * C below 2^31 (got L %lld, C %lld, n %lld)", (long long)L,
             (long long)C, (long long)n);
  TL_REQUIRE(ld_src < (1LL << 40) && T < (1LL << 40), "extract_windows: T and ld_src must be below 2^40");
  window_args a;
  a.src = (const char*)src;
  a.dst = (char*)dst;
  a.C = C, a.T = T, a.ld_src = ld_src, a.L = L;
  a.total = (unsigned long long)(n * C) * (unsigned long long)L;   // < 2^61
  a.q256 = (unsigned)(256 / L), a.r256 = (unsigned)(256 % L);
  a.qC = (unsigned)(a.q256 / C), a.rC = (unsigned)(a.q256 % C);
  const unsigned long long blocks = (a.total + WINDOW_PER_BLOCK - 1) / WINDOW_PER_BLOCK;
  TL_REQUIRE(blocks < (1ULL << 31), "extract_windows: too many workgroups (%llu elements in one launch)", a.total);
  const dim3 grid((unsigned)blocks), block(256);
  const long long* st = (const long long*)starts;
  switch (elem_bytes) {
    case 1: hipLaunchKernelGGL(extract_windows_kernel<uint8_t>, grid, block, 0, (hipStream_t)stream, a, st, (int*)err); break;
    case 2: hipLaunchKernelGGL(extract_windows_kernel<uint16_t>, grid, block, 0, (hipStream_t)stream, a, st, (int*)err); break;
    case 4: hipLaunchKernelGGL(extract_windows_kernel<uint32_t>, grid, block, 0, (hipStream_t)stream, a, st, (int*)err); break;
    default: hipLaunchKernelGGL(extract_windows_kernel<uint64_t>, grid, block, 0, (hipStream_t)stream, a, st, (int*)err); break;
  }
  return check_launch("extract_windows");
}
