/* tonal_hip.h - C ABI of libtonal_hip.so (gfx950 / MI355X).
 *
 * The reference (Daniel-Lin-S/decode_tonal_langauge) is pure Python and has no FFI; every
 * arithmetic call on its hot path goes to torch / scipy.  This header
 * is therefore the boundary *we* define: each entry point names the reference call site
 * (file:line under /root/reference) whose arithmetic it replaces.  The Python mirror of the
 * reference's classes (decode_tonal_langauge_amd/models/..., preprocess/signal/...) binds these
 * with ctypes (decode_tonal_langauge_amd/_lib.py); INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - the caller owns every buffer, including workspaces; no entry point allocates, frees or
 *    synchronises; work is enqueued on `stream` (a hipStream_t passed as void*);
 *  - return 0 on success, a negative TL_E* code otherwise; tl_last_error() gives the
 *    thread-local message of the last failure;
 *  - fp32 unless stated; "rows" are flattened (sequence, time) rows of channels-last
 *    activations: row = seq * Tp + t, seq = b * C + c (data layout).
 */
#ifndef TONAL_HIP_H
#define TONAL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TL_OK 0
#define TL_EINVAL (-1)   /* bad argument / shape */
#define TL_ELAUNCH (-2)  /* hip launch failure   */
#define TL_ENODEV (-3)   /* no gfx950 device     */

const char* tl_last_error(void);
int tl_version(void);
/* number of visible HIP devices, or negative error (does not initialise a context) */
int tl_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Windowed NT GEMM  ("conv (k,1) as implicit GEMM", fp32 MFMA 32x32x2):
 *   acc[R][n] = sum_{j<J} sum_{k<K} Arow(R + j + row_shift)[k] * Bw[j][n][k]
 * Replaces nn.Conv2d((k,1)) + LeakyReLU + MaxPool2d((2,1)) forward and input-gradient
 * (models/synthesis_models.py:86-105,116-131), nn.Linear forward (:133-135), and the
 * h @ W_hh^T product of nn.LSTM (:112,164-166).
 *
 * loader: 0 DIRECT  A rows are read from `A` (row stride lda);
 *         1 UNPOOL  A rows are the un-pooled gradient dZ built on the fly from the pooled
 *                   gradient G (`A`, row stride lda) and the arg-max bits written by the
 *                   forward epilogue (`abits`, [prow][ld_abits] 32-bit words):
 *                   dZ[Rz][k] = G[Rz/2][k] if bit(Rz/2,k)==(Rz&1) and (Rz%Tp)<Tvalid_in else 0.
 * epilogue: 0 STORE  out[R][n] = acc (+bias[n]); with splitk>1 partial sums go to
 *                    out + z*slab_stride (no bias) and the caller reduces;
 *           1 LRELU  out[R][n] = lrelu(acc + bias[n]);
 *           2 POOL   out[R/2][n] = max over the row pair of lrelu(acc + bias[n]), 0 for rows
 *                    with (R%Tp) >= Tvalid; arg-max bit -> obits[R/2][n/32];
 *           3 MASK   out[R][n] = acc * (aux[R][n] > 0 ? 1 : slope)    (LeakyReLU backward)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* A; const uint32_t* abits; const float* Bw; const float* bias; const float* aux;
  float* out; uint32_t* obits;
  int64_t M;          /* output rows to compute                                   */
  int64_t A_rows;     /* rows addressable in A (G rows for UNPOOL)                */
  int N, K;           /* output columns, reduction length per tap (K % 4 == 0)    */
  int lda, ldb, ldo, ldaux, ld_abits, ld_obits;
  int J;              /* taps (1..7); Bw is [J][N][ldb]                           */
  int row_shift;      /* 0 forward, -(J-1) input-gradient                         */
  int Tp, Tvalid, Tvalid_in;
  float slope;
  int loader, epilogue;
  int splitk; int64_t slab_stride;
  int bm;             /* row-tile height: 256 (8 waves, large M), 128 (default) or 32 (skinny M) */
  /* tl_conv3_wino63v_nt, compact-M mode (in the four bytes that padded `bm`: no offset moves).  A stores a_hps_extra more
   * hexes per sequence than the launch computes: M, Tp and Tvalid describe the COMPUTED geometry (Tp / 6 = 16 hexes per
   * sequence: a lane owns one whole sequence, a 128-hex tile eight), hex c of a tile is read from storage hex
   * c + (c / 16) a_hps_extra and a tile's operand starts 8 (16 + a_hps_extra) hexes behind the one before;
   * A_rows >= ceil(M / 768) * 8 * (16 + a_hps_extra).  The trailing hexes of every sequence (padding behind the last
   * valid conv row) are never fetched or multiplied.  0: off.                                                          */
  int a_hps_extra;
  /* 1 bit per element, rows x ceil(cols/32) words like abits/obits: the POOL epilogue also writes
   * "pooled output > 0" to osign (leading dimension ld_obits, may be null); the MASK epilogue reads
   * its LeakyReLU' mask from auxbits (leading dimension ld_auxbits) instead of the floats in aux
   * when auxbits is not null - 1/32 of the bytes                                                   */
  uint32_t* osign; const uint32_t* auxbits; int ld_auxbits;
  /* epilogue 4 (Winograd input-gradient kernels only): the masked result is G1 = dL/dZ of the first
   * conv stage (C_in = 1, models/synthesis_models.py:87-89) at its arg-max; instead of storing it
   * the epilogue contracts it with the raw signal: c1partial[row tile][j][col] = sum_rows G1[row][col]
   * * x[seq][2t + a + j] (j < c1kt taps) and [c1kt][col] = sum_rows G1 (bias), with a = arg-max bit
   * in c1bits (leading dimension ld_auxbits), x = c1x (S, c1T), rows valid for t < Tvalid.          */
  const float* c1x; const uint32_t* c1bits; float* c1partial; int c1T, c1kt;
  /* epilogue 5 (tl_conv3_wino43v_nt only, round 4): POOL that also writes V = the F(4,3) input transform of its pooled
   * OUTPUT for the next 3-tap stage: vout[vout_quads][6][ld_vout], quad Q' = pooled rows 4Q' .. 4Q'+5 of one sequence
   * (Tp % 8 == 0).  `out` becomes optional (null: the raw pooled rows are never stored).  The last quad of every
   * 512-row tile needs two rows of the next tile: it is left raw (rows 0..3 in its transform slots 0..3) and the tile
   * stores its own first two pooled rows to vhalo[tile][2][N]; tl_wino43_v_fixup finishes those quads.                */
  float* vout; float* vhalo; int64_t vout_quads; int ld_vout;
  /* tl_conv3_wino63v_nt, POOL epilogue: rows per sequence of out / obits / osign, [seq * out_tp + t'] (pooled rows t' >=
   * out_tp are dropped); 0: Tp / 2.  Decouples the row stride of a stage's output from the hex padding of its input.   */
  int out_tp;
  /* tl_conv3_wino63v_nt, epilogue 6 (MASKY): the input gradient of a stage hands the stage BELOW its operands instead of the
   * gradient rows G: vout = Y[hex][8][ld_vout] (Y = A dz: the second operand of that stage's weight gradient,
   * tl_conv3_wino63v_tn with loader 3) and vout2 = Vd[hex][8][ld_vout] (the operand of its input gradient), both in the pair
   * layout, hexes of the stage below (three output rows each; vout_quads of them); dz = G un-pooled with abits (ld_abits),
   * zero from Tvalid_in conv rows on; `out` is not written.  The first hex of every 768-row tile is finished by
   * tl_wino63_vd_fixup from vhalo[tile][2][N].                                                                        */
  float* vout2;
  /* tl_conv7_wino63v_dgrad_nt: the LeakyReLU' mask of a stage input that did NOT come out of a pooling epilogue (no sign words):
   * its float rows mask[R][ld_mask] (> 0 ? 1 : slope); exactly one of auxbits / mask is given                            */
  const float* mask; int ld_mask;
} tl_nt_params;
int tl_gemm_nt_window(const tl_nt_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Windowed TN GEMM (weight gradients, reduction over rows):
 *   slab[z][j*Mj + m][n] = sum_{R in split z} A[R + j][m] * Bz[R][n]
 * with Bz = B (DIRECT, rows masked by (R%Tp)<Tvalid) or the un-pooled dZ (UNPOOL, as above).
 * Replaces the weight-gradient of Conv2d/Linear/LSTM produced by loss.backward()
 * (models/synthesis_trainer.py:226).  The caller sums the `splitk` slabs.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const float* A; const float* B; const uint32_t* bbits; float* slab;
  int64_t Krows;      /* reduction rows                                            */
  int64_t A_rows, B_rows;
  int Mdim, Ndim;     /* A columns used (per tap), B columns                       */
  int lda, ldb, ldc, ld_bbits;
  int J;              /* taps (1..7; 3: the all-taps kernel)                        */
  int Tp, Tvalid;
  int loader;
  int splitk; int64_t slab_stride;
  float* colsum;      /* optional.  tl_gemm_tn_window on its short-reduction kernel (Krows <= 512, splitk 1): colsum[m] = sum
                         over the rows of A[.][m], Mdim floats (the bias gradient of a Linear layer); tl_gemm_tn_window on its
                         one-tap direct kernel (J == 1, loader 0, Mdim > 32, Krows > 512): colsum[z][n] = sum over the valid
                         rows of split z of B[.][n], Ndim floats per split (the bias gradient of a 1x1 convolution, from the
                         launch that reads its output gradient anyway); tl_conv3_wino43v_tn / tl_conv3_wino63v_tn:
                         colsum[z][n] = sum over split z of the un-pooled
                         dZ column n (the bias gradient partial sums; Ndim floats per split), or null */
  float* vd; int ld_vd; /* optional (tl_conv3_wino43v_tn): also write Vd[quad][6][ld_vd] = the F(4,3) input transform of
                         the un-pooled dZ rows 4q-2 .. 4q+3 - the operand of the stage's input-gradient pass
                         (tl_conv3_wino43v_nt, MASK / conv1-weight-gradient epilogue); Krows / 4 quads, or null    */
  int part;           /* with vd: 0 both launches (the Vd-writing first C_in tile, then the other tiles), 1 / 2 only the
                         first / second of them (to put them on different streams)                                  */
  int bm;             /* tl_conv3_wino43v_tn: C_in tile, 0 = 128 when Mdim % 128 == 0 else 64; 64 / 128 force one   */
  int g_tp;           /* tl_conv3_wino63v_tn: rows per sequence of B / bbits, [seq * g_tp + t']; 0: Tp / 2           */
  int a_hex;          /* tl_conv3_wino63v_tn, loader 3: 0 or 1 - hex h of B meets hex h + a_hex of A (the third segment of a
                         7-tap weight gradient: rows shifted by 6 ARE the next hex; hexes past A_rows read as zero)     */
} tl_tn_params;
int tl_gemm_tn_window(const tl_tn_params* p, void* stream);

/* ------------------------------------------------------------------------------------------
 * Winograd F(4,3) on PRE-TRANSFORMED operands for the 3-tap convolutions that are followed by MaxPool (2,1)
 * (conv2, conv3: models/synthesis_models.py:91-97; their backward in loss.backward(),
 * models/synthesis_trainer.py:226): 6 channel contractions per 4 conv rows instead of 12.  The A/B partner of the
 * F(6,3) default below (TONAL_KERNELS wino=4); the in-loop-transform F(2,3) / F(4,3) generation of rounds 1-2 was
 * retired in round 6 (shapes neither V form covers run on the windowed GEMMs above).
 * Both the forward pass and the weight gradient of a stage consume the same V = B^T d of its input rows; on gfx950 the
 * fp32 MFMA shares the vector ALU's rate, so transform / staging instructions inside the GEMM kernels
 * displace matrix work one for one.  V[quad][6][ldv] (quad Q = input rows 4Q..4Q+5 of one sequence,
 * rows past the sequence taken as zero) is written once and the GEMM kernels are transform-free:
 *   tl_wino43_weights          w (O, I, 3, 1) -> forward taps fwd [6][O][ld_f] and input-gradient taps dgr [6][I][ld_d]
 *                              (flipped; either may be null)
 *   tl_wino43_input_transform  P (rows, C; whole sequences of Tp rows, Tp % 4 == 0) -> V (rows / 4 quads)
 *   tl_conv3_wino43v_nt        tl_gemm_nt_window's contract with J = 3, Bw = the 6 transformed taps [6][N][ldb], loader = 2:
 *                              A = V, lda = ldv, A_rows = quads held by V (>= M / 4); POOL / POOLV epilogue (forward) or
 *                              MASK / conv1-weight-gradient epilogue on Vd (input gradient, row_shift -2); K % 16 == 0;
 *                              M and Tp multiples of 4; both operands reach LDS by buffer_load .. lds
 *   tl_conv3_wino43v_tn        tl_gemm_tn_window's contract (UNPOOL) writing the 6 transform accumulators
 *                              slab[z][6][Mdim][ldc] (slab_stride >= 6*Mdim*ldc) with A = V (lda = ldv, A_rows = quads
 *                              held by V, a whole number of 8-quad K-steps: pad with zero quads); V by
 *                              LDS-DMA into a 4-slot ring, Y = A dy staged through registers; Mdim % 64 == 0
 *   tl_wino43_wgrad_finalize   red [6][I][ld] (slabs summed by the caller) -> dW (O, I, 3, 1)
 * tl_conv1_fwd_v (below) writes V of the first stage's output directly.
 * ------------------------------------------------------------------------------------------ */
int tl_wino43_weights(const float* w, float* fwd, float* dgr, int O, int I, int ld_f, int ld_d, void* stream);
int tl_wino43_wgrad_finalize(const float* red, float* gw, int O, int I, int ld, void* stream);
int tl_wino43_input_transform(const float* P, float* V, int64_t rows, int Tp, int C, int ldp, int ldv, void* stream);
int tl_conv3_wino43v_nt(const tl_nt_params* p, void* stream);
/* second half of epilogue 5: for every tile (64 output quads) of a tl_conv3_wino43v_nt launch that wrote V, the last quad
 * Q' = 64 t + 63 (if < quads): rows 0..3 from its slots 0..3, rows 4, 5 from vhalo[t + 1] - or zeros where the quad ends
 * its sequence (Tq = pooled rows per sequence) or is the last of the matrix - transformed in place.                     */
int tl_wino43_v_fixup(float* V, const float* vhalo, int64_t quads, int64_t tiles, int Tq, int C, int ldv, void* stream);
/* Vd[conv_rows / 4][6][ldv] of a pooled 3-tap stage from its output gradient G (g_rows pooled rows, ldg) and arg-max bits:
 * the F(4,3) input transform of the un-pooled dZ rows 4q-2 .. 4q+3 = the operand of tl_conv3_wino43v_nt with the MASK /
 * conv1-weight-gradient epilogue.  LDS-free and register-light: meant to run on a side stream beside the stage's
 * MFMA-bound weight-gradient kernel.                                                                                    */
int tl_wino43_unpool_transform(const float* G, const uint32_t* bits, float* V, int64_t conv_rows, int64_t g_rows, int Tp,
                               int Tvalid, int C, int ldg, int ld_bits, int ldv, void* stream);
int tl_conv3_wino43v_tn(const tl_tn_params* p, void* stream);
/* ------------------------------------------------------------------------------------------
 * Round 4 - Winograd F(6,3) on pre-transformed operands (csrc/tonal_wino63.hip): the same three passes of conv2 / conv3
 * (models/synthesis_models.py:91-97 and their backward in loss.backward(), models/synthesis_trainer.py:226) with HEXES:
 * 8 channel contractions per 6 conv rows (0.444 of the direct form's multiplies; F(4,3): 0.5).  Points 0, +-1, +-2,
 * +-1/2, inf (numerics: oracle/winograd_f63_gate.py).  A sequence holds Tp rows, Tp % 6 == 0 (% 12 where the pooled
 * output feeds another F(6,3) stage); V[hex][8][ldv], hex H of a sequence = its rows 6H .. 6H+7 (rows past the sequence
 * taken as zero), zero hexes appended to whole tiles (tl_wino63_nt_tile_rows() / 6 hexes; the callers of this package pad to
 * 128, a multiple of it); Vd the same of the un-pooled dZ rows 6H-2 .. 6H+5.
 *   tl_wino63_weights        w (O, I, 3, 1) -> forward taps [8][O][ld_f], input-gradient taps [8][I][ld_d] (flipped)
 *   tl_conv3_wino63v_nt      tl_conv3_wino43v_nt with A = V in hex form (loader 2, A_rows = hexes, whole tiles;
 *                            M % 6 == 0, K % 8 == 0, K >= 40, N % 32 == 0); epilogues POOL (+ out_tp), POOLV (vout in
 *                            hex form, vout_quads = hexes, Tp % 12 == 0), MASK, conv1-weight-gradient (4: row_shift -2 with
 *                            A = Vd and the flipped taps, row_shift 0 with A = Y and the taps of tl_wino63_weights_y), MASKY
 *                            (6: vout = Y of the stage below; vout2 = its Vd and vhalo together, or both NULL: Y only)
 *   tl_wino63_nt_tile_rows   conv rows of a row tile of tl_conv3_wino63v_nt (768: 128 hexes): vhalo holds 2 x C floats per row tile, c1partial one row per row tile, the fix-up passes
 *                            take tiles = ceil(M / that)
 *   tl_wino63_v_fixup        second half of POOLV: the last output hex of every row tile (rows 6, 7 from vhalo)
 *   tl_conv3_wino63v_tn      tl_conv3_wino43v_tn with hexes (Mdim % 128 == 0, Ndim % 64 == 0; slab[z][8][Mdim][ldc],
 *                            slab_stride >= 8*Mdim*ldc; B / bbits rows [seq * g_tp + t']); vd optional: Vd[hex][8][ld_vd].
 *                            loader 3: B = Y[hex][8][ldb] written by epilogue 6 of the stage above - no transform in the
 *                            kernel (Mdim % 256 == 0; colsum from Y plane 1)
 *   tl_wino63_wgrad_finalize red [8][I][ld] -> dW (O, I, 3, 1)
 *   tl_conv1_fwd_v6          tl_conv1_fwd_v writing V[S * Tp / 6][8][C1] (Tp % 6 == 0)
 * ------------------------------------------------------------------------------------------ */
int tl_wino63_weights(const float* w, float* fwd, float* dgr, int O, int I, int ld_f, int ld_d, void* stream);
/* taps of an input gradient that runs on Y = A dz (tl_conv3_wino63v_nt, epilogue 4 with row_shift 0): the un-flipped transform,
 * contracted over C_out, [ld_d / 8][8][I][8] - the layout of the flipped set of tl_wino63_weights                              */
int tl_wino63_weights_y(const float* w, float* dgy, int O, int I, int ld_d, void* stream);
int tl_conv3_wino63v_nt(const tl_nt_params* p, void* stream);
int tl_wino63_nt_tile_rows(void);
int tl_wino63_v_fixup(float* V, const float* vhalo, int64_t hexes, int64_t tiles, int Tq, int C, int ldv, void* stream);
int tl_conv3_wino63v_tn(const tl_tn_params* p, void* stream);
int tl_wino63_wgrad_finalize(const float* red, float* gw, int O, int I, int ld, void* stream);
/* second half of epilogue 6: the first hex of every row tile (tile rows / 3 hexes of the stage below) of a Vd written by it - its front row comes from
 * vhalo[tile - 1] (zero where the hex starts its sequence: hexes_per_seq)                                              */
int tl_wino63_vd_fixup(float* Vd, const float* vhalo, int64_t hexes, int64_t tiles, int hexes_per_seq, int C, int ldv, void* stream);
/* Y[conv_rows / 6][8][ldv] = A dz and Vd = B^T (dz rows 6h-2 .. 6h+5) of a pooled 3-tap stage from its output gradient G (rows
 * [seq * g_tp + t'], ldg) and arg-max bits, pair layout: the operands of tl_conv3_wino63v_tn (loader 3) and of the stage's input
 * gradient for a stage whose G comes from a kernel without epilogue 6 (HBM-bound; conv3 of the reference stack)             */
int tl_wino63_unpool_yvd(const float* G, const uint32_t* bits, float* Y, float* Vd, int64_t conv_rows, int64_t g_rows, int Tp,
                         int g_tp, int Tvalid, int C, int ldg, int ld_bits, int ldv, void* stream);
int tl_conv1_fwd_v6(const float* x, const float* w, const float* b, float* P, float* V, uint32_t* bits, uint32_t* sign,
                    int64_t S, int T, int ktaps, int C1, int Tp, int Tout, float slope, void* stream);
/* Round 5 - the CNN-RNN classifier's 7-tap (7,1) convolutions + LeakyReLU (models/deep_classifiers.py:250-256) on the F(6,3) NT
 * kernel: three 3-tap segments summed in the transform domain by ONE launch whose K loop runs over 3 K channels.
 *   tl_wino63_xform2     x rows [seq * Tp + t][C] -> V0 = B^T (rows 6h .. 6h+7), V1 = B^T (rows 6h+3 .. 6h+10), pair layout, rows
 *                        from Tvalid on taken as zero (segment 2 - rows 6h+6 .. 6h+13 - is V0 of hex h + 1: no third array)
 *   tl_wino63_weights7   w (O, I, taps = 7..9) -> taps [3 I / 8][8][O][8] (segment s = taps 3s .. 3s+2, missing ones zero)
 *   tl_conv7_wino63v_nt  A = V0, aux = V1 (A_rows hexes each, whole 128-hex tiles), Bw = the taps, K = I, ldb >= 3 K, J = 7..9,
 *                        loader 2, epilogue LRELU: out[R][n] = lrelu(conv + bias), R < M (M % 6 == 0).  Windows stop at the end
 *                        of their sequence EXCEPT in the last hex of a sequence (rows t >= Tp - 6), whose third segment is
 *                        the first hex of the next sequence: those rows are never valid outputs of a 7-tap convolution     */
int tl_wino63_xform2(const float* P, float* V0, float* V1, int64_t rows, int Tp, int Tvalid, int C, int ldp, int ldv, void* stream);
int tl_wino63_weights7(const float* w, float* fwd, int O, int I, int taps, void* stream);
int tl_conv7_wino63v_nt(const tl_nt_params* p, void* stream);
/* The backward of those 7-tap stages on the same kernels (TONAL_KERNELS conv7=wino63bwd).  dz = the gradient at the stage's
 * pre-activation, rows [seq * Tp + t], zero from t_out = t_in - 6 <= Tp - 6 on.
 *   weight gradient  dW_j = sum_R dz[R] (x) x[R + j]: segment s (taps 3s .. 3s+2) is a 3-tap F(6,3) weight gradient of x shifted by
 *                    3s rows - three tl_conv3_wino63v_tn launches with loader 3 on (V0(x), Y), (V1(x), Y) and (V0(x) with
 *                    a_hex = 1, Y), each followed by tl_wino63_wgrad_finalize; taps 7, 8 of the last one are dropped
 *   tl_wino63_ydz    dz rows (ldg) -> Y[rows / 6][8][ldv] = A dz (rows 6h .. 6h+5; rows from Tvalid on taken as zero), pair layout,
 *                    plane order of tl_wino63_unpool_yvd (plane 1 = the sum of the six rows: colsum stays the bias gradient)
 *   input gradient   dx[t] = sum_j W_j^T dz[t - j] = conv7_forward(dz moved DOWN six rows inside its sequence; taps flipped,
 *                    channels transposed)[t]: the moved rows still fit (t_out + 6 <= Tp), so no window leaves its sequence
 *   tl_wino63_xform2s  tl_wino63_xform2 of the rows moved down by `shift` (0 <= shift <= 6): row t of a sequence enters as row
 *                    t + shift, rows in front of it as zeros
 *   tl_conv7_wino63v_dgrad_nt  tl_conv7_wino63v_nt on those V0 / V1 with Bw = tl_wino63_weights7 of the flipped, transposed
 *                    weight (I, O, 7), epilogue MASK: out[R][n] = conv * (input > 0 ? 1 : slope), the sign of the stage input
 *                    from auxbits (sign words, ld_auxbits) or from its float rows `mask` (ld_mask) - exactly one of the two */
int tl_wino63_ydz(const float* G, float* Y, int64_t rows, int Tp, int Tvalid, int C, int ldg, int ldv, void* stream);
int tl_wino63_xform2s(const float* P, float* V0, float* V1, int64_t rows, int Tp, int Tvalid, int shift, int C, int ldp, int ldv,
                      void* stream);
int tl_conv7_wino63v_dgrad_nt(const tl_nt_params* p, void* stream);
/* Round 5 - the input gradient of a ONE-tap pooled stage whose input is the pooled output of a 3-tap F(6,3) stage (conv4 of the
 * reference stack: nn.Conv2d(512, 256, (1,1)) + LeakyReLU + MaxPool behind conv3, models/synthesis_models.py:96-101, backward in
 * loss.backward(), models/synthesis_trainer.py:226) on the F(6,3) NT kernel: its eight batched GEMMs take the six rows of a hex
 * (same taps W^T in each; two batches idle), so the accumulators are the gradient rows G of the stage below and the MASKY epilogue
 * (epilogue 7 = epilogue 6 without the inverse transform) writes that stage's Y / Vd directly - tl_wino63_unpool_yvd and the
 * gradient rows themselves go.  Row geometry: [seq * Tp + t], Tp % 3 == 0 rows per sequence = the hexes of the stage below
 * (three of its pooled rows each); hex H here = rows 6 H .. 6 H + 5 (may straddle two sequences).
 *   tl_wino63_unpool_rows6     G (the stage's pooled output gradient, rows [seq * g_tp + t / 2], ldg) + its arg-max bits ->
 *                              A[ceil(rows / 6)][8][lda], pair layout: slot i < 6 = un-pooled row 6 H + i (zero from Tvalid on),
 *                              slots 6, 7 zero (written only when pad != 0: a zero-filled buffer stays valid)
 *   tl_wino63_weights1         w (O, I) -> taps [ldb / 8][8][I][8]: slot t < 6 = w[o][n], slots 6, 7 zero
 *   tl_conv1_wino63v_dgrad_nt  A as above (A_rows hexes, whole 128-hex tiles), Bw = the taps, M = sequences x Tp rows, N = I,
 *                              K = O (K % 8 == 0, K >= 40), J = 1, loader 2, epilogue 7; auxbits / abits = sign / arg-max words
 *                              of the stage below in the layout [seq * out_tp + t] (out_tp <= Tp), Tvalid_in its valid conv
 *                              rows; vout / vout2 / vhalo / vout_quads / ld_vout as epilogue 6; then tl_wino63_vd_fixup       */
int tl_wino63_unpool_rows6(const float* G, const uint32_t* bits, float* A, int64_t rows, int64_t g_rows, int Tp, int g_tp, int Tvalid,
                           int C, int ldg, int ld_bits, int lda, int pad, void* stream);
int tl_wino63_weights1(const float* w, float* taps, int O, int I, int ldb, void* stream);
int tl_conv1_wino63v_dgrad_nt(const tl_nt_params* p, void* stream);
/* ------------------------------------------------------------------------------------------
 * RCCL handle (round 5; SURVEY 8b names it): the exchange step of the data-parallel trainer - between loss.backward() and
 * optimizer.step(), models/synthesis_trainer.py:226-227 - on plain fp32 device buffers.  One communicator per process (= per GPU);
 * rank 0 draws the id, the host side broadcasts its 128 bytes out of band (the Python host: through the torch.distributed store).
 * librccl is resolved at first use (the copy the process has loaded, else librccl.so.1): the library loads without it.
 *   tl_comm_unique_id   id128 <- ncclGetUniqueId
 *   tl_comm_init        *comm <- ncclCommInitRank(nranks, id, rank) on the current HIP device; tl_comm_destroy frees it
 *   tl_allreduce        recv[i] = op over ranks of send[i], i < count (op 0 sum, 1 max, 2 min; send == recv allowed)
 *   tl_reduce_scatter   recv[recv_count] = this rank's block of the sum over ranks of send[nranks * recv_count]
 *   tl_all_gather       recv[nranks * send_count] = the ranks' send[send_count] in rank order
 * all asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------ */
int tl_comm_unique_id(void* id128);
int tl_comm_init(void** comm, int rank, int nranks, const void* id128);
int tl_comm_destroy(void* comm);
int tl_allreduce(void* comm, const float* send, float* recv, int64_t count, int op, void* stream);
int tl_reduce_scatter(void* comm, const float* send, float* recv, int64_t recv_count, void* stream);
int tl_all_gather(void* comm, const float* send, float* recv, int64_t send_count, void* stream);
/* sizeof() of the two parameter structs as compiled into the library (binding self-check) */
int tl_sizeof_nt_params(void);
int tl_sizeof_tn_params(void);

/* ---- first conv stage, C_in = 1 (models/synthesis_models.py:87-89) ----------------------
 * x (S, T) -> P1 rows (S*Tp, C1) + arg-max bits (+ sign bits "P1 > 0", may be null); w (C1,3) b (C1). */
int tl_conv1_fwd(const float* x, const float* w, const float* b, float* P, uint32_t* bits, uint32_t* sign,
                 int64_t S, int T, int ktaps, int C1, int Tp, int Tout, float slope, void* stream);
/* the same stage writing V = the F(4,3) input transform of its pooled output (V[S * Tp / 4][6][C1], Tp % 4 == 0)
 * for tl_conv3_wino43v_nt / _tn of the next stage; P is optional (null: the raw pooled rows are never stored)     */
int tl_conv1_fwd_v(const float* x, const float* w, const float* b, float* P, float* V, uint32_t* bits, uint32_t* sign,
                   int64_t S, int T, int ktaps, int C1, int Tp, int Tout, float slope, void* stream);
/* its weight/bias gradient from G1 = dL/dZ at the arg-max: partial[nblk][(ktaps+1)*C1]      */
int tl_conv1_wgrad(const float* x, const float* G, const uint32_t* bits, float* partial,
                   int nblk, int64_t S, int T, int ktaps, int C1, int Tp, int Tout, void* stream);

/* nn.Dropout of the deep classifiers (models/deep_classifiers.py:81,258) in train mode, in place on a flat buffer:
 * x[i] = keep(seed, i) ? x[i] / (1 - p) : 0 with the counter-hash stream of tl_concat_pack (index = position i)   */
int tl_dropout_scale(float* x, int64_t n, float p, uint64_t seed, void* stream);
/* the same kernel on a slice of the buffer the mask is defined on: x[i] = keep(seed, index0 + i) ? x[i] / (1 - p) : 0.  A
 * data-parallel rank whose shard starts at row b0 of the global batch passes index0 = b0 * (elements per batch row) and draws
 * its rows of the single-process mask; index0 = 0 is tl_dropout_scale bit for bit.  index0 >= 0.                          */
int tl_dropout_scale_at(float* x, int64_t n, float p, uint64_t seed, int64_t index0, void* stream);

/* ---- small strided helpers --------------------------------------------------------------- */
/* dst[i0][i1][i2][i3] (contiguous) = sum_{z<nz} src[z*zs + i0*s0 + i1*s1 + i2*s2 + i3*s3];
 * elements whose i_d >= lim_d (source extents) read as 0. Used to pack torch-layout weights
 * into GEMM layouts and to reduce + unpack split-K weight-gradient slabs.                   */
int tl_permute_reduce(const float* src, float* dst, const int64_t dims[4], const int64_t strides[4],
                      const int64_t lims[4], int nz, int64_t zs, const float* bias_last, void* stream);
/* out[c] partial sums over valid rows: partial[nblk][ncols]; rows valid iff (r%Tp)<Tvalid   */
int tl_colsum(const float* G, float* partial, int nblk, int64_t rows, int ncols, int ld,
              int Tp, int Tvalid, void* stream);

/* ---- label LSTM (models/synthesis_models.py:112,164-167; :249-252,288-289) --------------- */
/* one time step, pointwise part: gates = hh + x_t W_ih^T + b_ih + b_hh -> (i,f,g,o), c, h.
 * hh (U, 4H) may be null for t = 0 (zero state).  act (U,4H) keeps the activated gates.     */
int tl_lstm_cell_fwd(const float* hh, const float* x_t, const float* w_ih, const float* b_ih,
                     const float* b_hh, const float* c_prev, float* act, float* c, float* h,
                     int U, int H, int in_dim, int ld_hh, void* stream);
/* dgates . W of the label LSTM on its U <= 8 distinct label rows as a pure stream of W (N x K, row stride ldw;
 * label_lstm.weight_hh_l0: 73 728 x 18 432 at the north-star shape) - torch's LSTM backward inside loss.backward(),
 * models/synthesis_trainer.py:226:  slab[b][u][k] = sum_{n in row block b} g[u][n] W[n][k]; ceil(N / rows_per_block) slabs of
 * U x K floats, summed by the caller (tl_permute_reduce); rows_per_block 8..1024; K % 4 == 0, 16-byte aligned W / slab.       */
int tl_lstm_gw(const float* g, const float* W, float* slab, int U, int64_t N, int K, int64_t ldg, int64_t ldw, int rows_per_block,
               void* stream);
/* inference-only sequence (models/deep_classifiers.py:230-233,294-296,316-318: the CNN-RNN classifier's two LSTMs, run
 * forward-only by the synthesis trainer): xp[u*xp_row_stride + t*4H + gate*H + k] = input projection + both biases of every
 * step, pre-computed by one GEMM (rows are (b, t): xp_row_stride = T*4H or more).
 * One fused launch per step (recurrent product + cell update; no split-K slabs): wp = the recurrent weight
 * packed unit-major (row 4 u + g = W_hh row g H + u), H % 8 == 0, h_a / h_b ping-pong state buffers (the
 * first step ignores both); *last_in_b tells which one holds h_T.                                        */
int tl_lstm_infer_seq_fused(const float* xp, int64_t xp_row_stride, const float* wp, float* h_a, float* h_b, float* c,
                            int B, int H, int T, int* last_in_b, void* stream);
/* backward of the same step: dh, dc_next -> dgates (U,4H) row-major and transposed (4H,ldt),
 * dc_prev.  c_prev may be null (t = 0).                                                     */
int tl_lstm_cell_bwd(const float* dh, const float* dh_rec, const float* dc_next, const float* act,
                     const float* c, const float* c_prev, float* dgates, float* dgates_t, float* dc_prev,
                     int U, int H, int ldt, void* stream);
/* dW_ih (4H,in_dim), db (4H) from dgates (L,U,4H) and x (L,U,in_dim)                        */
int tl_lstm_ih_grad(const float* dgates, const float* x, float* dw_ih, float* db, float* db2 /* optional second copy of db: bias_hh */,
                    int L, int U, int H, int in_dim, void* stream);

/* ---- concat / dropout glue (models/synthesis_models.py:107,160-170) ----------------------- */
/* Xc[row][0:Cc] = O5[row][0:Cc] * keep(row,ch); Xc[row][Cc+lc] = h[uid[b]][lc*lat*C + t*C + c];
 * remaining pad columns = 0.  keep = 1 if p_drop == 0 else Bernoulli via a counter hash of
 * (seed, (drop_row0 + row)*Cc + ch): drop_row0 = first row of this rank's shard in the GLOBAL
 * batch (b0*C*Tp), so a data-parallel run draws the masks of the single-process run.        */
int tl_concat_pack(const float* O5, const float* h, const int32_t* uid, float* Xc,
                   int B, int C, int Tp, int lat, int Cc, int Lc, int ld5, int ldh, int ldx,
                   float p_drop, uint64_t seed, int64_t drop_row0, void* stream);
/* backward: G5[row][ch] = dXc[row][ch]*keep*lrelu'(O5); dh[u][..] = sum_{b in u} dXc[..][Cc+lc], the members of u
 * taken from members[offsets[u] .. offsets[u+1]) - or, with members == NULL, by scanning offsets = the batch's label
 * ids (B entries) in batch order (the order a stable sort would give: same sums, nothing to prepare)              */
int tl_concat_unpack_bwd(const float* dXc, const float* O5, const int32_t* members, const int32_t* offsets,
                         float* G5, float* dh, int B, int U, int C, int Tp, int lat, int Cc, int Lc,
                         int ld5, int ldh, int ldx, float slope, float p_drop, uint64_t seed, int64_t drop_row0,
                         void* stream);

/* ---- loss / metric (models/synthesis_trainer.py:14-43,140,222-229) ------------------------ */
/* targets are truncated toward zero when trunc_targets != 0 (the reference's .long()).
 * dout (row stride ldd) = sign(out - t) / (B*D) * grad_scale; stats[0] += L1 mean,
 * stats[1] += MCD mean, stats[2], stats[3] = this call's L1 / MCD                            */
int tl_l1_mcd(const float* out, const float* targets, float* dout, float* stats,
              int B, int D, int ldd, int trunc_targets, float grad_scale, void* stream);

/* ---- NAdam (torch.optim.NAdam as built at models/synthesis_trainer.py:131-137) ------------ */
int tl_nadam(float* p, const float* g, float* m, float* v, int64_t n, float coef_grad, float coef_mom,
             float beta1, float beta2, float bias_corr2, float eps, float weight_decay, float grad_scale,
             void* stream);
/* One launch for a list of tensors sharing the step's scalars.  entries (DEVICE memory, count of them,
 * every pointer 16-byte aligned): block0 = first block of the tensor = sum over the tensors before it of
 * ceil(n / tl_nadam_multi_chunk()); total_blocks = that sum over all.  Same arithmetic as tl_nadam.   */
typedef struct { float* p; const float* g; float* m; float* v; int64_t n; int64_t block0; } tl_nadam_entry;
int tl_nadam_multi(const tl_nadam_entry* entries_dev, int count, int64_t total_blocks, float coef_grad, float coef_mom,
                   float beta1, float beta2, float bias_corr2, float eps, float weight_decay, float grad_scale,
                   void* stream);
int tl_nadam_multi_chunk(void);
/* tl_nadam_multi with the step's scalars (coef_grad, coef_mom, bias_corr2) read from device memory scalars_dev[0..2]: the
 * launch can be captured in a HIP graph and replayed with new values (models/synthesis_trainer.py:227, one optimizer.step
 * per batch)                                                                                                         */
/* scalars_dev[0..2] = (coef_grad, coef_mom, bias_corr2), *seed_dev = seed (either may be null): the values travel as
 * launch arguments, stream-ordered in front of a graph replay that reads them                                       */
int tl_set_step_scalars(float* scalars_dev, uint64_t* seed_dev, float coef_grad, float coef_mom, float bias_corr2,
                        uint64_t seed, void* stream);
/* dstA[i] = sum_{z < nz} srcA[z nA + i], dstB[j] = sum_z srcB[z nB + j] (nB may be 0): two slab reductions in one launch - the
 * per-window partials of a Conv1d's weight and bias gradient (SynthesisLite, models/synthesis_models.py:236-244)          */
int tl_sum_slabs2(const float* srcA, float* dstA, int64_t nA, const float* srcB, float* dstB, int64_t nB, int nz, void* stream);
/* tl_set_step_scalars plus the step's input tensors (n <= 4: host tables of device pointers and byte counts) copied into the
 * static buffers a captured step reads - all a replay needs in ONE launch (models/synthesis_trainer.py:201-205, the batch
 * tuple of the loop)                                                                                                    */
int tl_stage_step(float* scalars_dev, uint64_t* seed_dev, float coef_grad, float coef_mom, float bias_corr2, uint64_t seed,
                  const void* const* src, void* const* dst, const int64_t* nbytes, int n, void* stream);
/* A batch of up to four tensors gathered by one index vector in ONE launch (data_loading/resident.py: the device-resident
 * counterpart of the DataLoader's per-sample indexing + torch.stack).  Host tables of n_seg <= 4 entries, one per output
 * tensor ("segment"): src (N = src_rows[s] samples of C[s] rows of inner_bytes[s] bytes, contiguous), dst, and an optional
 * device list chan[s] of n_chan[s] int32 row numbers (chan[s] null: n_chan[s] = 0 and all C rows are taken in order).
 * idx: n_idx int64 sample numbers in device memory, shared by the segments.  For segment s, batch row b, output row j:
 *     dst[b][j][:] = src[idx[b]][chan ? chan[j] : j][:]          copied as bytes, any dtype; indices may repeat.
 * 16-byte accesses when the copy unit (a whole sample without a list, one row with one) and both bases are multiples of
 * 16 bytes, 4-byte ones when multiples of 4, bytes otherwise.  An idx[b] outside [0, src_rows) or a chan[j] outside [0, C)
 * is never dereferenced: bit 0 (index) or bit 1 (channel) of *err (device int32, never cleared here) is set and nothing is
 * written for that row.                                                                                              */
int tl_gather_rows(const void* const* src, void* const* dst, const int64_t* src_rows, const int64_t* C,
                   const int64_t* inner_bytes, const int32_t* const* chan, const int64_t* n_chan, int n_seg,
                   const int64_t* idx, int64_t n_idx, int32_t* err, void* stream);
/* ---- window extraction (data_loading/epoching.py): n windows of L samples cut from one (C, T) recording in ONE launch --------
 * src: C rows of T elements of elem_bytes (1, 2, 4 or 8) bytes each, row stride ld_src >= T elements.  starts: n int64 first
 * samples in device memory, read on the device (no host synchronisation).  dst: (n, C, L), contiguous:
 *     dst[i][c][j] = src[c * ld_src + starts[i] + j]               copied as bytes, any dtype; windows may overlap or repeat.
 * One element per access: nothing but elem_bytes alignment of src and dst is assumed, and only bytes that are copied are
 * read (lanes of a bad window, or past the end, read src[0]).  A window with starts[i] < 0 or starts[i] + L > T is never
 * dereferenced: bit 1 (value 2) of *err (device int32, never cleared here) is set, its (C, L) destination is left as it was,
 * and every other window of the launch is copied.  All offsets are 64-bit: src and dst may exceed 4 GiB.
 * Limits: L <= T, L and C below 2^30, n * C below 2^31.  n = 0 returns TL_OK without a launch.                            */
int tl_extract_windows(const void* src, int64_t C, int64_t T, int64_t ld_src, const int64_t* starts, int64_t n, int64_t L,
                       int elem_bytes, void* dst, int32_t* err, void* stream);
/* ---- group launches: M models of equal shape ("members") trained side by side (_classifier_ensemble_engine.py) -----------
 * Every tl_*_group entry is its single-model neighbour with a member dimension on the grid: member m works on pointers
 * s_* ELEMENTS (of the pointer's type, unless stated otherwise) behind the ones given, which are member 0's.  It is the SAME
 * kernel - the single entry launches it with M = 1 - so a member's outputs have the bits of the single launch on the same
 * inputs.  `active` (M device int32 words, may be null = all): the workgroups of a member whose word is 0 return before their
 * first load and write nothing - no parameter, moment, statistics word or output.  1 <= M <= 65535.  Where the single entry
 * wants a pointer 16-byte aligned, the member stride must be a multiple of 16 bytes; the strides of everything a member
 * writes must cover its extent (members never share an output).  Every other check is the single entry's.
 *
 * tl_gather_rows with M index vectors over the one dataset: idx is an (M, idx_stride) int64 table and member m's batch is
 * rows idx[m][0 .. n_idx) (pass idx + start, as with the single entry), written dst_stride[s] BYTES behind member 0's
 * destination of segment s: x as (M, B, ...), y as (M, B).  The access width also has to divide dst_stride[s].  One error word,
 * ORed into as by the single entry.                                                                                       */
int tl_gather_rows_group(const void* const* src, void* const* dst, const int64_t* dst_stride, const int64_t* src_rows,
                         const int64_t* C, const int64_t* inner_bytes, const int32_t* const* chan, const int64_t* n_chan,
                         int n_seg, const int64_t* idx, int64_t idx_stride, int64_t n_idx, int M, const int32_t* active,
                         int32_t* err, void* stream);
/* tl_nadam on M tensors of n elements each: p, m, v at member stride s_p, g at s_g (multiples of 4; a bias row of N floats is
 * therefore stored at row stride 4 ceil(N / 4))                                                                            */
int tl_nadam_group(float* p, const float* g, float* m, float* v, int M, int64_t n, int64_t s_p, int64_t s_g, float coef_grad,
                   float coef_mom, float beta1, float beta2, float bias_corr2, float eps, float weight_decay, float grad_scale,
                   const int32_t* active, void* stream);
int tl_nadam_multi_dev(const tl_nadam_entry* entries_dev, int count, int64_t total_blocks, const float* scalars_dev,
                       float beta1, float beta2, float eps, float weight_decay, float grad_scale, void* stream);
/* the same update for a parameter (rows x cols) whose gradient is low rank, g = fa^T . fb with
 * fa (kr, rows), fb (kr, cols), kr <= 64: the gradient is formed in registers and never stored
 * (label_lstm.weight_hh_l0: 5.4 GB less written and read per step).                              */
int tl_nadam_lowrank(float* p, float* m, float* v, const float* fa, const float* fb, int kr, int rows, int cols,
                     int ldfa, int ldfb, float coef_grad, float coef_mom, float beta1, float beta2,
                     float bias_corr2, float eps, float weight_decay, float grad_scale, void* stream);
/* ... for M members (see the group launches above): grid (row tiles, column tiles, M); p, m, v at member stride s_p, the
 * factors at s_fa (a member's dlogits, B x ldfa) and s_fb (a member's batch rows, B x ldfb); s_p and s_fb multiples of 4   */
int tl_nadam_lowrank_group(float* p, float* m, float* v, const float* fa, const float* fb, int M, int kr, int rows, int cols,
                           int ldfa, int ldfb, int64_t s_p, int64_t s_fa, int64_t s_fb, float coef_grad, float coef_mom,
                           float beta1, float beta2, float bias_corr2, float eps, float weight_decay, float grad_scale,
                           const int32_t* active, void* stream);
/* ... and, in the same pass over p, dh = fa[0:U] . p_OLD (U x cols): the last step of the label LSTM's BPTT
 * (dh_1 = dgates_2 . W_hh reads the weight as it was BEFORE this update, and the W_hh gradient has no term for the first step,
 * so the update does not wait for it; torch's LSTM backward inside loss.backward(), models/synthesis_trainer.py:226, followed by
 * optimizer.step(), :227).  Rows 0..U-1 of fa must be the dgates of that step (U <= 8, U <= kr).  The kernel writes
 * ceil(rows / (32 row_tiles)) partial slabs dh_slab[slab][U][cols] (caller-owned, 16-byte aligned); their sum over `slab`
 * (tl_permute_reduce) is dh.  One 5.4 GB stream of W_hh less per train step.                                                 */
int tl_nadam_lowrank_dh(float* p, float* m, float* v, const float* fa, const float* fb, int kr, int rows, int cols,
                        int ldfa, int ldfb, float coef_grad, float coef_mom, float beta1, float beta2,
                        float bias_corr2, float eps, float weight_decay, float grad_scale, float* dh_slab, int U,
                        int row_tiles, void* stream);

/* ---- tone dynamics gather (data_loading/utils.py:32-79) ----------------------------------- */
/* labels[b][0][l] = syl[b]; labels[b][1][l] = table[tone[b]][l]; err flag set if tone out of range */
int tl_tone_dynamics(const int64_t* tone, const int64_t* syl, const float* table, float* labels,
                     int32_t* err, int B, int n_tones, int L, void* stream);
/* out[i] = LeakyReLU(sum_z slab[z][i] + bias[i % ncols]), i < n: split-K reduction + bias + activation of a Linear layer
 * (models/synthesis_models.py:252-256, fc.1 of SynthesisLite)                                                       */
int tl_splitk_bias_lrelu(const float* slab, const float* bias, float* out, int nz, int64_t n, int ncols, float slope, void* stream);
/* out (B, N) = x (B, K; row stride ldx) . w (N, K)^T + bias (N, may be NULL): the Linear layer of LogisticRegressionClassifier
 * on the flattened window (models/simple_classifiers.py:34-60) and the output layer of ShallowNNClassifier (:112-121) - a
 * handful of columns over a long K, where a GEMM tile would be empty.  act = 1 applies the sigmoid the deep classifiers end
 * with (models/deep_classifiers.py:97-99,265-267).  N <= 64, K % 4 == 0, 16-byte aligned rows.                        */
int tl_linear_rows(const float* x, const float* w, const float* bias, float* out, int B, int K, int N, int64_t ldx, int act,
                   void* stream);
/* ... for M members (see the group launches above): grid (B, M); x (M, B, K), w (M, N, K), bias and out at the member strides
 * s_x, s_w, s_bias, s_out; s_x and s_w multiples of 4                                                                      */
int tl_linear_rows_group(const float* x, const float* w, const float* bias, float* out, int M, int B, int K, int N, int64_t ldx,
                         int act, int64_t s_x, int64_t s_w, int64_t s_bias, int64_t s_out, const int32_t* active, void* stream);
/* the whole label pass of a train step (models/synthesis_trainer.py:207-218) in one launch: tone = argmax of tone_scores
 * (B, n_tone_cls), syl = argmax of syl_scores (B, n_syl_cls) (first maximum), the gather of tl_tone_dynamics (n_rows table
 * rows) and, if pair is given, pair[b] = tone * n_syl + syl                                                        */
int tl_labels_from_scores(const float* tone_scores, const float* syl_scores, const float* table, float* labels, int64_t* tone,
                          int64_t* syl, int32_t* pair, int32_t* err, int B, int n_tone_cls, int n_syl_cls, int n_rows, int n_syl,
                          int L, void* stream);

/* ---- classifier training (models/classifier_trainer.py:72-89: nn.CrossEntropyLoss, loss.backward(), the confusion matrix) ---- */
/* softmax cross-entropy of logits (B, N; row stride ldl >= N), 1 <= N <= 64, against labels (B) int64, and its statistics.
 * Optional outputs (null to skip):
 *   dlogits[b][n] = (softmax(logits[b])[n] - [n == labels[b]]) * grad_scale at row stride ldd, N <= ldd <= 64; columns
 *                   N .. ldd - 1 are written as zeros (pad to a multiple of 4 and the rows are GEMM operands); pass
 *                   grad_scale = 1 / B for the mean loss
 *   dbias[n]      = sum over b of dlogits[b][n]
 *   pred[b]       = arg-max of the row by torch's rule (first maximum, a NaN counts as the maximum), int64
 * Accumulating outputs - ADDED to, so a caller zeroes them once per epoch and reads them once per epoch:
 *   loss_sum      += sum over b of logsumexp(logits[b]) - logits[b][labels[b]]  (fp64; the row maximum is subtracted first)
 *   count         += rows counted (int64);  confusion[t][p] += 1, (N, N) int64, row = true class
 * A label outside [0, N) sets *err = 1 and contributes nothing (its dlogits row is zero).  The same inputs give the same
 * bits of every output on every run (one workgroup walks the rows; the sums have a fixed order).
 * labels = null: only pred is written (loss_sum, count, confusion and err are not touched and may be null).               */
int tl_ce_loss(const float* logits, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred, double* loss_sum,
               int64_t* count, int64_t* confusion, int32_t* err, int B, int N, int ldl, int ldd, float grad_scale, void* stream);
/* ... for M members (see the group launches above): one 16-wave workgroup per member, so each member's sums keep the fixed
 * order of the single launch.  s_stats is the member stride of loss_sum, count, confusion AND err alike, in 8-byte words (the
 * engine keeps M x (3 + N N) int64 words: loss, count, err, confusion); dbias and pred are rows per member.                  */
int tl_ce_loss_group(const float* logits, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred, double* loss_sum,
                     int64_t* count, int64_t* confusion, int32_t* err, int M, int B, int N, int ldl, int ldd, float grad_scale,
                     int64_t s_logits, int64_t s_labels, int64_t s_dlogits, int64_t s_dbias, int64_t s_pred, int64_t s_stats,
                     const int32_t* active, void* stream);
/* the same step for the deep classifiers, whose forward ends in a sigmoid and whose trainer applies nn.CrossEntropyLoss to those
 * sigmoid outputs (models/deep_classifiers.py:97-99 under models/classifier_trainer.py:72-89): `scores` (B, N) are the fp32
 * s = sigmoid(z) exactly as tl_linear_rows(act = 1) writes them, the loss is CE(s), and
 *   dlogits[b][n] = (softmax(s[b])[n] - [n == labels[b]]) * s (1 - s) * grad_scale
 * is the gradient with respect to the PRE-sigmoid z - what tl_head_bwd takes; s (1 - s) is formed from the stored score, so a
 * score saturated at 0.0f or 1.0f gives exactly 0.  dbias, pred (arg-max of the scores), the accumulating statistics, the
 * label check, the fixed summation order and the argument checks are tl_ce_loss's.                                        */
int tl_ce_scores_loss(const float* scores, const int64_t* labels, float* dlogits, float* dbias, int64_t* pred, double* loss_sum,
                      int64_t* count, int64_t* confusion, int32_t* err, int B, int N, int ldl, int ldd, float grad_scale,
                      void* stream);
/* backward of a head layer z = h W^T + b with N <= 64 outputs over K inputs (K % 4 == 0), in one pass over its input:
 * dlogits (B, N; row stride ldd), h (B, K) the layer's input, W (N, K).  Optional outputs (null to skip; each has the same
 * bits whichever of the others are asked for):
 *   dh[b][k]   = (sum_n dlogits[b][n] W[n][k]) * act'(h[b][k])   (B, K), act' of the layer BELOW read off its stored output
 *                h: act 0 none (1), 1 ReLU (h > 0), 2 LeakyReLU (h > 0 ? 1 : slope) - the sign of the output is the sign of
 *                the pre-activation
 *   dbias_h[k] = sum_b dh[b][k]   (K)
 *   dw[n][k]   = sum_b dlogits[b][n] h[b][k]   (N, K)
 * All sums over b are taken in row order by the thread that owns the column: deterministic.  h, W and the outputs 16-byte
 * aligned.  With dh null and h = x this is the weight gradient of LogisticRegressionClassifier's layer.                    */
int tl_head_bwd(const float* dlogits, const float* h, const float* W, float* dh, float* dbias_h, float* dw, int B, int K, int N,
                int ldd, int act, float slope, void* stream);
/* ... for M members (see the group launches above; the output layer of ShallowNNClassifier): grid (column blocks, M), any subset
 * of dh, dbias_h, dw, act 0 / 1 / 2; the strides of h, W, dh, dbias_h and dw non-negative multiples of 4, and with M > 1 those of
 * the outputs asked for at least a member's B K, K and N K elements                                                        */
int tl_head_bwd_act_group(const float* dlogits, const float* h, const float* W, float* dh, float* dbias_h, float* dw, int M, int B,
                          int K, int N, int ldd, int act, float slope, int64_t s_dlogits, int64_t s_h, int64_t s_W, int64_t s_dh,
                          int64_t s_dbias_h, int64_t s_dw, const int32_t* active, void* stream);
/* ... and its dw-only form (the dense route of the logistic group): tl_head_bwd_act_group with dh = dbias_h = NULL and act 0,
 * dw[m] = dlogits[m]^T . h[m]                                                                                               */
int tl_head_bwd_group(const float* dlogits, const float* h, const float* W, float* dw, int M, int B, int K, int N, int ldd,
                      int64_t s_dlogits, int64_t s_h, int64_t s_W, int64_t s_dw, const int32_t* active, void* stream);
/* tl_gemm_nt_window for M members (the hidden layer of ShallowNNClassifier): *p describes member 0; member m works on A + m s_A,
 * Bw + m s_Bw, bias + m s_bias and out + m s_out (elements).  Only the plain GEMM with bias and LeakyReLU has a group form:
 * J = 1, loader DIRECT, row_shift 0, splitk <= 1, bm 0 or 128, epilogue LRELU (ReLU is slope 0), bias given, and none of aux /
 * auxbits / abits / obits / osign / vout* / vhalo / c1* / mask; everything else is refused.  s_A and s_Bw non-negative multiples
 * of 4, s_bias non-negative, s_out >= p->M * ldo when M > 1.  The kernel is chosen as tl_gemm_nt_window chooses it for *p
 * (direct-to-LDS when K % 16 == 0, in its 64-column form for N <= 64, else register-staged) and runs that kernel's body with
 * the member on grid.z, so a member's out has the bits of the single launch.                                                */
int tl_gemm_nt_window_group(const tl_nt_params* p, int M, int64_t s_A, int64_t s_Bw, int64_t s_bias, int64_t s_out,
                            const int32_t* active, void* stream);
/* A second group form of tl_gemm_nt_window, for the Linear layers of SynthesisLite and their input gradients
 * (_lite_ensemble_engine.py): J = 1, loader DIRECT, row_shift 0, bm 32 or 128, and
 *   epilogue STORE, bias optional, split-K on grid.y as in the single launch: member m's slab z is out + m s_out + z slab_stride,
 *                  so slab_stride >= p->M * ldo and, with M > 1, s_out >= splitk * slab_stride (s_out >= p->M * ldo without split-K);
 *   epilogue MASK  with aux (never auxbits) at the member stride s_aux.
 * Everything else is refused.  s_A and s_Bw non-negative multiples of 4, s_bias and s_aux non-negative.  The kernel is chosen as
 * tl_gemm_nt_window chooses it for *p and runs that kernel's body with the member on grid.z.                                 */
int tl_gemm_nt_window_group_fc(const tl_nt_params* p, int M, int64_t s_A, int64_t s_Bw, int64_t s_bias, int64_t s_aux,
                               int64_t s_out, const int32_t* active, void* stream);
/* tl_gemm_tn_window for M members, for the parameters the single entry runs on its short-reduction kernel only: J = 1, loader
 * DIRECT, Krows <= 512, splitk <= 8, Mdim * Ndim <= 2^20, ldc % 4 == 0 (and slab_stride >= Mdim * ldc under split-K); Tp / Tvalid
 * masking and the optional colsum (written without split-K, as by the single launch) included; bbits and vd null.  Member m works
 * on A + m s_A, B + m s_B, slab + m s_slab and colsum + m s_colsum: s_A, s_B, s_slab non-negative multiples of 4, and with M > 1
 * s_slab >= splitk * slab_stride (>= Mdim * ldc without split-K), s_colsum >= Mdim.  Everything else is refused.  The member sits
 * on grid.z and runs the single kernel's body.                                                                            */
int tl_gemm_tn_window_group(const tl_tn_params* p, int M, int64_t s_A, int64_t s_B, int64_t s_slab, int64_t s_colsum,
                            const int32_t* active, void* stream);

/* ---- group forms of the SynthesisLite step (see the group launches above; _lite_ensemble_engine.py) ------------------------
 * Each is its single neighbour's kernel with the member on the grid (grid.z of the tl_lite_* kernels, grid.y of the four
 * one-dimensional ones); the arguments are the single entry's, then M where stated, the member strides in ELEMENTS of the
 * pointer they move, `active` and the stream.  A stride shared by several pointers is named once:
 *   s_stat  mean and rstd            s_run  running_mean and running_var     s_gb   gamma and beta (BatchNorm weight / bias)
 *   s_dgb   dgamma and dbeta         s_b    bias_ih and bias_hh              s_cs   cs and hs       s_act  act (and dgates)
 *   s_db    db and db2
 * The stride of every pointer a member writes must cover the member's extent when M > 1 (TL_EINVAL otherwise); strides of inputs
 * are non-negative (0 shares one input among the members).                                                                */
int tl_lite_conv_fwd_group(const float* x, const float* w, const float* bias, float* z, float* part, int M, int B, int Cin,
                           int Cout, int T, int k, int pad, int64_t s_x, int64_t s_w, int64_t s_bias, int64_t s_z,
                           int64_t s_part, const int32_t* active, void* stream);
/* every member has its own mean / rstd, running statistics and num_batches_tracked word (s_tracked, int64 words)              */
int tl_lite_bn_finalize_group(const float* part, float* mean, float* rstd, float* run_mean, float* run_var, int M, int nparts,
                              int C, int64_t count, int T, float momentum, float eps, int training, int64_t* tracked,
                              int64_t s_part, int64_t s_stat, int64_t s_run, int64_t s_tracked, const int32_t* active,
                              void* stream);
int tl_lite_bn_act_pool_fwd_group(const float* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                  float* y, int M, int B, int C, int T, float slope, int64_t s_z, int64_t s_stat, int64_t s_gb,
                                  int64_t s_y, const int32_t* active, void* stream);
/* work: B * C * 2 floats per member at s_work                                                                                 */
int tl_lite_bn_act_pool_bwd_group(const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma,
                                  const float* beta, float* dz, float* dgamma, float* dbeta, float* work, int M, int B, int C,
                                  int T, float slope, int training, int64_t s_dy, int64_t s_z, int64_t s_stat, int64_t s_gb,
                                  int64_t s_dz, int64_t s_dgb, int64_t s_work, const int32_t* active, void* stream);
int tl_lite_conv_bwd_group(const float* dz, const float* x, const float* w, float* dx, float* dwpart, float* dbpart, int M, int B,
                           int Cin, int Cout, int T, int k, int pad, int64_t s_dz, int64_t s_x, int64_t s_w, int64_t s_dx,
                           int64_t s_dwpart, int64_t s_dbpart, const int32_t* active, void* stream);
/* tl_colsum per member: partial (nblk, ncols) per member at s_part, G at s_G (multiples of 4)                                 */
int tl_colsum_group(const float* G, float* partial, int nblk, int64_t rows, int ncols, int ld, int Tp, int Tvalid, int M,
                    int64_t s_G, int64_t s_part, const int32_t* active, void* stream);
int tl_sum_slabs2_group(const float* srcA, float* dstA, int64_t nA, const float* srcB, float* dstB, int64_t nB, int nz, int M,
                        int64_t s_srcA, int64_t s_dstA, int64_t s_srcB, int64_t s_dstB, const int32_t* active, void* stream);
int tl_lite_lstm_fwd_group(const float* xl, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* act,
                           float* cs, float* hs, int M, int B, int L, int H, int in_dim, int64_t s_xl, int64_t s_wih,
                           int64_t s_whh, int64_t s_b, int64_t s_act, int64_t s_cs, const int32_t* active, void* stream);
/* dgates lies at the stride of act (the two have one shape)                                                                   */
int tl_lite_lstm_bwd_group(const float* dh_last, const float* w_hh, const float* act, const float* cs, float* dgates, int M, int B,
                           int L, int H, int ld_dh, int64_t s_dh, int64_t s_whh, int64_t s_act, int64_t s_cs,
                           const int32_t* active, void* stream);
int tl_lstm_ih_grad_group(const float* dgates, const float* x, float* dw_ih, float* db, float* db2, int M, int L, int U, int H,
                          int in_dim, int64_t s_dg, int64_t s_x, int64_t s_dw, int64_t s_db, const int32_t* active, void* stream);
/* the dropout seed always comes from device memory: seed_dev is a table of M words and member m draws the mask
 * tl_lite_cat_dev / tl_lite_uncat_dev draw with seed_dev[m]                                                                   */
int tl_lite_cat_group(const float* y2, const float* hs, float* feat, int M, int B, int F, int H, int L, int ldf, float p_drop,
                      const uint64_t* seed_dev, int64_t s_y2, int64_t s_hs, int64_t s_feat, const int32_t* active, void* stream);
int tl_lite_uncat_group(const float* dfeat, float* dy2, float* dh, int M, int B, int F, int H, int ldf, float p_drop,
                        const uint64_t* seed_dev, int64_t s_dfeat, int64_t s_dy2, int64_t s_dh, const int32_t* active,
                        void* stream);
/* zs: elements between two split-K slabs of one member (>= n): n for [M][nz][n] slabs (s_slab = nz n), M n for [nz][M][n]
 * (s_slab = n); bias (may be null) at s_bias                                                                                 */
int tl_splitk_bias_lrelu_group(const float* slab, const float* bias, float* out, int nz, int64_t n, int ncols, float slope, int M,
                               int64_t zs, int64_t s_slab, int64_t s_bias, int64_t s_out, const int32_t* active, void* stream);
/* stats is (M, 4); one workgroup per member, so each member's sums keep the single launch's order                             */
int tl_l1_mcd_group(const float* out, const float* targets, float* dout, float* stats, int M, int B, int D, int ldd,
                    int trunc_targets, float grad_scale, int64_t s_out, int64_t s_tgt, int64_t s_dout, const int32_t* active,
                    void* stream);

/* ---- training of CNNRNNClassifier (models/deep_classifiers.py:158-343 under models/classifier_trainer.py:72-89) ----------
 * The LSTM pair keeps ROWS TIME-MAJOR (row = t * B + b), so the kept arrays are directly the (T B)-row operands of the
 * weight-gradient GEMMs (tl_gemm_tn_window): dW_hh = dgates[1:]^T . hs[:-1] (a row offset of B between the operands),
 * dW_ih = dgates^T . x, db = column sums of dgates, dX = dgates . W_ih as the TN GEMM with A = dgates_t.  H is the hidden
 * width padded to a multiple of 8; a padded unit (zero weight rows / columns and bias) keeps c = h = 0.
 *   tl_lstm_train_seq   all T steps, one fused launch per step (the tiling of tl_lstm_infer_seq_fused: 32 batch rows x 8 units
 *                       per workgroup, 8 K slices).  xp[b * xp_row_stride + t * xp_step_stride + gate * H + u] = input projection
 *                       + both biases; wp = W_hh packed unit-major (row 4 u + g = W_hh row g H + u), (4 H, H).  Step t reads
 *                       hs[t-1], cs[t-1] (zero state at t = 0) and writes hs[t], cs[t] (T, B, H) and the activated gates
 *                       act[t] (T, B, 4 H; columns gate * H + u, gates i, f, g, o).  Rows beyond B are clamped for loads and never
 *                       stored.
 *   tl_lstm_bptt_seq    steps t = T-1 .. 0, one fused launch per step: dh_t = [t == T-1] dh_last (B, H) + dgates_{t+1} . W_hh on
 *                       the matrix cores (whT = W_hh^T (H, 4 H), row u contiguous over the gate rows g H + u'), then the cell
 *                       backward of tl_lstm_cell_bwd per (row, unit); dc (B, H) is scratch carried in place (need not be
 *                       initialised); dgates (T, B, 4 H) row-major; dgates_t optional: (4 H, ldt) with column t * B + b,
 *                       ldt >= T * B.  No atomics: the same inputs give the same bits.  Pad units come out exactly zero when
 *                       dh_last's pad columns are zero.                                                                       */
int tl_lstm_train_seq(const float* xp, int64_t xp_row_stride, int64_t xp_step_stride, const float* wp, float* hs, float* cs,
                      float* act, int B, int H, int T, void* stream);
int tl_lstm_bptt_seq(const float* whT, const float* dh_last, const float* act, const float* cs, float* dc, float* dgates,
                     float* dgates_t, int64_t ldt, int B, int H, int T, void* stream);
/* MaxPool2d((3,1)) + Dropout behind the un-pooled last conv stage (:256-258) and the reference's raw view of the result as the
 * second LSTM's input (:309-315).  Y rows [seq * Tp + t][ldy] (post-activation), sequences branch-major: B * w1 LSTM-branch
 * columns (seq = b * w1 + j), then B * Cn electrode columns.  Element (b, ch, s, w) of the contiguous (B, C, tq, W = w1 + Cn)
 * activation, w in torch.cat((x1, x), dim=3) order, has offset f = (ch * tq + s) * W + w in its batch element and lands in
 * X[(b * rs_b + (f / (C W)) * rs_t) * C W + f % (C W)]: rs_b = tq, rs_t = 1 is the reference's (B tq, C W) matrix, rs_b = 1,
 * rs_t = B its time-major form.  keep = tl_dropout_scale's decision at position (seq * tq + s) * C + ch (p = 0: none).
 *   tl_pool3_fwd   X = first maximum of rows 3 s .. 3 s + 2, times keep / (1 - p)
 *   tl_pool3_bwd   dZ[seq * Tp + 3 s + arg][ch] = dX * keep / (1 - p) * (Y[arg] > 0 ? 1 : slope) with the arg-max recomputed
 *                  from Y (torch's rule: the first maximum); the other two rows of the triple, rows t >= 3 tq and the pad rows of
 *                  every sequence are written as zeros (all Tp rows, C columns of dZ, row stride lddz)                        */
int tl_pool3_fwd(const float* Y, float* X, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int64_t rs_b, int64_t rs_t, float p,
                 uint64_t seed, void* stream);
int tl_pool3_bwd(const float* Y, const float* dX, float* dZ, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int lddz,
                 int64_t rs_b, int64_t rs_t, float p, uint64_t seed, float slope, void* stream);
/* the same two kernels on rows [b0, b0 + B) of a global batch of B_global (data-parallel shard): Y / X / dX / dZ are this rank's
 * (local addressing, B local rows); only the keep position changes - seq becomes the sequence's number in the GLOBAL batch's
 * branch-major order, (b0 + b) * w1 + j for an LSTM-branch column and B_global * w1 + (b0 + b) * Cn + e for an electrode column.
 * b0 = 0, B_global = B are tl_pool3_fwd / tl_pool3_bwd bit for bit.  0 <= b0, b0 + B <= B_global.                           */
int tl_pool3_fwd_shard(const float* Y, float* X, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int64_t rs_b, int64_t rs_t,
                       float p, uint64_t seed, int b0, int B_global, void* stream);
int tl_pool3_bwd_shard(const float* Y, const float* dX, float* dZ, int B, int w1, int Cn, int C, int Tp, int tq, int ldy, int lddz,
                       int64_t rs_b, int64_t rs_t, float p, uint64_t seed, float slope, int b0, int B_global, void* stream);
/* input gradient of the first conv stage (C_in = 1) from G1 = dL/dZ at the arg-max (rows [seq * Tp + t][C1], C1 = 1024),
 * its arg-max bits and w (C1, ktaps = 7: the one shape built): dx[seq][u] = sum over the (t, j) with 2 t + a + j = u of sum_c G1[t][c] w[c][j];
 * every sample u < T is written (zero where nothing reaches it) to dx[(seq / n_inner) * stride_outer + u * stride_t +
 * (seq % n_inner) * stride_inner].  One workgroup per sequence, no atomics.                                                  */
int tl_conv1_dgrad(const float* G, const uint32_t* bits, const float* w, float* dx, int64_t S, int T, int ktaps, int C1, int Tp,
                   int Tout, int n_inner, int64_t stride_outer, int64_t stride_t, int64_t stride_inner, void* stream);

/* ---- SynthesisLite blocks (models/synthesis_models.py:236-263,265-296) ----------------------
 * x (B,Cin,T) channels-first like the reference's Conv1d; 'same' padding (2*pad == k-1).       */
/* z = conv1d(x,w)+bias; part[(b*ntile+tile)][Cout][2] = per-tile (sum z, sum (z - tile mean)^2),
 * ntile=ceil(T/64); Cin * (64 + k - 1) floats must fit 64 KB of LDS                            */
int tl_lite_conv_fwd(const float* x, const float* w, const float* bias, float* z, float* part,
                     int B, int Cin, int Cout, int T, int k, int pad, void* stream);
/* BatchNorm1d statistics: training -> batch mean / rstd from `part` (+ running-stat update,
 * unbiased variance); eval -> from the running buffers                                        */
int tl_lite_bn_finalize(const float* part, float* mean, float* rstd, float* run_mean, float* run_var,
                        int nparts, int C, int64_t count /* = rows * T */, int T, float momentum, float eps, int training,
                        int64_t* tracked /* optional: BatchNorm's num_batches_tracked, += 1 in training */, void* stream);
/* y (B,C,T/2) = MaxPool1d(2)(LeakyReLU(BN(z)))                                                 */
int tl_lite_bn_act_pool_fwd(const float* z, const float* mean, const float* rstd, const float* gamma,
                            const float* beta, float* y, int B, int C, int T, float slope, void* stream);
/* backward of the same: dy (B,C,T/2) -> dz (B,C,T), dgamma, dbeta; work holds (B*C*2 + C*2) floats */
int tl_lite_bn_act_pool_bwd(const float* dy, const float* z, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, float* dz, float* dgamma, float* dbeta,
                            float* work, int B, int C, int T, float slope, int training, void* stream);
/* conv backward: dx (B,Cin,T) (may be null), dwpart (B,Cout*Cin*k), dbpart (B,Cout) per-sample partials */
int tl_lite_conv_bwd(const float* dz, const float* x, const float* w, float* dx, float* dwpart, float* dbpart,
                     int B, int Cin, int Cout, int T, int k, int pad, void* stream);
/* label LSTM over the whole sequence: xl (B,L,in_dim) -> act (B,L,4H), cs, hs (B,L,H)          */
int tl_lite_lstm_fwd(const float* xl, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                     float* act, float* cs, float* hs, int B, int L, int H, int in_dim, void* stream);
/* BPTT from the gradient of the last hidden state: dgates (B,L,4H)                             */
int tl_lite_lstm_bwd(const float* dh_last, const float* w_hh, const float* act, const float* cs, float* dgates,
                     int B, int L, int H, int ld_dh, void* stream);
/* feat (B,ldf) = Dropout([flatten(y2) | h_L]) and its backward split                           */
int tl_lite_cat(const float* y2, const float* hs, float* feat, int B, int F, int H, int L, int ldf,
                float p_drop, uint64_t seed, void* stream);
int tl_lite_uncat(const float* dfeat, float* dy2, float* dh, int B, int F, int H, int ldf, float p_drop,
                  uint64_t seed, void* stream);
/* the same two with the dropout seed in device memory (*seed_dev): capturable in a HIP graph whose replays draw new masks */
int tl_lite_cat_dev(const float* y2, const float* hs, float* feat, int B, int F, int H, int L, int ldf,
                    float p_drop, const uint64_t* seed_dev, void* stream);
int tl_lite_uncat_dev(const float* dfeat, float* dy2, float* dh, int B, int F, int H, int ldf, float p_drop,
                      const uint64_t* seed_dev, void* stream);

/* ---- preprocess/signal band extraction (preprocess/signal/frequency_filter.py) ------------ */
/* Gaussian-bank analytic envelope, circular, exact DFT-domain taps supplied by the host:
 * taps (nb, ntap, 2) complex float64 kernels h_b[n], n = k - half for k in [0, ntap), ntap <= T
 * (frequency_filter.py:158-184); x (C,T) float32 or float64 (x_is_f64), y (C,T) float64 =
 * mean_b |sum_n h_b[n] x[(t-n) mod T]| (envelope != 0) or the mean of the real parts.        */
int tl_gauss_envelope(const void* x, int x_is_f64, const double* taps, double* y, int C, int64_t T,
                      int nb, int ntap, int half, int envelope, void* stream);
/* The same bank through the kernel's Hermitian symmetry (the reference's per-band DFT multiplier is real:
 * h_b[-n] = conj(h_b[n]), frequency_filter.py:155-175): taps (half + 1, 8, 2) = Re / Im of h_b[n], n = 0..half (tap-major); 0.56 x
 * the fp64 operations of tl_gauss_envelope.  8 bands, 2 half + 1 <= T taps within the LDS window.                   */
int tl_gauss_envelope_sym(const void* x, int x_is_f64, const double* taps, double* y, int C, int64_t T, int nb, int half,
                          int envelope, void* stream);
/* The same bank by overlap-save on an LDS-resident FFT (fp64) of nfft = 1024 points: G (8, nfft, 2) = FFT_nfft of each
 * band's truncated kernel (h_b[n], n = -half..half, placed at 0..2 half) / nfft, tw (nfft, 2) = (cos, -sin)(2 pi m / nfft);
 * 2 half <= nfft / 2.
 * 2.4 x fewer fp64 operations per sample than tl_gauss_envelope_sym at 209 taps.                                       */
int tl_hilbert_ols(const void* x, int x_is_f64, const double* G, const double* tw, double* y, int C, int64_t T, int nb,
                   int half, int nfft, int envelope, void* stream);
/* tl_hilbert_ols for band-limited kernels (the Gaussian bank: frequency_filter.py:155-175): when every |G_b| outside a window
 * of nfft / 4 bins [k0_b, k0_b + nfft / 4) is negligible (the caller checks: < 1e-10 of the peak in sum), band b's inverse
 * transform is four independent (nfft / 4)-point transforms, one wave each, with no workgroup barrier in the band loop.
 * Gp (nb, 4, nfft / 4, 2) = G_b[(k0_b + k) % nfft] . exp(+2 pi i k r / nfft), r < 4; k0 (nb) int32, device memory.
 * x_is_f64: 1 = float64 recording, fp64 transforms; 0 = float32 recording, fp32 transforms - the reference's own arithmetic
 * for that dtype (scipy.fft keeps single precision: complex64, frequency_filter.py:167-181); 2 = float32 recording, fp64
 * transforms (round 3's behaviour).  The output is float64 either way, as the reference returns it.                    */
int tl_hilbert_ols_bl(const void* x, int x_is_f64, const double* Gp, const int* k0, const double* tw, double* y, int C,
                      int64_t T, int nb, int half, int nfft, int envelope, void* stream);
/* The same bank evaluated in the DFT domain exactly as the reference writes it (frequency_filter.py:155-184):
 * X = DFT(x), z_b = IDFT(X . K_b), y = mean_b |z_b| (envelope) or mean_b Re z_b.  Arbitrary T (Bluestein chirp-z
 * over radix-2 Stockham passes, fp64).  kernels (nb, T) real = H_b x analytic multiplier; w (T,2) chirp, bf (m2,2) FFT
 * of the chirp filter, tw (m2/2,2) twiddles, m2 >= 2T-1 a power of two: coefficient data from the host, as for
 * tl_fft_resample.  work: (2 C m2 + C T) complex128.  No limit on the kernel length: used when the time-domain
 * taps exceed tl_gauss_envelope's LDS window (low bands at a raw recording rate).                              */
int tl_hilbert_fft(const void* x, int x_is_f64, double* y, int C, int64_t T, const double* kernels, int nb,
                   const double* w, const double* bf, const double* tw, int m2, int envelope, double* work, void* stream);
/* zero-phase IIR (scipy filtfilt, odd padding, lfilter_zi), fp64 (frequency_filter.py:226-227);
 * work holds 2*C*(T + 6*ntaps) doubles                                                        */
int tl_filtfilt_f64(const void* x, int x_is_f64, const double* b, const double* a, const double* zi,
                    double* y, double* work, int C, int64_t T, int ntaps, void* stream);
/* the same zero-phase filter evaluated TIME-PARALLEL (opt-in; frequency_filter.py:226-227): blocks of L samples run scipy's
 * recurrence from a zero state, the block-start states follow from a per-channel scan with the matrices
 * M[m] = A^(L 2^m) (nlev x 8 x 8 x (hi, lo) double-double pairs, from the host: exact powers of the recurrence's transition
 * matrix rounded once; nlev >= 7: the scan takes chunks of 128 blocks), and the blocks are re-run from their true start states.  Agrees with
 * tl_filtfilt_f64 to 2e-8 - 5e-8 relative - the size of the reference's own rounding error - not to the last bit.
 * ntaps <= 9, L >= 8, at most 65 535 blocks.  work: 2*C*(T + 6*ntaps) doubles; swork: 2 * blocks * 8 * C doubles.        */
int tl_filtfilt_scan_f64(const void* x, int x_is_f64, const double* b, const double* a, const double* zi, const double* M,
                         int nlev, double* y, double* work, double* swork, int C, int64_t T, int ntaps, int L, void* stream);
/* causal cascade of biquads (sosfilt), fp64 (frequency_filter.py:223-224)                     */
int tl_sosfilt_f64(const void* x, int x_is_f64, const double* sos, double* y, int C, int64_t T,
                   int nsec, void* stream);
/* the same causal cascade evaluated TIME-PARALLEL (opt-in, TONAL_KERNELS=butter=scan): the recording goes time-major into
 * work, every (channel, block of L samples) runs tl_sosfilt_f64's statements from a zero state, the 2 nsec stacked section
 * states (z0, z1 of section 0, 1, ...) at the block starts follow from a per-channel scan z_{j+1} = A^L z_j + s_j, z_0 = 0,
 * with M[m] = A^(L 2^m) (nlev x 16 x 16 x (hi, lo) double-double pairs, row-major, zero beyond 2 nsec; from the host: exact
 * powers of the cascade's zero-input transition matrix rounded once), and the blocks are re-run from their true start states.  The first L samples
 * of a channel are bit-equal to tl_sosfilt_f64; the rest agrees to a small multiple of the reference's own rounding error.
 * nsec 1..8 (the scan takes chunks of 128 blocks, nlev >= 7, for nsec <= 4; chunks of 64, nlev >= 6, beyond), C <= 65 535,
 * L >= 8, at most 65 535 blocks.  work: C*T doubles; swork: 2 * blocks * 2 nsec * C doubles.                            */
int tl_sosfilt_scan_f64(const void* x, int x_is_f64, const double* sos, const double* M, int nlev, double* y, double* work,
                        double* swork, int C, int64_t T, int nsec, int L, void* stream);
/* causal FIR bank, mean over bands (frequency_filter.py:260-274); taps (nb, ntap) float64      */
int tl_fir_bank(const void* x, int x_is_f64, const double* taps, void* y, int y_is_f64, int C, int64_t T,
                int nb, int ntap, void* stream);
/* the same causal bank by overlap-save on the LDS-resident 1024-point FFT of tl_hilbert_ols: G (nb, 1024, 2) = FFT_1024 of each
 * band's taps / 1024, tw (1024, 2) the twiddle table; ntap <= 513                                                      */
int tl_fir_bank_ols(const void* x, int x_is_f64, const double* G, const double* tw, void* y, int y_is_f64, int C, int64_t T,
                    int nb, int ntap, void* stream);

/* ---- other preprocess/signal steps (same run(data, params) plugin ABI) --------------------------
 * per-channel z-score with statistics over [t0, t1): channel_zscore.py:22-27 (t0=0, t1=T) and
 * zscore_rereference.py:66-68 (baseline interval); y has the input dtype; stats (C,2) f64 workspace */
int tl_row_zscore(const void* x, int is_f64, void* y, double* stats, int C, int64_t T, int64_t t0, int64_t t1,
                  int zero_nans, void* stream);
/* mean and population std (np.std) of the segments x[c][s0 + i L : s0 + (i + 1) L], i < n_seg, of a (C, T) float32 or
 * float64 recording with row_stride elements between rows -> mean, std (C, n_seg) float64 (utils/diagnostics.py
 * segment_mean_std).  Two-pass (the mean, then the squared deviations of the same samples), fp64.  TL_EINVAL on a null
 * pointer, s0 < 0, L < 1, n_seg < 1, s0 + n_seg L > T or row_stride < T                                              */
int tl_segment_moments(const void* x, int x_is_f64, int64_t row_stride, double* mean, double* std, int C, int64_t T,
                       int64_t s0, int64_t L, int64_t n_seg, void* stream);
/* common-average re-reference over the channels with include[c] != 0 (car_rereference.py:34-39)   */
int tl_car(const void* x, int is_f64, const int32_t* include, void* y, int C, int64_t T, int n_inc, void* stream);
/* pandas rolling(window, min_periods=1) z-score, sample std (rolling_zscore.py:36-49); y float64   */
int tl_rolling_zscore(const void* x, int is_f64, double* y, int C, int64_t T, int window, int zero_nans, void* stream);
/* the same quantity in O(1) per sample, for min(window, T) >= 256: per-tile moments (count, sum and sum of squares as (hi, lo)
 * pairs, minimum, maximum) of the 256-sample tiles go to `work`, at least 8 * C * ceil(T / 256) doubles owned by the caller
 * (work_elems says how many it holds); every window is then the sum of a head, whole tiles and a tile prefix.  Agrees with
 * the exact value to a few ulp, not with tl_rolling_zscore bit for bit.  TL_EINVAL, before any launch, on a
 * null pointer, C outside [1, 65535], window <= 1, T > INT32_MAX - 256, min(window, T) < 256 (use tl_rolling_zscore) or a
 * workspace that is too small.                                                                                           */
int tl_rolling_zscore_blocked(const void* x, int is_f64, double* y, double* work, int64_t work_elems, int C, int64_t T,
                              int window, int zero_nans, void* stream);

/* ---- channel selection: one-way ANOVA at every (channel, timepoint) column (channel_selection/active.py:58-76,
 * channel_selection/discriminative.py:171-180 run scipy.stats.f_oneway per channel).  x is (n_rows, cols) row-major with
 * cols = C*T contiguous, float32 or float64 (is_f64); all arithmetic is fp64.
 *
 * per-group column sums: for the n samples idx[0..n) (int32, device; each in [0, n_rows), anything else poisons the
 * column with NaN) of ONE group,  sum[s][col] = sum_i (x[idx[i]][col] - shift[col])  and  sumsq[s][col] = the same of the
 * squares; shift is a row of cols values of x's dtype close to the data (any row of x), and must be the same row for
 * every group of one test.  The samples are cut into `splits` contiguous parts (grid.y), part s writes slab s:
 * sum and sumsq are (splits, cols) float64.  1 <= splits <= 1024                                                          */
int tl_group_moments(const void* x, int is_f64, int64_t n_rows, int64_t cols, const int32_t* idx, int n, const void* shift,
                     int splits, double* sum, double* sumsq, void* stream);
/* F statistic and p-value from the sums of k groups: sum / sumsq are (k, splits, cols) float64 as written above, counts
 * a HOST array of the k group sizes (each >= 1; it travels in the kernel arguments).  F = (ssb/(k-1)) / (ssw/(N-k)),
 * p = the F survival function I_x((N-k)/2, (k-1)/2), x = (N-k)/((N-k) + (k-1) F), evaluated on the device (continued
 * fraction, log-space prefactor).  Degenerate columns as IEEE gives them and scipy returns them: NaN in -> NaN, ssw = 0 with
 * ssb > 0 -> (inf, 0), both 0 -> NaN, N <= k -> NaN.  2 <= k <= 64                                                       */
int tl_anova_finalize(const double* sum, const double* sumsq, const int32_t* counts, int k, int splits, int64_t cols,
                      double* F, double* p, void* stream);
/* per row of p (C, T) float64: count[c] = number of p < thr, maxrun[c] = longest run of consecutive p < thr (NaN is not
 * below) - channel_selection/utils.py:4-30 per channel; one wave per row.  count / maxrun are (C) int32                   */
int tl_max_run_below(const double* p, int C, int64_t T, double thr, int32_t* count, int32_t* maxrun, void* stream);
/* label-permutation test of the same ANOVA: for P relabellings of the N = n0 + n1 samples, where does the statistic pass the
 * threshold?  Sample i is row i of x0 (n0, cols) for i < n0, else row i - n0 of x1 (n1, cols); x1 may be null with n1 = 0
 * (rest and ERP stay two arrays).  x0, x1 and shift (cols; one data row, as for tl_group_moments) share one dtype (is_f64).
 * labels is (P, N) uint8, device: the group of every sample under every relabelling; a label >= k belongs to no group (labels
 * are compared, never used as an index).  counts is a HOST array of the k group sizes (each >= 1, adding up to N): a
 * relabelling keeps them, so sst and the degrees of freedom are those of the observed labelling and p < alpha' is
 *   exceed[pi][col] = ( sum_g S_g^2 / counts[g]  >  tau[col] ),   S_g = sum over the samples labelled g of (x - shift),
 * with tau (cols) float64 = theta sst + total^2 / N formed by the caller (total the shifted column sum of all samples,
 * theta = F_crit dfb / (dfw + F_crit dfb)).  False where the sum or tau is NaN, like p < thr in tl_max_run_below.  exceed is
 * (P, cols) bytes, 0 or 1.  The group sums are one fp64 product onehot (P k x N) . (x - shift) on v_mfma_f64_16x16x4_f64;
 * the samples are staged 32 at a time.  TL_EINVAL, before any launch, on a null pointer, n0 < 1, n1 < 0 or n1 > 0 without
 * x1, cols or P < 1, k outside [2, 64], a group size < 1, sizes that do not add up to N, or more than 2^31 - 1 blocks
 * (ceil(cols / 64) * ceil(P / 64), ceil(P / 128) for k = 2)                                                              */
int tl_perm_exceed(const void* x0, int64_t n0, const void* x1, int64_t n1, int is_f64, int64_t cols, const void* shift,
                   const uint8_t* labels, int P, const int32_t* counts, int k, const double* tau, uint8_t* exceed,
                   void* stream);
/* per row of a byte mask (rows, T), e.g. exceed above read as (P * C, T): maxrun[row] = the longest run of consecutive
 * non-zero cells (0 if none); one wave per row, 64 cells a step.  maxrun is (rows) int32                                  */
int tl_perm_runs(const uint8_t* mask, int64_t rows, int64_t T, int32_t* maxrun, void* stream);
/* rank form of the same test (Kruskal-Wallis, scipy.stats.kruskal along axis 0): midranks down the sample axis.  Sample i is
 * row i of x0 (n0, cols) for i < n0, else row i - n0 of x1 (n1, cols); x1 may be null with n1 = 0.  x0 and x1 share one dtype
 * (is_f64).  ranks (n0 + n1, cols) float32:  ranks[i][col] = scipy.stats.rankdata(column col, method='average')[i], bit for bit
 * (a midrank is a multiple of 0.5, exact in float32; tl_group_moments and tl_perm_exceed take the array as float32 input).
 * Values are ranked on their own bits, float64 on float64; -0.0 and +0.0 tie; +-inf rank as values; a column that holds a
 * NaN gets NaN in every row.  One block sorts a tile of consecutive columns in LDS (bitonic network on order-preserving keys
 * with 16-bit sample indices, padded to a power of two); the tile is the largest power of two of at most 64 columns for which
 * npad * columns * (4 or 8 key bytes + 2) <= 40 KiB, npad = max(2, n0 + n1 rounded up to a power of two), and one column where
 * a column alone takes more (up to 80 KiB).  TL_EINVAL, before
 * any launch, on a null pointer, n0 < 1, n1 < 0 or n1 > 0 without x1, cols < 1, n0 + n1 > 8192, or more than 2^31 - 1 tiles  */
int tl_rank_columns(const void* x0, int64_t n0, const void* x1, int64_t n1, int is_f64, int64_t cols, float* ranks,
                    void* stream);
/* Kruskal-Wallis H and p from the sums of k groups of MIDRANKS: sum / sumsq / counts / splits as for tl_anova_finalize.
 * H = (N - 1) ssb / (ssb + ssw) - the statistic with its tie correction - and p = Q((k - 1)/2, H/2), the chi-square tail with
 * k - 1 degrees of freedom, evaluated on the device in float64 (series of P below a + 1, continued fraction of Q above;
 * the power part of the prefactor in log space).  NaN in -> NaN; ssb + ssw = 0 (every value of the column identical, where
 * scipy raises) -> H = p = NaN.  2 <= k <= 64                                                                            */
int tl_kruskal_finalize(const double* sum, const double* sumsq, const int32_t* counts, int k, int splits, int64_t cols,
                        double* H, double* p, void* stream);

/* ---- mel-spectrogram targets of a batch of trials (utils/audio.py audio_to_mel, one trial at a time on the host):
 * STFT -> |X|^power -> mel bank -> dB, two launches, fp64 throughout, float32 at the final store.
 *
 * audio is (N, S) float32 or float64 (audio_is_f64) with row_stride elements between trials.  Frame f of a trial covers the
 * samples f*hop - (center ? n_fft/2 : 0) + [0, n_fft); samples outside [0, S) read as zero (no padded copy).  window
 * (n_fft) float64 = periodic Hann of win_length, zero-padded and centred to n_fft; tw (n_fft, 2) float64 = (cos, -sin)
 * (2 pi i / n_fft); the mel bank as per-band runs: bands (n_mels, 3) int32 = {first bin, one past the last bin, offset of
 * the run's first weight in weights}, weights (n_weights) float64 (a run outside [0, n_fft/2 + 1) or outside weights makes
 * its band NaN).  Writes mel (N, n_mels, n_frames) float64 and rowmax (N) float64 = each trial's maximum (cleared here).
 * n_fft in {256, 512, 1024, 2048}, 1 <= win_length <= n_fft, hop >= 1, power 1 or 2, n_mels >= 1, and
 * n_frames == 1 + (S + (center ? n_fft : 0) - n_fft) / hop                                                              */
int tl_mel_power(const void* audio, int audio_is_f64, int64_t row_stride, const double* window, const double* tw,
                 const int32_t* bands, const double* weights, int n_weights, double* mel, double* rowmax, int N, int64_t S,
                 int n_fft, int win_length, int hop, int center, int power, int n_mels, int64_t n_frames, void* stream);
/* mel / rowmax as written above -> out (N, n_mels * n_frames) float32, band-major per trial.  in_db = 0: a cast; 1:
 * 10 log10(max(1e-10, v)) - 10 log10(max(1e-10, rowmax[n])), clipped from below at the trial's largest dB value - 80
 * (power_to_db(ref=np.max, top_db=80) per trial)                                                                      */
int tl_mel_finish(const double* mel, const double* rowmax, float* out, int N, int n_mels, int64_t n_frames, int in_db,
                  void* stream);

/* ---- Welch power spectral density of every row of a recording (utils/diagnostics.py welch_psd; the meaning of
 * scipy.signal.welch(axis=1, return_onesided=True, average='mean')), on the transform of tl_mel_power, fp64 throughout.
 *
 * x is (C, T) float32 or float64 (x_is_f64) with row_stride elements between rows, read in place.  Segment s covers the
 * samples s * (nperseg - noverlap) + [0, nperseg); it is zero-padded to n_fft in registers (the padding is never read from
 * memory).  detrend 0 = none, 1 = constant (the segment's mean is removed before windowing).  window (n_fft) float64 = the
 * nperseg coefficients followed by zeros; tw as for tl_mel_power; scale = 1 / (fs sum w^2) or 1 / (sum w)^2, from the host.
 * Two launches: every (channel, slab of consecutive segments) adds |X|^2 over its segments into work (C, n_slabs, n_fft/2+1)
 * float64 (work_elems doubles; a slab past the last segment writes zeros), then psd (C, n_fft/2 + 1) float64 = the slabs
 * added in order / n_seg * scale, doubled except at DC and Nyquist.  No atomics: two runs give the same bits.
 * TL_EINVAL, before any launch, on a null pointer, n_fft outside {256, 512, 1024, 2048}, nperseg outside [2, n_fft],
 * noverlap < 0 or nperseg - noverlap < 1, detrend outside {0, 1}, C outside [1, 65535], T < nperseg, row_stride < T,
 * n_seg != (T - noverlap) / (nperseg - noverlap), n_slabs < 1 or a workspace that is too small                          */
int tl_welch_psd(const void* x, int x_is_f64, int64_t row_stride, const double* window, const double* tw, double* work,
                 int64_t work_elems, double* psd, int C, int64_t T, int n_fft, int nperseg, int noverlap, int detrend,
                 double scale, int64_t n_seg, int n_slabs, void* stream);

/* ---- the way back (utils/audio.py mel_to_audio, one trial at a time on the host): mel -> linear spectrum -> Griffin-Lim.
 * window, tw, bands, weights are the tables of tl_mel_power; n_fft in {256, 512, 1024, 2048}; every array float64.
 *
 * min_{x >= 0} ||fb x - p||^2 per frame by nnls_iter iterations of accelerated projected gradient (FISTA) from x = 0 with
 * step = 1 / (largest singular value of fb)^2 (utils/audio.py mel_to_linear).  mel_power is (N, n_mels, n_frames); the bank
 * a second time by bin: bin_bands (n_fft/2 + 1, 2) int32 = the at most two bands that cover the bin (-1 = none),
 * bin_weights (n_fft/2 + 1, 2) their weights; momentum (nnls_iter) = the factors (t_k - 1) / t_{k+1} of the t_k sequence.
 * Every product and sum is rounded on its own, in the order utils/audio.py bank_operators writes out, so x has the bits of
 * the host statement.  out (N, n_fft/2 + 1, n_frames) = x^(1/power), power 1 or 2.
 * 1 <= n_mels <= 256, n_weights <= n_fft + 2, nnls_iter >= 1, step > 0                                                   */
int tl_mel_invert(const double* mel_power, const int32_t* bands, const double* weights, int n_weights, const int32_t* bin_bands,
                  const double* bin_weights, const double* momentum, double* out, int N, int n_fft, int n_mels,
                  int64_t n_frames, int nnls_iter, double step, int power, void* stream);
/* Griffin-Lim, one iteration = tl_gl_synth + tl_gl_analyse (utils/audio.py griffinlim).  Spectra are frame-major here:
 * mag (N, n_frames, n_fft/2 + 1), angles and tprev (N, n_frames, n_fft/2 + 1, 2) = (re, im).
 * synth: frames (N, n_frames, n_fft) = irfft(mag * angles) * window, per frame; angles_shared = 1: angles is one
 * (n_frames, n_fft/2 + 1, 2) table used for every trial (the initial phases)                                             */
int tl_gl_synth(const double* mag, const double* angles, int angles_shared, const double* window, const double* tw,
                double* frames, int N, int n_fft, int64_t n_frames, void* stream);
/* analyse: signal = samples [n_fft/2, n_fft/2 + length) of the overlap-add of frames over wsum (n_fft + hop (n_frames - 1)) =
 * the window-square sum where it exceeds float32 tiny, else undivided (istft); rebuilt = its centred STFT, frames from
 * 1 + length / hop on zero; angles = rebuilt - momentum / (1 + momentum) * tprev (first = 1: rebuilt alone, tprev not
 * read), angles /= |angles| + 1e-16, tprev = rebuilt.  1 <= win_length <= n_fft, 1 <= hop <= win_length,
 * 1 <= length <= n_fft/2 + hop (n_frames - 1)                                                                            */
int tl_gl_analyse(const double* frames, const double* wsum, const double* window, const double* tw, double* angles,
                  double* tprev, int N, int n_fft, int win_length, int hop, int64_t n_frames, int64_t length, double momentum,
                  int first, void* stream);
/* out (N, length) = the signal as tl_gl_analyse forms it, as a gather per sample: no atomics, the same bits every run     */
int tl_gl_overlap_add(const double* frames, const double* wsum, double* out, int N, int n_fft, int win_length, int hop,
                      int64_t n_frames, int64_t length, void* stream);

/* ---- F0 tracking of a batch of clips (utils/audio.py yin_f0, one clip at a time on the host): the YIN estimator with the
 * steps of librosa 0.10's yin(pad_mode='constant'), one workgroup per frame, fp64 throughout, no atomics (two runs give the
 * same bits), one launch.
 *
 * audio is (N, S) float32 or float64 (audio_is_f64) with row_stride elements between clips, read in place.  Frame f of a clip
 * covers the samples f*hop - (center ? frame_length/2 : 0) + [0, frame_length); samples outside [0, S) read as zero (no padded
 * copy).  Per frame x, with W = win_length, pmin = min_period, pmax = max_period:
 *   d[tau]  = sum_{j<W} (x[j] - x[j+tau])^2, tau <= pmax, as a direct sum (never E(0) + E(tau) - 2 r(tau), which cancels where
 *             d -> 0);  cm[tau] = (d[1] + ... + d[tau]) / tau;  c[i] = d[pmin+i] / (cm[pmin+i] + DBL_MIN), i <= pmax - pmin;
 *   troughs: i = 0 iff c[0] < c[1]; interior i iff c[i] < c[i-1] && c[i] <= c[i+1]; the last index never;
 *   pick i  = the first trough with c[i] < threshold, else the lowest index of the global minimum;
 *   shift   = -b / a with a = c[i+1] + c[i-1] - 2 c[i], b = (c[i+1] - c[i-1]) / 2 when i is interior and |b| < |a|, else 0.
 * Writes, each (N, n_frames): f0 = sr / (pmin + i + shift) and aperiodicity = c[i] (float64), period_index = i (int32),
 * rms = sqrt(mean(x[0:W]^2)) (float64); and, where cmnd is not null, the whole curve c as (N, n_frames, pmax - pmin + 1)
 * float64.  TL_EINVAL, before any GPU call, on a null required pointer, N < 1, S < 1, win_length outside
 * [1, frame_length), frame_length > 4096, hop < 1, min_period < 1, max_period outside [min_period + 1, frame_length -
 * win_length - 1], threshold <= 0, sr <= 0, S < frame_length with center = 0, n_frames != 1 + S / hop (center) resp.
 * 1 + (S - frame_length) / hop, row_stride < S with N > 1, or more than 2^31 - 1 frames                                   */
int tl_yin_f0(const void* audio, int audio_is_f64, int64_t row_stride, double* f0, double* aperiodicity,
              int32_t* period_index, double* rms, double* cmnd, int N, int64_t S, int frame_length, int win_length, int hop,
              int center, int min_period, int max_period, double threshold, double sr, int64_t n_frames, void* stream);

/* FFT resampling = scipy.signal.resample(x, num, axis=1) (downsample.py:21-27): Bluestein chirp-z on
 * power-of-two FFTs.  Host-prepared coefficient arrays (complex128 interleaved): w1 (nx) / w2 (num)
 * chirps exp(i pi m^2 / n); bf1 (m2a) / bf2 (m2b) spectra of the chirp filters; tw1 (m2a/2) / tw2
 * (m2b/2) twiddles exp(-2 pi i k / m2).  work: C * (2*max(m2a,m2b) + m2b) complex128.  y has x's dtype. */
int tl_fft_resample(const void* x, int is_f64, void* y, int C, int64_t nx, int64_t num, const double* w1,
                    const double* bf1, const double* tw1, int m2a, const double* w2, const double* bf2,
                    const double* tw2, int m2b, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
