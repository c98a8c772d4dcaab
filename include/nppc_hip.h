/* C ABI of libnppc_hip.so -- the gfx950 (MI355X / CDNA4) kernels behind the NPPC-audio train step.
 *
 * The reference (kfirc1503/generative-audio) has no FFI: its hot path is stock PyTorch ops called from Python
 * (SURVEY.md section 8b).  Each entry point below replaces the ATen call sites cited beside it (file:line under
 * the reference root).  Conventions:
 *   - plain device pointers + sizes, no torch types; every tensor is borrowed for the launch, nothing is
 *     allocated or freed here; outputs / workspaces are pre-allocated by the caller
 *   - `stream` is a hipStream_t; launches are asynchronous and never synchronise the device
 *   - return 0 on success, non-zero on bad arguments (1) / launch failure (2) / unsupported shape (3)
 *   - prec: 0 = bf16 MFMA operands + bf16 saved activations, fp32 accumulate / cell state / statistics
 *           1 = fp32 everywhere (exact-f32 MFMA) -- the parity mode
 *   - activations of the full-band nets are time-major [batch][Tp][ld] (Tp = T' rounded up to 128, ld = channels
 *     rounded up to 64, padding zero); sub-band tensors are time-major [T'][N][...], N = B*F' sequences
 */
#ifndef NPPC_HIP_H
#define NPPC_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- signal front end ------------------------------------------------------------------------------------
 * torch.stft(center, periodic hann, onesided): utils.py:107-147, nppc_audio/trainer.py:349-355 */
int nppc_stft(const float* wave, float* re, float* im, float* mag /*nullable*/, int B, int L, int nfft, int hop,
              void* stream);
/* drop_band: audio_zen/acoustics/feature.py:254-285 */
int nppc_dropband(const float* in, float* out, int B, int C, int F, int T, int G, void* stream);
/* build_complex_ideal_ratio_mask + compress_cIRM (+ drop_band of trainer.py:359-362): audio_zen/acoustics/mask.py:24-54 */
int nppc_cirm_build_compress(const float* nr, const float* ni, const float* cr, const float* ci, float* out, int B, int F,
                             int T, int G, float eps, void* stream);
/* decompress_cIRM (mask.py:57-60) + crm_to_stft_components (utils.py:241-249 -> :75-79, conj(mask)*noisy) */
int nppc_cirm_decompress_apply_conj(const float* crm, const float* nr, const float* ni, float* dec /*nullable*/,
                                    float* emag, float* ere, float* eim, int B, int F, int T, void* stream);

/* the same with the true product mask*noisy: utils.model_outputs_to_waveforms (utils.py:37-58), crm_to_spectogram (:252-256) */
int nppc_cirm_decompress_apply(const float* crm, const float* nr, const float* ni, float* dec /*nullable*/, float* emag,
                               float* ere, float* eim, int B, int F, int T, void* stream);
/* torch.istft(center, periodic hann, length=L): utils.py:60-70, nppc_audio/validator.py:136-143 */
int nppc_istft(const float* re, const float* im, float* out, int B, int T, int nfft, int hop, int L, void* stream);

/* ---- full-band front: offline_laplace_norm + ChannelTimeSenseSELayer ---------------------------------------
 * audio_zen/model/base_model.py:210-224, audio_zen/model/module/attention_model.py:43-98,
 * fullsubnet_plus.py:158-185, nppc_audio/networks.py:80-112 */
int nppc_rowsum(const float* x, double* sums, long R, int T, void* stream);
/* the same for ALL input maps of a net at once (maps: host array of nmaps = 3 or 6 device pointers, map j = m*3 + z with
 * z the mag / real / imag branch and m the noisy / enhanced call): three launches (row sums, attention, scale + transpose)
 * instead of three per map.  rowsum [nmaps][B][C]; scale and the saved tensors [3][nm][B][..]; parameters of branch z sit
 * z * sW elements behind the pointers given; X0 [3][B][Tp][ld] with branch stride sY, map j -> branch z, columns m*C.. */
int nppc_tsse_fwd_maps(int prec, const float* const* maps, int nmaps, double* rowsum, const float* cw0, const float* cb0,
                       const float* cw1, const float* cb1, const float* cw2, const float* cb2, int ks0, int ks1, int ks2,
                       const float* fcw, const float* fcb, const float* w1, const float* b1, const float* w2, const float* b2, long sW,
                       float* scale, float* ns, float* pre, float* sq, float* h1, float* sg, void* X0, long sY, int B, int C, int T,
                       int look_ahead, int Tp, int ld, void* stream);
/* ... and its backward (parameter gradients only: the maps are data), three launches, NO atomics: every gradient element
 * has one writer and a fixed summation order (samples, then maps, in index order), so repeated runs are bit-identical.
 * ws: nppc_tsse_bwd_ws_elems(nmaps, ..) floats (per map: dsg | da2 | da1 | per-sample conv / fc contributions) */
int nppc_tsse_bwd_ws_elems(int nmaps, int B, int C, int ks0, int ks1, int ks2, long* elems);
int nppc_tsse_bwd_maps(int prec, const void* dX0, long sY, const float* const* maps, int nmaps, const double* rowsum,
                       const float* cw0, const float* cw1, const float* cw2, int ks0, int ks1, int ks2, const float* fcw,
                       const float* w1, const float* w2, long sW, const float* ns, const float* pre, const float* sq,
                       const float* h1, const float* sg, float* ws, float* g_cw0, float* g_cb0, float* g_cw1, float* g_cb1,
                       float* g_cw2, float* g_cb2, float* g_fcw, float* g_fcb, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                       int B, int C, int T, int look_ahead, int Tp, int ld, void* stream);
int nppc_tsse_fwd(const float* x, const double* rowsum, const float* cw0, const float* cb0, const float* cw1,
                  const float* cb1, const float* cw2, const float* cb2, int ks0, int ks1, int ks2, const float* fcw,
                  const float* fcb, const float* w1, const float* b1, const float* w2, const float* b2, float* scale,
                  float* ns, float* pre, float* sq, float* h1, float* sg, int B, int C, int T, int look_ahead,
                  void* stream);
int nppc_tsse_bwd(int prec, const void* dX0, const float* x, const double* rowsum, const float* cw0, const float* cw1,
                  const float* cw2, int ks0, int ks1, int ks2, const float* fcw, const float* w1, const float* w2,
                  const float* ns, const float* pre, const float* sq, const float* h1, const float* sg, float* dsg_ws, /* nppc_tsse_bwd_ws_elems(1, ..) floats */
                  float* g_cw0, float* g_cb0, float* g_cw1, float* g_cb1, float* g_cw2, float* g_cb2, float* g_fcw,
                  float* g_fcb, float* g_w1, float* g_b1, float* g_w2, float* g_b2, int B, int C, int T, int look_ahead, int Tp,
                  int ld, int coff, void* stream);
int nppc_scale_transpose(int prec, const float* x, const float* scale /*nullable*/, void* y, int B, int C, int T, int Tp,
                         int ld, int coff, void* stream);

/* ---- full-band TCN stack: TCNBlock x8 + Linear + ReLU ------------------------------------------------------
 * audio_zen/model/module/causal_conv.py:67-108, audio_zen/model/module/sequence_model.py:47-58,106-112
 * nppc_gemm_nt: C[R][N] = A[R][K] * B[N][K]^T (+ epilogue); epi: 0 plain, 1 bias+PReLU+GroupNorm statistics,
 * 2 bias+residual, 3 bias+ReLU, 4 fp32 output (split-K slabs), 5 mask by (res > 0).  ksplit > 1 splits K: epi 4 only, with
 * no bias and no stats (NPPC_EUNSUPPORTED otherwise); slab z * ksplit + s starts at C + (z * ksplit + s) * sC. */
int nppc_gemm_nt(int prec, int epi, const void* A, long lda, long sA, const void* B, long ldb, long sB, void* C, long ldc,
                 long sC, const float* bias, long sBias, const void* res, long ldres, long sRes, const float* slope,
                 long sSlope, double* stats, long sStats, int R, int N, int K, int Tp, int Tv, int Nv, int relu_in,
                 int batch, int ksplit, void* stream);
/* *bn = the tile width nppc_gemm_nt / _colsum / _gn run a product of these sizes on: 128 or 64 columns (LDS-staged),
 * 0 = the register-staged kernel (the K slice is no multiple of 64 bf16 / 32 fp32 elements) */
int nppc_gemm_nt_tile(int prec, int N, int K, int ksplit, int* bn);
/* long-K weight-gradient product: C_slab[z][M][N] (fp32) = A[M][K/ksplit slice z] * B[N][same slice]^T, LDS-staged
 * 128x128 tiles; M, N multiples of 128, K a multiple of (64 bf16 | 32 fp32) * ksplit */
int nppc_gemm_nt_splitk(int prec, const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, long K,
                        int ksplit, void* stream);
/* the same product on ROW-major operands (no transposed copies): C_slab[z][M][N] = A[rows z][M]^T * B[rows z][N], bf16,
 * LDS tiles read back with ds_read_b64_tr_b16; M % 128 == 0, N % 64 == 0, R % (64*ksplit) == 0 */
int nppc_gemm_tn_splitk(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, long R, int ksplit,
                        void* stream);
/* the same plus rowsum[z][m] = sum over the rows of slice z of A[r][m] ([ksplit][M] fp32): the bias gradient of an LSTM
 * layer out of the weight-gradient product that reads the same gate gradients (LDS-DMA kernel shapes only: M % 256 == 0,
 * N % 128 == 0, (R / ksplit) % 64 == 0, at least 256 workgroups; NPPC_EUNSUPPORTED otherwise) */
int nppc_gemm_tn_splitk_rowsum(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, long R,
                               int ksplit, float* rowsum, void* stream);
/* two B operands side by side behind ONE pass over A: C_slab[z][m][0 .. N1) = A^T . B1, C_slab[z][m][N1 .. N1 + N2) = A^T . B2
 * over the rows of K slice z (the weight gradients of one LSTM layer, W_ih | W_hh, share their gate gradients: torch's
 * autograd of nn.LSTM, audio_zen/model/module/sequence_model.py:113-123, computes them as separate products).  rowsum
 * optional ([ksplit][M], as above).  bf16; M % 256 == 0, N1 % 192 == 0, N2 == 64 or N2 % 192 == 0, (R / ksplit) % 64 == 0,
 * ldc >= N1 + N2, at least 256 workgroups; NPPC_EUNSUPPORTED otherwise (run the products separately) */
int nppc_gemm_tn_splitk2(const void* A, long lda, const void* B1, long ldb1, int N1, const void* B2, long ldb2, int N2, float* C,
                         long ldc, int M, long R, int ksplit, float* rowsum, void* stream);
int nppc_gemm_tn_splitk_batched(const void* A, long lda, long sA, const void* B, long ldb, long sB, float* C, long ldc, long sC,
                                int M, int N, long R, int ksplit, int batch, void* stream);
/* `nprob` TN products of ONE shape in one launch, no split-K, each written FINISHED to its destination (no fp32 slabs, no
 * reduction launch): the weight gradients of the TCN 1x1 convolutions of all blocks x branches.  `table` lives in DEVICE
 * memory (nprob entries of 8 x 64 bits) and is read by the kernel only: the caller vouches for lda >= M, ldb >= N (multiples
 * of 8), operands of at least R rows and 0 <= nvalid <= N.  Only columns n < nvalid of the product reach the destination:
 *   NPPC_TN_STORE_ASIS        dst[m * dst_ld + n] = sum_r A[r][m] * B[r][n]
 *   NPPC_TN_STORE_TRANSPOSED  dst[n * dst_ld + m] = the same
 * One workgroup sums all R rows of its output tile (128 x 128; a last column tile of 64 takes N % 128): deterministic, one
 * writer per element.  The rows are summed in k row blocks (k = 8, or the largest k < 8 that divides R / 64) from zero and
 * the block sums added in order from zero: the same fp32 additions, hence
 * the same bits, as nppc_gemm_tn_splitk_batched with ksplit = k followed by nppc_reduce_slabs / nppc_reduce_slabs_t
 * (where that launch takes the register-staged kernel, as it does at the TCN shapes: its k-step order is the one used here).
 * bf16; M % 128 == 0, N % 64 == 0, R % 64 == 0, nprob <= 65535; NPPC_EUNSUPPORTED otherwise */
enum { NPPC_TN_STORE_ASIS = 0, NPPC_TN_STORE_TRANSPOSED = 1 };
typedef struct nppc_tn_problem {
  const void* A; long lda;      /* [R][lda] bf16 */
  const void* B; long ldb;      /* [R][ldb] bf16 */
  float* dst; long dst_ld;
  long nvalid;
  long kind;
} nppc_tn_problem;
int nppc_gemm_tn_grouped(const nppc_tn_problem* table, int nprob, int M, int N, long R, void* stream);
int nppc_gemm_tn_splitk_taps(const void* A, long lda, const void* B, long ldb, float* C, long ldc, int M, int N, long R,
                             int ksplit, int Wp, int shift_a, void* stream);
int nppc_pack_matrix(int prec, const float* src, void* dst, int N, int K, int Npad, int ldd, int transpose, void* stream);
/* the same for an n_a x n_b grid of equally shaped matrices at constant strides (elements) in ONE launch: the 8 TCN blocks
 * x 3 full-band branches of a FullSubNet+ keep their parameters at constant offsets in the flat parameter buffer */
int nppc_pack_matrix_batched(int prec, const float* src, void* dst, int N, int K, int Npad, int ldd, int transpose, int n_a,
                             int n_b, long src_stride_a, long src_stride_b, long dst_stride_a, long dst_stride_b, void* stream);
int nppc_tcn_dwconv(int prec, const void* in, void* out, const double* st1, double* st2, const float* gamma,
                    const float* beta, const float* wd, const float* bd, const float* slope2, int B, int Cc, int ld, int Tp,
                    int Tv, int dil, float eps, long sAct, long sSt, long sP, int batch, void* stream);
int nppc_tcn_gn_apply(int prec, const void* in, void* out, const double* st, const float* gamma, const float* beta, int B,
                      int Cc, int ld, int Tp, int Tv, float eps, long sAct, long sSt, long sP, int batch, void* stream);
/* backward of GroupNorm(1,C)+PReLU and of the depthwise dilated conv (autograd of causal_conv.py:96-108) */
int nppc_tcn_gn_bwd(int prec, const void* dA, const void* y, const double* st, const float* gamma, const float* slope,
                    double* S, void* dpre, float* dgamma, float* dbeta, float* dslope, int B, int Cc, int Tp, int Tv, float eps,
                    long sAct, long sSt, long sP, int batch, void* stream);
int nppc_tcn_dwconv_bwd(int prec, const void* du, const void* y1, const double* st1, const float* gamma, const float* beta,
                        const float* wd, void* dz, float* dwd, float* dbd, int B, int Cc, int Tp, int Tv, int dil, float eps,
                        long sAct, long sSt, long sP, int batch, void* stream);
/* fused backward of a TCNBlock's middle (causal_conv.py:98-106 in reverse: GroupNorm-2, PReLU-2, depthwise dilated conv,
 * GroupNorm-1, PReLU-1): dA = gradient of GN2's output -> dpre1 = gradient of conv1x1's output, every parameter gradient of
 * those stages and the conv1x1 bias gradient, in ONE reduce + ONE apply launch (csrc/tcn_bwd.hip).  y1 / y2: the saved PReLU
 * outputs, st1 / st2 their GroupNorm (sum, sumsq); S: [batch][B][Cc/64][8] fp64 workspace for the channel groups' shares of the per-sample sums (no initial state; no atomics: the apply pass adds the shares in index order); part:
 * nppc_tcn_mid_bwd_part_elems(B, Cc, Tp, batch, &n) -> n floats of workspace for per-workgroup partial sums (a third, tiny launch adds
 * them to the gradients in a fixed order: no atomics anywhere, repeated runs are bit-identical); a2 (nullable) receives GN2(y2), the operand of the sconv weight
 * gradient.  Gradients are ACCUMULATED into their destinations.  colpart (nullable): the tile column sums that
 * nppc_gemm_nt_colsum left for the block's upstream gradient, [batch][cp_tiles][cp_ld] -> the finishing launch also writes the
 * sconv bias gradient dbias2[z*sP + c] = sum over the tiles, c < cp_cols (sconv.bias: causal_conv.py:107). */
int nppc_tcn_mid_bwd_part_elems(int B, int Cc, int Tp, int batch, long* n);
int nppc_tcn_mid_bwd(int prec, const void* dA, const void* y2, const void* y1, const double* st1, const double* st2, double* S,
                     float* part,
                     const float* gamma1, const float* beta1, const float* gamma2, const float* beta2, const float* wd,
                     const float* slope1, const float* slope2, void* a2, void* dpre1, float* dgamma2, float* dbeta2,
                     float* dgamma1, float* dbeta1, float* dwd, float* dbd, float* dslope1, float* dslope2, float* dbias1,
                     const float* colpart, int cp_tiles, int cp_ld, int cp_cols, float* dbias2, int B,
                     int Cc, int Tp, int Tv, int dil, float eps, long sAct, long sSt, long sP, int batch, int finish_now,
                     void* stream);
/* finish_now = 0 defers the finishing launch: one nppc_tcn_mid_bwd_finish then adds up the partial rows of `nblk` blocks at
 * once (block k: part + k * partL, colpart + k * colpartL, gradients k * sL elements behind the pointers given -- the blocks of
 * the TCN stack sit at a constant stride in the flat buffer).  Round 3 ran eight 5-us finishing launches per step, each of
 * which waited up to 0.5 ms for CUs beside the weight-gradient GEMMs of the side queue. */
int nppc_tcn_mid_bwd_finish(const float* part, long partL, const float* colpart, long colpartL, int cp_tiles, int cp_ld,
                            int cp_cols, float* dgamma2, float* dbeta2, float* dgamma1, float* dbeta1, float* dwd, float* dbd,
                            float* dslope1, float* dslope2, float* dbias1, float* dbias2, int B, int Cc, long sP, long sL,
                            int batch, int nblk, void* stream);
/* sconv of a TCNBlock with the GroupNorm in front of it (norm2, causal_conv.py:104-106) folded into the product:
 *   C = rstd_b * (A Wg^T) - mean_b * rstd_b * v + u + res,  A = the un-normalised depthwise output, stats = its per-sample
 * (sum, sumsq), cnt = elements per sample; nppc_tcn_pack_sconv builds Wg[n][k] = gamma[k] W[n][k], v[n] = sum_k Wg[n][k],
 * u[n] = sum_k beta[k] W[n][k] + bias[n] for n_a x n_b equally shaped blocks at constant parameter strides */
int nppc_gemm_nt_gn(int prec, const void* A, long lda, long sA, const void* Wg, long ldb, long sB, void* C, long ldc, long sC,
                    const float* u, const float* v, long sUV, const void* res, long ldres, long sRes, const double* stats,
                    long sStats, double cnt, float eps, int R, int N, int K, int Tp, int Tv, int Nv, int batch, void* stream);
/* nppc_gemm_nt with epi EPI_RESIDUAL or EPI_MASK_POS (LDS-staged shapes only: K % 64 == 0 in bf16 / % 32 in fp32) that also
 * leaves colpart[z][R/128][N] (fp32) = the column sums of every 128-row tile of the stored output.  The output is the upstream
 * gradient of the next 1x1 convolution down the backward chain (causal_conv.py:107, fullsubnet_plus.py fc_output_layer), whose
 * bias gradient is the sum of these partials over the tiles (nppc_tcn_mid_bwd adds them up): no pass of its own over C. */
int nppc_gemm_nt_colsum(int prec, int epi, const void* A, long lda, long sA, const void* B, long ldb, long sB, void* C, long ldc,
                        long sC, const float* bias, long sBias, const void* res, long ldres, long sRes, int R, int N, int K,
                        int Tp, int Tv, int Nv, int batch, float* colpart, void* stream);
int nppc_tcn_pack_sconv(int prec, const float* W, const float* gamma, const float* beta, const float* bias, void* Wg, float* u,
                        float* v, int N, int K, int Npad, int ldd, int n_a, int n_b, long src_stride_a, long src_stride_b,
                        long dst_stride_a, long dst_stride_b, void* stream);
int nppc_transpose(int prec, const void* in, void* out, int rows, int cols, long ld_in, long ld_out, long sIn, long sOut,
                   int relu, int batch, void* stream);
/* out[z][c] += sum_r M[z][r][c] (bias gradients), two launches, NO atomics: row blocks leave partial sums in `scratch`
 * (nppc_colsum_scratch_elems floats, caller-owned: one scratch per concurrently running call) and a finishing launch adds them
 * in a fixed order, so repeated runs are bit-identical */
int nppc_colsum_scratch_elems(int rows, int cols, int batch, long* n);
int nppc_colsum(int prec, const void* M, float* out, int rows, int cols, long ld, long sM, long sOut, int batch,
                float* scratch, long scratch_elems, void* stream);
int nppc_reduce_slabs_t(const float* slabs, int S, long slab_stride, long ld, float* dst, long dst_ld, int rows, int ncols,
                        long sSlab, long sDst, int batch, void* stream);
int nppc_reduce_slabs(const float* slabs, int S, long slab_stride, long ld, float* dst, long dst_ld, int rows, int col0,
                      int ncols, int permH, int accumulate, long sSlab, long sDst, int batch, void* stream);

/* ---- sub-band stage: unfold + concat + laplace norm + drop_band + LSTM input layout, output head ------------
 * audio_zen/model/base_model.py:15-46, fullsubnet_plus.py:188-230, nppc_audio/networks.py:115-161,
 * sequence_model.py:118-123 (fc_output_layer) */
/* work: caller-owned, 2*B 8-byte words (B fp64 partial sums + B arrival counters), zeroed ONCE by the caller; the kernel
 * re-arms it, so the same workspace serves every later launch and launches on different workspaces may overlap */
int nppc_subband_mean(int prec, const void* src, int ldS, const void* fb, int ldF, long strideFb, const float* mult,
                      float* scale, double* work, int B, int F, int Tp, int Tv, int nfeat, void* stream);
int nppc_subband_stage(int prec, const void* src, int ldS, const void* fb, int ldF, long strideFb, const float* scale,
                       void* x, int B, int F, int Tp, int Tv, int nb, int G, int KX, int ones_col, void* stream);
int nppc_subband_stage_bwd(int prec, const void* dx, const void* x, const void* fb, const float* scale, double* D,
                           void* dpre, int B, int F, int Tp, int Tv, int ldF, long strideFb, int nb, int G, int KX,
                           void* stream);
/* restorer (n_maps = 1) only: gradient of the unfolded, laplace-normalised attention columns (the first 2nb+1 of a
 * sub-band row) with respect to the TCN input of the magnitude branch, ADDED into dX0 [B][Tp][ldX] (bf16 | fp32) for
 * t < Tv: dX0[b][t][f] += sc_b sum dx[t][n(b,f')][k] - sc_b D[bo] mult[f] / Nn over the kept rows f' whose column k reads
 * bin f (reflect padding, drop-band as in nppc_subband_stage).  scale / D as left by nppc_subband_mean /
 * nppc_subband_stage_bwd, mult = unfold multiplicity [F].  A gather without atomics: bit-identical on repeat. */
int nppc_subband_unfold_bwd(int prec, const void* dx, const float* scale, const double* D, const float* mult, void* dX0,
                            int ldX, int B, int F, int Tp, int Tv, int nb, int G, int KX, void* stream);
int nppc_sb_head(int prec, const void* h2, const void* wh, const float* bias, float* out, long Nseq, int Tn, int la,
                 int Hd, int O, int Fo, void* stream);
int nppc_sb_head_bwd(int prec, const float* dout, const void* whT, const void* h2, void* dh2, float* dWh, float* dbh,
                     long Nseq, int Tn, int la, int Hd, int O, int Fo, void* stream);

/* ---- sub-band sequence model: nn.LSTM(I,H,2) -----------------------------------------------------------------
 * audio_zen/model/module/sequence_model.py:30-37 (construction), :113-123 (forward) and its autograd */
int nppc_lstm2_packed_elems(int I, int H, long* n1, long* n2, int* kx);
int nppc_lstm2_pack_weights(int prec, const float* w_ih0, const float* w_hh0, const float* b_ih0, const float* b_hh0,
                            const float* w_ih1, const float* w_hh1, const float* b_ih1, const float* b_hh1, int I, int H,
                            void* wp1, void* wp2, float* bias1, float* bias2, void* stream);
/* x [Tn][N][kx]; h2 [Tn][N][H] time-major; when train also h1, c1, c2 [Tn][N][H] and g1, g2 [Tn][N][H][4] (i,g,f,o) */
int nppc_lstm2_fwd(int prec, int train, int mtile, const void* x, const void* wp1, const void* wp2, const float* bias1,
                   const float* bias2, void* h2, void* h1, void* g1, void* g2, void* c1, void* c2, long N, int Tn, int I,
                   int H, void* stream);
/* Cooperative forward: G workgroups (CUs) share a tile of 16*mtile sequences and split the hidden units, each streaming
 * 1/G of the weights; h slices cross CUs through `xch` with bounded-spin epoch flags.  `flags` (caller-owned, at least
 * clusters*2*G + 4 words, zero-initialised ONCE by the caller) = the epoch words, which every launcher of this family
 * zeroes itself, followed by the STICKY hand-off time-out counter flags[clusters*2*G]: a workgroup whose bounded spin
 * gives up adds 1 to it and carries on with wrong numbers; no launcher ever clears it, so a host read at any later time
 * sees a time-out of any earlier launch on this flag block.  The caller clears it (a 4-byte memset) after handling it.
 * Same tensor contract as nppc_lstm2_fwd. */
int nppc_lstm2_coop_plan(int prec, int train, long N, int H, int n_cu, int* G, int* mtile, int* clusters);
int nppc_lstm2_fwd_coop(int prec, int train, int G, int mtile, const void* x, const void* wp1, const void* wp2,
                        const float* bias1, const float* bias2, void* h2, void* h1, void* g1, void* g2, void* c1, void* c2,
                        void* xch, long xch_bytes, unsigned* flags, long N, int Tn, int I, int H, void* stream);
/* the same with the output head fused (SequenceModel.forward's fc_output_layer, sequence_model.py:119-123): the CU pair
 * also leaves hpart [2][Tn][N][O] fp32 = per-CU partial sums of h2[t][n][:] . whp[o][:] (whp [16][H], rows >= O zero);
 * nppc_sb_head_finalize adds them and the bias and writes out[bo][o][fo][t - la] like nppc_sb_head (O <= 16).
 * Inference (train = 0): h2 is not stored at all (h2 .. c2 may be null); training keeps the saved state. */
int nppc_lstm2_fwd_coop_head(int prec, int train, int mtile, const void* x, const void* wp1, const void* wp2,
                             const float* bias1, const float* bias2, void* h2, void* h1, void* g1, void* g2, void* c1, void* c2,
                             void* xch, long xch_bytes, unsigned* flags, long N, int Tn, int I, int H, const void* whp,
                             float* hpart, int O, int x_ld /* row stride of x in elements: 0 or 64 = [Tn][N][64]; a packed width
                             (multiple of 8, I < x_ld <= 64): only x_ld columns per row are fetched (the frozen restorer's input,
                             staged 40 wide: -37 % of its bytes) */, void* stream);
int nppc_sb_head_finalize(const float* hpart, int G, const float* bias, float* out, long Nseq, int Tn, int la, int O, int Fo,
                          void* stream);
/* Weight-STATIONARY forward of the same LSTM (sequence_model.py:113-123; bf16, H = 384, I <= 64; any N, the last 32-sequence chunk may be ragged): clusters of
 * 12 CUs keep all weights in registers for the whole launch and exchange the hidden state instead (csrc/lstm_ws.hip).
 * nppc_lstm2_ws_plan: clusters == 0 -> not applicable.  wp1 / wp2: nppc_lstm2_ws_pack of the fp32 weights.
 * train = 0: h1 / h2 are [2][N][H] exchange rings and g / c may be null; train = 1: the saved state of nppc_lstm2_fwd
 * (h1 / h2 [Tn][N][H] double as the exchange medium).  cst: clusters * nch_max * 2048 floats of scratch; flags: clusters *
 * nch_max * 16 + 4 u32, the last 4 behind the epochs hold the sticky time-out counter (never cleared here).
 * whp != null: hpart [Tn][N][O] fp32 = h2[t][n][:] . whp[o][:] (finish with nppc_sb_head_finalize, G = 1). */
int nppc_lstm2_ws_plan(int prec, long N, int H, int I, int n_cu, int* clusters, int* nch_max);
int nppc_lstm2_ws_packed_elems(long* n1, long* n2);
int nppc_lstm2_ws_pack(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1, int I, void* wp1, void* wp2,
                       void* stream);
int nppc_lstm2_fwd_ws(int train, const void* x, const void* wp1, const void* wp2, const float* bias1, const float* bias2, void* h1,
                      void* h2, void* g1, void* g2, void* c1, void* c2, float* cst, unsigned* flags, const void* whp, float* hpart,
                      int O, long N, int Tn, int clusters, int nch_max, void* stream);
/* cooperative backward (bf16, H = 384): CU pairs share 32 sequences, each owns half the hidden units / output columns */
int nppc_lstm2_coop_bwd_packed_elems(long* n);
int nppc_lstm2_coop_bwd_pack(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1, int I, void* wb1,
                             void* wb2, void* stream);
int nppc_lstm2_bwd_coop(const void* g1, const void* g2, const void* c1, const void* c2, const void* dh2, const void* wb1,
                        const void* wb2, void* dx, void* dg1, void* dg2, void* xch, long xch_bytes, unsigned* flags, long N,
                        int Tn, int n_cu, void* stream);
/* K-split variant of the cooperative backward (each CU multiplies its own gate-gradient half with all output columns and
 * the pair exchanges bf16 partial sums, accumulator to accumulator: 38 KB per step instead of 96 KB); same tensor contract,
 * except flags: ceil(N / 32) * 48 + 4 u32 ([cluster][layer 2][CU 2][wave 12] epochs -- every wave hands off its own tiles --
 * followed by the 4 sticky time-out words); xch: ceil(N / 32) * 2 * 2 * 2 * 32 * 384 bf16 */
int nppc_lstm2_coop_bwd2_packed_elems(long* n);
int nppc_lstm2_coop_bwd2_pack(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1, int I, void* wb1,
                              void* wb2, void* stream);
int nppc_lstm2_bwd_coop2(const void* g1, const void* g2, const void* c1, const void* c2, const void* dh2, const void* wb1,
                         const void* wb2, void* dx, void* dg1, void* dg2, void* xch, long xch_bytes, unsigned* flags, long N,
                         int Tn, int n_cu, void* stream);
/* the same with the head backward fused: instead of dh2 the kernel takes the dY rows dyt [Tn][N][16] bf16
 * (nppc_head_dy_gather: dout [B'][O][Fo][Tn - la] -> rows, zero beyond O and before the look-ahead) and the packed head
 * weights whT [H][32] ([u][o]) and forms d h2 += dY . Wh itself; nppc_sb_head_bwd_w is the weight / bias half of
 * nppc_sb_head_bwd (no dh2 output). */
int nppc_lstm2_bwd_coop2_head(const void* g1, const void* g2, const void* c1, const void* c2, const void* dyt, const void* whT,
                              const void* wb1, const void* wb2, void* dx, void* dg1, void* dg2, void* xch, long xch_bytes,
                              unsigned* flags, long N, int Tn, int n_cu, void* stream);
/* The same K-split backward on FOUR-CU clusters of 64 sequences (each CU owns 96 hidden units and streams a quarter of the weight
 * fragments per step; three bf16 partial-sum shipments per layer and step, accumulator to accumulator, per-wave epochs).  Same
 * tensor contract as nppc_lstm2_bwd_coop2 / _head: dh2 != null, or dh2 == null with the fused head's dyt + whT.  Needs
 * ceil(N / 64) * 4 <= n_cu.  nppc_lstm2_coop_bwd4_sizes: elements of each packed weight buffer (nppc_lstm2_coop_bwd4_pack),
 * bytes of xch and u32 words of flags (epochs + the 4 sticky time-out words) for N sequences. */
int nppc_lstm2_coop_bwd4_sizes(long N, long* packed_elems, long* xch_bytes, long* flag_words);
int nppc_lstm2_coop_bwd4_pack(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1, int I, void* wb1,
                              void* wb2, void* stream);
int nppc_lstm2_bwd_coop4(const void* g1, const void* g2, const void* c1, const void* c2, const void* dh2, const void* dyt,
                         const void* whT, const void* wb1, const void* wb2, void* dx, void* dg1, void* dg2, void* xch,
                         long xch_bytes, unsigned* flags, long N, int Tn, int n_cu, void* stream);
int nppc_head_dy_gather(const float* dout, void* dyt, long Nseq, int Tn, int la, int O, int Fo, void* stream);
int nppc_sb_head_bwd_w(int prec, const float* dout, const void* h2, float* dWh, float* dbh, long Nseq, int Tn, int la, int Hd,
                       int O, int Fo, void* stream);
int nppc_lstm2_bwd_packed_elems(int I, int H, long* n1, long* n2);
int nppc_lstm2_pack_weights_bwd(int prec, const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1,
                                int I, int H, void* wb1, void* wb2, void* stream);
/* dh2 [Tn][N][H] -> dx [Tn][N][kx], gate gradients dg1/dg2 [Tn][N][4H] (column k = unit*4 + gate in i,g,f,o order) */
int nppc_lstm2_bwd(int prec, const void* g1, const void* g2, const void* c1, const void* c2, const void* dh2,
                   const void* wb1, const void* wb2, void* dx, void* dg1, void* dg2, long N, int Tn, int I, int H,
                   void* stream);

/* ---- Gram-Schmidt on the K complex directions + NPPC loss ----------------------------------------------------
 * nppc_audio/pc_wrapper.py:8-44 (gram_schmidt_to_crm), nppc_audio/trainer.py:259-317 (base_step) */
int nppc_gram(const float* a, const float* b_or_null, const float* gt, const float* pred, double* out, int B, int K,
              long N, void* stream);
int nppc_combine(const float* a, const double* M1, const float* b, const double* M2, const float* gt, const float* pred,
                 float* out, int B, int K, long N, void* stream);
int nppc_gs_solve(const double* G, double* C, double* Ch, int B, int K, int KV, void* stream);
int nppc_gs_bwd_solve(const double* G, const double* P, const double* Ch, double* D, int B, int K, int KV, void* stream);
int nppc_loss_solve(const double* G, float* err_norm, float* proj_re, float* proj_im, float* proj_mag, float* w_norms,
                    float* reconst, float* sm, double* coefA, double* coefE, int B, int K, void* stream);
int nppc_loss_solve_eps(const double* G, float* err_norm, float* proj_re, float* proj_im, float* proj_mag, float* w_norms,
                        float* reconst, float* sm, double* coefA, double* coefE, int B, int K, double eps, int eps_in_norms,
                        void* stream);
/* the same, which also leaves the step's objective = mean_b reconst + lam * mean_{b,i} sm (trainer.py:300-304) in objective[0]:
 * one workgroup, B <= 1024 (NPPC_EUNSUPPORTED beyond) */
int nppc_loss_solve_obj(const double* G, float* err_norm, float* proj_re, float* proj_im, float* proj_mag, float* w_norms,
                        float* reconst, float* sm, double* coefA, double* coefE, int B, int K, double eps, int eps_in_norms,
                        float lam, float* objective, void* stream);
int nppc_loss_bwd_coef(const double* coefA, const double* coefE, const float* grec, float gobj_over_B, float gsm, double* M1,
                       int B, int K, void* stream);
/* the same with the upstream gradient of the objective read from DEVICE memory (gobj, one float): the coefficients are
 * (gobj * inv_B, gobj * sm_weight); autograd's backward then never reads a scalar back to the host */
int nppc_loss_bwd_coef_dev(const double* coefA, const double* coefE, const float* grec, const float* gobj, float inv_B,
                           float sm_weight, double* M1, int B, int K, void* stream);

/* ---- optimizer: torch.optim.Adam (nppc_audio/trainer.py:64-69,102-104) -------------------------------------- */
int nppc_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                   double wd, int step, double gscale, void* stream);
/* the same, guarded: `guards` = device array of n_guards device pointers to the sticky hand-off time-out counters of the
 * cooperative LSTM launches; if any is non-zero the update is skipped (p, m, v untouched) and *poison (nullable, the step's
 * objective) becomes NaN -- wrong numbers never reach the weights between two host checks of the counters */
int nppc_adam_step_guarded(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                           double wd, int step, double gscale, const void* guards, int n_guards, float* poison, void* stream);

/* ---- on-device batch synthesis (dataset/audio_dataset.py:92-152: dBFS normalisation, SNR mix, clip guard) -------
 * target_item (nullable): per-clip normalisation level [B] in dBFS (the reference's target_dB_FS_floating_value > 0
 * draws one per item, :94-101); null = target_dbfs for every clip */
int nppc_mix_snr(const float* clean, const float* noise, const float* snr_db, float target_dbfs, const float* target_item,
                 float* noisy_out, float* clean_out, int B, int L, void* stream);

/* inpainting batch synthesis (dataset/audio_dataset_inpainting.py __getitem__ :291-313), one launch per batch:
 * _normalize_audio (:154-168, when do_norm), the gap mask of _create_random_mask (:170-181: zeros on
 * [gap_start[b], gap_end[b])) applied to the audio (masked_out, nullable), and time_to_spec_mask (:223-251, centred)
 * for that gap -> mask_frames [B, T]. */
int nppc_inpaint_prepare(const float* clean, const int* gap_start, const int* gap_end, int do_norm, float target_dbfs,
                         float* clean_out /*nullable*/, float* masked_out /*nullable*/, float* mask_frames, int B, int L,
                         int win, int hop, int T, void* stream);
/* time_to_spec_mask (:223-251) for an arbitrary sample mask [B, L]: frame = 1 iff every sample of its clamped window is 1 */
int nppc_time_to_spec_mask(const float* mask_time, float* mask_frames, int B, int L, int win, int hop, int center, int T,
                           void* stream);
/* utils.audio_to_stft (utils.py:150-175) for any nfft = win_length <= 512: [B, L] -> spec [B, 2, F, T] (T = 1 + L / hop);
 * masked_spec (nullable) = spec * mask_frames[b, t] (audio_dataset_inpainting.py:307-310) */
int nppc_stft_pair(const float* wave, const float* mask_frames /*nullable*/, float* spec, float* masked_spec /*nullable*/,
                   int B, int L, int nfft, int hop, void* stream);

/* ---- inpainting dataset on the device (csrc/inpaint_data.hip; specification tests/vad_ref.py) ------
 * What AudioInpaintingDataset.__getitem__ (:253-293) does before the STFT, for a batch, from a corpus that stays in HBM:
 * corpus = every decoded file back to back, file f = corpus[offsets[f], offsets[f + 1]) with the gain gains[f] of its
 * whole-file _normalize_audio.  Item b is cut from file file_index[b] (at least L samples long):
 *   crop_start = uniform_int(0, len - L) when random_crop and len > L, else 0;  clean[b] = crop * gain (nullable);
 *   dbfs_float > 0 multiplies the gain by 10^(d / 20), d uniform in +-dbfs_float (target_dB_FS_floating_value);
 *   use_vad: an energy voice-activity detector over W = L / win windows (win a multiple of 64; W <= 2048, above that
 *   NPPC_EUNSUPPORTED): level e_w = 10 log10(mean x^2 + 1e-12), floor = nearest-rank floor_percentile of the levels,
 *   peak = their maximum, theta_on = max(floor + on_db, peak - range_db), theta_off = theta_on - hysteresis_db, no
 *   segment when peak - floor < on_db; segments by the state machine of silero's get_speech_timestamps (min_silence in
 *   samples, minimum length = missing, no padding) -> segments [B][s_max][2] (-1 past n_segments[b]; W <= 2 s_max <= 2048);
 *   gap (_create_mask :199-221): a uniformly chosen segment, gap_start = its start + uniform_int(0, its length - missing)
 *   when it is longer than missing; otherwise, and always without use_vad, the fallback (_create_random_mask):
 *   fixed_start when >= 0, else uniform_int(0, L - missing).  used_fallback [B] = 1 for the fallback (-1: file_index[b]
 *   does not name a file of at least L samples; nothing was read, clean[b] = 0).
 * Random numbers: Philox4x32-10, key = seed, counter (item_index[b], epoch, 0, purpose), purpose 0 crop start, 1 segment,
 * 2 gap offset, 3 level; uniform_int(0, n) = the high 32 bits of word0 * (n + 1).  One workgroup per item, no atomics: an
 * item's result does not depend on the rest of the batch. */
int nppc_inpaint_vad_batch(const float* corpus, long corpus_len, const long* offsets, const float* gains, int n_files,
                           const int* file_index, const int* item_index, int B, int L, int win, int missing, int fixed_start,
                           int use_vad, int random_crop, long seed, int epoch, float dbfs_float, double on_db, double range_db,
                           double hysteresis_db, double floor_percentile, int min_silence, int s_max,
                           float* clean /*nullable*/, int* crop_start /*nullable*/, int* gap_start, int* gap_end, int* segments,
                           int* n_segments, int* used_fallback, void* stream);
/* the gap draw of nppc_inpaint_vad_batch alone, on given segments [B][s_max][2] / n_segments [B] */
int nppc_inpaint_draw_gaps(const int* segments, const int* n_segments, const int* item_index, int B, int L, int missing,
                           int fixed_start, int s_max, long seed, int epoch, int* gap_start, int* gap_end, int* used_fallback,
                           void* stream);

/* ---- MC-dropout + PCA baseline (utils.py:334-648) -----------------------------------------------
 * nn.Dropout(p) (tmp_utils.py:28-29) in place on channels [0, C) of a haloed NHWC activation X [rows][ld]:
 * keep bit = Philox4x32-10(seed; row, channel / 4, stream_id) >= p * 2^32, kept values scaled by 1 / (1 - p);
 * keep_out (nullable) [rows][C] u8 receives the bits. */
int nppc_dropout(int prec, void* X, long ld, long rows, int C, float p, long seed, int stream_id,
                 unsigned char* keep_out /*nullable*/, void* stream);
/* compute_pca_sklearn_batch (utils.py:393-496) for all items at once: X [K][B][D] fp32 (K <= 60 samples per item) ->
 * mean [B][D], comps [B][n][D] (unit, largest-magnitude entry positive), scaled = comps * singular value,
 * svals [B][n], weights = svals / sum(svals) [B][n]; work = *elems of nppc_pca_work_elems doubles. */
int nppc_pca_work_elems(int K, int B, int n, long* elems);
int nppc_pca_batch(const float* X, int K, int B, int D, int n, float* mean, float* comps, float* scaled, float* svals,
                   float* weights, double* work, void* stream);

/* base_step2's projection loss (inpainting/trainer/nppc_trainer.py:285-323): rows w, m [B*K][N] (NPPC directions, scaled MC
 * components), sv [B][K] -> proj, w_norms (= |w| + eps) [B][K], reconst, second [B]; sums [B*K*3] / coef [B*K*3] doubles are
 * workspace kept for nppc_pair_loss_bwd: dw = d(sum_b grec[b] * reconst_b + g_rec_all * sum_b reconst_b
 * + g_sm_all * sum_b second_b) / dw. */
int nppc_pair_loss(const float* w, const float* m, const float* sv, double* sums, float* proj, float* w_norms, float* reconst,
                   float* second, double* coef, int B, int K, long N, double eps, void* stream);
int nppc_pair_loss_bwd(const float* w, const float* m, const double* coef, const float* grec /*nullable*/, float g_rec_all,
                       float g_sm_all, float* dw, int B, int K, long N, void* stream);

/* compute_metrics (inpainting/validator/validator_nppc_model.py:742-828): out [3][N] = {pred - clean, the same on the gap
 * only (mask == 0), (mean - clean) on the gap only}; nppc_rows_gram: G [Ra][Rb] (fp64) = A [Ra][N] . Bm [Rb][N]^T */
int nppc_metric_rows(const float* pred, const float* clean, const float* mean, const float* mask, float* out, long N,
                     void* stream);
int nppc_rows_gram(const float* A, int Ra, const float* Bm, int Rb, long N, double* G, void* stream);

/* clip_grad_norm_(max_norm) + Adam without a host round trip (inpainting/trainer/nppc_trainer.py:149-154):
 * nppc_sumsq accumulates sum(g^2) into a zeroed device double, nppc_adam_step_clip reads it. */
int nppc_sumsq(const float* g, long n, double* out, void* stream);
int nppc_adam_step_clip(float* p, const float* g, float* m, float* v, long n, double lr, double b1, double b2, double eps,
                        double wd, int step, double gscale, const double* sumsq, double max_norm, void* stream);

/* ---- inpainting sibling: U-Net on haloed NHWC activations ------------------------------------------------------
 * nppc_audio/inpainting/networks/unet.py:247-313, tmp_utils.py:8-99 (conv3x3 + BatchNorm2d + LeakyReLU(0.2),
 * MaxPool2d(2), bilinear x2 align_corners + pad + cat, conv1x1), utils.py:273-306 (log-magnitude, batch-global
 * mean / unbiased std), inpainting/nppc/pc_wrapper.py:75-84 and unet.py:299-312 (mask blending).
 * Activations: X[(b*(H+2)+y)*(W+2)+x][ld], zero halo, zero guard rows; see csrc/unet.hip. */
int nppc_logmag(const float* spec, float* out, long out_bstride, int B, long FT, double* st, void* stream);
int nppc_standardize(float* a, float* b_or_null, long bstride, int B, long FT, const double* st, float* mean_std, void* stream);
int nppc_unet_stage_map(int prec, const float* src, long src_bstride, void* dst, long ld, int c, int B, int H, int W,
                        void* stream);
int nppc_conv_pack(int prec, const float* w, void* wf, void* wb, int Cout, int Cin, int ksize, int Np, int Cinp, int Mb,
                   int Coutp, void* stream);
int nppc_conv_fwd(int prec, const void* A, long lda, const void* Wp, void* C, long ldc, const float* bias, const float* scale,
                  const float* shift, float slope, int B, int H, int W, int Cin, int Cout, int Np, int ksize, void* stream);
/* the same convolution without the folded-BatchNorm epilogue, which also leaves the column sums (sum, sum of squares) of every
 * 128-row tile of its STORED output in stat_part [ceil(B (H+2) (W+2) / 128)][2][Np] (fp32): the batch statistics of the
 * train-mode BatchNorm that follows (tmp_utils.py:8-37) come from nppc_bn_stats_from_parts instead of from a pass over the
 * tensor (nppc_bn_stats).  Tiled-kernel shapes only (Cin % 64 == 0 in bf16, % 32 in fp32; NPPC_EUNSUPPORTED otherwise).
 * nppc_bn_stats_from_parts: st[c] = sum x, st[C + c] = sum x^2 (fp64, plain stores: no initial state, fixed summation order);
 * scratch: 2 * C * 128 doubles. */
int nppc_conv_fwd_stats(int prec, const void* A, long lda, const void* Wp, void* C, long ldc, const float* bias, int B, int H, int W,
                        int Cin, int Cout, int Np, int ksize, float* stat_part, void* stream);
int nppc_bn_stats_from_parts(const float* stat_part, int B, int H, int W, int Np, int C, double* st, double* scratch, void* stream);
int nppc_conv_wgrad(int prec, const void* dY, long lddy, const void* X, long ldx, float* slabs, int M, int N, int B, int H, int W,
                    int ksize, int ksplit, void* stream);
int nppc_conv_wgrad_transposed(int M, int N);
int nppc_conv_wgrad_reduce(int prec, const float* slabs, int ksplit, int M, int N, float* dW, int Cout, int Cin, int ksize,
                           void* stream);
/* The thin ends of the U-Net (unet.py:247-262 `inc`: conv3x3 from 1-2 channels; `outc`: conv1x1 64 -> K <= 8; tmp_utils.py:8-37):
 * memory-bound products that the MFMA path computes 32-64 channels wide.  Direct kernels, same haloed NHWC tensors and the same
 * results as nppc_conv_fwd / nppc_conv_wgrad + _reduce / the transposed nppc_conv_fwd, but w / dW are the fp32 parameter
 * tensors in torch layout ([Cout][Cin][kh][kw], no packing) and the products accumulate in fp32.  part: workspace of
 * nppc_conv_thin_part_elems floats.  3x3: Cin 1 or 2, Cout % 8 == 0, <= 64; 1x1: Cin == 64, K <= 8. */
int nppc_conv_thin_part_elems(long* n);
int nppc_conv3x3_thin_fwd(int prec, const void* A, long lda, const float* w, const float* bias, const float* scale,
                          const float* shift, float slope, void* C, long ldc, int B, int H, int W, int Cin, int Cout, void* stream);
int nppc_conv3x3_thin_wgrad(int prec, const void* dY, long lddy, const void* X, long ldx, float* part, float* dW, int B, int H,
                            int W, int Cin, int Cout, void* stream);
int nppc_conv1x1_thin_fwd(int prec, const void* X, long ldx, const float* w, const float* bias, void* C, long ldc, int B, int H,
                          int W, int Cin, int K, void* stream);
int nppc_conv1x1_thin_bwd_data(int prec, const void* dY, long lddy, const float* w, void* dX, long lddx, int B, int H, int W,
                               int Cin, int K, void* stream);
int nppc_conv1x1_thin_wgrad(int prec, const void* dY, long lddy, const void* X, long ldx, float* part, float* dW, int B, int H,
                            int W, int Cin, int K, void* stream);
int nppc_bn_stats(int prec, const void* X, long ld, long P, int C, double* st, void* stream);
int nppc_bn_finalize(const double* st, const float* gamma, const float* beta, float* rmean, float* rvar, float* ss, int C,
                     double n, float eps, float momentum, int train, void* stream);
int nppc_bn_act(int prec, const void* X, long ldx, void* Y, long ldy, const float* ss, int C, int B, int H, int W, float slope,
                void* stream);
/* (Y is accepted and not read since round 4: the LeakyReLU mask is recomputed from X with bn_act's own expression) */
int nppc_bn_bwd(int prec, const void* dyA, long ldA, const void* dyB, long ldB, const void* Y, long ldy, const void* X, long ldx,
                const float* ss, double* S, void* dX, long lddx, float* dgamma, float* dbeta, int C, int B, int H, int W,
                float slope, void* stream);
/* nppc_bn_bwd for a block whose output went through nn.Dropout(p) in place (nppc_dropout with the same seed / stream_id):
 * the keep bits are regenerated from Philox4x32-10(seed; pixel row, channel / 4, stream_id), not read from memory, and
 * g = (dyA + dyB) * keep / (1 - p) before the LeakyReLU slope.  p = 0 gives nppc_bn_bwd's result bit for bit. */
int nppc_bn_bwd_dropout(int prec, const void* dyA, long ldA, const void* dyB, long ldB, const void* Y, long ldy, const void* X,
                        long ldx, const float* ss, double* S, void* dX, long lddx, float* dgamma, float* dbeta, int C, int B,
                        int H, int W, float slope, float p, long seed, int stream_id, void* stream);
int nppc_maxpool2(int prec, const void* X, long ldx, void* Y, long ldy, unsigned char* idx, int C, int B, int H, int W,
                  void* stream);
int nppc_maxpool2_bwd(int prec, const void* dY, long ldy, const unsigned char* idx, void* dX, long ldx, int C, int B, int H, int W,
                      void* stream);
int nppc_upsample2(int prec, const void* X, long ldx, void* Y, long ldy, int C, int B, int Hi, int Wi, int Ht, int Wt,
                   void* stream);
int nppc_upsample2_bwd(int prec, const void* dY, long ldy, void* dX, long ldx, int C, int B, int Hi, int Wi, int Ht, int Wt,
                       void* stream);
int nppc_unet_out(int prec, const void* raw, long ld, const float* mask, const float* xin, long xin_bstride, float* out,
                  long out_pstride, int K, int B, int H, int W, int mode, void* stream);
int nppc_unet_out_bwd(int prec, const float* dout, long dout_pstride, const float* mask, void* draw, long ld, int K, int B,
                      int H, int W, void* stream);

/* ---- restorer trainer (inpainting/trainer/restoration_trainer.py:189-191) ---------------------------------------------
 * masked spectral MSE: out, clean [B][F][T] fp32, mask [B][T] (1 = known), broadcast over F:
 * *loss = sum (out - clean)^2 (1 - m) / (F sum (1 - m) + 1e-6), fp64 partials folded in a fixed order (no float atomics,
 * bit-identical on repeat).  work = *elems of nppc_masked_mse_work_elems doubles; it keeps the denominator for the
 * backward, dout = 2 g (out - clean) (1 - m) / den with g (the incoming gradient of the loss) read from device memory. */
int nppc_masked_mse_work_elems(long* elems);
int nppc_masked_mse(const float* out, const float* clean, const float* mask, int B, int F, int T, double* work, float* loss,
                    void* stream);
int nppc_masked_mse_bwd(const float* out, const float* clean, const float* mask, const float* g, const double* work,
                        float* dout, int B, int F, int T, void* stream);

/* ---- speech-enhancement restorer trainer (Trainer_Finetune._train_epoch, trainer.py:337-343) -------------------------
 * cIRM MSE: noisy / clean STFT nr, ni, cr, ci [B][F][T] fp32, model output crm [B][2][Fo][T] in drop-band order (G groups,
 * Fo = (F - F % G) / G, G = 1: no drop-band).  The compressed cIRM target is built per element as
 * nppc_cirm_build_compress does; gt (nullable) receives it.  *loss = mean (gt - crm)^2 over the 2 B Fo T elements, fp64
 * partials folded in a fixed order (no float atomics, bit-identical on repeat); work = *elems of nppc_crm_mse_work_elems
 * doubles.  Backward: dcrm = 2 g (crm - gt) / N, g (the incoming gradient of the loss) read from device memory. */
int nppc_crm_mse_work_elems(long* elems);
int nppc_crm_mse(const float* nr, const float* ni, const float* cr, const float* ci, const float* crm, float* gt /*nullable*/,
                 int B, int F, int T, int G, float eps, double* work, float* loss, void* stream);
int nppc_crm_mse_bwd(const float* nr, const float* ni, const float* cr, const float* ci, const float* crm, const float* g,
                     float* dcrm, int B, int F, int T, int G, float eps, void* stream);

/* ---- speech-enhancement metrics (audio_zen/metrics.py:61-85 SI_SDR + :88-89 STOI; model_validator.py:56-65) ----------
 * Ragged batches: rows [B][ld] fp32 padded, lengths[B] (device int); no sample past an item's length is read, one item's
 * values do not depend on the rest of the batch, no atomics (bit-identical on repeat).  All arithmetic after the fp32 input
 * samples is fp64.
 * SI-SDR: out[B][2] = (audio_zen SI_SDR, ModelValidator's mean-removed SI-SDR); sums (nullable) [B][9] = sum s, sum e,
 * sum s^2, sum e^2, sum s e, sum s~^2, sum e~ s~, sum (e - a1 s)^2, sum (a2 s~ - e~)^2 (s = ref, e = est, ~ = mean removed). */
int nppc_sisdr_sums(const float* ref, const float* est, const int* lengths, int B, long ld, double* sums /*nullable*/,
                    double* out, void* stream);
/* scipy.signal.resample_poly(x, up, down, window=h): h [ntaps] fp64 (<= 4096 taps, odd length), y [B][ldy] fp64, item b
 * gets ceil(lengths[b] up / down) samples (clipped to ldy), zeros after them */
int nppc_resample_poly(const float* x, const int* lengths, int B, long ldx, const double* h, int ntaps, int up, int down,
                       double* y, long ldy, void* stream);
/* STOI at 10 kHz (DESIGN.md "Speech-enhancement metrics"), on the resampled clean xr / estimate yr [B][ldr], lr[B] = their
 * lengths, nfr >= every item's frame count max(0, ceil((lr - 256) / 128)):
 * frames: energy [B][nfr] of the windowed clean frames (dB), slot [B][nfr] = kept position or -1, kidx [B][nfr] = frame of
 *         the k-th kept frame (-1 past K), K [B] = kept frames;
 * bands:  third-octave magnitudes x_tob, y_tob [B][15][nfr] of the K - 1 STFT frames of the silence-removed signals;
 * corr:   out [B] = STOI, 1e-5 for items with fewer than 30 STFT frames */
int nppc_stoi_frames(const double* xr, const int* lr, int B, long ldr, int nfr, double* energy, int* slot, int* kidx, int* K,
                     void* stream);
int nppc_stoi_bands(const double* xr, const double* yr, long ldr, const int* kidx, const int* K, int B, int nfr, double* x_tob,
                    double* y_tob, void* stream);
int nppc_stoi_corr(const double* x_tob, const double* y_tob, const int* K, int B, int nfr, double* out, void* stream);

/* ---- BSS-eval SDR (csrc/bss_eval.hip, DESIGN.md section 7d "BSS-eval SDR"; audio_zen/metrics.py:56-58 = mir_eval's
 * bss_eval_sources for one source) and _scale_bss_eval (audio_zen/metrics.py:8-53) --------------------------------------
 * Same ragged convention as above.  Per item, s = ref, e = est, n = lengths[b], 1 <= P <= 512 the filter length,
 * M = n + P - 1: r[t] = sum_m s[m] s[m - t], d[t] = sum_m e[m] s[m - t] (t < P), toeplitz(r) c = d,
 * proj[m] = sum_t c[t] s[m - t], num = sum_{m < M} proj^2, den = sum_{m < M} (e - proj)^2 (e = 0 at m >= n),
 * SDR = 10 log10(num / den), +inf when den == 0.  All fp64, no atomics, partial sums added in ascending order. */
/* chunk sizes (samples per workgroup of the corr kernel, samples it stages in LDS at a time, output samples per workgroup
 * of the project kernel) and the doubles of workspace PER ITEM the corr and project launches need; no GPU needed; output
 * pointers may be null.  P > 512 is NPPC_EUNSUPPORTED. */
int nppc_bss_shape(long ld, int P, int* corr_chunk, int* corr_tile, int* proj_chunk, long* corr_elems_per_item,
                   long* proj_elems_per_item);
/* part [B][ceil(ld / corr_chunk)][2][P]: the r and d sums of every chunk of m that starts inside the item (rows of chunks
 * past the item's length are not written, and not read by the solve) */
int nppc_bss_corr(const float* ref, const float* est, const int* lengths, int B, long ld, int P, double* part,
                  long part_elems, void* stream);
/* part of nppc_bss_corr -> r, d, c [B][P] (Levinson-Durbin, one workgroup per item), status [B]: 0, or 1 when r[0] <= 0
 * (an all-zero reference), a prediction error is not positive or a value is not finite */
int nppc_bss_solve(const double* part, const int* lengths, int B, long ld, int P, double* r, double* d, double* c,
                   int* status, void* stream);
/* c, status -> num, den, sdr [B]; part [B][ceil((ld + P - 1) / proj_chunk)][2] is workspace.  status != 0: all three NaN. */
int nppc_bss_project(const float* ref, const float* est, const int* lengths, int B, long ld, int P, const double* c,
                     const int* status, double* part, long part_elems, double* num, double* den, double* sdr,
                     void* stream);
/* _scale_bss_eval(compute_sir_sar=False) per item, alpha = <s, e> / |s|^2: out [B][4] = si_sdr = 10 log10(|alpha s|^2 /
 * |e - alpha s|^2), sd_sdr = snr + 10 log10(alpha^2), snr = 10 log10(|s|^2 / |e - s|^2), srr = -10 log10((1 - 1 / alpha)^2);
 * sums (nullable) [B][4] = |s|^2, <s, e>, |e - s|^2, |e - alpha s|^2, each summed directly */
int nppc_bss_scale(const float* ref, const float* est, const int* lengths, int B, long ld, double* sums /*nullable*/,
                   double* out, void* stream);


/* ---- ragged inference of the FullSubNet+ restorer (csrc/ragged.hip; STFT / iSTFT in csrc/frontend.hip, TSSE front in
 * csrc/spec.hip) ---------------------------------------------------------------------------------------
 * A padded batch: item b is L_b = lengths[b] samples (device int[B]) and T_b = 1 + L_b / hop frames; frames[b] (device
 * int[B]) = T_b.  Item b's results equal the uniform entry point's for that item alone; nothing past an item's end is
 * read, and what is written past it is 0.  No float atomics (bit-identical on repeat).
 * STFT: wave [B][ld] (ld >= Lmax) -> re, im, mag (nullable) [B][F][T], T = 1 + Lmax / hop; frames t >= T_b are 0.
 * iSTFT: torch.istft(length=L_b) of the item's T_b frames: re, im [B][F][T] -> out [B][ld], samples >= L_b are 0. */
int nppc_stft_ragged(const float* wave, long ld, const int* lengths, float* re, float* im, float* mag /*nullable*/, int B, int T,
                     int nfft, int hop, void* stream);
int nppc_istft_ragged(const float* re, const float* im, float* out, long ld, const int* lengths, int B, int T, int nfft, int hop,
                      void* stream);
/* inference form of nppc_tsse_fwd_maps (no saved tensors): item b's laplace mean over F x (T_b + la), each TSSE conv pooled
 * over its T_b + la - k + 1 outputs; X0 rows t < T_b = scaled map, rows T_b <= t < Tp written as 0 */
int nppc_tsse_fwd_maps_ragged(int prec, const float* const* maps, int nmaps, double* rowsum, const float* cw0, const float* cb0,
                              const float* cw1, const float* cb1, const float* cw2, const float* cb2, int ks0, int ks1, int ks2,
                              const float* fcw, const float* fcb, const float* w1, const float* b1, const float* w2,
                              const float* b2, long sW, float* scale, void* X0, long sY, const int* frames, int B, int C, int T,
                              int look_ahead, int Tp, int ld, void* stream);
/* TCN depthwise stage of nppc_tcn_dwconv per item: the centred conv sees zeros at and past Tv_b = T_b + la (as it sees them
 * past Tv in the uniform launch), rows t >= Tv_b are written as 0; it accumulates no statistics. */
int nppc_tcn_dwconv_ragged(int prec, const void* in, void* out, const double* st1, const float* gamma, const float* beta,
                           const float* wd, const float* bd, const float* slope2, const int* frames, int la, int B, int Cc, int ld,
                           int Tp, int Tv, int dil, float eps, long sAct, long sSt, long sP, int batch, void* stream);
/* GroupNorm(1, C) sums (sum, sumsq) [batch][B][2] of the stored activation act [batch][B][Tp][ld] over item b's rows
 * t < T_b + la, scaled by Tv / (T_b + la): consumers that divide by C * Tv get the item's own mean and variance.  The
 * sums are overwritten. */
int nppc_tcn_gn_stats_ragged(int prec, const void* act, double* stats, const int* frames, int la, int B, int Cc, int ld, int Tp,
                             int Tv, long sAct, long sSt, int batch, void* stream);
/* nppc_subband_mean per item over its T_b + la frames (no workspace, no atomics) */
int nppc_subband_mean_ragged(int prec, const void* src, int ldS, const void* fb, int ldF, long strideFb, const float* mult,
                             float* scale, const int* frames, int la, int B, int F, int Tp, int Tv, int nfeat, void* stream);
/* x [B][rows][T] fp32: x[b][r][t] = 0 for t >= frames[b] (the output crop of the ragged forward) */
int nppc_crop_frames_ragged(float* x, long rows, int T, const int* frames, int B, void* stream);
/* per-item cIRM MSE, no drop-band: loss[b] (fp64) = mean over [2][F][T_b] of (gt - crm)^2, gt as in nppc_crm_mse;
 * nr, ni, cr, ci [B][F][T], crm [B][2][F][T] */
int nppc_crm_mse_ragged(const float* nr, const float* ni, const float* cr, const float* ci, const float* crm, const int* frames,
                        int B, int F, int T, float eps, double* loss, void* stream);

/* ---- ragged NPPC validation step (csrc/nppc_ragged.hip) ------------------------------------------------
 * Item b of a padded batch lives in frames t < T_b = frames[b] (device int[B]) of planes [..][F][T].  Its results equal
 * those of the item alone (B = 1, T = T_b) BIT FOR BIT: elements at t >= T_b are never loaded, every sum has one writer
 * and an order that depends on (F, T_b) only (no float or double atomics).  Forward only. */
/* raw magnitude x [B][F][T] -> y [B][Tp][ld] (the sub-band source of the direction net): rows t < T_b transposed, rows
 * T_b <= t < Tp written as 0 */
int nppc_rawmag_stage_ragged(int prec, const float* x, void* y, const int* frames, int B, int F, int T, int Tp, int ld,
                             void* stream);
/* doubles of workspace nppc_gram_ragged needs */
int nppc_gram_ragged_work_elems(int B, int K, int with_e, int F, long* n);
/* out [B][KV][KV] complex double = <a_i, a_n> summed over f < F, t < T_b; a [B][K][2][F][T]; with gt / pred [B][2][F][T]
 * the set has e = gt - pred as index K (KV = K + 1 <= 9).  `out` is overwritten (no need to zero it). */
int nppc_gram_ragged(const float* a, const float* gt /*nullable*/, const float* pred /*nullable*/, double* out, double* work,
                     long work_elems, const int* frames, int B, int K, int F, int T, void* stream);
/* out_i = sum_m M1[b][i][m] a_m on t < T_b, 0 on T_b <= t < T; a, out [B][K][2][F][T], M1 [B][K][K] complex double;
 * K <= 8 (NPPC_EUNSUPPORTED beyond) */
int nppc_combine_ragged(const float* a, const double* M1, float* out, const int* frames, int B, int K, int F, int T,
                        void* stream);
/* nppc_cirm_build_compress without drop-band: out [B][2][F][T], 0 on t >= T_b (inputs not read there) */
int nppc_cirm_build_compress_ragged(const float* nr, const float* ni, const float* cr, const float* ci, float* out,
                                    const int* frames, int B, int F, int T, float eps, void* stream);

/* ---- inpainting validator (csrc/inpaint_validator.hip, DESIGN.md section 8 "Inpainting validator") --------------------
 * nppc_istft_any: torch.istft(n_fft, hop, win_length = n_fft, periodic hann, center=True, length=L) for ANY n_fft <= 512,
 * 1 <= hop <= n_fft, ceil(n_fft / hop) <= 8: re, im [B][F][T] planes, item b at re + b * sb (sb >= F T floats) ->
 * out [B][ld] (ld >= L; nothing past L is written).  Samples at and past n_fft + hop (T - 1) - n_fft / 2 are 0 (torch pads
 * there); frames with t hop >= L + n_fft / 2 are never read.  Direct inverse DFT from LDS, exact twiddle phases, fp64
 * accumulation, every sample gathers its frames in ascending order: no atomics, an item's samples do not depend on the batch.
 * NPPC_EBADARG when the window envelope inside the kept range is below 1e-11 (torch raises there). */
int nppc_istft_any(const float* re, const float* im, long sb, float* out, long ld, int B, int T, int nfft, int hop, int L,
                   void* stream);
/* save_pc_audio_variations (inpainting/validator/validator_nppc_model.py:553-619) without files: pred, clean_norm [B][F][T],
 * pc [B][K][F][T], clean_spec [B][2][F][T], mean / stdev device scalars, alphas [A] (device) ->
 * out [B][K][A][L] = istft(exp((pred + alpha pc_k) stdev + mean) e^{i angle(clean)}),
 * clean_wave [B][L] = istft((exp(clean_norm stdev + mean) - 1e-6) e^{i angle(clean)}); angle(0) = 0.  The K A + 1 complex
 * spectrograms exist in LDS only; same transform, limits and determinism as nppc_istft_any. */
int nppc_pc_variation_waves(const float* pred, const float* pc, const float* clean_norm, const float* clean_spec,
                            const float* mean, const float* stdev, const float* alphas, float* out, float* clean_wave, int B,
                            int K, int A, int T, int nfft, int hop, int L, void* stream);
/* compute_metrics for a batch: G [B][2n+3][2n+3] (fp64) = Gram matrix of item b's rows {nppc [n], mc [n], pred - clean, the
 * same on the gap only, (mean - clean) on the gap only} (the rows of nppc_metric_rows, formed on the fly); nppc, mc
 * [B][n][N], pred, clean, mean, mask [B][N]; n <= 8.  One launch, one workgroup per (row, item), fixed summation order. */
int nppc_metrics_batch(const float* nppc, const float* mc, const float* pred, const float* clean, const float* mean,
                       const float* mask, double* G, int B, int n, long N, void* stream);

/* ---- DNS dynamic mixing (fullsubnet_plus/dataset/dataset_train.py) ------------------------------------------------
 * Batched, ragged, causal, truncated convolution with room impulse responses (:151, fftconvolve(clean, rir)[:L]):
 * out[b][n] = sum_{k = 0..min(n, len_b - 1)} rir[b][k] * clean[b][n - k], len_b = min(rir_len[b], ldr, L); clean, out
 * [B][L], rir [B][ldr], rir_len [B] on the device.  rir_len[b] == 0: out[b] is a bit-exact copy of clean[b].  Nothing at
 * or past rir[b][rir_len[b]] is read.  Direct form in fp64, taps in ascending order: an item's result does not depend
 * on B, ldr or the other items.  out must not alias clean. */
int nppc_rir_convolve(const float* clean, const float* rir, const int* rir_len, float* out, int B, int L, int ldr,
                      void* stream);
/* Dataset.snr_mix after the convolution (:153-182) for a batch: norm_amplitude and tailor_dB_FS(target_dbfs) of clean
 * and noise, SNR scaling by snr_db[b], tailor_dB_FS of the mixture to noisy_target_dbfs[b], and the clip rule (any
 * |noisy| > 0.999: both divided by max|noisy| / (0.99 - 1e-6)); eps = 1e-6 everywhere.  clean, noise, noisy_out,
 * clean_out [B][L]; the outputs must not alias the inputs.  fp64 sums in a fixed order, one workgroup per clip. */
int nppc_dns_snr_mix(const float* clean, const float* noise, const float* snr_db, const float* noisy_target_dbfs,
                     float target_dbfs, float* noisy_out, float* clean_out, int B, int L, void* stream);

/* ---- batched pYIN f0 tracking (csrc/pitch.hip; specification tests/pyin_ref.py) ------------------
 * Supported: 2 <= frame_length <= 2048, 1 <= win_length < frame_length, hop_length >= 1,
 * 1 <= min_period < max_period < frame_length - win_length, n_pitch_bins <= 768, n_thresholds <= 1024; anything else is
 * NPPC_EBADARG.  Item n of y [N][L] has lengths[n] samples (device int [N], nullable: L) and 1 + lengths[n] / hop_length
 * frames of its own; T = 1 + L / hop_length.  No atomics; an item's results do not depend on the batch. */
/* Shapes of a call, without a GPU: min_period = max(floor(sr / fmax), 1), max_period = min(ceil(sr / fmin), frame_length -
 * win_length - 1), P = max_period - min_period + 1, n_pitch_bins = floor(12 ceil(1 / resolution) log2(fmax / fmin)) + 1,
 * width = 2 round(max_transition_rate 12 hop_length / sr) ceil(1 / resolution) + 1 (round half to even), ws_bytes = the
 * bytes of the Viterbi back-pointers [N][T][2 n_pitch_bins] uint16.  Output pointers may be null. */
int nppc_pyin_shape(int N, long L, double sr, double fmin, double fmax, int frame_length, int win_length, int hop_length,
                    double resolution, double max_transition_rate, int* T, int* P, int* min_period, int* n_pitch_bins,
                    int* width, long* ws_bytes);
/* y [N][L] -> dprime [N][T][P] fp32: the cumulative-mean-normalised difference d'(tau), tau = min_period..max_period, of
 * every frame of the signal zero-padded by frame_length / 2 on both sides; d(tau) < 1e-6 counts as 0; rows of frames past
 * an item's own are 0. */
int nppc_pyin_cmnd(const float* y, const int* lengths, float* dprime, int N, long L, int frame_length, int win_length,
                   int hop_length, int min_period, int max_period, void* stream);
/* dprime [N][T][P] -> obs [N][T][2 n_pitch_bins] fp32 (voiced bins, then the unvoiced states) and voiced_prob [N][T];
 * beta_w [n_thresholds] (device, fp64) = the threshold weights.  Rows of frames past an item's own are 0. */
int nppc_pyin_observe(const float* dprime, const int* lengths, const double* beta_w, float* obs, float* voiced_prob, int N,
                      int T, long L, int hop_length, int P, int min_period, int n_thresholds, int n_pitch_bins,
                      int bins_per_semitone, double sr, double fmin, double boltzmann, double no_trough_prob, void* stream);
/* obs -> f0 [N][T] fp32 (NaN where unvoiced), voiced_flag [N][T] uint8; frames past an item's own: NaN / 0.  hmm_tab
 * (device, fp64) = log tri [width], log rowsum [n_pitch_bins], log stay, log switch, log init; backptr = ws_bytes of
 * nppc_pyin_shape. */
int nppc_pyin_viterbi(const float* obs, const int* lengths, const double* hmm_tab, unsigned short* backptr, float* f0,
                      unsigned char* voiced_flag, int N, int T, long L, int hop_length, int n_pitch_bins,
                      int bins_per_semitone, int width, double fmin, void* stream);

/* ---- gap-constrained Griffin-Lim (csrc/gl_gap.hip; specification tests/gl_gap_ref.py) ------------
 * Phase retrieval for the gap frames of an inpainted spectrogram: the target magnitude holds on the gap frames (mask == 0),
 * the complex STFT known_spec [B][2][F][T] holds on the known frames, only the gap frames' phase is iterated (momentum 0:
 * classic Griffin-Lim; 0.99: the fast variant).  STFT conventions of nppc_istft_any / nppc_stft_pair; 1 + L / hop == T.
 * One workgroup per (item, variation) keeps the span = bounding range of the item's gap frames + r = ceil(n_fft / hop) - 1
 * neighbours per side in LDS for all iterations.  An item whose span has more frames than the cap gets NaN in out, dist and
 * target_norm and status[b] = 1; the other items are unaffected.  No atomics, no host synchronisation; a waveform does not
 * depend on the batch.  Only gap frames of target_mag / init_phase and known frames of known_spec are read. */
#define NPPC_GL_MAX_SPAN_FRAMES 32
/* The argument rules, without a GPU.  max_span: 0 = NPPC_GL_MAX_SPAN_FRAMES, else a lower cap (less LDS, more workgroups
 * per CU).  *why (nullable) names the broken rule: 1 F != n_fft / 2 + 1, 2 1 + L / hop != T, 3 n_fft > 512 or
 * ceil(n_fft / hop) > 8, 4 n_iter < 0 or momentum < 0, 5 anything else.  *span_cap = the cap in force (the LDS budget of
 * 160 KB can lower it), *lds_bytes = dynamic LDS of the main kernel, *work_bytes = the workspace a call needs. */
int nppc_gl_gap_shape(int B, int V, int F, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span, int* why,
                      int* r, int* span_cap, long* lds_bytes, long* work_bytes);
/* phase_advance_init: phase [B][F][T] = angle(known[f][t0]) + 2 pi f hop (t - t0) / n_fft on gap frames, t0 = the known frame
 * left of the gap run (right of it for a run that starts at frame 0); 0 on known frames and where no frame is known */
int nppc_gl_phase_init(const float* known_spec, const float* mask, float* phase, int B, int T, int nfft, int hop, void* stream);
/* target_mag [B][V][F][T], mask [B][T] (1 = known), init_phase [B][V][F][T] (phase_per_variation) or [B][F][T] ->
 * out [B][V][L], dist [B][V][n_iter] (fp64: distance of stft(x_n) to the constraint set), target_norm [B][V] (fp64) */
int nppc_gl_gap(const float* target_mag, const float* known_spec, const float* mask, const float* init_phase,
                int phase_per_variation, float* out, double* dist, double* target_norm, int* status, void* work,
                long work_bytes, int B, int V, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span,
                void* stream);
/* the same with V = K A + 1 magnitudes formed on the fly: v < K A: exp((pred + alphas[v % A] pc[v / A]) stdev + mean), v = K A:
 * exp(pred stdev + mean); pred [B][F][T], pc [B][K][F][T], mean / stdev device scalars, alphas [A] (device), init_phase
 * [B][F][T] */
int nppc_gl_gap_pc(const float* pred, const float* pc, const float* mean, const float* stdev, const float* alphas,
                   const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                   double* target_norm, int* status, void* work, long work_bytes, int B, int K, int A, int T, int nfft, int hop,
                   int L, int n_iter, double momentum, int max_span, void* stream);

/* ---- Griffin-Lim for spans over the cap: the tiled path (csrc/gl_gap_long.hip) -------------------------
 * The same algorithm and the same bits per waveform as nppc_gl_gap, with a waveform's state (C, P, M, the span's time
 * segment) in the workspace and one launch per half-iteration over many workgroups: 2 n_iter + O(1) launches on the caller's
 * stream, no host read, no atomics, no kernel waits for another workgroup.  mode 1: items whose span is within the resident
 * cap (max_span, as above) run as nppc_gl_gap runs them, the others run tiled; mode 2: every item runs tiled.
 * long_max_span: 0 = T + 2 r (no gap of the clip is refused), else the span cap of the tiled path (> 2 r), which sizes the
 * workspace; an item over it gets NaN and status 1 as above.  dist and target_norm of a tiled item are folded over workgroups
 * in ascending order: they may differ from the resident kernel's in the last bits, the waveforms may not.
 * The argument rules without a GPU: as nppc_gl_gap_shape, plus *long_span_cap; *work_bytes covers both paths. */
int nppc_gl_gap_long_shape(int B, int V, int F, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span,
                           int long_max_span, int* why, int* r, int* span_cap, int* long_span_cap, long* lds_bytes,
                           long* work_bytes);
int nppc_gl_gap_long(const float* target_mag, const float* known_spec, const float* mask, const float* init_phase,
                     int phase_per_variation, float* out, double* dist, double* target_norm, int* status, void* work,
                     long work_bytes, int B, int V, int T, int nfft, int hop, int L, int n_iter, double momentum, int max_span,
                     int long_max_span, int mode, void* stream);
int nppc_gl_gap_pc_long(const float* pred, const float* pc, const float* mean, const float* stdev, const float* alphas,
                        const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                        double* target_norm, int* status, void* work, long work_bytes, int B, int K, int A, int T, int nfft,
                        int hop, int L, int n_iter, double momentum, int max_span, int long_max_span, int mode, void* stream);

/* ---- ragged-gap MC-dropout + PCA baseline (csrc/mc_pca_ragged.hip, the PCA in csrc/mc_pca.hip; specification
 * tests/mc_ragged_ref.py): the items of a batch may have different numbers of gap (mask == 0) elements ---------------------
 * mask [B][N] (any mask, N = F T <= 2^31 - 1) -> counts [B] = gap elements per item; then, with Nmax >= max counts,
 * idx [B][Nmax] = their positions in row-major order (the order of boolean indexing and masked_scatter_), -1 past counts[b].
 * One workgroup per item, block scan, no atomics. */
int nppc_gap_count(const float* mask, int* counts, int B, long N, void* stream);
int nppc_gap_index(const float* mask, int* idx, int B, long N, int Nmax, void* stream);
/* out [B][Nmax] = src [B][N] through idx, 0 where idx < 0 */
int nppc_gap_gather(const float* src, const int* idx, float* out, int B, long N, int Nmax, void* stream);
/* out [B][R][N] = 0, then vals [B][R][Nmax] written through idx (entries < 0 skipped) */
int nppc_gap_scatter(const float* vals, const int* idx, float* out, int B, int R, long N, int Nmax, void* stream);
/* nppc_pca_batch for X [K][B][Nmax] where item b owns its first counts[b] (1 <= counts[b] <= Nmax) elements: outputs as
 * nppc_pca_batch with rows of Nmax, zeros past counts[b].  The Gram is summed without atomics in a fixed order over chunks
 * of 64 elements that start at the item's element 0, so item b of a batch equals, bit for bit, the same call on that item
 * alone (B = 1, Nmax = counts[b]), and two runs agree bit for bit.  Same limits: 2 <= K <= 60, n <= min(K, 8).
 * work = *elems of nppc_pca_ragged_work_elems doubles. */
int nppc_pca_ragged_work_elems(int K, int B, int Nmax, int n, long* elems);
int nppc_pca_ragged(const float* X, const int* counts, int K, int B, int Nmax, int n, float* mean, float* comps, float* scaled,
                    float* svals, float* weights, double* work, void* stream);

/* ---- whole-recording restoration (csrc/restore_rec.hip; specification tests/restore_ref.py) --------
 * The top layer of the inpainting side: a recording wave [L] with gaps -> windows for the nets -> the window outputs spliced
 * back.  gaps [G][2] (long): half-open sample intervals [s, e), sorted ascending and disjoint.  Plain vector loads and stores,
 * no float atomics, sums in a fixed order: two runs give identical bits. */
#define NPPC_REC_GAIN_WORK 256      /* doubles of nppc_rec_gain's workspace */
#define NPPC_ZERO_RUN_CHUNK 4096    /* samples per workgroup of nppc_zero_runs' first phase */
/* gain[0] (fp64) = 10^((target_dbfs - 20 log10(rms + 1e-8)) / 20), rms over the samples outside every gap
 * (dataset/audio_dataset_inpainting.py:154-168 on the known samples).  G = 0 (gaps nullable): every sample. */
int nppc_rec_gain(const float* wave, long L, const long* gaps, int G, float target_dbfs, double* work, double* gain,
                  void* stream);
/* one workgroup per window w: out [W][win_len] = (float)(wave[win_start[w] + j] * gain[0]) (one fp64 product), 0 inside
 * every gap and outside [0, L); mask [W][win_len] = 0 there, 1 elsewhere */
int nppc_rec_windows(const float* wave, long L, const long* gaps, int G, const long* win_start, int W, int win_len,
                     const double* gain, float* out, float* mask, void* stream);
/* out [V][L]: out[v] = wave except around gap g, which window g (start win_start[g]) owns; with
 * y = wout[g * w_stride + v * v_stride + (n - win_start[g])] / gain[0] (fp64):
 *   n in [s, e): y;  n in [s - xf, s), t = n - (s - xf), and n in [e, e + xf), t = e + xf - 1 - n:
 *   wave[n] + c (y - wave[n]) with c = 0.5 - 0.5 cos(pi (t + 1) / (xf + 1)), in fp64, rounded to fp32 once;
 * clipped at the recording's ends and at the window's; every other sample is copied bit for bit.  The regions
 * [s - xf, e + xf) must not overlap (where they do, the lower gap wins). */
int nppc_rec_splice(const float* wave, long L, const long* gaps, const long* win_start, int G, const float* wout,
                    long w_stride, long v_stride, int win_len, int V, int xf, const double* gain, float* out, void* stream);
/* maximal runs of samples == 0 with at least min_len (>= 1) samples -> runs [cap][2] (start, end) ascending, count[0] = how
 * many there are (it may exceed cap: nothing is written past the buffer).  work: at least
 * nchunks (4 + 2 (NPPC_ZERO_RUN_CHUNK / (min_len + 1) + 1)) longs, nchunks = ceil(L / NPPC_ZERO_RUN_CHUNK). */
int nppc_zero_runs(const float* wave, long L, long min_len, long* work, long work_elems, long* runs, int cap, long* count,
                   void* stream);

/* ---- whole-recording enhancement (csrc/enhance_core.h + csrc/enhance_rec.hip; specification
 * tests/enhance_ref.py) ---------------------------------------------------------------------------------------------------
 * A recording of L samples enhanced in n chunks of C samples (C even) at a hop of H = C / 2: chunk c is an enhanced waveform
 * e_c = enh + c e_cs and K direction waveforms p_{c,k} = pcs + c p_cs + k p_ks (strides in elements, samples contiguous),
 * 0 < L - (n - 1) H <= C.  The rule (boundary Gram, chain, splice) is stated once in csrc/enhance_core.h.
 * Null pointers, n < 1, an odd C, negative strides: NPPC_EBADARG; K > NPPC_ENH_MAX_K: NPPC_EUNSUPPORTED; before any launch. */
#define NPPC_ENH_MAX_K 16          /* directions */
#define NPPC_ENH_MAX_SPLIT 64      /* workgroups that share one boundary's H samples */
#define NPPC_ENH_TILE 1024         /* output samples per workgroup of nppc_enh_splice */
#define NPPC_ENH_MATCH_GREEDY 0
#define NPPC_ENH_MATCH_SIGN 1
/* *S = the split nppc_enh_gram should run with (split = 0: chosen to fill the machine; split > 0: that value, clamped to
 * 1 .. min(NPPC_ENH_MAX_SPLIT, H)) and *work_bytes = 8 (n - 1) S K (K + 2), its workspace.  Either may be null.  No GPU. */
int nppc_enh_shape(int n, int K, int C, int split, int* S, long* work_bytes);
/* work [n - 1][S][K (K + 2)] (fp64): workgroup s of boundary c (1 <= c < n) sums samples [s seg, (s + 1) seg), seg =
 * ceil(H / S), of G[j][k] = sum p_{c-1,j}[H + i] p_{c,k}[i], na[j], nb[k] (G row-major, then na, then nb).  n >= 2. */
int nppc_enh_gram(const float* pcs, long p_cs, long p_ks, int n, int K, int C, int S, double* work, void* stream);
/* one workgroup: the S partials of every boundary summed in index order into gram [n - 1][K (K + 2)] (fp64), then the chain
 * -> perm [n][K], sign [n][K] (int), continuity [n - 1][K] (fp64).  n = 1 writes the identity (work, continuity and gram
 * may be null). */
int nppc_enh_chain(const double* work, int n, int K, int S, int match, int* perm, int* sign, double* continuity, double* gram,
                   void* stream);
/* out [1 + K A][ldo] (ldo >= L): row 0 the enhanced recording, row 1 + s A + a slot s at alphas[a]; w [H] the fp32 table
 * 0.5 - 0.5 cos(2 pi i / C); perm / sign [n][K] device tables (an entry of perm outside 0 .. K - 1 is clamped).  A = 0 or
 * K = 0: the enhanced row alone (pcs, alphas, perm, sign may be null); n = 1: w may be null.  16-byte loads when H, the
 * strides and the bases allow them, 16-byte stores when ldo % 4 == 0 and out is 16-byte aligned; the bits are the same. */
int nppc_enh_splice(const float* enh, long e_cs, const float* pcs, long p_cs, long p_ks, int n, int K, int C, long L,
                    const float* alphas, int A, const float* w, const int* perm, const int* sign, float* out, long ldo,
                    void* stream);
/* host only, serial, the same core: the Gram in ascending sample order and the chain (gram nullable) */
int nppc_enh_chain_host(const float* pcs, long p_cs, long p_ks, int n, int K, int C, int match, int* perm, int* sign,
                        double* continuity, double* gram);
/* host only, serial, the same core: nppc_enh_splice on host pointers */
int nppc_enh_splice_host(const float* enh, long e_cs, const float* pcs, long p_cs, long p_ks, int n, int K, int C, long L,
                         const float* alphas, int A, const float* w, const int* perm, const int* sign, float* out, long ldo);

/* ---- posterior samples from the NPPC directions (csrc/posterior.hip; specification
 * tests/posterior_ref.py) ------------------------------------------------------------------------------------------------
 * pred_crm [B][2][F][T] compressed cIRM, w_mat [B][K][2][F][T] directions, noisy re / im [B][F][T], z [B][S][K][2] a real and
 * an imaginary coefficient per sample and direction.  Sample s is the centred inverse STFT (periodic hann, nppc_istft's
 * rules) of mask_s * noisy, with, in fp32, k ascending, every multiply and add rounded on its own,
 *   NPPC_POST_COMPRESSED:    mask_s = decompress(pred + sum_k z_sk w_k)           (complex z w, each part decompressed)
 *   NPPC_POST_DECOMPRESSED:  mask_s = decompress(pred) + sum_k z_sk decompress(w_k)
 * lengths (nullable) [B]: item b uses its first 1 + L_b / hop frames and is 0 in samples L_b .. ld - 1, as
 * nppc_istft_ragged.  nfft in {64, 128, 256, 512}, nfft % hop == 0, nfft / hop <= 8, 0 <= K <= NPPC_POST_MAX_K,
 * S >= 1; anything else NPPC_EBADARG before any launch.  No atomics: the same bits from run to run, an item of a batch equals
 * the item alone and a sample does not depend on S. */
#define NPPC_POST_MAX_K 16             /* directions */
#define NPPC_POST_TILE 8               /* samples one workgroup runs when no statistics are asked for */
#define NPPC_POST_MAX_STAT_S 4096      /* most samples when statistics are asked for */
#define NPPC_POST_MAX_STAT_TILES 32    /* most sample tiles when statistics are asked for */
#define NPPC_POST_FILL 1024            /* workgroups that count as a full machine */
#define NPPC_POST_COMPRESSED 0
#define NPPC_POST_DECOMPRESSED 1
/* stats: bit 0 the time-domain mean / std, bit 1 the magnitude mean / std (then 2 <= S <= NPPC_POST_MAX_STAT_S).  With
 * nblk = max(ceil((ld + nfft / 2) / (4 hop)), ceil(T / 4)) workgroups per item and sample tile:
 *   n = ceil(S / NPPC_POST_TILE); stats: n = min(n, clamp(ceil(NPPC_POST_FILL / (B nblk)), 1, NPPC_POST_MAX_STAT_TILES));
 *   *tile_samples = ceil(S / n), *tiles = ceil(S / *tile_samples) (gridDim.z),
 *   *work_bytes = 16 *tiles B ((stats & 1 ? ld : 0) + (stats & 2 ? F T : 0)).  Each output may be null.  No GPU. */
int nppc_post_sample_shape(int B, int S, int K, int T, int nfft, int hop, long ld, int stats, int* tiles, int* tile_samples,
                           long* work_bytes);
/* Outputs, each nullable (mean with std, mag_mean with mag_std; at least one output): samples [B][S][ld]; mean, std [B][ld]
 * over s of the samples; mag_mean, mag_std [B][F][T] over s of |X_s| = sqrtf(xr^2 + xi^2) (0 in frames past an item's end).
 * The statistics are fp64 sums of y and y^2 per sample tile (work, 16-byte aligned, work_bytes as above), folded in tile order
 * by a finishing launch: mean = sum / S, std = sqrt(max(0, (sum y^2 - (sum y)^2 / S) / (S - 1))), rounded to fp32 once. */
int nppc_post_sample(const float* pred_crm, const float* w_mat, const float* re, const float* im, const float* z,
                     const int* lengths, int domain, int B, int S, int K, int T, int nfft, int hop, long ld, float* samples,
                     float* mean, float* std, float* mag_mean, float* mag_std, double* work, long work_bytes, void* stream);

/* ---- posterior samples of a whole recording (csrc/enhance_post.hip; the rule: item 4 of
 * csrc/enhance_core.h; specification tests/enhance_posterior_ref.py) -----------------------------------------------------
 * The planes of the n chunks of a recording of L samples (chunks of C at a hop of H = C / 2, the last one L - (n - 1) H
 * long): pred_crm [n][2][F][T], w_mat [n][K][2][F][T], noisy re / im [n][F][T]; z [S][K][2], one set of coefficients per
 * sample for the whole recording, indexed by slot; perm, sign [n][K] the device tables of nppc_enh_chain; w [H] the
 * cross-fade table of nppc_enh_splice.  Sample s of chunk c is nppc_post_sample's sample with direction k =
 * (sign[c][k] < 0 ? -1 : 1) w_mat[c][perm[c][k]] (an entry of perm outside 0 .. K - 1 is clamped) at the chunk's length; the
 * recording is their cross-fade by nppc_enh_splice's rule.  One launch: a workgroup owns 4 hop output samples of the
 * recording and a tile of consecutive s.  Beyond nppc_post_sample's limits: nfft / hop >= 2, H % (4 hop) == 0, stats 0 or 1
 * (then 2 <= S <= NPPC_POST_MAX_STAT_S) and nppc_enh_splice's plan (0 < L - (n - 1) H <= C, K <= NPPC_ENH_MAX_K); anything
 * else NPPC_EBADARG from the shape function, before any launch.  No atomics: the same bits from run to run, and a sample
 * does not depend on S.
 *   nblk = ceil(L / (4 hop)); n_t = ceil(S / NPPC_POST_TILE); stats: n_t = min(n_t, clamp(ceil(NPPC_POST_FILL / nblk), 1,
 *   NPPC_POST_MAX_STAT_TILES)); *tile_samples = ceil(S / n_t), *tiles = ceil(S / *tile_samples) (gridDim.y),
 *   *work_bytes = stats ? 16 *tiles L : 0.  Each output may be null.  No GPU. */
int nppc_enh_post_sample_shape(int n, int S, int K, int C, long L, int T, int nfft, int hop, int stats, int* tiles,
                               int* tile_samples, long* work_bytes);
/* Outputs, each nullable (mean with std; at least one): samples [S][ldo] (ldo >= L; the first L samples of every row are
 * written, nothing else); mean, std [L] over s, by nppc_post_sample's fp64 sums per sample tile in work (16-byte aligned)
 * and its finishing launch.  perm, sign, w_mat and z may be null when K == 0, w when n == 1. */
int nppc_enh_post_sample(const float* pred_crm, const float* w_mat, const float* re, const float* im, const float* z,
                         const int* perm, const int* sign, const float* w, int domain, int n, int S, int K, int C, long L,
                         int T, int nfft, int hop, float* samples, long ldo, float* mean, float* std, double* work,
                         long work_bytes, void* stream);

/* ---- posterior samples of inpainted gaps (csrc/inpaint_posterior.hip; specification
 * tests/inpaint_posterior_ref.py) ----------------------------------------------------------------------------------------
 * pred [B][F][T] and pc [B][K][F][T] normalised log-magnitudes (the directions orthogonal, un-normalised, zero on known
 * frames), mean / stdev device scalars, z [B][S][K] real coefficients.  Sample s of item b, bin o, in fp64, k ascending:
 *   x = pred[b][o]; for k: x = fma(z[b][s][k], pc[b][k][o], x); mag = exp(fma(x, stdev, mean))
 * (at z = alpha e_k the expression, and the bits, of nppc_pc_variation_waves / nppc_gl_gap_pc).
 * nppc_inp_post_sample gives mag the phase of clean_spec [B][2][F][T] (angle(0) = 0) and inverts with nppc_istft_any's
 * transform, S samples per item in one launch: a workgroup owns 256 output samples of one item and a tile of consecutive s.
 * K <= NPPC_INP_POST_MAX_K, S >= 1, nfft <= 512 and nppc_istft_any's limits; anything else NPPC_EBADARG before any launch.
 * No atomics: the same bits from run to run, an item alone equals the item in a batch, a sample does not depend on S. */
#define NPPC_INP_POST_MAX_K 16
#define NPPC_INP_POST_TILE 8               /* samples one workgroup runs when no statistics are asked for */
#define NPPC_INP_POST_MAX_STAT_S 4096
#define NPPC_INP_POST_MAX_STAT_TILES 32
#define NPPC_INP_POST_FILL 1024            /* workgroups that count as a full machine */
#define NPPC_INP_POST_LDS_STAGE 65536      /* most LDS bytes of a workgroup that stages its planes (2 workgroups per CU) */
#define NPPC_INP_POST_NO_STAGE 1           /* flags: re-read the planes from global memory whatever the shape */
/* stats: bit 0 the time-domain mean / std, bit 1 the magnitude mean / std (then 2 <= S <= NPPC_INP_POST_MAX_STAT_S).
 *   n = ceil(S / NPPC_INP_POST_TILE); stats: n = min(n, clamp(ceil(NPPC_INP_POST_FILL / (B ceil(L / 256))), 1,
 *   NPPC_INP_POST_MAX_STAT_TILES)); *tile_samples = ceil(S / n), *tiles = ceil(S / *tile_samples) (gridDim.z),
 *   *work_bytes = 16 *tiles B ((stats & 1 ? L : 0) + (stats & 2 ? F T : 0)).
 * With nfr = (254 + nfft) / hop + 1 frames per workgroup, *staged = 1 when 16 nfft + (24 + 4 (K + 1)) nfr F (twiddles, unit
 * phasors, frame buffer, K + 1 planes) <= NPPC_INP_POST_LDS_STAGE and flags does not forbid it; *lds_bytes is what the chosen
 * path takes.  Each output may be null.  No GPU. */
int nppc_inp_post_sample_shape(int B, int S, int K, int T, int nfft, int hop, int L, int stats, int flags, int* tiles,
                               int* tile_samples, long* work_bytes, int* staged, long* lds_bytes);
/* Outputs, each nullable (mean with std, mag_mean with mag_std; at least one output): samples [B][S][L]; mean, std [B][L]
 * over s of the samples; mag_mean, mag_std [B][F][T] over s of mag (fp64, every frame).  Statistics as nppc_post_sample's:
 * fp64 sums of y and y^2 per sample tile in work (16-byte aligned), folded in tile order by a finishing launch. */
int nppc_inp_post_sample(const float* pred, const float* pc, const float* clean_spec, const float* mean_p, const float* stdev,
                         const float* z, int B, int S, int K, int T, int nfft, int hop, int L, int flags, float* samples,
                         float* mean, float* std, float* mag_mean, float* mag_std, double* work, long work_bytes, void* stream);
/* nppc_gl_gap_pc / nppc_gl_gap_pc_long with the magnitudes of S posterior samples: V = S + 1, v < S by the rule above from
 * z [B][S][K], v = S the prediction (z = 0), formed bin by bin where the iteration starts (no [B][S][F][T] stack). */
int nppc_gl_gap_post(const float* pred, const float* pc, const float* mean, const float* stdev, const float* z,
                     const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                     double* target_norm, int* status, void* work, long work_bytes, int B, int K, int S, int T, int nfft, int hop,
                     int L, int n_iter, double momentum, int max_span, void* stream);
int nppc_gl_gap_post_long(const float* pred, const float* pc, const float* mean, const float* stdev, const float* z,
                          const float* known_spec, const float* mask, const float* init_phase, float* out, double* dist,
                          double* target_norm, int* status, void* work, long work_bytes, int B, int K, int S, int T, int nfft,
                          int hop, int L, int n_iter, double momentum, int max_span, int long_max_span, int mode, void* stream);

/* ---- FLAC decoding (csrc/flac_core.h + csrc/flac.hip; specification tests/flac_ref.py) --------------
 * Every entry point returns NPPC_OK / an NPPC_E* code for its ARGUMENTS; what is wrong with a FILE is a per-file status: */
#define NPPC_FLAC_OK 0
#define NPPC_FLAC_BAD_MARKER 1        /* the file does not begin with fLaC */
#define NPPC_FLAC_TRUNCATED 2         /* the file ends inside its metadata or inside a frame */
#define NPPC_FLAC_BAD_STREAMINFO 3    /* no STREAMINFO block first, or one that cannot be */
#define NPPC_FLAC_UNSUPPORTED 4       /* 32-bit (or odd-sized) samples, total_samples == 0, an ID3v2 prefix, an Ogg container */
#define NPPC_FLAC_BAD_HEADER 5        /* no valid frame header where a frame has to begin */
#define NPPC_FLAC_RESERVED 6          /* a reserved subframe or residual type, or parameters the format rules out */
#define NPPC_FLAC_CRC16 7             /* a frame's CRC-16 does not match */
#define NPPC_FLAC_COUNT_MISMATCH 8    /* a frame's sample position is not the running count, or runs past total_samples */
#define NPPC_FLAC_MD5 9               /* the decoded samples do not match STREAMINFO's MD5 (nppc_flac_md5's verdict 2) */
#define NPPC_FLAC_INFO 8              /* longs of nppc_flac_probe's info */
#define NPPC_FLAC_META 12             /* longs per file of the device entry points' meta */
/* host only.  info[0..6] = sample rate, channels, bits per sample, total samples, min blocksize, max blocksize, byte offset
 * of the first frame (info[7] = 0); *status as above (info is valid when it is 0).  nbytes >= 2^31: NPPC_EUNSUPPORTED. */
int nppc_flac_probe(const unsigned char* bytes, long nbytes, long* info, int* status);
/* host only, the serial decoder: probes, then decodes frame after frame into pcm [C][n] (int32, n = total samples;
 * pcm_elems >= C n) and, when mono is not null, mono [n] (float; mono_elems >= n) = (sum_c (float)pcm[c] / 2^(bps-1)) / C,
 * summed left to right in fp32.  A status other than 0 leaves the outputs partly written. */
int nppc_flac_decode_host(const unsigned char* bytes, long nbytes, int* pcm, long pcm_elems, float* mono, long mono_elems,
                          int* status);
/* device, a batch of nfiles files laid back to back in bytes [total_bytes].  meta [nfiles][NPPC_FLAC_META] (long, device):
 *   0 byte_begin  1 byte_end  2 sample rate  3 channels  4 bits per sample  5 min blocksize  6 max blocksize  7 total samples
 *   8 first-frame byte offset within the file  9 pcm offset (int32 elements)  10 mono offset (floats)  11 unused
 * with byte_begin ascending, byte_end[f] == byte_begin[f + 1], values 2..8 from nppc_flac_probe.  work: *elems longs of
 * nppc_flac_work_elems(cap), cap = how many frame-header candidates fit.  The four calls run in this order on one stream
 * with no host read between them (a clear and four kernels, whatever nfiles is):
 *   scan    clears work; tests EVERY byte position for a frame header of its file (flac_parse_header) and appends the
 *           candidates (an integer counter; nothing depends on the order) and enters them in a hash table by offset
 *   parse   one lane per candidate: the frame parsed to its end with stores off -> end offset, status (CRC-16 included)
 *   chain   one lane per file: from the first-frame offset along the end offsets exactly as the serial decoder walks;
 *           marks the accepted candidates; status [nfiles + 1] (int): per file, then 1 when more than cap candidates were
 *           found (every status is then void: call again with cap >= total_bytes / 4 + 1, which always suffices)
 *   decode  one lane per accepted candidate: pcm [pcm_elems] int32 and, when not null, mono [mono_elems] float, at the
 *           offsets of meta; a file whose range does not fit pcm_elems / mono_elems is skipped
 * No kernel waits for another workgroup and there are no float atomics: two runs give identical bits, and a file's output
 * does not depend on its neighbours. */
int nppc_flac_work_elems(long cap, long* elems);
int nppc_flac_scan(const unsigned char* bytes, long total_bytes, const long* meta, int nfiles, long* work, long cap, void* stream);
int nppc_flac_parse(const unsigned char* bytes, const long* meta, int nfiles, long* work, long cap, void* stream);
int nppc_flac_chain(const unsigned char* bytes, const long* meta, int nfiles, long* work, long cap, int* status, void* stream);
int nppc_flac_decode(const unsigned char* bytes, const long* meta, int nfiles, long* work, long cap, int* pcm, long pcm_elems,
                     float* mono, long mono_elems, void* stream);
/* ---- MD5 of the decoded samples (csrc/md5_core.h + csrc/flac_md5.hip) -------------------------------
 * STREAMINFO holds the MD5 (RFC 1321) of the unencoded samples, written by the encoder: the one check that does not depend
 * on how the bitstream is read.  The entry points above ignore the field; these read it and compute what it should be.
 * The message, as libFLAC forms it: the samples interleaved by channel, sample-major, each a signed little-endian integer
 * of (bps + 7) / 8 bytes (the low bytes of the sign-extended int32: 12 bits fill 2 bytes, 20 bits 3), n C bytes_per_sample
 * bytes in all.  It is never materialised; lengths are 64-bit, so 2^31 message bytes and more hash like any other.
 *
 * host only.  md5 [16] = bytes 18..34 of STREAMINFO, *present = whether any of them is non-zero (sixteen zero bytes are the
 * format's "not computed"); *status as nppc_flac_probe gives it (md5 is zeroed and *present 0 when it is not 0). */
int nppc_flac_stream_md5(const unsigned char* bytes, long nbytes, unsigned char* md5, int* present, int* status);
/* host only, the serial hash: digest [16] of pcm [channels][n] (int32).  n >= 0 (n = 0: the MD5 of the empty message, pcm
 * may be null); channels outside 1..8, bps outside 4..32 or n < 0: NPPC_EBADARG. */
int nppc_flac_md5_host(const int* pcm, long n, int channels, int bps, unsigned char* digest);
/* device, one launch, one lane per file.  pcm [pcm_elems] and meta [nfiles][NPPC_FLAC_META] are the decode calls' (of meta
 * only channels 3, bits per sample 4, total samples 7 and the pcm offset 9 are read; total samples may be 0 here).  order
 * [nfiles] (int, device): a permutation of the files, lane i hashes file order[i]; built on the host by descending message
 * length so that the lanes of a wave run similar block counts.  No result depends on it.  expected [nfiles][16] or null:
 * the digests nppc_flac_stream_md5 gave.  status [nfiles] or null: nppc_flac_chain's, read on the same stream.
 *   digest  [nfiles][16]  the MD5 of each file's samples
 *   verdict [nfiles] int  0 = nothing to compare (expected null or all zero) or the file was skipped, 1 = match, 2 = mismatch
 * A file with a non-zero status, channels outside 1..8, bits outside 4..32 or a pcm range outside pcm_elems is skipped:
 * digest zeroed, verdict 0.  16-bit (9..16) mono and stereo take a path of two samples per message word with 16-byte loads
 * where the address allows; every other format is formed byte by byte.  Two runs give identical bytes. */
int nppc_flac_md5(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* order, const unsigned char* expected,
                  const int* status, unsigned char* digest, int* verdict, void* stream);

/* ---- FLAC encoding (csrc/flac_enc_core.h + csrc/flac_enc.hip; specification tests/flac_enc_ref.py) ----
 * Lossless, fixed predictors (LPC as well through the _lpc entry points below), one stated decision rule
 * (csrc/flac_enc_core.h): the bytes are a function of the samples,
 * bits per sample (8, 12, 16, 20 or 24), rate (1 .. 2^20 - 1) and block size (16 .. 4608) alone.  The stream is fLaC, one
 * STREAMINFO (min = max blocksize = block_size, min / max frame size, total samples, MD5 of the samples) and frames of
 * block_size samples, the last one shorter.  An unsupported bps or block size: NPPC_EUNSUPPORTED. */
#define NPPC_FLAC_ENC_PLAN 8          /* ints per frame of the plan: bytes, assignment, (type, order, partition order) x 2 */
/* host only.  *bytes = the most bytes the stream of n samples per channel can take (every subframe verbatim, plus headers);
 * *frames = ceil(n / block_size).  Either may be null.  n < 1 or channels outside 1..8: NPPC_EBADARG. */
int nppc_flac_enc_bound(long n, int channels, int bps, int block_size, long* bytes, long* frames);
/* host only, the serial encoder: pcm [channels][n] int32 -> out [cap], cap >= the bound; *nbytes = the stream's length.
 * 1..8 channels (stereo tries the four assignments, channels 3..8 are independent).  A sample outside bps bits, n < 1, a
 * rate outside 1 .. 2^20 - 1 or cap below the bound: NPPC_EBADARG. */
int nppc_flac_encode_host(const int* pcm, long n, int channels, int bps, int rate, int block_size, unsigned char* out, long cap,
                          long* nbytes);
/* x [V][ldx] fp32, lengths [V] (long, device; null = ldx each; clamped to [0, ldx]) -> pcm[pcm_off[v] + i] =
 * clip(rint(x 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1), halves to even, NaN -> 0.  pcm_off [V] (long, device); an item
 * whose range leaves pcm_elems is skipped. */
int nppc_pcm_quantize(const float* x, long ldx, const long* lengths, int V, int bits, int* pcm, const long* pcm_off, long pcm_elems,
                      void* stream);
/* device, a ragged batch of nfiles files of one bps, rate and block size.  pcm [pcm_elems] int32, planar per file; meta
 * [nfiles][NPPC_FLAC_META] (long, device) as for decoding, of which 3 channels (1 or 2), 4 bits per sample, 7 samples and 9 the
 * pcm offset are read; ftab [nframes][2] (int, device) = (file, frame number) of every frame, files ascending and each
 * file's frames ascending.  The calls run in this order on one stream with nppc_flac_md5 (digest [nfiles][16]) anywhere
 * before write, and no host read between them:
 *   plan    plan [nframes][NPPC_FLAC_ENC_PLAN] int: one workgroup per frame
 *   scan    goff [nframes] long: where every frame begins in out, the files back to back, each behind its 42-byte stream
 *           header; stats [nfiles + 1][4] long: per file begin, end, min and max frame size; stats[nfiles][0] = all bytes
 *   write   out [out_cap] bytes, out_cap >= the sum of the files' bounds; a frame that would leave it is not written
 * Integer atomics only, no waiting between workgroups: two runs give identical bytes and a file's bytes do not depend on
 * the rest of the batch. */
int nppc_flac_enc_plan(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                       int block_size, int* plan, void* stream);
int nppc_flac_enc_scan(const int* plan, const int* ftab, long nframes, int nfiles, long* goff, long* stats, void* stream);
int nppc_flac_enc_write(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                        int rate, int block_size, const int* plan, const long* goff, const long* stats,
                        const unsigned char* digest, unsigned char* out, long out_cap, void* stream);
/* predictor "lpc" (the rule is stated in csrc/flac_enc_core.h, specification tests/flac_lpc_ref.py):
 * every non-constant subframe also costs LPC orders 1 .. min(max_order, block) (integer Welch window, exact int64
 * autocorrelation, Levinson-Durbin in fp64 without contraction, 12-bit coefficients up to 16 bits per sample and 15-bit
 * above) exactly, beside the fixed orders; ties go to the fixed orders, so no frame is longer than the fixed one.
 * max_order outside 1..12: NPPC_EBADARG; every other refusal as for the entry points above.  The plan record is wider:
 * bytes, assignment, then per coded channel type (3 = LPC), order, partition order, shift and 12 coefficients.  The calls
 * run as above: plan_lpc, scan_stride with stride NPPC_FLAC_ENC_PLAN_LPC (nppc_flac_enc_scan is the stride
 * NPPC_FLAC_ENC_PLAN; a stride outside 1..1024: NPPC_EBADARG), nppc_flac_md5, write_lpc, which range-checks every field of
 * the record and does not recompute it.  Host and device give the same bytes. */
#define NPPC_FLAC_ENC_PLAN_LPC 34     /* ints per frame of the LPC plan: 2 + 2 x (4 + 12) */
#define NPPC_FLAC_ENC_MAX_LPC 12
int nppc_flac_encode_host_lpc(const int* pcm, long n, int channels, int bps, int rate, int block_size, int max_order,
                              unsigned char* out, long cap, long* nbytes);
int nppc_flac_enc_plan_lpc(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                           int block_size, int max_order, int* plan, void* stream);
int nppc_flac_enc_scan_stride(const int* plan, int stride, const int* ftab, long nframes, int nfiles, long* goff, long* stats,
                              void* stream);
int nppc_flac_enc_write_lpc(const int* pcm, long pcm_elems, const long* meta, int nfiles, const int* ftab, long nframes, int bps,
                            int rate, int block_size, const int* plan, const long* goff, const long* stats,
                            const unsigned char* digest, unsigned char* out, long out_cap, void* stream);

/* ---- windowed-sinc resampling of ragged batches (csrc/resample.hip; specification
 * tests/resample_ref.py): torchaudio's default Resample (Hann window).  With orig / new the two rates reduced by their gcd,
 * Klen = 2 width + orig and xpad the item padded with `width` zeros on the left and zeros on the right,
 *   y[i new + p] = sum_k xpad[i orig + k] kern[p][k],  cut to ceil(new len / orig) outputs.
 * table [new][stride] 32-bit words (device): per phase p (int k0, int count, float taps[maxcount]) = kern[p][k0 .. k0 +
 * count), every other tap of kern[p] being exactly 0.0f; stride = (2 + maxcount) | 1.  Each output is one fp32 fma chain
 * over its `count` taps in ascending k, started from 0: no atomics, no workspace, identical bits run to run, and an item's
 * bits do not depend on the tile or on the rest of the batch. */
#define NPPC_RESAMPLE_LDS_BUDGET 65536     /* bytes of LDS a workgroup may take: table + the tile's input span */
#define NPPC_RESAMPLE_TABLE_BUDGET 40960   /* bytes the table may take of that */
/* host only.  *stride as above; *table_bytes = new stride 4; *span_elems = ((tile - 1) / new + 1) orig + Klen, the most
 * input samples a tile of `tile` outputs touches; *lds_bytes = table + span; *fits = both budgets hold.  Out pointers
 * may be null.  Non-positive arguments or maxcount > Klen: NPPC_EBADARG. */
int nppc_resample_sinc_shape(int orig, int new_, int width, int maxcount, int tile, int* stride, long* table_bytes,
                             long* span_elems, long* lds_bytes, int* fits);
/* x [B][ldx] fp32, lengths [B] (long, device; null = every item has ldx samples; clamped to [0, ldx]) -> y [B][ldy]:
 * columns below ceil(new len / orig) as above, zeros from there to ldy (every column is written).  Samples at or past an
 * item's length are never read.  grid (ceil(ldy / tile), B).  A (ratio, tile) that does not fit: NPPC_EUNSUPPORTED. */
int nppc_resample_sinc(const float* x, long ldx, const long* lengths, int B, const int* table, int orig, int new_, int width,
                       int maxcount, int tile, float* y, long ldy, void* stream);

/* ---- spectrogram sheets as PNG (csrc/png_core.h + csrc/spec_png.hip; specification tests/png_ref.py)
 * The file: signature, IHDR (8 bits, indexed), PLTE (256 entries), one IDAT, IEND.  Every scanline has filter type 2 (Up);
 * zlib 78 01 and one fixed-Huffman deflate block whose only matches are distance-1 runs (the token rule: csrc/png_core.h), so
 * the bytes are a function of the pixels alone, the same from the serial host encoder and from the device.
 * W, H in 1..16384 and W H <= 2^26, else NPPC_EBADARG (as are null pointers and empty batches), before any launch. */
#define NPPC_SPEC_CELL 8   /* ints per cell: plane of P (-1: none), plane of Q (-1: none), g (0 identity, 1 abs, 2 dB), flags (1
                              autoscale, 2 gap markers), alpha, vmin, scale = fp32(254 / (vmax - vmin)) (three floats' bits), the
                              cell's image.  P = Q = -1: a blank cell */
#define NPPC_SPEC_IMG 8    /* ints per image: item b, rows R, columns C, first cell (row-major R x C), sx, sy, gutter, 0 */
/* host only.  *bytes = 8 + 25 + 780 + 12 + (2 + ceil((3 + 9 H (W + 1) + 7) / 8) + 4) + 12: no file is longer */
int nppc_png_bound(long W, long H, long* bytes);
/* host only, serial.  idx [H][W], palette [256][3] -> out[0 .. *nbytes); cap below the bound: NPPC_EBADARG. */
int nppc_png_encode_host(const unsigned char* idx, long W, long H, const unsigned char* palette, unsigned char* out, long cap,
                         long* nbytes);
/* A ragged batch of device index images -> files back to back in out (device, 4-byte aligned, out_cap a multiple
 * of 4, cleared here).
 *   pix [pix_elems] uint8; meta [nimg][4] long (device): the image's first pixel, W, H, unused;
 *   ttab [ntiles][2] int (device): (image, tile number) of every 4096-byte tile of every filtered stream, image-major;
 *   tfirst [nimg + 1] int (device): the first tile of every image; palette [256][3] (HOST);
 *   work: plan [ntiles][4] int, toff [ntiles] long;
 *   stats [nimg + 1][4] long: file begin, file end, Adler-32, token bits; stats[nimg][0] = the batch's bytes.
 * A tile past its image's end, or an image whose meta cannot be (W = H = 0 included), is left out: its file has no bytes.
 * A memset and four launches: plan, scan, write, finish. */
int nppc_png_encode(const unsigned char* pix, long pix_elems, const long* meta, int nimg, const int* ttab, const int* tfirst,
                    long ntiles, const unsigned char* palette, int* plan, long* toff, long* stats, unsigned char* out, long out_cap,
                    void* stream);
/* mask [B][T_frames] fp32, 0 inside the gap -> win [B][4] int: t0, t1, marker 0, marker 1.  The gap [s, e) (first to last
 * zero frame) widened by its own length on each side and clamped to the clip; markers at s and e.  No gap: 0, T, -1, -1. */
int nppc_spec_windows(const float* mask, int B, int T_frames, int* win, void* stream);
/* planes [B][NP][CH][F][T_frames] fp32 (CH 1 real, 2 complex) -> the index images of nimg sheets.  A sheet is a grid of R x C
 * cells of item b's frames [t0, t1); a cell shows g(P + alpha Q): idx = clamp(floor((v - vmin) scale), 0, 253), NaN 0; 254 the
 * gap markers (the first pixel column of a marker frame, cell rows with (y / 4) % 2 == 0), 255 blank cells and gutters; bin 0
 * is the bottom row; every source pixel is sx x sy pixels.  Real planes: multiply, add, subtract, multiply, floor, each rounded
 * to fp32 on its own.  An autoscaled cell takes vmin and vmax from its finite values (equal: all zeros).
 *   img [nimg][NPPC_SPEC_IMG], cell [ncells][NPPC_SPEC_CELL], win [B][4] (device);
 *   rng [ncells][2] fp32 (work); meta [nimg][4] long: first pixel (given), W, H (written), pixels allowed (given; an image
 *   that needs more gets W = H = 0); pix [pix_elems] uint8; max_pixels: the largest allowance.
 * Three launches: layout, autoscale, render. */
int nppc_spec_render(const float* planes, int B, int NP, int CH, int F, int T_frames, const int* img, int nimg, const int* cell,
                     int ncells, const int* win, float* rng, long* meta, unsigned char* pix, long pix_elems, long max_pixels,
                     void* stream);
/* nppc_spec_render, then nppc_png_encode of what it drew (ttab and tfirst laid out for the pixels allowed) */
int nppc_spec_render_png(const float* planes, int B, int NP, int CH, int F, int T_frames, const int* img, int nimg, const int* cell,
                         int ncells, const int* win, float* rng, long* meta, unsigned char* pix, long pix_elems, long max_pixels,
                         const int* ttab, const int* tfirst, long ntiles, const unsigned char* palette, int* plan, long* toff,
                         long* stats, unsigned char* out, long out_cap, void* stream);

/* ---- curve sheets as index images and PNG files (csrc/curve_core.h) ------------------------------------
 * plot_pitch_comparison of the reference's validator_nppc_model.py:19-154: curves over frames (values [N][T_frames] fp32, NaN: no
 * point) in stacked panels with an axes box, grid lines, tick labels in a 5 x 7 font and a legend.  The drawing rule (fp32
 * quantisation of rows, integer segments, widths, crop to the window, paint order, layout) is stated once in csrc/curve_core.h.
 * Palette indices: the curves' own, 250 box and glyphs, 251 grid, 254 gap markers, 255 background.
 *   sheet [nimg][8]: item, first panel, panels, sx, plot height, glyph scale, 0, 0
 *   panel [npanels][8]: first curve, curves, flags (1 autoscale, 2 markers), ymin, scale = fp32(PH / (ymax - ymin)) (floats' bits),
 *                       first stamp, stamps, xtick_every (0: none)
 *   curve [ncurves][4]: row of values, colour, width 1..5, 0
 *   stamp [nstamps][8]: kind (0 y tick, 1 x label, 2 legend entry), value (float's bits / frame / entry), swatch colour, characters
 *                       (at most 16), glyph codes 4 bits each in two ints (0-9, 10 '.', 11 '-', 12 ' '), 0, 0
 *   win [nitems][4]: t0, t1, marker 0, marker 1 in curve frames (-1: no marker), the layout of nppc_spec_windows.
 * A panel's curves times (t1 - t0 + 2) may not exceed 16384 (the 16-bit rows a workgroup stages in LDS). */
/* host only: the tables are host memory.  W, H of sheet i for a window of `frames` frames; margins (nullable) [4]: left margin,
 * right margin, plot width, the most curves of a panel.  A sheet that cannot be drawn: NPPC_EBADARG. */
int nppc_curve_shape(const int* sheet, int nimg, const int* panel, int npanels, const int* curve, int ncurves, const int* stamp,
                     int nstamps, int N, int T_frames, int i, int frames, long* W, long* H, int* margins);
/* host only, serial: everything is host memory.  rng [npanels][2] fp32 (written: ymin, scale); meta [nimg][4] long: first pixel
 * (given), W, H (written), pixels allowed (given; a sheet that needs more, or cannot be drawn, gets W = H = 0). */
int nppc_curve_render_host(const float* values, int N, int T_frames, const int* sheet, int nimg, const int* panel, int npanels,
                           const int* curve, int ncurves, const int* stamp, int nstamps, const int* win, int nitems, float* rng,
                           long* meta, unsigned char* pix, long pix_elems);
/* the same on the device: everything is device memory; pix 4-byte aligned and every image's first pixel a multiple of 4;
 * max_panels: the most panels of a sheet (at most 64).  Three launches: layout, autoscale, render. */
int nppc_curve_render(const float* values, int N, int T_frames, const int* sheet, int nimg, const int* panel, int npanels,
                      const int* curve, int ncurves, const int* stamp, int nstamps, const int* win, int nitems, int max_panels,
                      float* rng, long* meta, unsigned char* pix, long pix_elems, void* stream);
/* nppc_curve_render, then nppc_png_encode of what it drew (ttab and tfirst laid out for the pixels allowed) */
int nppc_curve_render_png(const float* values, int N, int T_frames, const int* sheet, int nimg, const int* panel, int npanels,
                          const int* curve, int ncurves, const int* stamp, int nstamps, const int* win, int nitems, int max_panels,
                          float* rng, long* meta, unsigned char* pix, long pix_elems, const int* ttab, const int* tfirst, long ntiles,
                          const unsigned char* palette, int* plan, long* toff, long* stats, unsigned char* out, long out_cap,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
