/*
 * vd_hip.h - C ABI of libvd_hip.so, the MI355X (gfx950 / CDNA4) kernel library behind the
 * Versatile-Diffusion sampling hot path.
 *
 * The reference (SHI-Labs/Versatile-Diffusion) has no native layer: every FLOP of the path is a
 * stock torch op issued from Python.  This header is therefore the boundary the *new* Python
 * modules (versatile-diffusion_amd/lib/model_zoo/...) bind with ctypes; each entry point names
 * the reference code whose arithmetic it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - all pointers are device pointers owned by the caller (torch caching allocator); nothing is
 *     allocated, freed or synchronised inside the library; every launch goes to `stream`
 *   - activations are fp16, channels-last: [B, H, W, C] == (B*H*W, C) row-major
 *   - weights are fp16, K-contiguous: Linear [out][in] as torch stores it, conv repacked once at
 *     load time to [Cout][kh][kw][Cin]
 *   - statistics (GroupNorm, LayerNorm, softmax) and MFMA accumulation are fp32
 *   - return value: 0 on success, negative VD_ERR_* otherwise; vd_last_error() returns the
 *     thread-local message of the last failure
 *   - threads: entry points may be called concurrently from several host threads (one stream per
 *     thread).  Process-wide state is limited to the optional tuned launch table (vd_gemm_tune_*,
 *     mutex-protected), the developer tile override (atomic), per-device kernel attributes
 *     (atomic bit mask, idempotent) and development switches read once from the environment
 *     (VD_GEMM_TILE / VD_CONV_HALO / VD_ATTN_PIPE: function-local statics, initialised under the
 *     C++11 guarantee).  Scratch (workspaces, split-K counters) is caller-owned, one set per stream.
 *
 * ABI 8 (round 6) REMOVED entry points and options that had lost every measurement (vd_conv3x3_wreg_*,
 * vd_gemm_groupnorm_ok, VD_EPI_GROUPNORM / VD_EPI_GN_SILU: rejected, VdGemmDesc.gn_*: reserved); nothing
 * was added, and no struct layout changed.
 */
#ifndef VD_HIP_H
#define VD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t; /* same declaration as <hip/hip_runtime_api.h>: plain C hosts need no HIP headers */

#define VD_HIP_ABI_VERSION 8
#define VD_MAX_SPLIT_K 32

/* ---- epilogue description for vd_gemm_f16 ------------------------------------------------ */
#define VD_EPI_BIAS 1         /* + bias[n]                                                    */
#define VD_EPI_ROWVEC 2       /* + rowvec[m / rows_per_batch][n]  (ResBlock "h + emb_out")    */
#define VD_EPI_RESIDUAL 4     /* + res[m][n] after activation and alpha                       */
#define VD_EPI_BIAS_ALONG_M 8 /* bias indexed by output row (V^T = Wv x^T in the VAE AttnBlock) */
#define VD_EPI_OUT_F32 16     /* store fp32 instead of fp16                                   */
#define VD_EPI_LNFOLD 32      /* A rows are LayerNorm'ed on the fly, see VdGemmDesc.colsum     */
#define VD_EPI_LN_INLOOP 64   /* with VD_EPI_LNFOLD and ln_stats == NULL: row statistics inside the K loop (explicit opt-in) */
#define VD_EPI_GROUPNORM 128  /* reserved (ABI 5-7: GroupNorm inside the split-K reduce; removed in ABI 8, rejected)              */
#define VD_EPI_GN_SILU 256    /* reserved, as above                                                                        */
#define VD_EPI_LN_SUMS 512    /* with VD_EPI_LNFOLD (ABI 6): ln_stats points at the int64 [M][2] fixed-point (sum, sum of squares)
                               * of every A row that a producer launch accumulated through VdGemmDesc.row_sums, instead of fp32
                               * (mean, rstd); the epilogue derives mean / rstd over K with ln_eps */

#define VD_ACT_NONE 0
#define VD_ACT_GEGLU 1      /* out[:, j] = val_j * gelu_erf(gate_j); W/bias packed per 64 rows as [32 val | 32 gate] */
#define VD_ACT_QUICK_GELU 2 /* x * sigmoid(1.702 x)  (HF CLIP)                                 */
#define VD_ACT_SILU 3
#define VD_ACT_GELU_TANH 4  /* 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))  (GPT-2 MLP of the Optimus decoder) */

/*
 * One fused GEMM / implicit-GEMM convolution:
 *    out[m][n] = ( act( sum_k A[m][k] W[n][k] + bias + rowvec ) ) * alpha + res[m][n]
 * With VD_EPI_LNFOLD the A rows are layer-normalised over K on the fly:
 *    LN(a)[m][k] = (a[m][k] - mean_m) * rstd_m * gamma[k] + beta[k]
 *    sum_k LN(a)[m][k] W[n][k] = rstd_m * ( sum_k a[m][k] W'[n][k] - mean_m * colsum[n] ) + bias'[n]
 * with W' = gamma (*) W (passed as `w`), colsum[n] = sum_k W'[n][k] (fp32) and bias' = beta W^T + bias (passed as `bias`),
 * all prepared once per layer by the host.  (mean_m, rstd_m) are read from `ln_stats` (vd_row_stats_f16: two-pass
 * statistics, one extra read of A).  With VD_EPI_LN_INLOOP and `ln_stats` == NULL the kernel instead accumulates sum and sum
 * of squares of every A row from the operand fragments inside its K loop (biased variance, `ln_eps`; one-pass E[x^2] - mean^2
 * on the raw fp16 values, less robust for |mean| >> std, hence opt-in: a NULL `ln_stats` without the flag is an error), so
 * the nn.LayerNorm in front of a projection (lib/model_zoo/attention.py:214-218) costs no pass over memory and no launch.
 * Plain (non-conv, single-source) A only, no split-K.
 * A[m][k] is gathered on the fly: m -> (b, oy, ox) over Hout x Wout, k -> (ky, kx, c) with c running
 * over the channels of a0 (c0) then a1 (c1) -- i.e. torch.cat([a0, a1], dim=1) is never materialised --
 * at input pixel ((oy*stride - pad + ky) >> ups, (ox*stride - pad + kx) >> ups) (ups=1: nearest 2x upsample
 * fused in front of the conv).  Plain matrices: set Hout = Wout = 0.
 */
typedef struct VdGemmDesc {
    const void* a0;      /* fp16 activation source 0, row stride lda0 (elements)                 */
    const void* a1;      /* optional fp16 source 1 (channel concat), row stride lda1             */
    const void* w;       /* fp16 [N][ldw]                                                        */
    const void* bias;    /* fp16 [N] (or [M] with VD_EPI_BIAS_ALONG_M)                            */
    const void* rowvec;  /* fp16 [M / rows_per_batch][N]                                          */
    const void* res;     /* fp16 [M][ldr]                                                        */
    void* out;           /* fp16 (or fp32) [M][ldc]                                              */
    float* ws;           /* split-K workspace (vd_gemm_workspace_bytes), may be NULL             */
    int32_t M, N, K;
    int32_t c0, c1, lda0, lda1, ldw, ldc, ldr;
    int32_t Hin, Win, Hout, Wout, ksize, stride, pad, ups;
    int32_t rows_per_batch;
    int32_t flags, act;
    float alpha;
    int32_t batch;       /* blockIdx.z batches with the element strides below                    */
    int32_t split_k;     /* 0 = heuristic                                                        */
    int64_t stride_a, stride_w, stride_out, stride_res;
    const float* colsum; /* VD_EPI_LNFOLD: fp32 [N] row sums of w                                */
    float ln_eps;        /* VD_EPI_LNFOLD with ln_stats == NULL: epsilon of the in-loop statistics              */
    int32_t reserved;
    int32_t* sync;       /* optional split-K arrival counters: VD_GEMM_SYNC_INTS ints, ZERO before their first use and
                          * private to the stream (launches on one stream are ordered; the kernel leaves them zero).  With
                          * them the last-arriving block of each output tile sums the tile's fp32 slabs (in split order:
                          * results stay run-to-run identical) and runs the fused epilogue itself -- no reduce launch.   */
    const float* ln_stats; /* VD_EPI_LNFOLD: fp32 [batch*M][2] = (mean, rstd) of every A row from vd_row_stats_f16 (NULL only
                            * with VD_EPI_LN_INLOOP)                                                                */
    float* out_stats;      /* optional (ABI 5): per-channel statistics of the STORED output for a consuming GroupNorm, fp32
                            * [M / R][N][2] = (mean, M2 = sum (x - mean)^2) over blocks of R rows of one image; R =
                            * vd_gemm_stat_rows(desc) (depends on the launch the planner picks; 0 = this launch cannot emit
                            * them: leave out_stats NULL and use vd_chan_stats_f16).  fp16 output, batch 1, N % 8 == 0.     */
    int32_t stat_img_rows; /* rows of one image for out_stats (partials never mix images); 0 = Hout * Wout (M for plain matrices) */
    int32_t gn_groups;     /* reserved, must be 0 / NULL / 0 (ABI 5-7: operands of VD_EPI_GROUPNORM, the consuming GroupNorm inside the */
    const void* gn_gamma;  /* kernel that sums split-K slabs; measured neutral against out_stats + the apply launch and removed in   */
    const void* gn_beta;   /* ABI 8 -- the fields keep the descriptor layout)                                                       */
    float gn_eps;
    int32_t reserved3;
    /* Skip 1x1 convolution folded into a 3x3 convolution (ABI 5): out += W_s [N][skip_c0 + skip_c1] . cat(skip_a0, skip_a1)[pixel]
     * -- ResBlock's `skip_connection(x) + h` (lib/model_zoo/openaimodel.py:238-251,272-274) as extra K of the second conv
     * instead of its own GEMM and a residual round trip.  skip_a0 / skip_a1: fp16 tensors on the OUTPUT grid (row strides
     * skip_lda0 / skip_lda1, channels multiples of 64); skip_w: fp16 [N][skip_ldw], K-contiguous.  Only the halo-resident
     * convolution takes it (vd_gemm_skip_ok); its bias belongs into `bias`. */
    const void* skip_a0;
    const void* skip_a1;
    const void* skip_w;
    int32_t skip_c0, skip_c1, skip_lda0, skip_lda1, skip_ldw, reserved4;
    /* Row statistics for a consuming LayerNorm fold (ABI 6): int64 [M][2], ZEROED by the caller; every block adds (atomically)
     * the sum and the sum of squares of the fp16 values it stores over its columns of each row, in fixed point (sum x 2^24, sum
     * of squares x 2^16: integer adds, so the result does not depend on the order the blocks arrive in), so after the launch
     * row_sums[m] = (sum_n out[m][n], sum_n out[m][n]^2) -- the statistics half of the nn.LayerNorm in front of the NEXT
     * projection (lib/model_zoo/attention.py:214-218) without vd_row_stats_f16's launch and extra read.  The consumer passes the
     * buffer as ln_stats with VD_EPI_LN_SUMS.  Only unsplit gemm_f16_kernel launches with vector-aligned fp16 output take it:
     * ask vd_gemm_row_sums_ok(desc) first. */
    void* row_sums;
    /* Per-(image, channel) sums for a consuming GroupNorm (ABI 7), next to out_stats: int64 [images][N][2], ZEROED by the caller.
     * Every launch that writes an out_stats partial (mean, M2 over R rows of one image) also adds, atomically and in fixed point,
     * R * mean x 2^32 and (M2 + R * mean^2) x 2^16 (formed in fp64 from the shifted partial) for the image the partial lies in
     * (row / stat_img_rows), so after the launch stat_sums[img][n] = (sum, sum of squares) over the image's rows of channel n:
     * ONE pair per (image, channel) whatever the producer's tile shape, which the consumer folds itself (vd_gn_apply_sums_f16:
     * no vd_gn_table_f32 launch).  Integer adds: the result does not depend on the order the blocks arrive in.  Needs out_stats
     * and stat_img_rows > 0; launchers that cannot emit out_stats ignore it (the consumer checks the producer's report). */
    void* stat_sums;
} VdGemmDesc;
#define VD_GEMM_SYNC_INTS 16384

/* Replaces nn.Conv2d / nn.Linear / torch.bmm call sites:
 *   lib/model_zoo/openaimodel.py:89-117 (Upsample), :133-159 (Downsample), :254-274 (ResBlock._forward)
 *   lib/model_zoo/attention.py:37-64 (GEGLU FF), :170-193 (q/k/v/out projections), :255-266 (proj_in/out)
 *   lib/model_zoo/autokl_modules.py:42-79,82-141,150-202 (VAE convs, AttnBlock bmm)
 *   HF CLIP linear layers reached from lib/model_zoo/clip.py:58-61,95-100 */
int vd_gemm_f16(const VdGemmDesc* desc, hipStream_t stream);
size_t vd_gemm_workspace_bytes(const VdGemmDesc* desc);
/* 1 when the launch vd_gemm_f16 would plan for `desc` can accumulate VdGemmDesc.row_sums (see there), else 0. */
int vd_gemm_row_sums_ok(const VdGemmDesc* desc);
/* Dry run of the launch planner: tile_cfg indexes the instantiation table of vd_gemm_config_name(); nsplit = split-K
 * factor.  Lets bench.py attribute measured time / algorithmic FLOPs to the kernel instantiation that actually ran. */
int vd_gemm_plan(const VdGemmDesc* desc, int* tile_cfg, int* nsplit);
/* Rows per statistics partial the launch planned for `desc` would write to desc->out_stats (the pointer itself is not
 * read): the halo-resident convolution emits one partial per 256-pixel patch (or per whole small image), gemm_f16_kernel one
 * per min(tile rows, image rows), the split-K reduce one per 64 rows.  *rows = 0: no statistics from this launch. */
int vd_gemm_stat_rows(const VdGemmDesc* desc, int* rows);
/* 1 when the launch planned for `desc` takes the folded skip 1x1 convolution (skip_a0 / skip_w set): the halo-resident 3x3
 * convolution with 256 x 160 blocks, no upsample, the skip tensors on the output grid. */
int vd_gemm_skip_ok(const VdGemmDesc* desc);
/* "gemm_f16_kernel<BM,BN,WM,WN,NT,STAGES,KB>" of tile_cfg (NULL when out of range); vd_gemm_num_configs() entries. */
const char* vd_gemm_config_name(int tile_cfg);
int vd_gemm_num_configs(void);
/* Development hook (tools/gemm_sweep.py, A/B runs): force every following vd_gemm_f16 of this process onto tile_cfg
 * (-1 = planner's choice) where the shape permits.  Process-global and unsynchronised: not for production use. */
int vd_gemm_set_override(int tile_cfg);
/* 3x3 / stride 1 / pad 1 convolutions (VdGemmDesc.ksize = 3) whose output grid tiles into 8 x 32 pixel patches run on
 * conv3x3_halo_kernel: the (rows + 2) x (cols + 2) input halo of a patch is staged in LDS once per 64-channel chunk and the
 * nine taps read shifted views of it, instead of gemm_f16_kernel's nine gathers (ResBlock / Upsample / VAE convs:
 * lib/model_zoo/openaimodel.py:89-117,254-274, autokl_modules.py:82-141).  vd_gemm_plan reports these launches as
 * tile_cfg = vd_gemm_num_configs() + variant, 0 <= variant < VD_CONV_HALO_VARIANTS (vd_gemm_config_name knows them).
 * Development hook: -1 = planner's choice (default; also the environment variable VD_CONV_HALO), 0 = never (every conv on
 * gemm_f16_kernel), k > 0 = force variant k - 1 where the geometry permits.  Process-global like vd_gemm_set_override. */
#define VD_CONV_HALO_VARIANTS 13
int vd_conv_halo_set_variant(int setting);
/* Tuned launch table: a problem (M, N, K, ksize, epilogue class: bit 0 GEGLU, bit 1 LayerNorm fold, bit 2 two-source A) is
 * launched with tile_cfg / split-K nsplit (0 / 1 = none) instead of the cost model's choice.  The host loads the table
 * (lib/gemm_tune.py) from a file tools/tune_forward.py measured inside a UNet forward -- the setting that decides, since
 * weights then stream from HBM and activations come hot from the previous kernel.  Thread-safe. */
/* The 3x3 / stride 1 / pad 1 convolutions on 8x8 images (the ResBlocks at ds = 8: lib/model_zoo/openaimodel.py:254-274 with
 * 1280 / 2560 input channels) as a WEIGHT-STREAMING kernel: M = images x 64 is tiny, the layer is its 29.5 / 59 MB weight
 * stream.  `desc` as for vd_gemm_f16 (its `w` is not read; `ws` must hold vd_gemm_workspace_bytes); `w_stream` holds the same
 * weights in MFMA-fragment order, fp16 [N / 32][(c0 + c1) / 64][9 taps][4 k-steps][64 lanes][8]: lane l of the fragment of
 * (n tile t, chunk c, tap, k-step s) holds W[32 t + (l & 31)][tap][64 c + 16 s + 8 (l >> 5) .. + 8] (vd_hip/pack.py:
 * pack_conv_weight_stream) -- every A operand of an MFMA is one coalesced 1-KiB load straight into registers, the input halo
 * of a chunk is staged in LDS once, K is split over chunks (fp32 slabs + the reduce kernel, which runs desc's epilogue and
 * emits desc->out_stats in partials of 64 rows when asked).  A folded skip convolution (desc->skip_a0 / skip_a1 / skip_c0 /
 * skip_c1) is taken too: desc->skip_w then holds the 1x1 weights in fragment order, fp16 [N / 32][(skip_c0 + skip_c1) / 64][4]
 * [64 lanes][8] (pack_linear_weight_stream).  vd_conv3x3_wstream_supported: 1 when desc's geometry fits. */
int vd_conv3x3_wstream_f16(const VdGemmDesc* desc, const void* w_stream, hipStream_t stream);
/* vd_gemm_wstream_f16: plain GEMM y = x W^T (+ fused epilogue of the descriptor) for long-K, small-M projections -- the output
 * projection of the gated feed-forward at the 16x16 / 8x8 levels (lib/model_zoo/attention.py:37-64, FeedForward.net[2]) -- with
 * the weights in MFMA-fragment order (w_stream: fp16 [N / 32][K / 64][4][64 lanes][8], pack_linear_weight_stream) streamed
 * straight into registers; only the activation tile takes the LDS path.  Split over K in 64-deep chunks + the split-K reduce
 * (needs desc->ws, vd_gemm_workspace_bytes).  vd_gemm_wstream_supported: 1 when desc's shape fits (single source, M % 128 ==
 * 0, N % 256 == 0, K % 64 == 0, plain fp16 epilogue). */
int vd_gemm_wstream_supported(const VdGemmDesc* desc);
int vd_gemm_wstream_f16(const VdGemmDesc* desc, const void* w_stream, hipStream_t stream);
int vd_conv3x3_wstream_supported(const VdGemmDesc* desc);
/* Split factors the two weight-streaming launchers will use for `desc` (ABI 6): set VdGemmDesc.split_k to *nsplit before sizing
 * the workspace with vd_gemm_workspace_bytes.  vd_conv3x3_wstream_plan answers 0 when the launch goes to the whole-K kernel
 * (conv_wsk_kernel.h, round 5: a block owns 128 pixels x 32 channels for the whole K, its four waves split the k-steps, the
 * fused epilogue and the GroupNorm statistics run in the kernel): no workspace, no reduce launch. */
int vd_conv3x3_wstream_plan(const VdGemmDesc* desc, int* nsplit);
int vd_gemm_wstream_plan(const VdGemmDesc* desc, int* nsplit);
/* vd_gemm_wstream_cat_f16: vd_gemm_wstream_f16 over a CONCATENATED K axis, y = [a0 | a1] W^T: chunk c of the activation tile
 * comes from desc->a0 (lda0) while c < c0 / 64 and from desc->a1 (lda1) after that (c0 % 64 == 0, c1 % 64 == 0, K = c0 + c1; a1 may
 * be null: one source); w_stream is ONE fragment-order stream over K (pack_linear_weight_stream of the concatenated matrix).  A
 * block takes up to 34 chunks, so K = 6400 on 2048 rows runs as 3 splits (240 blocks) -- FeedForward.net[2] with
 * SpatialTransformer.proj_out folded in (A = [h | x2], vd_hip/pack.py: pack_ff_proj_fold).  The reduce runs desc's epilogue (bias,
 * alpha, residual) and emits desc->out_stats in partials of 64 rows when asked.  _supported / _plan as for vd_gemm_wstream_f16;
 * the answers of those three entries are unchanged. */
int vd_gemm_wstream_cat_supported(const VdGemmDesc* desc);
int vd_gemm_wstream_cat_plan(const VdGemmDesc* desc, int* nsplit);
int vd_gemm_wstream_cat_f16(const VdGemmDesc* desc, const void* w_stream, hipStream_t stream);
/* vd_gemm_wstream_epi_f16: the same weight-streaming main loop over the WHOLE K in one block (K / 64 <= 32 chunks, no split: no
 * workspace, no reduce launch) with the fused epilogue of vd_gemm_f16 in the kernel -- the LayerNorm-folded projections of a
 * transformer block at widths 640 / 1280, norm1 -> q | k | v and norm3 -> GEGLU (lib/model_zoo/attention.py:37-45,170-176,214-218).
 * `desc` as for vd_gemm_f16 (its `w` is not read); w_stream: the same [N][K] weights -- GEGLU-packed per 64 rows as [32 value |
 * 32 gate] where act = VD_ACT_GEGLU -- in fragment order (pack_linear_weight_stream; for GEGLU pack_linear_weight_stream(pack_geglu(w))):
 * value and gate of an output then sit in the same lane and register of a wave's two MFMA tiles.  Epilogue: VD_EPI_BIAS,
 * VD_EPI_LNFOLD with either form of ln_stats ((mean, rstd) table or VD_EPI_LN_SUMS), alpha, act none or GEGLU, fp16 output in
 * 16-byte row segments; the float sequence is gemm_f16_kernel's, so results agree with vd_gemm_f16 on the same operands bit for bit
 * wherever the fp32 sums over K agree (both add 16-deep products in ascending K).  Two blocks share a CU (238 VGPRs, no scratch).
 * vd_gemm_wstream_epi_supported: 1 for a plain single-source matrix (Hout = Wout = 0, ksize <= 1), batch 1, M % 128 == 0,
 * N % 64 == 0 (GEGLU: N % 128 == 0; a block covers 256 columns, the waves past N idle), K % 64 == 0, K <= 2048, split_k <= 1,
 * no residual / rowvec / fp32 output / in-loop statistics / out_stats / row_sums / stat_sums / skip convolution / sync. */
int vd_gemm_wstream_epi_supported(const VdGemmDesc* desc);
int vd_gemm_wstream_epi_f16(const VdGemmDesc* desc, const void* w_stream, hipStream_t stream);
/* Development hook: kernel instance (0 = default) and the grid size the split over chunks aims for (256). Process-global. */
int vd_conv3x3_wstream_set_variant(int variant, int target_blocks);
/* The 3x3 / stride 1 / pad 1 convolution behind a nearest-2x upsample (VdGemmDesc.ups = 1: Upsample.conv of the UNet and of the
 * VAE decoder, lib/model_zoo/openaimodel.py:89-117, autokl_modules.py:42-56) as four 2x2 PHASE convolutions of the
 * low-resolution image.  Output pixel (2i + a, 2j + b), a, b in {0, 1}, sees only a 2x2 window of source pixels; the 3x3 weights
 * that meet the same source pixel are summed once at pack time:
 *     out[2i + a][2j + b][n] = sum_{p, q in {0, 1}} sum_c Wph[a][b][n][p][q][c] x[i + a - 1 + p][j + b - 1 + q][c]
 *     Wph[a][b][n][p][q][c]  = sum_{ky in R(a, p)} sum_{kx in R(b, q)} w[n][ky][kx][c]
 *     R(0, 0) = {0}, R(0, 1) = {1, 2}, R(1, 0) = {0, 1}, R(1, 1) = {2};  source indices outside the image read zero
 * so the launch executes 4 / 9 of the multiplies of the upsampled form.  The sums are exact algebra with ONE added rounding: w_phase
 * (fp16 [4 phases = 2a + b][N][4 taps = 2p + q][C], vd_hip/pack.py: pack_conv_weight_ups_phase) holds the fp32 sums of the fp16
 * weights rounded to fp16 once, so results agree with vd_gemm_f16 on the same descriptor to that rounding (bit for bit where
 * every sum is exact), not bit for bit in general.  `desc` as for vd_gemm_f16 (single source, ups = 1, its `w` is validated but
 * not read; every epilogue of the halo-resident convolution, out_stats / stat_sums included); the TAPS = 4 instances of
 * conv3x3_halo_kernel run it, split over channel chunks + the split-K reduce where the grid is small (needs desc->ws).
 * vd_conv3x3_ups_phase_supported: 1 when desc's geometry fits (else the caller stays on vd_gemm_f16).
 * vd_conv3x3_ups_phase_plan: the instance (vd_conv3x3_ups_phase_name), the split factor (set VdGemmDesc.split_k to it before
 * sizing the workspace) and the rows per out_stats partial (0: none) the launch will use. */
int vd_conv3x3_ups_phase_supported(const VdGemmDesc* desc);
int vd_conv3x3_ups_phase_plan(const VdGemmDesc* desc, int* variant, int* nsplit, int* stat_rows);
const char* vd_conv3x3_ups_phase_name(int variant);
int vd_conv3x3_ups_phase_f16(const VdGemmDesc* desc, const void* w_phase, hipStream_t stream);
/* (a tile_cfg that is not built is refused: non-zero return, table unchanged) */
int vd_gemm_tune_set(int M, int N, int K, int ksize, int epi_class, int tile_cfg, int nsplit);
int vd_gemm_tune_clear(void);

/* y[M][N] = [LayerNorm](x[M][320]) W[N][320]^T + bias (+ res) with the block's 128 rows of x resident in registers (no activation
 * tile, no activation DMA): the K = 320 projections of the UNet's 64x64 level (proj_in / proj_out / to_out, N = 320; the fused
 * q | k | v projection, N = 960, with the LayerNorm applied in registers).  x: fp16 [M][320] contiguous; w: fp16 [N][320]
 * (gamma-folded when layernorm != 0), bias: fp16 [N] or NULL (beta W^T + bias when layernorm != 0), res: fp16 [M][N] or NULL,
 * y: fp16 [M][N]; N a multiple of 320 (vd_gemm_row320_supported).  Same result as vd_gemm_f16 on the same operands
 * (VD_EPI_BIAS | VD_EPI_RESIDUAL | VD_EPI_LNFOLD) up to fp16 rounding of the normalised rows.
 * Replaces nn.Linear / 1x1 nn.Conv2d of lib/model_zoo/attention.py:159-163,170-193,245-258 at inner width 320. */
int vd_gemm_row320_f16(const void* x, const void* w, const void* bias, const void* res, void* y, int64_t M, int N,
                       int layernorm, float ln_eps, hipStream_t stream);
int vd_gemm_row320_supported(int64_t M, int N, int K);

/* The entry of a SpatialTransformer at inner width 320 in one launch (after the statistics): GroupNorm applied as a per-sample
 * affine map -> proj_in -> h (the residual stream, written out), LayerNorm(h) -> fused q | k | v projection:
 *     h = (x * scale[img] + shift[img]) W1^T + b1,     y2 = LayerNorm(h) W2^T + b2
 * gn_center (ABI 7, may be NULL): fp16 [M / rows_per_image][320] = fp16(group mean) per channel; the map is then applied as
 * (x - center) * scale + shift with shift = beta - (mean - center) * scale (vd_gn_affine_from_stats_f16 with `center`): x - center is
 * exact in fp16 near the mean and both operands are O(1), so the fp16 map loses 2^-11 of the NORMALISED value instead of
 * |mean| / sigma * 2^-11.
 * x, h: fp16 [M][320]; gn_scale / gn_shift: fp16 [M / rows_per_image][320] from vd_groupnorm_affine_f16; w1: fp16 [320][320],
 * b1: fp16 [320]; w2: fp16 [N2][320] with the LayerNorm's gamma folded in, b2: fp16 [N2] = beta W2^T (or NULL); y2: fp16
 * [M][N2], N2 a multiple of 320; rows_per_image a multiple of 128.  Replaces Normalize -> proj_in (lib/model_zoo/
 * attention.py:236-258), norm1 and to_q / to_k / to_v (:214, :170-176) and this library's vd_groupnorm_silu_f16 (apply pass) ->
 * vd_gemm_f16 -> vd_gemm_row320_f16 chain. */
int vd_gemm_row320_chain_f16(const void* x, const void* gn_scale, const void* gn_shift, const void* gn_center, int rows_per_image, const void* w1,
                             const void* b1, void* h, const void* w2, const void* b2, void* y2, int64_t M, int N2,
                             float ln_eps, hipStream_t stream);
/* GroupNorm statistics as a per-(sample, channel) affine map: scale = rstd * gamma, shift = beta - mean * scale (fp16 [B][C]),
 * for consumers that apply the normalisation themselves.  stats: fp32 scratch of vd_groupnorm_workspace_bytes(). */
int vd_groupnorm_affine_f16(const void* x, const void* gamma, const void* beta, void* scale, void* shift, float* stats, int B,
                            int HW, int C, int groups, float eps, hipStream_t stream);

/* The gated feed-forward of a BasicTransformerBlock in one launch (inner width C = 320 only: vd_ff_geglu_supported):
 *     y[m] = res[m] + ( v (*) gelu_erf(g) ) W2^T + b2,     [v | g] = LayerNorm(x[m]) W1^T + b1
 * x, res, y: fp16 [M][C]; w1_packed: fp16 [8C][C] with LayerNorm's gamma folded in (W1 * gamma) and rows packed per 64 as
 * [32 value | 32 gate] (VD_ACT_GEGLU layout); b1_packed: fp16 [8C] = beta W1^T + b1, packed likewise; w2: fp16 [C][4C];
 * b2: fp16 [C].  The rows of x are layer-normalised in registers (biased variance, ln_eps), the [M, 4C] intermediate never
 * leaves the chip.  Replaces norm3 -> ff (GEGLU -> Linear) -> + x of lib/model_zoo/attention.py:37-64,214-218 and this
 * library's vd_row_stats_f16 -> vd_gemm_f16(VD_ACT_GEGLU | VD_EPI_LNFOLD) -> vd_gemm_f16(VD_EPI_RESIDUAL) chain. */
int vd_ff_geglu_f16(const void* x, const void* w1_packed, const void* b1_packed, const void* w2, const void* b2,
                    const void* res, void* y, int64_t M, int C, float ln_eps, hipStream_t stream);
int vd_ff_geglu_supported(int C);
/* The same feed-forward with the C x C projections on either side of it in the SAME launch (ABI 6, C = 320:
 * vd_ff_chain_supported) -- the row-local tail of a 64x64-level transformer block,
 *     x1  = a wo^T + bo + x                 (given a: CrossAttention.to_out + residual, attention.py:192-193,216)
 *     y   = x1 + FF(LayerNorm(x1))           (attention.py:37-64,217)
 *     out = alpha (y wp^T + bp) + res        (given wp: SpatialTransformer.proj_out + skip / context mixing, attention.py:262-266)
 * instead of vd_gemm_f16 -> vd_ff_geglu_f16 -> vd_gemm_f16.  Without `a` the feed-forward reads x itself; without `wp` it
 * stores y.  x1_scratch: [M][C] fp16 the kernel parks x1 in (needed with `a`).  out_stats (with wp, M % 128 == 0): fp32
 * [M / 128][C][2] per-channel (mean, M2) over blocks of 128 stored rows, the VdGemmDesc.out_stats format with R = 128. */
typedef struct VdFfChain {
    const void* x;          /* fp16 [M][C] */
    const void* a;          /* fp16 [M][C] or NULL */
    const void* wo;         /* fp16 [C][C] */
    const void* bo;         /* fp16 [C] */
    void* x1_scratch;       /* fp16 [M][C] */
    const void* w1_packed;  /* fp16 [8C][C]: LayerNorm-folded, GEGLU-packed (as vd_ff_geglu_f16) */
    const void* b1_packed;  /* fp16 [8C] */
    const void* w2;         /* fp16 [C][4C] */
    const void* b2;         /* fp16 [C] */
    const void* wp;         /* fp16 [C][C] or NULL */
    const void* bp;         /* fp16 [C] */
    const void* res;        /* fp16 [M][C]: residual of the last projection */
    void* out;              /* fp16 [M][C] */
    float* out_stats;       /* or NULL */
    void* stat_sums;        /* or NULL (with out_stats): int64 [M / stat_img_rows][C][2], as VdGemmDesc.stat_sums (ABI 7) */
    int64_t stat_img_rows;  /* rows of one image (a multiple of 128) for stat_sums */
    int64_t M;
    int32_t C;
    float ln_eps, alpha;
    int32_t period_rows;    /* 0 (or M): off.  0 < period_rows < M: x (given a) and res hold period_rows rows and output row m reads
                             * their row m % period_rows -- the replicas of a classifier-free-guidance batch share them.  Needs
                             * stat_img_rows (rows of one image, % 128 == 0) dividing period_rows, and period_rows dividing M. */
} VdFfChain;
int vd_ff_chain_f16(const VdFfChain* chain, hipStream_t stream);
int vd_ff_chain_supported(int C);

/* GroupNorm(groups) [+ SiLU] over channels-last input that may be the concatenation of two tensors.
 * stats is a caller-provided fp32 scratch of vd_groupnorm_workspace_bytes().
 * Replaces GroupNorm32 + SiLU (lib/model_zoo/diffusion_utils.py:175-191, openaimodel.py:196-200,230-237),
 * Normalize (attention.py:76-77, autokl_modules.py:38-39) and the torch.cat in vd.py:371. */
int vd_groupnorm_silu_f16(const void* x0, int c0, const void* x1, int c1, const void* gamma, const void* beta,
                          void* y, float* stats, int B, int HW, int groups, float eps, int apply_silu,
                          hipStream_t stream);
size_t vd_groupnorm_workspace_bytes(int B, int HW, int C, int groups);

/* ---- GroupNorm without its own statistics pass (ABI 5, csrc/gn_fused.hip) ----------------------------------------------
 * The producer of a tensor emits per-channel partial statistics while it stores it (VdGemmDesc.out_stats): fp32
 * [B * T][C][2] = (mean, M2 = sum (x - mean)^2) over T blocks of HW / T rows per sample.  Per channel, so the consumer folds
 * the channels of one tensor, or of both tensors of a skip concat (vd.py:371), into its groups whatever the producers' tile
 * shapes were, and a tensor consumed twice (every skip connection) is measured once.
 * vd_groupnorm_from_stats_f16: y = GroupNorm(cat(x0, x1)) [+ SiLU] in ONE launch that reads x once -- each block folds the
 *   partials of its groups (Chan's parallel variance update, fp32) and streams its panel.  Same contract as
 *   vd_groupnorm_silu_f16 otherwise; replaces GroupNorm32 + SiLU / Normalize at the same reference lines.
 * vd_chan_stats_f16: the same partials computed with one read of x [M][C] (row stride ldx), one per rows_per_partial
 *   consecutive rows (a divisor of the sample's row count): for tensors whose producer cannot emit them, and the reference
 *   the producers are tested against.
 * vd_gn_table_f32: partials -> the normalisation as a per-(sample, channel) affine map, fp32 table [B][2][C0 + C1]:
 *   scale = rstd * gamma, shift = beta - mean * scale;  vd_gn_apply_table_f16: y = act(x * scale + shift), elementwise. */
int vd_groupnorm_from_stats_f16(const void* x0, int c0, const float* stats0, int T0, const void* x1, int c1,
                                const float* stats1, int T1, const void* gamma, const void* beta, void* y, int B, int HW,
                                int groups, float eps, int apply_silu, hipStream_t stream);
int vd_chan_stats_f16(const void* x, long M, int C, int ldx, int rows_per_partial, float* stats, hipStream_t stream);
int vd_gn_table_f32(const float* stats0, int T0, int c0, const float* stats1, int T1, int c1, int B, int HW,
                    const void* gamma, const void* beta, int groups, float eps, float* table, hipStream_t stream);
int vd_gn_apply_table_f16(const void* x0, int c0, const void* x1, int c1, int B, int HW, const float* table, int apply_silu,
                          void* y, hipStream_t stream);
/* vd_gn_apply_sums_f16 (ABI 7): y = act(GroupNorm(cat(x0, x1))) from the per-(image, channel) fixed-point sums the producers
 * accumulated (VdGemmDesc.stat_sums: sums0 int64 [B][c0][2], sums1 int64 [B][c1][2] or NULL): every block folds the sums of its
 * image into (mean, rstd) per group in fp64 (8 lanes per group, no partial lists), builds scale / shift of its channel octets in
 * registers and streams its rows once.  groups <= 32.  Replaces the vd_gn_table_f32 + vd_gn_apply_table_f16 pair (same reference
 * lines as vd_groupnorm_silu_f16). */
int vd_gn_apply_sums_f16(const void* x0, int c0, const void* sums0, const void* x1, int c1, const void* sums1, int B, int HW,
                         const void* gamma, const void* beta, int groups, float eps, int apply_silu, void* y, hipStream_t stream);
/* The same map as fp16 [B][C0 + C1] scale / shift vectors: the gn_scale / gn_shift operands of vd_gemm_row320_chain_f16
 * (what vd_groupnorm_affine_f16 computes with a pass over x).  center (ABI 7, may be NULL): fp16 [B][C0 + C1] = fp16(group mean);
 * shift is then beta - (mean - center) * scale, for the centred application described at vd_gemm_row320_chain_f16. */
int vd_gn_affine_from_stats_f16(const float* stats0, int T0, int c0, const float* stats1, int T1, int c1, int B, int HW,
                                const void* gamma, const void* beta, int groups, float eps, void* scale, void* shift,
                                void* center, hipStream_t stream);

/* GroupNorm(groups) [+ SiLU] of the 0-D (text-latent) data flow: FCBlock normalises the flattened [C, sdim] vector of a
 * sample with one affine pair per flat element (reference openaimodel.py:2084-2141 with the [C, sdim, 1] -> C*sdim view
 * of FCBlock_MultiDim, :2295-2332).  x0 (++ x1 on channels): [B, S, C] channels-last; gamma / beta: [S, C] (the
 * reference's c * sdim + s order re-ordered once at load); y: [B, S, C]. */
int vd_groupnorm0d_silu_f16(const void* x0, int c0, const void* x1, int c1, const void* gamma, const void* beta, void* y,
                            int B, int S, int groups, float eps, int apply_silu, hipStream_t stream);

/* LayerNorm over the last dim of [rows][C]. Replaces nn.LayerNorm in BasicTransformerBlock
 * (lib/model_zoo/attention.py:205-207) and the HF CLIP layer norms. */
int vd_layernorm_f16(const void* x, const void* gamma, const void* beta, void* y, int rows, int C, float eps,
                     hipStream_t stream);
/* (mean, rstd = 1 / sqrt(var + eps)) of every row of x [rows][ldx >= C] (fp16, biased variance over the C columns,
 * two-pass in registers) -> stats fp32 [rows][2]: the statistics half of nn.LayerNorm for VD_EPI_LNFOLD. */
int vd_row_stats_f16(const void* x, float* stats, int64_t rows, int C, int64_t ldx, float eps, hipStream_t stream);

/* Fused softmax(Q K^T * scale) V, online softmax, no score tensor in HBM.
 * q [B][Nq][ldq], k/v [B][Nk][ldk/ldv], out [B][Nq][ldo]; head h occupies columns h*D..h*D+D-1.
 * D in {40, 64, 80, 160}.  causal = 1 masks key > query (CLIP text tower); causal = 1 + n masks key > query + n (n memory
 * slots in front of the keys that every query sees: the latent memory of the Optimus GPT-2 decoder, n = 1).
 * Replaces CrossAttention.forward einsum/softmax/einsum (lib/model_zoo/attention.py:176-191). */
int vd_attention_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                     int ldq, int ldk, int ldv, int ldo, int64_t sq, int64_t sk, int64_t sv, int64_t so,
                     float scale, int causal, hipStream_t stream);

/* The query side of a cross-attention layer in one launch (vd_xattn_supported: head dim 40 / 80 / 160, width H*D a
 * multiple of 64):
 *     out[b, n, h*D..] = softmax( (LayerNorm(x[b, n]) Wq_h^T) K_h^T * scale ) V_h
 * x, out: fp16 [B][Nq][H*D] contiguous; wq: fp16 [H*D][H*D] with LayerNorm's gamma folded in, bq: fp16 [H*D] = Wq beta (or
 * NULL), colsum: fp32 [H*D] row sums of the folded wq (the VD_EPI_LNFOLD operands of vd_gemm_f16); k / v [B][Nk][ldk / ldv]
 * the pre-projected context, head h in columns h*D..h*D+D-1.  Row statistics (biased variance, ln_eps) are accumulated
 * inside the projection loop; the query tensor never exists in memory.  Replaces norm2 -> to_q -> einsum -> softmax ->
 * einsum of lib/model_zoo/attention.py:170-193,216 and this library's vd_row_stats_f16 -> vd_gemm_f16(VD_EPI_LNFOLD) ->
 * vd_attention_f16 chain. */
int vd_xattn_f16(const void* x, const void* wq, const void* bq, const float* colsum, float ln_eps, const void* k,
                 const void* v, void* out, int B, int H, int Nq, int Nk, int D, int ldk, int ldv, int64_t sk, int64_t sv,
                 float scale, hipStream_t stream);
int vd_xattn_supported(int H, int D);
/* vd_xattn_f16 with x shared by the replicas of a sample: x is fp16 [x_samples][Nq][H*D] and sample b of k / v / out reads
 * sample b % x_samples of it (B a multiple of x_samples; x_samples == B is vd_xattn_f16).  The batch the reference feeds under
 * classifier-free guidance is [x; x] (lib/model_zoo/ddim.py:144-149): up to the first cross-attention the replicas are equal
 * and need not be materialised. */
int vd_xattn_rep_f16(const void* x, const void* wq, const void* bq, const float* colsum, float ln_eps, const void* k,
                     const void* v, void* out, int B, int x_samples, int H, int Nq, int Nk, int D, int ldk, int ldv,
                     int64_t sk, int64_t sv, float scale, hipStream_t stream);

/* Row softmax fp32 [rows][n] -> fp16 (VAE AttnBlock, lib/model_zoo/autokl_modules.py:192). */
int vd_softmax_rows_f32_f16(const float* s, void* p, int64_t rows, int n, hipStream_t stream);
/* softmax(scale * s) per row in fp32: token probabilities of the Optimus GPT-2 decoder, scale = 1 / temperature
 * (lib/model_zoo/optimus.py:679-681: logits / temperature -> softmax -> multinomial). */
int vd_softmax_rows_f32_f32(const float* s, float* p, int64_t rows, int n, float scale, hipStream_t stream);

/* Sinusoidal timestep embedding, fp32 math, fp16 out [B][dim] = [cos | sin].
 * Replaces timestep_embedding (lib/model_zoo/diffusion_utils.py:131-151). */
int vd_timestep_embedding_f16(const int64_t* t, void* out, int B, int dim, float max_period, hipStream_t stream);

/* Classifier-free-guidance combine + DDIM update in one pass (fp32 math):
 *   e = e_u + s (e_c - e_u); pred_x0 = (x - sqrt(1-a_t) e)/sqrt(a_t);
 *   x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma^2) e + sigma * noise
 * eps holds [e_uncond ; e_cond] (2n elements) when guided != 0, else n elements.
 * Replaces p_sample_ddim (lib/model_zoo/ddim.py:144-170). */
int vd_cfg_ddim_step_f16(const void* x, const void* eps, const void* noise, void* x_prev, void* pred_x0, int64_t n,
                         int guided, float guidance_scale, float a_t, float a_prev, float sigma,
                         float sqrt_one_minus_at, hipStream_t stream);

/* Same update with the step scalars in device memory: coef[6] = {guidance scale, 1/sqrt(a_t), sqrt(a_prev),
 * sqrt(1 - a_prev - sigma^2), sigma, sqrt(1 - a_t)}.  Lets one captured HIP graph of a DDIM step be replayed for
 * every step (the host only refreshes coef / the timestep tensor between replays). */
int vd_cfg_ddim_step_dev_f16(const void* x, const void* eps, const void* noise, void* x_prev, void* pred_x0, int64_t n,
                             int guided, const float* coef, hipStream_t stream);

/* Classifier-free-guidance combine + DPM-Solver++(2M) multistep update in one pass (fp32 math), step scalars in device
 * memory: coef[8] = {guidance scale, 1/sqrt(a_t), sqrt(1 - a_t), sigma_next/sigma_t, c_d, w_cur, w_prev, 0}.
 *   e = e_u + s (e_c - e_u); x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); D = w_cur x0 + w_prev x0_hist;
 *   x_next = (sigma_next/sigma_t) x + c_d D; then x0_hist = x0 (fp32[n]) and pred_x0 = x0 (fp16, may be NULL).
 * x0_hist is not read when w_prev == 0 (first-order steps).  x_next may alias x.  Lets one captured HIP graph of a
 * solver step be replayed for every step, like vd_cfg_ddim_step_dev_f16.
 * Roundings (part of the contract; one kernel serves this entry point and vd_cfg_dpmpp_sde_step_dev_f16).  e and x0 are
 * fma(s, e_c - e_u, e_u) and fma(-sqrt(1-a_t), e, x) / sqrt(a_t) everywhere; D and x_next depend on how an element moves:
 *   16-byte loop (every pointer 16-byte aligned; elements [0, n/8*8)): every product-sum is one fma,
 *       D = fma(w_prev, x0_hist, w_cur x0), x_next = fma(sigma_next/sigma_t, x, c_d D)
 *   scalar loop (the other elements) without noise: the two products of D and of x_next are rounded before they are added
 *   elements that get noise (the SDE entry point with coef[7] != 0), on either loop: fused as in the 16-byte loop, then
 *       x_next = fma(coef[7], z, x_next)
 * Each of these is an fp32 operation; x_next and pred_x0 are the fp32 results rounded to fp16 (never a sum rounded
 * straight to fp16). */
int vd_cfg_dpmpp_step_dev_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0, int64_t n,
                              int guided, const float* coef, hipStream_t stream);

/* Seeded normal noise from a counter-based generator: Philox4x32-10 (Salmon et al., SC'11; Random123), multipliers
 * 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85.  The noise of an element is a pure function of its
 * sample's seed, so it does not depend on the batch, the batch position, the graph or the rank a sample runs in.
 *   key     = the sample's 64-bit seed, 0 <= seed < 2^63: (low word, high word)
 *   counter = (j, 0, draw, stream): j indexes the block of elements 4j .. 4j+3 of the sample's flattened [C, *spatial]
 *             latent; draw is the step number in sampling order (0 for the first step run; 0 for non-step streams);
 *             stream is 0 for x_T, 1 for forward-process (q_sample) noise, 2 for step noise
 *   normals : output words (r0, r1) give elements 4j, 4j+1 and (r2, r3) give 4j+2, 4j+3 by Box-Muller in fp32 with
 *             u1 = ((r_even >> 9) + 0.5) 2^-23, u2 = ((r_odd >> 9) + 0.5) 2^-23 (both exact, in (0, 1)):
 *             z_even = sqrt(-2 ln u1) cos(2 pi u2), z_odd = sqrt(-2 ln u1) sin(2 pi u2), accurate logf / sincospif
 * out[B, per_sample] = scale * z (fp32 when out_is_f32 != 0, else that fp32 value rounded once to fp16); any per_sample
 * (a last partial block of four is handled).  Returns < 0 for null pointers, B or per_sample <= 0, negative draw or
 * stream_tag, or per_sample beyond 2^34 (the block counter is one word). */
int vd_philox_normal(const int64_t* seeds, void* out, int out_is_f32, int B, int64_t per_sample, int draw,
                     int stream_tag, float scale, hipStream_t stream);

/* vd_cfg_dpmpp_step_dev_f16 plus seeded noise: x_next = (that update) + coef[7] * z, the SDE variant of DPM-Solver++(2M)
 * with rows of dpm_solver.dpmpp_sde_coef_table.  z is generated in place by the generator above for sample
 * b = i / per_sample (seeds: int64[n / per_sample] in device memory) and element i % per_sample, with
 * rng = int32[2] {draw, stream} in device memory, refreshed between graph replays like coef.  coef[7] == 0 generates
 * nothing and gives the bits of vd_cfg_dpmpp_step_dev_f16 (the same kernel; roundings: the rule stated there).  With noise,
 * 16-byte accesses when every pointer is 16-byte aligned and per_sample % 8 == 0, else the scalar loop, with the same
 * noise and the same bits per (sample, element).  x_next may alias x.
 * Returns < 0 for null pointers (pred_x0 may be NULL), n or per_sample <= 0, or n not a multiple of per_sample. */
int vd_cfg_dpmpp_sde_step_dev_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0, int64_t n,
                                  int64_t per_sample, int guided, const float* coef, const int64_t* seeds,
                                  const int* rng, hipStream_t stream);

/* Guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4; diffusers'
 * guidance_rescale): the guided prediction is scaled back towards the standard deviation of the conditional one.  For sample
 * b with m = per_sample elements (its flattened [C, *spatial] latent), guidance scale s = coef[0] and weight phi in [0, 1]:
 *   eg_i = fmaf(s, ec_i - eu_i, eu_i)            fp32, the same value the updates compute
 *   V(v) = sum v_i^2 - (sum v_i)^2 / m           sums over the sample, accumulated in fp64 (an fp32 value squared is exact there)
 *   r    = sqrt(max(V(ec), 0) / V(eg))           fp64; r = 1 if V(eg) <= 0, m == 1 or r is not finite
 *   k_b  = (float)(phi * r + (1 - phi))          fp64 (the product rounded, then the sum), rounded once to fp32
 *   e'_i = k_b * eg_i                            fp32; e' takes the place of e everywhere in the update
 * The ratio of standard deviations does not depend on the estimator's ddof, so this is diffusers' rule; phi = 0 gives k_b = 1
 * exactly.  eps = [e_uncond ; e_cond] (2n fp16), coef and phi in device memory (coef: the row the update reads, only coef[0] is
 * read; phi: one float), kfac: fp32 [n / per_sample].  One block of 256 lanes reduces a sample, whatever the batch, in an order
 * that depends on per_sample alone (per-lane fp64 sums, a fixed butterfly over the wave, the waves added in order; no atomics),
 * so k_b is a pure function of the sample's e_u and e_c, s and phi: the same bits for any batch size, batch position, alignment
 * (16-byte loads when both halves of the sample are 16-byte aligned, else 2-byte loads of the same elements), graph or rank.
 * Any per_sample.  Does not allocate or synchronise (capturable).  Returns < 0 for null pointers, n or per_sample <= 0, or n
 * not a multiple of per_sample. */
int vd_cfg_rescale_factor_f16(const void* eps, int64_t n, int64_t per_sample, const float* coef, const float* phi,
                              float* kfac, hipStream_t stream);

/* The fused updates with the guidance rescale: the sibling entry point (same name without _rs) with e' = kfac[i / per_sample] * e
 * in the place of e -- one fp32 multiply right after e; everything after it follows the sibling's rounding rule, and with every
 * kfac[b] == 1.0f the outputs are the sibling's bits.  The same kernels, instantiated with the multiply.  kfac: fp32
 * [n / per_sample] in device memory (vd_cfg_rescale_factor_f16).  Return < 0 for the sibling's errors, a null kfac,
 * per_sample <= 0, n not a multiple of per_sample, and guided == 0 (there is nothing to rescale). */
int vd_cfg_ddim_step_rs_f16(const void* x, const void* eps, const void* noise, void* x_prev, void* pred_x0, int64_t n,
                            int64_t per_sample, int guided, float guidance_scale, float a_t, float a_prev, float sigma,
                            float sqrt_one_minus_at, const float* kfac, hipStream_t stream);
int vd_cfg_ddim_step_dev_rs_f16(const void* x, const void* eps, const void* noise, void* x_prev, void* pred_x0, int64_t n,
                                int64_t per_sample, int guided, const float* coef, const float* kfac, hipStream_t stream);
int vd_cfg_dpmpp_step_dev_rs_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0, int64_t n,
                                 int64_t per_sample, int guided, const float* coef, const float* kfac, hipStream_t stream);
int vd_cfg_dpmpp_sde_step_dev_rs_f16(const void* x, const void* eps, float* x0_hist, void* x_next, void* pred_x0, int64_t n,
                                     int64_t per_sample, int guided, const float* coef, const int64_t* seeds, const int* rng,
                                     const float* kfac, hipStream_t stream);

/* Classifier-free-guidance combine + UniPC corrector + predictor (Zhao et al. 2023, variant bh2, data prediction; what
 * diffusers' UniPCMultistepScheduler(solver_type="bh2", predict_x0=True) computes) of one sampling step in one pass, step
 * scalars in device memory: one captured HIP graph of a step serves every step.  Both updates are linear in their operands
 * and the host collapses them (float64, unipc.unipc_coef_table) into one fp32 row
 *   coef[16] = {guidance scale s, 1/sqrt(a_t), sqrt(1 - a_t), corrector on (0 / 1), c_x, c_1, c_2, c_3, c_t,
 *               p_x, p_t, p_1, p_2, hist, 0, 0}
 * hist = min(steps of this call already run, 3): how many of the data predictions m_1 (the most recent), m_2, m_3 exist.
 *   e      = fma(s, e_c - e_u, e_u), or e_u when guided == 0          (the _rs twin: e' = kfac[i / per_sample] * e)
 *   m_t    = fma(-sqrt(1 - a_t), e, x) * (1/sqrt(a_t))
 *   x_c    = fma(c_x, x_last, fma(c_3, m_3, fma(c_2, m_2, fma(c_1, m_1, c_t * m_t))))   corrector on; else x_c = x (widened)
 *   x_next = fma(p_x, x_c, fma(p_2, m_2, fma(p_1, m_1, p_t * m_t)))
 *   then x_last = x_c, (m_1, m_2, m_3) = (m_t, m_1, m_2), pred_x0 = m_t (fp16, may be NULL)
 * Roundings (part of the contract): every line above is fp32 and every product-sum is ONE fma, nested in the order written
 * (innermost first); a term whose coefficient is 0 is left out of the chain, not multiplied; x_next and pred_x0 are the fp32
 * results rounded to fp16 as a rounding of their own (never a sum rounded straight to fp16).  The 16-byte loop (every pointer
 * 16-byte aligned; elements [0, n/8*8), 8 per lane) and the scalar loop (every other element) follow the same rule: an
 * element has the same bits on either.
 * What is read: x_last only with the corrector on; m_3 only when c_3 != 0; m_1 when hist >= 1 and m_2 when hist >= 2 (every
 * non-zero coefficient implies that, and the shift of the history needs them).  A row with hist == 0 -- the first step of a
 * call -- reads no state, so the state may be uninitialised there, and it writes m_1 = m_2 = m_3 = m_t: after any step all
 * four state buffers hold defined values.
 * x, x_next, pred_x0: fp16 [n]; eps: fp16 [e_uncond ; e_cond] (2n) when guided != 0, else [n]; x_last, m1, m2, m3: fp32 [n],
 * four distinct buffers.  x_next may alias x.  Does not allocate or synchronise (capturable).  Returns < 0 (vd_last_error)
 * for null pointers (pred_x0 may be NULL), n <= 0, or state buffers that coincide; the _rs twin also for the errors of the
 * other _rs entry points (a null kfac, per_sample <= 0, n not a multiple of per_sample, guided == 0).  With every
 * kfac[b] == 1.0f the twin gives the plain entry point's bits; a lane of its 16-byte loop that straddles samples looks the
 * factor up per element. */
int vd_cfg_unipc_step_dev_f16(const void* x, const void* eps, float* x_last, float* m1, float* m2, float* m3, void* x_next,
                              void* pred_x0, int64_t n, int guided, const float* coef, hipStream_t stream);
int vd_cfg_unipc_step_dev_rs_f16(const void* x, const void* eps, float* x_last, float* m1, float* m2, float* m3, void* x_next,
                                 void* pred_x0, int64_t n, int64_t per_sample, int guided, const float* coef,
                                 const float* kfac, hipStream_t stream);

/* Masked blend of blended latent diffusion (inpainting; not in the reference), after a sampler step lands on a_prev:
 *   out = m x + (1 - m) (ca x0 + cn noise),  coef[2] = {ca, cn} = {sqrt(a_prev), sqrt(1 - a_prev)} (or {1, 0} on the
 *   last step) in device memory, fp32 math, one fp16 rounding.
 * x, x0, noise, out: fp16 [B, C, HW]; mask: fp16 [Bm, HW], Bm = 1 or B, broadcast over channels (1 = regenerate,
 * 0 = keep).  out may alias x.  Returns < 0 (vd_last_error) for null pointers, B, C or HW <= 0, or another Bm. */
int vd_masked_blend_f16(const void* x, const void* x0, const void* noise, const void* mask, void* out, int B, int C,
                        int64_t HW, int Bm, const float* coef, hipStream_t stream);

/* Windowed (MultiDiffusion, Bar-Tal et al. 2023) sampling: every step runs the UNet on overlapping windows of the canvas latent
 * and fuses the windows' predictions (not in the reference; tables: lib/model_zoo/windows.py).
 *
 * vd_window_gather_f16 cuts the windows: x fp16 [B, C, H, W] -> win fp16 [B, slots, C, h, w],
 *   win[b, k, c, i, j] = x[b, c, oy_k + i, ox_k + j],  the column (ox_k + j) % W when wrap != 0,
 * with offs = int32 [slots][2] rows {oy_k, ox_k} in DEVICE memory.  The copy is bit-exact: 16-byte accesses where a row segment
 * of 8 elements is whole, does not cross the wrap seam and is 16-byte aligned on both sides, else 2-byte accesses of the same
 * elements.
 *
 * vd_window_merge_f16 fuses them: eps_win fp16 [RB, slots, C, h, w] (the UNet's output for one chunk of windows; RB = the
 * [uncond ; cond] rows), acc fp32 [RB, C, H, W], eps fp16 [RB, C, H, W], wgt fp32 [h, w], inv_den fp32 [H, W].  One thread
 * owns one canvas element (rb, c, Y, X) -- a gather: no atomics, a fixed order:
 *   a = first ? 0 : acc[...]
 *   for k = 0 .. valid-1 ascending, if window k covers the pixel at (i, j) = (Y - oy_k, X - ox_k [mod W when wrap]):
 *       a = fmaf(wgt[i, j], (float)eps_win[rb, k, c, i, j], a)
 *   acc[...] = a  unless first && last
 *   if last: eps[...] = fp16(a * inv_den[Y, X])     one fp32 multiply, then one rounding to fp16
 * Slots >= valid are never read (the padded slots of a call's last chunk).  acc may be NULL only when first && last; eps is
 * written only when last (and may be NULL otherwise).  The chain runs in ascending window order and acc is exact fp32 between
 * launches, so the result has the same bits however the windows are split into launches.
 *
 * Both neither allocate nor synchronise (capturable).  They return < 0 (vd_last_error) for null pointers, non-positive sizes,
 * h > H or w > W, and the merge for valid outside [1, slots].  The offsets live in device memory and are NOT validated by
 * these entry points: callers pass tables built by windows.window_offsets (0 <= oy <= H - h; 0 <= ox <= W - w, or 0 <= ox < W
 * when wrapping).  Neither kernel leaves its buffers for another table -- the gather brings an offset outside that range back
 * into it, the merge tests coverage from the pixel's side -- but what they then compute is unspecified. */
int vd_window_gather_f16(const void* x, void* win, const int32_t* offs, int B, int C, int H, int W, int h, int w, int slots,
                         int wrap, hipStream_t stream);
int vd_window_merge_f16(const void* eps_win, float* acc, void* eps, const float* wgt, const float* inv_den,
                        const int32_t* offs, int RB, int C, int H, int W, int h, int w, int slots, int valid, int wrap,
                        int first, int last, hipStream_t stream);

/* Regional prompts on the windowed path (the region-based generation of MultiDiffusion, section 4.3): every region r has a mask
 * on the canvas latent grid and contexts of its own, every (region, chunk of windows) is one UNet forward, and the predictions
 * are fused weighted per pixel by window weight x region mask.  vd_window_merge_masked_f16 is one launch of that fusion: the
 * arguments, layouts and thread ownership of vd_window_merge_f16 plus mask, fp32 [H, W] in device memory, the region of this
 * launch (shared by all RB rows):
 *   a  = first ? 0 : acc[...]
 *   mv = mask[Y, X]
 *   if mv != 0:                                 a zero mask adds nothing: a NaN predicted outside a region never reaches a
 *     for k = 0 .. valid-1 ascending, if window k covers the pixel at (i, j):
 *         wm = wgt[i, j] * mv                   one fp32 multiply, rounded once
 *         a  = fmaf(wm, (float)eps_win[rb, k, c, i, j], a)
 *   acc[...] = a  unless first && last
 *   if last: eps[...] = fp16(a * inv_den[Y, X])     one fp32 multiply, then one rounding to fp16
 * first / last span all (region, chunk) launches of a step: the sum runs region-major, inside a region in ascending window
 * order, and acc is exact fp32 between launches, so the split into launches does not decide a bit.  inv_den is the reciprocal
 * of the sum over regions and covering windows of the fp32 products wm (windows.region_inv_den); with one region whose mask is
 * all ones the launch gives vd_window_merge_f16's bits.  Mask values are expected finite in [0, 1] (windows.region_masks_arg)
 * and are not validated here.  Neither allocates nor synchronises (capturable).  Returns < 0 (vd_last_error) for what
 * vd_window_merge_f16 refuses and for a null mask. */
int vd_window_merge_masked_f16(const void* eps_win, float* acc, void* eps, const float* wgt, const float* mask,
                               const float* inv_den, const int32_t* offs, int RB, int C, int H, int W, int h, int w, int slots,
                               int valid, int wrap, int first, int last, hipStream_t stream);

/* Tiled VAE decode / encode (not in the reference; tables: lib/model_zoo/vae_tiles.py on lib/model_zoo/windows.py): the KL-f8
 * autoencoder runs on overlapping tiles of a canvas, every tile a sample of its own, and vd_tile_blend_f16 (additive to ABI 8)
 * fuses the tiles' outputs into the canvas -- weighted sum, normalisation, affine, clamp and layout change in one pass.
 *   tiles   fp16 [RB, slots, ph, pw, C]  channels-last, as the decoder (C = 3) / quant_conv (C = 2 zc) leave them; batch order
 *                                        (sample, slot); one chunk of the call's tiles
 *   acc     fp32 [RB, C, PH, PW]         the running sum, exact between launches; may be NULL only when first && last
 *   out     fp16 [RB, C, PH, PW] (out_nhwc == 0) or [RB, PH, PW, C] (out_nhwc != 0); written only when last (else may be NULL)
 *   wgt     fp32 [ph, pw], inv_den fp32 [PH, PW], offs int32 [slots][2] rows {oy_k, ox_k} in the units of the canvas being
 *           written, all in DEVICE memory
 * One work item owns one canvas pixel (rb, Y, X) with all its C channels -- a gather: no atomics, a fixed order.  Per element:
 *   a = first ? 0 : acc[...]
 *   for k = 0 .. valid-1 ascending, if tile k covers the pixel at (i, j) = (Y - oy_k, X - ox_k [+ PW when wrap and that
 *   is negative: the column mod PW for 0 <= ox_k < PW]):
 *       a = fmaf(wgt[i, j], (float)tiles[rb, k, i, j, c], a)
 *   acc[...] = a  unless first && last
 *   if last:
 *       v = a * inv_den[Y, X]                       one fp32 multiply, rounded to fp32
 *       v = fmaf(v, scale, shift)
 *       if clamp01: v = fminf(fmaxf(v, 0), 1)       (a NaN comes out as 0, as fmaxf has it)
 *       out[...] = fp16(v)                          one rounding to fp16
 * The decode uses (scale, shift, clamp01) = (0.5, 0.5, 1) and NCHW out (the image in [0, 1]); the encode (1, 0, 0) and
 * channels-last out (the moments).  Slots >= valid are never read.  The chain runs in ascending tile order and acc is exact fp32
 * between launches, so the result has the same bits however the tiles are split into launches.  The C fp16 of a tile pixel are
 * read (and a channels-last pixel written) with accesses of up to 16 bytes when C is even and the buffers start on such a
 * boundary, else one by one: the same elements, the same bits.
 * Neither allocates nor synchronises.  Returns < 0 (vd_last_error) for null pointers (acc and out as above), non-positive sizes,
 * ph > PH or pw > PW, valid outside [1, slots] and C outside [1, 16].  The offsets are NOT validated (windows.window_offsets
 * builds them); coverage is tested from the pixel's side, so no table makes the kernel leave its buffers. */
int vd_tile_blend_f16(const void* tiles, float* acc, void* out, const float* wgt, const float* inv_den, const int32_t* offs,
                      int RB, int C, int PH, int PW, int ph, int pw, int slots, int valid, int wrap, int first, int last,
                      int out_nhwc, float scale, float shift, int clamp01, hipStream_t stream);

/* FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024; not in the reference) at one skip concatenation of the
 * UNet's decoder.  The setting is four real numbers (b1, b2, s1, s2).  With W1 the width of the widest h that enters any
 * output-stage block of the 2-D data net and W2 = W1 / 2 (integer), a skip load whose entering h [B, H, W, C0] has C0 == W1 is
 * stage 1 and uses (b, s) = (b1, s1), C0 == W2 is stage 2 and uses (b2, s2), any other width is untouched (lib/model_zoo/vd.py:
 * freeu_stages).  vd_freeu_f16 is one stage's work on h and the popped skip [B, H, W, C1], both channels-last fp16, in ONE launch:
 *
 *   backbone  h_out[..., c] = fp16(fp32(h[..., c]) * b)  for c < C0 / 2 (the product rounded to fp32, then once to fp16);
 *             the other channels are copied bit for bit.
 *   skip      per sample and channel, on the H x W plane x (H, W >= 2):  y = Re(ifft2(mask * fft2(x))),  mask = s on the
 *             frequencies {-1, 0} x {-1, 0} and 1 elsewhere (diffusers' fourier_filter with threshold 1).  Written out, with
 *             tp = 2 pi p / H and fq = 2 pi q / W:
 *                 S0  = sum x
 *                 Ay  = sum x cos tp          By  = sum x sin tp
 *                 Ax  = sum x cos fq          Bx  = sum x sin fq
 *                 Axy = sum x cos(tp + fq)    Bxy = sum x sin(tp + fq)
 *                 y[p, q] = x[p, q] + g (S0 + Ay cos tp + By sin tp + Ax cos fq + Bx sin fq + Axy cos(tp + fq) + Bxy sin(tp + fq))
 *                 g = (s - 1) / (H W)      formed in double from the fp32 s, rounded once to fp32
 *
 * Tables (DEVICE memory, fp32): cy, sy [H] = cos / sin tp;  cx, sx [W] = cos / sin fq;  cxy, sxy [H W] = cos / sin(tp + fq) at
 * index p W + q.  There is no trig on the device: the host builds them in float64 and rounds once to fp32, with the angle
 * reduced on integers first -- k / n of a turn with k = p mod H, q mod W, (p W + q H) mod (H W) -- and the multiples of a quarter
 * turn set to exactly 0 or +-1 (vd_hip/ops.py: freeu_tables).
 *
 * Arithmetic: the seven sums are fp32 (S0 by additions, the others by one fma per pixel), in an order that depends on (H, W)
 * alone: thread t of the 256 of a block takes pixels t, t + 256, .. ascending, a wave adds its lanes by the xor butterfly
 * 32, 16, .. 1, the four waves are added in ascending order.  A block owns 8 channels of one sample; nothing is atomic, so a
 * sample's output has the same bits for any batch size, batch position and run.  The bracket is S0 followed by the six fmas in
 * the order written, y = fma(g, bracket, x) in fp32, then one rounding to fp16.
 *
 * h_out and skip_out are separate tensors: nothing is filtered in place (the outputs must not alias the inputs).  Neither
 * allocates nor synchronises (capturable).  Returns < 0 (vd_last_error) for null pointers, non-positive sizes, H or W < 2, C0 or
 * C1 not a multiple of 8, pointers that are not 16-byte aligned, aliased outputs, or b or s not finite. */
int vd_freeu_f16(const void* h, const void* skip, void* h_out, void* skip_out, const float* cy, const float* sy, const float* cx,
                 const float* sx, const float* cxy, const float* sxy, int B, int H, int W, int C0, int C1, float b, float s,
                 hipStream_t stream);

/* Perturbed-attention guidance (Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance", 2024;
 * diffusers' pag_scale / pag_applied_layers; not in the reference).  A step predicts a further replica e_p in which chosen
 * self-attention layers replace their attention map softmax(q k^T) by the identity, and combines
 *     e = e_u + s (e_c - e_u) + s_pag (e_c - e_p)        (unguided, s == 1:  e = e_c + s_pag (e_c - e_p)).
 * Two entry points (additive to ABI 8).
 *
 * vd_attention_ident_f16: the arguments of vd_attention_f16 plus ident_from.  Samples b < ident_from: exactly the call
 * vd_attention_f16(q, k, v, out, ident_from, ...) -- the same kernel instances, so their bits are those of a call on these
 * samples alone.  Samples b >= ident_from: out[b, n, c] = v[b, n, c] for every row n < Nq and column c < H * D, bit for bit
 * (softmax replaced by I: every head keeps its own columns), through ldv / ldo and the sample strides sv / so; q and k of these
 * samples are not read.  The copy is ONE launch of 16-byte accesses; ident_from == B launches no copy, ident_from == 0 no
 * softmax kernel.  q / k / v may be column slices of one fused [B, N, 3 C] projection (ld = 3 C) and contiguous batch-slice
 * views.  Returns < 0 (vd_last_error, the text starts with this entry's name) for null pointers, an empty problem, Nq != Nk,
 * causal != 0, ident_from outside [0, B], H * D, a leading dimension or a sample stride of v / out that is no multiple of 8,
 * ldv or ldo below H * D, v or out not 16-byte aligned, and whatever vd_attention_f16 refuses for the leading samples (its
 * text follows the name).  Neither allocates nor synchronises (capturable). */
int vd_attention_ident_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                           int ldq, int ldk, int ldv, int ldo, int64_t sq, int64_t sk, int64_t sv, int64_t so,
                           float scale, int causal, int ident_from, hipStream_t stream);

/* vd_pag_fold_f16: eps is fp16 [reps][n], reps = 3 ([e_uncond ; e_cond ; e_perturbed]) or 2 ([e_cond ; e_perturbed]); w is a
 * fp32[1] in DEVICE memory (one captured launch serves every weight).  With a = replica 0, c = replica reps - 2 (for reps == 2
 * that is a itself) and p = replica reps - 1, replica 0 is rewritten in place, element by element:
 *     d = fp32(c) - fp32(p)          one fp32 subtraction (the conversions are exact)
 *     r = fmaf(w, d, fp32(a))        one fp32 fused multiply-add
 *     a = fp16(r)                    a rounding of its own, to nearest even (never the exact fma result rounded to fp16)
 * The other replicas are not written.  w == 0 writes nothing: replica 0 keeps its bits.
 * reps == 3: the host loads w = -s_pag / (s - 1), formed in double and rounded once to fp32; then a' + s (c - a') is the
 * formula above (up to that rounding), so every fused update vd_cfg_*_step_* and vd_cfg_rescale_factor_f16 run on the leading
 * [2][n] unchanged -- the rescale targets the standard deviation of the unperturbed e_c, as diffusers'
 * rescale_noise_cfg(noise_pred, noise_pred_text).  reps == 2: w = s_pag, and the unguided update reads the leading [n].
 * Any n > 0: replicas that are all 16-byte aligned (eps aligned, n a multiple of 8) take 16-byte accesses, any other call one
 * element per lane, with the same arithmetic.  An element's result depends on its three operands and w alone.  Returns < 0
 * for a null pointer, n <= 0, reps outside {2, 3} or a misaligned eps / w.  Neither allocates nor synchronises (capturable). */
int vd_pag_fold_f16(void* eps, int64_t n, int reps, const float* w, hipStream_t stream);

/* Smoothed energy guidance (Hong, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of Attention",
 * NeurIPS 2024; ComfyUI's SEG node, diffusers' SmoothedEnergyGuidance; not in the reference).  The perturbed replica of
 * perturbed-attention guidance with a milder perturbation: chosen self-attention layers keep their softmax and Gaussian-blur the
 * replica's QUERIES over the token grid, per channel; k and v are untouched.  The prediction is combined by vd_pag_fold_f16 as
 * above, e = e_u + s (e_c - e_u) + s_seg (e_c - e_p).  One entry point (additive to ABI 8).
 *
 * vd_attention_qblur_f16: the arguments of vd_attention_f16 plus blur_from, the token grid gh x gw (gh * gw == Nq == Nk), the taps
 * (DEVICE fp32 [2 R + 1], w[d] at index d + R; one captured call serves every sigma of the same R), R, and the caller's workspace qb,
 * fp16 [(B - blur_from)][Nq][H * D] contiguous.  Samples b < blur_from: exactly the call vd_attention_f16(q, k, v, out, blur_from,
 * ...) -- the same kernel instances, so their bits are those of a call on these samples alone.  Samples b >= blur_from: ONE launch
 * writes their blurred queries qb from the strided q (which may be a column slice of a fused [B, N, 3 C] projection, ld = 3 C), then
 * ONE call vd_attention_f16(qb, k + blur_from * sk, v + blur_from * sv, out + blur_from * so, B - blur_from, ..., ldq = H * D,
 * sq = Nq * H * D, ...) -- so their output is, bit for bit, that call on qb.  blur_from == B launches no blur and does not touch qb
 * (which may then be NULL); blur_from == 0 runs one softmax call.  With token n = y * gw + x and channel c, per element:
 * R >= 0 (the taps are whatever the caller loads; lib/model_zoo/vd.py's seg_taps forms the normalised Gaussian in double and rounds
 * once), each line ONE fp32 operation:
 *     h[y'][x] = 0;  for dx = -R .. R ascending:  h = fmaf(w[dx], fp32(q[refl(x + dx, gw) of row y']), h)      the horizontal pass
 *     a        = 0;  for dy = -R .. R ascending:  a = fmaf(w[dy], h[refl(y + dy, gh)][x], a)                    the vertical pass
 *     qb[n][c] = fp16(a)         a rounding of its own, to nearest even; h is kept in fp32 and never rounded to fp16
 * refl(i, n) is the reflection that does not repeat the edge (torch's 'reflect' padding), folded as often as needed, period
 * 2 (n - 1): i mod 2 (n - 1) = j, then j if j < n else 2 (n - 1) - j; 0 for n == 1.  So any R is defined, R >= n too, and for R < n the
 * result is that of F.pad(mode="reflect") followed by a depthwise conv2d with the outer product of the taps.
 * R == -1 (sigma = infinity, the upstream default): every query of a sample becomes its mean query.  Per (sample, channel): thread t
 * of 256 adds the tokens t, t + 256, ... ascending in fp32 from 0, the 256 partial sums are added in a fixed binary tree (t takes
 * t + 128, then t + 64, ... t + 1), one IEEE fp32 division by (float)Nq, one rounding to fp16, to nearest even, broadcast to all Nq
 * rows.  The order depends on Nq alone: no atomics, the same bits run to run, for any batch, grid of the launch or graph.
 * An element of qb is a pure function of its sample's q, the taps and the grid: whether the horizontal pass is staged in LDS (a band
 * of grid rows per block) or recomputed per vertical tap in registers (a hull that does not fit) the operations above are the same.
 * Returns < 0 (vd_last_error, the text starts with this entry's name) for null pointers, an empty problem, Nq != Nk, causal != 0,
 * blur_from outside [0, B], gh * gw != Nq, R < -1, R >= 0 without taps or with taps not 4-byte aligned, H * D, ldq or sq no multiple
 * of 8, ldq below H * D, q or qb not 16-byte aligned, and whatever vd_attention_f16 refuses (its text follows the name).  Neither
 * allocates nor synchronises (capturable). */
int vd_attention_qblur_f16(const void* q, const void* k, const void* v, void* out, int B, int H, int Nq, int Nk, int D,
                           int ldq, int ldk, int ldv, int ldo, int64_t sq, int64_t sk, int64_t sv, int64_t so,
                           float scale, int causal, int blur_from, int gh, int gw, const float* taps, int R, void* qb,
                           hipStream_t stream);

/* Self-attention guidance (Hong et al., "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance", ICCV 2023;
 * diffusers' StableDiffusionSAGPipeline(sag_scale); not in the reference).  A step reads the self-attention map of the middle
 * context block, blurs the pixels of its data prediction that the map attends to, re-noises the result, predicts a second time
 * from that degraded latent (e_d) and combines, with e0 the first forward's replica 0 (e_u when guided, else e_c),
 *     e = e_u + s (e_c - e_u) + s_sag (e0 - e_d)        (unguided, s == 1:  e = e_c + s_sag (e_c - e_d)).
 * Three entry points (additive to ABI 8); none allocates or synchronises (capturable).  Each returns < 0 (vd_last_error, the text
 * starts with the entry's name) for null or misaligned pointers, an empty problem and what is listed with it.
 *
 * vd_sag_mass_f16 (the attention map and `attn_map.mean(1).sum(1)` of diffusers' sag_masking): q and k are fp16 with the leading
 * dimensions ldq / ldk and the sample strides sq / sk of vd_attention_f16 (column slices of one fused [B, N, 3 C] projection and
 * contiguous batch-slice views included; 16-byte aligned, strides multiples of 8); head h reads the columns [h D, (h + 1) D).
 * With s(i, j) = scale * sum_d q[i, d] k[j, d] (the products of fp16 values summed in fp32 in ascending d, one fp32 multiplication
 * by scale) and P[i, j] = exp(s(i, j) - max_j s) / sum_j exp(s(i, j) - max_j s), all fp32 -- P is never rounded to fp16 --
 *     mass[b * N + j] = (1 / H) * sum_h sum_i P[b, h, i, j]          fp32 [B][N]: the sum over QUERIES, per KEY, the mean over heads.
 * Two passes per head (row maximum and row sum of every query; then the scores again, summed per key), every sum in a fixed
 * order: no float atomics, the same input gives the same bits on every run.  D as vd_attention_f16: 40, 64, 80, 160, or one head
 * of 128 / 256 / 512 (any other: < 0).  N <= 1024 (more: < 0).
 *
 * vd_sag_degrade_f16 (the mask and interpolate of sag_masking, gaussian_blur_2d, pred_x0 and add_noise for an epsilon model, in
 * ONE launch): x, eps0, xd are fp16 [B, C, H, W]; mass fp32 [T][B][Hm Wm] (one map per context type); ratio fp32 [T]; taps fp32
 * [9] (the normalised Gaussian, g[k] ~ exp(-((k - 4) / sigma)^2 / 2)); coef fp32 [3] = {sa, s1, isa} = {sqrt(a_t), sqrt(1 - a_t),
 * 1 / sqrt(a_t)} -- all DEVICE operands, so one captured launch serves every step, scale and sigma.  Per sample b, all in fp32:
 *     m[j]       = fmaf(ratio[t], mass[t][b][j], m[j])  for t ascending, from 0
 *     M(y, x)    = m[((y * Hm) / H) * Wm + (x * Wm) / W] > 1.0            strict; nearest neighbour in integers; every channel alike
 *     p0(y, x)   = fmaf(-s1, eps0, x) * isa                               one fma, one multiplication
 *     row(y, x)  = sum_j g[j] p0(y, refl(x + j - 4, W))                   nine fmas from 0, j ascending
 *     blur(y, x) = sum_i g[i] row(refl(y + i - 4, H), x)                  nine fmas from 0, i ascending
 *     d          = M ? blur : p0
 *     xd         = fp16(fmaf(sa, d, s1 * eps0))                           a rounding of its own, to nearest even
 * refl is torch's "reflect" padding, without edge repeat (-1 -> 1, n -> n - 2): H, W >= 5 (less: < 0).  A 32 x 32 tile of a plane
 * with its 4-pixel halo of p0 is staged in LDS; a tile without a masked pixel skips the blur (the same bits: d = p0).
 *
 * vd_sag_fold_f16: eps is fp16, its leading [n] replica 0 of the step's prediction; e_d fp16 [n]; w a fp32[1] in DEVICE memory.
 *     a = fp16(fmaf(w, fp32(a) - fp32(e_d), fp32(a)))        one fp32 subtraction, one fma, a rounding of its own to fp16
 * in place on the leading [n]; nothing else is written, and w == 0 writes nothing (replica 0 keeps its bits).  Guided: the host
 * loads w = -s_sag / (s - 1), formed in double and rounded once to fp32, so the update's a' + s (e_c - a') is the formula above and
 * every fused update vd_cfg_*_step_* and vd_cfg_rescale_factor_f16 run unchanged; unguided: w = s_sag.  16-byte accesses when eps
 * and e_d are 16-byte aligned and n is a multiple of 8, else one element per lane with the same arithmetic.  n <= 0: < 0. */
int vd_sag_mass_f16(const void* q, const void* k, float* mass, int B, int H, int N, int D, int ldq, int ldk, int64_t sq,
                    int64_t sk, float scale, hipStream_t stream);
int vd_sag_degrade_f16(const void* x, const void* eps0, const float* mass, const float* ratio, int T, const float* taps,
                       const float* coef, void* xd, int B, int C, int H, int W, int Hm, int Wm, hipStream_t stream);
int vd_sag_fold_f16(void* eps, const void* e_d, int64_t n, const float* w, hipStream_t stream);

/* Adaptive projected guidance (Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance Scales in
 * Diffusion Models", 2024, Algorithm 1; diffusers' AdaptiveProjectedGuidance(eta, norm threshold, momentum); not in the reference).
 * The guidance direction, taken between the DATA predictions, gets a momentum across steps, has its norm clipped per sample, and
 * loses the share (1 - eta) of its part parallel to the conditional data prediction.  One entry point (additive to ABI 8), one
 * launch per step, in front of the unchanged update.
 *
 * vd_apg_fold_f16: x is fp16 [n] (the latent); eps is fp16 with the leading [2][n] = [e_u ; e_c], of which only the leading [n] is
 * written; v is fp32 [n], the running direction (read only when coef[3] != 0, always written); coef is fp32 [8] in DEVICE memory,
 * {s1, isa, ig, beta_eff, r, 1 - eta, 0, 0} with s1 = sqrt(1 - a_t), isa = 1 / sqrt(a_t), ig = 1 / (s1 isa), each formed in double
 * and rounded once by the host (one captured launch serves every step and setting); fac is fp32 [n / per_sample][4].
 * For sample b with m = per_sample elements (its flattened [C, *spatial] latent), per element, each line ONE fp32 operation:
 *     D   = fmaf(-s1, e_c, x) * isa               the conditional data prediction: one fma, one multiplication
 *     dD  = (-g32) * (e_c - e_u)                  g32 = s1 * isa rounded once; one subtraction, one multiplication (= D_c - D_u)
 *     v   = fmaf(beta_eff, v_prev, dD)            or v = dD when beta_eff == 0 (v_prev is then not read: it may hold anything)
 * over the sample, in fp64 (the product of two fp32 values is exact there), then rounded ONCE to fp32 where they are used:
 *     Svv = sum v^2,  Svd = sum v D,  Sdd = sum D^2
 *     k   = min(1, r / sqrt(Svv)),  1 when r == 0 or Svv == 0                    the norm threshold, in units of the data prediction
 *     p   = k Svd / Sdd,  0 when Sdd == 0;      q = (1 - eta) p                  the parallel coefficient and the share removed
 *     fac[b] = {(float)sqrt(Svv), (float)k, (float)p, (float)sqrt(Sdd)}
 * and per element again, with k and q as fp32:
 *     nn  = fmaf(-q, D, k * v)                    one multiplication, one fma: the orthogonal part + eta times the parallel part
 *     e_u = fp16(fmaf(nn, ig, e_c))               one fma, then a rounding of its own to fp16, to nearest even
 * The unchanged update then forms e_u' + s (e_c - e_u') = e_c - (s - 1) nn / g, the epsilon form of D_c + (s - 1) nn; the fold does
 * not read s.  With eta = 1, r = 0, beta_eff = 0 it writes e_u back (up to the roundings above): plain guidance.  Downstream
 * nothing changes: vd_cfg_rescale_factor_f16 (which keeps targeting the standard deviation of e_c) and every vd_cfg_*_step_* run on
 * the folded pair; vd_pag_fold_f16 runs after this fold and only adds to replica 0, so the two compose additively.
 * One block reduces and rewrites a sample, whatever the batch, in an order that depends on per_sample alone (per-lane fp64 sums, a
 * fixed butterfly over the wave, the waves added in order; no atomics; the same lane handles the same elements before and after the
 * block barrier), so a sample's fac, v and e_u are a pure function of its operands and coef: the same bits for any batch size,
 * batch position, alignment (16-byte accesses when x, both replicas and v of the sample are 16-byte aligned, else element-wise
 * accesses of the same elements with the same arithmetic), graph or rank.  Any per_sample.  Neither allocates nor synchronises
 * (capturable).  Returns < 0 (vd_last_error, the text starts with this entry's name) for null pointers, n or per_sample <= 0, n not
 * a multiple of per_sample, or x / eps / v / coef / fac not aligned to their element size. */
int vd_apg_fold_f16(const void* x, void* eps, float* v, const float* coef, float* fac, int64_t n, int64_t per_sample,
                    hipStream_t stream);

/* LoRA adapters (Hu et al., "LoRA: Low-Rank Adaptation of Large Language Models", 2021; not in the reference): the merge of up to
 * eight rank-r updates into one weight matrix, W = base + sum_a scale_a up_a down_a.  One entry point (additive to ABI 8), one launch
 * per parameter, between forwards (lib/model_zoo/lora.py).  The merge is always recomputed from a kept base, in a fixed order, so
 * its bits do not depend on which adapters were active before, and switching every adapter off gives the base back.
 *
 * vd_lora_merge: base and out are [N][K] row-major in the parameter's dtype, fp32 (out_is_f16 == 0) or fp16 (out_is_f16 != 0), and
 * never alias; terms is a HOST array of n_terms entries (copied into the kernel arguments: the array may be freed on return), up is
 * DEVICE fp32 [N][r] row-major, down DEVICE fp32 [r][K] row-major, scale the adapter's strength times alpha / r, formed by the host
 * in double and rounded once.  Per element, each line ONE fp32 operation, in this order and no other:
 *     acc = (float)base[n][k]                               exact
 *     for each term a in table order:
 *         d = 0;  for j = 0 .. r_a - 1 ascending:  d = fmaf(up_a[n][j], down_a[j][k], d)
 *         acc = fmaf(scale_a, d, acc)
 *     out[n][k] = acc                                       as it is (fp32), or rounded once to fp16, to nearest even
 * VALU fp32 throughout (the summation order inside an MFMA is not part of any contract), compiled without contraction; no padded
 * rank step is executed.  An element's result is a pure function of its own operands: the same bits for any alignment (16-byte /
 * 8-byte accesses of base and out when K % 4 == 0 and both are 16-byte aligned, else element-wise accesses of the same elements),
 * tile position or device.  Any N, K >= 1, 1 <= r <= 256, 1 <= n_terms <= 8.  Neither allocates nor synchronises (capturable).
 * Returns < 0 (vd_last_error, the text starts with this entry's name) for null pointers (the terms' included), n_terms outside 1..8,
 * r outside 1..256, N or K <= 0, base == out or overlapping, or operands not aligned to their element size. */
typedef struct VdLoraTerm {
    const float* up;   /* [N][r] row-major */
    const float* down; /* [r][K] row-major */
    float scale;
    int r;
} VdLoraTerm;
int vd_lora_merge(const void* base, void* out, int out_is_f16, const VdLoraTerm* terms, int n_terms, int N, int K,
                  hipStream_t stream);

/* Token merging for self-attention (Bolya & Hoffman, "Token Merging for Fast Stable Diffusion", 2023; the tomesd package with
 * sx = sy = 2, use_rand = False; not in the reference).  Four entry points (additive to ABI 8); none allocates or synchronises
 * (capturable).  Every one returns < 0 (vd_last_error, the text starts with the entry's name) for null pointers, an empty problem,
 * odd H or W, misaligned pointers, leading dimensions or sample strides, and r outside [0, Ns].
 *
 * Sets.  The tokens of a sample are n = y * W + x on its H x W grid (H, W even), N = H W.  Destinations: y and x both even, ordinal
 * d = (y / 2) (W / 2) + x / 2, Nd = N / 4.  Sources: every other token in ascending n, ordinal i, Ns = 3 N / 4.
 *
 * vd_tome_match_f16: h is the metric, fp16 rows [C] at h + b * sample_stride + n * ldh (16-byte aligned, ldh and sample_stride
 * multiples of 8), C in {32, 64, 128, 320, 640} (any other: < 0).  inv(n) = 1 / sqrt(sum_c h[n, c]^2) in fp32, 0 for an all-zero
 * row.  For every source i:  score(i, d) = <h_i, h_d> inv(i) inv(d), the products of fp16 values accumulated in fp32
 * (v_mfma_f32_32x32x16_f16; the score matrix never reaches memory); node_idx[b * Ns + i] = argmax_d score(i, d), among equal fp32
 * values of dot * inv(d) the lowest d; node_max[b * Ns + i] = that score (the factor inv(i) is applied once, behind the argmax).
 * The same input gives the same bits on every run.
 *
 * vd_tome_plan: rank[i] = #{j : node_max[j] > node_max[i], or node_max[j] == node_max[i] and j < i} per sample (a descending,
 * stable order on the fp32 values; NaN must not occur); source i is merged iff rank[i] < r.  The merged tensor has N' = N - r rows:
 * rows [0, Ns - r) are the unmerged sources, each at row rank[i] - r, rows [Ns - r, N') the destinations in ordinal order.
 * row_of is int32 [B, N] per TOKEN: a destination's own row, an unmerged source's own row, for a merged source the row of
 * destination node_idx[i].
 *
 * vd_tome_merge_f16: x fp16 [B, N, cols] (row n of sample b at x + b * sx + n * ldx; cols a multiple of 8, so a column slice of a
 * fused projection is fine) -> out [B, N', cols] (ldo, so).  Unmerged source rows are bit-exact copies.  A destination row is the
 * mean over itself and every source merged into it: the sum is EXACT (fp16 values are integers in units of 2^-24, summed as
 * int64), the quotient is double(sum) / count, rounded ONCE to nearest even straight to fp16 (not double -> float -> half) -- so
 * the result does not depend on the order of the members.  No atomics touch the data tensor.  Ns <= 12288 (grids up to 128 x 128),
 * else < 0.
 *
 * vd_tome_unmerge_f16: out[b, n, :] = a[b, row_of[b, n], :] for the N tokens, a bit-exact gather of a [B, N', cols] (lda, sa). */
int vd_tome_match_f16(const void* h, int ldh, int64_t sample_stride, int B, int H, int W, int C, int* node_idx, float* node_max,
                      hipStream_t stream);
int vd_tome_plan(const int* node_idx, const float* node_max, int B, int H, int W, int r, int* row_of, hipStream_t stream);
int vd_tome_merge_f16(const void* x, int ldx, int64_t sx, int cols, const int* row_of, int B, int H, int W, int r, void* out,
                      int ldo, int64_t so, hipStream_t stream);
int vd_tome_unmerge_f16(const void* a, int lda, int64_t sa, int cols, const int* row_of, int B, int H, int W, int r, void* out,
                        int ldo, int64_t so, hipStream_t stream);

/* HyperTile: tiled self-attention (tfernd, "HyperTile: Tiled-optimizations for Stable-Diffusion", 2023; not in the reference).  Two
 * entry points (additive to ABI 8); neither allocates or synchronises (capturable), each is ONE launch whatever B is, and both are
 * bit-exact copies of 16-byte chunks: a fixed, data-independent permutation of rows.
 *
 * The tokens of a sample are n = y * W + x on its H x W grid, cut into nty x ntx tiles of th x tw tokens (nty = H / th,
 * ntx = W / tw).  The tiled tensor t is CONTIGUOUS fp16 [B nty ntx, th tw, cols]: a tile is a sample of its own, so an attention
 * over t attends inside a tile only.
 *
 * vd_tile_tokens_f16: x fp16 [B, H W, cols], row n of sample b at x + b * sx + n * ldx (elements; cols a multiple of 8 and rows
 * 16-byte aligned, so the fused q | k | v of a block, a column slice of it and a batch slice qualify as they are) ->
 *     out[(b * nty + ty) * ntx + tx, i * tw + j, :] = x[b, (ty * th + i) * W + tx * tw + j, :]      0 <= i < th, 0 <= j < tw
 * vd_untile_tokens_f16: the exact inverse, a [B nty ntx, th tw, cols] contiguous -> out [B, H W, cols] (ldo, so): every row of out
 * is written exactly once.  One tile (th = H, tw = W) is the identity copy.
 *
 * Both return < 0 (vd_last_error, the text starts with the entry's name) and launch nothing for a null pointer, a non-positive
 * size, cols % 8 != 0, H % th != 0 or W % tw != 0, a leading dimension below cols, a pointer that is not 16-byte aligned, a leading
 * dimension or sample stride that is no multiple of 8, a sample stride (B > 1) below the rows of a sample, and B H W cols / 8 >= 2^32
 * (the chunk index is 32-bit; every offset is 64-bit). */
int vd_tile_tokens_f16(const void* x, int ldx, int64_t sx, int cols, int B, int H, int W, int th, int tw, void* out,
                       hipStream_t stream);
int vd_untile_tokens_f16(const void* a, int cols, int B, int H, int W, int th, int tw, void* out, int ldo, int64_t so,
                         hipStream_t stream);

/* q_sample: out = sa[b] * x0 + sb[b] * noise  (lib/model_zoo/vd.py:221-224). */
int vd_q_sample_f16(const void* x0, const void* noise, const float* sa, const float* sb, void* out, int B,
                    int64_t per_batch, hipStream_t stream);

/* layout changes at the API boundary (reference tensors are NCHW) */
int vd_nchw_to_nhwc_f16(const void* x, void* y, int B, int C, int H, int W, hipStream_t stream);
int vd_nhwc_to_nchw_f16(const void* x, void* y, int B, int C, int H, int W, float scale, float shift, int clamp01,
                        hipStream_t stream);

/* Small-Cin im2col: A[m][kpad] (zero padded, k = (ky*ks+kx)*C + c) from a strided fp16 image, with the
 * affine x*in_scale+in_shift applied to valid pixels (fuses `x*2-1`, autokl.py:34 and `z/scale`, vd.py:294). */
int vd_im2col_small_f16(const void* x, void* a, int B, int C, int Hin, int Win, int Hout, int Wout, int ksize,
                        int stride, int pad, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int kpad,
                        float in_scale, float in_shift, hipStream_t stream);

/* DiagonalGaussianDistribution.sample fused with the latent scale:
 *   z = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale ; moments channels-last [M][2*zc], z NCHW
 * (lib/model_zoo/distributions.py:24-37, vd.py:282-289). */
int vd_diag_gaussian_sample_f16(const void* moments, const void* noise, void* z, int B, int zc, int HW, float scale,
                                hipStream_t stream);

/* out = a * x + b * y (context mixing helpers, vd.py:383-396) */
int vd_axpby_f16(const void* x, const void* y, void* out, float a, float b, int64_t n, hipStream_t stream);

/* out = f(x) element-wise (in place allowed): erf-GELU of BERT's intermediate layer and the tanh of its pooler in the
 * Optimus encoder (lib/model_zoo/optimus_models/optimus_bert.py:139-150 `gelu`, :451-463 BertPooler). */
#define VD_UNARY_GELU_ERF 0
#define VD_UNARY_TANH 1
int vd_unary_f16(const void* x, void* out, int op, int64_t n, hipStream_t stream);

/* CLIP helpers (arithmetic of HF transformers CLIPModel as called from lib/model_zoo/clip.py) */
int vd_embed_tokens_f16(const int64_t* ids, const void* tok_emb, const void* pos_emb, void* out, int B, int L, int C,
                        hipStream_t stream);
int vd_clip_vision_embed_f16(const void* patches, const void* class_emb, const void* pos_emb, const float* token_scale,
                             void* out, int B, int L, int C, hipStream_t stream);
int vd_patchify_f16(const void* pixels, void* a, int B, int C, int H, int W, int P, int kpad, hipStream_t stream);
/* z[b][l][:] *= row_scale[b][l] / ||ref[b][:]||  (ref row = z[b][pool_idx[b]], or `ref` if given) */
int vd_scale_by_row_norm_f16(void* z, const void* ref, const int32_t* pool_idx, const float* row_scale, int B, int L,
                             int C, hipStream_t stream);

/* CLIP image pre-processing on the device, bit-exact with the reference's host path (lib/model_zoo/clip.py:88-94:
 * torchvision ToPILImage -> HuggingFace CLIPProcessor = Pillow 8-bit bicubic resize of the shortest edge, centre crop,
 * rescale, normalise).  img [B,3,H,W]: img_kind 0 = float32 / 1 = float16 in [0,1] (quantised like ToPILImage:
 * mul(255).byte()), 2 = uint8.  (rh, rw) = resized size, crop window (crop_t, crop_l, size).  hb/hk, vb/vk: Pillow's
 * fixed-point taps per output column / row (device int32: bounds[out][2] = {first input index, taps}, kk[out][ks], 22
 * fractional bits; ks = 0 and null tables when that axis is not resized).  norm_table: device float32 [256][3] =
 * (level * (1/255) - mean[c]) / std[c].  tmp: B*3*H*size bytes of scratch.  out [B,3,size,size] float16. */
int vd_clip_preprocess_f16(const void* img, int img_kind, int B, int H, int W, int rh, int rw, const int32_t* hb,
                           const int32_t* hk, int hks, const int32_t* vb, const int32_t* vk, int vks, int crop_t, int crop_l,
                           int size, const float* norm_table, uint8_t* tmp, void* out, hipStream_t stream);

/* Decoded image [B,3,H,W] (img_kind 0 = float32, 1 = float16, values in [0,1]) -> uint8 [B,H,W,3], the arithmetic of
 * torchvision ToPILImage on the output of vae_decode (reference app.py:319): mul(255) in the tensor's dtype, .byte(). */
int vd_image_to_u8(const void* img, int img_kind, int B, int H, int W, uint8_t* out, hipStream_t stream);

/* Mask -> per-token weights of the masked CLIP image context (lib/model_zoo/clip.py:104-122): masks [B,1,H,W]
 * (mask_kind 0 = float32, 1 = float16) are clamped to [0,1], resized to size x size like F.interpolate(mode='bilinear')
 * and averaged per patch x patch cell; out [B][1 + (size/patch)^2] fp32 = [global mean | patch means]. */
int vd_mask_patch_weights(const void* masks, int mask_kind, int B, int H, int W, int size, int patch, float* out,
                          hipStream_t stream);

/* 'Simple' colour adjustment of image variation (app.py:373-379): per image and channel
 *   out = clamp((img - mean(img)) / std(img) * std(ref) + mean(ref), 0, 1)   (unbiased std over the H*W pixels)
 * img / out [B,3,H,W] fp16, ref [3,H,W] (ref_batch_stride = 0: one input image for the whole batch, as the app does) or
 * [B,3,H,W] (ref_batch_stride = 3*H*W). */
int vd_color_adjust_f16(const void* img, const void* ref, void* out, int B, int H, int W, int64_t ref_batch_stride,
                        hipStream_t stream);

/* Focus control of the image context ("adjust_rank", app.py:48-127): per sample x [L][C] (fp16 in, fp16 out)
 *   A = x - rowmean(x);  U = top-q left singular vectors of A (= what torch.pca_lowrank(q, niter=100) converges to)
 *   x_new = keep * A + sum_i g[i] * U[:,i] (U[:,i]^T A) + rowmean(x);   y = x_new * std(x) / std(x_new)   (unbiased std)
 * with g[i] = f_i - keep from the reference's level -> singular-value-scale curves (host side, lib/app_ops.py); keep = 1
 * keeps the remainder beyond rank q (lvl < 0.5), keep = 0 drops it (lvl > 0.5).  U comes from `iters` steps of a
 * 32-column subspace iteration on A A^T in fp32.  32 <= L <= 512, q <= 32.  ws: vd_adjust_rank_workspace_bytes(). */
int vd_adjust_rank_f16(const void* x, void* y, int B, int L, int C, int q, const float* g, float keep, int iters, float* ws,
                       hipStream_t stream);
size_t vd_adjust_rank_workspace_bytes(int B, int L, int C, int q);

/* diagnostics */
const char* vd_last_error(void);
int vd_abi_version(void);
/* writes lane->(row,col) maps of the 32x32x16 f16 MFMA as observed on the device; used by tests */
int vd_probe_mfma_layout(int32_t* out_a_k, int32_t* out_c_row, int32_t* out_c_col, hipStream_t stream);
/* ds_read_b64_tr_b16 as observed on the device: LDS holds lds[i] = i (4096 int16); lane l reads at byte address
 * addr_bytes[l] (64 entries) and out[l*4 + j] receives its four 16-bit results; used by tests (the attention kernel's
 * V operand relies on this gather) */
int vd_probe_lds_tr16(const int32_t* addr_bytes, int16_t* out, hipStream_t stream);
/* XCD (HW_REG_XCC_ID) of every block of a grid_x x grid_y launch of 256-thread blocks, int32 [grid_y][grid_x]: pins the
 * dispatcher's round-robin placement (block b of the linearised grid runs on XCD b % 8) that the tile order of the GEMM /
 * convolution kernels exploits for L2 locality and the ticketed split of conv3x3_halo_kernel relies on. */
int vd_probe_xcc_ids(int32_t* out, int grid_x, int grid_y, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VD_HIP_H */
