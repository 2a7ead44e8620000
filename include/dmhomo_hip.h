/*
 * dmhomo_hip.h — C ABI of libdmhomo_hip.so: the gfx950 (MI355X / CDNA4) kernels under
 * the DGM denoising hot path of lhaippp/DMHomo.
 *
 * The reference is pure Python/PyTorch and has NO native / FFI layer (SURVEY.md §0 fact 1,
 * §8b): every entry point below replaces a *sequence of stock ATen ops* in the reference,
 * cited per function as
 *      CFG = DGM/denoising_diffusion_models/classifier_free_guidance.py
 *      DDP = DGM/denoising_diffusion_models/denoising_diffusion_pytorch.py
 * and is bound from Python with ctypes (dmhomo_amd/_lib.py; INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller
 *     (torch tensors' data_ptr()), unless the name says host;
 *   - activations are fp32 NHWC ([B][H][W][C], C % 4 == 0); API-boundary images are the
 *     reference's fp32 NCHW;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued asynchronously on it, nothing synchronises, nothing allocates
 *     (graph-capture safe);
 *   - return 0 on success, a negative DMH_E* code otherwise; dmh_last_error() gives the
 *     thread-local message. No exceptions cross the ABI.
 */
#ifndef DMHOMO_HIP_H
#define DMHOMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMH_OK 0
#define DMH_EINVAL (-1)  /* bad argument / unsupported shape */
#define DMH_ELAUNCH (-2) /* hip launch error */

const char* dmh_last_error(void);
/* DMH_ABI_VERSION of the library: bumped whenever a struct layout or an entry point changes; a binding must refuse a
 * library whose version differs from the header it was written against (dmhomo_amd/_lib.py does). */
#define DMH_ABI_VERSION 500
int dmh_version(void);

/* ---------------------------------------------------------------------------------------
 * Weight preparation (once per load_state_dict; weights are constant while sampling)
 * ------------------------------------------------------------------------------------- */

/* N1  WeightStandardizedConv2d weight fold, CFG:120-126:
 *   w_out[o] = (w[o] - mean_o) * rsqrt(var_biased_o + eps), stats over the K = Cin*kh*kw
 *   elements of output channel o.  w, w_out: [Cout][K]. */
int dmh_ws_standardize(const float* w, float* w_out, int Cout, int K, float eps, void* stream);

/* number of floats of the packed image of an OIHW weight for dmh_conv2d.
 * Every pure size function of this header (dmh_*_floats, dmh_conv_tiles, dmh_*_splits, dmh_multi_blocks) answers -1 for a
 * dimension outside (0, 2^20] (pixel counts: 2^26) or a NULL array instead of entering the size arithmetic with it. */
int64_t dmh_conv_pack_floats(int Cout, int C0, int C1, int KH, int KW);

/* OIHW [Cout][C0+C1][KH][KW] -> the image dmh_conv2d consumes (an opaque blob of dmh_conv_pack_floats floats; pack
 * again whenever the weight changes).  Default kernels (3x3, 1x1, 7x7, 4x4/stride 2): every output channel scaled by
 * a power of two, split into two fp16 planes and stored in MFMA-fragment order, followed by the per-channel 2^-k
 * (dmhomo_amd/csrc/conv_f16x3.hip); exact-fp32 kernels (2x2/stride 2, channel counts that are not a multiple of 32
 * for the strided conv, or DMH_CONV3_VARIANT != 9): tile-major fp32 [ntile][chunk][tap][64][KC].  Chunks never
 * straddle the two concatenated sources; padding is zero. */
int dmh_pack_conv_weight(const float* w_oihw, float* wpack, int Cout, int C0, int C1, int KH, int KW,
                         void* stream);
/* Many weights at once (the training step re-packs ~140 convolution weights after every optimiser update, DDP:1857: one
 * image for the forward conv and one for the data-gradient conv of each): three kernel phases over ALL jobs — weight
 * standardisation (N1) where a job asks for it, the per-output-channel power-of-two scales, the fp16-piece images — instead of
 * two or three launches per weight.  Only the fp16-piece images of stride-1 1x1 / 3x3 convolutions (the default kernels).
 *   src          OIHW weight the image is made from (after standardisation when ws != NULL)
 *   ws           NULL, or [Cout_src][K] scratch: src is standardised into it first (CFG:120-126) and the image is made from it;
 *                a later job may name this buffer as its src (phase 1 completes before phase 2 starts)
 *   transposed   0: the image of conv(src).  1: the image of the DATA-GRADIENT conv of conv(src) — taps flipped, (Cout, Cin)
 *                exchanged — for which Cout / C0 below are Cin_src / Cout_src and src is [C0][Cout][KH][KH]
 * jobs is a HOST array; nothing is read from it after the call returns. */
typedef struct DmhPackJob {
  const float* src;
  float* ws;
  float* wpack;       /* dmh_conv_pack_floats(Cout, C0, C1, KH, KH) floats */
  int32_t Cout, C0, C1, KH;
  int32_t transposed;
} DmhPackJob;
int dmh_pack_conv_weights_multi(const DmhPackJob* jobs, int njobs, float ws_eps, void* stream);

/* Upsample(nearest x2) + conv3x3 (CFG:106-107) in its sub-pixel form: output pixel (2y+dy, 2x+dx) depends on a 2x2
 * low-resolution neighbourhood through sums of the 3x3 taps, so the conv runs as four 2x2 convs (16 instead of 36
 * multiply-adds per low-resolution pixel; tap sums are formed in fp32 at pack time).  dmh_conv_up2_pack_floats returns
 * -1 when the build's conv variant / the shape (Cout % 64, one source) does not offer it; use the image with
 * DmhConv.upsample2 = 2, KH = KW = 3, stride = 1. */
int64_t dmh_conv_up2_pack_floats(int Cout, int C0);
int dmh_pack_conv_weight_up2(const float* w_oihw, float* wpack, int Cout, int C0, void* stream);

/* ---------------------------------------------------------------------------------------
 * Row subsets (round 5): de-duplication of the two classifier-free-guidance passes inside a captured denoise step.
 * forward_with_cond_scale (CFG:403-410) runs the UNet on the batch twice: once with the class embedding of every row
 * replaced by the null embedding with probability cond_drop_prob (CFG:415-425 — 0.5 in DGM, also while sampling), once with
 * all of them replaced.  A row the first pass dropped has exactly the inputs of its row in the second pass, so its logits are
 * the second pass's logits and need not be computed.  Which rows are kept is DEVICE data (the mask is drawn inside the
 * captured step), so every batched entry point of the UNet takes an optional `rows`:
 *     rows == NULL          all B rows of the launch
 *     rows[0]               n <= B, the number of active rows
 *     rows[1 + j], j < n    the row (sample slot) logical row j works on
 * The launch keeps its B-row grid; workgroups of logical rows >= n retire before touching memory, tensors are addressed by
 * the slot, nothing is gathered or scattered, and the slots that are not listed are neither read nor written.  Rows are
 * independent of each other in every kernel of the path, so the listed rows come out bit for bit as in the full launch.
 * dmh_rows_from_keep builds the list: the slots b < B with keep[b] != 0 in ascending order, followed by B .. B+extra-1
 * (the null pass's rows when both passes share one 2B-row launch); rows: int32 [1 + B + extra], all DEVICE memory. */
int dmh_rows_from_keep(const uint8_t* keep, int B, int extra, int32_t* rows, void* stream);

/* ---------------------------------------------------------------------------------------
 * K1/K2  convolution as an implicit GEMM.  fp32 tensors in and out; by default the products run on the fp16
 * matrix cores with every fp32 operand carried as block-scaled fp16 pieces (three v_mfma_f32_16x16x32_f16 per
 * product block, fp32 accumulation; error at the level of the fp32 accumulation rounding, fp32 exponent range —
 * DESIGN.md 3.1).  DMH_CONV3_VARIANT=0 / 6 (environment, read once) selects the exact-fp32 MFMA kernels.
 * ------------------------------------------------------------------------------------- */
typedef struct DmhConv {
  uint64_t struct_size; /* sizeof(DmhConv) of the header the caller was built against: dmh_conv2d refuses any other value
                           (the struct has grown between library versions; a shorter one would be read past its end) */
  const float* src0; /* NHWC [B][Hin][Win][C0] */
  const float* src1; /* NHWC [B][Hin][Win][C1] or NULL: torch.cat((src0, src1), dim=1) fused (CFG:454,457,463) */
  const float* wpack; /* dmh_pack_conv_weight image */
  const float* bias;  /* [Cout] or NULL */
  /* prologue on src0 (C1 must be 0): x <- SiLU(a[b][c]*x + b[b][c]) with coef = [B][2][C0]
   * from dmh_gn_finalize: GroupNorm + (scale+1, shift) + SiLU of the producing Block, CFG:206-212 */
  const float* in_coef;
  /* epilogue residual, NHWC [B][Hout][Wout][Cout] or NULL:
   *   res_coef == NULL : out += res                      (Residual, CFG:102-103)
   *   res_coef != NULL : out += SiLU(a*res + b)          (h + res_conv(x), CFG:241, h = block2 output) */
  const float* res;
  const float* res_coef;
  float* out;   /* NHWC [B][Hout][Wout][Cout] */
  float* stats; /* NULL or [B][tiles][Cout][2] per-tile (sum, sum of squares) of `out` for GroupNorm */
  int32_t B, Hin, Win, C0, C1, Cout;
  int32_t KH, KW;     /* 1x1, 3x3, 7x7 (stride 1, pad k/2); 4x4 (stride 2, pad 1); 2x2 (stride 2, pad 0) */
  int32_t stride;     /* 1 or 2 */
  int32_t upsample2;  /* 1: nearest x2 of the input fused into the 3x3 gather (Upsample, CFG:106-107);
                         2: the same conv with a wpack from dmh_pack_conv_weight_up2 (four 2x2 sub-pixel convs) */
  /* optional, with in_coef: in_bound[b * in_bound_n + i], i < in_bound_n — upper bounds of |a*x + b| over the elements
   * of sample b (dmh_gn_finalize_bound: one per GroupNorm group).  The fp16-piece kernels then take their block scale
   * from max_i in_bound instead of searching the staged tile for its maximum; the result is the same convolution. */
  const float* in_bound;
  int32_t in_bound_n;
  /* optional (1x1, stride 1, Cout <= 64, the fp16-piece kernels): a second, pointwise projection applied to the finished
   * output pixel while it is still in registers — fin_out[b][o][y][x] = fin_b[o] + sum_c fin_w[o][c] * out[b][y][x][c],
   * o < fin_n <= 8, written NCHW: the UNet's final_conv (CFG:341, 471-472) fused into the last ResnetBlock's res_conv
   * launch, bit for bit what dmh_final_conv_nchw computes from `out`.  With fin_w set, out may be NULL (not stored). */
  int32_t fin_n;
  const float* fin_w; /* [fin_n][Cout] */
  const float* fin_b; /* [fin_n] or NULL */
  float* fin_out;     /* NCHW [B][fin_n][Hout][Wout] */
  /* optional (1x1, stride 1, Cout == 64, the fp16-piece kernels): pix_stats[(b*Hout + y)*Wout + x][2] = (mean, rstd) of the
   * channel LayerNorm (CFG:137-141, eps pix_eps) of every finished output pixel — bit for bit what dmh_pixel_stats computes
   * from `out` — for the fused LinearAttention that consumes this launch's output (the up path's res_conv, CFG:241 -> 246). */
  float* pix_stats;
  float pix_eps;
  /* optional: the active row subset of this launch (see "Row subsets" below); NULL = all B rows */
  const int32_t* rows;
} DmhConv;

/* tiles per sample that dmh_conv2d will use for this geometry (size of the stats buffer) */
int dmh_conv_tiles(int Hout, int Wout, int KH, int stride);
int dmh_conv2d(const DmhConv* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Normalisation / activation glue (HBM-bound)
 * ------------------------------------------------------------------------------------- */

/* N2  GroupNorm statistics -> per-(sample, channel) affine of Block.forward, CFG:206-210:
 *   coef[b][0][c] = a = rstd*gamma*(scale+1), coef[b][1][c] = (beta - mean*rstd*gamma)*(scale+1) + shift
 * stats: [B][tiles][C][2] from dmh_conv2d; ss: NULL or row b at ss + b*ss_stride holds
 * (scale[C], shift[C]) (ResnetBlock mlp output chunk(2), CFG:233-235). Reduction in f64, fixed order. */
int dmh_gn_finalize(const float* stats, int tiles, const float* gamma, const float* beta, const float* ss,
                    int64_t ss_stride, float* coef, int B, int C, int groups, int hw, float eps, const int32_t* rows,
                    void* stream);

/* dmh_gn_finalize + bound[B][groups]: max over the group's channels of |a| * sqrt(sum x^2) + |b + mean*a| >= |a*x + b|
 * for every element x of the (sample, group) the statistics describe (DmhConv.in_bound) */
int dmh_gn_finalize_bound(const float* stats, int tiles, const float* gamma, const float* beta, const float* ss,
                          int64_t ss_stride, float* coef, float* bound, int B, int C, int groups, int hw, float eps,
                          const int32_t* rows, void* stream);

/* out = SiLU(a*y + b) + res   (identity res_conv branch of ResnetBlock, CFG:225,241) */
int dmh_gn_silu_residual(const float* y, const float* coef, const float* res, float* out, int B, int HW, int C,
                         const int32_t* rows, void* stream);

/* same, also writing pstats [B*HW][2] = (mean, rstd) of the channel LayerNorm (CFG:137-141) of every output pixel —
 * bitwise what dmh_pixel_stats(out) gives — for a LinearAttention that follows the block (CFG:176-183). C in {64,128,256}. */
int dmh_gn_silu_residual_stats(const float* y, const float* coef, const float* res, float* out, float* pstats, int B,
                               int HW, int C, float eps, const int32_t* rows, void* stream);

/* N4  channel LayerNorm (biased var, gain only), CFG:137-141, optionally + res (Residual, CFG:103).
 * rows (optional row subset) comes with pix_per_row = the pixels of one row, npix = B * pix_per_row. */
int dmh_chan_layernorm(const float* x, const float* g, const float* res, float* out, int64_t npix, int C,
                       float eps, const int32_t* rows, int64_t pix_per_row, void* stream);

/* ---------------------------------------------------------------------------------------
 * K3  LinearAttention core, CFG:258-269.  qkv: NHWC [B][n][384] = (q|k|v) x 4 heads x 32.
 * ------------------------------------------------------------------------------------- */
int dmh_linattn_splits(int n);
int64_t dmh_linattn_partial_floats(int B, int n);
/* pass 1: per split of the n pixels, running max / sum of exp / unnormalised k^T v per head */
int dmh_linattn_context(const float* qkv, float* partial, int B, int n, const int32_t* rows, void* stream);
/* merge the splits: ctx[b][h][d][e] = softmax_n(k)[d,:] . (v/n)[e,:] */
int dmh_linattn_merge(const float* partial, float* ctx, int B, int n, const int32_t* rows, void* stream);
/* pass 2: out[b][p][h*32+e] = sum_d ctx[d][e] * (softmax_d(q[p]) * scale)[d]; out NHWC [B][n][128] */
int dmh_linattn_apply(const float* qkv, const float* ctx, float* out, int B, int n, float scale, const int32_t* rows,
                      void* stream);

/* Fused LinearAttention (PreNorm LayerNorm + to_qkv + attention core, CFG:96-103,246-269): q, k, v stay on chip.
 *   stats  = dmh_pixel_stats(x)                         per-pixel (mean, rstd) of the PreNorm LayerNorm, [npix][2]
 *   wpack  = dmh_linattn_fused_pack(to_qkv.weight)      once per weight version; dmh_linattn_fused_pack_floats(C) floats
 *   dmh_linattn_fused_context -> partial[B][dmh_linattn_fused_splits(B,n)][4][1088]
 *   dmh_linattn_merge_n       -> ctx[B][4][32][32]
 *   dmh_linattn_fused_apply   -> out[B][n][128]         (then to_out conv + LayerNorm + residual as before)
 * x: NHWC [B][n][C], C a multiple of 32. */
int dmh_pixel_stats(const float* x, float* stats, int64_t npix, int C, float eps, const int32_t* rows, int64_t pix_per_row,
                    void* stream);
int64_t dmh_linattn_fused_pack_floats(int C);
int dmh_linattn_fused_pack(const float* w_qkv, float* wpack, int C, void* stream);
int dmh_linattn_fused_splits(int B, int n);
int dmh_linattn_fused_context(const float* x, const float* stats, const float* ln_g, const float* wpack,
                              float* partial, int B, int n, int C, const int32_t* rows, void* stream);
int dmh_linattn_merge_n(const float* partial, float* ctx, int B, int n, int nsplit, const int32_t* rows, void* stream);
int dmh_linattn_fused_apply(const float* x, const float* stats, const float* ln_g, const float* wpack,
                            const float* ctx, float* out, int B, int n, int C, float scale, const int32_t* rows,
                            void* stream);
/* C == 64: pass 2 carries the rest of the block too — y[B][n][64] = x + LayerNorm(to_out(attention) + bias) * g
 * (CFG:254-256, 103): the to_out weight [64][128] is packed once by dmh_linattn_out_pack
 * (dmh_linattn_out_pack_floats() floats). */
int64_t dmh_linattn_out_pack_floats(void);
int dmh_linattn_out_pack(const float* w_out, float* wpack, void* stream);
int dmh_linattn_fused_apply_out(const float* x, const float* stats, const float* ln_g, const float* wpack,
                                const float* ctx, const float* wopack, const float* out_bias, const float* out_ln_g,
                                float* y, int B, int n, int C, float scale, float eps, const int32_t* rows, void* stream);

/* K4  Attention core, CFG:287-295: softmax_j((q*scale)^T k) v; out NHWC [B][n][128] */
int dmh_attention(const float* qkv, float* out, int B, int n, float scale, const int32_t* rows, void* stream);

/* ---------------------------------------------------------------------------------------
 * K5  embeddings / small linears
 * ------------------------------------------------------------------------------------- */
/* N7  SinusoidalPosEmb, CFG:165-172: out[r] = (sin(t_r*f), cos(t_r*f)); freq[dim/2] fp32 table */
int dmh_sinusoidal_embed(const int64_t* t, const float* freq, float* out, int R, int dim, void* stream);
/* RandomOrLearnedSinusoidalPosEmb, CFG:175-190 [DDP:179-195] (Unet(learned_sinusoidal_cond / random_fourier_features)):
 * out[r] = (t_r, sin(t_r*w_i*2*pi) i < half, cos(t_r*w_i*2*pi) i < half), out [R][2*half + 1]; weights [half] */
int dmh_fourier_embed(const int64_t* t, const float* weights, float* out, int R, int half, void* stream);
/* N8  classes_emb lookup + null swap, CFG:419-425: keep==NULL keeps every row; table [num_classes][dim] — a kept class id
 * outside [0, num_classes) yields a NaN row (device data: it cannot be refused at launch) */
int dmh_class_embed(const int64_t* classes, const uint8_t* keep, const float* table, const float* null_emb,
                    float* out, int R, int dim, int num_classes, void* stream);
/* y[r][o] = act_out( sum_i act_in(x[r][i]) * wt[i][o] + bias[o] ), wt = W^T [in][out].
 * act: 0 none, 1 SiLU, 2 GELU(erf).  (time_mlp / classes_mlp CFG:353,362; ResnetBlock.mlp CFG:220) */
int dmh_linear(const float* x, int64_t x_stride, const float* wt, const float* bias, float* y, int64_t y_stride,
               int R, int in_dim, int out_dim, int act_in, int act_out, void* stream);

/* The (scale, shift) rows of all ResnetBlocks (ResnetBlock.mlp CFG:220,231-235 over [time_mlp(t) | classes_mlp(c)], CFG:427,435)
 * of a REPLAYED denoise step from tables: out[b][0..N) = (T[*cursor] + C[keep[b] ? classes[b] : ncls]) + bias, with T [S][N] the
 * time half's partial sums of dmh_linear per denoise step and C [ncls+1][N] the class half's per class (last row: null
 * embedding), both made by dmh_linear itself on inputs whose other half is zero; bitwise dmh_linear on the full input.
 * cursor: the step cursor of dmh_sampler_seek (device); keep may be NULL (every class kept).  S = rows of T: a cursor outside
 * [0, S) or a kept class outside [0, ncls) cannot be refused at launch (device data) and yields a NaN row. */
int dmh_ss_gather(const float* T, const float* C, const float* bias, const int32_t* cursor, const int64_t* classes,
                  const uint8_t* keep, int ncls, float* out, int B, int N, int S, void* stream);

/* ---------------------------------------------------------------------------------------
 * K6  sampler glue (NCHW at the API boundary)
 * ------------------------------------------------------------------------------------- */
/* network input: out NHWC [reps*B][H][W][Cpad] <- cat(a [B][Ca][H][W], b*m [B][Cb][H][W]) zero padded;
 * b, m may be NULL (Cb = 0).  torch.concat((x, rgb_flow*mask)) CFG:430 / cat((x_self_cond, x)) DDP:411 */
int dmh_assemble_input(const float* a, int Ca, const float* b, int Cb, const float* m, float* out, int B, int reps,
                       int HW, int Cpad, void* stream);
/* final_conv 1x1 (CFG:401,466): NHWC [R][HW][C] -> NCHW [R][Cout][HW], Cout <= 16 */
int dmh_final_conv_nchw(const float* x, const float* w, const float* bias, float* out, int R, int HW, int C,
                        int Cout, void* stream);

typedef struct DmhStep {
  int32_t objective;  /* 0 pred_noise, 1 pred_x0, 2 pred_v            CFG:614-628 */
  int32_t clip;       /* clamp x_start to [-1,1]                       CFG:612 */
  int32_t mode;       /* 0 DDIM update, 1 DDIM last (img = x_start), 2 DDPM posterior step, 3 multistep (the _ms entry points) */
  float cond_scale;   /* CFG blend null + (cond-null)*s, CFG:410; ignored when model_null == NULL */
  float sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac, sqrt_1m_ac; /* extract(..., t) CFG:586-601 */
  float c0, c1, c2;   /* DDIM: sqrt(alpha_next), c, sigma (CFG:697-707); DDPM: coef1, coef2, exp(.5 logvar);
                       * multistep: img' = (c0 * x_start + c1 * img) + c2 * (the previous step's x_start) */
} DmhStep;
/* one sampler step on NCHW tensors of n elements: writes img_out and (if non-NULL) x_start, pred_noise.
 * keep (optional, with model_null; per_row = elements of one row): uint8 [n / per_row] — rows with keep == 0 were not computed
 * by the conditional pass (row subsets, above) and take model_null as their conditional logits, which is what CFG:404,409
 * compute for a row whose class was dropped. */
int dmh_sampler_step(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                     const float* noise, float* img_out, float* x_start, float* pred_noise, int64_t n,
                     const uint8_t* keep, int64_t per_row, void* stream);

/* The same step with its DmhStep read from DEVICE memory, for a sampling loop (CFG:683-707, DDP:647-735) that replays
 * ONE captured denoise step from a HIP graph: the host fills `table` (one DmhStep per denoise step, host-computed as
 * the reference computes them, CFG:697-701) and `times` once; a device cursor selects the current entry.
 * img_out may alias x (the loop's `img = ...` in place); mode and objective are validated when the table is built. */
int dmh_sampler_step_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                         const float* noise, float* img_out, float* x_start, float* pred_noise, int64_t n,
                         const uint8_t* keep, int64_t per_row, void* stream);
/* cursor handling of that loop (one tiny launch): k >= 0: *cursor = k; k < 0: *cursor = min(*cursor + 1, S - 1); then
 * *cur = table[*cursor] and tcond[0 .. B) = times[*cursor] (the `time_cond` tensor of CFG:684 / DDP:700).
 * table: [S] DmhStep, times: [S] int64, cursor: int32, all device memory. */
int dmh_sampler_seek(int32_t* cursor, int k, const DmhStep* table, const int64_t* times, int S, DmhStep* cur,
                     int64_t* tcond, int B, void* stream);

/* The replayed step of the UNCONDITIONAL loop (p_sample_loop / ddim_sample, DDP:647-729) in one launch: the step of
 * dmh_sampler_step_dev (entry *cur_dev, no model_null) applied in place to img [B][C][HW], plus its noise and the next step's
 * network input.  draws: [S] int32 device table next to the step table, indexed by *cursor: 0 for an entry that the eager loop
 * runs without noise (t == 0 of the ancestral loop, the last DDIM step) — it neither draws nor advances the generator.
 * Noise source (at most one): sample_ids + state = the keyed generator of dmh_rng_indexed (kind 0), drawn in the kernel with
 * the same counter layout, so bit-identical to what dmh_rng_indexed would have stored, and the draw index advanced once per
 * drawing launch as dmh_rng_indexed advances it; or noise [B][C][HW] (e.g. torch.randn).  A drawing entry without a source
 * yields NaN.  x_start (optional): [B][C][HW].  xin_next (optional): NHWC [B][HW][cpad] = cat(x_start, img) with self_cond,
 * img without, zero padded: what dmh_assemble_input builds for the next step (DDP:411).  cpad: multiple of 4 >= C*(1+self_cond). */
int dmh_sampler_step_ddp_dev(const DmhStep* cur_dev, const int32_t* cursor, const int32_t* draws, const float* model_out,
                             float* img, const float* noise, const int64_t* sample_ids, uint64_t* state, float* x_start,
                             float* xin_next, int B, int C, int HW, int cpad, int self_cond, void* stream);

/* The step of the second-order multistep solver (DPM-Solver++ 2M in data prediction; not in the reference): mode 3 computes
 * img_out = (c0 * x_start + c1 * x) + c2 * hist with x_start the clamped data prediction of the entry, exactly the value the
 * DDIM update uses; mode 1 is the last step as above.  No noise.  hist: [n] floats, the previous step's x_start: each thread
 * reads its own element when c2 != 0 (an entry with c2 == 0 never reads it: the first step may find anything there) and then
 * stores the new x_start.  Guided blend, keep / per_row and aliasing of img_out with x as dmh_sampler_step[_dev]; the host-struct
 * form refuses modes 0 and 2, the device-struct form is validated when the table is built. */
int dmh_sampler_step_ms(const DmhStep* s, const float* model_cond, const float* model_null, const float* x, float* hist,
                        float* img_out, float* x_start, int64_t n, const uint8_t* keep, int64_t per_row, void* stream);
int dmh_sampler_step_ms_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                            float* hist, float* img_out, float* x_start, int64_t n, const uint8_t* keep, int64_t per_row,
                            void* stream);
/* The same step for the UNCONDITIONAL loop in one launch: dmh_sampler_step_ddp_dev without any noise source, draws table or
 * generator, plus hist [B][C][HW] as above; in place on img, x_start and xin_next (both optional) as there.  cursor: the step
 * cursor that goes with cur_dev (required like its neighbour's; the entry itself is *cur_dev). */
int dmh_sampler_step_ddp_ms_dev(const DmhStep* cur_dev, const int32_t* cursor, const float* model_out, float* img, float* hist,
                                float* x_start, float* xin_next, int B, int C, int HW, int cpad, int self_cond, void* stream);

/* Dynamic thresholding of x_start (Saharia et al. 2022, "Imagen", 2.3; not in the reference).
 *
 * dmh_row_quantile_abs: x [B][n] -> out[b] = max(floor, q_b), q_b the quantile of the n values |x[b][.]| at rank k + frac
 * with linear interpolation (torch.quantile's): v = the values sorted ascending, a = v[k]; frac == 0 or v[k+1] == a: q = a,
 * else q = fmaf(v[k+1] - a, frac, a) in fp32.  a and v[k+1] are the EXACT order statistics of the fp32 values (a radix select
 * on their bit patterns, integer counting only: bitwise repeatable).  A row that holds a NaN answers NaN.  The host turns a
 * percentile p into k = floor(p * (n - 1)), frac = float(p * (n - 1) - k), in double.  1 <= n < 2^31, 0 <= k < n, 0 <= frac < 1,
 * k + 1 < n where frac != 0.  One workgroup per row; no workspace.
 *
 * dmh_sampler_threshold[_dev]: for one denoise step (DmhStep by value, or read from device memory as dmh_sampler_step_dev
 * reads it) writes x0_raw [B][n] = the step's x_start before any clamp — the guided blend (model_null, keep as
 * dmh_sampler_step's, per_row = n) and the objective branch, the same statement the step kernels use — and thr [B] =
 * max(1, quantile of |x0_raw[b]|) through the selector above.  x0_raw is scratch the caller provides; two launches.
 *
 * dmh_sampler_step_thr[_dev]: dmh_sampler_step / dmh_sampler_step_ms with a threshold per row, thr [n / per_row]: where the
 * entry's clip is set, x_start = clamp(x0_raw, -thr, thr) / thr instead of clamp(x0_raw, -1, 1) (thr == 1: the same bits;
 * thr NaN: the row becomes NaN); with clip == 0 thr is not read.  Everything behind the clamp is the step as it stands.
 * noise (a DDIM entry, mode 0) and hist (a multistep entry, mode 3; read where c2 != 0, then overwritten with the new
 * x_start) are optional and exclude each other; mode 1 needs neither; the host-struct form refuses mode 2 and an entry
 * without the buffer it reads, the device-struct form answers NaN there.  img_out may alias x. */
int dmh_row_quantile_abs(const float* x, float* out, int B, int64_t n, int64_t k, float frac, float floor, void* stream);
int dmh_sampler_threshold(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                          const uint8_t* keep, float* x0_raw, float* thr, int B, int64_t n, int64_t k, float frac,
                          void* stream);
int dmh_sampler_threshold_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                              const uint8_t* keep, float* x0_raw, float* thr, int B, int64_t n, int64_t k, float frac,
                              void* stream);
int dmh_sampler_step_thr(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                         const float* noise, float* hist, const float* thr, float* img_out, float* x_start, int64_t n,
                         const uint8_t* keep, int64_t per_row, void* stream);
int dmh_sampler_step_thr_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                             const float* noise, float* hist, const float* thr, float* img_out, float* x_start, int64_t n,
                             const uint8_t* keep, int64_t per_row, void* stream);

/* Guidance rescale of the guided blend (Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps are Flawed", 3.4;
 * not in the reference).  Per row b of n values (one sample: n = C*H*W):
 *   mo_c[i] = model_cond[i], or model_null[i] where keep[b] == 0     (the conditional logit as dmh_sampler_step reads it)
 *   cfg[i]  = nl + (mo_c - nl) * cond_scale, nl = model_null[i]      (the fp32 expression of the guided blend, CFG:410)
 *   ratio   = std(mo_c) / std(cfg) over the row (population variance; only the ratio is used), 1 where std(cfg) == 0 (n == 1,
 *             constant rows)
 *   g[b]    = 1 + phi * (ratio - 1), rounded to fp32 once
 * and a step works on blend * g[b] instead of the blend.  A row whose cond equals its null bitwise gets g == 1.0f exactly (the
 * dropped rows of the conditional pass; a product with 1.0f is exact); a NaN or an infinity in a row makes that row's g NaN,
 * and no other row's.
 *
 * dmh_guidance_splits(B, n): the workgroups per row of the first pass, a pure function of (B, n); -1 for B < 1 or n outside
 * [1, 2^31).
 * dmh_guidance_factor[_dev]: gfac [B] <- g.  Only cond_scale is read from the DmhStep (by value, or from device memory as
 * dmh_sampler_step_dev reads it).  model_null is required (without a null pass there is nothing to rescale), 0 <= phi <= 1.
 * ws: workspace of the caller, 4 * B * dmh_guidance_splits(B, n) doubles.  Two launches: per (row, split) the fp64 mean and sum
 * of squared deviations of mo_c and of cfg into ws, then one thread per row merges them in split order.  No floating-point
 * atomics, no arrival counter: bitwise repeatable, and a row's g does not depend on the rows beside it.
 * dmh_sampler_threshold_gr[_dev]: dmh_sampler_threshold[_dev] on the rescaled blend (gfac [B]): x0_raw = the raw x_start of
 * blend * g[b], thr = max(1, its row quantile) through dmh_row_quantile_abs's selector.
 * dmh_sampler_step_gr[_dev]: one entry for DDIM, last and multistep entries on the rescaled blend.  gfac [n / per_row] is
 * required; noise, hist and thr are optional: noise and hist as dmh_sampler_step_thr's (they exclude each other; the
 * host-struct form refuses a DDIM entry without noise, a multistep entry without hist and mode 2), thr == NULL is the static
 * clamp of dmh_sampler_step, thr [n / per_row] the threshold of dmh_sampler_step_thr.  gfac == 1 gives the bits of
 * dmh_sampler_step / dmh_sampler_step_ms / dmh_sampler_step_thr.  img_out may alias x. */
int dmh_guidance_splits(int B, int64_t n);
int dmh_guidance_factor(const DmhStep* s, const float* model_cond, const float* model_null, const uint8_t* keep, float phi,
                        double* ws, float* gfac, int B, int64_t n, void* stream);
int dmh_guidance_factor_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const uint8_t* keep,
                            float phi, double* ws, float* gfac, int B, int64_t n, void* stream);
int dmh_sampler_threshold_gr(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                             const uint8_t* keep, const float* gfac, float* x0_raw, float* thr, int B, int64_t n, int64_t k,
                             float frac, void* stream);
int dmh_sampler_threshold_gr_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                                 const uint8_t* keep, const float* gfac, float* x0_raw, float* thr, int B, int64_t n,
                                 int64_t k, float frac, void* stream);
int dmh_sampler_step_gr(const DmhStep* s, const float* model_cond, const float* model_null, const float* x, const float* noise,
                        float* hist, const float* thr, const float* gfac, float* img_out, float* x_start, int64_t n,
                        const uint8_t* keep, int64_t per_row, void* stream);
int dmh_sampler_step_gr_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                            const float* noise, float* hist, const float* thr, const float* gfac, float* img_out,
                            float* x_start, int64_t n, const uint8_t* keep, int64_t per_row, void* stream);

/* Guidance interval (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and Distribution
 * Quality in Diffusion Models"; not in the reference): classifier-free guidance on a middle part of the sampling loop only.
 * An UNGUIDED entry is the entry at cond_scale == 1: the conditional pass alone, no blend.  In the replayed loop ONE captured
 * step serves both kinds: guided [S] (uint8, device; one flag per entry of the step table, written by the host in front of
 * every replay) is indexed by the step cursor of dmh_sampler_seek; both entry points read guided[*cursor] with one uniform
 * load.  A cursor outside [0, S) cannot be refused at launch (device data) and counts as a guided entry.
 *
 * dmh_rows_gated: dmh_rows_from_keep behind that flag — rows in the format of "Row subsets", int32 [1 + B + extra], ascending,
 * the slots behind 1 + n left unwritten.  keep: uint8 [B] or NULL (every row kept).
 *   null_side == 0 (the conditional pass, or both passes in one 2B-row launch with extra = B):
 *     guided entry    the slots b < B with keep[b] != 0 (all B where keep == NULL), then B .. B+extra-1
 *     unguided entry  ALL B slots and no extras: a dropped row has no null row to borrow from, so it is computed, under the
 *                     null embedding its keep bit already selects
 *   null_side == 1 (a null-only pass; keep is not read):
 *     guided entry    all B slots, then B .. B+extra-1;   unguided entry  n = 0
 * One workgroup.
 *
 * dmh_guidance_gate: behind the network.  Guided entry: returns before touching cond or null.  Unguided entry: null[0 .. n)
 * <- cond[0 .. n), bit for bit (NaN payloads and the sign of zero included; cond is never written), in 16-byte vectors where
 * cond and null meet 16-byte boundaries together, with a scalar head and tail, in 4-byte words otherwise.  cond and null must
 * not overlap.  Behind it every step kernel above does the unguided step unchanged: null + (cond - null) * s is cond where
 * null == cond, dmh_guidance_factor answers exactly 1, rows with keep == 0 read a null row that holds their own conditional
 * logits.  One difference to a call with model_null == NULL remains: the blend turns a logit of -0.0 into +0.0 (and an
 * infinite one into NaN), where the call without a null pass hands it on; equal values otherwise, torch.equal does not see
 * the zero. */
int dmh_rows_gated(const uint8_t* keep, int B, int extra, const int32_t* cursor, const uint8_t* guided, int S, int null_side,
                   int32_t* rows, void* stream);
int dmh_guidance_gate(const int32_t* cursor, const uint8_t* guided, int S, const float* cond, float* null, int64_t n,
                      void* stream);

/* Adaptive projected guidance, APG (Sadat, Hilliges, Weber 2024, "Eliminating Oversaturation and Artifacts of High Guidance
 * Scales in Diffusion Models", Algorithm 1; not in the reference): the guidance update cond - null is split into its parts
 * parallel and orthogonal to the conditional logits; the parallel part is down-weighted (eta), the update's norm is capped per
 * sample (rho, 0: no cap) and a negative-momentum average of the update runs over the steps (beta, 0: none).  Per row b of n
 * values (one sample: n = C*H*W):
 *   c[i] = model_cond[i], or model_null[i] where keep[b] == 0        (the conditional logit as dmh_sampler_step reads it)
 *   u[i] = model_null[i]
 *   d[i] = c[i] - u[i]                                               fp32
 *   beta != 0:  r[i] = d[i] + beta * r_prev[i]  (fp32, the product rounded before the sum; r_prev = 0 at the first step); d <- r
 *   Sdd = sum d^2, Sdc = sum d*c, Scc = sum c^2                      each product and the sums in fp64
 *   s   = 1 if rho == 0 or Sdd == 0, else min(1, rho / sqrt(Sdd))
 *   p   = 0 if Scc == 0, else Sdc / Scc                              (the projection of d on c)
 *   A[b]  = 1 - (w - 1) * s * (1 - eta) * p                          w = cond_scale; fp64, rounded to fp32 once
 *   Cc[b] = (w - 1) * s                                              fp64, rounded to fp32 once
 *   guided[i] = A[b] * c[i] + Cc[b] * d[i]                           fp32: two products and one add, no contraction
 * which is c + (w - 1) * s * (d_orth + eta * d_par).  With eta = 1, rho = 0, beta = 0 it is the guided blend in exact arithmetic,
 * not bit for bit.  A row whose cond equals its null bitwise has d == 0 at beta == 0: A == 1 and guided == c exactly (the dropped
 * rows of the conditional pass).  A row whose sums are not all finite (a NaN or an infinity in it) gets A = Cc = NaN, and no
 * other row does.  The guided logits are handed to dmh_sampler_step / _ms / _thr / dmh_sampler_threshold (and their _dev forms)
 * as model_cond with model_null == NULL: those do the plain step on them.
 *
 * dmh_apg_splits(B, n): the workgroups per row of the first pass, a pure function of (B, n); -1 for B < 1 or n outside
 * [1, 2^31).
 * dmh_apg_coef[_dev]: coef [2 * B] <- (A[b], Cc[b]) at coef[2 * b], coef[2 * b + 1].  Only cond_scale is read from the DmhStep (by
 * value, or from device memory as dmh_sampler_step_dev reads it).  model_null is required, 0 <= eta <= 1, rho >= 0 and finite,
 * |beta| < 1.  run [B * n]: the running average r, read and overwritten in place; required with beta != 0 and refused with beta
 * == 0; the caller zeroes it in front of the first step.  ws: workspace of the caller, 3 * B * dmh_apg_splits(B, n) doubles.  Two
 * launches: per (row, split) the three fp64 sums into ws (and run, each element by the thread that read it), 16-byte loads where
 * cond, null and run meet 16-byte boundaries together; then one thread per row adds them in split order.  No atomics, no
 * arrival counter: bitwise repeatable, and a row's coefficients do not depend on the rows beside it.
 * dmh_apg_apply: guided [B * n] <- A[b] * c + Cc[b] * d, d = run[i] where run != NULL (the r dmh_apg_coef just wrote), else c - u
 * again.  It reads no DmhStep (cond_scale sits in coef), so one entry serves the eager and the replayed loop.  guided must not
 * overlap model_cond, model_null or run. */
int dmh_apg_splits(int B, int64_t n);
int dmh_apg_coef(const DmhStep* s, const float* model_cond, const float* model_null, const uint8_t* keep, float eta, float rho,
                 float beta, float* run, double* ws, float* coef, int B, int64_t n, void* stream);
int dmh_apg_coef_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const uint8_t* keep, float eta,
                     float rho, float beta, float* run, double* ws, float* coef, int B, int64_t n, void* stream);
int dmh_apg_apply(const float* model_cond, const float* model_null, const uint8_t* keep, const float* run, const float* coef,
                  float* guided, int B, int64_t n, void* stream);

/* Photometric-consistency guidance (not in the reference's sampler): at every denoise step the predicted x_start is moved down
 * the gradient of the photometric energy of the training loss (CFG:782-806, squared form), with the weight the loss gives that
 * term.  Per sample, x [6][H][W] the blended logits (objective pred_x0: the x_start prediction; x[:3] is im1, x[3:] im2):
 *   c = model_cond, or model_null where keep[b] == 0;  x = c where model_null == NULL, else null + (c - null) * cond_scale
 *                                                       (the device function of the step kernels, csrc/sampler_dev.h)
 *   w_p(q): the bilinear weights of dmh_flow_warp(pad border, mode bilinear) for the pixel p moved by flow(p): the sample point
 *           clamped to the image, its four taps, a tap one past the last row / column dropped
 *   u[c,p]   = sum_q w_p(q) * x[3+c,q]                       fp32, the fma chain of dmh_flow_warp (im2 warped to im1's frame)
 *   r[c,p]   = mask[p] * (u[c,p] - x[c,p])                   fp32
 *   s[q]     = sum_p mask[p] * w_p(q)                        (flow and mask only: dmh_photo_weights, once per sampling call)
 *   lambda   = w * (sqrt_ac * sqrt_ac)                       fp32, from the DmhStep: w * alphas_cumprod[t], the loss's weight
 *   y[c,p]   = x[c,p]   + (lambda / 2) * r[c,p]
 *   y[3+c,q] = x[3+c,q] - (lambda / 2) * ((sum_p w_p(q) * r[c,p]) / max(1, s[q]))
 *   E        = (1 / (3 H W)) * sum_{c,p} mask[p] * (u[c,p] - x[c,p])^2      float64 (u too), per sample
 * Where r (resp. the sum) is 0 the logit is handed on bit for bit.  With D = diag(1 / max(1, s)) and A = M^1/2 W D^1/2, the rows
 * of W summing to at most 1 give |A v|^2 <= sum_q d_q s_q v_q^2 <= |v|^2: the preconditioned Hessian has norm <= 2 and the step
 * lowers E for every flow and every lambda in (0, 1] (without the division it diverges where many pixels sample one target).
 *
 * Summation.  The two scatters (s, and sum_p w_p(q) * r) add with 64-bit INTEGER atomics in Q31.32 fixed point, so a launch's
 * result does not depend on the order in which workgroups run and is bitwise repeatable.  A contribution v (an fp32 product) is
 * rint(clamp(v, -2^30, 2^30) * 2^32); a NaN contributes 0 (it still shows in y[c,p] of its own pixel).  Exact to 2^-33 per
 * contribution while sum |v| < 2^31 at a target; beyond that the sum wraps (defined, and wrong).
 *
 * dmh_photo_acc_words(B, H, W): the 64-bit words of the accumulator, 3 * B * H * W; -1 for sizes the entries refuse.  acc is the
 * caller's, ZERO in front of the first call; every entry that uses it leaves it zero (the pass that finishes im2, resp. s, zeroes
 * what it read), so a sampling loop needs no memset.
 * dmh_photo_weights: s [B][H][W] from flow [B][2][H][W] and mask [B][1][H][W].  Two launches.
 * dmh_photo_guide[_dev]: guided [B][6][H][W] <- y.  cond_scale and sqrt_ac are read from the DmhStep (by value, or from device
 * memory as dmh_sampler_step_dev reads it) and nothing else.  model_null and keep may be NULL (keep needs model_null); 0 < w <= 1;
 * guided must not overlap model_cond or model_null.  Two launches: one thread per pixel p (blend, warp, residual, y[:3], scatter),
 * then one per element of im2.  The guided logits go to dmh_sampler_step / _ms / _thr / dmh_sampler_threshold as model_cond with
 * model_null == NULL.
 * dmh_photo_energy: E [B] (float64) of any x [B][6][H][W].  ws: dmh_photo_energy_splits(B, H, W) * B doubles.  Two launches: fp64
 * partial sums per (sample, split) in a fixed order, then one thread per sample adds them in split order.  No atomics.
 * Every entry: B in [1, 65535], H >= 2 and W >= 2 (the warp divides by W - 1), H * W <= 2^24. */
int64_t dmh_photo_acc_words(int B, int H, int W);
int dmh_photo_energy_splits(int B, int H, int W);
int dmh_photo_weights(const float* flow, const float* mask, uint64_t* acc, float* s, int B, int H, int W, void* stream);
int dmh_photo_guide(const DmhStep* s, const float* model_cond, const float* model_null, const uint8_t* keep, const float* flow,
                    const float* mask, const float* sw, float w, uint64_t* acc, float* guided, int B, int H, int W, void* stream);
int dmh_photo_guide_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const uint8_t* keep,
                        const float* flow, const float* mask, const float* sw, float w, uint64_t* acc, float* guided, int B, int H,
                        int W, void* stream);
int dmh_photo_energy(const float* x, const float* flow, const float* mask, double* ws, double* E, int B, int H, int W,
                     void* stream);

/* Guidance on the homography condition, flow_guidance (not in the reference; the two-scale form of InstructPix2Pix, Brooks,
 * Holynski, Efros 2023, with the flow in the image condition's place and the class in the text's).  The condition rgb_flow * mask
 * enters the network through three stem channels only.  A "no-flow" pass is the network on the same x, time and mask with those
 * three channels exactly +0.0.  flow_guidance = s_f is a finite number >= 0, w = s_f - 1 (computed on the host, passed as a
 * float).  Per element i of row b (one sample: n = C*H*W):
 *   case A, cond_scale != 1, three passes:  c = class kept by the drawn mask keep, with flow (the conditional pass);
 *            n = null class, with flow (the null pass);  u = null class, no flow
 *     e[i] = w * (n[i] - u[i])                                        fp32: the difference rounded, then the product
 *     model_null[i] <- n[i] + e[i]
 *     model_cond[i] <- c[i] + e[i]      on the rows the conditional pass computed (keep == NULL or keep[b] != 0); the other rows
 *                                       of model_cond are neither read nor written
 *   case B, cond_scale == 1, two passes:  c = the single pass with its class-dropout draw;  u = the SAME keep bits, no flow
 *     e[i] = w * (c[i] - u[i]);   model_cond[i] <- c[i] + e[i]        = u + s_f * (c - u) in exact arithmetic
 * In case A the blend of the step kernels, null' + (cond' - null') * s_c, is u + s_f * (n - u) + s_c * (c - n) in exact
 * arithmetic, and cond' - null' is c - n up to rounding: the rescale, APG, the thresholds, the photometric correction and both
 * samplers work on the shifted logits unchanged.  No random draw is added: the keep mask is drawn once, where it is drawn
 * without the switch, and in case B it serves both passes.  w == 0 leaves every value (e is a zero), a sample whose stem
 * channels are +0.0 already has n == u (c == u) bitwise and is left as it is.
 *
 * dmh_flow_guidance_shift: in place, one launch.  model_null != NULL: case A; model_null == NULL: case B, keep must be NULL.  It
 * reads no DmhStep, so one entry serves the eager and the replayed loop.  16-byte loads and stores where model_cond, model_null
 * and uncond meet 16-byte boundaries together (scalar head and tail; a vector that crosses a row boundary takes each element
 * under its own row's keep bit), 4-byte words otherwise; a grid-stride loop, no LDS, no atomics: bitwise repeatable.  uncond must
 * not overlap model_cond or model_null, model_cond not model_null; B >= 1, 1 <= n < 2^31, w finite.
 * dmh_affine_rows_keep: y[i] = keep[b] != 0 ? x[i] * scale + shift : +0.0f — dmh_affine's arithmetic on kept rows (a dropped
 * row's x is not read); the training side's normalisation of rgb_flow and the drop of flow_drop_prob in one launch.  y must not
 * overlap x. */
int dmh_flow_guidance_shift(float* model_cond, float* model_null, const float* uncond, const uint8_t* keep, float w, int B,
                            int64_t n, void* stream);
int dmh_affine_rows_keep(const float* x, float* y, float scale, float shift, const uint8_t* keep, int B, int64_t n, void* stream);

/* Perturbed-attention guidance, pag_scale (not in the reference; Ahn et al. 2024, "Self-Rectifying Diffusion Sampling with
 * Perturbed-Attention Guidance").  It needs no label, no null class and no retraining.
 * The perturbed pass p is the conditional pass — same x, same time, same rgb_flow * mask, same class-keep bits — with one change:
 * in mid_attn (the UNet's one full self-attention, K4) softmax(q k^T) is replaced by the identity matrix, so the attention
 * core's output is v itself:
 *     out[b][pix][h*32 + e] = qkv[b][pix][256 + h*32 + e]        exactly
 * to_qkv, to_out, the pre-norm and the residual around it are unchanged, and so are the LinearAttention blocks (they have no
 * attention map to replace).
 * The shift, per element i of row b (one sample: n = C*H*W), with s = pag_scale >= 0, in fp32 without contraction:
 *     c[i] = model_cond[i] where the conditional pass computed row b (keep == NULL or keep[b] != 0), else model_null[i]
 *     d = c[i] - p[i] (rounded);   e = s * d (rounded)
 *   case A, a null pass exists (cond_scale != 1):  model_null[i] <- model_null[i] + e
 *                                                  model_cond[i] <- model_cond[i] + e   where row b was computed; the other rows
 *                                                  of model_cond are neither read nor written
 *   case B, no null pass (cond_scale == 1):        model_cond[i] <- c[i] + e
 * In exact arithmetic the blend null' + (cond' - null') * cond_scale of the step kernels behind it is
 * n + cond_scale * (c - n) + s * (c - p); no kernel behind the shift knows about it (flow_guidance uses the same trick), and
 * because the update is linear it is the paper's epsilon-space formula under every objective.  s == 0 leaves every value (e is a
 * zero), c == p leaves every value bitwise.  No random draw is added.
 *
 * dmh_attention_pag: dmh_attention in which every wave whose physical row b (behind the row list) is >= pert_lo takes the
 * identity arm: lane (i, half) of the wave of (b, head h, queries q0 .. q0 + 31) copies the 16 floats v[q0 + i][h*32 + 16*half ..]
 * with 16-byte loads and stores where q0 + i < n, and retires before any q / k load.  The condition is uniform over a wave and
 * the kernel has no barrier.  0 <= pert_lo <= B; pert_lo == B perturbs nothing and is bitwise dmh_attention.
 * dmh_pag_shift: in place, one launch.  model_null != NULL: case A; model_null == NULL: case B, keep must be NULL.  It reads no
 * DmhStep, so one entry serves the eager and the replayed loop.  16-byte loads and stores where model_cond, model_null and pert
 * meet 16-byte boundaries together (scalar head and tail; a vector that crosses a row boundary takes each element under its own
 * row's keep bit), 4-byte words otherwise; a grid-stride loop, no LDS, no atomics: bitwise repeatable.  pert must not overlap
 * model_cond or model_null, model_cond not model_null; B >= 1, 1 <= n < 2^31, s finite and >= 0. */
int dmh_attention_pag(const float* qkv, float* out, int B, int n, float scale, const int32_t* rows, int pert_lo, void* stream);
int dmh_pag_shift(float* model_cond, float* model_null, const float* pert, const uint8_t* keep, float s, int B, int64_t n,
                  void* stream);

/* Noise of the sampling loop keyed by GLOBAL sample index: replaces torch.randn(shape) CFG:679,
 * torch.randn_like(img) CFG:705 and torch.zeros(B).uniform_(0, 1) CFG:90 where a run is sharded over ranks.
 * out [B][per_sample]: element e of row b = f(seed, sample_ids[b], draw, e) with f = Philox4x32-10 (key = seed, counter =
 * (e / 4, draw, sample id lo, hi)) followed by Box-Muller (kind 0: N(0,1)), the top 24 bits * 2^-24 (kind 1: uniform
 * [0,1)) or nothing (kind 2: the raw 32-bit words as float bit patterns, for known-answer tests) — so any row is the
 * same whichever rank, batch size or row position computes it.
 * state: 4 x uint64 in DEVICE memory: [0] seed, [1] draw index — read by every workgroup, advanced by one by the last
 * workgroup of the launch to finish, so a captured launch replays with the next draw —, [2] arrival tickets (0 between
 * launches), [3] reserved.  sample_ids: [B] int64. */
int dmh_rng_indexed(float* out, int B, int64_t per_sample, const int64_t* sample_ids, uint64_t* state, int kind,
                    void* stream);

/* prob_mask_like CFG:84-90 on the indexed generator in one launch: keep[b] = (the kind-1 uniform of row b at the current
 * draw) < prob, uint8; advances the draw index by one (it IS that draw) */
int dmh_rng_keep_mask(uint8_t* keep, int B, const int64_t* sample_ids, uint64_t* state, float prob, void* stream);

/* y = x*scale + shift elementwise (normalize / unnormalize, CFG:69-74) */
int dmh_affine(const float* x, float* y, float scale, float shift, int64_t n, void* stream);
/* in place on channels >= c0 of an NCHW tensor: x = x*scale + shift (flow channel remap, DDP:679,728) */
int dmh_affine_tail(float* x, int B, int C, int HW, int c0, float scale, float shift, void* stream);
/* D4 / D7 with a timestep per row: out = ca[b]*x (+ cb[b]*y) (/ dv[b]) (clamped to [-1,1] when clamp != 0); y, cb, dv may be
 * NULL.  predict_start_from_noise / predict_noise_from_start / predict_v / predict_start_from_v CFG:586-601, the posterior
 * mean of q_posterior CFG:603-608 and the optional clamp of model_predictions CFG:612, in the reference's op order */
int dmh_rows_lincomb(const float* x, const float* y, const float* ca, const float* cb, const float* dv, float* out, int B,
                     int64_t per_sample, int clamp, void* stream);
/* D9 q_sample CFG:738-742: out = ca[b]*x_start + cb[b]*noise, ca/cb = extract(sqrt_ac / sqrt_1m_ac, t) */
int dmh_q_sample(const float* x_start, const float* noise, const float* ca, const float* cb, float* out, int B,
                 int64_t per_sample, void* stream);
/* D9 loss terms of p_losses (CFG:796-806), forward value only:
 *   out[b] = mean over (C,HW) of m[b][hw] * |a - b|   (squared != 0: (a - b)^2); m may be NULL.
 * Deterministic two-stage reduction; ws: [B][64] f64 scratch. */
int dmh_diff_mean(const float* a, const float* b, const float* m, int squared, double* ws, float* out, int B, int C,
                  int HW, void* stream);
/* loss.mean() + (w * photo).mean() over the B per-sample means (CFG:804-806) -> out[0] */
int dmh_loss_combine(const float* l, const float* photo, const float* w, float* out, int B, void* stream);
/* G6  saveTrainPair DDP:1673: uint8 truncation of img*255 */
int dmh_to_uint8(const float* img, uint8_t* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------
 * K7-K9  condition builder & geometry
 * ------------------------------------------------------------------------------------- */
/* G2+G3  homo_to_flow DDP:927-975 + flow_to_image DDP:1471-1486.  Hm: [B][9] f64 (device);
 * flow NCHW [B][2][H][W] fp32, rgb NCHW [B][3][H][W] fp32 (either may be NULL) */
int dmh_homography_flow(const double* Hm, float* flow, float* rgb, int B, int H, int W, float max_flow,
                        void* stream);
/* G3 alone: flow NCHW [B][2][HW] -> rgb NCHW [B][3][HW] (flow_to_image DDP:1471-1486) */
int dmh_flow_to_image(const float* flow, float* rgb, int B, int HW, float max_flow, void* stream);
/* G4  flow_warp DDP:1262-1299 (grid_sample, align_corners=True); x/out NCHW [B][C][H][W], flow [B][2][H][W].
 * pad: 0 'border' (the reference's default), 1 'zeros', 2 'reflection'; mode: 0 'bilinear' (default), 1 'nearest', 2 'bicubic' — the
 * values flow_warp forwards to grid_sample's padding_mode / mode (DDP:1262,1270-1274).
 * x0/y0 (NULL or int32 [B][H][W]; pad == 0 && mode == 0 only) receive the top-left corner indices (bit-exact contract). */
int dmh_flow_warp(const float* x, const float* flow, float* out, int32_t* x0, int32_t* y0, int B, int C, int H,
                  int W, int pad, int mode, void* stream);
/* get_grid DDP:1558-1574: out (B,2,H,W) fp32 = (x + start, y + start) of every pixel */
int dmh_pixel_grid(float* out, int B, int H, int W, float start, void* stream);
/* norm_grid DDP:1292-1299: v (B,2,H,W) -> out (B,H,W,2) = (2.0*v_x/(W-1) - 1.0, 2.0*v_y/(H-1) - 1.0), fp32, that op order */
int dmh_norm_grid(const float* v, float* out, int B, int H, int W, void* stream);
/* get_flow_np DDP:927-969 in its general form: Hm (B,divide,3,3) f64 — row y uses band min(y / (H/divide), divide-1) —,
 * idx (Bi,3,H,W) f64 homogeneous coordinates (Bi == B or 1: mesh_grid_np), flow (B,2,H,W) f64 = H.p / (w' + 1e-6) - p */
int dmh_homography_flow_points(const double* Hm, const double* idx, double* flow, int B, int divide, int Bi, int H, int W,
                               void* stream);
/* DLT_solve DDP:1612-1643 on explicit correspondences: src, off (N,P,2) f64 -> Hout (N,3,3) f64, one least-squares
 * homography per system (P == 4: the square system solved directly; P > 4: f64 normal equations as dmh_dlt_homography);
 * ws: [N][DMH_DLT_BLOCKS][44] f64 (unused for P == 4) */
int dmh_dlt_points(const double* src, const double* off, double* ws, double* Hout, int N, int P, void* stream);
/* G5  homo_gen / DLT_solve DDP:1577-1661 through f64 normal equations; ws: [B][DMH_DLT_BLOCKS][44] f64 */
#define DMH_DLT_BLOCKS 64
int dmh_dlt_homography(const float* flow, double* ws, double* Hout, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training: the pieces of loss.backward() / clip_grad_norm_ / Adam.step / ema.update (DDP:1843-1865);
 * dmhomo_amd/train.py strings them into the optimiser step.
 * ------------------------------------------------------------------------------------- */

/* weight / bias gradient of a stride-1 KHxKH convolution, i.e. autograd of F.conv2d (CFG:128) wrt weight and bias:
 *   dw[o][c][ky][kx] = sum dy[b][y][x][o] * X[b][y+ky-p][x+kx-p][c],  db[o] = sum dy[b][y][x][o],
 * X = cat(src0, src1) with the optional consumer-side prologue X = SiLU(a*src0 + b) of dmh_conv2d.
 *   KH = 1, 3, 7: 'same' conv (p = KH/2); ups = 1 (KH = 3): the conv saw the nearest x2 upsampling of the stored
 *                 input [B][H/2][W/2][C0] (Upsample, CFG:106-107);
 *   KH = 2      : 'valid' 2x2 conv (p = 0) over a stored input [B][H+1][W+1][C0] — the space-to-depth form
 *                 (dmh_s2d_shift) of the 4x4 / stride-2 Downsample conv (CFG:110-111).
 * KH = 2, 3: fp16 pieces of both operands on the fp16 matrix cores, fp32 accumulate (error at the fp32-accumulation
 * level); KH = 1, 7: exact fp32 (v_mfma_f32_16x16x4_f32).  Deterministic
 * (pixel splits reduced in a fixed order).  The DATA gradient is
 * dmh_conv2d itself on dy with the weight flipped in both taps and transposed in (Cout, Cin).
 * dy: NHWC [B][H][W][Cout]; dw: OIHW [Cout][C0+C1][KH][KH]; db: [Cout] or NULL; work: ..._workspace_floats floats. */
int64_t dmh_conv_wgrad_workspace_floats(int B, int H, int W, int C0, int C1, int Cout, int KH);
int dmh_conv_wgrad(const float* dy, const float* src0, const float* src1, const float* in_coef, float* dw, float* db,
                   float* work, int B, int H, int W, int C0, int C1, int Cout, int KH, int ups, void* stream);
/* weight / bias gradient of the DDP Downsample, pixel-unshuffle + 1x1 (DDP:110-113), with W22 = weight.reshape(Cout, C, 2, 2):
 *   dw[o][c*4 + py*2 + px] = sum_{b,y,x} dy[b][y][x][o] * x[b][2y+py][2x+px][c],  db[o] = sum dy[b][y][x][o]
 * x: the stored NHWC input [B][H][W][C] (H, W even), read in place (no space-to-depth copy); dy [B][H/2][W/2][Cout];
 * dw [Cout][4C] (the reference's (Cout, 4C, 1, 1)); db [Cout] or NULL; work: ..._workspace_floats floats (-1: bad sizes).
 * The contract of dmh_conv_wgrad's KH = 1: exact fp32 (v_mfma_f32_16x16x4_f32), pixels as K split over workgroups, the
 * splits reduced in a fixed order (deterministic).  C, Cout multiples of 4.  The DATA gradient is the 1x1 dmh_conv2d of dy
 * with W22 transposed to [(py*2+px)*C + c][Cout] followed by dmh_d2s. */
int64_t dmh_conv_unshuffle_wgrad_workspace_floats(int B, int H, int W, int C, int Cout);
int dmh_conv_unshuffle_wgrad(const float* dy, const float* x, float* dw, float* db, float* work, int B, int H, int W, int C,
                             int Cout, void* stream);
/* layout helpers of the strided / upsampled convs' backward:
 *   dmh_s2d_shift  X[b][cy][cx][(py*2+px)*C + c] = x[b][2cy-1+py][2cx-1+px][c] (0 outside), [B][H/2+1][W/2+1][4C]
 *   dmh_d2s        out[b][2m+ry][2l+rx][c] = in[b][m][l][(ry*2+rx)*C + c]        [B][H][W][4C] -> [B][2H][2W][C]
 *   dmh_sumpool2   out[b][m][l][c] = sum of the 2x2 block of in                  [B][2H][2W][C] -> [B][H][W][C] */
int dmh_s2d_shift(const float* x, float* X, int B, int H, int W, int C, void* stream);
int dmh_d2s(const float* in, float* out, int B, int H, int W, int C, void* stream);
int dmh_sumpool2(const float* in, float* out, int B, int H, int W, int C, void* stream);

/* dmh_gn_finalize that also saves (mean, rstd) per (sample, group) for the backward pass: mr [B][groups][2] */
int dmh_gn_finalize_train(const float* stats, int tiles, const float* gamma, const float* beta, const float* ss,
                          int64_t ss_stride, float* coef, float* mr, int B, int C, int groups, int hw, float eps,
                          void* stream);

/* backward of Block's GroupNorm -> (scale+1, shift) -> SiLU (CFG:206-212) given the conv output y it normalised:
 *   dout: gradient wrt SiLU(GN(y)...) [B][HW][C];  y, coef [B][2][C], mr [B][groups][2]: as seen / saved by the forward;
 *   dy [B][HW][C];  pg [B][4][C]: per-sample parts of (dgamma, dbeta) — add them over b with dmh_sum_over_batch — and
 *   (d scale, d shift) of the ResnetBlock mlp output;  part [B][dmh_gn_bwd_chunks(HW)][C][2], bcoef [B][3][C]: work. */
int dmh_gn_bwd_chunks(int HW);
int dmh_gn_silu_backward(const float* dout, const float* y, const float* coef, const float* mr, const float* gamma,
                         const float* beta, const float* ss, int64_t ss_stride, float* dy, float* pg, float* part,
                         float* bcoef, int B, int HW, int C, int groups, void* stream);
/* out[i] = sum_b in[b][i], i < per (fixed order) */
int dmh_sum_over_batch(const float* in, float* out, int B, int64_t per, void* stream);
/* backward of the weight standardisation CFG:120-126: dw from the gradient dwh wrt the standardised weight. [Cout][K] */
int dmh_ws_backward(const float* w, const float* dwh, float* dw, int Cout, int K, float eps, void* stream);

/* backward of the channel LayerNorm N4 (CFG:137-141): dx [npix][C] and dmh_lnb_blocks() partial rows of dg
 * (dg_part [blocks][C]; add them with dmh_sum_over_batch).  d res = dout when the forward added a residual. */
int dmh_lnb_blocks(void);
int dmh_chan_layernorm_backward(const float* x, const float* g, const float* dout, float* dx, float* dg_part,
                                int64_t npix, int C, float eps, void* stream);

/* backward of the LinearAttention core (CFG:258-269) on a stored qkv [B][n][384]:  forward with dmh_linattn_context,
 * dmh_linattn_merge_ms (saves ms [B][4][32][2], the softmax-over-n statistics of k), dmh_linattn_apply;  then
 * dmh_linattn_backward(dout [B][n][128]) -> dqkv [B][n][384].  work: dmh_linattn_bwd_workspace_floats(B, n) floats. */
int dmh_linattn_merge_ms(const float* partial, float* ctx, float* ms, int B, int n, void* stream);
int64_t dmh_linattn_bwd_workspace_floats(int B, int n);
int dmh_linattn_backward(const float* qkv, const float* ctx, const float* ms, const float* dout, float* dqkv, float* work,
                         int B, int n, float scale, void* stream);

/* small strided batched fp32 GEMM (exact fp32 MFMA) for the backward pass: C[bo][bi] = alpha * A[bo][bi] (MxK) * B[bo][bi]
 * (KxN); sa / sb / sc: HOST arrays of 4 strides in floats {outer batch, inner batch, row, column}.  Row softmax and its
 * backward (dP <- P * (dP - sum_j dP*P), in place) for the bottleneck Attention (CFG:287-295). */
int dmh_bgemm(const float* A, const int64_t* sa, const float* B, const int64_t* sb, float* C, const int64_t* sc, int M,
              int N, int K, int nbo, int nbi, float alpha, void* stream);
int dmh_softmax_rows(const float* S, float* P, int64_t rows, int n, void* stream);
int dmh_softmax_rows_backward(const float* P, float* dP, int64_t rows, int n, void* stream);

/* elementwise SiLU (mode 1) / exact GELU (mode 2): dy == NULL -> out = f(x), else out = dy * f'(x) */
int dmh_act(const float* x, const float* dy, float* out, int64_t n, int mode, void* stream);
/* backward of the class embedding lookup + null-class select (CFG:419-425): d [B][D] -> dtable [num_classes][D], dnull [D];
 * keep: uint8 [B] (the mask drawn in the forward) */
int dmh_class_embed_backward(const float* d, const int64_t* classes, const unsigned char* keep, float* dtable, float* dnull,
                             int B, int D, int num_classes, void* stream);
/* gradient of p_losses (CFG:796-806) wrt the UNet output: out, target [B][6][H][W]; warped = flow_warp(out[:,3:6], flow)
 * [B][3][H][W]; mask [B][1][H][W]; abar [B] = alphas_cumprod[t]; squared: 0 L1, 1 L2.  dout [B][6][H][W]; gD [B][3][H][W]
 * work.  The transpose of the bilinear gather uses float atomics (order not fixed where the flow field folds). */
int dmh_loss_backward(const float* out, const float* target, const float* warped, const float* mask, const float* flow,
                      const float* abar, float* dout, float* gD, int B, int H, int W, int squared, void* stream);
/* gradient of the unconditional p_losses (DDP:804-811) wrt the UNet output: out, target NCHW [B][per] (per = C*H*W);
 * w [B] = p2_loss_weight[t];  dout = scale * w[b] * g(out - target) / (B * per), g = sign (L1, sign(0) = 0; squared = 0) or
 * 2 d (L2; squared = 1); scale: 1 / accum of gradient accumulation. */
int dmh_loss_backward_ddp(const float* out, const float* target, const float* w, float* dout, int B, int64_t per, int squared,
                          float scale, void* stream);
/* optimiser (DDP:1852-1862): per-tensor partial sums of squares (f64 [dmh_sumsq_blocks()] each) -> global norm and clip
 * coefficient (norm_out[0], norm_out[1] = min(1, max_norm / (norm + 1e-6))) -> Adam with the gradient scaled by
 * gscale[1] (torch.optim.Adam, no weight decay) -> EMA lerp */
int dmh_sumsq_blocks(void);
int dmh_sumsq(const float* g, int64_t n, double* part, void* stream);
int dmh_gradnorm_finalize(const double* part, int n, float max_norm, float* norm_out, void* stream);
int dmh_adam(float* p, const float* g, float* m, float* v, const float* gscale, int64_t n, float lr, float b1, float b2,
             float eps, int step, void* stream);
int dmh_ema(float* ema, const float* p, int64_t n, float decay, void* stream);
/* multi-tensor forms of the two above: p / g / m / v / n are HOST arrays of ``count`` device pointers / element counts
 * (the ~280 parameter tensors of the UNet go out in count/48 launches); part: f64 [dmh_multi_blocks(n, count)], to be
 * reduced by dmh_gradnorm_finalize */
int64_t dmh_multi_blocks(const int64_t* n, int count);
int dmh_sumsq_multi(const float* const* g, const int64_t* n, int count, double* part, void* stream);
int dmh_adam_multi(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int count,
                   const float* gscale, float lr, float b1, float b2, float eps, int step, void* stream);


/* ---------------------------------------------------------------------------------------
 * condition dataset path: UnHomoTrainData.__getitem__ DDP:1097-1163, a batch per launch
 * ------------------------------------------------------------------------------------- */
/* cv2.resize(img.astype(float32) / div, (Wd, Hd)) with INTER_LINEAR (DDP:1118-1123): src [B][Hs][Ws][C] uint8 interleaved
 * (as decoded), dst plane c of image b at dst + b*dst_bstride + c*Hd*Wd (the batch tensor's own planes) */
int dmh_resize_bilinear_u8(const unsigned char* src, float* dst, int B, int Hs, int Ws, int C, int Hd, int Wd,
                           int64_t dst_bstride, float div, void* stream);
/* cv2.dilate(cv2.erode(cv2.resize(mask, (Wd, Hd), INTER_NEAREST), ones(3,3)), ones(3,3)) (DDP:1129-1133):
 * src [B][Hs][Ws] fp32, dst plane of image b at dst + b*dst_bstride */
int dmh_mask_open_nearest(const float* src, float* dst, int B, int Hs, int Ws, int Hd, int Wd, int64_t dst_bstride,
                          void* stream);

/* ---------------------------------------------------------------------------------------
 * sample preview sheets (DDP:1489-1555; written by Trainer.train / Trainer.sample, DDP:1871-1935, 1972-2019)
 * ------------------------------------------------------------------------------------- */
/* postProcess DDP:1505-1517 in one launch: img [B][6][H][W], mask [B][1][H][W], flow [B][2][H][W] fp32 ->
 * buf1 = [img1 | img1 | mask x3 | flow_vis], buf2 = [img2 | flow_warp(img2, flow) | mask x3 | flow_vis], each [B][3][H][4W].
 * The warp panel is bit for bit the default (border, bilinear) flow warp above, the flow panel the flow-to-image kernel
 * with max_flow = 256. */
int dmh_post_process(const float* img, const float* mask, const float* flow, float* buf1, float* buf2, int B, int H, int W,
                     void* stream);
/* the same panels fused with the reference's channel swap [:, [2,1,0]] (bgr != 0), torchvision's make_grid(nrow, padding,
 * pad_value = 0) and save_image's quantisation (x*255 + 0.5 in two roundings, clamp to [0, 255], truncate): two uint8
 * sheets [Hs][Ws][3], 4-byte aligned.  xmaps = min(nrow, B), ymaps = ceil(B / xmaps), Hs = ymaps*(H+padding)+padding,
 * Ws = xmaps*(4W+padding)+padding; B == 1: the image alone, Hs = H, Ws = 4W. */
int dmh_preview_sheet(const float* img, const float* mask, const float* flow, unsigned char* sheet1, unsigned char* sheet2,
                      int B, int H, int W, int nrow, int padding, int bgr, void* stream);
/* cv2.warpPerspective(src, M, (Wd, Hd)) without the inverse-map flag (DDP:1527): src [B][3][H][W] fp32, homos [B][3][3]
 * float64 -> dst [B][3][Hd][Wd], dst(x, y) = src(M^-1 (x, y, 1)), bilinear, constant border 0 per neighbour.  Deliberate
 * deviation: the EXACT bilinear result (inverse, coordinates, weights in float64; one rounding to fp32), not cv2's
 * fixed-point coefficient tables (fraction quantised to 1/32). */
int dmh_homography_warp(const float* src, const double* homos, float* dst, int B, int H, int W, int Hd, int Wd, void* stream);

/* ---------------------------------------------------------------------------------------
 * HEM training batches from sampled pairs: DGMTrainData.__getitem__ / data_aug, HEM/dataset/data_loader.py:121-255,
 * a batch per launch (dmhomo_amd/hem_data.py)
 * ------------------------------------------------------------------------------------- */
/* img12 uint8 [B][6][h][w] (a saveTrainPair record, channel-planar); homo, homo_inv f64 [B][9] (device): the forward
 * homography at the output size and its inverse; start int32 [B][2] (device): the crop's (x, y); mean, std: HOST f64 [3].
 * (h, w) != (H, W): both images are resized with cv2's 8-bit INTER_LINEAR arithmetic (integer, bit-exact), else taken as is.
 * Outputs fp32, as the reference's collated batch:
 *   imgs_gray_full [B][2][H][W]  channel mean of (u8 - mean) / std in float64
 *   imgs_rgb_full  [B][6][H][W]  u8 / 255
 *   flow_gt_full   [B][4][H][W]  planes 0-1 dmh_hem_flow of homo_inv, planes 2-3 of homo
 *   imgs_gray_patch [B][2][ph][pw], flow_gt_patch [B][4][ph][pw]: bit for bit the window [y:y+ph, x:x+pw] of the full tensors.
 * A start outside [0, W-pw] x [0, H-ph] is device data: that sample's patch tensors are filled with NaN, nothing is read or
 * written out of bounds.  The full-size outputs must be 16-byte aligned. */
int dmh_hem_batch(const unsigned char* img12, const double* homo, const double* homo_inv, const int32_t* start,
                  const double* mean, const double* std, int B, int h, int w, int H, int W, int ph, int pw,
                  float* imgs_gray_full, float* imgs_rgb_full, float* flow_gt_full, float* imgs_gray_patch,
                  float* flow_gt_patch, void* stream);
/* homo_convert_to_flow (data_loader.py:42-52) alone: homo f64 [B][9] (device) -> flow fp32 [B][2][H][W] (16-byte aligned),
 * flow = fp32(H.(x, y, 1) / (w' + 1e-8)) - fp32(x, y), the mapping in float64 */
int dmh_hem_flow(const double* homo, int B, int H, int W, float* flow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMHOMO_HIP_H */
