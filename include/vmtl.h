/* vmtl.h — C ABI of libvmtl.so: the MI355X (gfx950) kernels behind the
 * vision_mtl multi-task dense-prediction training step.
 *
 * The reference (kirilllzaitsev/vision_mtl) has no FFI of its own: its "operator
 * API" for this path is torch.nn.Module.forward + autograd reaching ATen.  Each
 * entry point below therefore cites the reference call site (file:line, relative
 * to the reference repo root) whose ATen dispatch it replaces.  INTEGRATION.md
 * shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory (HBM) unless noted.
 *  - activations are NHWC fp32, [B][H][W][Cs], Cs = round_up(C,4); channels [C,Cs) are 0.
 *  - `stream` is a hipStream_t (void*); nothing here allocates, frees or synchronises,
 *    so every call can be captured into a hipGraph.
 *  - return 0 on success, <0 on error (never throws): -1 bad argument, -2 launch
 *    failure, -3 unsupported configuration.
 */
#ifndef VMTL_H
#define VMTL_H

#ifdef __cplusplus
extern "C" {
#endif

#define VMTL_ACT_NONE 0
#define VMTL_ACT_RELU 1
#define VMTL_ACT_HSWISH 2
#define VMTL_ACT_HSIGMOID 3
#define VMTL_ACT_SIGMOID 4

/* operand precision of the implicit-GEMM convolutions and the pointwise GEMMs (the *_p entry points below; their
 * namesakes without the suffix are VMTL_PREC_FP32).  VMTL_PREC_BF16: every product term is bf16(a)*bf16(b)
 * (round-to-nearest-even, NaN stays NaN), accumulated in fp32; tensors in memory, epilogues (bias, activation, statistics,
 * BatchNorm backward and its addend) stay fp32.  Tile choice, K split, persistent-program count, statistics layout and
 * weight-gradient slab counts do not depend on it.  Unknown values: -1, checked before anything else.  The value is per
 * call: which launches of a model run in which precision is the caller's routing (vision_mtl_amd/precision.py). */
#define VMTL_PREC_FP32 0
#define VMTL_PREC_BF16 1

const char* vmtl_version(void);
/* HIP's text for the last launch failure (status -2) seen on the calling thread */
const char* vmtl_last_error_string(void);
/* The VMTL_* tuning overrides (VMTL_FORCE_TILE, VMTL_BF16X3, ...) are read from the environment once and cached;
 * this makes the next use re-read them.  Returns the new epoch. */
int vmtl_reload_env(void);
/* tuning aid: *out = 100 MHz device wall clock at the moment `stream` gets there */
int vmtl_timestamp(long long* out, void* stream);

/* ---- convolution (implicit GEMM on exact-fp32 MFMA; bf16 operands on request: VMTL_PREC_*) ----------------
 * replaces nn.Conv2d / nn.ConvTranspose2d at utils/model_utils.py:71,74;
 * models/mtan_model.py:31-46,105-129,214-216,369; models/basic_model.py:30-41 (SegmentationHead);
 * utils/model_utils.py:25-34 (smp.Unet decoder + timm pointwise convs). */

/* y[m][n] = act(bias[n] + sum_kk gather(x)[m][kk] * wp[n][kk]).  wp is [Nw][KH*KW*Cs] (see
 * vmtl_pack_weights).  The same call with the tap-flipped packing and pad' = K-1-pad is the
 * data gradient of a stride-1 conv.  shuffle=1 scatters rows n=(u*2+v)*Cout+co to output pixel
 * (2h+u, 2w+v) channel co: ConvTranspose2d(k=2,s=2).  stats (optional) receives per-row-block
 * column (mean, M2 = sum (v-mean)^2), [vmtl_conv2d_stats_rows()][2][ldy], for BatchNorm. */
int vmtl_conv2d_fwd(const float* x, const float* wp, const float* bias, float* y, float* stats,
                    int B, int H, int W, int Cs, int Ho, int Wo, int ldy, int Nw, int Cout,
                    int KH, int KW, int stride, int pad, int act, int shuffle, void* stream);
int vmtl_conv2d_fwd_p(const float* x, const float* wp, const float* bias, float* y, float* stats,
                      int B, int H, int W, int Cs, int Ho, int Wo, int ldy, int Nw, int Cout,
                      int KH, int KW, int stride, int pad, int act, int shuffle, int precision, void* stream);
/* split-K form for contractions without activation / statistics / shuffle (data gradients, and forward convs of
 * tile-starved layers - decoder blocks 0-1 at small batch - whose BatchNorm then takes its statistics from a sweep):
 * ws = vmtl_conv2d_ksplit(...)*B*Ho*Wo*ldy floats; bias (nullable) is added by the slab sum */
int vmtl_conv2d_ksplit(int B, int Ho, int Wo, int ldy, int Ktot);
int vmtl_conv2d_fwd_ws(const float* x, const float* wp, const float* bias, float* y, float* ws, int B, int H, int W, int Cs,
                       int Ho, int Wo, int ldy, int Nw, int Cout, int KH, int KW, int stride, int pad, void* stream);
int vmtl_conv2d_fwd_ws_p(const float* x, const float* wp, const float* bias, float* y, float* ws, int B, int H, int W,
                         int Cs, int Ho, int Wo, int ldy, int Nw, int Cout, int KH, int KW, int stride, int pad,
                         int precision, void* stream);
int vmtl_conv2d_stats_rows(int B, int Ho, int Wo, int ldy);
int vmtl_conv2d_stats_block(int B, int Ho, int Wo, int ldy); /* output rows per stats row block */

/* Pointwise (1x1 / stride 1) conv as a plain GEMM y[M][ldy] = x[M][Ks] * wp[Nw][Ks]^T (+ bias) for small problems on a
 * dependent chain (timm pointwise convs via utils/model_utils.py:25-34; models/mtan_model.py:31,39,105,113,369):
 * fragments straight from global memory, K split over the waves of a workgroup when the tile grid is small
 * (csrc/conv_pw.hip).  stats (optional): [vmtl_conv1x1_stats_rows][2][ldy] per-row-block (mean, M2) of y,
 * vmtl_conv1x1_stats_block rows each. */
/* variant 0: vmtl_conv1x1_fwd / _cat_fwd / _bn_fwd / _cat_dgrad / _bnbwd (large problems run on the persistent large-M
 * kernel, whose row block differs); 1: launches with a residual operand or an addend (vmtl_conv1x1_bn_res_fwd,
 * vmtl_conv1x1_bnbwd_add: always the fragment-from-global kernel) */
int vmtl_conv1x1_stats_block(int M, int ldy, int Ks, int variant);
int vmtl_conv1x1_stats_rows(int M, int ldy, int Ks, int variant);
int vmtl_conv1x1_fwd(const float* x, const float* wp, const float* bias, float* y, float* stats, int M, int Ks, int ldy,
                     int Nw, int Cout, void* stream);
/* the pointwise GEMMs with the operand precision chosen per call (VMTL_PREC_BF16: bf16(x)*bf16(wp) products on the bf16
 * matrix cores, fp32 accumulation and epilogue; with a prologue the rounded operand is the fp32 value a_out receives).
 * vmtl_conv1x1_stats_block / _rows take no precision: the geometry is the same in both. */
int vmtl_conv1x1_fwd_p(const float* x, const float* wp, const float* bias, float* y, float* stats, int M, int Ks, int ldy,
                       int Nw, int Cout, int precision, void* stream);
/* conv1x1(cat[x, x2]) without the concat (mtan_model.py:57-59,139-141): x [M][K1] (K1 % 4 == 0), x2 [M][K2s], packed
 * weight rows [Nw][K1 + K2s]; and its data gradient writing [dx | dx2] (dx [M][N1], dx2 [M][N2s]) without a split pass */
int vmtl_conv1x1_cat_fwd(const float* x, int K1, const float* x2, int K2s, const float* wp, const float* bias, float* y,
                         float* stats, int M, int ldy, int Nw, int Cout, void* stream);
int vmtl_conv1x1_cat_dgrad(const float* dy, const float* wp, float* dx, int N1, float* dx2, int N2s, int N2, int M,
                           int Ks, void* stream);
int vmtl_conv1x1_cat_fwd_p(const float* x, int K1, const float* x2, int K2s, const float* wp, const float* bias, float* y,
                           float* stats, int M, int ldy, int Nw, int Cout, int precision, void* stream);
int vmtl_conv1x1_cat_dgrad_p(const float* dy, const float* wp, float* dx, int N1, float* dx2, int N2s, int N2, int M,
                             int Ks, int precision, void* stream);
/* and its weight gradient in one launch: slabs [splits][Nw][K1 + K2s], splits = vmtl_conv2d_wgrad_splits(M, Nw, K1 + K2s) */
int vmtl_conv1x1_cat_wgrad(const float* x, int K1, const float* x2, int K2s, const float* dy, float* slabs, int splits,
                           int M, int ldy, int Nw, void* stream);
int vmtl_conv1x1_cat_wgrad_p(const float* x, int K1, const float* x2, int K2s, const float* dy, float* slabs, int splits,
                             int M, int ldy, int Nw, int precision, void* stream);
/* pointwise pre-activation node (the 1x1 counterpart of vmtl_conv3x3_small's prologue / vmtl_conv2d_bnbwd):
 * y = conv1x1(act(coef_a[k]*x + coef_c[k])) - BatchNorm + activation (none / relu / hardswish) of the layer that produced
 * x applied to the operand fragments, a_out (nullable [M][Ks]) = the activated matrix for the weight gradient;
 * and the data gradient ending with that activation's + BatchNorm's backward: dz = (dy*W) * act'(gamma*xhat + beta),
 * stats [vmtl_conv1x1_stats_rows(M, ldy, Ks)][2][ldy] = per-row-block (sum dz, sum dz*xhat). */
int vmtl_conv1x1_bn_fwd(const float* x, const float* coef_a, const float* coef_c, int act_in, float* a_out,
                        const float* wp, const float* bias, float* y, float* stats, int M, int Ks, int ldy, int Nw,
                        int Cout, void* stream);
int vmtl_conv1x1_bnbwd(const float* dy, const float* wp, float* dz, float* stats, const float* ez_x,
                       const float* ez_mean, const float* ez_invstd, const float* ez_gamma, const float* ez_beta,
                       int ez_act, int M, int Ks, int ldy, int Nw, int Cout, void* stream);
int vmtl_conv1x1_bn_fwd_p(const float* x, const float* coef_a, const float* coef_c, int act_in, float* a_out,
                          const float* wp, const float* bias, float* y, float* stats, int M, int Ks, int ldy, int Nw,
                          int Cout, int precision, void* stream);
int vmtl_conv1x1_bnbwd_p(const float* dy, const float* wp, float* dz, float* stats, const float* ez_x,
                         const float* ez_mean, const float* ez_invstd, const float* ez_gamma, const float* ez_beta,
                         int ez_act, int M, int Ks, int ldy, int Nw, int Cout, int precision, void* stream);
/* with a residual operand: the GEMM input is a = act(coef_a*x + coef_c) + res (an inverted-residual block's bn3 output +
 * skip connection consumed by the next block's expand conv; a_out receives a), and with a second gradient of the
 * differentiated tensor added before the backward: dz = (dy*W + addend) * act'(...) */
int vmtl_conv1x1_bn_res_fwd(const float* x, const float* coef_a, const float* coef_c, int act_in, const float* res,
                            float* a_out, const float* wp, const float* bias, float* y, float* stats, int M, int Ks,
                            int ldy, int Nw, int Cout, void* stream);
int vmtl_conv1x1_bnbwd_add(const float* dy, const float* wp, const float* addend, float* dz, float* stats,
                           const float* ez_x, const float* ez_mean, const float* ez_invstd, const float* ez_gamma,
                           const float* ez_beta, int ez_act, int M, int Ks, int ldy, int Nw, int Cout, void* stream);
int vmtl_conv1x1_bn_res_fwd_p(const float* x, const float* coef_a, const float* coef_c, int act_in, const float* res,
                              float* a_out, const float* wp, const float* bias, float* y, float* stats, int M, int Ks,
                              int ldy, int Nw, int Cout, int precision, void* stream);
int vmtl_conv1x1_bnbwd_add_p(const float* dy, const float* wp, const float* addend, float* dz, float* stats,
                             const float* ez_x, const float* ez_mean, const float* ez_invstd, const float* ez_gamma,
                             const float* ez_beta, int ez_act, int M, int Ks, int ldy, int Nw, int Cout, int precision,
                             void* stream);

/* vmtl_conv2d_fwd used as a DATA GRADIENT with the BatchNorm + activation backward of the layer that produced the
 * differentiated tensor fused into the epilogue (reference utils/model_utils.py:72-76 run backwards): y = conv *
 * act'(ez_gamma*xhat + ez_beta), xhat = (ez_x - ez_mean)*ez_invstd; stats[vmtl_conv2d_stats_rows(B,Ho,Wo,ldy)][2][ldy] =
 * per-row-block (sum y, sum y*xhat) -> vmtl_bn_bwd_finalize -> vmtl_bn_bwd_apply. */
int vmtl_conv2d_bnbwd(const float* x, const float* wp, float* y, float* stats, const float* ez_x, const float* ez_mean,
                      const float* ez_invstd, const float* ez_gamma, const float* ez_beta, int ez_act, int B, int H,
                      int W, int Cs, int Ho, int Wo, int ldy, int Nw, int Cout, int KH, int KW, int stride, int pad,
                      void* stream);
int vmtl_conv2d_bnbwd_p(const float* x, const float* wp, float* y, float* stats, const float* ez_x, const float* ez_mean,
                        const float* ez_invstd, const float* ez_gamma, const float* ez_beta, int ez_act, int B, int H,
                        int W, int Cs, int Ho, int Wo, int ldy, int Nw, int Cout, int KH, int KW, int stride, int pad,
                        int precision, void* stream);

/* nearest-x2 upsample of xl + concat with skip + 3x3/pad-1 conv (smp DecoderBlock entry, reference
 * utils/model_utils.py:25-34) as four 2x2 phase convolutions on the low-res map: wp_eff from
 * vmtl_pack_up2_fwd ([4][Cout][4*C0s + 9*C1s]); y is [B][2*H2][2*W2][ldy].  Backward uses
 * vmtl_conv2d_fwd(k4,s2,p1) over dY with vmtl_pack_up2_dgrad, vmtl_conv2d_wgrad(k4,s2,p1) + vmtl_unpack_up2. */
int vmtl_conv2d_up2_fwd(const float* xl, const float* skip, const float* wp_eff, float* y, float* stats,
                        int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout, void* stream);
int vmtl_conv2d_up2_fwd_p(const float* xl, const float* skip, const float* wp_eff, float* y, float* stats,
                          int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout, int precision, void* stream);
int vmtl_conv2d_up2_stats_block(int B, int H2, int W2, int ldy);
/* split-K form of vmtl_conv2d_up2_fwd (no statistics): ws = vmtl_conv2d_up2_ksplit(...)*B*2H2*2W2*ldy floats */
int vmtl_conv2d_up2_ksplit(int B, int H2, int W2, int ldy, int Ktot);
int vmtl_conv2d_up2_fwd_ws(const float* xl, const float* skip, const float* wp_eff, float* y, float* ws, int B, int H2,
                           int W2, int C0s, int C1s, int ldy, int Cout, void* stream);
int vmtl_conv2d_up2_fwd_ws_p(const float* xl, const float* skip, const float* wp_eff, float* y, float* ws, int B, int H2,
                             int W2, int C0s, int C1s, int ldy, int Cout, int precision, void* stream);
/* the same computation for the narrow decoder shapes (vmtl_conv2d_up2_halo_supported: 68 + 0 -> 33 and 136 + 16 -> 67
 * channels, ldy = round_up(Cout, 4), every tensor under 2 GiB) on a halo-tile kernel, fp32 only, without split-K.  stats (optional):
 * [vmtl_conv2d_up2_halo_stat_rows(...)][2][ldy] per-tile (mean, M2), vmtl_conv2d_up2_halo_stat_block(...) pixels per
 * row; stat_rows is 0 (and stats must be null) unless the tiles cover the image exactly.  Unsupported shapes return -3. */
int vmtl_conv2d_up2_halo(const float* xl, const float* skip, const float* wp_eff, float* y, float* stats,
                         int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout, void* stream);
int vmtl_conv2d_up2_halo_supported(int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout);
int vmtl_conv2d_up2_halo_stat_rows(int B, int H2, int W2, int C0s, int C1s, int ldy, int Cout);
int vmtl_conv2d_up2_halo_stat_block(int C0s, int C1s, int ldy, int Cout);
int vmtl_pack_up2_fwd(const float* w, float* dst, int Cout, int C0, int C0s, int C1, int C1s, void* stream);
int vmtl_pack_up2_dgrad(const float* w, float* dst, int Cout, int Cos, int C0, int Cin, void* stream);
int vmtl_unpack_up2(const float* slabs, float* grad, int Cout, int Cos, int C0, int Cin, int nslabs, void* stream);

/* slabs[z][n][kk] = sum_{m in pixel slice z} dy[m][n] * gather(x)[m][kk]  (packed layout, plain
 * stores, no atomics).  splits = vmtl_conv2d_wgrad_splits(B*Ho*Wo, Nw, KH*KW*Cs); the caller
 * provides splits*Nw*KH*KW*Cs floats and vmtl_unpack_weights(..., nslabs=splits) adds the slabs
 * in index order while converting to the torch layout (deterministic weight gradient). */
int vmtl_conv2d_wgrad_splits(int M, int Nw, int Ktot);
int vmtl_conv2d_wgrad(const float* x, const float* dy, float* slabs, int splits, int B, int H, int W, int Cs,
                      int Ho, int Wo, int ldy, int Nw, int KH, int KW, int stride, int pad, void* stream);
int vmtl_conv2d_wgrad_p(const float* x, const float* dy, float* slabs, int splits, int B, int H, int W, int Cs,
                        int Ho, int Wo, int ldy, int Nw, int KH, int KW, int stride, int pad, int precision,
                        void* stream);
/* Host-side routing queries (no launch).  _wgrad_route: what vmtl_conv2d_wgrad[_p] runs for this layer, as
 * loader + 4 * peeled + 8 * PD + 64 * tile rows (loader 0 = general, 1 = scalar chunk of one output row, 2 = row group:
 * 32 / Wo whole output rows per chunk; peeled = the branch-free prefetch loop; PD = chunks in flight), -1 = bad arguments.
 * _pipe_depth: K chunks the implicit GEMM keeps in flight (1 or 2) for a launch of tile id `tile` with gather segments of
 * Cs (and, up2 != 0, C2s) channels, nk K chunks per workgroup and a grid of `workgroups`.  _last_pipe_depth: what the most
 * recent implicit-GEMM launch of the calling thread ran (0 before the first one): tests pin the launcher's own arithmetic. */
int vmtl_conv2d_wgrad_route(int B, int H, int W, int Cs, int Ho, int Wo, int Nw, int KH, int KW, int stride, int pad,
                            int precision);
int vmtl_conv2d_pipe_depth(int tile, int Cs, int C2s, int nk, long long workgroups, int up2, int precision);
int vmtl_conv2d_last_pipe_depth(void);

/* Weight gradient of a NARROW 3x3 / stride 1 / pad 1 conv on a strip-walking halo kernel (csrc/conv_wgrad_small.hip): x is read
 * from memory once instead of once per tap.  Replaces the same conv2d backward-weight call sites of the reference as
 * vmtl_conv2d_wgrad (reference models: smp DecoderBlock / SegmentationHead convs, utils/model_utils.py:61-80 DoubleConv) where
 * supported(Cs, ldy, W) says so: Cs, ldy <= 68 (multiples of 4; which of those widths are routed here is decided there, class
 * by class, by measurement), W a multiple of 32.  slabs: [vmtl_conv3x3_wgrad_small_slabs_for(B, H, W, Cs, ldy, Nw)][Nw][9*Cs],
 * summed by vmtl_unpack_weights(..., nslabs) exactly like the slabs of vmtl_conv2d_wgrad.  _slabs(B, H, W) is _slabs_for of a
 * layer with Cs, ldy <= 36 (wider layers run fewer, longer strip segments).  _supported says what the (fp32) kernel can run;
 * _supported_p(..., pixels, precision) is the routing question of a training step whose launch of pixels = B*H*W would otherwise
 * run vmtl_conv2d_wgrad[_p] at `precision` (VMTL_PREC_*): the widths added last (33-36 on both sides, 40-68 on either) come here
 * in fp32 and from 65,536 pixels only, where they were measured. */
int vmtl_conv3x3_wgrad_small_supported(int Cs, int ldy, int W);
int vmtl_conv3x3_wgrad_small_supported_p(int Cs, int ldy, int W, long long pixels, int precision);
int vmtl_conv3x3_wgrad_small_slabs(int B, int H, int W);
int vmtl_conv3x3_wgrad_small_slabs_for(int B, int H, int W, int Cs, int ldy, int Nw);
int vmtl_conv3x3_wgrad_small(const float* x, const float* dy, float* slabs, int nslabs, int B, int H, int W, int Cs,
                             int ldy, int Nw, void* stream);


/* 3x3 / stride 1 / pad 1 conv for the narrow full-resolution layers (Cs in {16,20,32,36} storage channels in,
 * Nw <= 36 rows of the packed [Nw][9*Cs] weight out): the last decoder block and the heads of `basic`
 * (models/basic_model.py:30-51; smp DecoderBlock conv2 via utils/model_utils.py:25-34) and their data gradients.
 * Halo tile in LDS, weights resident in LDS, persistent workgroups (csrc/conv_small.hip).
 *   prologue: v = act_in(pa[c]*x + pb[c]*x2 + pc[c]) once per input element (pa null: identity; x2/pb null:
 *             one operand); a_out (optional, needs pa) receives the transformed input.
 *   ep_mode 0: y = conv + bias.  yb != null: NCHW split store, channels [0,Ca) -> y [B][Ca][H][W], the rest -> yb.
 *   ep_mode 1: y = conv, stats[row][2][ldy] = (mean, M2) of y over the row's pixels; rows / pixels per row:
 *              vmtl_conv3x3_small_stat_rows / _stat_block (a row is one 128-pixel tile, or all tiles of a workgroup).
 *   ep_mode 2: y = conv * act'(z), z = ez_gamma*xhat + ez_beta, xhat = (ez_x - ez_mean)*ez_invstd (BatchNorm + activation
 *              backward of the layer that produced the tensor whose gradient this conv computes);
 *              stats[row][2][ldy] = (sum y, sum y*xhat) over the row's pixels.
 * ep_mode 1/2 need H % 4 == 0 and W % 32 == 0. */
int vmtl_conv3x3_small_supported(int Cs, int Nw);
int vmtl_conv3x3_small_tiles(int B, int H, int W);
int vmtl_conv3x3_small_stat_rows(int B, int H, int W);  /* rows of stats ... */
int vmtl_conv3x3_small_stat_block(int B, int H, int W); /* ... and the pixels each row covers */
int vmtl_conv3x3_small(const float* x, const float* x2, const float* pa, const float* pb, const float* pc,
                       int act_in, float* a_out, const float* wp, const float* bias, float* y, float* yb, int Ca,
                       float* stats, int ep_mode, const float* ez_x, const float* ez_mean, const float* ez_invstd,
                       const float* ez_gamma, const float* ez_beta, int ez_act, int B, int H, int W, int Cs, int ldy,
                       int Nw, int Cout, void* stream);

/* The same 3x3 / stride 1 / pad 1 conv for the MID-WIDTH layers on a halo-tile kernel (csrc/conv3x3_halo.hip), fp32 only:
 * Cs in {64, 68} storage channels in, ldy in {16, 32, 64, 68} storage channels out, Nw rows of the packed [Nw][9*Cs] weight,
 * ldy = round_up(Nw, 4), x under 2 GiB (vmtl_conv3x3_halo_supported; anything else returns -3).  One workgroup per
 * 4 x 32 output tile; the weights stream from L2.
 *   prologue: v = act_in(pa[c]*x + pc[c]) once per input element (pa null: identity); a_out (optional, needs pa)
 *             receives the transformed input.
 *   ep_mode 0: y = conv + bias (stats must be null).
 *   ep_mode 1: y = conv + bias, stats[row][2][ldy] = (mean, M2) of y over the row's pixels.
 *   ep_mode 2: y = conv * act'(z), z = ez_gamma*xhat + ez_beta, xhat = (ez_x - ez_mean)*ez_invstd;
 *              stats[row][2][ldy] = (sum y, sum y*xhat) over the row's pixels (no bias).
 * A statistics row is one tile: vmtl_conv3x3_halo_stat_rows / _stat_block; rows = 0 (and ep_mode 1/2 are refused) unless
 * H % 4 == 0 and W % 32 == 0. */
int vmtl_conv3x3_halo_supported(int B, int H, int W, int Cs, int ldy, int Nw);
int vmtl_conv3x3_halo_stat_rows(int B, int H, int W);
int vmtl_conv3x3_halo_stat_block(int B, int H, int W);
int vmtl_conv3x3_halo(const float* x, const float* pa, const float* pc, int act_in, float* a_out, const float* wp,
                      const float* bias, float* y, float* stats, int ep_mode, const float* ez_x, const float* ez_mean,
                      const float* ez_invstd, const float* ez_gamma, const float* ez_beta, int ez_act, int B, int H,
                      int W, int Cs, int ldy, int Nw, int Cout, void* stream);

/* depthwise KxK (K in {3,5}, stride in {1,2}); wp is packed [K*K][Cs]. */
int vmtl_dwconv_fwd(const float* x, const float* wp, float* y, int B, int H, int W, int Cs, int Ho, int Wo,
                    int K, int stride, int pad, void* stream);
/* depthwise conv as a pre-activation node: v = act(coef_a[c]*x + coef_c[c]) applied to the taps while loading (the
 * BatchNorm + activation of the pointwise conv that produced x; coefficients from vmtl_bn_stats_coef), y = dwconv(v),
 * a_out (optional) = v, partial (optional) = [vmtl_dwconv_bn_stats_rows(M, Cs)][2][Cs] (mean, M2) rows of y over
 * vmtl_dwconv_bn_stats_block(M, Cs) output pixels each, M = B*Ho*Wo.  pad must be (K-1)/2. */
int vmtl_dwconv_bn_stats_rows(int M, int Cs);
int vmtl_dwconv_bn_stats_block(int M, int Cs);
int vmtl_dwconv_bn_fwd(const float* x, const float* coef_a, const float* coef_c, int act, const float* wp, float* y,
                       float* a_out, float* partial, int B, int H, int W, int Cs, int Ho, int Wo, int K, int stride,
                       int pad, void* stream);
int vmtl_dwconv_bwd_data(const float* dy, const float* wp, float* dx, int B, int H, int W, int Cs, int Ho,
                         int Wo, int K, int stride, int pad, void* stream);
/* dx = dwconv^T(dy) + addend (a second gradient of the same tensor, e.g. the residual branch of the block) */
int vmtl_dwconv_bwd_data_add(const float* dy, const float* wp, const float* addend, float* dx, int B, int H, int W,
                             int Cs, int Ho, int Wo, int K, int stride, int pad, void* stream);
/* partial: vmtl_dwconv_bwd_weight_rows(B*Ho*Wo, Cs) * K*K * Cs floats of scratch; dw in the torch (C,1,K,K) layout */
int vmtl_dwconv_bwd_weight_rows(int M, int Cs);
int vmtl_dwconv_bwd_weight(const float* x, const float* dy, float* partial, float* dw, int B, int H, int W,
                           int C, int Cs, int Ho, int Wo, int K, int stride, int pad, void* stream);
/* The three row queries above (vmtl_dwconv_bn_stats_rows, vmtl_dwconv_bn_stats_block, vmtl_dwconv_bwd_weight_rows) never
 * trap: for M <= 0 or Cs <= 0 the two row counts are 1 and the block is some positive even number.  Every launcher above
 * answers Ho <= 0, Wo <= 0 or a padded map smaller than the kernel (H + 2*pad < K, W + 2*pad < K) with -1.
 *
 * Which kernel a depthwise launcher starts: host-only queries over the launcher's own integer arguments.  The launchers
 * switch on these results, so the answer is the dispatch.  < 0: the status the launcher returns for these arguments.
 * Otherwise a bit field:
 *   VMTL_DW_ROUTE_ACT_MASK  fused forward: the VMTL_ACT_* code the kernel is instantiated for (none / relu / hswish)
 *   VMTL_DW_ROUTE_SPEC      the compile-time specialisation (fused forward: the pair kernel, needs an even Wo; data
 *                           gradient: even W, for stride 2 also even H; weight gradient: the pair kernel, even Wo; the
 *                           gradients also need pad == (K-1)/2); clear = the run-time-K "generic" kernel.  VMTL_DWBN_GENERIC
 *                           (non-zero, read with the other VMTL_* overrides) clears it everywhere
 *   VMTL_DW_ROUTE_K5        K == 5.  Set on specialised routes and on the generic weight gradient (its <25> instantiation;
 *                           clear = <9>); always clear on the generic forward and data gradient, which take K at run time
 *   VMTL_DW_ROUTE_S2        stride == 2, specialised routes only
 *   VMTL_DW_ROUTE_WLDS      fused forward, 5x5 pair kernel: the packed weights go through LDS - when a statistics block has
 *                           at least 12 output pixels and the 25*Cs floats fit into a workgroup's 160 KB next to the
 *                           kernel's 9216 static bytes (Cs <= 1544)
 *   VMTL_DW_ROUTE_FIN32     weight gradient: the finalize with 32 elements per workgroup (C*K*K >= 4096), clear = 8
 *   VMTL_DW_ROUTE_QL(r)     weight gradient: quad lanes of the first stage, 1, 2, 4, 8 or 16
 * The fused forward has 3 generic + 18 specialised routes, the data gradient 1 + 4, the weight gradient 2 + 4 first stages
 * x 2 finalizes x 5 lane counts. */
#define VMTL_DW_ROUTE_ACT_MASK 3
#define VMTL_DW_ROUTE_SPEC 4
#define VMTL_DW_ROUTE_K5 8
#define VMTL_DW_ROUTE_S2 16
#define VMTL_DW_ROUTE_WLDS 32
#define VMTL_DW_ROUTE_FIN32 64
#define VMTL_DW_ROUTE_QL(r) (1 << (((r) >> 8) & 7))
int vmtl_dwconv_bn_fwd_route(int B, int H, int W, int Cs, int Ho, int Wo, int K, int stride, int pad, int act);
int vmtl_dwconv_bwd_data_route(int B, int H, int W, int Cs, int Ho, int Wo, int K, int stride, int pad);
int vmtl_dwconv_bwd_weight_route(int B, int H, int W, int C, int Cs, int Ho, int Wo, int K, int stride, int pad);

/* torch parameter layout <-> packed GEMM operand (formula in csrc/pack.hip). */
int vmtl_pack_weights(const float* src, float* dst, int R1, int R0, int T, int C, int Cs, long long sr1,
                      long long sr0, long long st, long long sc, int flip, void* stream);
/* the same with a per-input-channel factor folded into the operand: the cross-stitch scale of the tensor the conv reads
 * (models/cross_stitch_model.py:32-37 followed by the next conv of the CSNet walk :108-142) - conv(W, s*x) = conv(W*s, x).
 * smode 1: packed column channel = input channel (forward packing); 2: packed row (data-gradient packing);
 * factor = scale[channel * sstride] (sstride 0: layer-wise stitching, one scalar) */
int vmtl_pack_weights_scaled(const float* src, float* dst, int R1, int R0, int T, int C, int Cs, long long sr1,
                             long long sr0, long long st, long long sc, int flip, const float* scale, int sstride,
                             int smode, void* stream);
/* weight gradient behind a folded stitch scale: slabs hold dL/d(W*s); grad <- dL/dW (torch layout (R0, C, T)),
 * ds <- dL/ds (C entries, or one scalar when reduce_all) - the CrossStitchLayer weight gradient without a pass over
 * activations; work: R0*C*T + C floats */
int vmtl_unpack_weights_stitch(const float* packed, float* grad, const float* w, const float* scale, int sstride,
                               float* ds, float* work, int R0, int T, int C, int Cs, int nslabs, long long slab_stride,
                               int reduce_all, void* stream);
/* batched form: descs = device array of n records {src*, dst*, i64 sr1, sr0, st, sc, start; scale*; i32 R1, R0, T, C,
 * Cs, flip, sstride, smode} (vmtl_pack_desc_bytes() bytes each), start = first flat work index; total = sum R1*R0*T*Cs. */
int vmtl_pack_desc_bytes(void);
int vmtl_pack_weights_batch(const void* descs, int n, long long total, void* stream);
int vmtl_pack_weights_slice(const float* src, float* dst, int R0, int T, int C, int group, long long sr0,
                            long long st, long long sc, int flip, void* stream);
int vmtl_unpack_weights(const float* packed, float* grad, int R1, int R0, int T, int C, int Cs,
                        long long sr1, long long sr0, long long st, long long sc, int flip, int nslabs,
                        long long slab_stride, void* stream); /* slab_stride 0: R1*R0*T*Cs */

/* ---- BatchNorm2d (+ activation, gate multiply, residual add) -----------------------------
 * replaces nn.BatchNorm2d/ReLU/Sigmoid/mul at utils/model_utils.py:72-76;
 * models/mtan_model.py:67-81,139-167. */
int vmtl_reduce_rows(int M); /* partial rows used by the two-stage reductions */
/* Statistics rows (partial [nblk][2][Cs], vmtl_bn_stats with nblk_from_conv > 0 and vmtl_bn_apply_fused): row b holds
 * (mean_b, M2_b) of the rows [b*rows_per_blk, min(M, (b+1)*rows_per_blk)); any M <= nblk * rows_per_blk < 2^31 is accepted and
 * a row that lies wholly past M may hold anything: both consumers skip it. */
int vmtl_bn_stats(const float* x, int M, int C, int Cs, float* partial, int nblk_from_conv,
                  int rows_per_blk_from_conv, float eps, float momentum, float* running_mean, float* running_var, long long* num_batches_tracked,
                  float* save_mean, float* save_invstd, void* stream);
int vmtl_bn_eval_stats(const float* running_mean, const float* running_var, int C, int Cs, float eps,
                       float* save_mean, float* save_invstd, void* stream);
/* the same two, additionally emitting the normalisation as per-channel prologue coefficients of the consumer
 * conv (vmtl_conv3x3_small): act(BN(x)) = act(coef_a[c] * x + coef_c[c]), zeros on the pad channels */
int vmtl_bn_stats_coef(const float* x, int M, int C, int Cs, float* partial, int nblk_from_conv,
                       int rows_per_blk_from_conv, float eps, float momentum, float* running_mean, float* running_var,
                       long long* num_batches_tracked, float* save_mean, float* save_invstd, const float* gamma,
                       const float* beta, float* coef_a, float* coef_c, void* stream);
int vmtl_bn_eval_stats_coef(const float* running_mean, const float* running_var, int C, int Cs, float eps,
                            float* save_mean, float* save_invstd, const float* gamma, const float* beta,
                            float* coef_a, float* coef_c, void* stream);
/* batched eval statistics: one launch for n layers.  descs = device array of n records {running_mean*, running_var*,
 * gamma*, beta*, save_mean*, save_invstd*, coef_a*, coef_c*, i32 C, Cs, f32 eps, i32 pad} (vmtl_bn_eval_desc_bytes()
 * bytes each); every record writes what vmtl_bn_eval_stats(_coef) writes for it (gamma / beta / coef_a+coef_c may be
 * null, as there).  max_cs = the largest Cs of the table (a multiple of 4); host-only size query. */
int vmtl_bn_eval_desc_bytes(void);
int vmtl_bn_eval_stats_batch(const void* descs, int n, int max_cs, void* stream);
int vmtl_bn_apply(const float* x, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, const float* mul, const float* res, float* y, long long M, int C,
                  int Cs, int act, void* stream);
/* finalize + apply in one launch for training-mode BatchNorm whose statistics come as few per-block rows
 * (nblk <= vmtl_bn_fuse_max_rows(); same arguments as vmtl_bn_stats with conv partials + vmtl_bn_apply) */
int vmtl_bn_fuse_max_rows(void);
int vmtl_bn_apply_fused(const float* x, const float* partial, int nblk, int rows_per_blk, float eps, float momentum,
                        float* running_mean, float* running_var, long long* num_batches_tracked, float* save_mean,
                        float* save_invstd, const float* gamma, const float* beta, const float* mul, const float* res,
                        float* y, long long M, int C, int Cs, int act, void* stream);
int vmtl_bn_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma,
                const float* beta, const float* mul, float* dmul, float* partial, float* sum_dz,
                float* sum_dzx, float* dx, int M, int C, int Cs, int act, int training, void* stream);
/* vmtl_bn_bwd in two halves, for producers whose epilogue already emitted dz = dy * act'(z) and the per-block
 * column sums rows [nblk][2][Cs] = (sum dz, sum dz*xhat): finalize -> BatchNorm parameter gradients (+ optional
 * coefficients of dx = coef_a*dz + coef_b*x + coef_c for a consumer that applies it while loading); apply -> dx. */
int vmtl_bn_bwd_finalize(const float* partial, int nblk, int M, int C, int Cs, float* sum_dz, float* sum_dzx,
                         const float* mean, const float* invstd, const float* gamma, int training, float* coef_a,
                         float* coef_b, float* coef_c, void* stream);
int vmtl_bn_bwd_apply(const float* x, const float* dz, const float* mean, const float* invstd, const float* gamma,
                      const float* sum_dz, const float* sum_dzx, float* dx, int M, int C, int Cs, int training,
                      void* stream);

/* BatchNorm + activation + MaxPool2d(2) as ONE node (csrc/bn.hip): reference models/mtan_model.py:67-83 (AttentionModuleEncoder:
 * conv3 -> bn3 -> ReLU -> max_pool2d, nobody else reads the full-resolution activation).  fwd: y [B][H/2][W/2][Cs] from x
 * [B][H][W][Cs] (H, W even) with mean / invstd from vmtl_bn_stats; bwd: the pooled gradient dyp is scattered to each window's
 * arg-max inside the BatchNorm reduce / apply sweeps (sum_dz, sum_dzx [C] = dbeta, dgamma; partial:
 * vmtl_reduce_rows(B*(H/2)*(W/2))*2*Cs floats). */
int vmtl_bn_act_pool2_fwd(const float* x, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, float* y, int B, int H, int W, int C, int Cs, int act, void* stream);
int vmtl_bn_act_pool2_bwd(const float* x, const float* dyp, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, float* partial, float* sum_dz, float* sum_dzx,
                          float* dx, int B, int H, int W, int C, int Cs, int act, int training, void* stream);

/* ---- torchvision BasicBlock ResNet encoder (smp ResNetEncoder "resnet18" / "resnet34" behind encoder_name,
 * reference vision_mtl/utils/model_utils.py:10-31, models/basic_model.py:10-29; csrc/resnet.hip) ---------------------
 * Data gradient of a stride-2 dense conv (dx [B][H][W][Cs] from dy [B][Ho][Wo][ldy], Ho = (H + 2*pad - K)/2 + 1) by phase
 * decomposition: the pixels of phase (ih & 1, iw & 1) get a stride-1 correlation of dy with that phase's subset of the
 * flipped taps - one launch per phase into ws (implicit GEMM, split-K where the stride-1 data gradient of that shape
 * splits too; single-tap unpadded phases in fp32 on the pointwise GEMM), then one gather interleaves them; pixels no
 * window covers get an exact 0.  wp: vmtl_pack_dgrad_s2 of the torch (Cout, Cin, K, K) weight (vmtl_pack_dgrad_s2_size floats);
 * ws: vmtl_conv2d_dgrad_s2_ws floats.  Supported (K, pad): those whose phases share one correlation pad, e.g. (1, 0),
 * (3, 1), (7, 3) (vmtl_conv2d_dgrad_s2_supported; the size queries return -1 otherwise). */
int vmtl_conv2d_dgrad_s2_supported(int K, int pad);
long long vmtl_conv2d_dgrad_s2_ws(int B, int H, int W, int Cs, int Ho, int Wo, int ldy, int K, int pad);
long long vmtl_pack_dgrad_s2_size(int Cin, int ldy, int K, int pad);
int vmtl_pack_dgrad_s2(const float* w, float* dst, int Cout, int Cin, int ldy, int K, int pad, void* stream);
int vmtl_conv2d_dgrad_s2(const float* dy, const float* wp, float* dx, float* ws, int B, int H, int W, int Cs, int Ho,
                         int Wo, int ldy, int Cin, int K, int pad, void* stream);
int vmtl_conv2d_dgrad_s2_p(const float* dy, const float* wp, float* dx, float* ws, int B, int H, int W, int Cs, int Ho,
                           int Wo, int ldy, int Cin, int K, int pad, int precision, void* stream);
/* BatchNorm + activation + MaxPool2d(3, stride 2, pad 1) of the ResNet stem as one node: a_out (nullable) [B][H][W][Cs] =
 * act(BN(x)) (the decoder skip), y [B][Ho][Wo][Cs] its pool, Ho = (H-1)/2 + 1 (floor mode, -inf padding, torch CPU
 * max_pool2d's tie and NaN rule), idx [B][Ho][Wo][Cs] bytes = the arg-max's window position (0..8).  mean == invstd ==
 * NULL: no BatchNorm (the plain pool of an activated map: act NONE).  bwd: each input pixel gathers dskip (nullable) plus
 * dyp of the windows whose arg-max it is (no atomics); with BatchNorm then act' (dz, [B][H][W][Cs] scratch), the partial
 * rows (partial: vmtl_reduce_rows(B*H*W)*2*Cs floats), sum_dz / sum_dzx [C] = dbeta / dgamma and dx; without, dx = the
 * gathered gradient times act'(x). */
int vmtl_bn_act_pool3s2_fwd(const float* x, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* a_out, float* y, unsigned char* idx, int B, int H, int W, int C,
                            int Cs, int act, void* stream);
int vmtl_bn_act_pool3s2_bwd(const float* x, const float* dskip, const float* dyp, const unsigned char* idx,
                            const float* mean, const float* invstd, const float* gamma, const float* beta, float* dz,
                            float* partial, float* sum_dz, float* sum_dzx, float* dx, int B, int H, int W, int C, int Cs,
                            int act, int training, void* stream);
/* Residual close of a BasicBlock: y = act(BN_a(z) + r), r = res (identity) or BN_b(zd) (downsample branch: res NULL);
 * mean / invstd from vmtl_bn_stats (train) or the running buffers (eval).  bwd: g = dy * act'(pre) (the identity
 * gradient), the partial rows (partial: vmtl_reduce_rows(M)*3*Cs floats), sum_dz_* / sum_dzx_* [C] = dbeta / dgamma of
 * each BatchNorm, and dz / dzd (nullable) = the gradients of z / zd through their BatchNorm. */
int vmtl_bn_add_act_fwd(const float* z, const float* mean_a, const float* invstd_a, const float* gamma_a,
                        const float* beta_a, const float* res, const float* zd, const float* mean_b, const float* invstd_b,
                        const float* gamma_b, const float* beta_b, float* y, int M, int C, int Cs, int act, void* stream);
int vmtl_bn_add_act_bwd(const float* z, const float* mean_a, const float* invstd_a, const float* gamma_a,
                        const float* beta_a, const float* res, const float* zd, const float* mean_b, const float* invstd_b,
                        const float* gamma_b, const float* beta_b, const float* dy, float* g, float* partial,
                        float* sum_dz_a, float* sum_dzx_a, float* sum_dz_b, float* sum_dzx_b, float* dz, float* dzd, int M,
                        int C, int Cs, int act, int training, void* stream);

/* out[c] = sum_m a[m][c] (mode 0) or a*b (mode 1); reduce_all sums over channels too.
 * partial: (vmtl_reduce_rows(M) + 1) * Cs floats of scratch */
int vmtl_colsum(const float* a, const float* b, int M, int C, int Cs, int mode, int reduce_all,
                float* partial, float* out, void* stream);

/* ---- gathers / elementwise ---------------------------------------------------------------
 * concat2: utils/model_utils.py:46-58; models/mtan_model.py:65,152,229;
 *          models/cross_stitch_model.py:126-134; smp DecoderBlock (nearest x2 + cat). */
int vmtl_concat2(const float* a, int Ha, int Wa, int Ca, int Csa, int upa, int oha, int owa,
                 const float* b, int Hb, int Wb, int Cb, int Csb, int upb, int ohb, int owb, float* y,
                 int B, int H, int W, int Cd, void* stream);
int vmtl_concat2_bwd(const float* dy, float* dx, int B, int H, int W, int Cd, int c_off, int Hs, int Ws,
                     int C, int Cs, int up, int oh, int ow, void* stream);
/* models/mtan_model.py:49,81,364,388 */
int vmtl_maxpool2_fwd(const float* x, float* y, int B, int H, int W, int Cs, void* stream);
int vmtl_maxpool2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int Cs, void* stream);
/* models/mtan_model.py:125,143-144 (bilinear x2, align_corners=True) */
int vmtl_bilinear_up2_fwd(const float* x, float* y, int B, int H, int W, int Cs, void* stream);
int vmtl_bilinear_up2_bwd(const float* dy, float* dx, int B, int H, int W, int Cs, void* stream);
/* timm SqueezeExcite pieces (utils/model_utils.py:25-34) */
int vmtl_spatial_mean(const float* x, float* y, int B, int HW, int Cs, void* stream);
int vmtl_channel_bcast(const float* x, const float* s, float* y, int B, int HW, int Cs, int mode, void* stream);
int vmtl_channel_scale_bwd_s(const float* x, const float* dy, float* ds, int B, int HW, int Cs, void* stream);
/* The squeeze-excite gate as batch-sized GEMMs (M = B <= vmtl_fc_max_rows() rows): the 1x1 convs of timm
 * SqueezeExcite on a (B,1,1,C) map (encoder of models/basic_model.py:17-28).
 * vmtl_fc_fwd: z = bias + A W^T, y = act(z); A = a_scale * sum_{s<a_parts} a[s] (partial sums of a spatial
 *   reduction), optionally multiplied by act'(a_z) with activation a_act (data gradient with the activation
 *   backward fused: pass the transposed weight as w).  w is [N][ldw] with K contiguous; z may be NULL;
 *   a_out (may be NULL) receives the finished A operand [M][lda] (summed, scaled, unmasked).
 * vmtl_fc_wgrad: dw[n][k] = sum_m dz[m][n] x[m][k], db[n] = sum_m dz[m][n], dz = (sum of dy parts) * act'(zo);
 *   dw in the torch (N, K, 1, 1) layout.
 * vmtl_hw_reduce: part[s][b][c] = sum over HW slice s of x (* y if given); S = vmtl_hw_reduce_parts(B,HW,Cs).
 * vmtl_channel_scale_add: y = x * s[b][c] + t[b][c] * t_scale (t may be NULL). */
int vmtl_fc_max_rows(void);
int vmtl_fc_fwd(const float* a, int a_parts, long long a_part_stride, float a_scale, const float* a_z, int a_act,
                float* a_out, const float* w, const float* bias, float* z, float* y, int M, int K, int N, int lda,
                int ldw, int ldy, int act, void* stream);
int vmtl_fc_wgrad(const float* x, int x_parts, long long x_part_stride, float x_scale, const float* dyo, int dy_parts,
                  long long dy_part_stride, const float* zo, float* dw, float* db, int M, int K, int N, int lda, int ldn,
                  int act, void* stream);
int vmtl_hw_reduce_parts(int B, int HW, int Cs);
int vmtl_hw_reduce(const float* x, const float* y, float* part, int B, int HW, int Cs, void* stream);
int vmtl_channel_scale_add(const float* x, const float* s, const float* t, float t_scale, float* y, int B, int HW,
                           int Cs, void* stream);
/* The same gate in one launch per direction (timm SqueezeExcite.forward, utils/model_utils.py:25-34, on the encoder of
 * models/basic_model.py:17-28): one workgroup per image reduces the map and walks both weight matrices in the torch
 * (R, C, 1, 1) / (C, R, 1, 1) layout.  Cs = ceil4(C), Rs = ceil4(R); every [B][Cs] / [B][Rs] output has zero pad columns.
 * vmtl_se_gate_supported: the launches ops.squeeze_excite takes for the shape: bit 0 - vmtl_se_gate_bwd and vmtl_se_wgrad,
 *   bit 1 - vmtl_se_gate_fwd (small weights only: csrc/fc.hip).  VMTL_SE_FUSED=0: none, 2: all wherever supported.
 * vmtl_se_gate_fwd: pooled = mean_hw x, z1 = W_r pooled + b_r, h = act1(z1), z2 = W_e h + b_e, g = act2(z2).
 * vmtl_se_gate_bwd: dg = sum_hw dy * x, dh = (dg * act2'(z2)) W_e, dmean (may be NULL) = (dh * act1'(z1)) W_r.
 * vmtl_se_wgrad: dW_e, db_e from (dg * act2'(z2), h) and dW_r, db_r from (dh * act1'(z1), pooled), torch layout. */
int vmtl_se_gate_supported(int B, int C, int R);
int vmtl_se_gate_fwd(const float* x, const float* wr, const float* br, const float* we, const float* be, float* pooled,
                     float* z1, float* h, float* z2, float* g, int B, int HW, int C, int R, int act1, int act2,
                     void* stream);
int vmtl_se_gate_bwd(const float* dy, const float* x, const float* z1, const float* z2, const float* wr, const float* we,
                     float* dg, float* dh, float* dmean, int B, int HW, int C, int R, int act1, int act2, void* stream);
int vmtl_se_wgrad(const float* pooled, const float* h, const float* dg, const float* dh, const float* z1, const float* z2,
                  float* dwr, float* dbr, float* dwe, float* dbe, int B, int C, int R, int act1, int act2, void* stream);
/* models/cross_stitch_model.py:32-37 (diagonal of the 2x2 stitch matrix) */
int vmtl_stitch(const float* x, const float* w, float* y, long long M, int C, int Cs, int wstride, void* stream);
/* its backward in one sweep: dx (nullable) = w * dy, dw[c] = sum_m x*dy (reduce_all: one scalar);
 * partial: (vmtl_reduce_rows(M) + 1) * Cs floats of scratch */
int vmtl_stitch_bwd(const float* x, const float* dy, const float* w, float* dx, float* partial, float* dw, int M,
                    int C, int Cs, int wstride, int reduce_all, void* stream);
/* The full 2x2 cross-stitch unit of Misra et al. (csrc/stitch_mix.hip) - the opt-in mode that models/cross_stitch_model.py's
 * einsum never reaches (it only uses the diagonal: vmtl_stitch).  Two tasks: y0 = w00*x0 + w01*x1, y1 = w10*x0 + w11*x1 on
 * [M][Cs] activations, lanes c >= C written as zeros.  w is the parameter as stored: entry (a,b,c) at (a*2+b)*C + c
 * (wstride 1, channel-wise) or (a,b) at a*2+b (wstride 0, layer-wise).  Not in place: an output may not overlap an input
 * or the other output. */
int vmtl_stitch_mix(const float* x0, const float* x1, const float* w, float* y0, float* y1, int M, int C, int Cs,
                    int wstride, void* stream);
/* its backward in one sweep: dx0 = w00*dy0 + w10*dy1, dx1 = w01*dy0 + w11*dy1 (nullable together), dw (nullable) = the
 * whole gradient in parameter layout, block (a,b) = sum_m dy_a * x_b (4*C floats, or 4 when wstride 0), overwritten,
 * fp64 fixed-order finalize, no atomics.  dw NULL: data gradients only, no reduction is launched (x0, x1, partial unused).
 * partial: (4 * vmtl_reduce_rows(M) + 4) * Cs floats of scratch */
int vmtl_stitch_mix_bwd(const float* x0, const float* x1, const float* dy0, const float* dy1, const float* w, float* dx0,
                        float* dx1, float* partial, float* dw, int M, int C, int Cs, int wstride, void* stream);
/* mode 0 add, 1 sigmoid, 2 sigmoid-backward-from-output, 3 scale by *b */
int vmtl_eltwise(const float* a, const float* b, float* y, int mode, long long total, void* stream);
/* y = a + b (+ c) (+ d), c / d nullable, total % 4 == 0: the gradient sum of an activation with 2..4 consumers - what
 * autograd's AccumulateGrad / add nodes do for x, d, merged in models/mtan_model.py:364-399 and every residual branch */
int vmtl_add_n(const float* a, const float* b, const float* c, const float* d, float* y, long long total, void* stream);
/* y = wa*a + wb*b: the weighted sum of the task losses (lit_module.py:127-129) */
int vmtl_axpby(const float* a, const float* b, float* y, float wa, float wb, long long total, void* stream);
int vmtl_fill_zero(float* p, long long n, void* stream); /* n floats <- 0 (a memset node) */
/* lit_module.py:137-138 (argmax of softmax == argmax of logits) */
int vmtl_argmax_channels(const float* z, long long* out, int B, int HW, int C, long long sb, long long sc,
                         long long sp, void* stream);
int vmtl_nchw_to_nhwc(const float* x, float* y, int B, int C, int HW, int Cs, int Cw, void* stream);
int vmtl_nhwc_to_nchw(const float* x, float* y, int B, int C, int HW, int Cs, void* stream);
/* input side (lit_module.py:211-219 + the dataset sample contract of data_modules/cityscapes.py:39-83,
 * nyuv2.py:100-141): HWC pixel rows [P][C] -> internal NHWC storage [P][Cs] (zero pad channels), y = x * scale */
int vmtl_hwc_to_nhwc_pad(const float* x, float* y, long long P, int C, int Cs, float scale, void* stream);
/* NYUv2 sample transform on the device (csrc/resize.hip): the reference's host chain ToTensor() + Resize((Ho, Wo),
 * antialias=True) of cfg.py:144-155, applied per sample by data_modules/nyuv2.py:100-141, followed by the value rules of
 * that loader (img in [0,1], mask class ids, depth = counts / 1e4, then / max_depth for a sample whose resized maximum
 * exceeds 1).  Inputs are the decoded files as stacked by data.collate_raw: img uint8 [B][Hi][Wi][3], mask uint8
 * [B][Hi][Wi], depth [B][Hi][Wi] of type depth_dtype (VMTL_DEPTH_*).  Outputs: img_out the model's NHWC input storage
 * [B][Ho][Wo][4] (pad channel 0), mask_out int64 [B][Ho][Wo], depth_out float [B][Ho][Wo]; part holds
 * vmtl_nyuv2_resize_parts(...) floats of scratch (per-tile depth maxima).  img, mask, depth and img_out are 16-byte
 * aligned.  Two launches; -3 for a downscale too steep for the kernel's LDS tiles. */
#define VMTL_DEPTH_U16 0
#define VMTL_DEPTH_I32 1
int vmtl_nyuv2_resize_parts(int B, int Hi, int Wi, int Ho, int Wo, int depth_dtype);
int vmtl_nyuv2_resize(const void* img, const void* mask, const void* depth, int depth_dtype, float* img_out,
                      long long* mask_out, float* depth_out, float* part, int B, int Hi, int Wi, int Ho, int Wo,
                      float max_depth, void* stream);
/* Joint training augmentation on the device (csrc/augment.hip): random scale-crop + horizontal
 * flip (+ brightness gain) of image, mask and depth together.  Two launches, no allocation, no synchronisation.
 * vmtl_augment_draw: state int64[2] = {seed, counter}; fills params int32 [B][8] = {scale_idx, top, left, flip, gain
 * (float bits), 0, 0, 0} with the counter-based generator of DESIGN.md section 19 and then stores counter + 1, so a
 * replayed graph draws fresh rows.  crop_hw int32 [S][2] = {int(H / s), int(W / s)} per scale (computed by the host in
 * double precision), S <= 8; flip_threshold = round(p_flip * 2^24) in [0, 2^24]; 0 <= brightness < 1.  params is
 * 16-byte aligned.
 * vmtl_augment_apply: img float with pixel stride ld = 3 ([B][H][W][3], dataset sample layout) or 4 (the model's NHWC
 * input storage, 16-byte aligned), mask int64 [B][H][W], depth float [B][H][W]; scales float [S].  Outputs: img_out
 * NHWC storage [B][H][W][4] (pad lane 0), mask_out int64, depth_out float (depth / s).  Image: bilinear,
 * align_corners=True; mask and depth: nearest; both as torch's CPU F.interpolate of the crop window.  Every parameter
 * row is clamped into range before use.  -1 when an output overlaps its input. */
int vmtl_augment_draw(long long* state, int* params, const int* crop_hw, int B, int H, int W, int S, int flip_threshold,
                      float brightness, void* stream);
int vmtl_augment_apply(const float* img, int ld, const long long* mask, const float* depth, const int* params,
                       const float* scales, const int* crop_hw, float* img_out, long long* mask_out, float* depth_out,
                       int B, int H, int W, int S, void* stream);
/* Test-time augmentation and output-size predictions (csrc/tta.hip): the model is run on resized
 * and mirrored views of a batch, the views are merged at the base size (H, W), and the merged map is turned into
 * predictions at any output size without the (B, C, Ho, Wo) map ever being written.  Forward only; one launch each, one
 * thread per output pixel, no atomics, no workspace, bit-identical from run to run.  Every resampling is
 * F.interpolate(mode="bilinear", align_corners=False, antialias=False): src = (dst + 0.5) * in / out - 0.5 clamped
 * below at 0, the second tap clamped to the last index; equal sizes are an exact copy.  1 <= C <= 32, else -3.
 * vmtl_tta_view: img float with pixel stride ld = 3 or 4 as vmtl_augment_apply takes it ([B][H][W][ld]; ld 4 is 16-byte
 * aligned) -> out, the model's NHWC input storage [B][Ho][Wo][4] (16-byte aligned, pad lane +0.0f), resampled and then,
 * with flip != 0, mirrored in x: out[.., x, :] = resized[.., Wo - 1 - x, :].
 * vmtl_tta_accumulate: one view.  logits [B][C][h][w] and depth_logits [B][1][h][w] (NCHW, as the model returns them
 * for that view) are un-mirrored with flip != 0 (the sample at x' is read from w - 1 - x'), resampled to (H, W) and
 * merged into acc [B][C][H][W] and acc_depth [B][H][W]:
 *   VMTL_TTA_PROB   acc (+)= weight * softmax_c(resampled logits)
 *   VMTL_TTA_LOGIT  acc (+)= weight * resampled logits
 *   both            acc_depth (+)= weight * depth_gain * bilinear(sigmoid(depth_logits)), the sigmoid of vmtl_eltwise
 *                   mode 1 applied per tap
 * first != 0 assigns (whatever the accumulators held), first == 0 adds.  depth_logits and acc_depth are null together.
 * vmtl_tta_finish: acc (and acc_depth, nullable together with depth) resampled from (H, W) to (Ho, Wo) channel by
 * channel, keeping a running best: segm int64 [B][Ho][Wo] = arg-max (the first maximum wins, as vmtl_argmax_channels),
 * depth float [B][Ho][Wo] = inv_weight * bilinear(acc_depth), confidence (nullable) float [B][Ho][Wo] = the largest
 * softmax probability of the merged map there: best / sum for VMTL_TTA_PROB, max softmax_c(inv_weight * resampled acc)
 * by an online softmax in the same pass for VMTL_TTA_LOGIT.  mode: the one the accumulator was filled with. */
#define VMTL_TTA_PROB 0
#define VMTL_TTA_LOGIT 1
int vmtl_tta_view(const float* img, int ld, float* out, int B, int H, int W, int Ho, int Wo, int flip, void* stream);
int vmtl_tta_accumulate(const float* logits, const float* depth_logits, float* acc, float* acc_depth, int B, int C,
                        int h, int w, int H, int W, int flip, float weight, float depth_gain, int mode, int first,
                        void* stream);
int vmtl_tta_finish(const float* acc, const float* acc_depth, float inv_weight, long long* segm, float* depth,
                    float* confidence, int B, int C, int H, int W, int Ho, int Wo, int mode, void* stream);

/* ---- losses ------------------------------------------------------------------------------
 * lit_module.py:31,123 (CrossEntropyLoss); losses.py:14-36 (SILogLoss); lit_module.py:68,112 (MAE). */
long long vmtl_ce_workspace_bytes(long long P);
/* element (b,c,hw) of logits / dlogits sits at [b*sb + c*sc + hw*sp] (NCHW: C*HW, HW, 1). */
int vmtl_ce_fwd(const float* logits, const long long* target, float* loss, void* workspace, int B, int HW,
                int C, long long sb, long long sc, long long sp, void* stream);
/* the same, also writing argmax_c logits per pixel (the prediction of lit_module.py:137-138) */
int vmtl_ce_fwd_argmax(const float* logits, const long long* target, float* loss, void* workspace,
                       long long* argmax, int B, int HW, int C, long long sb, long long sc, long long sp,
                       void* stream);
int vmtl_ce_bwd(const float* logits, const long long* target, const float* grad_out, float* dlogits, int B,
                int HW, int C, long long sb, long long sc, long long sp, void* stream);
/* as vmtl_ce_bwd with separate strides (dsb, dsc, dsp) for dlogits, e.g. NHWC (HW*ld, 1, ld) */
int vmtl_ce_bwd_strided(const float* logits, const long long* target, const float* grad_out, float* dlogits, int B,
                        int HW, int C, long long sb, long long sc, long long sp, long long dsb, long long dsc,
                        long long dsp, void* stream);
/* Weighted / ignoring cross entropy (torch's `weight` and `ignore_index`, reduction "mean"):
 *   loss = sum_valid w[t_i] nll_i / sum_valid w[t_i],  valid: t_i != ignore_index.
 * weight: C device floats, or null for all ones.  ignore_index: VMTL_NO_IGNORE when there is nothing to ignore.  A valid
 * pixel whose target is outside [0, C) still makes the loss (and its gradient row) NaN; with every pixel ignored the loss
 * is NaN (0/0), as in torch.  The denominator depends on the data and never visits the host: the forward leaves it in
 * `stats` (2 device floats: stats[0] = sum of weights over valid pixels, stats[1] = the weighted nll sum), the backward
 * reads stats[0].  workspace: vmtl_ce_ex_workspace_bytes(P) bytes, 8-byte aligned.  argmax: null, or the per-pixel
 * prediction as vmtl_ce_fwd_argmax writes it (for ignored pixels too).
 * Backward: dz_c = w[t] (softmax_c - 1[c == t]) grad_out / stats[0], exactly 0.0f in every written lane of an ignored
 * pixel; the same three layouts and the same written lanes as vmtl_ce_bwd_strided. */
#define VMTL_NO_IGNORE (-0x7fffffffffffffffLL - 1)
long long vmtl_ce_ex_workspace_bytes(long long P);
int vmtl_ce_fwd_ex(const float* logits, const long long* target, const float* weight, long long ignore_index,
                   float* loss, float* stats, void* workspace, long long* argmax, int B, int HW, int C, long long sb,
                   long long sc, long long sp, void* stream);
int vmtl_ce_bwd_ex(const float* logits, const long long* target, const float* weight, long long ignore_index,
                   const float* stats, const float* grad_out, float* dlogits, int B, int HW, int C, long long sb,
                   long long sc, long long sp, long long dsb, long long dsc, long long dsp, void* stream);
/* Online hard example mining (OHEM, bootstrapped cross entropy) on the weighted / ignoring cross entropy (ce_ohem.hip):
 *   nll_i = -log softmax(z_i)[t_i] (unweighted; NaN for a valid pixel with a label outside [0, C) or non-finite logits,
 *   which ranks as the hardest), K = min(min_kept_total, V) with V the number of valid pixels, kappa = the K-th largest
 *   nll among the valid pixels, cut = min(nll_thresh, kappa); kept: valid and not (nll_i < cut), ties included.
 *   loss = sum_kept w[t_i] nll_i / sum_kept w[t_i]  (NaN when V = 0).
 * nll_thresh = -log(thresh) >= 0 for a probability threshold in (0, 1] (+inf: pure top-K); min_kept_total = min_kept * B
 * >= 1.  weight, ignore_index, argmax as vmtl_ce_fwd_ex.  The selection is exact (a three-round radix select over the
 * fp32 bits of nll, integer atomics only) and neither K, the cut nor the denominator visits the host.  The forward writes
 * loss, stats (4 device floats: sum_kept w, sum_kept w nll, cut, 0), counts (2 device int64: V, kept) and nll (P floats;
 * -1 for ignored pixels).  workspace: vmtl_ce_ohem_workspace_bytes(P) bytes, 8-byte aligned.
 * Backward: dz_c = w[t] (softmax_c - 1[c == t]) grad_out / stats[0] on the kept pixels, decided from the SAVED nll and
 * stats[2]; exactly 0.0f in every written lane of every other pixel; layouts and written lanes as vmtl_ce_bwd_strided. */
long long vmtl_ce_ohem_workspace_bytes(long long P);
int vmtl_ce_ohem_fwd(const float* logits, const long long* target, const float* weight, long long ignore_index,
                     float nll_thresh, long long min_kept_total, float* loss, float* stats, long long* counts,
                     float* nll, void* workspace, long long* argmax, int B, int HW, int C, long long sb, long long sc,
                     long long sp, void* stream);
int vmtl_ce_ohem_bwd(const float* logits, const long long* target, const float* weight, long long ignore_index,
                     const float* stats, const float* nll, const float* grad_out, float* dlogits, int B, int HW, int C,
                     long long sb, long long sc, long long sp, long long dsb, long long dsc, long long dsp,
                     void* stream);
/* Cross entropy plus a Dice / Jaccard / Tversky region-overlap term (ce_region.hip).  No reference call site: the
 * multiclass DiceLoss / JaccardLoss / TverskyLoss of segmentation_models_pytorch, the library behind the reference's
 * models (vision_mtl/utils/model_utils.py:3), next to the CrossEntropyLoss of lit_module.py:31,123.  With p = softmax(z) and every
 * sum over the valid pixels (t_i != ignore_index) of the whole batch:
 *   TP_c = sum p_ic 1[t_i = c], S_c = sum p_ic, N_c = #{i valid: t_i = c},
 *   D_c = TP_c + alpha (S_c - TP_c) + beta (N_c - TP_c) + smooth,  T_c = (TP_c + smooth) / D_c,
 *   L_region = (1/C) sum_{c: N_c > 0} (1 - T_c)   (alpha = beta = 0.5: Dice; alpha = beta = 1: Jaccard),
 *   loss = ce_weight * CE + region_weight * L_region, CE as vmtl_ce_fwd_ex (weight applies to CE only).
 * alpha, beta finite > 0; smooth, ce_weight finite >= 0; region_weight finite > 0.  ce_weight == 0: CE is neither
 * evaluated nor differentiated (terms[0] = 0, stats = {0, 0}).  2 <= C <= VMTL_CE_REGION_MAX_CLASSES, else
 * VMTL_ERR_UNSUPPORTED without a launch (and 0 workspace bytes).  The forward writes loss, terms (2 device floats: CE,
 * L_region, unweighted), stats (2 floats as vmtl_ce_fwd_ex), coef (2*C floats: a_c, then b_c, with
 * dL_region/dp_ic = b_c + a_c 1[t_i = c]; exactly 0 for an absent class) and counts (C+1 int64: N_c, then the number of
 * valid pixels).  Every pixel ignored: L_region = 0 exactly, CE = NaN.  A valid label outside [0, C): loss, terms and
 * the whole of coef are NaN.  workspace: vmtl_ce_region_workspace_bytes(P, C) bytes, 8-byte aligned; weight,
 * ignore_index, argmax as vmtl_ce_fwd_ex.  Sums are fp64 per-block partials added in a fixed order (no floating-point
 * atomics): results are bit-identical run to run.
 * Backward: dz_c = grad_out [ce_weight w[t] (p_c - 1[c == t]) / stats[0] + region_weight p_c (g_c - sum_k p_k g_k)],
 * g_c = b_c + a_c 1[c == t]; exactly 0.0f in every written lane of an ignored pixel; layouts and written lanes as
 * vmtl_ce_bwd_ex. */
#define VMTL_CE_REGION_MAX_CLASSES 32
long long vmtl_ce_region_workspace_bytes(long long P, int C);
int vmtl_ce_region_fwd(const float* logits, const long long* target, const float* weight, long long ignore_index,
                       float alpha, float beta, float smooth, float ce_weight, float region_weight, float* loss,
                       float* terms, float* stats, float* coef, long long* counts, void* workspace, long long* argmax,
                       int B, int HW, int C, long long sb, long long sc, long long sp, void* stream);
int vmtl_ce_region_bwd(const float* logits, const long long* target, const float* weight, long long ignore_index,
                       const float* stats, const float* coef, const float* grad_out, float ce_weight,
                       float region_weight, float* dlogits, int B, int HW, int C, long long sb, long long sc,
                       long long sp, long long dsb, long long dsc, long long dsp, void* stream);
long long vmtl_silog_workspace_bytes(long long P);
int vmtl_silog_fwd(const float* pred, const float* target, float min_depth, float* loss, float* stats,
                   void* workspace, long long P, void* stream);
int vmtl_silog_bwd(const float* pred, const float* target, const float* stats, const float* grad_out,
                   float min_depth, float* dpred, long long P, void* stream);
/* SILog over the pixels with mask[i] != 0 (P bytes) instead of those with target > min_depth (losses.py:29-31 with a
 * mask given); same stats / workspace; masked-out pixels get gradient 0.0f */
int vmtl_silog_fwd_mask(const float* pred, const float* target, const unsigned char* mask, float* loss, float* stats,
                        void* workspace, long long P, void* stream);
int vmtl_silog_bwd_mask(const float* pred, const float* target, const unsigned char* mask, const float* stats,
                        const float* grad_out, float* dpred, long long P, void* stream);
int vmtl_l1_fwd(const float* pred, const float* target, float* loss, void* workspace, long long P, void* stream);
int vmtl_l1_bwd(const float* pred, const float* target, const float* grad_out, float* dpred, long long P,
                void* stream);

/* ---- depth loss with multi-scale gradient matching (csrc/depth_grad.hip) --------------------
 * MegaDepth's / MiDaS' scale-invariant gradient-matching term on log depth, next to SILog (no reference call site: the
 * reference's depth criterion is SILogLoss alone, losses.py:7-36).  pred, target: [B][H][W] floats.  Valid pixels: those
 * with mask[i] != 0 (B*H*W bytes), or, mask NULL, those with target > min_depth.  R = log(pred) - log(target) on valid
 * pixels.  For k < scales (1..6), s = 2^k, G_k = pixels with y % s == 0 and x % s == 0:
 *   N_k = #valid pixels of G_k (whole batch);  S_k = sum over G_k of |R(y,x+s) - R(y,x)| + |R(y+s,x) - R(y,x)|, each pair
 *   counted when its neighbour is inside the image and both pixels are valid;  L_grad = sum_k (N_k > 0 ? S_k / N_k : 0)
 *   loss = silog_weight * SILog + grad_weight * L_grad        (both weights finite and >= 0)
 * R is evaluated as ONE log of the quotient pred / target (smaller rounding than a difference of two logs); it differs from
 * log(pred) - log(target) only where the fp32 quotient under- or overflows (magnitudes 2^126 apart: no depth range).  Nothing
 * is clamped: pred < 0 on a valid pixel gives R = NaN and a NaN loss, pred == 0 gives R = -inf: NaN with SILog on, +inf
 * for the term alone, when the pixel is in a valid pair (no valid pair: the term does not see it).
 * silog_weight == 0: SILog is neither evaluated nor differentiated (terms[0], stats[1], stats[2] are 0), so the term
 * alone stays finite with fewer than two valid pixels.  H or W below a scale's step: that scale has no pair there.
 * The forward writes loss, terms (2 floats: SILog, L_grad, unweighted), stats (3 floats: SILog's N, mu, Dg), counts
 * (`scales` int64: N_k, exact) and resid (B*H*W floats: R, 0.0f at invalid pixels) in three launches: residual + SILog
 * partials, stencil partials, a one-workgroup fp64 finalize in a fixed order (run-to-run bit-identical; no float
 * atomics, no host sync).  workspace: vmtl_depth_grad_workspace_bytes(B, H, W, scales) bytes, 8-byte aligned.
 * Backward, one launch, a gather: dpred_i = grad_out * dL/dR_i / pred_i with the signs of d|.| taken from the SAVED
 * resid (0 at a tie) and 1/N_k from counts; +0.0f at invalid pixels; dpred is written for every pixel.  The validity
 * predicate is evaluated again on target / mask. */
long long vmtl_depth_grad_workspace_bytes(int B, int H, int W, int scales);
int vmtl_depth_grad_fwd(const float* pred, const float* target, const unsigned char* mask, float min_depth, int B, int H,
                        int W, int scales, float silog_weight, float grad_weight, float* loss, float* terms,
                        float* stats, long long* counts, float* resid, void* workspace, void* stream);
int vmtl_depth_grad_bwd(const float* pred, const float* target, const unsigned char* mask, float min_depth,
                        const float* resid, const float* stats, const long long* counts, const float* grad_out, int B,
                        int H, int W, int scales, float silog_weight, float grad_weight, float* dpred, void* stream);

/* ---- task-loss balancing (csrc/balance.hip) ------------------------------------------------
 * Opt-in replacements of lit_module.py:120-131 (loss = w_segm * loss_segm + w_depth * loss_depth with two host floats):
 * T = 1..4 scalar task losses L_k, given as the pointers l0..l3 (the first T non-null, in the style of vmtl_add_n), become
 * `total`, and weights_k = d total / d L_k (T floats) is kept for the backward.  Losses, param and grad_out are read by
 * pointer at run time, so a captured launch follows an optimizer step or an epoch update without a recapture.
 *   VMTL_BALANCE_UNCERTAINTY  total = sum_k exp(-s_k) L_k + s_k, s_k = log sigma_k^2 = param[k] (Kendall et al. 2018);
 *                             weights_k = exp(-s_k); d total / d s_k = 1 - exp(-s_k) L_k.  s = 0 is the reference's default.
 *   VMTL_BALANCE_DWA          total = sum_k w_k L_k, w = param (Liu et al. 2019, set by vmtl_dwa_epoch_update); with
 *                             `accumulate` the forward adds L_k to the epoch's sums in `state` and 1 to its step count -
 *                             only when every L_k is finite.  No parameter gradient.
 *   VMTL_BALANCE_GEOMETRIC    total = exp(mean_k log L_k) (Chennupati et al. 2019), weights_k = total / (T L_k); param may
 *                             be null.  A loss that is not positive makes total and every weight NaN.
 * state (DWA only; may be null without `accumulate`): vmtl_task_balance_state_bytes(T) bytes, 8-byte aligned, zeroed once
 * by the caller, 3 T + 2 doubles:
 *   [0, T) sums of L_k over the epoch's accumulated steps   [T] their number   [T + 1] completed epochs
 *   [T + 2, 2T + 2) prev: mean losses of the last completed epoch   [2T + 2, 3T + 2) prev2: of the one before
 * (a data-parallel caller sum-reduces the first T + 1 doubles over its ranks before the epoch update). */
#define VMTL_BALANCE_UNCERTAINTY 0
#define VMTL_BALANCE_DWA 1
#define VMTL_BALANCE_GEOMETRIC 2
long long vmtl_task_balance_state_bytes(int T); /* host only; 0 for T outside 1..4 */
int vmtl_task_balance_fwd(const float* l0, const float* l1, const float* l2, const float* l3, int T, int mode,
                          const float* param, void* state, int accumulate, float* total, float* weights, void* stream);
/* g_k = grad_out * weights_k (each nullable) and dparam (T floats, nullable) = grad_out * (1 - weights_k L_k) for
 * VMTL_BALANCE_UNCERTAINTY, zeros otherwise; dparam is overwritten, not accumulated.  One launch. */
int vmtl_task_balance_bwd(const float* grad_out, const float* weights, const float* l0, const float* l1, const float* l2,
                          const float* l3, const float* param, int mode, int T, float* g0, float* g1, float* g2, float* g3,
                          float* dparam, void* stream);
/* End of a training epoch (the reference has no such hook: its weights come from hyperparam_tuning.py).  mean = sums /
 * steps; prev2 <- prev, prev <- mean; completed epochs += 1; sums and step count <- 0.  From the second completed epoch on
 * param[k] = T exp(r_k / temperature) / sum_j exp(r_j / temperature) with r_k = prev_k / prev2_k, before that 1.  A step
 * count of zero changes nothing; an r_k that is not finite or not positive drops the epoch (sums and step count are
 * zeroed; param, history and the epoch count stay as they were). */
int vmtl_dwa_epoch_update(void* state, float* param, int T, float temperature, void* stream);

/* ---- per-step metrics (lit_module.py:48-69,106-118: torchmetrics Accuracy / Jaccard / FBeta) ---- */
int vmtl_confusion_matrix(const long long* pred, const long long* target, int* cm, long long P, int C,
                          void* stream);
int vmtl_segm_metrics(const int* cm, int C, float beta, float* out, void* stream);
/* the same with torchmetrics' ignore_index: pixels whose target equals it are not counted; a class in [0, C) is left out
 * of the Jaccard class mean (divide by C - 1) and has zero support in F-beta; accuracy is over the valid pixels */
int vmtl_confusion_matrix_ex(const long long* pred, const long long* target, int* cm, long long P, int C,
                             long long ignore_index, void* stream);
int vmtl_segm_metrics_ex(const int* cm, int C, float beta, long long ignore_index, float* out, void* stream);

/* ---- dataset-level evaluation metrics (csrc/eval_accum.hip) ------------
 * Opt-in; the reference only averages the per-step metrics above.  The caller owns the state, zeroes it once per epoch and
 * keeps it on the device; every evaluation step ADDS its batch to it (no allocation, no memset, no host sync in the call):
 *   cm   int64   [C][C]   confusion matrix, target row, prediction column (C <= 64)
 *   acc  float64 [16]     over the valid depth pixels, with p = max(prediction, min_depth), t = target:
 *     [0] valid-pixel count   [1] sum |p - t|   [2] sum |p - t| / t   [3] sum (p - t)^2 / t   [4] sum (p - t)^2
 *     [5] sum g^2 and [6] sum g, g = ln p - ln t   [7] sum |log10 p - log10 t|
 *     [8] [9] [10] counts of max(p / t, t / p) < 1.25, 1.25^2, 1.25^3   [11..15] reserved, left at zero
 * The prediction is clamped below at min_depth before EVERY term (Eigen-style evaluation: a prediction at or below zero
 * would make the log terms meaningless), whichever validity rule is in use.  Every term is computed in fp64 from the fp32
 * inputs (g as the fp64 log of the correctly rounded fp64 quotient p / t, |log10 p - log10 t| as |g| / ln 10).  cm and the counts are integers all the way (a count enters acc as one exact fp64 addition); the floating sums go
 * through one fp64 partial row per workgroup in `workspace` and a fixed-order fold by a single workgroup: no floating-point
 * atomics, the state after a given sequence of batches is bit-identical from run to run.
 *
 * vmtl_eval_accumulate.  Segmentation part, one of two forms (the other null), or absent (all three null):
 *   pred / target: int64, P pixels; a pixel whose target equals ignore_index (-1: none) or whose target or prediction is
 *                  outside [0, C) is skipped, as vmtl_confusion_matrix_ex does;
 *   step_cm:       a ready int32 [C][C] matrix of this step (what vmtl_confusion_matrix* built), added element-wise.
 * Depth part (absent: dpred, dtarget null): float dpred / dtarget of Pd pixels at any 4-byte alignment; a pixel is valid
 * when valid[i] != 0 (uint8, Pd bytes), or with valid null when dtarget[i] > min_depth (SILog's rule).  With a valid mask
 * the caller answers for t > 0 on the valid pixels.  workspace: vmtl_eval_accum_workspace_bytes(Pd) bytes, 8-byte aligned,
 * contents don't matter; needed by the depth part only. */
#define VMTL_EVAL_ACC_SIZE 16
long long vmtl_eval_accum_workspace_bytes(long long P); /* host only */
int vmtl_eval_accumulate(const long long* pred, const long long* target, const int* step_cm, long long P, int C,
                         long long ignore_index, const float* dpred, const float* dtarget, const unsigned char* valid,
                         float min_depth, long long Pd, long long* cm, double* acc, void* workspace, void* stream);
/* State -> metrics, one single-workgroup launch.  out: float64 [16]
 *   [0] pixel accuracy  [1] mean class accuracy  [2] mIoU  [3] F-beta, support weighted
 *   [4] abs_err = E|p - t|  [5] rel_err = E|p - t| / t  [6] sq_rel = E (p - t)^2 / t  [7] rmse  [8] rmse_log = sqrt(E g^2)
 *   [9] log10 = E|log10 p - log10 t|  [10] silog = sqrt(max(E g^2 - (E g)^2, 0))  [11] [12] [13] delta1..3 (fractions)
 *   [14] n_valid (depth pixels)  [15] n_pixels (the sum of cm)
 * iou: float64 [C], per-class intersection over union.
 * The two class means run over the classes whose union tp + fp + fn (mIoU), or support (mean accuracy), is non-zero, and
 * never over a class named by ignore_index; iou[c] is NaN for a class left out.  This is the convention of the Cityscapes
 * evaluation scripts and of MTAN's ConfMatrix, and it DIFFERS ON PURPOSE from the per-step Jaccard of vmtl_segm_metrics,
 * which (as torchmetrics' absent_score = 0) scores an absent class 0: over a whole evaluation set an absent class says
 * nothing about the model, within one batch the reference counts it.  Pixel accuracy and F-beta are over all of cm (the row
 * of an ignored class is empty when cm was built with the same ignore_index).  [0..3] and iou are NaN when cm is all zero,
 * [4..13] are NaN when acc[0] == 0; nothing divides by zero. */
int vmtl_eval_finalize(const long long* cm, const double* acc, int C, float beta, long long ignore_index, double* out,
                       double* iou, void* stream);

/* ---- optimizer (training_lit.py:51,87: torch.optim.Adam) ---------------------------------- */
int vmtl_adam_step(float* p, const float* g, float* m, float* v, const float* step_ptr, float lr, float b1,
                   float b2, float eps, float weight_decay, float grad_scale, long long n, void* stream);

/* ---- global-norm clipping + extended Adam / AdamW (csrc/optim.hip) ------------------------
 * Flat fp32 buffers of n >= 1 elements, any 4-byte-aligned pointers.  `workspace`: vmtl_grad_sumsq_workspace_bytes(n)
 * bytes, 8-byte aligned.  `ctl`: the control block, 16 floats, zeroed once by the caller:
 *   [0] total norm of g * grad_scale (NaN when no norm was computed)  [1] clip coefficient
 *   [2] the norm is not finite  [3] this step is skipped  [4] running count of skipped steps
 *   [5..10] bias corrections and betas for vmtl_adam_step_ex  [11..15] unused
 * A beta is passed as the fp32 pair (hi, lo) with hi + lo == the double value.  max_norm 0: no clipping. */
long long vmtl_grad_sumsq_workspace_bytes(long long n);
/* per-workgroup fp64 partial sums of (g[i] * grad_scale)^2 into workspace; deterministic, no atomics */
int vmtl_grad_sumsq(const float* g, float grad_scale, void* workspace, long long n, void* stream);
/* partials -> ctl (norm, torch's clip coefficient min(1, max_norm / (norm + 1e-6)), flags); step_ptr[0] += 1 on the
 * device unless skip_nonfinite is set and the norm is not finite (then ctl[4] += 1).  n: the element count workspace was
 * filled for; n == 0 (workspace may be null): no norm, clipping and skip_nonfinite are then refused */
int vmtl_optim_control(const void* workspace, long long n, float max_norm, int skip_nonfinite, float* step_ptr,
                       float b1, float b1_lo, float b2, float b2_lo, float* ctl, void* stream);
/* torch.optim.Adam (decoupled 0: g += wd * p) / AdamW (decoupled 1: p *= 1 - lr * wd) with the gradient read as
 * g * grad_scale * ctl[1]; lr_ptr (nullable) overrides lr; a skipped step (ctl[3]) leaves p, m and v untouched; g is
 * never written.  Runs after vmtl_optim_control on the same stream */
int vmtl_adam_step_ex(float* p, const float* g, float* m, float* v, const float* ctl, float lr,
                      const float* lr_ptr, float eps, float weight_decay, int decoupled, float grad_scale,
                      long long n, void* stream);
/* g *= grad_scale * clip coefficient in place, after vmtl_grad_sumsq with the same grad_scale and n; writes ctl[0..2] */
int vmtl_grad_clip_(float* g, const void* workspace, float grad_scale, float max_norm, float* ctl, long long n,
                    void* stream);

/* ---- averaged weights: EMA / SWA over flat fp32 buffers (csrc/weight_avg.hip) -------------
 * `state`: the state block, 8 four-byte words, 8-byte aligned, zeroed once by the caller:
 *   [0..1] n_averaged (one 64-bit integer)  [2] the weight w of this update  [3] this update copies
 *   [4] this update is skipped  [5] running count of skipped updates  [6..7] unused
 * Other pointers need 4-byte alignment only. */
#define VMTL_WAVG_EMA 0
#define VMTL_WAVG_SWA 1
/* One workgroup.  ctl (nullable): an optimizer control block; when ctl[3] (its step was skipped) is set, this update is
 * skipped too: state[4] = 1, the counter stays.  Otherwise state[2] = w, state[3] = (n_averaged == 0), state[4] = 0 and
 * n_averaged += 1, with w computed in fp64 from n = n_averaged before the increment and rounded once:
 *   n == 0: 1 (and the copy flag)   VMTL_WAVG_SWA: 1 / (n + 1)
 *   VMTL_WAVG_EMA: 1 - d, d = decay + decay_lo (the fp32 pair of a double in [0, 1]); with warmup != 0
 *   d = min(d, (1 + n) / (10 + n)) */
int vmtl_wavg_control(float* state, const float* ctl, int mode, float decay, float decay_lo, int warmup,
                      void* stream);
/* e[i] = fma(w, p[i] - e[i], e[i]), or e[i] = p[i] on the copy flag; nothing is written on the skip flag; p is only read */
int vmtl_wavg_update(float* e, const float* p, const float* state, long long n, void* stream);
/* vmtl_adam_step_ex, then vmtl_wavg_update of the new p into e, in one pass and with the same bits as the two launches */
int vmtl_adam_step_wavg(float* p, const float* g, float* m, float* v, float* e, const float* ctl,
                        const float* state, float lr, const float* lr_ptr, float eps, float weight_decay,
                        int decoupled, float grad_scale, long long n, void* stream);
/* descs: device array of n records {float* src; float* avg; long long count} (vmtl_wavg_desc_bytes() each, 8-byte
 * aligned, 1 <= n <= 65535), count <= max_n, written and validated by the host; one launch for all records.
 * vmtl_wavg_buffers: avg <- the update above with src as p.  vmtl_swap_table_: src <-> avg, bit for bit. */
int vmtl_wavg_desc_bytes(void);
int vmtl_wavg_buffers(const void* descs, int n, long long max_n, const float* state, void* stream);
int vmtl_swap_table_(const void* descs, int n, long long max_n, void* stream);
/* a <-> b in place, moved as integers (NaN payloads survive); overlapping ranges are refused with VMTL_ERR_ARG */
int vmtl_swap_(float* a, float* b, long long n, void* stream);

/* ---- two-task gradient surgery on a pair of fp32 gradients (csrc/surgery.hip) -------------
 * PCGrad (Yu et al. 2020), the two-point MGDA min-norm solution (Sener & Koltun 2018) and the gradient part of IMTL-G
 * (Liu et al. 2021) need the 2x2 Gram matrix of the two per-task gradients and nothing else.  a and b are `rows` rows
 * of `width` floats with leading dimensions lda, ldb >= width (in floats): two maps, two flat buffers (rows 1), or the
 * two halves of one interleaved [rows][2*Cs] map (b = a + Cs, lda = ldb = 2*Cs).  Pointers need 4-byte alignment; the
 * 16-byte body is taken when pointers, width and leading dimensions allow it, a scalar body otherwise.
 * `state`: 12 four-byte words, 8-byte aligned, zeroed once by the caller:
 *   [0] n_a = <a,a>  [1] d = <a,b>  [2] n_b = <b,b>  [3] alpha  [4] beta  [5] cosine d / sqrt(n_a n_b)  [6..7] unused
 *   [8..9] steps seen (one 64-bit integer)  [10..11] steps with d < 0 (one 64-bit integer) */
#define VMTL_SURGERY_STATE_FLOATS 12
#define VMTL_SURGERY_SUM 0    /* alpha = beta = 1: Gram matrix, cosine and counters only */
#define VMTL_SURGERY_PCGRAD 1 /* d < 0: alpha = 1 - d / n_a, beta = 1 - d / n_b; else 1, 1 */
#define VMTL_SURGERY_MGDA 2   /* alpha = clip((n_b - d) / (n_a - 2 d + n_b), 0, 1) (0.5 when that denominator is <= 0), beta = 1 - alpha */
#define VMTL_SURGERY_IMTL_G 3 /* alpha = sqrt(n_b) / (sqrt(n_a) + sqrt(n_b)), beta = 1 - alpha */
long long vmtl_surgery_workspace_bytes(long long rows, long long width); /* host only; 0 for a bad shape */
/* per-workgroup partial sums of a*a, a*b, b*b into workspace (8-byte aligned): products and sums in fp64, fixed order,
 * no atomics */
int vmtl_surgery_gram(const float* a, long long lda, const float* b, long long ldb, long long rows, long long width,
                      void* workspace, void* stream);
/* One workgroup.  Folds the partials of vmtl_surgery_gram(rows, width) in fp64, stores the Gram matrix as fp32, derives
 * (alpha, beta) in fp64 FROM THOSE fp32 VALUES and rounds them once; steps += 1, conflicts += 1 when d < 0.
 * n_a == 0, n_b == 0 (fp32 underflow included) or a Gram entry that is not finite: alpha = beta = 1 for every method,
 * cosine = 0, the conflict counter stays.  An unknown method returns -3 without a launch. */
int vmtl_surgery_control(const void* workspace, long long rows, long long width, int method, float* state,
                         void* stream);
/* out[r][c] = alpha * a[r][c] + beta * b[r][c], evaluated in fp64 and rounded to fp32 once, for c < width, alpha = state[3],
 * beta = state[4]; ldo >= width.
 * out may be a (same pointer, ldo == lda); any other overlap of out with a or b (elements, not byte ranges: the
 * interleaved halves of one map do not overlap) returns -1.  Lanes [width, ldo) of out are LEFT ALONE: in the interleaved layout they
 * hold b. */
int vmtl_surgery_combine(const float* a, long long lda, const float* b, long long ldb, const float* state, float* out,
                         long long ldo, long long rows, long long width, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VMTL_H */
