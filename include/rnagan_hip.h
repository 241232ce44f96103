/* rnagan_hip.h -- C ABI of librnagan_hip.so: the MI355X (gfx950) kernels behind the RNA-GAN
 * WGAN-GP training path.
 *
 * The reference (gevaertlab/RNA-GAN) has no native code; its hot path reaches native kernels only
 * through PyTorch ATen/cuDNN/cuBLAS calls made from Python.  Each entry point below replaces one
 * such implicit native op (SURVEY.md 2.2 "native-op inventory", K1..K15) and cites the reference
 * call site (paths relative to /root/reference) whose arithmetic it provides.  The Python side
 * (rna_gan_amd/_abi.py, ctypes) binds exactly these symbols; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); the library never
 *     allocates, frees or retains memory.  Workspace is passed in (rg_*_workspace_bytes).
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises.
 *     Safe under HIP graph capture.  Re-entrant; no global mutable state except the thread-local
 *     error string.
 *   - return value: 0 = RG_OK, <0 = error (rg_last_error() gives the text).  Launch errors are
 *     detected with hipGetLastError() only.
 *   - activations: NHWC ([N][H][W][C], C fastest) in `dtype` = RG_F32 or RG_BF16; arithmetic and
 *     all per-channel statistics are fp32.  Image-side boundary tensors (discriminator input,
 *     generator output) are NCHW fp32 exactly as in PyTorch.
 *   - a 4x4 / stride-2 / pad-1 conv weight is w[O][I][4][4] fp32 (PyTorch memory layout), where
 *     O = channels on the LOW-resolution side and I = channels on the HIGH-resolution side: this is
 *     nn.Conv2d.weight (out,in,kh,kw) in the discriminator and nn.ConvTranspose2d.weight
 *     (in,out,kh,kw) in the generator, so "down"/"up" serve both networks and each other's backward.
 *   - `algo`: RG_ALGO_AUTO picks the MFMA implicit-GEMM kernels when dtype is bf16 and the shape
 *     is tile-aligned, else the generic tiled fp32 kernels; RG_ALGO_GENERIC / RG_ALGO_MFMA force one
 *     (MFMA returns RG_EUNSUPPORTED for shapes it cannot take).
 */
#ifndef RNAGAN_HIP_H
#define RNAGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_OK 0
#define RG_EINVAL (-1)
#define RG_EUNSUPPORTED (-2)
#define RG_EWORKSPACE (-3)
#define RG_EHIP (-4)

#define RG_F32 0
#define RG_BF16 1
#define RG_U8 3    /* unsigned 8-bit image samples: a SOURCE type only (rg_resize_bilinear01, rg_tile_transform) */
#define RG_F16 2   /* IEEE fp16 storage: librnagan_hip_f16.so only (the same sources built with -DRG_HALF_F16; see "fp16 build" below) */

#define RG_ALGO_AUTO 0
#define RG_ALGO_GENERIC 1
#define RG_ALGO_MFMA 2

int rg_version(void);
const char* rg_last_error(void);
/* Kernel-selection knobs for A/B measurements inside one process (tools/, tests/): name = the part of the matching
 * environment variable after "RNAGAN_", lower case ("conv8", "conv8_blocks", "conv_tile", "xcd", "class_fast",
 * "wgrad_blocks", "wgrad8", ..., "f32mma": 0 sends the RG_F32 conv / dense launches back to the vector-ALU GEMM instead of the
 * f32 matrix-core one, 1 keeps every such launch on the f32 matrix instruction, 2 (the default) lets their 128 x 128-tile launches
 * form every fp32 product as six bf16 matrix-core products of the operands' exact three-way bf16 splits (fp32-grade accuracy,
 * ~11 % faster fp32 iteration); "wslab16": 0 keeps the deferred
 * weight-gradient slabs fp32; "bn_rev": which BatchNorm row passes walk their rows from the end (bit 2, the default: reductions); "convd": 0 sends the 64 -> 128 channel stride-2 conv back from the parity-plane-resident kernel to the
 * implicit-GEMM one, "convd_blocks": its persistent grid; "slab16": 0 keeps the split-K partial tiles of the conv launches fp32 (the fp16 build's default; 1 is unsupported there);
 * "skinny128": 0 sends the image-side layers of 256 x 256 images back
 * from the control-flow-free row kernels to the general row-staged ones; "wgrad8_mfma": 32 (default) / 16 = the matrix instruction
 * shape of the 256 x 256-tile weight-gradient kernel, bit-identical results; "narrow32": 0 sends 3 x 3 convs of <= 32 output columns
 * back to the kernel that issues MFMAs for all 64 columns of its tile; "upimg": 0 sends the resize-convolution generator's image
 * block back to the path that materialises its upsampled + padded input, "upimg_blocks": the fused kernel's grid).  An option set here
 * overrides the environment; value < 0 clears the override.  Returns RG_EINVAL for an
 * unknown name.  Not thread-safe against concurrent launches. */
int rg_set_option(const char* name, int value);

/* ---------------------------------------------------------------------------------------------
 * Stride-2 4x4 convolution family (K1/K2/K3 of SURVEY 2.2)
 * ------------------------------------------------------------------------------------------- */

/* Weight layout of this family: fp32 masters and gradients are TAP-MAJOR, w[O][4][4][I] (O = channels on the
 * low-resolution side, I = on the high-resolution side), i.e. nn.Conv2d's weight[O][I][kh][kw] /
 * nn.ConvTranspose2d's weight[O][I][kh][kw] with the dimensions permuted (0,2,3,1).  The host side keeps the
 * nn.Parameter as a strided view of this storage, so state_dicts and checkpoints still show the PyTorch shape.
 * With this order the bf16 GEMM operand of rg_conv_down is an element-wise cast of the master and rg_conv_wgrad
 * writes dw without a permuting pass.
 *
 * bf16 operand images for the MFMA kernels (either output may be NULL):
 *   wdn[O][16][I]  (B operand of rg_conv_down: k = (tap, i) contiguous in i) = cast of w
 *   wup[16][I][O]  (B operand of rg_conv_up:   k = (tap, o) contiguous in o) = transpose of w as [O][16*I]
 * both in `dtype`.  Runs after every optimizer step (src/wgan_loss.py:127,261,388). */
int rg_pack_conv_weight(const float* w, void* wdn, void* wup, int O, int I, int dtype, void* stream);
/* The same wup / G.0 operand images built from the bf16 copy of the masters that rg_adam_step_dev(shadow_bf16) keeps
 * (2-byte instead of 4-byte reads; w_bf16 is [O][16][I] resp. [E][C][16], the master's order). */
int rg_pack_conv_wup_from_bf16(const void* w_bf16, void* wup, int O, int I, void* stream);
/* the same for n <= 8 layers in ONE launch (arrays of n pointers / sizes on the host): every layer needs O % 64 == 0,
 * 16 * I % 128 == 0 and 16-byte aligned buffers, else RG_EUNSUPPORTED (use the single-layer call) */
int rg_pack_conv_wup_from_bf16_multi(int n, const void* const* w_bf16, void* const* wup, const int* O, const int* I, void* stream);
int rg_pack_g0_weight_from_bf16(const void* w_bf16, void* wp, int E, int C, void* stream);

/* y[N][Hi/2][Wi/2][O] = conv2d(x[N][Hi][Wi][I], w[O][4][4][I], stride 2, pad 1).
 * nn.Conv2d forward in the discriminator (D(.) at src/wgan_loss.py:119,241,253,379) and the
 * data-gradient of nn.ConvTranspose2d in the generator (loss.backward(), :126).
 * `wdn` may be NULL when the generic kernel runs (it reads `w`).
 * stats_partial (may be NULL): when the layer is followed by a train-mode BatchNorm, the MFMA epilogue also writes
 * per-tile column sums of y and y^2 (of the bf16 values as stored), fp32 [rows][2][O] with
 * rows = rg_conv_stats_rows(...) (0: this shape takes split-K or the generic kernel -- pass NULL and use
 * rg_bn_forward).  rg_bn_forward_partials finishes them: the separate statistics pass over y disappears. */
int rg_conv_stats_rows(int up, int N, int Hlow, int Wlow, int O, int I, int dtype, int algo);
int rg_conv_down(const void* x, const float* w, const void* wdn, void* y, int N, int Hi, int Wi, int I,
                 int O, float* stats_partial, int dtype, int algo, void* ws, size_t ws_bytes, void* stream);
/* workspace of rg_conv_down (up = 0) / rg_conv_up (up = 1): split-K partial slabs for layers whose tile
 * grid cannot fill the chip (few rows, long K); Hlow/Wlow = low-resolution side.  May be 0. */
size_t rg_conv_workspace_bytes(int up, int N, int Hlow, int Wlow, int O, int I, int dtype, int algo);

/* y[N][2Ho][2Wo][I] = conv_transpose2d(x[N][Ho][Wo][O], w[O][4][4][I], stride 2, pad 1).
 * nn.ConvTranspose2d forward in the generator (G(.) at src/wgan_loss.py:113,247,371) and the
 * data-gradient of nn.Conv2d in the discriminator (.backward() :126,260,387; autograd.grad :34-41).
 * mask_act (may be NULL): an activation tensor with y's shape and dtype; then y *= (mask_act > 0 ? 1 : mask_slope),
 * i.e. the LeakyReLU backward of the layer below is applied in the epilogue (the data-gradient of discriminator
 * layer 1 feeding layer 0's LeakyReLU) instead of in a separate pass over y. */
int rg_conv_up(const void* x, const float* w, const void* wup, void* y, int N, int Ho, int Wo, int O, int I,
               const void* mask_act, float mask_slope, float* stats_partial, int dtype, int algo, void* ws,
               size_t ws_bytes, void* stream);

/* dw[O][kh][kw][I] (+)= sum_{n,ho,wo} low[n][ho][wo][o] * high[n][2ho-1+kh][2wo-1+kw][i].
 * Weight gradient of both layer kinds (every .backward()).  Deterministic: split-K partial slabs
 * in `ws` are summed in a fixed order. */
size_t rg_conv_wgrad_workspace_bytes(int N, int Ho, int Wo, int O, int I, int dtype, int algo);
int rg_conv_wgrad(const void* low, const void* high, float* dw, int N, int Ho, int Wo, int O, int I, int dtype,
                  int accumulate, int algo, void* ws, size_t ws_bytes, void* stream);
/* Two contributions of the same layer in one launch: dw (+)= wgrad(low0, high0) + wgrad(low1, high1).
 * Used where the reference's autograd accumulates two backward passes into one .grad: D(real) + D(fake)
 * in the discriminator step (wgan_loss.py:241-260) and primal + tangent in the penalty step (:379-387).
 * Same workspace as rg_conv_wgrad. */
int rg_conv_wgrad2(const void* low0, const void* high0, const void* low1, const void* high1, float* dw, int N,
                   int Ho, int Wo, int O, int I, int dtype, int accumulate, int algo, void* ws, size_t ws_bytes,
                   void* stream);
/* rg_conv_wgrad (low1 = high1 = NULL) / rg_conv_wgrad2 with the split-K reduction LEFT TO THE CALLER'S OPTIMIZER STEP
 * (.backward() directly followed by optimizer.step(), src/wgan_loss.py:126-127, :260-261, :387-388): a plan with
 * *nsplit_out > 1 leaves its fp32 partial slabs [nsplit][O][16][I] in `slab` (>= rg_conv_wgrad_workspace_bytes, caller-owned,
 * must stay untouched until rg_adam_step_slabs has consumed it; *slab_dtype_out says whether the partial tiles are fp32 or
 * bf16 -- option wslab16, default bf16: each partial sum rounded once, added in fp32) and does not write dw; *nsplit_out == 1: dw was written
 * (not accumulated) and nothing is pending -- also the outcome for every shape / dtype the matrix-core kernel does not take
 * (the generic kernel runs with `slab` as its workspace). */
int rg_conv_wgrad_slabs(const void* low0, const void* high0, const void* low1, const void* high1, float* dw, int N, int Ho,
                        int Wo, int O, int I, int dtype, int algo, void* slab, size_t slab_bytes, int* nsplit_out,
                        int* slab_dtype_out, void* stream);
/* The same pair of calls (weight gradient, then optimizer.step()) as ONE launch for a layer whose plan has no split-K: the
 * gradient tile is never written -- the kernel's epilogue applies the Adam update (the arithmetic of rg_adam_step_dev, bit for
 * bit) to the tensor's fp32 master p, moments m, v and optional bf16 operand image, all tap-major [O][16][I] like dw.
 * hyper = the 8 constants rg_adam_hyper_dev wrote for THIS step.  26 bytes per parameter instead of 4 + 30.
 * rg_conv_wgrad_adam_supported: 1 when the shape / dtype has such a plan (bf16, 256 | O, 16 | I, no split-K at this pixel
 * count); the caller's streaming step then leaves the tensor out (rg_adam_step_slabs, seg_nsplit = -1). */
int rg_conv_wgrad_adam_supported(int N, int Ho, int Wo, int O, int I, int two, int dtype, int algo);
int rg_conv_wgrad_adam(const void* low0, const void* high0, const void* low1, const void* high1, float* p, float* m, float* v,
                       const float* hyper, void* shadow_bf16, int N, int Ho, int Wo, int O, int I, int dtype, int algo,
                       void* stream);

/* Image-side layers (I = 3 channels, NCHW fp32 on the high-resolution side; HBM-bound).  Their weights keep
 * the PyTorch layout w[O][I][4][4] (48 values per O).
 * rg_first_down: y[N][H/2][W/2][O] = lrelu_slope(conv2d(x_nchw, w) + bias); bias may be NULL,
 *   slope = 1 disables the activation.  Discriminator layer 0 forward
 *   (Conv2d(3,64,4,2,1)+LeakyReLU, histopathology_gan.py:186-192) and data-gradient of the
 *   generator's last ConvTranspose2d.
 * rg_last_up: y_nchw[N][I][2Ho][2Wo] = act(conv_transpose2d(x, w) + bias), act = tanh or none.
 *   Generator last layer forward (ConvTranspose2d(64,3,4,2,1)+Tanh, dcgan.py:82) and
 *   data-gradient of discriminator layer 0 (gives d/d xhat for the penalty, wgan_loss.py:34-41).
 * rg_skinny_wgrad: weight gradient of those two layers. */
int rg_first_down(const float* x_nchw, const float* w, const float* bias, void* y, int N, int H, int W, int I,
                  int O, float slope, int dtype, void* stream);
int rg_last_up(const void* x, const float* w, const float* bias, float* y_nchw, int N, int Ho, int Wo, int O,
               int I, int apply_tanh, int dtype, void* stream);
/* Packed LeakyReLU mask of the discriminator's layer 0 (histopathology_gan.py:186-192) for the data-gradient conv of
 * layer 1 (.backward() at src/wgan_loss.py:126,260,387 and autograd.grad :34-41): bits[pixel] (uint64, pixel = NHWC row of
 * y) has bit c set when y[pixel][c] > 0 (the bf16 value as stored).  rg_first_down_bits = rg_first_down + those bits
 * (O = 64, bf16; written by the same kernel); rg_sign_pack computes them from an existing activation [npix][64].
 * rg_conv_up_maskbits = rg_conv_up with mask_act given in this packed form (8 B instead of 128 B per output pixel, and the
 * kernel that keeps the input patch resident in LDS); rg_conv_up_maskbits_supported tells whether the shape takes it
 * (O = 128 -> I = 64 channels, Wo in {16, 32, 64}); otherwise use rg_conv_up with the activation itself. */
int rg_first_down_bits(const float* x_nchw, const float* w, const float* bias, void* y, void* bits, int N, int H, int W,
                       int I, int O, float slope, int dtype, void* stream);
int rg_sign_pack(const void* a, void* bits, long long npix, int C, int dtype, void* stream);
/* y = lrelu'(a) * conv2d(x_nchw, w) (no bias), lrelu'(a) taken from a's packed sign bits: the tangent of discriminator
 * layer 0 in the penalty's forward-mode pass (second-order term of src/wgan_loss.py:32-44) in one kernel.
 * rg_first_down_masked_supported == 0: use rg_first_down(slope 1) + rg_lrelu_bwd instead. */
int rg_first_down_masked_supported(int H, int W, int I, int O, int dtype);
int rg_first_down_masked(const float* x_nchw, const float* w, void* y, const void* mask_bits, float mask_slope, int N,
                         int H, int W, int I, int O, int dtype, void* stream);
int rg_conv_up_maskbits_supported(int N, int Ho, int Wo, int O, int I, int dtype, int algo);
int rg_conv_up_maskbits(const void* x, const void* wup, void* y, int N, int Ho, int Wo, int O, int I,
                        const void* mask_bits, float mask_slope, int dtype, int algo, void* ws, size_t ws_bytes,
                        void* stream);
/* rg_last_up (no bias, no activation) with the FIRST CONSUMER's pass over its fp32 NCHW output fused into the store phase:
 *   tanh_img (optional, shape of y): y *= 1 - tanh_img^2 -- in the generator-loss step the data gradient of the
 *     discriminator's layer 0 is the cotangent of the generator's Tanh output (.backward() at src/wgan_loss.py:126 through
 *     nn.Tanh, src/dcgan.py:82): rg_tanh_bwd's arithmetic without materialising the unmultiplied gradient;
 *   part (optional): float[rg_last_up_post_blocks(...)][4], one row per workgroup = sums over the rows it wrote of channel
 *     0, 1, 2 of y and of y^2.  rg_last_up_part_chan_sum adds the rows up into the bias gradient of the generator's last
 *     ConvTranspose2d (out3[c] (+)= sum); rg_gp_coef_parts into the penalty's squared norm ||d D(xhat) / d xhat||^2 over the
 *     WHOLE batch (src/wgan_loss.py:34-43: gradients.norm(2) of the flattened (N, -1) tensor), from which it writes loss =
 *     (norm - 1)^2 and coef = lambd * 2 (norm - 1) / norm as rg_gp_coef does (sq, optional, receives the squared norm).
 *   Fixed summation order: deterministic.  rg_last_up_post_blocks == 0: no such kernel for the shape (use rg_last_up +
 *   rg_tanh_bwd / rg_nchw_chan_sum / rg_sqnorm). */
int rg_last_up_post_blocks(int N, int Ho, int Wo, int O, int I, int dtype);
int rg_last_up_post(const void* x, const float* w, float* y_nchw, int N, int Ho, int Wo, int O, int I, int dtype,
                    const float* tanh_img, float* part, void* stream);
int rg_last_up_part_chan_sum(const float* part, int nblocks, float* out3, int accumulate, void* stream);
int rg_gp_coef_parts(const float* part, int nblocks, float* sq, float* loss, float* coef, float lambd, void* stream);
/* the same when the gradient whose squared norm the partials hold carries a loss scale (fp16 build): norm = sqrt(sum) / in_scale,
 * loss from that norm, coef = lambd * 2 (norm - 1) / norm * out_scale / in_scale -- the tangent direction coef * g' then carries
 * out_scale.  Scales are powers of two (exact); with in_scale = out_scale = 1 this is rg_gp_coef_parts bit for bit. */
int rg_gp_coef_parts_scaled(const float* part, int nblocks, float* sq, float* loss, float* coef, float lambd, float in_scale,
                            float out_scale, void* stream);
/* ... with in_scale = 2^floor(k/2), out_scale = 2^(k - floor(k/2)) for the exponent latched for `slot` (rg_amp_latch) */
int rg_gp_coef_parts_scaled_dev(const float* part, int nblocks, float* sq, float* loss, float* coef, float lambd,
                                const int* amp_state, int slot, void* stream);
/* rg_last_up with the generator's last train-mode BatchNorm + LeakyReLU applied to its input on the fly (z = the pre-BatchNorm
 * conv output; mean / invstd from rg_bn_finalize_partials or rg_bn_stats_finalize): the no-grad generator forwards of the
 * D-loss and penalty steps (src/wgan_loss.py:247,371) skip the normalisation pass over their largest activation.  Same bf16
 * rounding as rg_bn_act followed by rg_last_up.  rg_last_up_pre_supported == 0: use those two. */
int rg_last_up_pre_supported(int Wo, int O, int I, int dtype);
int rg_last_up_pre(const void* z, const float* w, const float* bias, float* y_nchw, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, float slope, int N, int Ho, int Wo, int O, int I, int apply_tanh,
                   int dtype, void* stream);
/* rg_skinny_wgrad / rg_skinny_wgrad_bias take a workspace of at least rg_skinny_wgrad_workspace_bytes (RG_EWORKSPACE, nothing
 * launched, with one byte less -- whichever kernel the shape takes). */
size_t rg_skinny_wgrad_workspace_bytes(int N, int Ho, int Wo, int O, int I);
int rg_skinny_wgrad(const void* low, const float* high_nchw, float* dw, int N, int Ho, int Wo, int O, int I,
                    int dtype, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* rg_skinny_wgrad with the reduction of its per-workgroup partial gradients LEFT to the optimizer step that follows at once
 * (src/wgan_loss.py:126-127, :260-261, :387-388): `slab` receives *nslab_out fp32 slabs of O * 48 elements in dw's layout
 * (at most rg_skinny_wgrad_workspace_bytes), to be handed to rg_adam_step_slabs as that tensor's segment; a second contribution
 * to the same tensor (D(real) + D(fake), primal + tangent) is a second call with `slab` advanced by the first call's slabs.
 * *nslab_out = 0: this shape / dtype has no such form and nothing was launched. */
int rg_skinny_wgrad_slabs(const void* low, const float* high_nchw, int N, int Ho, int Wo, int O, int I, int dtype, void* slab,
                          size_t slab_bytes, int* nslab_out, float* bias_slab, int* bias_done_out, void* stream);
/* rg_skinny_wgrad that also forms the layer's bias gradient dbias[O] = sum over the pixels of `low` (what autograd adds to
 * Conv2d(3, 64).bias.grad, histopathology_gan.py:186-192) as a by-product of its pass over `low` where the kernel can (a column of
 * ones in the patch operand of the 256 x 256 bf16 row kernel): *bias_done_out = 1; otherwise 0 and dbias is untouched (rg_col_sum
 * then).  bias_accumulate: add to dbias.  rg_skinny_wgrad_slabs' bias_slab / bias_done_out: the same by-product as partials
 * [*nslab_out][O] for the optimizer step (a segment of rg_adam_step_slabs). */
int rg_skinny_wgrad_bias(const void* low, const float* high_nchw, float* dw, float* dbias, int N, int Ho, int Wo, int O, int I,
                         int dtype, int accumulate, int bias_accumulate, void* ws, size_t ws_bytes, int* bias_done_out,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense layers: generator layer 0 (K4), discriminator head (K5), betaVAE encoder (K8)
 * ------------------------------------------------------------------------------------------- */

/* Generator layer 0, ConvTranspose2d(E,C,4,1,0) on a 1x1 input (dcgan.py:38-40):
 *   y[N][4][4][C] = sum_e z[n][e] * w[e][c][kh][kw].   w is [E][C][4][4] fp32;
 *   wp = packed [16*C][E] in dtype (rg_pack_g0_weight), NULL for the generic kernel. */
int rg_pack_g0_weight(const float* w, void* wp, int E, int C, int dtype, void* stream);
int rg_g0_fwd(const float* z, const float* w, const void* wp, void* y, int N, int E, int C, int dtype, int algo,
              void* ws, size_t ws_bytes, void* stream);
size_t rg_g0_workspace_bytes(int N, int E, int C, int dtype, int algo);
int rg_g0_wgrad(const float* z, const void* gy, float* dw, int N, int E, int C, int dtype, int accumulate,
                int algo, void* ws, size_t ws_bytes, void* stream);

/* Discriminator head, Conv2d(C,1,4,1,0)+LeakyReLU on a 4x4 map -> (N,):
 *   h[n] = sum a[n][kh][kw][c] * w[0][c][kh][kw];  out[n] = lrelu(h[n]). */
int rg_head_fwd(const void* a, const float* w, float* h, float* out, int N, int C, float slope, int dtype,
                void* stream);
/* the same with the head's bias (DCGANDiscriminator(batchnorm=False)): h[n] = <a[n], w> + bias[0], added inside the kernel */
int rg_head_fwd_bias(const void* a, const float* w, const float* bias, float* h, float* out, int N, int C, float slope,
                     int dtype, void* stream);
/* out[0] (+)= sum_i x[i], fixed order (the head's bias gradient sum_n gh[n]) */
int rg_vec_sum(const float* x, int n, float* out, int accumulate, void* stream);
/* gh[n] = coef * lrelu'(h[n])  (coef = d loss / d out[n]: -1/N, +1/N or 1; wgan_loss.py:24-29,33) */
int rg_head_grad(const float* h, float* gh, int N, float coef, float slope, void* stream);
/* the same with coef * 2^e, e from the exponent latched for `slot` (rg_amp_latch): part 0: e = k, 1: floor(k / 2) (the penalty's
 * first backward), 2: k - floor(k / 2) */
int rg_head_grad_dev(const float* h, float* gh, int N, float coef, const int* amp_state, int slot, int part, float slope,
                     void* stream);
int rg_head_bwd_data(const float* gh, const float* w, void* ga, int N, int C, int dtype, void* stream);
int rg_head_wgrad(const float* gh, const void* a, float* dw, int N, int C, int dtype, int accumulate,
                  void* stream);

/* y[M][ldy] = act((x[M][K] . w[Nout][K]^T) * scale[j] + shift[j]) : Linear + BatchNorm1d(eval)
 * folded + LeakyReLU(0.01) of the betaVAE encoder, and z_mu (betaVAE.py:26-42,102-107).
 * x is fp32 [M][ldx]; w fp32 [Nout][K] (PyTorch Linear layout); y fp32. slope=1: no activation.
 * wp: optional bf16 copy of w padded to [Nout_pad][K_pad] (rg_pack_linear_weight) for the MFMA
 * kernel (weight streaming is the bound: 2 B/weight instead of 4). */
int rg_pack_linear_weight(const float* w, void* wp, int Nout, int K, int Nout_pad, int K_pad, void* stream);
size_t rg_linear_workspace_bytes(int M, int K, int Nout, int algo);
int rg_linear_affine_act(const float* x, int ldx, const float* w, const void* wp, const float* scale,
                         const float* shift, float* y, int ldy, int M, int K, int Nout, float slope, int algo,
                         void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d in TRAIN mode + LeakyReLU: forward, backward, forward-mode tangent and the joint
 * (double) backward needed by the gradient penalty (K6/K7).  z, a, g* are [M][C] views of NHWC
 * tensors (M = N*H*W).  All column reductions are two-stage and deterministic; `ws` must hold
 * rg_colreduce_workspace_bytes(M, C, nq) bytes (nq = number of sums, <= 3).  Every entry point below that takes `ws` checks
 * the size it documents BEFORE any launch and returns RG_EWORKSPACE for one byte less -- also where the form it takes for
 * this shape needs less or none (rg_bn_forward's single-launch form; a partial-row finish that stays single-level).
 * ------------------------------------------------------------------------------------------- */
size_t rg_colreduce_workspace_bytes(int M, int C, int nq);

/* sum[c] = sum_m z, sumsq[c] = sum_m z^2 */
int rg_bn_stats(const void* z, float* sum, float* sumsq, int M, int C, int dtype, void* ws, size_t ws_bytes,
                void* stream);
/* mean, invstd = 1/sqrt(biased var + eps); if running_mean != NULL also the PyTorch running-stat
 * update (momentum, unbiased variance) and ++(*num_batches_tracked) (int64). */
int rg_bn_finalize(const float* sum, const float* sumsq, int M, int C, float eps, float momentum, float* mean,
                   float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                   void* stream);
/* rg_bn_stats + rg_bn_finalize in one pass: the finishing step of the column reduction writes mean / invstd and
 * updates the running statistics directly (one launch less per BatchNorm forward; same arithmetic). */
/* The whole train-mode BatchNorm2d + LeakyReLU forward: a = lrelu(gamma * (z - mean) * invstd + beta) with the batch
 * statistics of z (written to mean / invstd, running statistics updated when given): statistics pass (whose finishing
 * step does the finalize) + pointwise pass.  RNAGAN_BN_FUSED=1 selects a single-launch form for small tensors in this
 * and in rg_bn_act_bwd / rg_bn_tangent / rg_bn_double_bwd (measured slower on MI355X, kept for experiments). */
int rg_bn_forward(const void* z, int M, int C, float eps, float momentum, const float* gamma, const float* beta,
                  float slope, float* mean, float* invstd, float* running_mean, float* running_var,
                  int64_t* num_batches_tracked, void* a, int dtype, void* ws, size_t ws_bytes, void* stream);
/* rg_bn_forward with the statistics taken from the partial sums a conv epilogue wrote (rg_conv_down / rg_conv_up
 * stats_partial, G rows): finishing kernel + pointwise pass. */
int rg_bn_forward_partials(const float* partial, int G, const void* z, int M, int C, float eps, float momentum,
                           const float* gamma, const float* beta, float slope, float* mean, float* invstd,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, void* a, int dtype,
                           void* ws, size_t ws_bytes, void* stream);     /* ws: 32 * 2 * C floats (two-level finish); less is refused */
int rg_bn_stats_finalize(const void* z, int M, int C, float eps, float momentum, float* mean, float* invstd,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked, int dtype, void* ws,
                         size_t ws_bytes, void* stream);
/* a = lrelu((z-mean)*invstd*gamma + beta) */
int rg_bn_act(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
              void* a, int M, int C, float slope, int dtype, void* stream);
/* gy = ga*lrelu'(y); s_gy = sum gy; s_gyxh = sum gy*xhat; gz = gamma*invstd*(gy - s_gy/M - xhat*s_gyxh/M);
 * dgamma (+)= s_gyxh, dbeta (+)= s_gy when dgamma != NULL. */
int rg_bn_act_bwd(const void* z, const void* ga, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, void* gz, float* s_gy, float* s_gyxh, float* dgamma, float* dbeta,
                  int accumulate, int M, int C, float slope, int dtype, void* ws, size_t ws_bytes, void* stream);
/* mean / invstd (+ running statistics) from the conv epilogue's column sums, without the normalisation pass.
 * ws: 32 * 2 * C floats (the staging area of the two-level finish, G > 512 and C % 8 == 0); less is refused. */
int rg_bn_finalize_partials(const float* partial, int G, int M, int C, float eps, float momentum, float* mean,
                            float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, void* ws,
                            size_t ws_bytes, void* stream);
/* ---- generator layer 0: weight gradient + optimizer step in one pass --------------------------------------------------
 * rg_g0_wgrad (.backward() into nn.ConvTranspose2d(E, C, 4, 1, 0).weight, src/wgan_loss.py:126) followed by the Adam step
 * on that tensor (optimizer_generator.step(), :127) as ONE streaming kernel: the gradient dw[e][c][tap] = sum_n z[n][e] *
 * gz0[n][tap][c] (K = the batch) is formed in registers and torch.optim.Adam's update applied in place to p / m / v
 * ([E][C][4][4] fp32, 16-byte aligned), `hyper` = the 8 floats of rg_adam_hyper_dev, shadow_bf16 (may be NULL) = the bf16
 * image of p that rg_adam_step_dev keeps.  26 B per parameter instead of 4 (gradient written) + 30.  Single-process runs
 * only: a data-parallel step needs the gradient in memory for its all-reduce.  dtype = element type of gz0. */
int rg_g0_wgrad_adam_supported(int N, int E, int C, int dtype);
int rg_g0_wgrad_adam(const float* z, const void* gz0, float* p, float* m, float* v, const float* hyper, void* shadow_bf16,
                     int N, int E, int C, int dtype, void* stream);

/* The same fusion for an nn.Linear weight W[O][I] (fp32, row pitch I): dW[o][i] = sum_n g[n][o] * x[n][i], the batch being the
 * only contraction, formed on MFMA and consumed by torch.optim.Adam's update (weight decay included) in one pass over p / m / v
 * -- the betaVAE's layers in src/betaVAE_training.py (optimizer.step() at src/betaVAE.py:226 after loss.backward() :225).
 * gT [>= O][ldn] and xT [>= I][ldn]: bf16, samples contiguous, zero padded to ldn (a multiple of 64) -- the images
 * rg_transpose_pack_bf16 writes.  p / m / v: the weight's segment of the flat parameter / moment buffers; hyper: rg_adam_hyper_dev.
 * The gradient itself is not written anywhere.  wpack_bf16 (optional): the bf16 operand image [>= O][Kp] of the UPDATED weight in
 * rg_pack_linear_weight's layout (its zero padding is the caller's: only the O x I entries are written), so that the next
 * forward needs no packing pass. */
int rg_linear_wgrad_adam(const void* gT, const void* xT, int ldn, int N, float* p, float* m, float* v, const float* hyper, int O,
                         int I, void* wpack_bf16, int Kp, void* stream);

/* ---- Inception-v3 feature extractor of the FID metric (src/fid.py:33-94: torchvision inception_v3 up to Mixed_7c) --------
 * NHWC fp32.  A BasicConv2d (Conv2d(bias=False) + BatchNorm2d(eval, eps 1e-3) + ReLU) = rg_im2col_nhwc (not needed for 1x1
 * stride 1) + rg_linear_affine_act with the folded BatchNorm affine and slope 0; ldx / ldy are row strides in elements, so a
 * branch reads / writes a channel slice of a wider activation (torch.cat of the block outputs is free).
 *   rg_im2col_nhwc        cols[(n,ho,wo)][(i,j,c)] = x[n][ho*sh-ph+i][wo*sw-pw+j][c] or 0 outside the image
 *   rg_pool2d_nhwc        mode 0: F.max_pool2d(k, stride) ; mode 1: F.avg_pool2d(k, stride, pad) (padding counted)
 *   rg_nchw_to_nhwc_affine y[n][p][c] = x[n][c][p] * scale[c] + shift[c]  (x * 2 - 1 and torchvision's transform_input)
 *   rg_spatial_mean_nhwc  adaptive_avg_pool2d(., (1, 1)) */
int rg_im2col_nhwc(const float* x, int ldx, float* cols, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph,
                   int pw, void* stream);
int rg_pool2d_nhwc(const float* x, int ldx, float* y, int ldy, int N, int H, int W, int C, int k, int stride, int pad, int mode,
                   void* stream);
int rg_nchw_to_nhwc_affine(const float* x_nchw, float* y_nhwc, int N, int C, int H, int W, const float* scale, const float* shift,
                           void* stream);
int rg_spatial_mean_nhwc(const float* x, float* y, int N, int HW, int C, void* stream);

/* The two kernels a Frechet-distance evaluation needs around a feature extractor (rg_fidstat.hip; rna_gan_amd.fid
 * preprocess_images_device / FeatureMoments, rna_gan_amd.metrics.FrechetDistance) and the one kernel of the kernel distance
 * (rna_gan_amd.kid, rna_gan_amd.metrics.KernelDistance).  No 16-bit type is involved: both builds behave identically.
 *
 * rg_resize_bilinear01: bilinear resampling of an image batch to (Ho, Wo), half-pixel centres, no anti-aliasing (cv2.resize /
 * F.interpolate(align_corners=False)); dst is fp32 NCHW [N][C][Ho][Wo] in [0, 1], what InceptionV3.features takes.  src is
 * addressed as src[n*sn + c*sc + y*sh + x*sw] (ELEMENT strides: NCHW, NHWC and a slice of a larger batch are just strides).
 *   tap     RG_U8: t = (float)v / 255.0f (a true division, as rg_u8_to_norm);  RG_F32: t = v * mul + add, two fp32 operations
 *           ((1, 0) for images in [0, 1], (0.5, 0.5) for generator output in [-1, 1]; mul / add are ignored for RG_U8)
 *   axis    in fp64: s = max(0, (d + 0.5) * (double)in / out - 0.5), i0 = min(floor(s), in - 1), i1 = min(i0 + 1, in - 1),
 *           lambda = (float)(s - i0)
 *   value   (1 - ly) * ((1 - lx) * t00 + lx * t01) + ly * ((1 - lx) * t10 + lx * t11), every operation a separately rounded
 *           fp32 operation, then clamped into [0, 1] by comparisons (a NaN tap stays NaN).  in == out on both axes: the tap
 *           bit for bit.
 * Only the H x W taps of the N x C planes are read.  N == 0: RG_OK, nothing launched.  RG_EINVAL (nothing launched) for a
 * NULL buffer, a non-positive size or a src_dtype other than RG_F32 / RG_U8. */
int rg_resize_bilinear01(const void* src, int src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float mul, float add,
                         float* dst_nchw, int N, int C, int H, int W, int Ho, int Wo, void* stream);
/* rg_moments_update: first and second raw moments of n feature rows x[r][0..F) (row stride ldx >= F elements, any alignment),
 * accumulated in fp64 into caller-zeroed s1[F] and s2[F][F] (row-major):
 *   s1[j]    += sum_r x[r][j]
 *   s2[i][j] += sum_r (double)x[r][i] * (double)x[r][j]
 * The products are exact in fp64; the additions run in row order inside the ONE workgroup that owns a 64 x 64 tile of s2 (it
 * reads the tile, adds its sum over the n rows, writes it back): no atomics, the same bits on every run, and s2[i][j] ==
 * s2[j][i] bit for bit (each off-diagonal tile pair is computed once and written twice).  Only rows < n and columns < F of x
 * are read.  Any F >= 1, any n >= 0 (n == 0: RG_OK, nothing launched); RG_EINVAL for F < 1, n < 0, ldx < F or a NULL buffer.
 * (mu, sigma) = (s1 / n, (s2 - n mu mu^T) / (n - 1)) is finished on the host. */
int rg_moments_update(const float* x, int ldx, int n, int F, double* s1, double* s2, void* stream);
/* rg_polykernel_tile_sums: the Gram sums of the kernel distance (rna_gan_amd.kid; KID, Binkowski et al. 2018): sums of the
 * polynomial kernel k(x, y) = (gamma <x, y> + coef0)^degree over 64 x 64 tiles of row pairs, in fp64.
 *   a: na rows of F fp32 features, row stride lda >= F elements, any alignment; b: nb rows, row stride ldb >= F, likewise.
 *   Ta = ceil(na / 64), Tb = ceil(nb / 64); sums is a Ta x Tb row-major fp64 matrix, WRITTEN (not accumulated into):
 *     sums[ti][tj] = sum of k(a_r, b_s) over the rows r < na of tile ti and s < nb of tile tj.
 *   Rows past na / nb are masked out of the sum (k(0, y) = coef0^degree is not zero) and never read; columns past F are never
 *   read.  Nothing outside Ta * Tb doubles of sums and Ta doubles of diag is written.
 * Symmetric form, b == NULL: b = a, nb = na (ldb, nb are ignored).  Only tiles ti <= tj are computed; each value is stored to
 *   [ti][tj] and [tj][ti] (the same bits), and diag[ti] = sum_r k(a_r, a_r) over tile ti's rows, taken from the diagonal tile's
 *   own accumulators.  diag is required in this form; with b != NULL it must be NULL.  sums of the symmetric form equals sums of
 *   the two-operand call on (a, a) bit for bit (the order of a tile's sum is invariant under transposing the tile).
 * Arithmetic: every operand is converted to fp64; dot = sum_k a[k] * b[k] sequentially in ascending k (the products of fp32
 *   values are exact in fp64: fma and mul + add give the same bits); t = gamma * dot + coef0 as two separately rounded
 *   operations; v = t (degree 1), t * t (2), (t * t) * t (3).  A tile's up to 4096 values are added in one fixed order inside the
 *   ONE workgroup that owns the tile pair: no atomics, no split of a tile, the same bits on every run.
 * No host synchronisation, no allocation, safe under graph capture.  na == 0 or nb == 0: RG_OK, nothing written.  RG_EINVAL
 * (nothing launched) for F < 1, na < 0, nb < 0, lda < F, ldb < F, degree outside 1..3, a NULL a or sums, a NULL diag in the
 * symmetric form or a non-NULL diag with two operands; RG_EUNSUPPORTED for more than 2^31 - 1 tiles. */
int rg_polykernel_tile_sums(const float* a, int lda, int na, const float* b, int ldb, int nb, int F, double gamma, double coef0,
                            int degree, double* sums, double* diag, void* stream);

/* The two primitives of the precision / recall / density / coverage metrics (rg_knn.hip; rna_gan_amd.prdc,
 * rna_gan_amd.metrics.PrecisionRecall; Kynkaanniemi et al. 2019, Naeem et al. 2020): k-th nearest-neighbour radii of a set and
 * membership of the rows of one set in the balls of another.  All-pairs SQUARED distances in fp64 over 64 x 64 tiles of row
 * pairs; the n x n matrix is never in memory.  No 16-bit type is involved: both builds behave identically.
 *   Rows: fp32, F features, row stride lda / ldb >= F elements, any alignment.  Rows past the end and columns past F are never
 *   read; nothing outside the outputs and the first rg_pairdist_ws_bytes(...) bytes of ws is written.
 * Arithmetic: every operand is converted to fp64; diff = (double)a_f - (double)b_f is one rounded subtraction;
 *   d2(a, b) = sum_f diff^2 is accumulated sequentially in ascending f by fma(diff, diff, acc).  Consequences, relied upon:
 *   d2 >= 0; d2(a, a) = 0; d2(a, b) and d2(b, a) are the same bits; the value does not depend on tiling.  (The Gram form
 *   |a|^2 + |b|^2 - 2 <a, b> is deliberately not used: it cancels, can go negative and breaks the exact symmetry.)  A NaN d2
 *   never hits and counts as +inf in the selection and in the minimum.  Everything downstream of d2 (k-th smallest, count,
 *   minimum) is independent of order: no atomics, the same bits on every run.
 * rg_knn_radii2: r2[i] = the k-th smallest element of the multiset { d2(a_i, a_j) : j != i }, 1 <= k <= 16, n >= k + 1.  Row i
 *   is excluded BY INDEX, not by value: a duplicate row at distance 0 counts, so a radius can be 0.  Each pair of tiles is
 *   computed once (upper triangle) and serves both of its row sets.
 * rg_radius_hits: for every row r < na of a,
 *     count[r] = #{ s < nb : d2(a_r, b_s) <= rb2[s] }      (<= on squared distances, no square root anywhere)
 *     mind2[r] = min_s d2(a_r, b_s)
 *   rb2 == NULL: only mind2 is wanted, and count must be NULL too (count without rb2, or rb2 without count: RG_EINVAL).
 * Workspace: rg_pairdist_ws_bytes(na, nb, k) bytes, 8-byte aligned, contents irrelevant before and after: per-tile partials
 *   that a second small kernel (one thread per row) merges.  rg_knn_radii2 needs rg_pairdist_ws_bytes(n, n, k);
 *   rg_radius_hits needs rg_pairdist_ws_bytes(na, nb, 0).  (0 for arguments out of range.)
 * No host synchronisation, no allocation, safe under graph capture.  rg_radius_hits with na == 0 or nb == 0: RG_OK, nothing
 * written.  Nothing is launched on an error: RG_EINVAL for F < 1, a negative row count, lda / ldb < F, k outside 1..16,
 * n < k + 1, a NULL required buffer (a, b, ws, r2, mind2) or a misaligned ws; RG_EUNSUPPORTED for more than 2^31 - 1 tiles;
 * RG_EWORKSPACE for ws_bytes below the size above. */
size_t rg_pairdist_ws_bytes(int na, int nb, int k);
int rg_knn_radii2(const float* a, int lda, int n, int F, int k, void* ws, size_t ws_bytes, double* r2, void* stream);
int rg_radius_hits(const float* a, int lda, int na, const float* b, int ldb, int nb, int F, const double* rb2, void* ws,
                   size_t ws_bytes, int32_t* count, double* mind2, void* stream);

/* The two primitives of the per-patient representations and the RNA-conditioning metric (rg_groupstat.hip;
 * rna_gan_amd.representation, rna_gan_amd.metrics.ConditioningFidelity): fp64 sums of feature rows per GROUP (a patient's tiles)
 * and the rank of every row's designated partner among the rows of another set of fp64 centroids.  No 16-bit type is involved:
 * both builds behave identically.
 * rg_group_sums_update: x is n rows of F fp32 features, row stride ldx >= F elements, any alignment; group is n int32 ids;
 *   sums is [G][F] fp64 row-major and counts is [G] int64, both ACCUMULATED into:
 *     sums[g][j]  += sum of (double)x[r][j] over the rows r < n with group[r] == g
 *     counts[g]   += the number of such rows
 *   The additions of an entry (g, j) form ONE chain in ascending r that starts from the value already in sums[g][j]; the one
 *   thread that owns the entry walks the rows (group ids staged through LDS, only rows of its own group loaded): no atomics.
 *   Consequences, relied upon: the result equals a sequential fp64 loop in row order bit for bit, for any floats, and it is the
 *   same whether the rows arrive in one call or split over several calls at any boundary.
 *   A row whose id is outside [0, G) is ignored: neither summed nor counted, its features are not read.  Only rows < n and
 *   columns < F of x are read; nothing outside sums[G][F] and counts[G] is written; offsets into x and sums are computed in
 *   64 bits.  No workspace, no allocation, no host synchronisation, safe under graph capture.  n == 0: RG_OK, nothing launched.
 *   RG_EINVAL (nothing launched) for a NULL buffer, F < 1, G < 1, n < 0 or ldx < F; RG_EUNSUPPORTED for more than 2^31 - 1
 *   workgroups (G ceil(F / 256)).
 * rg_match_ranks: a is na rows and b is nb rows of F fp64 features, row strides lda / ldb >= F elements; target is na int32 row
 *   indices of b, or NULL = target[r] = r (then na <= nb is required).  d2 is the squared distance of rg_knn_radii2 on fp64
 *   operands: diff = a_f - b_f is one rounded subtraction, d2 = fma(diff, diff, d2) sequentially in ascending f from 0 (so the
 *   value does not depend on tiling).  With t = target[r] and d* = d2(a_r, b_t), both outputs WRITTEN (not accumulated into):
 *     dtarget[r] = d*
 *     rank[r]    = #{ s != t : d2(a_r, b_s) < d* } + #{ s < t : d2(a_r, b_s) == d* }
 *   Rank 0: the designated partner is the nearest row; ties are broken by index.  A NaN d2(a_r, b_s) never counts as closer; a
 *   NaN d* gives rank[r] = nb - 1.  A target outside [0, nb) is CLAMPED (negative -> 0, >= nb -> nb - 1): a memory-safety
 *   guarantee as in rg_rows_gather_f32, not an interface -- callers validate their targets.
 *   A workgroup owns 64 rows of a and a share of the 64-row tiles of b; the counts are integers, summed with integer atomics
 *   onto rank, which the call itself clears first (a memset node on the same stream) when the tiles of b are shared out: the
 *   same bits on every run.  Rows past na / nb and columns past F are never read; nothing outside rank[na] and dtarget[na] is
 *   written.  No workspace, no allocation, no host synchronisation, safe under graph capture.  na == 0: RG_OK, nothing written.
 *   RG_EINVAL (nothing launched) for a NULL a, b, rank or dtarget, F < 1, nb < 1, na < 0, lda < F, ldb < F, or target == NULL
 *   with na > nb. */
int rg_group_sums_update(const float* x, int ldx, int n, int F, const int32_t* group, int G, double* sums, long long* counts,
                         void* stream);
int rg_match_ranks(const double* a, int lda, int na, const double* b, int ldb, int nb, int F, const int32_t* target, int32_t* rank,
                   double* dtarget, void* stream);

/* The three primitives of the linear-probe scores (rg_linprobe.hip; rna_gan_amd.linprobe: the classifier two-sample test and
 * train-on-synthetic, tissue_probe.py): multinomial logistic regression on fp32 feature rows that stay on the device.  One objective
 * evaluation is scores, residual, column sums.  Everything is fp64, in a fixed order, without atomics: the same bits on every
 * run.  No 16-bit type is involved: both builds behave identically.  Every call: no allocation, no host synchronisation, safe
 * under graph capture, offsets computed in 64 bits; on an error nothing is launched.
 * rg_linear_scores_f64: x is n rows of F fp32 features, row stride ldx >= F elements, any alignment; w is [C][F] fp64, row stride
 *   ldw >= F; bias is [C] fp64 or NULL; z is [n][C] fp64, row stride ldz >= C, WRITTEN (not accumulated into):
 *     acc = 0.0;  acc = fma((double)x[r][f], w[c][f], acc) for f = 0 .. F - 1 in ascending order;
 *     z[r][c] = acc + bias[c]  (ONE rounded addition), or acc when bias == NULL.
 *   One chain per (r, c), never split over F: the value does not depend on tiling or launch plan and equals a sequential loop
 *   bit for bit (the product of an fp32 and an fp64 value is not exact, so the fma is part of the contract).  Any C >= 1.
 *   Only rows < n and columns < F of x, rows < C and columns < F of w are read; nothing outside z[r][0 .. C) is written (the
 *   columns C .. ldz of a row of z keep their contents).  n == 0: RG_OK, nothing launched.  RG_EINVAL for a NULL x, w or z,
 *   F < 1, C < 1, n < 0, ldx < F, ldw < F or ldz < C; RG_EUNSUPPORTED for more than 2^31 - 1 workgroups (ceil(n / 32) ceil(C / 8)).
 * rg_softmax_residual_f64: z is [n][C] fp64 logits, row stride ldz >= C; label is n int32; weight is n fp64 or NULL (= 1.0);
 *   resid is [n][C] fp64, row stride ldr >= C, and row_loss is n fp64, both WRITTEN.  Per row r, with y = label[r], wt = weight[r]:
 *     m = max_c z_c;  e_c = exp(z_c - m);  s = sum_c e_c in ascending c from 0.0;  p_c = e_c / s
 *     0 <= y < C:  resid[r][c] = wt * (p_c - [c == y]),  row_loss[r] = wt * (log(s) - (z_y - m))
 *     otherwise the row is MASKED: resid[r][0 .. C) are exact zeros and row_loss[r] is exact 0, whatever its logits and weight
 *     hold (this is how rows are held out of a fit without gathering the others: the caller labels them -1).
 *   m >= every z_c, so no exp overflows and s >= 1: logits of +-1e3 give finite results.  A NaN logit makes m NaN and with it
 *   the whole of ITS row (resid and row_loss), and no other row.  exp and log are the device's fp64 functions: the results are
 *   accurate to a few units in the last place, not bit-defined.  n == 0: RG_OK, nothing launched.  RG_EINVAL for a NULL z,
 *   label, resid or row_loss, C < 1, n < 0, ldz < C or ldr < C.
 * rg_rows_weighted_colsums_f64: x as above; r is [n][C] fp64, row stride ldr >= C; out is [C][F] fp64 row-major, WRITTEN:
 *     out[c][f] = sum over the rows of r[row][c] * t(x[row][f]),   t(v) = (double)v for power == 1,
 *                                                                  t(v) = (double)v * (double)v for power == 2 (exact in fp64).
 *   The order of the sum is part of the contract.  The rows are cut into blocks of RG_COLSUM_ROWS; inside a block an entry is
 *   ONE chain acc = fma(r[row][c], t, acc) in ascending row order from 0.0; the block partials of an entry are then added in
 *   ascending block order from 0.0.  So the result is the same whatever the grid, and equals that loop bit for bit.
 *   Two launches: the partials into ws ([blocks][C][F] fp64, rg_colsums_ws_bytes(n, F, C) bytes, 8-byte aligned, contents
 *   irrelevant before and after), then a finisher.  With r a column of ones (C = 1) it gives column sums (power 1) and sums of
 *   squares (power 2); with r = resid it gives the gradient of the loss with respect to W.
 *   Only rows < n and columns < F of x, columns < C of r are read; nothing outside out[C][F] and the first
 *   rg_colsums_ws_bytes(n, F, C) bytes of ws is written.  n == 0: RG_OK, out is written as the empty sums (+0.0 in every entry,
 *   the finisher alone is launched); x, r and ws are then not looked at and may be NULL.  RG_EINVAL for a NULL out, a NULL x, r
 *   or ws with n > 0, F < 1, C < 1, n < 0, ldx < F, ldr < C or a power other than 1 and 2; RG_EWORKSPACE (n > 0) for a ws that is
 *   not 8-byte aligned or ws_bytes below the size above; RG_EUNSUPPORTED for more than 2^31 - 1 workgroups
 *   (ceil(n / 256) ceil(F / 64) ceil(C / 8)).  rg_colsums_ws_bytes is 0 for arguments out of range. */
#define RG_COLSUM_ROWS 256
int rg_linear_scores_f64(const float* x, int ldx, int n, int F, const double* w, int ldw, int C, const double* bias, double* z,
                         int ldz, void* stream);
int rg_softmax_residual_f64(const double* z, int ldz, int n, int C, const int32_t* label, const double* weight, double* resid,
                            int ldr, double* row_loss, void* stream);
size_t rg_colsums_ws_bytes(int n, int F, int C);
int rg_rows_weighted_colsums_f64(const float* x, int ldx, int n, int F, const double* r, int ldr, int C, int power, void* ws,
                                 size_t ws_bytes, double* out, void* stream);

/* ---- split-K conv + train-mode BatchNorm without the intermediate passes (bf16 path) -------------------------------
 * The deep Conv2d / ConvTranspose2d layers at small batch run split-K (rg_conv_split(...) > 1): every launch leaves
 * nsplit fp32 slabs [nsplit][rows][C] in the workspace.  rg_conv_down_partial / rg_conv_up_partial run ONLY that launch
 * (slabs in `ws`, slab s at ws + s * rows * C floats, rows in output NHWC order); the consumer sums them:
 *   rg_bn_forward_slabs : z = bf16(sum_s slab_s) (written), batch statistics of z (per batch group, running statistics
 *                         updated group after group), a = lrelu(BN(z)) -- nn.Conv2d -> nn.BatchNorm2d(train) ->
 *                         nn.LeakyReLU of the torchgan DCGAN blocks, = rg_conv_* + rg_bn_forward[_g2];
 *   rg_bn_act_bwd_slabs : ga = bf16(sum_s slab_s) = the data gradient arriving at the block (written when ga_out != NULL),
 *                         then exactly rg_bn_act_bwd[_g2] (.backward() of the same block).
 * One launch each: the workgroups of a 128-column slice exchange their partial column sums through `scratch` and meet at
 * a counter in `sync` (agent-scope release/acquire hand-off, deterministic summation order).  `sync`: a caller-owned
 * buffer of rg_slab_bn_sync_words() 32-bit words, ZEROED ONCE when allocated and private to one stream (every launch
 * leaves it zero); `scratch`: rg_slab_bn_scratch_bytes(M, C, groups) bytes, contents irrelevant.  M = rows per batch group
 * (groups = 1 or 2, z is [groups * M][C]).  rg_slab_bn_supported: C % 128 == 0, nsplit in {2, 4, 8}, row count divisible
 * into 64 / 128 / 256-row blocks with at most 256 workgroups (one per CU: all co-resident -- required by the hand-off). */
int rg_conv_split(int up, int N, int Hlow, int Wlow, int O, int I, int dtype, int algo);
/* element type of the slabs that launch leaves: RG_F32, or RG_BF16 where the 8-wave kernel stores its partial tiles as bf16
 * (option "slab16", default on in the bf16 build: half the slab bytes written and re-read; each partial sum is rounded to
 * bf16 before the consumer adds them in fp32.  fp16 build: default OFF and unsupported -- a partial sum can leave fp16's range
 * where the sum does not, and two partials overflowing with opposite signs add up to NaN; the slabs are RG_F32 there).  Pass it to the consumer as slab_dtype; the slab stride stays in ELEMENTS. */
int rg_conv_slab_dtype(int up, int N, int Hlow, int Wlow, int O, int I, int dtype, int algo);
int rg_conv_down_partial(const void* x, const void* wdn, int N, int Hi, int Wi, int I, int O, int dtype, int algo,
                         void* ws, size_t ws_bytes, void* stream);
int rg_conv_up_partial(const void* x, const void* wup, int N, int Ho, int Wo, int O, int I, int dtype, int algo,
                       void* ws, size_t ws_bytes, void* stream);
int rg_slab_bn_supported(long long M, int C, int groups, int nsplit);
size_t rg_slab_bn_scratch_bytes(long long M, int C, int groups);
size_t rg_slab_bn_sync_words(void);
int rg_bn_forward_slabs(const void* slab, int nsplit, size_t slab_stride, int slab_dtype, void* z, void* a, long long M, int C, int groups,
                        float eps, float momentum, const float* gamma, const float* beta, float slope, float* mean,
                        float* invstd, float* running_mean, float* running_var, long long* num_batches_tracked,
                        void* scratch, size_t scratch_bytes, void* sync, void* stream);
/* the forward-mode tangent of the same block (rg_bn_tangent) with zt arriving as slabs (the penalty's tangent forward):
 * zt_out = bf16(sum_s slab_s) (always written), at, s_zt, s_xhzt as rg_bn_tangent */
int rg_bn_tangent_slabs(const void* slab, int nsplit, size_t slab_stride, int slab_dtype, const void* z, void* zt_out, void* at, long long M,
                        int C, const float* mean, const float* invstd, const float* gamma, const float* beta, float slope,
                        float* s_zt, float* s_xhzt, void* scratch, size_t scratch_bytes, void* sync, void* stream);
int rg_bn_act_bwd_slabs(const void* slab, int nsplit, size_t slab_stride, int slab_dtype, const void* z, void* ga_out, void* gz, long long M,
                        int C, int groups, const float* mean, const float* invstd, const float* gamma, const float* beta,
                        float slope, float* s_gy, float* s_gyxh, float* dgamma, float* dbeta, int accumulate, void* scratch,
                        size_t scratch_bytes, void* sync, void* stream);

/* Two batch groups in one call (the D-loss step runs D(real) and D(fake) -- src/wgan_loss.py:241-253 -- as one double
 * batch through the conv layers; BatchNorm must treat the halves as the two separate forward calls they are in the
 * reference): z / a / ga / gz are [2*M][C] (first half first), mean / invstd / s_gy / s_gyxh [2][C].  rg_bn_forward_g2 =
 * rg_bn_forward_partials (partial != NULL: 2*G rows [.][2][C] laid out [nblk][2 halves][G/nblk] -- nblk = 1 for
 * rg_conv_down's row-tile order, 4 for rg_conv_up's class-major order) or rg_bn_forward (partial == NULL) on the first half,
 * then on the second (running statistics and num_batches_tracked updated in that order); rg_bn_act_bwd_g2 = rg_bn_act_bwd on both
 * halves with dgamma / dbeta summed.  Workspace: twice rg_colreduce_workspace_bytes(M, C, 2) for rg_bn_act_bwd_g2 and for
 * rg_bn_forward_g2 without partial rows; 2 * 32 * 2 * C floats for rg_bn_finalize_partials_g2 and for rg_bn_forward_g2 with
 * partial rows.  Less is refused (RG_EWORKSPACE). */
int rg_bn_finalize_partials_g2(const float* partial, int G, int nblk, int M, int C, float eps, float momentum, float* mean,
                               float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                               void* ws, size_t ws_bytes, void* stream);
int rg_bn_forward_g2(const float* partial, int G, int nblk, const void* z, int M, int C, float eps, float momentum,
                     const float* gamma, const float* beta, float slope, float* mean, float* invstd, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, void* a, int dtype, void* ws, size_t ws_bytes,
                     void* stream);
int rg_bn_act_bwd_g2(const void* z, const void* ga, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, void* gz, float* s_gy, float* s_gyxh, float* dgamma, float* dbeta, int accumulate,
                     int M, int C, float slope, int dtype, void* ws, size_t ws_bytes, void* stream);
/* tangent of a = lrelu(bn(z)) along zt with batch statistics varying:
 * at = lrelu'(y)*gamma*invstd*(zt - s_zt/M - xhat*s_xhzt/M) */
int rg_bn_tangent(const void* z, const void* zt, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, void* at, float* s_zt, float* s_xhzt, int M, int C, float slope, int dtype,
                  void* ws, size_t ws_bytes, void* stream);
/* joint reverse through (a, at): see DESIGN.md "GP second-order pass" for the formula.
 * qa may be NULL (zero primal cotangent). */
int rg_bn_double_bwd(const void* z, const void* qa, const void* zt, const void* ga1, const float* mean,
                     const float* invstd, const float* gamma, const float* beta, const float* s_gy,
                     const float* s_gyxh, const float* s_zt, const float* s_xhzt, void* pz, float* dgamma,
                     float* dbeta, int accumulate, int M, int C, float slope, int dtype, void* ws,
                     size_t ws_bytes, void* stream);

/* ---- BatchNorm-free critic layers (DCGANDiscriminator(batchnorm=False); rg_plainact.hip).  A layer is
 *   a = lrelu(conv_down(x) + bias[c]);  backward / tangent: out = conv(.) * lrelu'(a) with the mask from the sign of the stored a.
 * Where the plain launch does not split K (rg_conv_split <= 1) the matrix-core stride-2 conv takes either in its epilogue, on the
 * fp32 accumulator, rounded once: rg_conv_down_epi with exactly one of shift (bias; the affine epilogue with scale 1) / mask_act
 * (rg_conv_up already takes a mask).  Where it splits, rg_conv_down_partial / rg_conv_up_partial leave their slabs
 * [nsplit][M][C] (element type rg_conv_slab_dtype, `stride` elements apart) and one of the two finishing kernels sums them in
 * the fixed order s = 0, 1, ... and writes the 16-bit result:
 *   rg_slab_bias_act:  y[m][c] = lrelu(sum_s slab[s][m][c] + bias[c], slope)
 *   rg_slab_mask:      y[m][c] = (sum_s slab[s][m][c]) * lrelu'(mask_act[m][c]);  col_parts (optional, fp32
 *                      [rg_slab_finish_rows(M, C)][C]): per-workgroup column sums of the STORED y -- the consumer layer's bias
 *                      gradient once rg_parts_col_sum has added the rows up (fixed order).
 * rg_slab_finish_rows == 0: the kernels' thread layout does not cover this C (C / 8 must divide 256 or be a multiple of it).
 * rg_bias_act: y = lrelu(z + bias[c]) elementwise (y may be z; RG_F32 or the 16-bit type; C % 8 == 0): the pass behind a conv
 * without a fused form (fp32 storage, generic kernels). */
int rg_slab_finish_rows(long long M, int C);
int rg_slab_bias_act(const void* slab, int nsplit, size_t stride, int slab_dtype, const float* bias, void* y, long long M, int C,
                     float slope, void* stream);
int rg_slab_mask(const void* slab, int nsplit, size_t stride, int slab_dtype, const void* mask_act, float mask_slope, void* y,
                 float* col_parts, long long M, int C, void* stream);
int rg_parts_col_sum(const float* parts, int rows, int C, float* out, int accumulate, void* stream);
int rg_bias_act(const void* z, const float* bias, void* y, long long M, int C, float slope, int dtype, void* stream);
int rg_conv_down_epi_supported(int N, int Hi, int Wi, int I, int O, int dtype, int algo);
int rg_conv_down_epi(const void* x, const void* wdn, void* y, int N, int Hi, int Wi, int I, int O, const float* shift, float slope,
                     const void* mask_act, float mask_slope, int dtype, int algo, void* ws, size_t ws_bytes, void* stream);

/* out = g * lrelu'(a) with the mask taken from the sign of the activation OUTPUT a */
int rg_lrelu_bwd(const void* g, const void* a, void* out, size_t n, float slope, int dtype, void* stream);
/* out[c] (+)= sum_m g[m][c]   (bias gradient) */
int rg_col_sum(const void* g, float* out, int M, int C, int dtype, int accumulate, void* ws, size_t ws_bytes,
               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image-side pointwise ops and reductions (NCHW fp32) (K7, K10, K11)
 * ------------------------------------------------------------------------------------------- */
int rg_tanh_bwd(const float* gy, const float* y, float* gz, size_t n, void* stream);
/* out[c] (+)= sum_{n,h,w} g[n][c][h][w] */
int rg_nchw_chan_sum(const float* g, float* out, int N, int C, int HW, int accumulate, void* ws, size_t ws_bytes,
                     void* stream);
/* xhat = eps*real + (1-eps)*fake (wgan_loss.py:377) */
int rg_interp(const float* real, const float* fake, float* out, size_t n, float eps, void* stream);
/* graph-replayable variant: eps read from device memory */
int rg_interp_dev(const float* real, const float* fake, float* out, size_t n, const float* eps, void* stream);
/* out[0] = sum x^2 (fp32 result, pairwise/blocked accumulation; deterministic) */
size_t rg_reduce_workspace_bytes(size_t n);
int rg_sqnorm(const float* x, float* out, size_t n, void* ws, size_t ws_bytes, void* stream);
/* from sq = ||g||^2: loss = (sqrt(sq)-1)^2 ; coef = lambd*2*(sqrt(sq)-1)/sqrt(sq) (wgan_loss.py:43) */
int rg_gp_coef(const float* sq, float* loss, float* coef, float lambd, void* stream);
int rg_gp_coef_scaled(const float* sq, float* loss, float* coef, float lambd, float in_scale, float out_scale, void* stream);
int rg_gp_coef_scaled_dev(const float* sq, float* loss, float* coef, float lambd, const int* amp_state, int slot, void* stream);
/* out = x * coef[0] (coef on device: no host sync inside the step) */
int rg_scale_by(const float* x, const float* coef, float* out, size_t n, void* stream);
/* out[0] = sign * mean(a - b) (b may be NULL) (wgan_loss.py:24-29) */
int rg_mean_diff(const float* a, const float* b, float* out, int n, float sign, void* stream);
/* noise = (u+z - mean_col)/std_col, unbiased std over the batch (wgan_loss.py:105-106) */
int rg_latent_prep(const float* u, const float* z, float* out, int N, int E, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimizer (K12/K13): torch.optim.Adam semantics on flat fp32 buffers
 * (histopathology_gan.py:252,257; stepped at wgan_loss.py:127,261,388), optional weight clamp
 * (wgan_loss.py:213-215).  step is 1-based.  Hyper-parameters are doubles, as torch holds them: the
 * kernel's constants (1-beta, lr/bias_correction1, 1/sqrt(bias_correction2)) are formed in double and
 * rounded once, which reproduces torch's fp32 results to the last bits.
 * ------------------------------------------------------------------------------------------- */
int rg_adam_step(float* p, const float* g, float* m, float* v, size_t n, int step, double lr, double beta1,
                 double beta2, double eps, void* stream);
int rg_clamp(float* p, size_t n, float lo, float hi, void* stream);
/* Same update with the step-dependent constants read from DEVICE memory, so the launch can live in
 * a captured HIP graph and be replayed every step: hyper[0..7] = {beta1, beta2, 1-beta1, 1-beta2, eps,
 * lr/bias_correction1, 1/sqrt(bias_correction2), weight_decay}, produced by rg_adam_hyper_dev.
 * shadow_bf16 (may be NULL): bf16[n], receives the rounded updated parameters in the same launch -- for the
 * tap-major conv weights that IS the wdn operand of rg_conv_down, so no separate pack pass reads the masters.
 * grad_bf16 (may be NULL): bf16[n] gradient read INSTEAD of g -- the all-reduced bf16 wire buffer of a data-parallel
 * run, which then needs no widening pass back to fp32. */
int rg_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, void* shadow_bf16,
                     const void* grad_bf16, void* stream);
/* rg_adam_step_dev over [p, p + n) cut into nseg <= 24 consecutive segments (seg_off / seg_n in elements, tiling the range in
 * order, every offset a multiple of 4): a segment with seg_slab[i] != NULL takes its gradient as the sum, in slab order, of
 * seg_nsplit[i] slabs of seg_n[i] elements, fp32 or bf16 by seg_dtype[i] (what rg_conv_wgrad_slabs left in the caller's buffer
 * and reported) instead of reading g --
 * the split-K reduction launches of the backward pass and the write + re-read of the reduced gradient disappear (one launch
 * for the whole buffer; deterministic summation order).  A segment with seg_slab[i] == NULL and seg_nsplit[i] == -1 is SKIPPED
 * (its tensor is stepped by rg_conv_wgrad_adam).  Segment tables are HOST arrays. */
int rg_adam_step_slabs(float* p, const float* g, float* m, float* v, size_t n, const float* hyper, void* shadow_bf16, int nseg,
                       const unsigned long long* seg_off, const unsigned long long* seg_n, const void* const* seg_slab,
                       const int* seg_nsplit, const int* seg_dtype, void* stream);
/* Data parallel (one process per GPU, bf16 gradient wire; the reference has no distributed path -- SURVEY 8 e): the flat fp32
 * gradient g[n] goes onto the bf16 wire buffer of the all-reduce with the segment table of rg_adam_step_slabs: a plain segment is
 * rounded, a slab segment is summed (slab order, fp32) and rounded once, a segment with seg_nsplit = -1 is left alone (its
 * weight-gradient launch wrote it: rg_conv_wgrad_wire).  Replaces the per-layer reduction launches + one cast pass. */
int rg_grad_to_wire(const float* g, void* wire_bf16, size_t n, int nseg, const unsigned long long* seg_off,
                    const unsigned long long* seg_n, const void* const* seg_slab, const int* seg_nsplit, const int* seg_dtype,
                    void* stream);
/* rg_conv_wgrad / rg_conv_wgrad2 (low1 = high1 = NULL: one segment) of a layer whose plan has no split-K
 * (rg_conv_wgrad_adam_supported) written as bf16 into the tensor's 16-byte aligned slice of that wire buffer. */
int rg_conv_wgrad_wire(const void* low0, const void* high0, const void* low1, const void* high1, void* wire_bf16, int N, int Ho,
                       int Wo, int O, int I, int dtype, int algo, void* stream);
/* ++(*step_dev) and recompute hyper[0..6] from it on the device (double arithmetic, one thread): with
 * this launch in front of rg_adam_step_dev the whole optimizer step replays from a graph untouched.
 * hyper[7] = weight_decay (torch.optim.Adam's L2 term g += wd * p; 0 on the GAN path, betaVAE training sets it,
 * src/betaVAE_training.py:163). */
int rg_adam_hyper_dev(int* step_dev, double lr, double beta1, double beta2, double eps, double weight_decay, float* hyper,
                      void* stream);
/* ... and hyper[8] = grad_scale_inv: every Adam kernel multiplies the gradient it reads (fp32 gradient, slab sums, wire, the tile
 * of the fused weight-gradient launches) by it before the update -- the unscale of a loss-scaled backward pass (fp16 build:
 * the backward seeds carry a static power-of-two scale, the mechanism sketched at src/betaVAE.py:184,230-236).  `hyper` is
 * therefore >= 9 floats for BOTH entry points; rg_adam_hyper_dev writes hyper[8] = 1 (exact: results unchanged). */
int rg_adam_hyper_dev2(int* step_dev, double lr, double beta1, double beta2, double eps, double weight_decay,
                       double grad_scale_inv, float* hyper, void* stream);
/* The hyper buffer is 12 floats: [0..8] as above, [9] = the SKIP WORD -- every kernel that applies an Adam update from `hyper`
 * (rg_adam_step_dev and its scalar form, rg_adam_step_slabs, rg_g0_wgrad_adam, rg_conv_wgrad_adam, rg_linear_wgrad_adam)
 * returns at once, touching nothing, when it is non-zero; rg_adam_hyper_dev / _dev2 write 0.  [10..11] unused.
 *
 * DYNAMIC LOSS SCALING (opt-in, rna_gan_amd.amp; rna_gan_amd/csrc/rg_amp.hip).  State: int32[RG_AMP_STATE_INTS] on the device:
 *   [RG_AMP_EXP] k with scale S = 2^k, [RG_AMP_TRACKER] finite steps since the last change, [RG_AMP_SKIPPED] skipped steps,
 *   [RG_AMP_LATCH + slot] k as latched at the first backward seed of the last train_op that steps network `slot`,
 *   [RG_AMP_FLAG + slot] non-zero when a probe of that network's step found a non-finite value.
 * rg_adam_hyper_dev3: rg_adam_hyper_dev2 with grad_scale_inv = 2^-latch[slot] and hyper[9] = flag[slot]; when the flag is set the
 *   step counter is NOT advanced (a skipped step does not count) and hyper[0..6] are left as they were. */
#define RG_AMP_EXP 0
#define RG_AMP_TRACKER 1
#define RG_AMP_SKIPPED 2
#define RG_AMP_LATCH 4
#define RG_AMP_FLAG 8
#define RG_AMP_SLOTS 4
#define RG_AMP_STATE_INTS 12
int rg_adam_hyper_dev3(int* step_dev, double lr, double beta1, double beta2, double eps, double weight_decay,
                       const int* amp_state, int slot, float* hyper, void* stream);
/* Exponential moving average of a parameter buffer (rna_gan_amd.ema.ParamEMA: the averaged generator), one launch behind the
 * Adam launches of a step:
 *   e[i] <- e[i] + omd * (p[i] - e[i]),  omd = 1.f - d, every operation a separately rounded fp32 operation in exactly that
 * order.  d = decay when step_dev == NULL; otherwise d = fminf(decay, (1.f + (float)t) / (10.f + (float)t)) with t = *step_dev
 * read on the device (Adam's 1-based step counter AFTER this step's rg_adam_hyper_dev* launch): the usual warm-up, so that the
 * average forgets its initial value quickly.  Returns at once, touching nothing, when hyper != NULL and hyper[9] != 0 (the skip
 * word above).  p is only read.  p, e: 16-byte aligned fp32, any n.  0 <= decay < 1, else RG_EINVAL (as for a NULL or
 * misaligned buffer with n > 0) and nothing is launched.  No 16-bit type is involved: both builds behave identically. */
int rg_ema_update(const float* p, float* e, size_t n, float decay, const int* step_dev, const float* hyper, void* stream);
/* OR "any non-finite value" into *flag: nseg <= 32 segments (HOST arrays) of seg_n[i] elements at seg_ptr[i], fp32 or this build's
 * 16-bit type by seg_dtype[i] (element-aligned; any length).  Exponent-mask test on the raw bits (fp32 0x7f800000, fp16 0x7c00,
 * bf16 0x7f80), wave-level OR, one atomic per wave that found something; nothing is written otherwise. */
int rg_nonfinite_probe(int nseg, const void* const* seg_ptr, const unsigned long long* seg_n, const int* seg_dtype, int* flag,
                       void* stream);
/* after the Adam launches of network `slot`: flag set -> k = max(k - 1, min_exp), tracker = 0, skipped += 1; flag clear ->
 * tracker += 1 and, when it reaches growth_interval, k = min(k + 1, max_exp), tracker = 0.  Then flag[slot] = 0. */
int rg_amp_update(int* amp_state, int slot, int growth_interval, int min_exp, int max_exp, void* stream);
/* latch[slot] = k: enqueued before the first backward seed of a train_op that steps network `slot` */
int rg_amp_latch(int* amp_state, int slot, void* stream);
/* The 16-bit storage type of this build of the library: RG_BF16 (librnagan_hip.so) or RG_F16 (librnagan_hip_f16.so: the same
 * sources compiled with -DRG_HALF_F16 -- activations, operand images, split-K slabs and the data-parallel wire are IEEE fp16,
 * the MFMAs the _f16 forms; every entry point takes RG_F16 where this header says RG_BF16; no rg_probe_* entry points).
 * BASELINE.json configs[3] names fp16 storage. */
int rg_storage_dtype(void);

/* ---------------------------------------------------------------------------------------------
 * betaVAE TRAINING (src/betaVAE.py:63-107 model, :145-163 loss, :166-284 train loop).
 * A Linear layer's three GEMMs all take the "NT" form C[M][Nout] = A[M][K] . B[Nout][K]^T:
 *   forward  y  = x  . W^T      A = x [N][in]        B = W   [out][in]
 *   data     dx = dy . W        A = dy [N][out]      B = W^T [in][out]     (rg_transpose_pack_bf16 of W)
 *   weight   dW = dy^T . x      A = dy^T [out][N]    B = x^T [in][N]       (both transposed packs; K = batch)
 * rg_gemm_nt_bf16: bf16 operands with K padded to K_pad (multiple of 64, zero filled), fp32 accumulate/output,
 *   epilogue y = lrelu(acc * scale[j] + shift[j], slope) (scale/shift may be NULL, slope 1 = none).  Nout need not
 *   be a multiple of 8; the columns Nout .. min(roundup8(Nout), ldy) - 1 are written as +0.0 (for every ldy, aligned or
 *   not), the columns from there to ldy - 1 are left untouched.
 * rg_transpose_pack_bf16: dst bf16 [C_pad][R_pad] = src^T (fp32 [R][C]), zero padded; R_pad % 64 == 0.
 * rg_transpose_f32: fp32 parity mode (the functor GEMM rg_linear_affine_act takes fp32 operands).
 * ------------------------------------------------------------------------------------------- */
int rg_transpose_f32(const float* src, float* dst, int R, int C, void* stream);
int rg_transpose_pack_bf16(const float* src, void* dst, int R, int C, int R_pad, int C_pad, void* stream);
size_t rg_gemm_nt_bf16_workspace_bytes(int M, int K_pad, int Nout);
int rg_gemm_nt_bf16(const void* a, const void* b, const float* scale, const float* shift, float* y, int ldy, int M,
                    int K_pad, int Nout, float slope, void* ws, size_t ws_bytes, void* stream);
/* y[N][ld] = Dropout(x[N][F]) with the caller's keep-mask (uint8, NULL = keep all) and scale 1/(1-p); columns
 * F..ld-1 are zero (src/betaVAE.py:27: nn.Dropout() in front of the encoder) */
int rg_vae_dropout(const float* x, const unsigned char* mask, float* y, int N, int F, int ld, float scale, void* stream);
/* z = mu + eps * exp(0.5 logvar) (betaVAE.py:96-100) and its backward joined with the loss gradients:
 * gmu = gmu_loss + gz ; glv = glv_loss + gz * eps * 0.5 exp(0.5 logvar) */
int rg_vae_reparam(const float* mu, const float* logvar, const float* eps, float* z, size_t n, void* stream);
int rg_vae_reparam_bwd(const float* gz, const float* logvar, const float* eps, const float* gmu_loss,
                       const float* glv_loss, float* gmu, float* glv, size_t n, void* stream);
int rg_tanh_inplace(float* x, size_t n, void* stream);
int rg_add_inplace(float* y, const float* x, size_t n, void* stream);     /* y += x (the two heads' gradients meet) */
/* betaVAEloss (betaVAE.py:145-163): losses[3] = {total, reconstruction (MSE over N*F), kl}; total = recons + beta*kl
 * when training else recons.  Also writes d total / d x_recons ([N][ld]), d total / d z_mean, d total / d z_logvar
 * ([N][Z]).  x and x_recons are [N][ld] with zero pad columns F..ld-1.  Deterministic two-stage reduction. */
size_t rg_vae_loss_workspace_bytes(void);
int rg_vae_loss(const float* x, const float* x_recons, int N, int F, int ld, const float* z_mean, const float* z_logvar,
                int Z, float beta, int training, float* losses, float* g_recons, float* g_mean, float* g_logvar, void* ws,
                size_t ws_bytes, void* stream);

/* bf16 -> fp32 widening of a flat buffer (gradient all-reduce decompression) */
int rg_widen_bf16(const void* src, float* dst, size_t n, void* stream);
/* fp32 -> dtype cast with optional row padding: dst[M][ldd] = src[M][K] (pad columns zeroed) */
int rg_cast_pad(const float* src, void* dst, int M, int K, int ldd, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hardware self-tests (used by tests/ on the GPU box): check the MFMA / transposed-LDS-read lane
 * maps this library relies on with exact integer data.  Return 0 when the layouts match.
 * ------------------------------------------------------------------------------------------- */
int rg_selftest_layouts(int* detail, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Resize-convolution block of DCGANUpGenerator (src/dcgan.py:45-56 and the last block :76-84):
 *   y[N][2H][2W][Cout] = Conv2d(Cin, Cout, 3, 1, 0)(ReflectionPad2d(1)(Upsample(x2, bilinear)(x[N][H][W][Cin]))) + bias
 * w[Cout][Cin][3][3] and bias[Cout] in PyTorch layout.  out_nchw_f32 / gy_nchw_f32 = 1: the image-side tensor is
 * NCHW fp32 (the generator's output block).  bf16 NHWC blocks run on the matrix cores: forward (Cin % 64 == 0) =
 * padded upsampled image materialised in the workspace + 9-tap stride-1 implicit GEMM with the bias in its epilogue;
 * data gradient (Cout % 64 == 0) = 9-tap full correlation onto the padded grid + adjoint of pad/upsample; weight
 * gradient = the pixel-contracting kernel of the 4x4 layers with 9 stride-1 taps.  Everything else (fp32, the NCHW
 * image block with Cout = 3): functor-GEMM kernels on the vector ALUs.
 * ------------------------------------------------------------------------------------------- */
size_t rg_upconv3_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int rg_upconv3_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                   int out_nchw_f32, int dtype, int algo, void* ws, size_t ws_bytes, void* stream);
/* gx[N][H][W][Cin] = d/dx of the block for the output gradient gy */
int rg_upconv3_bwd_data(const void* gy, int gy_nchw_f32, const float* w, void* gx, int N, int H, int W, int Cin,
                        int Cout, int dtype, int algo, void* ws, size_t ws_bytes, void* stream);
/* dw[Cout][Cin][3][3] (+)= weight gradient (the bias gradient is a column sum of gy: rg_col_sum / rg_nchw_chan_sum) */
int rg_upconv3_wgrad(const void* gy, int gy_nchw_f32, const void* x, float* dw, int N, int H, int W, int Cin, int Cout,
                     int dtype, int algo, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Split forms for synchronised (global-batch) statistics in a data-parallel run (--sync-stats): *_sums
 * writes the RANK-LOCAL column sums, the caller all-reduces them (tiny RCCL all-reduces), *_apply finishes with the
 * global sums and the global row count.  Forward statistics use rg_bn_stats + rg_bn_finalize(count = global) +
 * rg_bn_act; the penalty norm is one scalar all-reduce of rg_sqnorm's result.
 * ------------------------------------------------------------------------------------------- */
int rg_bn_bwd_sums(const void* z, const void* ga, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, float* s_gy, float* s_gyxh, int M, int C, float slope, int dtype, void* ws,
                   size_t ws_bytes, void* stream);
int rg_bn_bwd_apply(const void* z, const void* ga, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, const float* s_gy, const float* s_gyxh, void* gz, int M, int C, int M_total,
                    float slope, int dtype, void* stream);
int rg_bn_tangent_sums(const void* z, const void* zt, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, float* s_zt, float* s_xhzt, int M, int C, float slope, int dtype, void* ws,
                       size_t ws_bytes, void* stream);
int rg_bn_tangent_apply(const void* z, const void* zt, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, const float* s_zt, const float* s_xhzt, void* at, int M, int C, int M_total,
                        float slope, int dtype, void* stream);
/* raw3[3][C] = column sums of (gy*zt', qy, qy*xhat) of rg_bn_double_bwd's reduction */
int rg_bn_dbl_sums(const void* z, const void* qa, const void* zt, const void* ga1, const float* mean, const float* invstd,
                   const float* gamma, const float* beta, float* raw3, int M, int C, float slope, int dtype, void* ws,
                   size_t ws_bytes, void* stream);
/* dgamma / dbeta receive this rank's contribution (summed later by the gradient all-reduce); ws >= 5*C floats */
int rg_bn_dbl_apply(const void* z, const void* qa, const void* zt, const void* ga1, const float* mean, const float* invstd,
                    const float* gamma, const float* beta, const float* s_gy, const float* s_gyxh, const float* s_zt,
                    const float* s_xhzt, const float* raw3_global, const float* raw3_local, void* pz, float* dgamma,
                    float* dbeta, int accumulate, int M, int C, int M_total, float slope, int dtype, void* ws,
                    size_t ws_bytes, void* stream);
int rg_latent_stats(const float* u, const float* z, float* s, float* ss, int N, int E, void* stream);
int rg_latent_apply(const float* u, const float* z, const float* s, const float* ss, float* out, int N, int E, int N_total,
                    void* stream);

/* Generated images for export (src/gan_utils.py:236-241): y_nhwc[N][H][W][C] = x_nchw * 0.5 + 0.5 (the inverse of
 * the input normalisation, transforms.Normalize(-mean/std, 1/std) with mean = std = 0.5) in NHWC order. */
int rg_export_images_nhwc(const float* x_nchw, float* y_nhwc, int N, int C, int H, int W, void* stream);

/* Generator-only inference with eval-mode BatchNorm (torchgan's sample grid: generator.eval(); SURVEY 8 f1 / BASELINE
 * configs[4]): the folded BatchNorm affine and the LeakyReLU are applied to the fp32 accumulators in the conv epilogue,
 *   y = lrelu(conv(x) * scale[c] + shift[c], slope),  scale = gamma / sqrt(running_var + eps),  shift = beta - running_mean * scale
 * so an inference layer is ONE kernel (no statistics, no apply pass).  bf16 MFMA path only (RG_EUNSUPPORTED otherwise).
 * rg_g0_fwd_affine: the generator's first layer, scale / shift of length 16*C in the layer's (tap, c) column order. */
int rg_conv_up_affine(const void* x, const void* wup, void* y, int N, int Ho, int Wo, int O, int I, const float* scale,
                      const float* shift, float slope, void* ws, size_t ws_bytes, void* stream);
int rg_g0_fwd_affine(const float* z, const void* wp, void* y, int N, int E, int C, const float* scale, const float* shift,
                     float slope, void* ws, size_t ws_bytes, void* stream);

/* fp8 (OCP e4m3) operands for generator-only inference (BASELINE configs[4]: "Generator-only tile synthesis, batch 4096
 * fp8"): activations x8[N][Ho][Wo][O] and weights wup8[16][I][O] (rg_conv_up) / b8[Ncols][K] (plain GEMM: the generator's
 * first layer) are fp8 bytes, fp32 accumulation (v_mfma_f32_16x16x32_fp8_fp8, 128-deep k-tiles on the pipeline of
 * rg_conv8.hip), epilogue y = lrelu(acc * scale[c] + shift[c], slope) -- scale carries the folded BatchNorm AND the
 * per-column weight quantisation scale -- written as bf16 (out_fp8 = 0) or fp8 (1, the next fp8 layer's input).
 * rg_fp8_supported: 1 when a (M rows, K = taps * channels, Ncols) problem has an fp8 kernel (channels multiples of 128,
 * Ncols a multiple of 128, M >= 256 / 512); the caller keeps the layer in bf16 otherwise.
 * rg_cast_fp8: dst[i] = fp8(src[i] * mul).  rg_selftest_fp8: lane map of the fp8 MFMA and converter known answers. */
int rg_conv_up_fp8(const void* x8, const void* wup8, void* y, int N, int Ho, int Wo, int O, int I, const float* scale,
                   const float* shift, float slope, int out_fp8, void* stream);
int rg_gemm_fp8(const void* a8, const void* b8, void* y, int M, int K, int Ncols, const float* scale, const float* shift,
                float slope, int out_fp8, void* stream);
int rg_fp8_supported(int M, int K, int Ncols, int taps);
int rg_cast_fp8(const float* src, void* dst, size_t n, float mul, void* stream);
int rg_selftest_fp8(int* detail, void* stream);

/* Input contract of the discriminator (src/histopathology_gan.py:106-109: ToTensor + Normalize(0.5, 0.5); dataset
 * output src/read_data.py:339-342,366-370): dst[i] = ((float)src_u8[i] / 255 - mean) / std, element order unchanged
 * (uint8 CHW tiles stay CHW).  The same three fp32 operations as the host transform: bit-identical to it.  Lets the
 * loader hand over uint8 tiles (a quarter of the PCIe bytes) and normalise on the device. */
int rg_u8_to_norm(const void* src_u8, float* dst, size_t n, float mean, float stdv, void* stream);

/* The device-side input transform of the Trainer (rna_gan_amd.augment.InputTransform; rna_gan_amd/csrc/rg_augment.hip): normalise
 * a tile batch and apply one of the eight symmetries of the square (the dihedral group D4) per sample, in one launch.
 *   src   [N][C][S][S], RG_U8 or RG_F32;  dst [N][C][S][S] fp32 (the NCHW image the step's image-side kernels take)
 *   value RG_U8: v = ((float)b / 255.0f - mean) / stdv, the three fp32 operations of rg_u8_to_norm in the same order (a true
 *         division, no reciprocal, no contraction): bit-identical to it and to the host transform.  RG_F32: v is copied
 *         unchanged and mean / stdv are ignored (a loader that already normalised).
 *   codes device array of N ints, or NULL = code 0 for every sample.  Sample n uses c = codes[n] & 7 (any int is memory-safe);
 *         all C planes of a sample get the same code.  c = r + 4 f: flip left-right if f, then rotate counter-clockwise by r
 *         quarter turns (np.rot90(x[..., ::-1] if f else x, r, axes=(-2, -1))).  With T = S - 1, dst[i][j] = src[..]:
 *           0: [i][j]      1: [j][T-i]    2: [T-i][T-j]    3: [T-j][i]
 *           4: [i][T-j]    5: [j][i]      6: [T-i][j]      7: [T-j][T-i]
 * Any S >= 1; no workspace; no alignment beyond the element type's (S % 4 == 0 with a 4-byte-aligned uint8 / 16-byte-aligned
 * fp32 source and a 16-byte-aligned dst takes the vector path, same bits).  Nothing outside the two tensors is read or written;
 * src and dst must not overlap.  No host synchronisation, no allocation, safe under graph capture.  N == 0: RG_OK, nothing
 * launched.  RG_EINVAL (nothing launched) for a NULL src or dst, N < 0, C <= 0, S <= 0, a src_dtype other than RG_U8 / RG_F32,
 * or stdv == 0 with RG_U8; RG_EUNSUPPORTED for more than 2^31 - 1 tiles of 64 x 64.  No 16-bit type is involved: both builds
 * behave identically. */
int rg_tile_transform(const void* src, int src_dtype, float* dst, int N, int C, int S, const int* codes, float mean, float stdv,
                      void* stream);

/* The batch of a RESIDENT training set (rna_gan_amd.resident; rna_gan_amd/csrc/rg_augment.hip): gather, normalise and D4 in one
 * launch -- rg_tile_transform with a per-sample source tile.
 *   store [M][C][S][S] uint8, the whole set on the device;  dst [N][C][S][S] fp32
 *   index device array of N ints, or NULL = index[n] = n (then N <= M is required, and the output is bit-identical to
 *         rg_tile_transform(store, RG_U8, ...) on the first N tiles).  Repeated indices are allowed.
 *   dst[n] = the rg_tile_transform result for tile store[index[n]] under code codes[n] & 7 (codes NULL = 0): the same three
 *         separately rounded fp32 operations, the same code table.
 * Every source offset is computed in 64 bits.  The kernel never reads outside store[0 .. M): an index outside [0, M) is CLAMPED
 * to the nearest valid tile (negative -> 0, >= M -> M - 1).  That is a memory-safety guarantee, not an interface: callers
 * validate their indices.  No workspace; nothing outside dst is written; store and dst must not overlap; S % 4 == 0 with a
 * 4-byte-aligned store and a 16-byte-aligned dst takes the vector path for every gathered tile (C S S is then a multiple of 4),
 * same bits.  No host synchronisation, no allocation, safe under graph capture, any stream.  N == 0: RG_OK, nothing launched.
 * RG_EINVAL (nothing launched) for a NULL store or dst, M <= 0 with N > 0, N < 0, C <= 0, S <= 0, stdv == 0, or index == NULL
 * with N > M; RG_EUNSUPPORTED for more than 2^31 - 1 tiles of 64 x 64.  Both builds behave identically. */
int rg_tile_gather_transform(const uint8_t* store, long long M, const int* index, float* dst, int N, int C, int S,
                             const int* codes, float mean, float stdv, void* stream);

/* The batch of a RESIDENT expression table (rna_gan_amd.rna_tables; rna_gan_amd/csrc/rg_rows.hip): rows gathered by index into
 * a dense, zero padded fp32 batch in one launch -- what the betaVAE training loop takes as "rna_data".
 *   table [M][ld_table] fp32, of which columns [0, F) are read;  dst [N][ld_dst] fp32
 *   index device array of N ints, or NULL = index[n] = n (then N <= M is required).  Repeated indices are allowed.
 *   dst[n][c] = table[clamp(index[n], 0, M - 1)][c] for c < F, the bits unchanged;  dst[n][c] = 0 for F <= c < ld_dst.
 * Every offset is computed in 64 bits (index ld_table passes 2^31 elements at about 112 000 rows of 19 198).  The kernel never
 * reads outside table[0 .. M)[0 .. F): an index outside [0, M) is CLAMPED to the nearest valid row (negative -> 0, >= M ->
 * M - 1).  That is a memory-safety guarantee, not an interface: callers validate their indices.  No workspace, no allocation, no
 * host synchronisation; nothing outside dst[0 .. N)[0 .. ld_dst) is written; table and dst must not overlap.  Both buffers need
 * 4-byte alignment only: per row the kernel takes the widest access the actual addresses of the source row and of the
 * destination row allow (16-byte stores wherever a 16-byte-aligned chunk of the destination row lies inside it; 16-, 8- or
 * 4-byte loads), the same bits on every path.  A plain kernel node: safe under graph capture, any stream.  N == 0: RG_OK,
 * nothing launched.  RG_EINVAL (nothing launched) for a NULL table or dst, M <= 0 with N > 0, N < 0, F <= 0, ld_table < F,
 * ld_dst < F, or index == NULL with N > M; RG_EUNSUPPORTED for more than 2^31 - 1 workgroups (N ceil((ld_dst + 6) / 4 / 1024)).
 * No 16-bit type is involved: both builds behave identically. */
int rg_rows_gather_f32(const float* table, long long M, int F, long long ld_table, const int* index, float* dst, int N,
                       long long ld_dst, void* stream);

/* The device-side tile export(rna_gan_amd.export; rna_gan_amd/csrc/rg_export.hip): generated images -> uint8 tiles, quantised and
 * laid out in one launch, so a batch leaves the device as C bytes per pixel instead of 4 C.
 *   src   [N][C][H][W] fp32;  dst N C H W bytes
 *   flags RG_EXPORT_PLANAR   clear: dst [N][H][W][C], interleaved (a PNG, a tile record);  set: dst [N][C][H][W]
 *         RG_EXPORT_REVERSE  destination channel c takes source channel C - 1 - c (BGR for C = 3, the order of the tile records)
 *         RG_EXPORT_TRUNC    clear: the rounding rule;  set: the truncating rule
 *   value every step a separately rounded fp32 operation, no contraction, a true division, no reciprocal:
 *           v = (x - sub) / div      ((sub, div) = (-1, 2): bit for bit the value of rg_export_images_nhwc;
 *                                     (lo, max(hi - lo, 1e-5)): the min-max normalisation of an image grid)
 *           t = v * 255.0f + 0.5f    rounding rule (torchvision save_image's mul(255).add_(0.5));   t = v * 255.0f  truncating rule
 *           byte = 0 if !(t >= 0) (NaN and -0.0 included), 255 if t >= 255, otherwise t truncated toward zero
 * Any N >= 0, C >= 1, H, W >= 1; no workspace; src needs 4-byte and dst 1-byte alignment only (C == 3, W % 4 == 0, or the planar
 * layout with H W % 4 == 0, with a 16-byte-aligned src and a 4-byte-aligned dst take the vector paths, same bytes).  Nothing
 * outside the two tensors is read or written; they must not overlap.  No host synchronisation, no allocation, safe under graph
 * capture, any stream.  N == 0: RG_OK, nothing launched.  RG_EINVAL (nothing launched) for a NULL buffer, N < 0, C, H or W <= 0,
 * div == 0 or NaN, or an unknown flag bit; RG_EUNSUPPORTED for more than 2^31 - 1 workgroups.  No 16-bit type is involved: both
 * builds behave identically. */
#define RG_EXPORT_PLANAR 1
#define RG_EXPORT_REVERSE 2
#define RG_EXPORT_TRUNC 4
int rg_tile_export_u8(const float* src, uint8_t* dst, int N, int C, int H, int W, float sub, float div, int flags, void* stream);

/* Tile quality control on the device (rna_gan_amd.tissue; rna_gan_amd/csrc/rg_tissue.hip): what a tiler's acceptance rule needs to
 * know about a uint8 RGB tile -- Otsu thresholds, the tissue mask's coverage, luma percentiles -- as INTEGERS, so every value is
 * exact; fractions, percentile interpolation and the accept / low-contrast decisions are made on the host from them.
 *   tiles  N tiles of H x W pixels, 3 channels, uint8.  flags: RG_EXPORT_PLANAR clear: [N][H][W][3], set: [N][3][H][W];
 *          RG_EXPORT_REVERSE: the stored channel order is B, G, R.  No other bit.
 * Per tile, nothing shared between tiles:
 *   histograms  256 bins each of R, G, B and of s8 = (255 * (mx - mn)) / mx (integer division; 0 where mx == 0), mx / mn the
 *               pixel's largest / smallest channel: the HSV saturation on a fixed 8-bit grid.
 *   Otsu        on an integer histogram h: lo / hi the smallest / largest occupied bin, n = sum h, S = sum i h[i].  For every
 *               split k = lo .. hi - 1, in exactly this sequence of separately rounded fp64 operations (no contraction):
 *                 w1 = sum_{i <= k} h[i], w2 = n - w1, s1 = sum_{i <= k} i h[i], s2 = S - s1         (integers)
 *                 m1 = (double)s1 / (double)w1;  m2 = (double)s2 / (double)w2;  d = m1 - m2;
 *                 v = (((double)w1 * (double)w2) * d) * d;
 *               the threshold is the FIRST k with the largest v; lo == hi (a constant channel): the threshold is lo.
 *               Four thresholds tR, tG, tB, tS.
 *   raw mask    m = (s8 > tS) && !(R > tR && G > tG && B > tB) && R > rgb_min && G > rgb_min && B > rgb_min
 *   dilation    `dilate` (0..8) iterations of the 4-connected cross, background outside the tile: a pixel is set iff some raw-mask
 *               pixel lies within L1 distance `dilate` of it.
 *   luma        L = 2125 R + 7154 G + 721 B (<= 2 550 000); for each of the four ranks4[j] in [0, H W) the exact order statistic:
 *               the value at index ranks4[j] of the tile's ascending sorted L (a two-level histogram selection, no sort).
 *   stats  int32 [N][12]: tR, tG, tB, tS, raw_count, dilated_count, L[rank 0..3], 0, 0
 *   mask   NULL, or uint8 [N][H][W] that receives the dilated mask as 0 / 1.
 * ranks4: FOUR HOST ints, read before the launch.  workspace: rg_tile_qc_workspace_bytes(N, H, W) bytes of device memory, 4-byte
 * aligned, any content: the call zeroes what it accumulates into, so calling again on the same workspace gives the same answer.
 * Five launches on `stream`; the tile bytes are read twice.  No host synchronisation, no allocation, safe under
 * graph capture.  The results do not depend on N or on the other tiles.  N == 0: RG_OK, nothing launched.  RG_EINVAL (nothing
 * launched) for a NULL tiles / ranks4 / stats / workspace, N < 0, H or W <= 0, an unknown flag bit, rgb_min outside 0..255, dilate
 * outside 0..8, a rank outside [0, H W), misaligned stats / workspace, a short workspace; RG_EUNSUPPORTED for H W > 2^26 (beyond it
 * w1 w2 would no longer be exact in fp64) or more than 2^31 - 1 workgroups.  No 16-bit type is involved: both builds behave
 * identically. */
size_t rg_tile_qc_workspace_bytes(int N, int H, int W);
int rg_tile_qc(const uint8_t* tiles, int N, int H, int W, int flags, int rgb_min, int dilate, const int* ranks4, int32_t* stats,
               uint8_t* mask_or_null, void* workspace, size_t workspace_bytes, void* stream);

/* The tiler's device half (rna_gan_amd.tiler; rna_gan_amd/csrc/rg_tiler.hip): windows of a slide raster cropped and resized as
 * Pillow's 8-bit Image.resize does (bicubic with antialiasing), the erosion that closes a tissue mask, a box thumbnail.  Integer
 * arithmetic only, so every byte is exact.  Each is ONE plain kernel launch on `stream`: no host synchronisation, no allocation,
 * no workspace, safe under graph capture.  No 16-bit type is involved: both builds behave identically.
 *
 * rg_window_resize_u8
 *   raster   uint8 [RH][RW][3], interleaved, any alignment.  A pixel outside [0, RH) x [0, RW) reads as 0.  Byte offsets into it
 *            are 64-bit: RH RW 3 may exceed 2^32.
 *   origins  DEVICE int32 [N][2]: (x, y) of each window's top-left pixel, x the column; any values, negative or outside included.
 *   h, w     the read size of every window;  oh, ow  the output size;  out  uint8 [N][oh][ow][3], must not overlap the raster.
 *   flags    0, or RG_EXPORT_REVERSE: out holds B, G, R (the order of the tile records).
 *   xtab     DEVICE int32 [ow][2 + kx], ytab DEVICE int32 [oh][2 + ky]: per output index a row (xmin, count, k_0 .. k_{K-1}), zero
 *            padded -- Pillow's precompute_coeffs + normalize_coeffs_8bpc, made on the HOST in fp64 (rna_gan_amd.tiler.pillow_tables):
 *              scale = in / out; fs = max(scale, 1); support = 2.0 * fs; K >= (int)ceil(support) * 2 + 1
 *              center = (i + 0.5) * scale; xmin = max(0, (int)(center - support + 0.5)); xmax = min(in, (int)(center + support + 0.5))
 *              w_j = bicubic((j + xmin - center + 0.5) / fs), a = -0.5, j < count = xmax - xmin; summed left to right, each divided
 *              by the sum; k_j = (int)(w_j * 2^22 + 0.5) for w_j >= 0, (int)(w_j * 2^22 - 0.5) otherwise (both truncate toward zero)
 *   passes   horizontal first: per source row, output column and channel  t = clip(((1 << 21) + sum_j p[xmin + j] k_j) >> 22, 0, 255)
 *            (arithmetic shift), STORED AS A BYTE; then vertical, the same formula over those bytes with ytab.  The intermediate
 *            rounding is part of the contract.
 *   copy     w == ow: the columns are copied and xtab is not read (it may be NULL); h == oh likewise; both: a plain crop.
 *   RG_EINVAL (nothing launched): a NULL raster / origins / out, N < 0, a size <= 0, an unknown flag bit, misaligned origins or
 *   tables, a resized axis whose table is NULL or narrower than its K or wider than 35, out overlapping the raster.
 *   RG_EUNSUPPORTED: oh or ow > 1024, h or w > 8192, an axis that needs K > 35 (a scale above 8.5), more than 2^31 - 1 workgroups.
 *   N == 0: RG_OK, nothing launched.  A table that is not the contract's gives other bytes, never an access outside the raster or out.
 *
 * rg_mask_erode   mask, out: uint8 [N][H][W]; a byte != 0 is set.  out = 1 where every pixel within L1 distance `radius` (0..8) is
 *   set, everything outside the H x W rectangle counting as UNSET, else 0: scipy's binary_erosion(iterations = radius).  radius 0
 *   copies (as 0 / 1).  rg_tile_qc's dilated mask followed by this is the binary closing of the reference's thumbnail mask.
 *   RG_EINVAL: NULL buffer, N < 0, H or W <= 0, radius outside 0..8, out overlapping mask.  RG_EUNSUPPORTED: > 2^31 - 1 workgroups.
 *
 * rg_box_reduce_u8   raster uint8 [RH][RW][3] -> out uint8 [ceil(RH / f)][ceil(RW / f)][3]: per channel (sum + cnt / 2) / cnt over
 *   the f x f block, integer division, cnt the number of the block's pixels inside the raster.  RG_EINVAL: NULL buffer, RH or
 *   RW <= 0, f outside 1..64, out overlapping the raster. */
int rg_window_resize_u8(const uint8_t* raster, int RH, int RW, const int32_t* origins, int N, int h, int w, int oh, int ow,
                        const int32_t* xtab, int kx, const int32_t* ytab, int ky, uint8_t* out, int flags, void* stream);
int rg_mask_erode(const uint8_t* mask, uint8_t* out, int N, int H, int W, int radius, void* stream);
int rg_box_reduce_u8(const uint8_t* raster, int RH, int RW, int factor, uint8_t* out, void* stream);

/* Macenko stain normalisation of uint8 RGB tiles (rna_gan_amd.stain; rna_gan_amd/csrc/rg_stain.hip): the method of Macenko et al.
 * (2009) restated on fixed-point tables that the HOST builds in fp64 with rint, so that everything the device computes is an
 * INTEGER and every count, sum and byte is exact.  The fit of a set of tiles is three statistics passes with a little host
 * arithmetic between them; a fourth pass applies it.  tests/stain_refs.py restates all of it in numpy.
 *
 * Constants (rna_gan_amd.stain): IO 240 the white level; BETA 0.15 the stained-pixel floor on the optical density; ALPHA 1 the angle
 *   percentile; QOD 12 fixed-point bits of the optical density; QV 14 of the plane basis and the bin directions; K 1024 angle bins;
 *   QP 20 bits of the pseudo-inverse; CB 4096 concentration bins of width 2^CSH = 2^3 in Q12; QS 16, QH 14, QO 8 bits of the scale,
 *   the target stain matrix and the output optical density.
 * Conventions: every sum and product is exact in int64; >> is the arithmetic (floor) shift.
 * Host tables:
 *   od_lut[v] = rint(-ln((v + 1) / IO) 2^QOD), int32 [256]; negative for v >= IO, not clamped.  |od_lut[v]| <= 23170 is part of the
 *               contract (four squares then sum below 2^31): the table above reaches 22449.  beta_q = rint(BETA 2^QOD) = 614.
 *   dirs        int32 [K - 1][2]: for k = 1 .. K - 1, theta_k = -pi/2 + k pi / K, (rint(cos theta_k 2^QV), rint(sin theta_k 2^QV)).
 *   out_lut[j] = clip(rint(IO exp(-(j - OFF) / 2^QO)), 0, 255), uint8 [L]; OFF the smallest offset at which index 0 gives 255 (16),
 *               L the smallest length whose last entry is 0.
 * A pixel's optical density is od = od_lut[(R, G, B)]; it is STAINED when od_R, od_G and od_B are all >= beta_q.
 *   tiles  N tiles of H x W pixels, 3 channels, uint8, any alignment.  flags: RG_EXPORT_PLANAR clear: [N][H][W][3], set:
 *          [N][3][H][W]; RG_EXPORT_REVERSE: the stored channel order is B, G, R.  No other bit.
 *
 * rg_stain_moments     out int64 [10], over the stained pixels: the count, sum od_c (R, G, B), sum od_c od_d for (c, d) = RR, RG, RB,
 *                      GG, GB, BB.  Host: covariance (n S2 - S1 S1^T) / (n (n - 1)) / 2^(2 QOD), the numerator in exact integers;
 *                      numpy.linalg.eigh; the two leading eigenvectors e1, e2, each negated if its component sum is negative.
 * rg_stain_angle_hist  basis6: SIX HOST ints Eq1[3], Eq2[3] = rint(e 2^QV), each within +-30000.  Per stained pixel
 *                      p1 = sum od_c Eq1_c, p2 = sum od_c Eq2_c.  p1 <= 0: counted in hist[K] alone (outside).  Otherwise
 *                      bin = #{k in 1 .. K - 1 : cos_k p2 - sin_k p1 >= 0}, in 0 .. K - 1; the predicate is monotone in k for p1 > 0
 *                      (the quantised directions are strictly ordered by angle and have cos_k > 0), so the kernel finds the count by
 *                      binary search.  hist uint64 [K + 1].  2 <= K <= 2048.
 *                      Host: the percentile q (an integer) of a histogram is the first bin whose cumulative count exceeds
 *                      (q (total - 1)) / 100 (integer division), taken at the bin centre: phi = -pi/2 + (bin + 0.5) pi / K.
 *                      v = e1 cos phi + e2 sin phi for phi_ALPHA and phi_(100 - ALPHA); the column with the larger R component is
 *                      haematoxylin: HE (3 x 2).  Pq = rint(pinv(HE) 2^QP).
 * rg_stain_conc_hist   over ALL pixels: pinv6 SIX HOST long long Pq[stain][channel], each within +-2^40;
 *                      conc_s = (sum_c Pq[s][c] od_c) >> qp (Q12 for qp = QP); bin = clamp(conc_s >> csh, 0, bins - 1).
 *                      hist uint64 [2][bins].  1 <= bins <= 4096, 0 <= qp <= 40, 0 <= csh <= 31.
 *                      Host: max_conc_s = the centre of the 99th-percentile bin, (bin + 0.5) 2^CSH / 2^QOD.
 * rg_stain_apply       src -> dst, the same layout and channel order.  scale2: TWO HOST long long scale_q = rint(max_t / max_conc 2^QS)
 *                      >= 0; href6: SIX HOST ints Hq[channel][stain] = rint(HE_t 2^QH) of the target; shift = QH + QOD - QO.
 *                        conc2_s = (conc_s scale_q_s) >> qs
 *                        od2_c = (sum_s Hq[c][s] conc2_s + 2^(shift - 1)) >> shift          (no rounding term for shift == 0)
 *                        byte_c = out_lut[clamp(od2_c + off, 0, L - 1)]
 *                      One pass; dst == src is the in-place call, otherwise dst must not overlap src.  A lane takes four pixels
 *                      with dword loads and stores where src and dst are 4-byte aligned (planar: and H W % 4 == 0), single bytes
 *                      otherwise: the same bytes either way.  1 <= L <= 8192, 0 <= off < L, qp, qs, shift in 0 .. 40; operands so
 *                      large that a sum of the contract would leave int64 are refused.
 * accumulate == 0: the call zeroes its output first (a small kernel in front of the counting one); != 0: it adds to what is there, so a
 * set that arrives in batches gets the same integers in any order.  Device tables are staged in LDS; counting is integer LDS
 * atomics, then one 64-bit global integer atomic per occupied bin per workgroup: no floating-point atomics, so no result depends on
 * the launch plan.  Each entry point is one kernel launch (plus that zeroing one) on `stream`: no host synchronisation, no allocation,
 * safe under graph capture.  Only the stated buffers are read or written; a device table that is not the contract's gives other
 * numbers, never an access outside them.  N == 0: RG_OK, nothing launched and nothing zeroed.  RG_EINVAL (nothing launched) for a
 * NULL buffer, N < 0, H or W <= 0, an unknown flag bit, K, bins, L, off or a shift out of range, a host operand out of range, od_lut
 * or dirs not 4-byte aligned, out or hist not 8-byte aligned, dst partly overlapping src; RG_EUNSUPPORTED for more than 2^33
 * pixels per call (up to there sum od^2 stays exact in int64) or more than 2^31 - 1 workgroups.  No 16-bit type is involved: both
 * builds behave identically. */
int rg_stain_moments(const uint8_t* tiles, int N, int H, int W, int flags, const int32_t* od_lut, int beta_q, int64_t* out,
                     int accumulate, void* stream);
int rg_stain_angle_hist(const uint8_t* tiles, int N, int H, int W, int flags, const int32_t* od_lut, int beta_q, const int* basis6,
                        const int32_t* dirs, int K, uint64_t* hist, int accumulate, void* stream);
int rg_stain_conc_hist(const uint8_t* tiles, int N, int H, int W, int flags, const int32_t* od_lut, const long long* pinv6, int qp,
                       int csh, int bins, uint64_t* hist, int accumulate, void* stream);
int rg_stain_apply(const uint8_t* src, uint8_t* dst, int N, int H, int W, int flags, const int32_t* od_lut, const long long* pinv6,
                   int qp, const long long* scale2, int qs, const int* href6, int shift, const uint8_t* out_lut, int L, int off,
                   void* stream);

/* ---- memorisation audit: int8 tile descriptors and their exact nearest neighbours (rna_gan_amd/csrc/rg_nn.hip) ----
 * rna_gan_amd.nearest asks which training tiles a generated tile is closest to.  Tiles are compared through DESCRIPTORS: the tile
 * averaged over f x f blocks, recentred to int8.  Every quantity is an integer and is computed exactly; tests/nn_audit_refs.py
 * restates both entry points in numpy.
 *
 * rg_tile_descriptor_i8   tiles uint8 [N][C][S][S] -> desc int8 [N][ldd], norm2 int32 [N].  P = S / f, D = C P P:
 *                           desc[n][c P P + y P + x] = (sum of the f x f block (y, x) of channel c + f f / 2) / (f f) - 128
 *                         (integer division: round half up; bytes 0 and 255 give -128 and 127), columns D .. ldd - 1 = 0,
 *                         norm2[n] = sum_j desc[n][j]^2.  f in {1, 2, 4, 8, 16, 32}, S % f == 0, ldd % 64 == 0, ldd >= D.
 *                         D <= 32 768, else RG_EUNSUPPORTED: then D 255^2 < 2^31 and every norm, dot product and squared distance
 *                         fits int32.  One launch of N workgroups (a workgroup owns a tile, so norm2 is one block reduction); 16-byte
 *                         loads where S % 16 == 0, f <= 16 and tiles and desc are 16-byte aligned, single bytes otherwise: the same
 *                         integers.  No workspace.  N == 0: RG_OK, nothing launched.  RG_EINVAL (nothing launched) for a NULL
 *                         buffer, N < 0, C or S <= 0, a bad f, S % f != 0, a bad ldd, norm2 not 4-byte aligned, or desc / norm2
 *                         overlapping tiles or each other.  Only desc[N][ldd] and norm2[N] are written, only tiles is read.
 * rg_nn_topk_i8           a int8 [Q][ldd] with norms na2 int32 [Q], b int8 [N][ldd] with nb2 int32 [N]; columns 0 .. D - 1 of a row
 *                         are its descriptor (D % 64 == 0, D <= 32 768, ldd >= D, ldd % 16 == 0); columns beyond D are not read.
 *                           d2(q, r) = na2[q] + nb2[r] - 2 <a_q, b_r>          (int32; formed modulo 2^32 and read as unsigned, which
 *                                                                               is the distance itself when the norms are the rows')
 *                           key(q, r) = ((uint64) d2(q, r) << 32) | r
 *                         keys uint64 [Q][k] receives, ascending, the k smallest keys of query q over the candidate rows r: all of
 *                         [0, N) except exclude[q] (exclude: NULL, or int32 [Q]; a value outside [0, N) excludes nothing).  The
 *                         keys are one total order -- ties in d2 go to the lower row -- so the result depends neither on the tiling
 *                         nor on the sharing rule below nor on the run.  1 <= k <= 8.  The dot products are
 *                         v_mfma_i32_16x16x64_i8; no floating-point instruction, no atomic.
 *                         SHARING RULE: a workgroup owns 128 queries and walks consecutive 128-row tiles of b.  With
 *                         tiles = ceil(N / 128) and q_blocks = ceil(Q / 128), the tiles of a query block are cut into shares of
 *                         ceil(tiles / max(1, 1024 / q_blocks)) consecutive tiles, one workgroup each (Q <= 128: N > 128 already
 *                         gives two shares); each share's 8 best keys per query go to ws as [share][8][Q] and a second kernel, one
 *                         thread per query, merges them.  rg_nn_topk_ws_bytes(Q, N, k) is that size.  ws contents are irrelevant
 *                         before and after the call.  Two launches on `stream`; no host synchronisation, no allocation, safe under
 *                         graph capture.  Q == 0: RG_OK, nothing launched.
 *                         Fewer than k candidates is RG_EINVAL.  The host does not read exclude, so with exclude != NULL one row
 *                         counts as excluded whatever its values are: N - 1 >= k is required then, N >= k otherwise.
 *                         RG_EINVAL (nothing launched) also for a NULL a, na2, b, nb2 or keys, Q or N < 0, a bad D, ldd or k, a or b
 *                         not 16-byte, an int32 operand not 4-byte, keys or ws not 8-byte aligned; RG_EWORKSPACE for a NULL or short
 *                         workspace; RG_EUNSUPPORTED for D > 32 768 or more than 2^31 - 1 workgroups.
 * No 16-bit type is involved: both builds behave identically. */
int rg_tile_descriptor_i8(const uint8_t* tiles, int N, int C, int S, int f, int8_t* desc, long long ldd, int32_t* norm2, void* stream);
size_t rg_nn_topk_ws_bytes(int Q, long long N, int k);
int rg_nn_topk_i8(const int8_t* a, const int32_t* na2, int Q, const int8_t* b, const int32_t* nb2, long long N, int D, long long ldd,
                  int k, const int32_t* exclude, uint64_t* keys, void* ws, size_t ws_bytes, void* stream);

/* ---- MS-SSIM between pairs of uint8 RGB tiles (rna_gan_amd/csrc/rg_msssim.hip) ----
 * rna_gan_amd.msssim asks how similar pairs of tiles are in pixel space (Wang, Simoncelli & Bovik 2003); the mean over random
 * pairs of generated tiles is the diversity score of rna_gan_amd.metrics.PairDiversity.  tests/msssim_refs.py restates this in numpy.
 *
 * Definition, per channel of two tiles x, y of H x W:
 *   window   11 taps g (the host's fp64 Gaussian, sigma 1.5, normalised to sum 1), applied separably with valid extent: a level
 *            of h x w has (h - 10) (w - 10) window positions.
 *   pyramid  level 0 is the bytes; a pixel of level s is the exact integer sum of the aligned 2^s x 2^s block of bytes, divided
 *            by 4^s; h_s = H >> s, w_s = W >> s (a last odd row or column is dropped level by level).
 *   level    with the window means mx, my, E[x^2], E[y^2], E[xy]:  vx = E[x^2] - mx^2, vy likewise, cxy = E[xy] - mx my,
 *              cs = (2 cxy + C2) / (vx + vy + C2),   l = (2 mx my + C1) / (mx^2 + my^2 + C1),   C1 = 2.55^2, C2 = 7.65^2.
 *   result   out[P][S][3][2] fp64: per pair, level and channel (R, G, B) the SUMS of cs and of l cs over the window positions.
 *            The host divides by the position count, clamps, raises to the level weights and multiplies.
 *
 * rg_msssim_plan      S levels, 1 <= S <= 5, need min(H, W) >> (S - 1) >= 11.  info (NULL, or int32 [2 + 2 S]) receives
 *                     RG_MSSSIM_BAND, RG_MSSSIM_COLS, then (h_s, w_s) for s = 0 .. S - 1.  *pyramid_tile_bytes: what
 *                     rg_msssim_pyramid writes per tile (0 for S == 1); *pair_ws_bytes: the workspace of rg_msssim_pairs for P pairs.
 *                     Either may be NULL.  RG_EINVAL for H or W < 11, a bad S, P < 0; RG_EUNSUPPORTED for H or W > 4096 or more than
 *                     2^31 - 1 workgroups.
 * rg_msssim_pyramid   tiles: N tiles of H x W pixels, 3 channels, uint8, any alignment.  flags: RG_EXPORT_PLANAR clear:
 *                     [N][H][W][3], set: [N][3][H][W]; RG_EXPORT_REVERSE: the stored channel order is B, G, R.  No other bit.
 *                     pyr receives, per tile (pyramid_tile_bytes apart), levels 1 .. S - 1 one after the other, each uint16
 *                     [3][h_s][w_s] in R, G, B order: the block sums (at most 255 * 256).  2-byte aligned.  Built once per tile: the
 *                     pairs reuse it.  One launch; S == 1 or N == 0: RG_OK, nothing launched (pyr may be NULL for S == 1).
 * rg_msssim_pairs     pair p compares tile ia[p] of set a with tile ib[p] of set b (int32 on the device, [0, Na) and [0, Nb); the
 *                     host cannot see them: an index outside its set makes the six doubles per level of that pair NaN and is
 *                     never used as an address).  a and b may be the same set; both have the shape H x W and the layout `flags`.
 *                     pyr_a, pyr_b: their pyramids (NULL for S == 1).  taps: ELEVEN HOST doubles.
 *                     A workgroup owns RG_MSSSIM_BAND x RG_MSSSIM_COLS window positions of one level and channel of one pair: it
 *                     stages the (BAND + 10) x (COLS + 10) pixels of both tiles once in LDS, takes the five horizontal moments of
 *                     every staged row into LDS, the vertical pass and the two ratios out of it, and reduces in a fixed order to
 *                     one partial pair in ws; a second launch adds the partials of a (pair, level, channel) in ascending
 *                     workgroup order and WRITES out.  fp64 throughout, no atomics: the doubles of a pair depend on the two tiles'
 *                     bytes alone -- not on P, on the pair's position, on the other pairs or on which set a tile is read from.
 *                     ws: pair_ws_bytes, 8-byte aligned, contents irrelevant before and after.  Two launches on `stream`; no host
 *                     synchronisation, no allocation, safe under graph capture.  P == 0: RG_OK once shape, S and flags are
 *                     accepted; no pointer is looked at, nothing launched, nothing written.
 * Nothing is launched or written on an error: RG_EINVAL for a NULL tiles / index / taps / out buffer, a NULL pyramid with S > 1,
 * N, Na or Nb < 1 with work to do, P < 0, H or W < 11, a bad S, an unknown flag bit, a misaligned pyramid, index array, ws or out;
 * RG_EWORKSPACE for pyr_bytes below N pyramid_tile_bytes and for a NULL or short ws.  No 16-bit FLOAT type is involved: both builds behave identically. */
#define RG_MSSSIM_BAND 32
#define RG_MSSSIM_COLS 16
int rg_msssim_plan(int H, int W, int S, int P, int32_t* info, size_t* pyramid_tile_bytes, size_t* pair_ws_bytes);
int rg_msssim_pyramid(const uint8_t* tiles, int N, int H, int W, int flags, int S, void* pyr, size_t pyr_bytes, void* stream);
int rg_msssim_pairs(const uint8_t* a, const void* pyr_a, int Na, const uint8_t* b, const void* pyr_b, int Nb, const int32_t* ia,
                    const int32_t* ib, int P, int H, int W, int flags, int S, const double* taps, void* ws, size_t ws_bytes,
                    double* out, void* stream);

/* ---- the fp32 mode on the bf16 matrix cores, operands split ONCE PER TENSOR (rna_gan_amd/csrc/rg_conv8f.hip, rg_wgrad8f.hip) ----
 * The reference computes in fp32 (src/betaVAE.py:184,223; the GAN CLI never enables AMP).  An fp32 value is the exact sum of three
 * bf16 numbers v = h + m + l; rg_split_planes writes them as a plane-major buffer planes[3][n] (bf16, n % 8 == 0) in one
 * bandwidth-bound pass, and the stride-2 conv / transposed conv / weight gradient run the product's 8-wave bf16 kernels over
 * K-concatenated plane pairs with fp32 accumulation and an fp32 result:
 *   products = 6: hh hm mh hl lh mm -- every term down to 2^-24 |a b| (the f32 instruction's accuracy class)
 *   products = 3: hh hm mh          -- 2^-16 |a b| per product
 * x_planes: planes of the NHWC activation the bf16 entry point would take (rg_conv_down: [N][2Hlow][2Wlow][I]; rg_conv_up:
 * [N][Hlow][Wlow][O]); w_planes: planes of wdn[O][16][I] (down) / wup[16][I][O] (up); y fp32 NHWC.  stats_partial as rg_conv_down
 * (rg_f32p_conv_stats_rows rows; 0 = the launch splits K and writes none).  rg_f32p_wgrad: dw[O][16][I] (+)= one or two
 * (low, high) segments, all four operands as planes.  *_supported: 0 = use the RG_F32 entry points.  bf16 library only. */
int rg_split_planes(const float* src, void* planes_bf16, size_t n, void* stream);
int rg_f32p_conv_supported(int up, int N, int Hlow, int Wlow, int O, int I, int products);
size_t rg_f32p_conv_workspace_bytes(int up, int N, int Hlow, int Wlow, int O, int I, int products);
int rg_f32p_conv_stats_rows(int up, int N, int Hlow, int Wlow, int O, int I, int products);
int rg_f32p_conv(int up, const void* x_planes, const void* w_planes, float* y, int N, int Hlow, int Wlow, int O, int I,
                 int products, float* stats_partial, const float* mask_f32, float mask_slope, void* ws, size_t ws_bytes,
                 void* stream);
/* mask_f32 (optional, y's shape): y *= (mask > 0 ? 1 : mask_slope), the consumer's LeakyReLU backward as in rg_conv_up -- only
 * where rg_f32p_conv_mask_supported says 1 (the 64-column transposed conv); elsewhere the caller runs rg_lrelu_bwd behind it. */
int rg_f32p_conv_mask_supported(int up, int N, int Hlow, int Wlow, int O, int I, int products);
int rg_f32p_wgrad_supported(int N, int Ho, int Wo, int O, int I, int products);
size_t rg_f32p_wgrad_workspace_bytes(int N, int Ho, int Wo, int O, int I, int products, int two);
int rg_f32p_wgrad(const void* low0, const void* high0, const void* low1, const void* high1, float* dw, int N, int Ho, int Wo,
                  int O, int I, int products, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* On-box ceilings for the roofline object of bench.py ("re-measure both on the box (MFMA-loop and stream-copy
 * microbenchmarks) and report against both nominal and measured peak").  Measurement kernels only -- no product path calls
 * them; the caller times back-to-back launches with events on `stream`.  (rna_gan_amd/csrc/rg_probe.hip)
 * rg_probe_mfma_bare: `blocks` workgroups of 4 * waves_per_simd waves, each wave `iters` times the MFMAs of one 128 x 64 x 64
 *   wave k-tile (v_mfma_f32_16x16x32_bf16: mfma_shape 16, v_mfma_f32_32x32x16_bf16: 32) on random register operands.
 * rg_probe_lds_mfma: the product's 8-wave conv k-loop (conv8_kernel, 256 x 256 x 64 tile) over LDS-resident stages with its
 *   LDS-DMA issue compiled out; a[blocks * 256][128], b[256][128] bf16 operands, c[blocks * 256][256] bf16 result; iters even.
 * rg_probe_copy: float4 stream copy of nbytes (multiple of 16); variant 0 plain / 1 non-temporal loads and stores, `blocks`
 *   workgroups (0: 2048).  rg_probe_fill_bf16: n bf16 values uniform in [-1, 1).
 * *flops_out = algorithmic FLOPs of the launch. */
int rg_probe_mfma_bare(int mfma_shape, int waves_per_simd, int blocks, int iters, float* scratch, double* flops_out, void* stream);
int rg_probe_lds_mfma(int mfma_shape, int blocks, int iters, const void* a, const void* b, void* c, double* flops_out,
                      void* stream);
int rg_probe_copy(const void* src, void* dst, size_t nbytes, int variant, int blocks, void* stream);
int rg_probe_fill_bf16(void* p, size_t n, unsigned seed, void* stream);
/* The two-launch form of rg_window_resize_u8 (rna_gan_amd/csrc/rg_tiler.hip), kept to be measured against (tools/ab_tiler.py): the
 * same arguments, refusals and bytes, with the byte intermediate [N][h][ow][3] in `workspace` (N h ow 3 bytes).  Like every probe
 * it is not bound in the fp16 build's table and no product path calls it. */
int rg_probe_window_resize_2pass(const uint8_t* raster, int RH, int RW, const int32_t* origins, int N, int h, int w, int oh, int ow,
                                 const int32_t* xtab, int kx, const int32_t* ytab, int ky, uint8_t* out, int flags, void* workspace,
                                 size_t workspace_bytes, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* RNAGAN_HIP_H */
