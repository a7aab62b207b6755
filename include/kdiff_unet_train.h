/* C ABI of the image_v1 U-Net's PARAMETER-gradient kernels in libkdiff_hip.so (csrc/conv_wgrad_x3.hip, csrc/unet_train_f32.hip): what
 * ImageDenoiserModelV1.loss_forward's backward launches beside the reverse walk of kdiff_unet_grad.h and kd_wgrad_f32 / kd_colsum_f32 /
 * kd_cond_mlp_f32 of kdiff_hip.h (the conditioning chain, proj_in and proj_out).
 *
 * Conventions are those of kdiff_hip.h and kdiff_unet_grad.h: every function returns KD_OK (0) or a negative error code with the message in
 * kd_last_error(); `stream` is a hipStream_t (NULL: the default stream); activations and gradients are fp32 NHWC token rows
 * [batch * H * W, chan] with a row stride in floats (ld*), so that an operand may be a column range of a wider buffer.  No kernel uses atomics
 * or reads a library option; every sum has a fixed order that depends on the shape (and the chunking handed in) alone, so a repeat gives the
 * same bits.  The binding (_native.TRAIN_SIGNATURES) is read from this file by the parser that reads kdiff_hip.h, and none of these can be
 * named in a kd_run_list.
 *
 * kd_conv2d_wgrad_x3   dw[co, ci, ky, kx] (+)= scale(co) * sum over (b, y, x) of g[b, y, x, co] * a[b, y + ky - h, x + kx - h, ci], h = ks / 2:
 *                      the weight gradient of nn.Conv2d(c_in, c_out, ks, padding = ks / 2), ks 1 or 3, in the layer's own [c_out, c_in, ks, ks]
 *                      layout, from the gradient g on its output (row stride ldg) and its input a (row stride lda).  Positions outside the image
 *                      are selected to zero and never loaded.  c_in and c_out multiples of 64.  Split-bf16 x 3 arithmetic: every fp32 operand is
 *                      hi + lo bf16, a product is three v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  The sum over pixels is cut into
 *                      `nchunk` runs of `patches_per_chunk` consecutive 8 x 8 patches (patches counted sample-major, then row-major; nchunk =
 *                      ceil(batch * ceil(H / 8) * ceil(W / 8) / patches_per_chunk)); every run's partial goes to ws [nchunk, ks * ks, c_out, c_in]
 *                      floats, and a second pass adds the partials in ascending order.  scale(co) = 1 / 8 for co < q_rows, else 1: a qkv
 *                      projection runs with 1 / 8 folded into its q rows, and the gradient of the STORED weight is 1 / 8 of the folded one.
 *                      With `accumulate` the sum is added to what dw holds, otherwise it replaces it.
 * kd_adagn_wb_grad_f32 per (sample, channel) g_wb[b, c] = sum over pixels of g_pre * xh and g_wb[b, chan + c] = sum over pixels of g_pre: the
 *                      gradient of the (weight, bias) pair that kd_adagn_apply_f32 reads from `wb`, with xh, g_pre and `gelu` as
 *                      kd_adagn_vjp_stats_f32 defines them.  g_wb (row stride g_wb_stride) is the mapper's column range of the call's
 *                      [batch, sum of 2 chan] gradient table: the w part, then the b part, as chunk(2) cuts them.  Terms and sums in fp64.
 * kd_gelu_vjp_f32      g_x[i] = g_y[i] * (Phi(pre[i]) + pre[i] * phi(pre[i])): the reverse of the exact (erf) GELU at the pre-activation
 *                      `pre`, n elements, evaluated in fp64.  g_x may be g_y.
 * kd_bias_grad_f32     out[c] (+)= scale(c) * sum over rows of g[row, c], the sums in fp64: runs of 256 rows go to ws [ceil(rows / 256), cols]
 *                      DOUBLES, and a second pass adds them in ascending order.  `nchw` = 0: g is token rows [rows, cols] with row stride ldg;
 *                      `nchw` = hw > 0: g is an NCHW image [rows / hw, cols, hw] (a projection to image channels) and ldg is ignored.
 *                      scale(c) = 1 / 8 for c < q_cols, else 1 (the q part of a qkv bias). */
#ifndef KDIFF_UNET_TRAIN_H
#define KDIFF_UNET_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

int kd_conv2d_wgrad_x3(const float* g, int ldg, const float* a, int lda, float* ws, float* dw, int batch, int H, int W, int c_in, int c_out, int ks,
                       int q_rows, int patches_per_chunk, int nchunk, int accumulate, void* stream);
int kd_adagn_wb_grad_f32(const float* x, int ldx, const float* stats, const float* wb, int wb_stride, const float* g_y, int ldgy, float* g_wb,
                         int g_wb_stride, int batch, int hw, int chan, int groups, int gelu, void* stream);
int kd_gelu_vjp_f32(const float* pre, const float* g_y, float* g_x, int n, void* stream);
int kd_bias_grad_f32(const float* g, int ldg, void* ws, float* out, int rows, int cols, int nchw, int q_cols, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif

#endif
