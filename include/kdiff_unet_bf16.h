/* C ABI of the image_v1 U-Net's bf16 convolution arithmetic in libkdiff_hip.so (csrc/conv_bf16.hip): what
 * ImageDenoiserModelV1.set_conv_arithmetic("bf16") launches in place of kd_conv2d_x3 (kdiff_hip.h) in the sampling forward.
 *
 * Conventions are those of kdiff_hip.h.  The kernel uses no atomics and reads no library option; a repeat gives the same bits.  The binding
 * (_native.UNET_BF16_SIGNATURES) is read from this file by the parser that reads kdiff_hip.h, and the entry point cannot be named in a
 * kd_run_list.
 *
 * kd_conv2d_bf16 y[b, y, x, n] = bias[n] + res[b, y, x, n] + sum over (ky, kx, c) of bf16(w[n, c, ky, kx]) * bf16(x[b, y + ky - h, x + kx - h, c]),
 *                h = ks / 2: kd_conv2d_x3's contract -- arguments, the fp32 NHWC token buffers and their row strides, ks 1 or 3 with zero
 *                padding ks / 2, bias (or NULL), residual (or NULL) and the output's row stride in the epilogue, zero selection outside the
 *                image (such a position is never loaded) and the refusals -- in bf16 arithmetic: every activation is rounded once to bf16
 *                (round to nearest even, torch.Tensor.bfloat16()'s rounding) while it is staged, every weight is its bf16 rounding, a product
 *                is one v_mfma_f32_32x32x16_bf16 with fp32 accumulation; bias and residual are added in fp32.  wp is kd_pack_conv_x3's image:
 *                its first plane (hi = bf16(w)) is the rounded weight, and the only plane read. */
#ifndef KDIFF_UNET_BF16_H
#define KDIFF_UNET_BF16_H

#ifdef __cplusplus
extern "C" {
#endif

int kd_conv2d_bf16(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy, int batch, int H, int W,
                   int c_in, int c_out, int ks, void* stream);

#ifdef __cplusplus
}
#endif

#endif
