/* C ABI of the image_v1 U-Net's bf16 weight-gradient arithmetic in libkdiff_hip.so (csrc/conv_wgrad_bf16.hip): what
 * ImageDenoiserModelV1.set_wgrad_arithmetic("bf16") launches in place of kd_conv2d_wgrad_x3 (kdiff_unet_train.h); the weight-gradient GEMMs of
 * the same setting are kd_wgrad_f32's bf16 form in kdiff_hip.h.
 *
 * Conventions are those of kdiff_hip.h and kdiff_unet_train.h.  The kernel uses no atomics and reads no library option; a repeat gives the same
 * bits.  The binding (_native.MIXED_SIGNATURES) is read from this file by the parser that reads kdiff_hip.h, and the entry point cannot be
 * named in a kd_run_list.
 *
 * kd_conv2d_wgrad_bf16 dw[co, ci, ky, kx] (+)= scale(co) * sum over (b, y, x) of bf16(g[b, y, x, co]) * bf16(a[b, y + ky - h, x + kx - h, ci]),
 *                      h = ks / 2: kd_conv2d_wgrad_x3's contract -- arguments, layouts, row strides, zero selection outside the image, the
 *                      chunking and its workspace ws [nchunk, ks * ks, c_out, c_in], the ascending second pass, q_rows, accumulate and the
 *                      refusals -- in bf16 arithmetic: every operand is rounded once to bf16 (round to nearest even, torch.Tensor.bfloat16()'s
 *                      rounding) while it is staged, a product is one v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  scale(co) is a power
 *                      of two and stays exact. */
#ifndef KDIFF_UNET_MIXED_H
#define KDIFF_UNET_MIXED_H

#ifdef __cplusplus
extern "C" {
#endif

int kd_conv2d_wgrad_bf16(const float* g, int ldg, const float* a, int lda, float* ws, float* dw, int batch, int H, int W, int c_in, int c_out, int ks,
                         int q_rows, int patches_per_chunk, int nchunk, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif

#endif
