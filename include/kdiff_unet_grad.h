/* C ABI of the image_v1 U-Net's reverse (VJP) kernels in libkdiff_hip.so (csrc/unet_vjp_f32.hip): the entry points that
 * ImageDenoiserModelV1.forward_vjp walks back through beside kd_conv2d_x3 (on the transposed, flipped weight), kd_attn_global_vjp_f32,
 * kd_unet_in_f32 / kd_unet_out_f32 (each other's transposes) and kd_precond_vjp_f32 of kdiff_hip.h.
 *
 * Conventions are those of kdiff_hip.h: every function returns KD_OK (0) or a negative error code with the message in kd_last_error();
 * `stream` is a hipStream_t (NULL: the default stream); activations and gradients are fp32 NHWC token rows [batch * H * W, chan] with a row
 * stride in floats (ld*), so that an operand may be a column range of a wider buffer; rows stay 16-byte aligned.  No kernel uses atomics or
 * reads a library option; every sum has a fixed order, so a repeat gives the same bits.  The binding (_native.GRAD_SIGNATURES) is read from
 * this file by the parser that reads kdiff_hip.h, and none of these can be named in a kd_run_list.
 *
 * kd_adagn_vjp_stats_f32   gstats [batch, groups, 4] = {m1, m2, 0, 0} per (sample, group): m1 = mean(g_xh), m2 = mean(g_xh * xh) over the
 *                     group's (chan / groups channels x hw pixels), where xh = (x - mean) * rstd from `stats` (as kd_groupnorm_stats_f32 writes
 *                     them: the fp64 mean as mean_hi + mean_lo), pre = xh * (1 + w_b) + b_b with (w_b, b_b) from `wb` as in
 *                     kd_adagn_apply_f32, g_pre = g_y * (Phi(pre) + pre * phi(pre)) with `gelu` (exact erf form), else g_y, and g_xh = g_pre *
 *                     (1 + w_b).  Terms and sums in fp64, one workgroup per (sample, group).  Groups of a multiple of 4 channels.
 * kd_adagn_vjp_apply_f32   g_x = rstd * (g_xh - m1 - xh * m2) + g_add: the gradient of kd_adagn_apply_f32 (+ GELU) w.r.t. x, the conditioning
 *                     held fixed, plus the gradient g_add (row stride ldga; may be NULL) of whatever else read x (a residual block's skip).
 *                     g_x may be g_y or g_add (same row stride), not x.
 * kd_down2_vjp_f32    the transpose of kd_down2_f32: g_x [H, W] from g_y [H / 2, W / 2] (H, W even, >= 2), the reflected taps folded back.
 * kd_up2_vjp_f32      the transpose of kd_up2_f32: g_x [H, W] from g_y [2 H, 2 W] (H, W >= 2).
 *                     Both are gathers (one thread per g_x element); with `accumulate` the sum is added to what g_x holds (the skip's
 *                     gradient), otherwise it replaces it.  g_x must not overlap g_y. */
#ifndef KDIFF_UNET_GRAD_H
#define KDIFF_UNET_GRAD_H

#ifdef __cplusplus
extern "C" {
#endif

int kd_adagn_vjp_stats_f32(const float* x, int ldx, const float* stats, const float* wb, int wb_stride, const float* g_y, int ldgy, float* gstats,
                           int batch, int hw, int chan, int groups, int gelu, void* stream);
int kd_adagn_vjp_apply_f32(const float* x, int ldx, const float* stats, const float* gstats, const float* wb, int wb_stride, const float* g_y,
                           int ldgy, const float* g_add, int ldga, float* g_x, int ldgx, int batch, int hw, int chan, int groups, int gelu,
                           void* stream);
int kd_down2_vjp_f32(const float* g_y, int ldgy, float* g_x, int ldgx, int batch, int H, int W, int chan, int accumulate, void* stream);
int kd_up2_vjp_f32(const float* g_y, int ldgy, float* g_x, int ldgx, int batch, int H, int W, int chan, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif

#endif
