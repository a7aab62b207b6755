/* C ABI of the image_v1 U-Net's DROPOUT kernels in libkdiff_hip.so (csrc/unet_drop_f32.hip, csrc/conv_x3.hip, csrc/vjp_f32.hip): what
 * ImageDenoiserModelV1.loss_forward launches in training mode once enable_dropout() was called, beside the kernels of kdiff_hip.h,
 * kdiff_unet_grad.h and kdiff_unet_train.h.  The reference's sites (k_diffusion/models/image_v1.py:15-29, k_diffusion/layers.py:181-200):
 * a ResConvBlock runs AdaGN, GELU, Conv3x3, Dropout2d, AdaGN, GELU, Conv3x3, Dropout2d and adds the skip -- Dropout2d zeroes whole (sample,
 * channel) feature maps; SelfAttention2d hands dropout_p to scaled_dot_product_attention -- the mask is on the softmax PROBABILITIES, and there
 * is no dropout behind out_proj.
 *
 * Conventions are those of the other three headers: every function returns KD_OK (0) or a negative error code with the message in
 * kd_last_error(); `stream` is a hipStream_t (NULL: the default stream); activations and gradients are fp32 NHWC token rows
 * [batch * H * W, chan] with a row stride in floats (ld*).  No kernel uses atomics or reads a library option; a repeat gives the same bits.
 * The binding (_native.DROP_SIGNATURES) is read from this file by the parser that reads kdiff_hip.h, and none of these can be named in a
 * kd_run_list.
 *
 * No mask is stored: the primal, the backward's recomputation and the reverse rules regenerate the same bits.
 * Mask contract (the generator, threshold and scale of the dropout contract of kdiff_hip.h):
 *   key       one int64 per loss call, drawn on the device and read through a pointer (the kernels never sync with the host);
 *   site s    the layer at position L of the forward walk (models/image_v1.py: dropout_sites): a residual block has 2^62 | 2^33 | (2 L)
 *             behind its first convolution and 2^62 | 2^33 | (2 L + 1) behind its second, an attention layer 2^62 | 2^33 | (2 L).  Bit 62 set,
 *             bit 63 clear, bit 33 set: disjoint from the transformer's 2^62 | 2 i, 2^62 | (2 i + 1) (i < 2^31) and 2^62 | 2^32 | k (k < 2^32);
 *   element e channel site: the tensor is [batch, chan], e = b * chan + c;
 *             attention site: the tensor is [batch, nh, T, T4] with T4 = 4 * ceil(T / 4), e = ((b * nh + h) * T + i) * T4 + j for query i and
 *             key j < T -- every probability row starts on a counter boundary, so one generator call serves four consecutive keys;
 *   mask      w = word e & 3 of philox4x32_10(key, counter (e >> 2, s)) (csrc/philox.h); keep iff w >= threshold, threshold = floor(p 2^32);
 *             m = keep ? scale : 0 with scale = (float)(1 / (1 - p)) computed in double.  threshold 0 keeps everything.
 *
 * kd_chan_mask_f32    table[b, off_k + c] = m of channel site k at element b * chan_k + c, for ALL n_sites channel sites of a loss call in one
 *                     launch: `sites` is a device array of n_sites (site id, column offset off_k, chan_k) int64 triples; table has `batch` rows
 *                     of table_stride floats, and every off_k + chan_k <= table_stride (the CALLER's check: the triples live on the device).
 * kd_conv2d_x3_drop   kd_conv2d_x3 with a channel mask in its epilogue: y[b, pixel, n] = (acc + bias[n]) * chan_scale[b * chan_stride + n] + res.
 *                     chan_scale is a site's column range of the table.  NULL: kd_conv2d_x3 itself, the same code path and the same bits.
 *                     A dropped channel gets exactly res (or 0).
 * kd_chan_scale_f32   out[row, c] = g[row, c] * chan_scale[(row / hw) * chan_stride + c] over batch * hw rows: the transpose of the mask on a
 *                     gradient.  16-byte accesses: chan, ldg, ldo and chan_stride multiples of 4, 16-byte aligned pointers.  out may be g.
 * kd_attn_global_drop_f32      dense softmax attention with dropout on the probabilities, fp32 FMAs, heads of 64, any T: qkv [batch, T, 3 nh 64]
 *                     with whatever scale is wanted already in q, out [batch, T, nh 64]; O_i = sum_j P_ij M_ij v_j, P = softmax over j of q_i . k_j.
 * kd_attn_global_drop_vjp_f32  its reverse rule, kd_attn_global_vjp_f32's two recomputing passes with the mask: dP_ij = M_ij (gO_i . v_j),
 *                     D_i = sum_j P_ij dP_ij (= gO_i . O_i), dS_ij = P_ij (dP_ij - D_i), dV_j = sum_i P_ij M_ij gO_i, dQ_i = sum_j dS_ij k_j,
 *                     dK_j = sum_i dS_ij q_i.  g_qkv has qkv's shape; lse and dsum are [batch, nh, T] workspaces written in full. */
#ifndef KDIFF_UNET_DROP_H
#define KDIFF_UNET_DROP_H

#ifdef __cplusplus
extern "C" {
#endif

int kd_chan_mask_f32(const long long* key, const long long* sites, int n_sites, unsigned threshold, float scale, float* table, int table_stride,
                     int batch, void* stream);
int kd_conv2d_x3_drop(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, const float* chan_scale,
                      int chan_stride, float* y, int ldy, int batch, int H, int W, int c_in, int c_out, int ks, void* stream);
int kd_chan_scale_f32(const float* g, int ldg, const float* chan_scale, int chan_stride, float* out, int ldo, int batch, int hw, int chan,
                      void* stream);
int kd_attn_global_drop_f32(const float* qkv, float* out, int batch, int T, int nh, const long long* key, unsigned long long site,
                            unsigned threshold, float scale, void* stream);
int kd_attn_global_drop_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int T, int nh,
                                const long long* key, unsigned long long site, unsigned threshold, float scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif
