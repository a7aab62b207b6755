// Channel dropout (the reference's nn.Dropout2d, k_diffusion/models/image_v1.py:22,26) of the image_v1 U-Net's training loss (gfx950): the
// table of per-(sample, channel) factors of one loss call, and the mask's transpose on a gradient.  The mask itself rides in the convolution's
// epilogue (conv_x3.hip: kd_conv2d_x3_drop); the attention layers' probability dropout is in vjp_f32.hip.  Contract: include/kdiff_unet_drop.h.
//
//   kd_chan_mask_f32   table[b, off_k + c] = keep ? scale : 0 for every channel site k of a loss call in ONE launch (as the AdaGN table is filled
//                      for all mappers at once): workgroup row k walks site k's batch * chan_k elements, one Philox block per 4 of them per lane.
//   kd_chan_scale_f32  out[row, c] = g[row, c] * table[b(row), c]: a streaming pass, one 16-byte load and store per lane, out may be g (every
//                      element is read and written by the same lane).
// No kernel uses atomics or reads a library option.
#include "kd_common.h"
#include "philox.h"
#include "../../include/kdiff_unet_drop.h"

namespace kd {

namespace {

__global__ __launch_bounds__(256) void chan_mask_kernel(const long long* __restrict__ key_ptr, const long long* __restrict__ sites,
                                                        unsigned threshold, float scale, float* __restrict__ table, int table_stride, int batch) {
  const unsigned long long key = (unsigned long long)key_ptr[0];
  const long long* st = sites + 3 * (long)blockIdx.y;
  const unsigned long long site = (unsigned long long)st[0];
  const long off = (long)st[1], chan = (long)st[2];
  const long n = (long)batch * chan, quads = (n + 3) >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    const Philox4 r = philox4x32_10(key, (unsigned long long)q, site);
    for (int k = 0; k < 4 && 4 * q + k < n; ++k) {
      const long e = 4 * q + k, b = e / chan, c = e - b * chan;
      table[b * table_stride + off + c] = philox_word(r, k) >= threshold ? scale : 0.0f;
    }
  }
}

__global__ __launch_bounds__(256) void chan_scale_kernel(const float* g, int ldg, const float* __restrict__ m, int lds, float* out, int ldo,
                                                         long rows, int hw, int cv) {
  const long n = rows * cv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long row = i / cv;
    const int c4 = (int)(i - row * cv) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + row * ldg + c4);
    const f32x4 s = *reinterpret_cast<const f32x4*>(m + (row / hw) * lds + c4);
    *reinterpret_cast<f32x4*>(out + row * ldo + c4) = v * s;
  }
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_chan_mask_f32(const long long* key, const long long* sites, int n_sites, unsigned threshold, float scale, float* table,
                                int table_stride, int batch, void* stream) {
  if (!key || !sites || !table || n_sites <= 0 || n_sites > 65535 || table_stride <= 0 || batch <= 0)
    return fail(KD_EINVAL, "kd_chan_mask_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("chan_mask_f32", 0, 4.0 * batch * table_stride, s);
  // (a site has batch * chan elements, a few thousand: 8 workgroups of 256 lanes x 4 elements cover 8192 per sweep)
  launch<chan_mask_kernel>(dim3(8, (unsigned)n_sites), dim3(256), 0, s, key, sites, threshold, scale, table, table_stride, batch);
  return check_launch("kd_chan_mask_f32");
}

extern "C" int kd_chan_scale_f32(const float* g, int ldg, const float* chan_scale, int chan_stride, float* out, int ldo, int batch, int hw,
                                 int chan, void* stream) {
  if (!g || !chan_scale || !out || batch <= 0 || hw <= 0 || chan <= 0) return fail(KD_EINVAL, "kd_chan_scale_f32: bad arguments");
  if (ldg < chan || ldo < chan || chan_stride < chan) return fail(KD_EINVAL, "kd_chan_scale_f32: a row stride is shorter than its row");
  if ((chan | ldg | ldo | chan_stride) & 3) return fail(KD_EINVAL, "kd_chan_scale_f32: chan = %d and the strides %d, %d, %d must be multiples of 4", chan, ldg, ldo, chan_stride);
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(chan_scale) | reinterpret_cast<uintptr_t>(out)) & 15)
    return fail(KD_EINVAL, "kd_chan_scale_f32: g, chan_scale and out must be 16-byte aligned");
  const long rows = (long)batch * hw;
  if (rows > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_chan_scale_f32: %ld rows exceed the index range", rows);
  const long n = rows * (chan / 4);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("chan_scale_f32", 0, 8.0 * rows * chan, s);
  launch<chan_scale_kernel>(dim3((unsigned)std::min<long>((n + 255) / 256, 8192)), dim3(256), 0, s, g, ldg, chan_scale, chan_stride, out, ldo, rows,
                            hw, chan / 4);
  return check_launch("kd_chan_scale_f32");
}
