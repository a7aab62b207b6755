// Dropout of the HDiT training loss (gfx950): the reference's nn.Dropout sites (image_transformer_v2.py:394, :441, :474, :491, :564) on
// counter-based masks that the primal, the backward's recomputation and the reverse walk regenerate instead of storing.
//
//   kd_dropout_f32       y = x * m, m = keep ? scale : 0 (y may be x): the attention output and the FF hidden in the primal, and the
//                        gradient through the same site in the reverse walk (dropout is its own transpose)
//   dropout_bits_kernel  the site's mask as bits, word w bit j = keep(32 w + j): what the weight-gradient prologue reads
//                        (kd_wgrad_drop_f32 launches it), so that its per-element cost is one cached word load instead of a Philox block
//
// Mask contract (include/kdiff_hip.h): element e of site s keeps iff word e & 3 of philox4x32_10(key, e >> 2, s) >= threshold.  The key
// is read through a device pointer (the loss call draws it on the device: no host sync).
#include "kd_common.h"
#include "philox.h"

namespace kd {

namespace {

// one Philox block per 4 elements per lane; 16-byte loads and stores when both pointers allow it, the n % 4 tail one element at a time
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float* x, float* y, long n, const long long* __restrict__ key_ptr,
                                                      unsigned long long site, unsigned threshold, float scale) {
  const unsigned long long key = (unsigned long long)key_ptr[0];
  const long quads = (n + 3) >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    const Philox4 r = philox4x32_10(key, (unsigned long long)q, site);
    const long e = 4 * q;
    if (VEC && e + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(x + e);
      float4 o;
      o.x = v.x * (r.x0 >= threshold ? scale : 0.0f);
      o.y = v.y * (r.x1 >= threshold ? scale : 0.0f);
      o.z = v.z * (r.x2 >= threshold ? scale : 0.0f);
      o.w = v.w * (r.x3 >= threshold ? scale : 0.0f);
      *reinterpret_cast<float4*>(y + e) = o;
    } else {
      for (int j = 0; j < 4 && e + j < n; ++j) y[e + j] = x[e + j] * (philox_word(r, j) >= threshold ? scale : 0.0f);
    }
  }
}

__global__ __launch_bounds__(256) void dropout_bits_kernel(unsigned* __restrict__ bits, long words, const long long* __restrict__ key_ptr,
                                                           unsigned long long site, unsigned threshold) {
  const unsigned long long key = (unsigned long long)key_ptr[0];
  for (long w = (long)blockIdx.x * 256 + threadIdx.x; w < words; w += (long)gridDim.x * 256) {
    unsigned b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const Philox4 r = philox4x32_10(key, (unsigned long long)(8 * w + i), site);
      b |= (r.x0 >= threshold ? 1u : 0u) << (4 * i);
      b |= (r.x1 >= threshold ? 1u : 0u) << (4 * i + 1);
      b |= (r.x2 >= threshold ? 1u : 0u) << (4 * i + 2);
      b |= (r.x3 >= threshold ? 1u : 0u) << (4 * i + 3);
    }
    bits[w] = b;
  }
}

unsigned drop_grid(long work) { return (unsigned)std::min<long>((work + 255) / 256, 16384); }

}  // namespace

// (not exported: wgrad_f32.hip's kd_wgrad_drop_f32 launches it ahead of its GEMM)
int launch_dropout_bits(unsigned* bits, long long n, const long long* key, unsigned long long site, unsigned threshold, hipStream_t s) {
  const long words = (long)((n + 31) >> 5);
  LaunchScope prof("dropout_bits", 0, 4.0 * words, s);
  hipLaunchKernelGGL(dropout_bits_kernel, dim3(drop_grid(words)), dim3(256), 0, s, bits, words, key, site, threshold);
  return check_launch("kd_dropout_bits");
}

}  // namespace kd

using namespace kd;

extern "C" int kd_dropout_f32(const float* x, float* y, long long n, const long long* key, unsigned long long site, unsigned threshold, float scale,
                              void* stream) {
  if (!x || !y || !key || n <= 0) return fail(KD_EINVAL, "kd_dropout_f32: bad arguments");
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const long quads = (long)((n + 3) >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("dropout_f32", 0, 8.0 * (double)n, s);
  if (vec) hipLaunchKernelGGL(dropout_kernel<true>, dim3(drop_grid(quads)), dim3(256), 0, s, x, y, (long)n, key, site, threshold, scale);
  else hipLaunchKernelGGL(dropout_kernel<false>, dim3(drop_grid(quads)), dim3(256), 0, s, x, y, (long)n, key, site, threshold, scale);
  return check_launch("kd_dropout_f32");
}
