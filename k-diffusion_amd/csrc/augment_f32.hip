// Karras et al. augmentation on the device (gfx950): the reference's KarrasAugmentationPipeline.__call__ (k_diffusion/augmentation.py:40-89),
// which draws eight parameters per image on a data-loader worker and warps the image with scikit-image on the CPU, as two launches over the
// uploaded batch.
//
//   kd_augment_draw_f32  raw[B, 8] = (a0 .. a7): the reference's ungated x-flip and its five Bernoulli(a_prob)-gated groups (:44-70), from
//                        four Philox blocks per sample (counter contract: include/kdiff_hip.h); not torch's RNG stream
//   kd_augment_warp_f32  y = x warped by the inverse of the matrix the reference composes (:42-74), cond[B, 9] (:75) and, on request, the top
//                        two rows of that inverse.  The interpolation is what scikit-image's warp does for order = 3, mode = 'reflect' (:83):
//                        separable Catmull-Rom over 4 x 4 taps whose out-of-range indices fold with period 2 (N - 1).
//
// One workgroup per (sample, 256 consecutive pixels of the H x W plane): lane i owns pixel 256 tile + i, so the stores of every channel are
// contiguous along W (and across row ends); the 16 taps per channel are gathers that hit the cache (a sample's plane is read once from
// memory).  The sample's matrix is the same in every lane of the workgroup: each lane composes it from raw[b] (about ten libm calls, against
// 16 C loads per pixel).  Both fractions and all eight folded indices are computed once per pixel and serve every channel.
#include <cmath>

#include "kd_common.h"
#include "philox.h"

namespace kd {

namespace {

constexpr unsigned long long AUG_STREAM = 0xC000000000000000ull;     // bits 63 and 62 of the counter's second half: the augmentation blocks
constexpr float TWO_PI_BELOW = 6.28318501f;                          // the fp32 below 2 pi: (u - 1/2) * this stays inside [-pi, pi)

__device__ __forceinline__ bool aug_gate(unsigned w, float a_prob) { return unit24(w) < a_prob; }
__device__ __forceinline__ float aug_angle(unsigned w) { return (unit24(w) - 0.5f) * TWO_PI_BELOW; }
__device__ __forceinline__ float aug_normal(unsigned wr, unsigned wa) { return bm_radius(wr) * __builtin_amdgcn_cosf(unit24(wa)); }

__global__ __launch_bounds__(256) void augment_draw_kernel(float* __restrict__ raw, const long long* __restrict__ key_ptr, int batch, float a_prob) {
  const unsigned long long key = (unsigned long long)key_ptr[0];
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < batch; b += (long)gridDim.x * 256) {
    const Philox4 k0 = philox4x32_10(key, (unsigned long long)b, AUG_STREAM | 0ull);
    const Philox4 k1 = philox4x32_10(key, (unsigned long long)b, AUG_STREAM | 1ull);
    const Philox4 k2 = philox4x32_10(key, (unsigned long long)b, AUG_STREAM | 2ull);
    const Philox4 k3 = philox4x32_10(key, (unsigned long long)b, AUG_STREAM | 3ull);
    float* o = raw + 8 * b;
    o[0] = (float)(k0.x0 >> 31);                                                          // x-flip: ungated
    o[1] = aug_gate(k0.x1, a_prob) ? (float)(k0.x2 >> 31) : 0.0f;                        // y-flip
    o[2] = aug_gate(k0.x3, a_prob) ? aug_normal(k1.x0, k1.x1) : 0.0f;                    // log-scale
    o[3] = aug_gate(k1.x2, a_prob) ? aug_angle(k1.x3) : 0.0f;                            // rotation
    const bool aniso = aug_gate(k2.x0, a_prob);
    o[4] = aniso ? aug_angle(k2.x1) : 0.0f;                                              // anisotropy: direction ...
    o[5] = aniso ? aug_normal(k2.x2, k2.x3) : 0.0f;                                      // ... and log-ratio
    const bool trans = aug_gate(k3.x0, a_prob);
    const float r = bm_radius(k3.x2), rev = unit24(k3.x3);
    o[6] = trans ? r * __builtin_amdgcn_cosf(rev) : 0.0f;                                // translation: one Box-Muller pair
    o[7] = trans ? r * __builtin_amdgcn_cosf(rev - 0.25f) : 0.0f;                        // sin(a) = cos(a - 1/4 turn)
  }
}

// index i of an axis of n = m + 1 samples under numpy-pad 'reflect' (d c b | a b c d | c b a): period 2 m, any distance
__device__ __forceinline__ int reflect_index(int i, int m) {
  const int period = 2 * m;
  int j = i % period;
  if (j < 0) j += period;
  return j > m ? period - j : j;
}

// scikit-image's cubic_interpolation: Catmull-Rom (Keys a = -1/2) through p0 .. p3 at fraction t of [p1, p2]
__device__ __forceinline__ float catmull_rom(float t, float p0, float p1, float p2, float p3) {
  return p1 + 0.5f * t * (p2 - p0 + t * (2.0f * p0 - 5.0f * p1 + 4.0f * p2 - p3 + t * (3.0f * (p1 - p2) + p3 - p0)));
}

// a source coordinate as (first tap, fraction); the clamp keeps the tap an int for any raw (NaN and Inf included: they sample somewhere inside)
__device__ __forceinline__ int tap_of(float s, float* frac) {
  s = fminf(fmaxf(s, -1.0e9f), 1.0e9f);
  const float f = floorf(s);
  *frac = s - f;
  return (int)f - 1;
}

__global__ __launch_bounds__(256) void augment_warp_kernel(const float* __restrict__ x, const float* __restrict__ raw, float log2_scale,
                                                           float log2_aniso, float a_trans, float* __restrict__ y, float* __restrict__ cond,
                                                           float* __restrict__ mat, int chan, int H, int W, unsigned tiles) {
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const float* a = raw + 8 * (size_t)b;
  const float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
  // M^-1 = T(c) T(-d) R(a4) S(n^-a5, n^a5) R(-a4) R(a3) S(s^-a2) S(1, 1 - 2 a1) S(1 - 2 a0, 1) T(-c): the inverse factors in reverse order
  float s3, c3, s4, c4;
  sincosf(a3, &s3, &c3);
  sincosf(a4, &s4, &c4);
  const float inv_scale = exp2f(-a2 * log2_scale);
  const float d0 = exp2f(-a5 * log2_aniso), d1 = exp2f(a5 * log2_aniso);
  const float q00 = c4 * d0 * c4 + s4 * d1 * s4, q01 = c4 * s4 * (d0 - d1), q11 = s4 * d0 * s4 + c4 * d1 * c4;     // R(a4) S R(-a4), symmetric
  const float fx = (1.0f - 2.0f * a0) * inv_scale, fy = (1.0f - 2.0f * a1) * inv_scale;
  const float l00 = (q00 * c3 + q01 * s3) * fx, l01 = (q01 * c3 - q00 * s3) * fy;
  const float l10 = (q01 * c3 + q11 * s3) * fx, l11 = (q11 * c3 - q01 * s3) * fy;
  const float cx = 0.5f * (float)W - 0.5f, cy = 0.5f * (float)H - 0.5f;
  const float ox = cx - a_trans * (float)H * a6, oy = cy - a_trans * (float)W * a7;
  if (tile == 0 && threadIdx.x == 0) {
    float* c = cond + 9 * (size_t)b;
    c[0] = a0; c[1] = a1; c[2] = a2; c[3] = c3 - 1.0f; c[4] = s3; c[5] = a5 * c4; c[6] = a5 * s4; c[7] = a6; c[8] = a7;
    if (mat) {
      float* m = mat + 6 * (size_t)b;
      m[0] = l00; m[1] = l01; m[2] = ox - (l00 * cx + l01 * cy);
      m[3] = l10; m[4] = l11; m[5] = oy - (l10 * cx + l11 * cy);
    }
  }
  const int hw = H * W;
  const int p = (int)(tile * 256u + threadIdx.x);
  if (p >= hw) return;
  const int row = p / W, col = p - row * W;
  // the same map about the image centre: L (p - c) + (c - d)
  const float u = (float)col - cx, v = (float)row - cy;
  float tx, ty;
  const int ix = tap_of(l00 * u + l01 * v + ox, &tx), iy = tap_of(l10 * u + l11 * v + oy, &ty);
  int xo[4], yo[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    xo[k] = reflect_index(ix + k, W - 1);
    yo[k] = reflect_index(iy + k, H - 1) * W;
  }
  const size_t plane0 = (size_t)b * chan;
  for (int ch = 0; ch < chan; ++ch) {
    const float* src = x + (plane0 + ch) * (size_t)hw;
    float rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rows[k] = catmull_rom(tx, src[yo[k] + xo[0]], src[yo[k] + xo[1]], src[yo[k] + xo[2]], src[yo[k] + xo[3]]);
    y[(plane0 + ch) * (size_t)hw + p] = catmull_rom(ty, rows[0], rows[1], rows[2], rows[3]);
  }
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_augment_draw_f32(const long long* key, int batch, float a_prob, float* raw, void* stream) {
  if (!key || !raw || batch <= 0) return fail(KD_EINVAL, "kd_augment_draw_f32: bad arguments");
  if (!(a_prob >= 0.0f && a_prob <= 1.0f)) return fail(KD_EINVAL, "kd_augment_draw_f32: a_prob %g outside [0, 1]", (double)a_prob);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("augment_draw_f32", 0, 32.0 * batch, s);
  const unsigned blocks = (unsigned)std::min<long>(((long)batch + 255) / 256, 16384);
  hipLaunchKernelGGL(augment_draw_kernel, dim3(blocks), dim3(256), 0, s, raw, key, batch, a_prob);
  return check_launch("kd_augment_draw_f32");
}

extern "C" int kd_augment_warp_f32(const float* x, const float* raw, float a_scale, float a_aniso, float a_trans, float* y, float* cond, float* mat,
                                   int batch, int chan, int H, int W, void* stream) {
  if (!x || !raw || !y || !cond || batch <= 0 || chan <= 0) return fail(KD_EINVAL, "kd_augment_warp_f32: bad arguments");
  if (H < 2 || W < 2) return fail(KD_EINVAL, "kd_augment_warp_f32: the reflect rule needs H, W >= 2 (got %d x %d)", H, W);
  if (!(a_scale > 0.0f) || !(a_aniso > 0.0f) || !std::isfinite(a_scale) || !std::isfinite(a_aniso) || !std::isfinite(a_trans))
    return fail(KD_EINVAL, "kd_augment_warp_f32: a_scale and a_aniso must be positive and finite, a_trans finite");
  const long long hw = (long long)H * W;
  if (hw > 0x7FFFFFFFll - 256) return fail(KD_EINVAL, "kd_augment_warp_f32: H * W = %lld does not fit the 32-bit pixel index", hw);
  const long long tiles = (hw + 255) / 256;
  if (tiles * batch > 0x7FFFFFFFll) return fail(KD_EINVAL, "kd_augment_warp_f32: %lld workgroups exceed the grid", tiles * batch);
  const uintptr_t xb = reinterpret_cast<uintptr_t>(x), yb = reinterpret_cast<uintptr_t>(y);
  const uintptr_t bytes = (uintptr_t)batch * chan * hw * sizeof(float);
  if (xb < yb + bytes && yb < xb + bytes) return fail(KD_EINVAL, "kd_augment_warp_f32: y must not overlap x (every output pixel gathers 16 inputs)");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("augment_warp_f32", 0, 2.0 * (double)bytes + 4.0 * batch * (8 + 9 + (mat ? 6 : 0)), s);
  hipLaunchKernelGGL(augment_warp_kernel, dim3((unsigned)(tiles * batch)), dim3(256), 0, s, x, raw, (float)std::log2((double)a_scale),
                     (float)std::log2((double)a_aniso), a_trans, y, cond, mat, chan, H, W, (unsigned)tiles);
  return check_launch("kd_augment_warp_f32");
}
