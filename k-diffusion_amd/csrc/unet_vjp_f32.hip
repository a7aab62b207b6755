// The reverse (VJP) rules of the image_v1 U-Net's fp32 kernels (unet_f32.hip) w.r.t. their activation input, gfx950: what forward_vjp walks
// back through beside the convolutions' data gradients (kd_conv2d_x3 on the transposed, flipped weight) and ops.attn_global_vjp.  Same layout
// as unet_f32.hip: fp32 NHWC token rows [B H W, C] with an explicit row stride (ld, in floats), so that a gradient can be read from or
// written to one column range of a wider buffer (the two halves of a skip concatenation).
//
//   kd_adagn_vjp_stats_f32  per (sample, group) the two means the group norm's reverse needs, m1 = mean(g_xh) and m2 = mean(g_xh xh), where
//                           xh = (x - mean) rstd, pre = xh (1 + w_b) + b_b, g_pre = g_y (Phi(pre) + pre phi(pre)) behind a GELU (else g_y),
//                           g_xh = g_pre (1 + w_b).  One workgroup per (sample, group) and a binary tree over its 256 partial sums, as
//                           groupnorm_stats_kernel; every term is formed and summed in fp64, so m1 and m2 carry only the rounding of the rstd
//                           they were handed and their own
//   kd_adagn_vjp_apply_f32  g_x = rstd (g_xh - m1 - xh m2) + g_add in one streaming fp32 pass; pre and g_xh in the dual kernel's fp32 lines
//   kd_down2_vjp_f32 / kd_up2_vjp_f32   the transposes of kd_down2_f32 / kd_up2_f32 as gathers: one thread per float4 of g_x sums the up to
//                           3 x 3 (down) or 6 x 6 (up) outputs that read its pixel, the reflected taps folded back onto the interior
// No kernel uses atomics or reads a library option; every sum has a fixed order.
#include <cmath>

#include "kd_common.h"
#include "../../include/kdiff_unet_grad.h"

namespace kd {

namespace {

// The workgroup's sums of two fp64 terms in a fixed order (unet_f32.hip's): a binary tree over the 256 threads' partial sums.
__device__ __forceinline__ void block_sum2(double (*sh)[256], double& a, double& b) {
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  a = sh[0][0];
  b = sh[1][0];
}

// ---- AdaGN (+ GELU) --------------------------------------------------------------------------------------------------------------------------
// gstats[(b G + g) 4 ..] = {m1, m2, 0, 0}.  Thread t takes the float4s t + 256 k of the group's (pixel, 4-channel) grid.
template <bool GELU>
__global__ __launch_bounds__(256) void adagn_vjp_stats_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ stats,
                                                              const float* __restrict__ wb, int wb_stride, const float* __restrict__ gy, int ldgy,
                                                              float* __restrict__ gstats, int hw, int chan, int cpg, int groups) {
  __shared__ double sh[2][256];
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  const float* base = x + (size_t)b * hw * ldx + (size_t)g * cpg;
  const float* gbase = gy + (size_t)b * hw * ldgy + (size_t)g * cpg;
  const float* wrow = wb + (size_t)b * wb_stride + (size_t)g * cpg;
  const float* st = stats + 4 * (size_t)blockIdx.x;
  const double mean = (double)st[0] + (double)st[1], rstd = (double)st[2];
  const int cv = cpg >> 2;
  double s1 = 0.0, s2 = 0.0;
  for (long e = threadIdx.x; e < (long)hw * cv; e += 256) {
    const long pix = e / cv;
    const int ch = (int)(e - pix * cv) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(base + pix * ldx + ch);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gbase + pix * ldgy + ch);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double gain = 1.0 + (double)wrow[ch + u];
      const double xh = ((double)v[u] - mean) * rstd;
      double gp = (double)gv[u];
      if (GELU) {
        const double a = xh * gain + (double)wrow[chan + ch + u];
        gp *= 0.5 * (1.0 + erf(a * 0.70710678118654752440)) + a * (0.39894228040143267794 * exp(-0.5 * a * a));
      }
      const double gxh = gp * gain;
      s1 += gxh;
      s2 += gxh * xh;
    }
  }
  block_sum2(sh, s1, s2);
  if (threadIdx.x == 0) {
    const double n = (double)hw * cpg;
    float* o = gstats + 4 * (size_t)blockIdx.x;
    o[0] = (float)(s1 / n);
    o[1] = (float)(s2 / n);
    o[2] = 0.f;
    o[3] = 0.f;
  }
}

// A thread reads its float4 of x, g_y and g_add before it writes g_x there: g_x == g_y or g_x == g_add (same row stride) is in place.
template <bool GELU>
__global__ __launch_bounds__(256) void adagn_vjp_apply_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ stats,
                                                              const float* __restrict__ gstats, const float* __restrict__ wb, int wb_stride,
                                                              const float* gy, int ldgy, const float* gadd, int ldga, float* gx, int ldgx, int hw,
                                                              int chan, int cpg, long n_vec) {
  const int cv = chan >> 2, groups = chan / cpg;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long pix = i / cv;
    const int c = (int)(i - pix * cv) * 4;
    const int b = (int)(pix / hw);
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + pix * ldx + c);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gy + pix * ldgy + c);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (gadd) o = *reinterpret_cast<const f32x4*>(gadd + pix * ldga + c);
    const float* wrow = wb + (size_t)b * wb_stride;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t sg = 4 * ((size_t)b * groups + (c + u) / cpg);
      const float* st = stats + sg;
      const float* gs = gstats + sg;
      const float t = ((v[u] - st[0]) - st[1]) * st[2];
      const float gain = 1.0f + wrow[c + u];
      float gp = gv[u];
      if (GELU) {
        const float a = fmaf(t, gain, wrow[chan + c + u]);
        const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752440f));
        gp *= cdf + a * (0.39894228040143267794f * expf(-0.5f * a * a));
      }
      o[u] = fmaf(st[2], fmaf(-t, gs[1], gp * gain - gs[0]), o[u]);
    }
    *reinterpret_cast<f32x4*>(gx + pix * ldgx + c) = o;
  }
}

// ---- resampling --------------------------------------------------------------------------------------------------------------------------------
// Along one axis of n inputs, the outputs o (of n / 2) of the stride-2 'linear' filter that read input s, with their weights: output o reads
// the raw indices 2 o - 1 .. 2 o + 2 with {1, 3, 3, 1} / 8, and the raw indices -1 and n reflect onto 1 and n - 2.  Returns the count (<= 3).
__device__ __forceinline__ int down_taps(int s, int n, int (&o)[3], float (&w)[3]) {
  const int no = n >> 1;
  int k = 0;
  if (s & 1) {
    if ((s + 1) / 2 < no) { o[k] = (s + 1) / 2; w[k++] = 0.125f; }       // a = 0 of the next output
    o[k] = (s - 1) / 2; w[k++] = 0.375f;                                // a = 2
    if (s == 1) { o[k] = 0; w[k++] = 0.125f; }                          // raw -1 of output 0
  } else {
    o[k] = s / 2; w[k++] = 0.375f;                                      // a = 1
    if (s >= 2) { o[k] = s / 2 - 1; w[k++] = 0.125f; }                  // a = 3 of the previous output
  }
  if (s == n - 2) { o[k] = no - 1; w[k++] = 0.125f; }                   // raw n of the last output
  return k;
}

// Along one axis of n inputs, the outputs (of 2 n) of the transposed 'linear' filter that read input s: out[2 m] = 3/4 x[m] + 1/4 x[m - 1],
// out[2 m + 1] = 3/4 x[m] + 1/4 x[m + 1] with -1 -> 1 and n -> n - 2.  Returns the count (<= 6).
__device__ __forceinline__ int up_taps(int s, int n, int (&o)[6], float (&w)[6]) {
  int k = 0;
  o[k] = 2 * s; w[k++] = 0.75f;
  o[k] = 2 * s + 1; w[k++] = 0.75f;
  if (s + 1 < n) { o[k] = 2 * s + 2; w[k++] = 0.25f; }                  // the far input of out[2 (s + 1)]
  if (s >= 1) { o[k] = 2 * s - 1; w[k++] = 0.25f; }                     // the far input of out[2 (s - 1) + 1]
  if (s == 1) { o[k] = 0; w[k++] = 0.25f; }                             // out[0] reads -1 -> 1
  if (s == n - 2) { o[k] = 2 * n - 1; w[k++] = 0.25f; }                 // out[2 n - 1] reads n -> n - 2
  return k;
}

// g_x [H, W] from g_y [Ho, Wo]: UP false is down2's transpose (Ho = H / 2), true is up2's (Ho = 2 H)
template <bool UP>
__global__ __launch_bounds__(256) void resample_vjp_kernel(const float* __restrict__ gy, int ldgy, float* __restrict__ gx, int ldgx, int H, int W,
                                                           int chan, int accumulate, long n_vec) {
  constexpr int T = UP ? 6 : 3;
  const int cv = chan >> 2, Ho = UP ? 2 * H : H >> 1, Wo = UP ? 2 * W : W >> 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long pix = i / cv;
    const int c = (int)(i - pix * cv) * 4;
    const int sx = (int)(pix % W);
    const long t = pix / W;
    const int sy = (int)(t % H), b = (int)(t / H);
    int oy[T], ox[T];
    float wy[T], wx[T];
    int ny, nx;
    if constexpr (UP) {
      ny = up_taps(sy, H, oy, wy);
      nx = up_taps(sx, W, ox, wx);
    } else {
      ny = down_taps(sy, H, oy, wy);
      nx = down_taps(sx, W, ox, wx);
    }
    const float* src = gy + (size_t)b * Ho * Wo * ldgy + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < T; ++a) {
      if (a < ny) {
        f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < T; ++j)
          if (j < nx) row += *reinterpret_cast<const f32x4*>(src + ((size_t)oy[a] * Wo + ox[j]) * ldgy) * wx[j];
        acc += row * wy[a];
      }
    }
    float* dst = gx + pix * ldgx + c;
    if (accumulate) acc += *reinterpret_cast<const f32x4*>(dst);
    *reinterpret_cast<f32x4*>(dst) = acc;
  }
}

inline unsigned blocks_for(long n, long per_block) { return (unsigned)std::min<long>((n + per_block - 1) / per_block, 1 << 20); }
inline bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

int adagn_vjp_check(const char* what, int batch, int hw, int chan, int groups) {
  if (batch <= 0 || hw <= 0 || chan <= 0 || groups <= 0) return fail(KD_EINVAL, "%s: bad arguments", what);
  if ((chan % groups) || ((chan / groups) & 3))
    return fail(KD_EINVAL, "%s: %d channels in %d groups: groups of a multiple of 4 channels", what, chan, groups);
  if ((long)batch * groups > 0x7FFFFFFFl) return fail(KD_EINVAL, "%s: too many (sample, group) pairs", what);
  return KD_OK;
}

template <bool UP>
int resample_vjp(const char* what, const char* prof_name, const float* g_y, int ldgy, float* g_x, int ldgx, int batch, int H, int W, int chan,
                 int accumulate, void* stream) {
  if (!g_y || !g_x || batch <= 0 || chan <= 0) return fail(KD_EINVAL, "%s: bad arguments", what);
  if (H < 2 || W < 2) return fail(KD_EINVAL, "%s: the reflect rule needs H, W >= 2 (got %d x %d)", what, H, W);
  if (!UP && ((H | W) & 1)) return fail(KD_EINVAL, "%s: H = %d and W = %d must be even", what, H, W);
  if ((chan & 3) || ldgy < chan || ldgx < chan || (ldgy & 3) || (ldgx & 3) || misaligned(g_y) || misaligned(g_x))
    return fail(KD_EINVAL, "%s: channels a multiple of 4, row strides covering them, rows 16-byte aligned", what);
  const long n_vec = (long)batch * H * W * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof(prof_name, 0, (UP ? 20.0 : 5.0) * batch * H * W * chan, s);
  launch<resample_vjp_kernel<UP>>(dim3(blocks_for(n_vec, 256)), dim3(256), 0, s, g_y, ldgy, g_x, ldgx, H, W, chan, accumulate, n_vec);
  return check_launch(what);
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_adagn_vjp_stats_f32(const float* x, int ldx, const float* stats, const float* wb, int wb_stride, const float* g_y, int ldgy,
                                      float* gstats, int batch, int hw, int chan, int groups, int gelu, void* stream) {
  if (!x || !stats || !wb || !g_y || !gstats) return fail(KD_EINVAL, "kd_adagn_vjp_stats_f32: bad arguments");
  if (int e = adagn_vjp_check("kd_adagn_vjp_stats_f32", batch, hw, chan, groups)) return e;
  if (ldx < chan || ldgy < chan || (ldx & 3) || (ldgy & 3) || wb_stride < 2 * chan || misaligned(x) || misaligned(g_y))
    return fail(KD_EINVAL, "kd_adagn_vjp_stats_f32: row strides must cover the %d channels and keep rows 16-byte aligned; wb rows hold 2 C values", chan);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("adagn_vjp_stats_f32", 0, 8.0 * batch * hw * chan, s);
  const dim3 grid((unsigned)(batch * groups));
  if (gelu) launch<adagn_vjp_stats_kernel<true>>(grid, dim3(256), 0, s, x, ldx, stats, wb, wb_stride, g_y, ldgy, gstats, hw, chan, chan / groups, groups);
  else launch<adagn_vjp_stats_kernel<false>>(grid, dim3(256), 0, s, x, ldx, stats, wb, wb_stride, g_y, ldgy, gstats, hw, chan, chan / groups, groups);
  return check_launch("kd_adagn_vjp_stats_f32");
}

extern "C" int kd_adagn_vjp_apply_f32(const float* x, int ldx, const float* stats, const float* gstats, const float* wb, int wb_stride,
                                      const float* g_y, int ldgy, const float* g_add, int ldga, float* g_x, int ldgx, int batch, int hw, int chan,
                                      int groups, int gelu, void* stream) {
  if (!x || !stats || !gstats || !wb || !g_y || !g_x) return fail(KD_EINVAL, "kd_adagn_vjp_apply_f32: bad arguments");
  if (int e = adagn_vjp_check("kd_adagn_vjp_apply_f32", batch, hw, chan, groups)) return e;
  if (ldx < chan || ldgy < chan || ldgx < chan || (g_add && ldga < chan) || ((ldx | ldgy | ldgx | (g_add ? ldga : 0)) & 3) || wb_stride < 2 * chan ||
      misaligned(x) || misaligned(g_y) || misaligned(g_x) || (g_add && misaligned(g_add)))
    return fail(KD_EINVAL, "kd_adagn_vjp_apply_f32: row strides must cover the channels and keep rows 16-byte aligned; wb rows hold 2 C values");
  if (g_x == x) return fail(KD_EINVAL, "kd_adagn_vjp_apply_f32: g_x may be g_y or g_add, not x");
  if ((g_x == g_y && ldgx != ldgy) || (g_add && g_x == g_add && ldgx != ldga))
    return fail(KD_EINVAL, "kd_adagn_vjp_apply_f32: in place means the same row stride");
  const long n_vec = (long)batch * hw * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("adagn_vjp_apply_f32", 0, (g_add ? 16.0 : 12.0) * batch * hw * chan, s);
  const dim3 grid(blocks_for(n_vec, 256));
  if (gelu) launch<adagn_vjp_apply_kernel<true>>(grid, dim3(256), 0, s, x, ldx, stats, gstats, wb, wb_stride, g_y, ldgy, g_add, ldga, g_x, ldgx, hw, chan, chan / groups, n_vec);
  else launch<adagn_vjp_apply_kernel<false>>(grid, dim3(256), 0, s, x, ldx, stats, gstats, wb, wb_stride, g_y, ldgy, g_add, ldga, g_x, ldgx, hw, chan, chan / groups, n_vec);
  return check_launch("kd_adagn_vjp_apply_f32");
}

extern "C" int kd_down2_vjp_f32(const float* g_y, int ldgy, float* g_x, int ldgx, int batch, int H, int W, int chan, int accumulate, void* stream) {
  return resample_vjp<false>("kd_down2_vjp_f32", "down2_vjp_f32", g_y, ldgy, g_x, ldgx, batch, H, W, chan, accumulate, stream);
}

extern "C" int kd_up2_vjp_f32(const float* g_y, int ldgy, float* g_x, int ldgx, int batch, int H, int W, int chan, int accumulate, void* stream) {
  return resample_vjp<true>("kd_up2_vjp_f32", "up2_vjp_f32", g_y, ldgy, g_x, ldgx, batch, H, W, chan, accumulate, stream);
}
