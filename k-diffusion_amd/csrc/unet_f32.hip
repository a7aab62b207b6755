// The fp32 kernels of the image_v1 U-Net beside its convolutions (conv_x3.hip), gfx950.  Activations are fp32 NHWC, token-major
// [B H W, C] with an explicit row stride (ld, in floats), so that a kernel can read or write one column range of a wider buffer.
//
//   kd_groupnorm_stats_f32  F.group_norm's statistics (layers.py:174): per (sample, group) the mean and 1 / sqrt(biased variance + eps) over
//                           (C / G channels x H W), accumulated in fp64 in a fixed order (a large mean does not cancel the variance)
//   kd_adagn_apply_f32      AdaGN (layers.py:172-175): y = (x - mean) rstd (1 + w_b) + b_b, then optionally the exact (erf) GELU that follows it
//                           in ResConvBlock (image_v1.py:20,24)
//   kd_groupnorm_stats_jvp_f32 / kd_adagn_apply_jvp_f32   the same two with their tangents along x_dot (the dual pass of log_likelihood): the
//                           statistics' tangents {mean_dot, rstd_dot} from a second fp64 pass, then y and y_dot in one streaming pass
//   kd_down2_f32 / kd_up2_f32   Downsample2d / Upsample2d (layers.py:251-280) for the 'linear' kernel [1, 3, 3, 1] / 8 and 'reflect' padding:
//                           depthwise and separable, so the stride-2 conv is 4 x 4 taps of k (x) k and the transposed conv is, per axis,
//                           out[2m] = 3/4 x[m] + 1/4 x[m-1], out[2m+1] = 3/4 x[m] + 1/4 x[m+1] with indices -1 -> 1 and n -> n - 2
//   kd_unet_in_f32          proj_in (image_v1.py:101,148): NCHW image -> tokens, K = 1 .. 4 input channels as plain FMAs, x c_in folded in
//   kd_unet_out_f32         proj_out (:102,150): tokens -> NCHW, N = 1 .. 4 image channels, F c_out + x c_skip folded in (layers.py:88-90)
//   kd_cond_mlp_f32         act(x W^T + b + add) for a few rows in exact fp32 (MappingNet :80-86, mapping_cond :99, and all AdaGN mappers of
//                           a model concatenated into one weight: one launch per forward)
// No kernel uses atomics; every reduction has a fixed order.
#include <cmath>

#include "kd_common.h"

namespace kd {

namespace {

// ---- group norm -----------------------------------------------------------------------------------------------------------------------------
// one workgroup per (sample, group); stats[(b G + g) 4 ..] = {mean_hi, mean_lo, rstd, 0}: the fp64 mean as two fp32 (x - hi - lo loses nothing
// to the mean's rounding when the mean is large against the spread)
// The workgroup's sums of two fp64 terms in a fixed order: a binary tree over the 256 threads' partial sums; every thread gets both totals.
__device__ __forceinline__ void block_sum2(double (*sh)[256], double& a, double& b) {
  __syncthreads();                                             // an earlier reduction's totals have been read
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

// mean and 1 / sqrt(biased variance + eps) of one (sample, group), both in fp64: the one reduction of the forward statistics and of the
// dual pass's, so the two write the same bits
__device__ __forceinline__ void group_moments(const float* __restrict__ base, int ldx, long n, int cpg, float eps, double (*sh)[256], double& mean,
                                              double& rstd) {
  double s = 0.0, ss = 0.0;
  for (long e = threadIdx.x; e < n; e += 256) {
    const long pix = e / cpg;
    const int ch = (int)(e - pix * cpg);
    const double v = (double)base[pix * ldx + ch];
    s += v;
    ss += v * v;
  }
  block_sum2(sh, s, ss);
  mean = s / (double)n;
  rstd = 1.0 / sqrt(fmax(ss / (double)n - mean * mean, 0.0) + (double)eps);
}

__device__ __forceinline__ void write_stats(float* __restrict__ o, double mean, double rstd) {
  const float mh = (float)mean;
  o[0] = mh;
  o[1] = (float)(mean - (double)mh);
  o[2] = (float)rstd;
  o[3] = 0.f;
}

__global__ __launch_bounds__(256) void groupnorm_stats_kernel(const float* __restrict__ x, int ldx, float* __restrict__ stats, int hw, int cpg,
                                                              int groups, float eps) {
  __shared__ double sh[2][256];
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  double mean, rstd;
  group_moments(x + (size_t)b * hw * ldx + (size_t)g * cpg, ldx, (long)hw * cpg, cpg, eps, sh, mean, rstd);
  if (threadIdx.x == 0) write_stats(stats + 4 * (size_t)blockIdx.x, mean, rstd);
}

// The statistics and their tangents along x_dot: jstats[(b G + g) 4 ..] = {mean_dot, rstd_dot, 0, 0} with mean_dot = sum x_dot / n and
// rstd_dot = -rstd^3 sum (x - mean) x_dot / n.  The second pass centres x with the fp64 mean (a large mean does not cancel the covariance) and
// reads 16 bytes per lane: thread t takes the float4s t + 256 k of the group's (pixel, 4-channel) grid.
__global__ __launch_bounds__(256) void groupnorm_stats_jvp_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ xd, int ldxd,
                                                                  float* __restrict__ stats, float* __restrict__ jstats, int hw, int cpg, int groups,
                                                                  float eps) {
  __shared__ double sh[2][256];
  const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
  const float* base = x + (size_t)b * hw * ldx + (size_t)g * cpg;
  const float* based = xd + (size_t)b * hw * ldxd + (size_t)g * cpg;
  const long n = (long)hw * cpg;
  double mean, rstd;
  group_moments(base, ldx, n, cpg, eps, sh, mean, rstd);
  const int cv = cpg >> 2;
  double sd = 0.0, cov = 0.0;
  for (long e = threadIdx.x; e < (long)hw * cv; e += 256) {
    const long pix = e / cv;
    const int ch = (int)(e - pix * cv) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(base + pix * ldx + ch);
    const f32x4 d = *reinterpret_cast<const f32x4*>(based + pix * ldxd + ch);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      sd += (double)d[u];
      cov += ((double)v[u] - mean) * (double)d[u];
    }
  }
  block_sum2(sh, sd, cov);
  if (threadIdx.x == 0) {
    write_stats(stats + 4 * (size_t)blockIdx.x, mean, rstd);
    float* o = jstats + 4 * (size_t)blockIdx.x;
    o[0] = (float)(sd / (double)n);
    o[1] = (float)(-(rstd * rstd * rstd) * (cov / (double)n));
    o[2] = 0.f;
    o[3] = 0.f;
  }
}

template <bool GELU>
__global__ __launch_bounds__(256) void adagn_apply_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ stats,
                                                          const float* __restrict__ wb, int wb_stride, float* __restrict__ y, int ldy, int hw,
                                                          int chan, int cpg, long n_vec) {
  const int cv = chan >> 2, groups = chan / cpg;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long pix = i / cv;
    const int c = (int)(i - pix * cv) * 4;
    const int b = (int)(pix / hw);
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + pix * ldx + c);
    const float* wrow = wb + (size_t)b * wb_stride;
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* st = stats + 4 * ((size_t)b * groups + (c + u) / cpg);
      const float t = ((v[u] - st[0]) - st[1]) * st[2];
      const float a = fmaf(t, 1.0f + wrow[c + u], wrow[chan + c + u]);
      o[u] = GELU ? gelu_erf(a) : a;
    }
    *reinterpret_cast<f32x4*>(y + pix * ldy + c) = o;
  }
}

// AdaGN (+ GELU) and its tangent along x_dot, the conditioning (w, b) held fixed.  The primal lines are adagn_apply_kernel's, so y has its
// bits.  A thread reads its float4 of x and of x_dot before it writes y and y_dot there: y == x with y_dot == x_dot is in place.
template <bool GELU>
__global__ __launch_bounds__(256) void adagn_apply_jvp_kernel(const float* x, int ldx, const float* xd, int ldxd, const float* __restrict__ stats,
                                                              const float* __restrict__ jstats, const float* __restrict__ wb, int wb_stride, float* y,
                                                              int ldy, float* yd, int ldyd, int hw, int chan, int cpg, long n_vec) {
  const int cv = chan >> 2, groups = chan / cpg;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long pix = i / cv;
    const int c = (int)(i - pix * cv) * 4;
    const int b = (int)(pix / hw);
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + pix * ldx + c);
    const f32x4 d = *reinterpret_cast<const f32x4*>(xd + pix * ldxd + c);
    const float* wrow = wb + (size_t)b * wb_stride;
    f32x4 o, od;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t sg = 4 * ((size_t)b * groups + (c + u) / cpg);
      const float* st = stats + sg;
      const float* js = jstats + sg;
      const float xc = (v[u] - st[0]) - st[1];
      const float t = xc * st[2];
      const float gain = 1.0f + wrow[c + u];
      const float a = fmaf(t, gain, wrow[chan + c + u]);
      const float ad = fmaf(d[u] - js[0], st[2], xc * js[1]) * gain;
      if (GELU) {
        const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752440f));
        o[u] = gelu_erf(a);
        od[u] = ad * (cdf + a * (0.39894228040143267794f * expf(-0.5f * a * a)));
      } else {
        o[u] = a;
        od[u] = ad;
      }
    }
    *reinterpret_cast<f32x4*>(y + pix * ldy + c) = o;
    *reinterpret_cast<f32x4*>(yd + pix * ldyd + c) = od;
  }
}

// ---- resampling ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }      // one step past either end

__global__ __launch_bounds__(256) void down2_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int H, int W, int chan,
                                                    long n_vec) {
  const int cv = chan >> 2, Ho = H >> 1, Wo = W >> 1;
  const float k[4] = {0.125f, 0.375f, 0.375f, 0.125f};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long opix = i / cv;
    const int c = (int)(i - opix * cv) * 4;
    const int ox = (int)(opix % Wo);
    const long t = opix / Wo;
    const int oy = (int)(t % Ho), b = (int)(t / Ho);
    const float* src = x + (size_t)b * H * W * ldx + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int sy = reflect1(2 * oy + a - 1, H);
      f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sx = reflect1(2 * ox + j - 1, W);
        row += *reinterpret_cast<const f32x4*>(src + ((size_t)sy * W + sx) * ldx) * k[j];
      }
      acc += row * k[a];
    }
    *reinterpret_cast<f32x4*>(y + opix * ldy + c) = acc;
  }
}

__global__ __launch_bounds__(256) void up2_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int H, int W, int chan,
                                                  long n_vec) {
  const int cv = chan >> 2, Ho = 2 * H, Wo = 2 * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long opix = i / cv;
    const int c = (int)(i - opix * cv) * 4;
    const int ox = (int)(opix % Wo);
    const long t = opix / Wo;
    const int oy = (int)(t % Ho), b = (int)(t / Ho);
    const int my = oy >> 1, mx = ox >> 1;
    const int ny = reflect1((oy & 1) ? my + 1 : my - 1, H), nx = reflect1((ox & 1) ? mx + 1 : mx - 1, W);
    const float* src = x + (size_t)b * H * W * ldx + c;
    const f32x4 v00 = *reinterpret_cast<const f32x4*>(src + ((size_t)my * W + mx) * ldx);
    const f32x4 v01 = *reinterpret_cast<const f32x4*>(src + ((size_t)my * W + nx) * ldx);
    const f32x4 v10 = *reinterpret_cast<const f32x4*>(src + ((size_t)ny * W + mx) * ldx);
    const f32x4 v11 = *reinterpret_cast<const f32x4*>(src + ((size_t)ny * W + nx) * ldx);
    const f32x4 near = v00 * 0.75f + v01 * 0.25f, far = v10 * 0.75f + v11 * 0.25f;
    *reinterpret_cast<f32x4*>(y + opix * ldy + c) = near * 0.75f + far * 0.25f;
  }
}

// ---- proj_in / proj_out --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void unet_in_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ sigma, float sigma_data, float* __restrict__ y, int ldy, int hw,
                                                      int c_img, int chan, long n_vec) {
  const int cv = chan >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
    const long pix = i / cv;
    const int c = (int)(i - pix * cv) * 4;
    const int b = (int)(pix / hw);
    const long p = pix - (long)b * hw;
    float c_in = 1.0f;
    if (sigma) c_in = 1.0f / sqrtf(sigma[b] * sigma[b] + sigma_data * sigma_data);
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = bias ? bias[c + u] : 0.f;
    for (int k = 0; k < c_img; ++k) {
      const float v = img[((size_t)b * c_img + k) * hw + p] * c_in;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = fmaf(v, w[(c + u) * c_img + k], o[u]);
    }
    *reinterpret_cast<f32x4*>(y + pix * ldy + c) = o;
  }
}

// 32 lanes per pixel: lane j sums channels 4 j + 128 t, a fixed butterfly over the 32 lanes finishes the up to four outputs
__global__ __launch_bounds__(256) void unet_out_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ img, const float* __restrict__ sigma, float sigma_data,
                                                       float* __restrict__ out, int hw, int c_img, int chan, long n_pix) {
  const int j = threadIdx.x & 31;
  for (long pix = (long)blockIdx.x * 8 + (threadIdx.x >> 5); pix < n_pix; pix += (long)gridDim.x * 8) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 4 * j; c < chan; c += 128) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + pix * ldx + c);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (o < c_img) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (size_t)o * chan + c);
          acc[o] = fmaf(v[3], wv[3], fmaf(v[2], wv[2], fmaf(v[1], wv[1], fmaf(v[0], wv[0], acc[o]))));
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[o] = wave_sum_xor(acc[o], 32);
    if (j < c_img) {
      const int b = (int)(pix / hw);
      const long p = pix - (long)b * hw;
      float f = (j == 0 ? acc[0] : j == 1 ? acc[1] : j == 2 ? acc[2] : acc[3]) + (bias ? bias[j] : 0.f);
      const size_t at = ((size_t)b * c_img + j) * hw + p;
      if (sigma) {
        const float sg = sigma[b], var = sg * sg + sigma_data * sigma_data;
        f = fmaf(f, sg * sigma_data / sqrtf(var), img[at] * (sigma_data * sigma_data / var));
      }
      out[at] = f;
    }
  }
}

// ---- few-rows MLP layer -----------------------------------------------------------------------------------------------------------------------
// one wave per output feature n: lane l sums k = l + 64 t in order, a fixed butterfly finishes the dot product
template <bool GELU>
__global__ __launch_bounds__(256) void cond_mlp_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ add, float* __restrict__ y, int rows, int n_out, int k_in) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= n_out) return;
  const float* wr = w + (size_t)n * k_in;
  const float bv = bias ? bias[n] : 0.f;
  for (int r = 0; r < rows; ++r) {
    const float* xr = x + (size_t)r * k_in;
    float s = 0.f;
    for (int k = lane; k < k_in; k += 64) s = fmaf(xr[k], wr[k], s);
    s = wave_sum_xor(s, 64) + bv;
    if (add) s += add[(size_t)r * n_out + n];
    if (lane == 0) y[(size_t)r * n_out + n] = GELU ? gelu_erf(s) : s;
  }
}

inline unsigned blocks_for(long n, long per_block) { return (unsigned)std::min<long>((n + per_block - 1) / per_block, 1 << 20); }
inline bool misaligned(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_groupnorm_stats_f32(const float* x, int ldx, float* stats, int batch, int hw, int chan, int groups, float eps, void* stream) {
  if (!x || !stats || batch <= 0 || hw <= 0 || chan <= 0 || groups <= 0) return fail(KD_EINVAL, "kd_groupnorm_stats_f32: bad arguments");
  if (chan % groups) return fail(KD_EINVAL, "kd_groupnorm_stats_f32: %d channels do not divide into %d groups", chan, groups);
  if (ldx < chan) return fail(KD_EINVAL, "kd_groupnorm_stats_f32: row stride %d shorter than the %d channels", ldx, chan);
  if ((long)batch * groups > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_groupnorm_stats_f32: too many (sample, group) pairs");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("groupnorm_stats_f32", 0, 4.0 * batch * hw * chan, s);
  launch<groupnorm_stats_kernel>(dim3((unsigned)(batch * groups)), dim3(256), 0, s, x, ldx, stats, hw, chan / groups, groups, eps);
  return check_launch("kd_groupnorm_stats_f32");
}

extern "C" int kd_adagn_apply_f32(const float* x, int ldx, const float* stats, const float* wb, int wb_stride, float* y, int ldy, int batch, int hw,
                                  int chan, int groups, int gelu, void* stream) {
  if (!x || !stats || !wb || !y || batch <= 0 || hw <= 0 || chan <= 0 || groups <= 0) return fail(KD_EINVAL, "kd_adagn_apply_f32: bad arguments");
  if ((chan % groups) || (chan & 3)) return fail(KD_EINVAL, "kd_adagn_apply_f32: %d channels: a multiple of 4 and of the %d groups", chan, groups);
  if (ldx < chan || ldy < chan || (ldx & 3) || (ldy & 3) || wb_stride < 2 * chan || misaligned(x) || misaligned(y))
    return fail(KD_EINVAL, "kd_adagn_apply_f32: row strides must cover the channels and keep rows 16-byte aligned; wb rows hold 2 C values");
  const long n_vec = (long)batch * hw * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("adagn_apply_f32", 0, 8.0 * batch * hw * chan, s);
  if (gelu) launch<adagn_apply_kernel<true>>(dim3(blocks_for(n_vec, 256)), dim3(256), 0, s, x, ldx, stats, wb, wb_stride, y, ldy, hw, chan, chan / groups, n_vec);
  else launch<adagn_apply_kernel<false>>(dim3(blocks_for(n_vec, 256)), dim3(256), 0, s, x, ldx, stats, wb, wb_stride, y, ldy, hw, chan, chan / groups, n_vec);
  return check_launch("kd_adagn_apply_f32");
}

extern "C" int kd_groupnorm_stats_jvp_f32(const float* x, int ldx, const float* x_dot, int ldxd, float* stats, float* jstats, int batch, int hw,
                                          int chan, int groups, float eps, void* stream) {
  if (!x || !x_dot || !stats || !jstats || batch <= 0 || hw <= 0 || chan <= 0 || groups <= 0)
    return fail(KD_EINVAL, "kd_groupnorm_stats_jvp_f32: bad arguments");
  if ((chan % groups) || ((chan / groups) & 3))
    return fail(KD_EINVAL, "kd_groupnorm_stats_jvp_f32: %d channels in %d groups: groups of a multiple of 4 channels", chan, groups);
  if (ldx < chan || ldxd < chan || (ldx & 3) || (ldxd & 3) || misaligned(x) || misaligned(x_dot))
    return fail(KD_EINVAL, "kd_groupnorm_stats_jvp_f32: row strides must cover the %d channels and keep rows 16-byte aligned", chan);
  if ((long)batch * groups > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_groupnorm_stats_jvp_f32: too many (sample, group) pairs");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("groupnorm_stats_jvp_f32", 0, 12.0 * batch * hw * chan, s);
  launch<groupnorm_stats_jvp_kernel>(dim3((unsigned)(batch * groups)), dim3(256), 0, s, x, ldx, x_dot, ldxd, stats, jstats, hw, chan / groups, groups,
                                     eps);
  return check_launch("kd_groupnorm_stats_jvp_f32");
}

extern "C" int kd_adagn_apply_jvp_f32(const float* x, int ldx, const float* x_dot, int ldxd, const float* stats, const float* jstats, const float* wb,
                                      int wb_stride, float* y, int ldy, float* y_dot, int ldyd, int batch, int hw, int chan, int groups, int gelu,
                                      void* stream) {
  if (!x || !x_dot || !stats || !jstats || !wb || !y || !y_dot || batch <= 0 || hw <= 0 || chan <= 0 || groups <= 0)
    return fail(KD_EINVAL, "kd_adagn_apply_jvp_f32: bad arguments");
  if ((chan % groups) || (chan & 3)) return fail(KD_EINVAL, "kd_adagn_apply_jvp_f32: %d channels: a multiple of 4 and of the %d groups", chan, groups);
  if (ldx < chan || ldxd < chan || ldy < chan || ldyd < chan || ((ldx | ldxd | ldy | ldyd) & 3) || wb_stride < 2 * chan || misaligned(x) ||
      misaligned(x_dot) || misaligned(y) || misaligned(y_dot))
    return fail(KD_EINVAL, "kd_adagn_apply_jvp_f32: row strides must cover the channels and keep rows 16-byte aligned; wb rows hold 2 C values");
  if (y == x_dot || y_dot == x || y == y_dot) return fail(KD_EINVAL, "kd_adagn_apply_jvp_f32: in place means y == x and y_dot == x_dot, not crossed");
  const long n_vec = (long)batch * hw * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("adagn_apply_jvp_f32", 0, 16.0 * batch * hw * chan, s);
  const dim3 grid(blocks_for(n_vec, 256));
  if (gelu) launch<adagn_apply_jvp_kernel<true>>(grid, dim3(256), 0, s, x, ldx, x_dot, ldxd, stats, jstats, wb, wb_stride, y, ldy, y_dot, ldyd, hw, chan, chan / groups, n_vec);
  else launch<adagn_apply_jvp_kernel<false>>(grid, dim3(256), 0, s, x, ldx, x_dot, ldxd, stats, jstats, wb, wb_stride, y, ldy, y_dot, ldyd, hw, chan, chan / groups, n_vec);
  return check_launch("kd_adagn_apply_jvp_f32");
}

static int resample_check(const char* what, const float* x, int ldx, float* y, int ldy, int batch, int H, int W, int chan, bool down) {
  if (!x || !y || batch <= 0 || chan <= 0) return fail(KD_EINVAL, "%s: bad arguments", what);
  if (H < 2 || W < 2) return fail(KD_EINVAL, "%s: the reflect rule needs H, W >= 2 (got %d x %d)", what, H, W);
  if (down && ((H | W) & 1)) return fail(KD_EINVAL, "%s: H = %d and W = %d must be even", what, H, W);
  if ((chan & 3) || ldx < chan || ldy < chan || (ldx & 3) || (ldy & 3) || misaligned(x) || misaligned(y))
    return fail(KD_EINVAL, "%s: channels a multiple of 4, row strides covering them, rows 16-byte aligned", what);
  return KD_OK;
}

extern "C" int kd_down2_f32(const float* x, int ldx, float* y, int ldy, int batch, int H, int W, int chan, void* stream) {
  if (int e = resample_check("kd_down2_f32", x, ldx, y, ldy, batch, H, W, chan, true)) return e;
  const long n_vec = (long)batch * (H / 2) * (W / 2) * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("down2_f32", 0, 5.0 * batch * H * W * chan, s);
  launch<down2_kernel>(dim3(blocks_for(n_vec, 256)), dim3(256), 0, s, x, ldx, y, ldy, H, W, chan, n_vec);
  return check_launch("kd_down2_f32");
}

extern "C" int kd_up2_f32(const float* x, int ldx, float* y, int ldy, int batch, int H, int W, int chan, void* stream) {
  if (int e = resample_check("kd_up2_f32", x, ldx, y, ldy, batch, H, W, chan, false)) return e;
  const long n_vec = (long)batch * (2 * H) * (2 * W) * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("up2_f32", 0, 20.0 * batch * H * W * chan, s);
  launch<up2_kernel>(dim3(blocks_for(n_vec, 256)), dim3(256), 0, s, x, ldx, y, ldy, H, W, chan, n_vec);
  return check_launch("kd_up2_f32");
}

extern "C" int kd_unet_in_f32(const float* img, const float* w, const float* bias, const float* sigma, float sigma_data, float* y, int ldy, int batch,
                              int hw, int c_img, int chan, void* stream) {
  if (!img || !w || !y || batch <= 0 || hw <= 0 || c_img <= 0 || chan <= 0) return fail(KD_EINVAL, "kd_unet_in_f32: bad arguments");
  if ((chan & 3) || ldy < chan || (ldy & 3) || misaligned(y)) return fail(KD_EINVAL, "kd_unet_in_f32: channels a multiple of 4, ldy covering them, rows 16-byte aligned");
  const long n_vec = (long)batch * hw * (chan >> 2);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("unet_in_f32", 2.0 * batch * hw * c_img * chan, 4.0 * batch * hw * (c_img + chan), s);
  launch<unet_in_kernel>(dim3(blocks_for(n_vec, 256)), dim3(256), 0, s, img, w, bias, sigma, sigma_data, y, ldy, hw, c_img, chan, n_vec);
  return check_launch("kd_unet_in_f32");
}

extern "C" int kd_unet_out_f32(const float* x, int ldx, const float* w, const float* bias, const float* img, const float* sigma, float sigma_data,
                               float* out, int batch, int hw, int c_img, int chan, void* stream) {
  if (!x || !w || !out || batch <= 0 || hw <= 0 || chan <= 0) return fail(KD_EINVAL, "kd_unet_out_f32: bad arguments");
  if (c_img < 1 || c_img > 4) return fail(KD_EINVAL, "kd_unet_out_f32: %d image channels (1 .. 4)", c_img);
  if (sigma && !img) return fail(KD_EINVAL, "kd_unet_out_f32: the preconditioned form needs the input image for the skip term");
  if ((chan & 3) || ldx < chan || (ldx & 3) || misaligned(x) || misaligned(w)) return fail(KD_EINVAL, "kd_unet_out_f32: channels a multiple of 4, ldx covering them, rows 16-byte aligned");
  const long n_pix = (long)batch * hw;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("unet_out_f32", 2.0 * n_pix * c_img * chan, 4.0 * n_pix * (c_img + chan), s);
  launch<unet_out_kernel>(dim3(blocks_for(n_pix, 8)), dim3(256), 0, s, x, ldx, w, bias, img, sigma, sigma_data, out, hw, c_img, chan, n_pix);
  return check_launch("kd_unet_out_f32");
}

extern "C" int kd_cond_mlp_f32(const float* x, const float* w, const float* bias, const float* add, float* y, int rows, int n_out, int k_in, int gelu,
                               void* stream) {
  if (!x || !w || !y || rows <= 0 || n_out <= 0 || k_in <= 0) return fail(KD_EINVAL, "kd_cond_mlp_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("cond_mlp_f32", 2.0 * rows * n_out * k_in, 4.0 * ((double)n_out * k_in + (double)rows * (k_in + n_out)), s);
  const dim3 grid((unsigned)((n_out + 3) / 4));
  if (gelu) launch<cond_mlp_kernel<true>>(grid, dim3(256), 0, s, x, w, bias, add, y, rows, n_out, k_in);
  else launch<cond_mlp_kernel<false>>(grid, dim3(256), 0, s, x, w, bias, add, y, rows, n_out, k_in);
  return check_launch("kd_cond_mlp_f32");
}
