// The small parameter-gradient rules of the image_v1 U-Net (gfx950), beside the convolution's weight gradient (conv_wgrad_x3.hip): everything
// here is tiny or memory-bound, and every sum is formed in fp64 in a fixed order.  Same layout as unet_f32.hip / unet_vjp_f32.hip: fp32 NHWC
// token rows [B H W, C] with an explicit row stride (ld, in floats).
//
//   kd_adagn_wb_grad_f32  the gradient of the per-sample (weight, bias) pair AdaGN reads from the conditioning table: per (sample, channel)
//                         d w = sum over pixels of g_pre xh and d b = sum over pixels of g_pre, with xh = (x - mean) rstd, pre = xh (1 + w) + b
//                         and g_pre = g_y (Phi(pre) + pre phi(pre)) behind a GELU (else g_y): kd_adagn_vjp_stats_f32's terms.  One workgroup per
//                         (sample, 32 channels): 8 threads per channel take every 8th pixel, and thread 0 of the channel adds the 8 partial sums
//                         in ascending order.
//   kd_gelu_vjp_f32       the reverse of the mapping network's exact (erf) GELU at its pre-activation (a few rows).
//   kd_bias_grad_f32      column sums of a gradient -- token rows with a row stride, or an NCHW image -- in runs of 256 rows whose partial sums
//                         (doubles) a second pass adds in ascending order; the first q_cols columns take the folded 1 / 8 of a qkv projection.
// No kernel uses atomics or reads a library option.
#include <cmath>

#include "kd_common.h"
#include "../../include/kdiff_unet_train.h"

namespace kd {

namespace {

constexpr int RUN = 256;          // rows per partial sum of kd_bias_grad_f32

__device__ __forceinline__ double gelu_grad(double a) {
  return 0.5 * (1.0 + erf(a * 0.70710678118654752440)) + a * (0.39894228040143267794 * exp(-0.5 * a * a));
}

template <bool GELU>
__global__ __launch_bounds__(256) void adagn_wb_grad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ stats,
                                                            const float* __restrict__ wb, int wb_stride, const float* __restrict__ gy, int ldgy,
                                                            float* __restrict__ gwb, int gwb_stride, int hw, int chan, int cpg, int groups,
                                                            int c_blocks) {
  __shared__ double sh[2][8][32];
  const int b = blockIdx.x / c_blocks, cb = blockIdx.x - b * c_blocks;
  const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int c = cb * 32 + cl;
  double sw = 0.0, sb = 0.0;
  if (c < chan) {
    const float* st = stats + 4 * ((size_t)b * groups + c / cpg);
    const double mean = (double)st[0] + (double)st[1], rstd = (double)st[2];
    const float* wrow = wb + (size_t)b * wb_stride;
    const double gain = 1.0 + (double)wrow[c], shift = (double)wrow[chan + c];
    const float* xs = x + (size_t)b * hw * ldx + c;
    const float* gs = gy + (size_t)b * hw * ldgy + c;
    for (int pix = pl; pix < hw; pix += 8) {
      const double xh = ((double)xs[(size_t)pix * ldx] - mean) * rstd;
      double gp = (double)gs[(size_t)pix * ldgy];
      if (GELU) gp *= gelu_grad(xh * gain + shift);
      sw += gp * xh;
      sb += gp;
    }
  }
  sh[0][pl][cl] = sw;
  sh[1][pl][cl] = sb;
  __syncthreads();
  if (pl == 0 && c < chan) {
    sw = sh[0][0][cl];
    sb = sh[1][0][cl];
    for (int k = 1; k < 8; ++k) {
      sw += sh[0][k][cl];
      sb += sh[1][k][cl];
    }
    float* o = gwb + (size_t)b * gwb_stride;
    o[c] = (float)sw;
    o[chan + c] = (float)sb;
  }
}

__global__ __launch_bounds__(256) void gelu_vjp_kernel(const float* __restrict__ pre, const float* gy, float* gx, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) gx[i] = (float)((double)gy[i] * gelu_grad((double)pre[i]));
}

// ws[run][c] = the sum of g[row][c] over the run's rows: 64 columns x 4 row lanes per workgroup, the 4 partial sums added in ascending order
__global__ __launch_bounds__(256) void bias_grad_runs_kernel(const float* __restrict__ g, int ldg, double* __restrict__ ws, int rows, int cols,
                                                             int nchw, int col_blocks) {
  __shared__ double sh[4][64];
  const int run = blockIdx.x / col_blocks, cb = blockIdx.x - run * col_blocks;
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = cb * 64 + cl;
  const int r1 = min(rows, (run + 1) * RUN);
  double s = 0.0;
  if (c < cols)
    for (int row = run * RUN + rl; row < r1; row += 4) {
      const size_t at = nchw ? ((size_t)(row / nchw) * cols + c) * nchw + row % nchw : (size_t)row * ldg + c;
      s += (double)g[at];
    }
  sh[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < cols) ws[(size_t)run * cols + c] = ((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl];
}

__global__ __launch_bounds__(256) void bias_grad_sum_kernel(const double* __restrict__ ws, float* __restrict__ out, int runs, int cols, int q_cols,
                                                            int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (int k = 0; k < runs; ++k) s += ws[(size_t)k * cols + c];
  if (c < q_cols) s *= 0.125;
  out[c] = accumulate ? out[c] + (float)s : (float)s;
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_adagn_wb_grad_f32(const float* x, int ldx, const float* stats, const float* wb, int wb_stride, const float* g_y, int ldgy,
                                    float* g_wb, int g_wb_stride, int batch, int hw, int chan, int groups, int gelu, void* stream) {
  if (!x || !stats || !wb || !g_y || !g_wb || batch <= 0 || hw <= 0 || chan <= 0 || groups <= 0)
    return fail(KD_EINVAL, "kd_adagn_wb_grad_f32: bad arguments");
  if (chan % groups) return fail(KD_EINVAL, "kd_adagn_wb_grad_f32: %d channels in %d groups", chan, groups);
  if (ldx < chan || ldgy < chan || wb_stride < 2 * chan || g_wb_stride < 2 * chan)
    return fail(KD_EINVAL, "kd_adagn_wb_grad_f32: a row stride is shorter than its row");
  if ((long)batch * hw > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_adagn_wb_grad_f32: %ld rows exceed the index range", (long)batch * hw);
  const int c_blocks = (chan + 31) / 32;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("adagn_wb_grad_f32", 0, 8.0 * batch * hw * chan, s);
  const dim3 grid((unsigned)((long)batch * c_blocks));
  if (gelu)
    launch<adagn_wb_grad_kernel<true>>(grid, dim3(256), 0, s, x, ldx, stats, wb, wb_stride, g_y, ldgy, g_wb, g_wb_stride, hw, chan, chan / groups,
                                       groups, c_blocks);
  else
    launch<adagn_wb_grad_kernel<false>>(grid, dim3(256), 0, s, x, ldx, stats, wb, wb_stride, g_y, ldgy, g_wb, g_wb_stride, hw, chan, chan / groups,
                                        groups, c_blocks);
  return check_launch("kd_adagn_wb_grad_f32");
}

extern "C" int kd_gelu_vjp_f32(const float* pre, const float* g_y, float* g_x, int n, void* stream) {
  if (!pre || !g_y || !g_x || n < 0) return fail(KD_EINVAL, "kd_gelu_vjp_f32: bad arguments");
  if (n == 0) return KD_OK;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("gelu_vjp_f32", 0, 12.0 * n, s);
  launch<gelu_vjp_kernel>(dim3((unsigned)std::min((n + 255) / 256, 4096)), dim3(256), 0, s, pre, g_y, g_x, n);
  return check_launch("kd_gelu_vjp_f32");
}

extern "C" int kd_bias_grad_f32(const float* g, int ldg, void* ws, float* out, int rows, int cols, int nchw, int q_cols, int accumulate,
                                void* stream) {
  if (!g || !ws || !out || rows <= 0 || cols <= 0 || nchw < 0) return fail(KD_EINVAL, "kd_bias_grad_f32: bad arguments");
  if (nchw ? rows % nchw != 0 : ldg < cols) return fail(KD_EINVAL, "kd_bias_grad_f32: rows = %d, ldg = %d, nchw = %d for %d columns", rows, ldg, nchw, cols);
  if (q_cols < 0 || q_cols > cols) return fail(KD_EINVAL, "kd_bias_grad_f32: q_cols = %d outside 0 .. cols = %d", q_cols, cols);
  if (reinterpret_cast<uintptr_t>(ws) & 7) return fail(KD_EINVAL, "kd_bias_grad_f32: the workspace holds doubles (8-byte aligned)");
  const int runs = (rows + RUN - 1) / RUN, col_blocks = (cols + 63) / 64;
  if ((long)runs * col_blocks > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_bias_grad_f32: %ld workgroups exceed the grid", (long)runs * col_blocks);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("bias_grad_f32", 0, 4.0 * rows * cols, s);
  launch<bias_grad_runs_kernel>(dim3((unsigned)(runs * col_blocks)), dim3(256), 0, s, g, ldg, (double*)ws, rows, cols, nchw, col_blocks);
  launch<bias_grad_sum_kernel>(dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, (const double*)ws, out, runs, cols, q_cols, accumulate);
  return check_launch("kd_bias_grad_f32");
}
