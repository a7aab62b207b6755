// Implicit-GEMM convolution of the image_v1 U-Net (gfx950), fp32-parity ("split3") arithmetic: nn.Conv2d with kernel size 1 or 3, zero
// padding ks / 2 and stride 1 on fp32 NHWC activations (token-major [B H W, C] with a row stride), k_diffusion/models/image_v1.py:21,25 and
// the 1 x 1 convolutions of layers.py:187-188.
//
//   M = pixels, N = C_out, K = ks^2 C_in.  Every fp32 operand is hi + lo bf16 (hi = bf16(x), lo = bf16(x - hi)); a product is three
//   v_mfma_f32_32x32x16_bf16 (lo hi, hi lo, hi hi) with fp32 accumulation, as in gemm_x3.hip.
//
// One workgroup (4 waves) owns an 8 x 8 pixel patch of ONE sample x an N tile of 64 or 128 features.  Per chunk of 64 input channels it
// stages the haloed patch ((8 + 2 halo)^2 positions x 64 channels) into LDS once, split hi / lo while staging; the ks^2 taps then read their
// shifted 8 x 8 window from that one image (a GEMM per tap would fetch the activations nine times).  A position outside the image -- the
// zero padding, and the part of a ragged patch beyond the image's edge -- is SELECTED to zero: it is never loaded, so a patch never reads a
// neighbouring sample's rows or memory outside the tensor.  The packed weights (kd_pack_conv_x3: per tap a [C_out][C_in] hi image and a lo
// image, bf16) are staged per (chunk, tap).  Both LDS images have 128-byte rows with the chunk swizzle of bf16_common.h (swz128).
//
// MFMA roles: A = activations (rows = the wave's 32 pixels), B = weights (columns = 32 features), so a lane owns feature lane & 31 and the
// 16 pixels (r & 3) + 8 (r >> 2) + 4 (lane >> 5): every accumulator register is stored as two 128-byte row segments.  The epilogue adds the
// bias and a residual (with its own row stride) and writes through the output's row stride -- the two halves of a skip concatenation are
// column ranges of one buffer.  No atomics: the accumulation order is fixed, a second run gives the same bits.
//
// kd_conv2d_x3_stacked is the same kernel for the dual pass of log_likelihood, whose batch is [primal | tangent]: only the samples below
// bias_batch get the bias.  A workgroup's sample index decides it, so an output's accumulation order -- and its bits -- are kd_conv2d_x3's.
//
// kd_conv2d_x3_drop (include/kdiff_unet_drop.h) is the same kernel again with the training loss's channel dropout in the epilogue:
// y = (acc + bias) m[b, n] + res, m a column range of the loss call's factor table (kd_chan_mask_f32).  Without a table the epilogue takes
// the branch it always took: the bits of kd_conv2d_x3.
#include "x3_common.h"
#include "../../include/kdiff_unet_drop.h"

namespace kd {

namespace {

using b16::bf16x8;
using b16::u16;
using b16::u32x4;
using b16::swz128;

constexpr int PATCH = 8;          // pixels per patch side
constexpr int KC = 64;            // input channels per chunk (one 128-byte LDS row)

struct ConvP {
  const float* x;
  const u16* wp;
  const float* bias;
  const float* res;
  float* y;
  int ldx, ldr, ldy;
  int H, W, c_in, c_out;
  int ty_n, tx_n, n_tiles;
  int bias_batch;                 // samples b < bias_batch get the bias (a stacked [primal | tangent] batch: the tangent of conv(x) + bias has none)
  const float* chan_scale;        // kd_conv2d_x3_drop: the (sample, channel) dropout factors m[b * chan_stride + n], or NULL
  int chan_stride;
};

__global__ __launch_bounds__(256) void pack_conv_kernel(const float* __restrict__ w, u16* __restrict__ out, int c_out, int c_in, int taps) {
  const long n_el = (long)taps * c_out * c_in;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long)gridDim.x * 256) {
    const int ci = (int)(i % c_in);
    const long t = i / c_in;
    const int n = (int)(t % c_out), tap = (int)(t / c_out);
    const float v = w[((long)n * c_in + ci) * taps + tap];
    const __bf16 hi = (__bf16)v;
    const __bf16 lo = (__bf16)(v - (float)hi);
    out[i] = __builtin_bit_cast(u16, hi);
    out[n_el + i] = __builtin_bit_cast(u16, lo);
  }
}

template <int KS, int NB>      // kernel size, 32-feature blocks per wave (N tile = 64 NB)
__global__ __launch_bounds__(256) void conv_x3_kernel(const ConvP p) {
  constexpr int HALO = KS / 2, PWH = PATCH + 2 * HALO, PP = PWH * PWH, NT = 64 * NB, TAPS = KS * KS;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* a_hi = lds;
  char* a_lo = lds + PP * 128;
  char* w_hi = lds + 2 * PP * 128;
  char* w_lo = w_hi + NT * 128;

  const int item = KD_XCD_CHUNK();
  const int nt = item % p.n_tiles;
  int patch = item / p.n_tiles;
  const int tx = patch % p.tx_n;
  patch /= p.tx_n;
  const int ty = patch % p.ty_n, b = patch / p.ty_n;
  const int n0 = nt * NT, y0 = ty * PATCH, x0 = tx * PATCH;
  const size_t pix0 = (size_t)b * p.H * p.W;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int pi = 32 * wm + r;                                  // this lane's pixel of the patch (A operand row)
  const int pos0 = (pi >> 3) * PWH + (pi & 7);                 // its position in the haloed image for tap (0, 0)
  const size_t plane = (size_t)TAPS * p.c_out * p.c_in;        // elements of the hi image; the lo image follows

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  for (int c0 = 0; c0 < p.c_in; c0 += KC) {
    __syncthreads();                                           // the previous chunk's last tap has been consumed
    for (int it = tid; it < PP * 8; it += 256) {
      const int pos = it >> 3, q = it & 7;
      const int hy = pos / PWH, hx = pos - hy * PWH;
      const int gy = y0 + hy - HALO, gx = x0 + hx - HALO;
      f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
      if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
        const float* src = p.x + (pix0 + (size_t)gy * p.W + gx) * p.ldx + c0 + 8 * q;
        v0 = *reinterpret_cast<const f32x4*>(src);
        v1 = *reinterpret_cast<const f32x4*>(src + 4);
      }
      u32x4 hi, lo;
      x3::split8(v0, v1, hi, lo);
      *reinterpret_cast<u32x4*>(a_hi + swz128(pos, q)) = hi;
      *reinterpret_cast<u32x4*>(a_lo + swz128(pos, q)) = lo;
    }
    for (int tap = 0; tap < TAPS; ++tap) {
      if (tap) __syncthreads();                                // the previous tap's weights have been consumed
      for (int it = tid; it < 2 * NT * 8; it += 256) {
        const int pl = it / (NT * 8), row = (it - pl * NT * 8) >> 3, q = it & 7;
        const u16* src = p.wp + pl * plane + ((size_t)tap * p.c_out + n0 + row) * p.c_in + c0 + 8 * q;
        *reinterpret_cast<u32x4*>(w_hi + pl * (NT * 128) + swz128(row, q)) = *reinterpret_cast<const u32x4*>(src);
      }
      __syncthreads();
      const int pos = pos0 + (tap / KS) * PWH + (tap % KS);
#pragma unroll
      for (int s = 0; s < KC / 16; ++s) {
        const int q = 2 * s + h;
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi + swz128(pos, q));
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(a_lo + swz128(pos, q));
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int row = (wn * NB + nb) * 32 + r;
          const bf16x8 wh = *reinterpret_cast<const bf16x8*>(w_hi + swz128(row, q));
          const bf16x8 wl = *reinterpret_cast<const bf16x8*>(w_lo + swz128(row, q));
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, wh, acc[nb], 0, 0, 0);
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, wl, acc[nb], 0, 0, 0);
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, wh, acc[nb], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = n0 + (wn * NB + nb) * 32 + r;
    const float bv = (p.bias && b < p.bias_batch) ? p.bias[n] : 0.f;
    const float ms = p.chan_scale ? p.chan_scale[(size_t)b * p.chan_stride + n] : 1.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int po = 32 * wm + mfma32_row(i, lane);
      const int gy = y0 + (po >> 3), gx = x0 + (po & 7);
      if (gy < p.H && gx < p.W) {
        const size_t pix = pix0 + (size_t)gy * p.W + gx;
        float v = acc[nb][i] + bv;
        if (p.chan_scale) v *= ms;
        if (p.res) v += p.res[pix * p.ldr + n];
        p.y[pix * p.ldy + n] = v;
      }
    }
  }
}

template <int KS, int NB>
int launch_conv(const ConvP& p, long n_wg, hipStream_t s) {
  constexpr int PWH = PATCH + 2 * (KS / 2), LDS = (2 * PWH * PWH + 2 * 64 * NB) * 128;
  launch<conv_x3_kernel<KS, NB>>(dim3((unsigned)n_wg), dim3(256), LDS, s, p);
  return check_launch("kd_conv2d_x3");
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_pack_conv_x3(const float* w, void* out, int c_out, int c_in, int ks, void* stream) {
  if (!w || !out || c_out <= 0 || c_in <= 0) return fail(KD_EINVAL, "kd_pack_conv_x3: bad arguments");
  if (ks != 1 && ks != 3) return fail(KD_EINVAL, "kd_pack_conv_x3: kernel size %d (1 or 3)", ks);
  const long n_el = (long)ks * ks * c_out * c_in;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("pack_conv_x3", 0, 8.0 * n_el, s);
  launch<pack_conv_kernel>(dim3((unsigned)std::min<long>((n_el + 255) / 256, 65536)), dim3(256), 0, s, w, (u16*)out, c_out, c_in, ks * ks);
  return check_launch("kd_pack_conv_x3");
}

// bias_batch: the samples that get the bias (kd_conv2d_x3: all of them)
static int conv2d_x3(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy, int batch, int H, int W,
                     int c_in, int c_out, int ks, int bias_batch, void* stream, const float* chan_scale = nullptr, int chan_stride = 0) {
  if (!x || !wp || !y || batch <= 0 || H <= 0 || W <= 0) return fail(KD_EINVAL, "kd_conv2d_x3: bad arguments");
  if (ks != 1 && ks != 3) return fail(KD_EINVAL, "kd_conv2d_x3: kernel size %d (1 or 3)", ks);
  if (c_in <= 0 || c_out <= 0 || (c_in % 64) || (c_out % 64))
    return fail(KD_EINVAL, "kd_conv2d_x3: c_in = %d and c_out = %d must be multiples of 64", c_in, c_out);
  if (ldx < c_in || (ldx & 3) || ldy < c_out || (res && ldr < c_out)) return fail(KD_EINVAL, "kd_conv2d_x3: a row stride is shorter than its row (or ldx is no multiple of 4)");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wp)) & 15) return fail(KD_EINVAL, "kd_conv2d_x3: x and the packed weight must be 16-byte aligned");
  ConvP p{x, (const u16*)wp, bias, res, y, ldx, ldr, ldy, H, W, c_in, c_out, (H + PATCH - 1) / PATCH, (W + PATCH - 1) / PATCH, 0, bias_batch, chan_scale, chan_stride};
  const int nb = (c_out % 128) ? 1 : 2;
  p.n_tiles = c_out / (64 * nb);
  const long n_wg = (long)batch * p.ty_n * p.tx_n * p.n_tiles;
  if (n_wg > 0x7FFFFFFFl || (long)batch * H * W > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_conv2d_x3: %ld workgroups exceed the grid", n_wg);
  hipStream_t s = (hipStream_t)stream;
  const double m = (double)batch * H * W;
  ProfName nm(chan_scale ? "conv2d_x3_drop" : "conv2d_x3", "conv2d_x3%s<k%d,n%d> M=%ld N=%d K=%d", chan_scale ? "_drop" : "", ks, 64 * nb, (long)m, c_out,
              ks * ks * c_in);
  LaunchScope prof(nm, 2.0 * m * c_out * ks * ks * c_in, 4.0 * m * (c_in + c_out * (res ? 2 : 1)) + 4.0 * ks * ks * c_in * c_out, s);
  if (ks == 3) return nb == 2 ? launch_conv<3, 2>(p, n_wg, s) : launch_conv<3, 1>(p, n_wg, s);
  return nb == 2 ? launch_conv<1, 2>(p, n_wg, s) : launch_conv<1, 1>(p, n_wg, s);
}

extern "C" int kd_conv2d_x3(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy,
                            int batch, int H, int W, int c_in, int c_out, int ks, void* stream) {
  return conv2d_x3(x, ldx, wp, bias, res, ldr, y, ldy, batch, H, W, c_in, c_out, ks, batch, stream);
}

extern "C" int kd_conv2d_x3_stacked(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy,
                                    int batch, int H, int W, int c_in, int c_out, int ks, int bias_batch, void* stream) {
  if (bias_batch < 0 || bias_batch > batch) return fail(KD_EINVAL, "kd_conv2d_x3_stacked: bias_batch = %d outside 0 .. batch = %d", bias_batch, batch);
  return conv2d_x3(x, ldx, wp, bias, res, ldr, y, ldy, batch, H, W, c_in, c_out, ks, bias_batch, stream);
}

extern "C" int kd_conv2d_x3_drop(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, const float* chan_scale,
                                 int chan_stride, float* y, int ldy, int batch, int H, int W, int c_in, int c_out, int ks, void* stream) {
  if (chan_scale && chan_stride < c_out) return fail(KD_EINVAL, "kd_conv2d_x3_drop: chan_stride = %d shorter than c_out = %d", chan_stride, c_out);
  return conv2d_x3(x, ldx, wp, bias, res, ldr, y, ldy, batch, H, W, c_in, c_out, ks, batch, stream, chan_scale, chan_scale ? chan_stride : 0);
}
