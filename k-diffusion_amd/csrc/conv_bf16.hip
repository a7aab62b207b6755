// Implicit-GEMM convolution of the image_v1 U-Net (gfx950) in bf16 arithmetic: what ImageDenoiserModelV1.set_conv_arithmetic("bf16") launches
// in place of kd_conv2d_x3 in the sampling forward.  kd_conv2d_x3's contract (conv_x3.hip): nn.Conv2d with kernel size 1 or 3, zero padding
// ks / 2 and stride 1 on fp32 NHWC activations (token-major [B H W, C] with a row stride), bias and a residual in the epilogue.
//
//   M = pixels, N = C_out, K = ks^2 C_in.  Every activation is rounded ONCE to bf16, round to nearest even (v_cvt_pk_bf16_f32: the rounding
//   of torch.Tensor.bfloat16()), while it is staged; every weight is its bf16 rounding -- the hi plane of kd_pack_conv_x3's image, the only
//   plane read here; a product is ONE v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Bias and residual are added in fp32.
//
// The tiling is conv_x3.hip's: one workgroup (4 waves) owns an 8 x 8 pixel patch of ONE sample x an N tile of 64 or 128 features, and stages
// the haloed patch once per chunk of 64 input channels; a position outside the image is SELECTED to zero and never loaded.  The schedule is
// not: without the lo images the patch is 12.8 KB and a tap's weight tile 16 KB, so the weight tile is double-buffered (45 KB in all at ks 3,
// N tile 128: three workgroups per CU).  The (chunk, tap) steps form one sequence; the global loads of step s + 1's weights -- and, on a
// chunk's last tap, of the next chunk's patch -- are requested into registers before step s's MFMAs and written to LDS after them, so they
// are in flight while the MFMAs run, and a tap costs ONE barrier: the write of step s + 1 goes to the buffer step s - 1 read, which every
// wave left before the barrier of step s.  The patch image has one buffer at ks 3 (one more barrier per 9 taps) and two at ks 1.
//
// MFMA roles and the epilogue are conv_x3.hip's: A = activations (rows = the wave's 32 pixels), B = weights (columns = 32 features).  No
// atomics, no library option: the accumulation order is fixed by the shape, a repeat gives the same bits.
#include "x3_common.h"
#include "../../include/kdiff_unet_bf16.h"

namespace kd {

namespace {

using b16::bf16x8;
using b16::pack_bf16;
using b16::u16;
using b16::u32x4;
using b16::swz128;

constexpr int PATCH = 8;          // pixels per patch side
constexpr int KC = 64;            // input channels per chunk (one 128-byte LDS row)

struct ConvB {
  const float* x;
  const u16* wp;
  const float* bias;
  const float* res;
  float* y;
  int ldx, ldr, ldy;
  int H, W, c_in, c_out;
  int ty_n, tx_n, n_tiles;
};

template <int KS>
constexpr int a_bufs() { return KS == 1 ? 2 : 1; }
template <int KS, int NB>
constexpr int lds_bytes() { return (a_bufs<KS>() * (PATCH + 2 * (KS / 2)) * (PATCH + 2 * (KS / 2)) + 2 * 64 * NB) * 128; }

template <int KS, int NB>      // kernel size, 32-feature blocks per wave (N tile = 64 NB)
__global__ __launch_bounds__(256, 3) void conv_bf16_kernel(const ConvB p) {
  constexpr int HALO = KS / 2, PWH = PATCH + 2 * HALO, PP = PWH * PWH, NT = 64 * NB, TAPS = KS * KS;
  constexpr int A_IT = (PP * 8 + 255) / 256;       // 32-byte pieces of the patch per thread
  constexpr int W_IT = NT * 8 / 256;               // 16-byte pieces of a weight tile per thread
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* a_img = lds;                                // a_bufs() images of PP rows
  char* w_img = lds + a_bufs<KS>() * PP * 128;      // two images of NT rows

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

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  f32x4 a_reg[A_IT][2];
  u32x4 w_reg[W_IT];

  // where this thread's pieces of the patch (8 channels of one position each) lie inside the sample, the same for every chunk; a piece outside
  // the image has no bit in a_ok and is never loaded
  size_t a_off[A_IT];
  unsigned a_ok = 0;
#pragma unroll
  for (int j = 0; j < A_IT; ++j) {
    const int it = tid + 256 * j;
    const int pos = it >> 3, q = it & 7;
    const int hy = pos / PWH, hx = pos - hy * PWH;
    const int gy = y0 + hy - HALO, gx = x0 + hx - HALO;
    const bool ok = it < PP * 8 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
    a_off[j] = ok ? ((size_t)gy * p.W + gx) * p.ldx + 8 * q : 0;
    a_ok |= (ok ? 1u : 0u) << j;
  }
  const float* x_b = p.x + pix0 * p.ldx;
  // ... and of a weight tile: row it >> 3, 16-byte piece it & 7 (the rows of piece j lie 32 j rows further on)
  const unsigned w_off = (unsigned)(tid >> 3) * p.c_in + 8 * (tid & 7);
  const u16* w_n0 = p.wp + (size_t)n0 * p.c_in;
  const size_t w_tap = (size_t)p.c_out * p.c_in;

  // request the patch of chunk c0
  auto load_a = [&](int c0) {
#pragma unroll
    for (int j = 0; j < A_IT; ++j) {
      a_reg[j][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      a_reg[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a_ok >> j & 1) {
        const float* src = x_b + c0 + a_off[j];
        a_reg[j][0] = *reinterpret_cast<const f32x4*>(src);
        a_reg[j][1] = *reinterpret_cast<const f32x4*>(src + 4);
      }
    }
  };
  // round it to bf16 and write it
  auto write_a = [&](char* img) {
#pragma unroll
    for (int j = 0; j < A_IT; ++j) {
      const int it = tid + 256 * j;
      if (it < PP * 8) {
        const f32x4 v0 = a_reg[j][0], v1 = a_reg[j][1];
        *reinterpret_cast<u32x4*>(img + swz128(it >> 3, it & 7)) =
            u32x4{pack_bf16(v0[0], v0[1]), pack_bf16(v0[2], v0[3]), pack_bf16(v1[0], v1[1]), pack_bf16(v1[2], v1[3])};
      }
    }
  };
  // request the weight tile of (chunk c0, tap): NT rows of 64 bf16 from the packed image's hi plane
  auto load_w = [&](int c0, int tap) {
    const u16* src = w_n0 + tap * w_tap + c0;
#pragma unroll
    for (int j = 0; j < W_IT; ++j) w_reg[j] = *reinterpret_cast<const u32x4*>(src + w_off + (size_t)(32 * j) * p.c_in);
  };
  auto write_w = [&](char* img) {
#pragma unroll
    for (int j = 0; j < W_IT; ++j) {
      const int it = tid + 256 * j;
      *reinterpret_cast<u32x4*>(img + swz128(it >> 3, it & 7)) = w_reg[j];
    }
  };

  load_a(0);
  load_w(0, 0);
  int step = 0;
  for (int c0 = 0; c0 < p.c_in; c0 += KC) {
    char* a_cur = a_img + (a_bufs<KS>() == 2 ? ((c0 / KC) & 1) * (PP * 128) : 0);
    if (a_bufs<KS>() == 1 && c0) __syncthreads();              // the previous chunk's last tap has left the one patch image
    write_a(a_cur);
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap, ++step) {
      char* w_cur = w_img + (step & 1) * (NT * 128);
      write_w(w_cur);
      // the next step's tile, requested on ONE path (two requests on two branches meet in a register copy, which waits for the data before
      // the MFMAs); the last step of all asks for its own tile again, which nobody reads
      const bool last_tap = tap == TAPS - 1, more = c0 + KC < p.c_in;
      load_w(last_tap && more ? c0 + KC : c0, last_tap ? (more ? 0 : tap) : tap + 1);
      if (last_tap && more) load_a(c0 + KC);
      __syncthreads();                                         // this step's images are in; everyone has left the previous step
      const int pos = pos0 + (tap / KS) * PWH + (tap % KS);
#pragma unroll
      for (int s = 0; s < KC / 16; ++s) {
        const int q = 2 * s + h;
        const bf16x8 av = *reinterpret_cast<const bf16x8*>(a_cur + swz128(pos, q));
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const int row = (wn * NB + nb) * 32 + r;
          const bf16x8 wv = *reinterpret_cast<const bf16x8*>(w_cur + swz128(row, q));
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, wv, acc[nb], 0, 0, 0);
        }
      }
    }
  }

#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = n0 + (wn * NB + nb) * 32 + r;
    const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int po = 32 * wm + mfma32_row(i, lane);
      const int gy = y0 + (po >> 3), gx = x0 + (po & 7);
      if (gy < p.H && gx < p.W) {
        const size_t pix = pix0 + (size_t)gy * p.W + gx;
        float v = acc[nb][i] + bv;
        if (p.res) v += p.res[pix * p.ldr + n];
        p.y[pix * p.ldy + n] = v;
      }
    }
  }
}

template <int KS, int NB>
int launch_conv(const ConvB& p, long n_wg, hipStream_t s) {
  launch<conv_bf16_kernel<KS, NB>>(dim3((unsigned)n_wg), dim3(256), lds_bytes<KS, NB>(), s, p);
  return check_launch("kd_conv2d_bf16");
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_conv2d_bf16(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy,
                              int batch, int H, int W, int c_in, int c_out, int ks, void* stream) {
  if (!x || !wp || !y || batch <= 0 || H <= 0 || W <= 0) return fail(KD_EINVAL, "kd_conv2d_bf16: bad arguments");
  if (ks != 1 && ks != 3) return fail(KD_EINVAL, "kd_conv2d_bf16: kernel size %d (1 or 3)", ks);
  if (c_in <= 0 || c_out <= 0 || (c_in % 64) || (c_out % 64))
    return fail(KD_EINVAL, "kd_conv2d_bf16: c_in = %d and c_out = %d must be multiples of 64", c_in, c_out);
  if (ldx < c_in || (ldx & 3) || ldy < c_out || (res && ldr < c_out))
    return fail(KD_EINVAL, "kd_conv2d_bf16: a row stride is shorter than its row (or ldx is no multiple of 4)");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wp)) & 15)
    return fail(KD_EINVAL, "kd_conv2d_bf16: x and the packed weight must be 16-byte aligned");
  ConvB p{x, (const u16*)wp, bias, res, y, ldx, ldr, ldy, H, W, c_in, c_out, (H + PATCH - 1) / PATCH, (W + PATCH - 1) / PATCH, 0};
  const int nb = (c_out % 128) ? 1 : 2;
  p.n_tiles = c_out / (64 * nb);
  const long n_wg = (long)batch * p.ty_n * p.tx_n * p.n_tiles;
  if (n_wg > 0x7FFFFFFFl || (long)batch * H * W > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_conv2d_bf16: %ld workgroups exceed the grid", n_wg);
  hipStream_t s = (hipStream_t)stream;
  const double m = (double)batch * H * W;
  ProfName nm("conv2d_bf16", "conv2d_bf16<k%d,n%d> M=%ld N=%d K=%d", ks, 64 * nb, (long)m, c_out, ks * ks * c_in);
  LaunchScope prof(nm, 2.0 * m * c_out * ks * ks * c_in, 4.0 * m * (c_in + c_out * (res ? 2 : 1)) + 2.0 * ks * ks * c_in * c_out, s);
  if (ks == 3) return nb == 2 ? launch_conv<3, 2>(p, n_wg, s) : launch_conv<3, 1>(p, n_wg, s);
  return nb == 2 ? launch_conv<1, 2>(p, n_wg, s) : launch_conv<1, 1>(p, n_wg, s);
}
