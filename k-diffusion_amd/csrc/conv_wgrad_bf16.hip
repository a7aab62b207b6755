// Weight gradient of the image_v1 U-Net's convolutions (gfx950) in bf16 arithmetic: what ImageDenoiserModelV1.set_wgrad_arithmetic("bf16")
// selects.  For nn.Conv2d with kernel size 1 or 3, zero padding ks / 2 and stride 1 on fp32 NHWC activations,
//
//   dW[co, ci, ky, kx] (+)= sum over (b, y, x) of bf16(G[b, y, x, co]) * bf16(A[b, y + ky - h, x + kx - h, ci]),   h = ks / 2.
//
// conv_wgrad_x3.hip with its lo half removed: the same 64 x 64 (co, ci) tile per workgroup for all ks^2 taps, the same run of 8 x 8 pixel
// patches, the same pixel-contiguous LDS layout [row][channel][8 pixels] with the A image kept once per x shift, the same workspace and the same
// second pass (conv_wgrad_reduce.h).  Every operand is rounded ONCE to bf16, round to nearest even (v_cvt_pk_bf16_f32: the rounding of
// torch.Tensor.bfloat16()), while it is staged; a product is one v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  There is no lo image:
// 38 912 B of LDS at ks = 3 (16 KB at ks = 1) against the split kernel's 77 824, a third of its MFMAs and half of its LDS writes; the global
// loads -- now the larger share of a patch -- are the same.
//
// A position outside the image is SELECTED to zero in both operands and never loaded; the order of every sum is fixed by the shape and the
// chunking handed in; no atomics.
#include "x3_common.h"
#include "conv_wgrad_reduce.h"
#include "../../include/kdiff_unet_mixed.h"

namespace kd {

namespace {

using b16::bf16x8;
using b16::pack_bf16;
using b16::u32x4;

constexpr int PATCH = 8;          // pixels per patch side
constexpr int TILE = 64;          // output channels / input channels per workgroup
constexpr int SLOT = 16;          // bytes of 8 bf16 pixels

struct WgB {
  const float* g;
  const float* a;
  float* ws;
  int ldg, lda;
  int H, W, c_in, c_out;
  int ty_n, tx_n, n_patches;      // patches per column / row of one sample, and of the whole batch
  int ci_tiles, n_tiles;          // 64-wide tiles along c_in, and of the whole weight
  int ppc;                        // patches per chunk
};

constexpr int lds_bytes(int ks) { return (PATCH + ks * (PATCH + 2 * (ks / 2))) * TILE * SLOT; }

// 8 consecutive fp32 pixels v[at .. at + 7] -> one slot of 8 bf16, each rounded to nearest even
template <int N>
__device__ __forceinline__ u32x4 round8(const float (&v)[N], int at) {
  return u32x4{pack_bf16(v[at], v[at + 1]), pack_bf16(v[at + 2], v[at + 3]), pack_bf16(v[at + 4], v[at + 5]), pack_bf16(v[at + 6], v[at + 7])};
}

template <int KS>
__global__ __launch_bounds__(256) void conv_wgrad_bf16_kernel(const WgB p) {
  constexpr int HALO = KS / 2, PWH = PATCH + 2 * HALO, TAPS = KS * KS;
  constexpr int G_IMG = PATCH * TILE * SLOT, A_IMG = PWH * TILE * SLOT;       // bytes of one image
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* g_img = lds;
  char* a_img = lds + G_IMG;                                                   // copy kx at a_img + kx A_IMG

  const int item = KD_XCD_CHUNK();
  const int tile = item % p.n_tiles, chunk = item / p.n_tiles;
  const int co0 = (tile / p.ci_tiles) * TILE, ci0 = (tile % p.ci_tiles) * TILE;
  const int pt0 = chunk * p.ppc, pt1 = min(p.n_patches, pt0 + p.ppc);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave & 1, wn = wave >> 1;

  f32x16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  for (int pt = pt0; pt < pt1; ++pt) {
    const int tx = pt % p.tx_n;
    const int rest = pt / p.tx_n;
    const int ty = rest % p.ty_n, b = rest / p.ty_n;
    const int y0 = ty * PATCH, x0 = tx * PATCH;
    const size_t pix0 = (size_t)b * p.H * p.W;
    __syncthreads();                                           // the previous patch has been consumed
    // G: one (patch row, co) per thread and round
    for (int it = tid; it < PATCH * TILE; it += 256) {
      const int py = it >> 6, c = it & 63;
      const int gy = y0 + py;
      float v[PATCH];
#pragma unroll
      for (int j = 0; j < PATCH; ++j) {
        const int gx = x0 + j;
        v[j] = 0.f;
        if (gy < p.H && gx < p.W) v[j] = p.g[(pix0 + (size_t)gy * p.W + gx) * p.ldg + co0 + c];
      }
      *reinterpret_cast<u32x4*>(g_img + it * SLOT) = round8(v, 0);
    }
    // A: one (haloed row, ci) per thread and round, written once per x shift
    for (int it = tid; it < PWH * TILE; it += 256) {
      const int hy = it >> 6, c = it & 63;
      const int gy = y0 + hy - HALO;
      float v[PWH];
#pragma unroll
      for (int j = 0; j < PWH; ++j) {
        const int gx = x0 + j - HALO;
        v[j] = 0.f;
        if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) v[j] = p.a[(pix0 + (size_t)gy * p.W + gx) * p.lda + ci0 + c];
      }
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) *reinterpret_cast<u32x4*>(a_img + kx * A_IMG + it * SLOT) = round8(v, kx);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PATCH / 2; ++s) {                      // a k-step: the 16 pixels of patch rows 2 s and 2 s + 1
      const int py = 2 * s + h;
      const bf16x8 gv = *reinterpret_cast<const bf16x8*>(g_img + (py * TILE + 32 * wm + r) * SLOT);
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int a_at = ((py + ky) * TILE + 32 * wn + r) * SLOT;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(a_img + kx * A_IMG + a_at);
          f32x16& d = acc[ky * KS + kx];
          d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gv, av, d, 0, 0, 0);
        }
      }
    }
  }

  // the partial tile: rows = co (the first operand's), a lane's column = ci
  const size_t plane = (size_t)p.c_out * p.c_in;
  float* dst = p.ws + (size_t)chunk * TAPS * plane + ci0 + 32 * wn + r;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = co0 + 32 * wm + mfma32_row(i, lane);
      dst[t * plane + (size_t)co * p.c_in] = acc[t][i];
    }
}

template <int KS>
int launch_wgrad(const WgB& p, long n_wg, hipStream_t s) {
  launch<conv_wgrad_bf16_kernel<KS>>(dim3((unsigned)n_wg), dim3(256), lds_bytes(KS), s, p);
  return check_launch("kd_conv2d_wgrad_bf16");
}

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_conv2d_wgrad_bf16(const float* g, int ldg, const float* a, int lda, float* ws, float* dw, int batch, int H, int W, int c_in,
                                    int c_out, int ks, int q_rows, int patches_per_chunk, int nchunk, int accumulate, void* stream) {
  if (!g || !a || !ws || !dw || batch <= 0 || H <= 0 || W <= 0) return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: bad arguments");
  if (ks != 1 && ks != 3) return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: kernel size %d (1 or 3)", ks);
  if (c_in <= 0 || c_out <= 0 || (c_in % TILE) || (c_out % TILE))
    return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: c_in = %d and c_out = %d must be multiples of 64", c_in, c_out);
  if (ldg < c_out || lda < c_in) return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: a row stride is shorter than its row");
  if (q_rows < 0 || q_rows > c_out) return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: q_rows = %d outside 0 .. c_out = %d", q_rows, c_out);
  const long pixels = (long)batch * H * W;
  if (pixels > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: %ld pixels exceed the index range", pixels);
  const int ty_n = (H + PATCH - 1) / PATCH, tx_n = (W + PATCH - 1) / PATCH;
  const long n_patches = (long)batch * ty_n * tx_n;
  if (patches_per_chunk <= 0 || nchunk <= 0 || (long)nchunk != (n_patches + patches_per_chunk - 1) / patches_per_chunk)
    return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: %d chunks of %d patches do not cut %ld patches", nchunk, patches_per_chunk, n_patches);
  WgB p{g, a, ws, ldg, lda, H, W, c_in, c_out, ty_n, tx_n, (int)n_patches, c_in / TILE, (c_in / TILE) * (c_out / TILE), patches_per_chunk};
  const long n_wg = (long)nchunk * p.n_tiles;
  if (n_wg > 0x7FFFFFFFl) return fail(KD_EINVAL, "kd_conv2d_wgrad_bf16: %ld workgroups exceed the grid", n_wg);
  hipStream_t s = (hipStream_t)stream;
  const double m = (double)pixels, n_el = (double)ks * ks * c_in * c_out;
  {
    ProfName nm("conv2d_wgrad_bf16", "conv2d_wgrad_bf16<k%d> M=%ld N=%d K=%d chunks=%d", ks, (long)pixels, c_out, ks * ks * c_in, nchunk);
    LaunchScope prof(nm, 2.0 * m * n_el, 4.0 * m * (c_in + c_out) + 4.0 * nchunk * n_el, s);
    const int rc = ks == 3 ? launch_wgrad<3>(p, n_wg, s) : launch_wgrad<1>(p, n_wg, s);
    if (rc != KD_OK) return rc;
  }
  LaunchScope prof("conv2d_wgrad_reduce", 0, 4.0 * (nchunk + 1) * n_el, s);
  const long n_out = (long)ks * ks * c_in * c_out;
  launch<conv_wgrad_reduce_kernel>(dim3((unsigned)std::min<long>((n_out + 255) / 256, 65536)), dim3(256), 0, s, (const float*)ws, dw, c_out, c_in,
                                   ks * ks, nchunk, q_rows, accumulate);
  return check_launch("kd_conv2d_wgrad_bf16");
}
