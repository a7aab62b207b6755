// Parameter-gradient kernels of the HDiT denoiser (gfx950), fp32-grade arithmetic: what models/vjp.py adds to its reverse walk when
// Denoiser.loss asks for the gradients of the weights.
//
//   kd_wgrad_f32          dW[N, K] (+)= alpha * sum_m G[m, n] * A[m, k]: the weight gradient of a projection, both operands stored
//                         M-major.  split3 (the backward pass's rule under split3 / bf16 / fp8): every operand split into bf16 hi + lo in
//                         the staging pass, 3 bf16 MFMAs per product (hi hi, hi lo, lo hi), fp32 accumulate; exact: fp32 FMAs; bf16 (opt-in,
//                         the reference's --mixed-precision bf16 Linear backward): both operands rounded to bf16 after their whole
//                         prologue, 1 bf16 MFMA per product, fp32 accumulate.  Either operand may be read through the 2x2 token-merge or the NCHW patch gather; A may be
//                         scaled per row (RMSNorm rrms) and per (sample, column) (AdaRMSNorm scale) or be the GEGLU of [value | gate]
//                         rows, so normalised rows are never written to memory just to be read back.
//   kd_wgrad_drop_f32     the same with A's plain rows under a dropout mask (the FF hidden's dW_down = G^T (mask * geglu(U))): the
//                         site's mask is first written as bits (dropout_f32.hip) and the prologue multiplies by
//                         scale or 0 from one cached word per element.
//   kd_row_rrms_f32       rrms[r] = rsqrt(mean(x[r]^2) + eps), the RMSNorm statistic the operand prologue and the scale gradients use
//   kd_colsum_f32         out[s, j] (+)= sum over the rows r of segment s of a[r, j] * (b[r, j] - b2[r, j]) * rs[r]: AdaRMSNorm / RMSNorm
//                         scale gradients, the TokenSplit fac, the attention scale's per-column terms
//   kd_attn_scale_grad_f32  d scale[h] (+)= sum of the q and k columns of head h / (2 scale[h])
//   kd_class_emb_grad_f32   d class_emb[c, :] (+)= sum over {b : ids[b] == c} of g[b, :], b ascending
//   kd_loss_prep_f32 / kd_loss_f32 / kd_loss_vjp_f32   the Karras denoiser loss (k_diffusion/layers.py:76-86) and its gradient
//
// Every sum has a fixed shape and order: the row dimension is cut into chunks that depend on the problem shape alone, each chunk's
// partial goes to a workspace and a second launch adds the chunks in ascending order.  No atomics: bit-identical on repeat.
#include "kd_common.h"
#include "x3_common.h"

#include <cmath>
#include <cstdint>

namespace kd {

namespace {

enum { WG_PLAIN = 0, WG_MERGE2x2 = 1, WG_PATCH_NCHW = 2 };
enum { WG_EXACT = 0, WG_SPLIT3 = 1, WG_BF16 = 2 };      // the arithmetic selector (the C ABI's split3 argument)

struct WgOperand {
  const float* p;
  int mode;              // WG_* gather of the stored rows
  int cols;              // logical columns
  int geglu;             // A only: p holds [value | gate] rows of 2 * cols, the operand is value * gelu(gate)
  const float* row_scale;
  const float* col_scale;
  int col_stride;        // 0: one shared row of col_scale; else per sample (rows_per_sample rows each)
  const unsigned* bits;  // A only, DROP kernels: the dropout mask of the plain [M, cols] operand (dropout_f32.hip), kept elements times drop_scale
  float drop_scale;
  int wide;              // bf16 kernel: plain rows, cols % 4 == 0 and 16-byte aligned pointers: 4 columns per load
};

struct WgGeom {
  int gh, gw;            // coarse token grid of the gathered operand's rows
  int ph, pw, chan;      // patch size and image channels (PATCH), or fine channels (MERGE, ph = pw = 2)
  int rows_per_sample;
};

__device__ __forceinline__ float gelu_erf(float g) { return g * 0.5f * (1.0f + erff(g * 0.70710678118654752440f)); }

// the operand's element (m, k); m < M and k < cols are checked by the caller
template <bool DROP>
__device__ __forceinline__ float wg_load(const WgOperand& o, const WgGeom& q, long m, int k) {
  float v;
  if (o.mode == WG_PLAIN) {
    if (o.geglu) {
      const float* r = o.p + m * 2 * (long)o.cols;
      v = r[k] * gelu_erf(r[o.cols + k]);
    } else {
      v = o.p[m * o.cols + k];
    }
    if (DROP) {
      const long e = m * o.cols + k;
      v *= ((o.bits[e >> 5] >> (e & 31)) & 1u) ? o.drop_scale : 0.0f;
    }
  } else {
    const long per = (long)q.gh * q.gw;
    const long b = m / per;
    const int t = (int)(m - b * per);
    const int i = t / q.gw, j = t - (t / q.gw) * q.gw;
    const int blk = k / q.chan, e = k - blk * q.chan;      // (py px e) ordering of the token merge / patch
    const int py = blk / q.pw, px = blk - py * q.pw;
    const long H = (long)q.gh * q.ph, W = (long)q.gw * q.pw;
    const long y = (long)i * q.ph + py, x = (long)j * q.pw + px;
    if (o.mode == WG_MERGE2x2) v = o.p[((b * H + y) * W + x) * q.chan + e];        // NHWC fine grid
    else v = o.p[((b * q.chan + e) * H + y) * W + x];                             // NCHW image
  }
  if (o.row_scale) v *= o.row_scale[m];
  if (o.col_scale) v *= o.col_scale[(m / q.rows_per_sample) * o.col_stride + k];
  return v;
}

// ---- weight gradient: 64 (n) x 64 (k) output tile per workgroup, 16 rows of m per LDS step, 4 x 4 products per lane ---------------
constexpr int WT = 64, WR = 16;

template <bool DROP>
__global__ __launch_bounds__(256) void wgrad_partial_kernel(WgOperand G, WgOperand A, WgGeom q, long M, int N, int K, int chunk_rows,
                                                            float* __restrict__ ws) {
  __shared__ float gs[WR][WT];
  __shared__ float as[WR][WT];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.x * WT, k0 = blockIdx.y * WT;
  const long m_begin = (long)blockIdx.z * chunk_rows;
  const long m_end = min(M, m_begin + chunk_rows);
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (long m0 = m_begin; m0 < m_end; m0 += WR) {
#pragma unroll
    for (int e = tid; e < WR * WT; e += 256) {
      const int r = e / WT, c = e % WT;
      const long m = m0 + r;
      const bool in_m = m < m_end;
      gs[r][c] = (in_m && n0 + c < N) ? wg_load<false>(G, q, m, n0 + c) : 0.f;
      as[r][c] = (in_m && k0 + c < K) ? wg_load<DROP>(A, q, m, k0 + c) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < WR; ++r) {
      float gv[4], av[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) gv[i] = gs[r][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) av[j] = as[r][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(gv[i], av[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* out = ws + (long)blockIdx.z * N * K;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 16 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + tx + 16 * j;
      if (n < N && k < K) out[(long)n * K + k] = acc[i][j];
    }
  }
}

// ---- weight gradient, split3 on the matrix cores: 64 (n) x 64 (k) output tile per workgroup of 4 waves (2 x 2 of 32 x 32), 32 rows of m
// per LDS step.  Staging: lane (c, g) loads 8 consecutive rows of column c of each panel (coalesced along the columns), splits them into
// bf16 hi / lo and writes each as ONE 16-byte store at [column c][rows 8g .. 8g+7] of an m-contiguous image: the transpose happens in the
// staging write, so each MFMA fragment (8 consecutive m of one row of G^T or one column of A) is one ds_read_b128.  Rows of the images are
// padded to 80 bytes (rows 16 banks apart would put 4 lanes of a half-wave on one bank).  The next panel's global loads are issued before
// the current panel's MFMAs.  MFMA 32x32x16 bf16: src0 = G^T (row n), src1 = A (column k), accumulated over m in a fixed order.
constexpr int XR = 32, XS = 40;                    // rows of m per step; image row stride in bf16 (80 bytes)

template <bool DROP>
__device__ __forceinline__ void x3_load(const WgOperand& o, const WgGeom& q, long m0, long m_end, int col, int cols, float (&v)[8]) {
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const long m = m0 + g * 8 + i;
    v[i] = (m < m_end && col + c < cols) ? wg_load<DROP>(o, q, m, col + c) : 0.f;
  }
}

__device__ __forceinline__ void x3_stage(const float (&v)[8], b16::u16* hi_img, b16::u16* lo_img) {
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  b16::u32x4 hi, lo;
  x3::split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, hi, lo);
  *reinterpret_cast<b16::u32x4*>(hi_img + c * XS + g * 8) = hi;
  *reinterpret_cast<b16::u32x4*>(lo_img + c * XS + g * 8) = lo;
}

__device__ __forceinline__ b16::bf16x8 x3_frag(const b16::u16* img, int row, int k8) {
  return __builtin_bit_cast(b16::bf16x8, *reinterpret_cast<const b16::u32x4*>(img + row * XS + k8));
}

template <bool DROP>
__global__ __launch_bounds__(256) void wgrad_x3_partial_kernel(WgOperand G, WgOperand A, WgGeom q, long M, int N, int K, int chunk_rows,
                                                               float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) b16::u16 img[4][WT * XS];     // G^T hi, G^T lo, A^T hi, A^T lo
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wn = wave & 1, wk = wave >> 1;
  const int n0 = blockIdx.x * WT, k0 = blockIdx.y * WT;
  const long m_begin = (long)blockIdx.z * chunk_rows;
  const long m_end = min(M, m_begin + chunk_rows);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float gv[8], av[8];
  x3_load<false>(G, q, m_begin, m_end, n0, N, gv);
  x3_load<DROP>(A, q, m_begin, m_end, k0, K, av);
  for (long m0 = m_begin; m0 < m_end; m0 += XR) {
    x3_stage(gv, img[0], img[1]);
    x3_stage(av, img[2], img[3]);
    __syncthreads();
    if (m0 + XR < m_end) {
      x3_load<false>(G, q, m0 + XR, m_end, n0, N, gv);
      x3_load<DROP>(A, q, m0 + XR, m_end, k0, K, av);
    }
#pragma unroll
    for (int ks = 0; ks < XR / 16; ++ks) {
      const int k8 = ks * 16 + lh * 8;
      const b16::bf16x8 gh = x3_frag(img[0], wn * 32 + l31, k8), gl = x3_frag(img[1], wn * 32 + l31, k8);
      const b16::bf16x8 ah = x3_frag(img[2], wk * 32 + l31, k8), al = x3_frag(img[3], wk * 32 + l31, k8);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl, ah, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, al, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh, ah, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  float* out = ws + (long)blockIdx.z * N * K;
  const int k = k0 + wk * 32 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (n < N && k < K) out[(long)n * K + k] = acc[r];
  }
}

// ---- weight gradient, bf16 operands on the matrix cores: 128 (n) x 128 (k) output tile per workgroup of 4 waves (2 x 2 of 64 x 64, four
// 32 x 32 accumulators each), 32 rows of m per LDS step, ONE MFMA per product.  Every operand element is rounded to bf16 (nearest even) after
// its whole prologue (gather, GEGLU, dropout mask, row and column scale).  Staging of its own: waves 0, 1 stage the G panel and waves 2, 3
// the A panel, a lane holding 4 adjacent columns x 8 consecutive rows -- one 16-byte load per row where the operand's rows are plain
// (WgOperand::wide), element loads through wg_load otherwise -- and writing each column's 8 rows as ONE 16-byte store of an m-contiguous
// image, so each MFMA fragment is one ds_read_b128.  Image: 4 columns x 32 m (64 bytes each) + 16 bytes of padding per column group
// (272 bytes): the 8 lanes of a ds_write_b128 group (8 column groups, 272 bytes apart) and the 16 lanes of a ds_read_b128 group land on
// distinct banks.  Two images per operand: the next panel is loaded before the current panel's MFMAs and staged after them into the other
// buffer, one barrier per step.
constexpr int BT = 128, BR = 32;                   // output tile edge; rows of m per step
constexpr int BGRP = 136;                          // image stride of a 4-column group in bf16 (272 bytes)
constexpr int BIMG = (BT / 4) * BGRP;              // one operand image in bf16

__device__ __forceinline__ long wg_sample(long m, int rows_per_sample) {
  return (m >> 31) ? m / rows_per_sample : (long)((unsigned)m / (unsigned)rows_per_sample);
}

// rows m0 .. m0 + 7 (the caller's panel row + 8 g) of columns col .. col + 3 (the tile's first column + 4 cq), zero outside the chunk and the matrix
template <bool DROP>
__device__ __forceinline__ void b16_load(const WgOperand& o, const WgGeom& q, long m0, long m_end, int col, int cols, float (&v)[8][4]) {
  if (o.wide) {
    const bool in_c = col < cols;                  // cols % 4 == 0: the 4 columns are inside together
    f32x4 cs{1.f, 1.f, 1.f, 1.f};
    long cs_sample = -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long m = m0 + i;
      f32x4 x{0.f, 0.f, 0.f, 0.f};
      if (in_c && m < m_end) {
        if (o.geglu) {
          const float* r = o.p + m * 2 * (long)o.cols + col;
          const f32x4 val = *reinterpret_cast<const f32x4*>(r), gate = *reinterpret_cast<const f32x4*>(r + o.cols);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = val[j] * gelu_erf(gate[j]);
        } else {
          x = *reinterpret_cast<const f32x4*>(o.p + m * o.cols + col);
        }
        if (DROP) {
          const long e = m * o.cols + col;          // e % 4 == 0: the 4 bits share a word
          const unsigned nib = o.bits[e >> 5] >> (e & 31);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] *= ((nib >> j) & 1u) ? o.drop_scale : 0.0f;
        }
        if (o.row_scale) {
          const float rs = o.row_scale[m];
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] *= rs;
        }
        if (o.col_scale) {
          const long sm = o.col_stride ? wg_sample(m, q.rows_per_sample) : 0;
          if (sm != cs_sample) {
            cs = *reinterpret_cast<const f32x4*>(o.col_scale + sm * o.col_stride + col);
            cs_sample = sm;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] *= cs[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = x[j];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long m = m0 + i;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = (m < m_end && col + j < cols) ? wg_load<DROP>(o, q, m, col + j) : 0.f;
    }
  }
}

// column group cq, rows 8g .. 8g + 7 of one operand image: the transpose happens here
__device__ __forceinline__ void b16_stage(const float (&v)[8][4], b16::u16* img, int cq, int g) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<b16::u32x4*>(img + cq * BGRP + j * BR + g * 8) =
        b16::u32x4{b16::pack_bf16(v[0][j], v[1][j]), b16::pack_bf16(v[2][j], v[3][j]), b16::pack_bf16(v[4][j], v[5][j]), b16::pack_bf16(v[6][j], v[7][j])};
}

__device__ __forceinline__ b16::bf16x8 b16_frag(const b16::u16* img, int row, int k8) {
  return __builtin_bit_cast(b16::bf16x8, *reinterpret_cast<const b16::u32x4*>(img + (row >> 2) * BGRP + (row & 3) * BR + k8));
}

template <bool DROP>
__global__ __launch_bounds__(256) void wgrad_b16_partial_kernel(WgOperand G, WgOperand A, WgGeom q, long M, int N, int K, int chunk_rows,
                                                                float* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) b16::u16 img[2][2][BIMG];     // [buffer][G^T, A^T]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wn = wave & 1, wk = wave >> 1;
  const int n0 = blockIdx.x * BT, k0 = blockIdx.y * BT;
  const long m_begin = (long)blockIdx.z * chunk_rows;
  const long m_end = min(M, m_begin + chunk_rows);
  const int side = wave >> 1;                      // waves 0, 1 stage G, waves 2, 3 stage A
  const int cq = threadIdx.x & 31, g = (threadIdx.x >> 5) & 3;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float v[8][4];
  auto load = [&](long m0) {
    if (side) b16_load<DROP>(A, q, m0 + g * 8, m_end, k0 + 4 * cq, K, v);
    else b16_load<false>(G, q, m0 + g * 8, m_end, n0 + 4 * cq, N, v);
  };
  load(m_begin);
  b16_stage(v, img[0][side], cq, g);
  __syncthreads();
  int buf = 0;
  for (long m0 = m_begin; m0 < m_end; m0 += BR, buf ^= 1) {
    const bool more = m0 + BR < m_end;
    if (more) load(m0 + BR);
#pragma unroll
    for (int ks = 0; ks < BR / 16; ++ks) {
      const int k8 = ks * 16 + lh * 8;
      b16::bf16x8 gf[2], af[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        gf[i] = b16_frag(img[buf][0], wn * 64 + i * 32 + l31, k8);
        af[i] = b16_frag(img[buf][1], wk * 64 + i * 32 + l31, k8);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf[i], af[j], acc[i][j], 0, 0, 0);
    }
    if (more) b16_stage(v, img[buf ^ 1][side], cq, g);
    __syncthreads();
  }
  float* out = ws + (long)blockIdx.z * N * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk * 64 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (n < N && k < K) out[(long)n * K + k] = acc[i][j][r];
      }
    }
}

// chunks added in ascending order; alpha (a device scalar or NULL) scales the sum; accumulate adds the result to dW
__global__ __launch_bounds__(256) void chunk_reduce_kernel(const float* __restrict__ ws, int nchunk, long n, const float* alpha, int accumulate,
                                                           float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float s = 0.f;
    for (int c = 0; c < nchunk; ++c) s += ws[(long)c * n + i];
    if (alpha) s *= alpha[0];
    out[i] = accumulate ? out[i] + s : s;
  }
}

// ---- RMSNorm statistic: one wave per row ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_rrms_kernel(const float* __restrict__ x, float* __restrict__ rrms, long rows, int d, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                 // whole waves exit together
  const float* xr = x + row * d;
  float ss = 0.f;
  for (int i = lane; i < d; i += 64) ss = fmaf(xr[i], xr[i], ss);
  ss = wave_sum_xor(ss, 64);
  if (lane == 0) rrms[row] = rsqrtf(ss / (float)d + eps);
}

// ---- column sums: a lane per column, CS_ROWS rows per chunk --------------------------------------------------------------------------
constexpr int CS_ROWS = 64;

__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ b2,
                                                             const float* __restrict__ rs, long rows_per_seg, int cols, int nchunk,
                                                             float* __restrict__ ws) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int chunk = blockIdx.y;
  const long seg = blockIdx.z;
  if (j >= cols) return;
  const long r0 = seg * rows_per_seg + (long)chunk * CS_ROWS;
  const long r1 = min(seg * rows_per_seg + rows_per_seg, r0 + CS_ROWS);
  float s = 0.f;
  for (long r = r0; r < r1; ++r) {
    float v = a[r * cols + j];
    if (b) v *= b2 ? b[r * cols + j] - b2[r * cols + j] : b[r * cols + j];
    if (rs) v *= rs[r];
    s += v;
  }
  ws[(seg * nchunk + chunk) * cols + j] = s;
}

__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ ws, int nseg, int nchunk, int cols, int accumulate,
                                                            float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)nseg * cols) return;
  const long seg = i / cols;
  const int j = (int)(i - seg * cols);
  float s = 0.f;
  for (int c = 0; c < nchunk; ++c) s += ws[(seg * nchunk + c) * cols + j];
  out[i] = accumulate ? out[i] + s : s;
}

// ---- attention scale: colsum holds sum over tokens of g_p * p per column of the [3, nh, 64] qkv row (p the prepared q, k) ------------
// p = sqrt(scale) R(q rho)  =>  d scale = sum g_p . p / (2 scale)
__global__ void attn_scale_grad_kernel(const float* __restrict__ colsum, const float* __restrict__ scale, int nh, int accumulate, float* out) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= nh) return;
  float s = 0.f;
  for (int t = 0; t < 2; ++t)
    for (int d = 0; d < 64; ++d) s += colsum[(t * nh + h) * 64 + d];
  s = s / (2.0f * scale[h]);
  out[h] = accumulate ? out[h] + s : s;
}

// ---- class embedding: a lane per (class, column), samples in ascending order ---------------------------------------------------------
__global__ __launch_bounds__(256) void class_emb_grad_kernel(const float* __restrict__ g, const long long* __restrict__ ids, int batch, int d,
                                                             int n_cls, int accumulate, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n_cls * d) return;
  const int c = (int)(i / d), j = (int)(i - (long)c * d);
  float s = 0.f;
  for (int b = 0; b < batch; ++b)
    if (ids[b] == c) s += g[(long)b * d + j];
  out[i] = accumulate ? out[i] + s : s;
}

// ---- the loss (k_diffusion/layers.py:70-86) ----------------------------------------------------------------------------------------
enum { LW_KARRAS = 0, LW_SOFT_MIN_SNR = 1, LW_SNR = 2, LW_GIVEN = 3 };

struct Karras {
  float c_skip, c_out, c_in, c_weight;
};

__device__ __forceinline__ Karras karras(float sigma, float sd, int weighting, const float* c_weight, int b) {
  const float var = sigma * sigma + sd * sd;
  Karras k;
  k.c_skip = sd * sd / var;
  k.c_out = sigma * sd / sqrtf(var);
  k.c_in = 1.0f / sqrtf(var);
  if (weighting == LW_SOFT_MIN_SNR) k.c_weight = (sigma * sd) * (sigma * sd) / (var * var);
  else if (weighting == LW_SNR) k.c_weight = sd * sd / var;
  else if (weighting == LW_GIVEN) k.c_weight = c_weight[b];
  else k.c_weight = 1.0f;
  return k;
}

__global__ __launch_bounds__(256) void loss_prep_kernel(const float* __restrict__ input, const float* __restrict__ noise, const float* __restrict__ sigma,
                                                        float sd, float* __restrict__ noised, float* __restrict__ x_in, int batch, long per) {
  const long n = (long)batch * per;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int b = (int)(i / per);
    const float s = sigma[b];
    const float v = input[i] + noise[i] * s;
    noised[i] = v;
    x_in[i] = v * (1.0f / sqrtf(s * s + sd * sd));
  }
}

// one workgroup per sample: strided partial sums, then a fixed tree over the 256 lanes
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ f, const float* __restrict__ input, const float* __restrict__ noised,
                                                   const float* __restrict__ sigma, float sd, int weighting, const float* c_weight, long per,
                                                   float* __restrict__ losses) {
  __shared__ float red[256];
  const int b = blockIdx.x;
  const Karras k = karras(sigma[b], sd, weighting, c_weight, b);
  const long base = (long)b * per;
  float s = 0.f;
  for (long i = threadIdx.x; i < per; i += 256) {
    const float t = (input[base + i] - k.c_skip * noised[base + i]) / k.c_out;
    const float e = f[base + i] - t;
    s = fmaf(e, e, s);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) losses[b] = red[0] / (float)per * k.c_weight;
}

// dF = g[b] c_weight[b] 2 (F - target) / n
__global__ __launch_bounds__(256) void loss_vjp_kernel(const float* __restrict__ f, const float* __restrict__ input, const float* __restrict__ noised,
                                                       const float* __restrict__ sigma, float sd, int weighting, const float* c_weight,
                                                       const float* __restrict__ g_loss, int batch, long per, float* __restrict__ df) {
  const long n = (long)batch * per;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int b = (int)(i / per);
    const Karras k = karras(sigma[b], sd, weighting, c_weight, b);
    const float t = (input[i] - k.c_skip * noised[i]) / k.c_out;
    df[i] = g_loss[b] * k.c_weight * 2.0f * (f[i] - t) / (float)per;
  }
}

unsigned grid_of(long n) { return (unsigned)std::min<long>((n + 255) / 256, 8192); }

}  // namespace
}  // namespace kd

using namespace kd;

namespace kd {
int launch_dropout_bits(unsigned* bits, long long n, const long long* key, unsigned long long site, unsigned threshold, hipStream_t s);  // dropout_f32.hip
}

static int wgrad(const char* what, const float* G, int g_mode, const float* A, int a_mode, int a_geglu, long long M, int N, int K, int gh, int gw, int ph,
                 int pw, int chan, const float* row_scale, const float* col_scale, int col_stride, int rows_per_sample, const float* alpha,
                 int accumulate, int arith, int chunk_rows, int nchunk, float* ws, float* dW, const unsigned* bits, float drop_scale, hipStream_t s) {
  if (arith < WG_EXACT || arith > WG_BF16) return fail(KD_EINVAL, "%s: arithmetic %d (0 exact, 1 split3, 2 bf16)", what, arith);
  if (!G || !A || !dW || !ws || M <= 0 || N <= 0 || K <= 0 || chunk_rows <= 0 || nchunk <= 0 || nchunk > 65535)
    return fail(KD_EINVAL, "%s: bad arguments", what);
  if ((long long)chunk_rows * nchunk < M) return fail(KD_EINVAL, "%s: %d chunks of %d rows do not cover %lld rows", what, nchunk, chunk_rows, M);
  if (g_mode < WG_PLAIN || g_mode > WG_PATCH_NCHW || a_mode < WG_PLAIN || a_mode > WG_PATCH_NCHW || (g_mode && a_mode))
    return fail(KD_EINVAL, "%s: bad gather modes %d / %d (one operand at most is gathered)", what, g_mode, a_mode);
  if (a_geglu && a_mode != WG_PLAIN) return fail(KD_EINVAL, "%s: the GEGLU prologue reads plain rows", what);
  if (bits && a_mode != WG_PLAIN) return fail(KD_EINVAL, "%s: the dropout mask applies to plain A rows", what);
  if (g_mode || a_mode) {
    if (gh <= 0 || gw <= 0 || ph <= 0 || pw <= 0 || chan <= 0 || M % ((long long)gh * gw))
      return fail(KD_EINVAL, "%s: bad gather geometry", what);
    if ((g_mode ? N : K) != ph * pw * chan) return fail(KD_EINVAL, "%s: gathered operand has %d columns, expected %d", what, g_mode ? N : K, ph * pw * chan);
  }
  if (col_scale && (rows_per_sample <= 0 || col_stride < 0)) return fail(KD_EINVAL, "%s: bad column scale layout", what);
  const auto aligned16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const int g_wide = arith == WG_BF16 && g_mode == WG_PLAIN && N % 4 == 0 && aligned16(G);
  const int a_wide = arith == WG_BF16 && a_mode == WG_PLAIN && K % 4 == 0 && aligned16(A) && (!col_scale || (aligned16(col_scale) && col_stride % 4 == 0));
  WgOperand go{G, g_mode, N, 0, nullptr, nullptr, 0, nullptr, 0.f, g_wide};
  WgOperand ao{A, a_mode, K, a_geglu, row_scale, col_scale, col_stride, bits, drop_scale, a_wide};
  WgGeom q{gh, gw, ph, pw, chan, rows_per_sample > 0 ? rows_per_sample : 1};
  {
    static const char* const names[3][2] = {{"wgrad_f32", "wgrad_drop_f32"}, {"wgrad_x3_f32", "wgrad_x3_drop_f32"}, {"wgrad_b16_f32", "wgrad_b16_drop_f32"}};
    LaunchScope prof(names[arith][bits != nullptr], 2.0 * (double)M * N * K, 4.0 * (double)M * (N + K), s);
    const int tile = arith == WG_BF16 ? BT : WT;
    const dim3 grid((unsigned)((N + tile - 1) / tile), (unsigned)((K + tile - 1) / tile), (unsigned)nchunk);
    if (bits) {
      if (arith == WG_BF16) hipLaunchKernelGGL(wgrad_b16_partial_kernel<true>, grid, dim3(256), 0, s, go, ao, q, (long)M, N, K, chunk_rows, ws);
      else if (arith == WG_SPLIT3) hipLaunchKernelGGL(wgrad_x3_partial_kernel<true>, grid, dim3(256), 0, s, go, ao, q, (long)M, N, K, chunk_rows, ws);
      else hipLaunchKernelGGL(wgrad_partial_kernel<true>, grid, dim3(256), 0, s, go, ao, q, (long)M, N, K, chunk_rows, ws);
    } else {
      if (arith == WG_BF16) hipLaunchKernelGGL(wgrad_b16_partial_kernel<false>, grid, dim3(256), 0, s, go, ao, q, (long)M, N, K, chunk_rows, ws);
      else if (arith == WG_SPLIT3) hipLaunchKernelGGL(wgrad_x3_partial_kernel<false>, grid, dim3(256), 0, s, go, ao, q, (long)M, N, K, chunk_rows, ws);
      else hipLaunchKernelGGL(wgrad_partial_kernel<false>, grid, dim3(256), 0, s, go, ao, q, (long)M, N, K, chunk_rows, ws);
    }
  }
  const int e = check_launch(what);
  if (e) return e;
  const long n = (long)N * K;
  LaunchScope prof("wgrad_reduce_f32", 0, (double)n * nchunk, s);
  hipLaunchKernelGGL(chunk_reduce_kernel, dim3(grid_of(n)), dim3(256), 0, s, ws, nchunk, n, alpha, accumulate, dW);
  return check_launch(what);
}

extern "C" int kd_wgrad_f32(const float* G, int g_mode, const float* A, int a_mode, int a_geglu, long long M, int N, int K, int gh, int gw, int ph,
                            int pw, int chan, const float* row_scale, const float* col_scale, int col_stride, int rows_per_sample,
                            const float* alpha, int accumulate, int split3, int chunk_rows, int nchunk, float* ws, float* dW, void* stream) {
  return wgrad("kd_wgrad_f32", G, g_mode, A, a_mode, a_geglu, M, N, K, gh, gw, ph, pw, chan, row_scale, col_scale, col_stride, rows_per_sample, alpha,
               accumulate, split3, chunk_rows, nchunk, ws, dW, nullptr, 0.f, (hipStream_t)stream);
}

extern "C" int kd_wgrad_drop_f32(const float* G, int g_mode, const float* A, int a_mode, int a_geglu, long long M, int N, int K, int gh, int gw,
                                 int ph, int pw, int chan, const float* row_scale, const float* col_scale, int col_stride, int rows_per_sample,
                                 const float* alpha, int accumulate, int split3, int chunk_rows, int nchunk, float* ws, float* dW,
                                 const long long* key, unsigned long long site, unsigned threshold, float scale, unsigned* bits, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (threshold == 0)          // nothing dropped: kd_wgrad_f32's kernels and bits
    return wgrad("kd_wgrad_drop_f32", G, g_mode, A, a_mode, a_geglu, M, N, K, gh, gw, ph, pw, chan, row_scale, col_scale, col_stride, rows_per_sample,
                 alpha, accumulate, split3, chunk_rows, nchunk, ws, dW, nullptr, 0.f, s);
  if (!key || !bits || a_mode != WG_PLAIN || M <= 0 || K <= 0) return fail(KD_EINVAL, "kd_wgrad_drop_f32: bad dropout arguments");
  const int e = launch_dropout_bits(bits, M * (long long)K, key, site, threshold, s);
  if (e) return e;
  return wgrad("kd_wgrad_drop_f32", G, g_mode, A, a_mode, a_geglu, M, N, K, gh, gw, ph, pw, chan, row_scale, col_scale, col_stride, rows_per_sample,
               alpha, accumulate, split3, chunk_rows, nchunk, ws, dW, bits, scale, s);
}

extern "C" int kd_row_rrms_f32(const float* x, float* rrms, long long rows, int d, float eps, void* stream) {
  if (!x || !rrms || rows <= 0 || d <= 0) return fail(KD_EINVAL, "kd_row_rrms_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("row_rrms_f32", 0, 2.0 * (double)rows * d, s);
  hipLaunchKernelGGL(row_rrms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rrms, (long)rows, d, eps);
  return check_launch("kd_row_rrms_f32");
}

extern "C" int kd_colsum_f32(const float* a, const float* b, const float* b2, const float* row_scale, long long rows, int cols, long long rows_per_seg,
                             int accumulate, float* ws, float* out, void* stream) {
  if (!a || !ws || !out || rows <= 0 || cols <= 0 || rows_per_seg <= 0 || rows % rows_per_seg || (b2 && !b))
    return fail(KD_EINVAL, "kd_colsum_f32: bad arguments");
  const long nseg = (long)(rows / rows_per_seg);
  const long nchunk = (long)((rows_per_seg + CS_ROWS - 1) / CS_ROWS);
  if (nseg > 65535 || nchunk > 65535) return fail(KD_EINVAL, "kd_colsum_f32: %ld segments of %ld chunks: too many", nseg, nchunk);
  hipStream_t s = (hipStream_t)stream;
  {
    LaunchScope prof("colsum_f32", 0, 3.0 * (double)rows * cols, s);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)((cols + 255) / 256), (unsigned)nchunk, (unsigned)nseg), dim3(256), 0, s, a, b, b2,
                       row_scale, (long)rows_per_seg, cols, (int)nchunk, ws);
  }
  const int e = check_launch("kd_colsum_f32");
  if (e) return e;
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3((unsigned)((nseg * cols + 255) / 256)), dim3(256), 0, s, ws, (int)nseg, (int)nchunk, cols,
                     accumulate, out);
  return check_launch("kd_colsum_f32 (reduce)");
}

extern "C" int kd_attn_scale_grad_f32(const float* colsum, const float* scale, int nh, int accumulate, float* out, void* stream) {
  if (!colsum || !scale || !out || nh <= 0) return fail(KD_EINVAL, "kd_attn_scale_grad_f32: bad arguments");
  hipLaunchKernelGGL(attn_scale_grad_kernel, dim3((unsigned)((nh + 63) / 64)), dim3(64), 0, (hipStream_t)stream, colsum, scale, nh, accumulate, out);
  return check_launch("kd_attn_scale_grad_f32");
}

extern "C" int kd_class_emb_grad_f32(const float* g, const long long* ids, int batch, int d, int n_cls, int accumulate, float* out, void* stream) {
  if (!g || !ids || !out || batch <= 0 || d <= 0 || n_cls <= 0) return fail(KD_EINVAL, "kd_class_emb_grad_f32: bad arguments");
  const long n = (long)n_cls * d;
  hipLaunchKernelGGL(class_emb_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, ids, batch, d, n_cls, accumulate,
                     out);
  return check_launch("kd_class_emb_grad_f32");
}

extern "C" int kd_loss_prep_f32(const float* input, const float* noise, const float* sigma, float sigma_data, float* noised, float* x_in, int batch,
                                long long per_sample, void* stream) {
  if (!input || !noise || !sigma || !noised || !x_in || batch <= 0 || per_sample <= 0) return fail(KD_EINVAL, "kd_loss_prep_f32: bad arguments");
  hipLaunchKernelGGL(loss_prep_kernel, dim3(grid_of((long)batch * per_sample)), dim3(256), 0, (hipStream_t)stream, input, noise, sigma, sigma_data,
                     noised, x_in, batch, (long)per_sample);
  return check_launch("kd_loss_prep_f32");
}

extern "C" int kd_loss_f32(const float* f, const float* input, const float* noised, const float* sigma, float sigma_data, int weighting,
                           const float* c_weight, float* losses, int batch, long long per_sample, void* stream) {
  if (!f || !input || !noised || !sigma || !losses || batch <= 0 || per_sample <= 0 || weighting < LW_KARRAS || weighting > LW_GIVEN ||
      (weighting == LW_GIVEN && !c_weight))
    return fail(KD_EINVAL, "kd_loss_f32: bad arguments");
  hipLaunchKernelGGL(loss_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, f, input, noised, sigma, sigma_data, weighting, c_weight,
                     (long)per_sample, losses);
  return check_launch("kd_loss_f32");
}

extern "C" int kd_loss_vjp_f32(const float* f, const float* input, const float* noised, const float* sigma, float sigma_data, int weighting,
                               const float* c_weight, const float* g_loss, float* g_f, int batch, long long per_sample, void* stream) {
  if (!f || !input || !noised || !sigma || !g_loss || !g_f || batch <= 0 || per_sample <= 0 || weighting < LW_KARRAS || weighting > LW_GIVEN ||
      (weighting == LW_GIVEN && !c_weight))
    return fail(KD_EINVAL, "kd_loss_vjp_f32: bad arguments");
  hipLaunchKernelGGL(loss_vjp_kernel, dim3(grid_of((long)batch * per_sample)), dim3(256), 0, (hipStream_t)stream, f, input, noised, sigma, sigma_data,
                     weighting, c_weight, g_loss, batch, (long)per_sample, g_f);
  return check_launch("kd_loss_vjp_f32");
}
