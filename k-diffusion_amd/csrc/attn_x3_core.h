// The neighbourhood-attention core of the fp32-parity ("split3") mode for ONE 8 x 16 query tile of one (sample, head), as a device
// function: attn_x3.hip wraps it into a kernel of its own (one workgroup per tile and head), attn_ffn_x3.hip runs it for both heads of a
// tile in front of the fused out projection + feed-forward block.  See attn_x3.hip for what the core does and why.
#pragma once
#include "x3_common.h"
#include "attn_geo.h"

namespace kd {
namespace x3a {


using b16::bf16x8;
using b16::u32x2;
using b16::u32x4;

constexpr int DH = 64;
using geo::NA_TH;
using geo::NA_TW;
constexpr int ROWB = 256;                                    // bytes of an image row: 64 head dims as 16 chunks [hi4 | lo4]
// Image sizes of kernel size KS (3 .. 9), attn_geo.h: rows of 256 bytes, 4 per LDS-DMA instruction, ONE image for K, then V.
// KS = 7: 79 872 B, two workgroups per CU (3, 5 too; 9: one)
template <int KS> using NaGeo = geo::NaGeoX3<KS>;
static_assert(NaGeo<3>::LDS == 48128 && NaGeo<5>::LDS == 62464 && NaGeo<7>::LDS == 79872 && NaGeo<9>::LDS == 98304, "image sizes");

struct NArgs {
  const float* qkv; float* out;
  int batch, H, W, nh;
  int warm;
  unsigned long long* clk;       // kd_prof_clock_buffer: per-workgroup entry / exit stamps (x3_common.h: wg_stamp_begin)
};

using b16::glds16;
using b16::max3f;
using b16::min3f;
using b16::s16x4;

// chunk c (0..15) of an image row sits at slot c ^ rsw(r), r = the row's index in the global core and in the 11 / 13 neighbourhood form, its
// halo COLUMN in the neighbourhood kernel (sizes 3 .. 9).  rsw swaps the two 2-bit fields of r & 15: 16 consecutive rows (columns) take 16
// different slots for one chunk (the ds_read_b128 of a K fragment: 16 lanes, 16 rows), and FOUR consecutive ones differ in slot bits
// 2-3, so the 4 rows x 4 chunks of a ds_read_b64_tr_b16 group land in 16 different slots.  rsw(r + 8) = rsw(r) ^ 2.
// (Keys past the halo's last column -- a patch may poke 1 - 2 keys over -- then read another chunk of a real row: finite values, always
// masked.)
__device__ __forceinline__ int rsw(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

__device__ __forceinline__ u32x2 tr_read(const char* img, int addr) {
  return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(img + addr)));
}

// Tile (ty, tx) of (sample b, head), thread `tid` of the 256: K and V through the image `img` (NaGeo<KS>::LDS bytes), scores, softmax, O^T = V^T P^T.  `mid()` runs
// once behind the first vector-memory wait (code warm-up), `sink(q_ok, q_tok, l, O)` takes the lane's unnormalised output (its query's
// features 32 e + 8 g + 4 h2 + 0..3 in O[e][4 g ..]) and the softmax denominator.  The image may be reused once every wave has left.
template <int KS, class Mid, class Sink>
__device__ __forceinline__ void na2d_x3_tile(char* img, const NArgs& a, int tid, int b, int head, int ty, int tx, Mid&& mid, Sink&& sink) {
  using G = NaGeo<KS>;
  constexpr int HC = G::HC, NKT = G::NKT, ROWS = G::ROWS;
  const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, h2 = lane >> 5;
  const int wy_ = wid >> 1, wx_ = wid & 1;
  const int T = a.H * a.W;
  const size_t row_bytes = (size_t)3 * a.nh * DH * 4;
  const char* base = reinterpret_cast<const char*>(a.qkv) + (size_t)b * T * row_bytes + head * (DH * 4);
  KD_NA_HALO(G, a, ty, tx)      // ty0, tx0, hy0, hx0 (attn_geo.h)

  // ---- halo rows -> image: image row 4 pc + (lane >> 4) = halo position (y, x), 16 rows per round of the 4 waves.  Rows past the halo's
  // last key and out-of-image positions (images smaller than the halo) take a real token: they lie outside every window.  The byte offsets of
  // this lane's pieces are computed ONCE (the K pass) and kept for the V pass: the same rows, `nh * 256` bytes further ------------------------------
  constexpr int NPC = (ROWS / 4 + 3) / 4;                // staging rounds of a wave
  unsigned soff[NPC];
  {
    int row = 4 * wid + (lane >> 4);
    int y = row / HC, x = row % HC;
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int ky = min(hy0 + y, a.H - 1), kx = min(hx0 + x, a.W - 1);
      soff[i] = (unsigned)((ky * a.W + kx) * (int)row_bytes + (((lane & 15) ^ rsw(x)) << 4));
      x += 16;
      if (x >= HC) { x -= HC; ++y; }
    }
  }
  auto stage = [&](int part_bytes) {
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int pc = wid + 4 * i;
      if (pc < ROWS / 4) glds16(base + (size_t)soff[i] + part_bytes, img + pc * 1024);
    }
  };
  stage(a.nh * DH * 4);                                  // K
  // ---- this lane's query: B fragments of the 4 k-steps (head dims 16 st + 8 h2 .. + 7: chunks 4 st + 2 h2, + 1) --------------------------
  KD_NA_QUERY(a, ty0, tx0, wy_, wx_, l31)      // q_ok, qy, qx, q_tok
  // Q operands per k-step: a stored chunk is [hi4 | lo4] of 4 head dims.  A K chunk goes into the MFMA AS IT IS READ (k-slots hi0..3, lo0..3 of
  // its 4 dims) against qa = [qhi0..3, qhi0..3] of the same dims: K_hi Q_hi + K_lo Q_hi of those dims in one instruction, no regrouping of the
  // K registers; the third term K_hi Q_lo takes the hi quads of both chunks (the only regrouped fragment: 4 moves per tile and step instead
  // of 8) against ql = [qlo of chunk 0, qlo of chunk 1].
  bf16x8 qa[4][2], ql[4];
  {
    const u32x4* qp = reinterpret_cast<const u32x4*>(base + (size_t)q_tok * row_bytes + 32 * h2);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const u32x4 c0 = qp[4 * st], c1 = qp[4 * st + 1];
      qa[st][0] = __builtin_bit_cast(bf16x8, u32x4{c0[0], c0[1], c0[0], c0[1]});
      qa[st][1] = __builtin_bit_cast(bf16x8, u32x4{c1[0], c1[1], c1[0], c1[1]});
      ql[st] = __builtin_bit_cast(bf16x8, u32x4{c0[2], c0[3], c1[2], c1[3]});
    }
  }
  KD_NA_PATCH(G, a, ty0, tx0, hy0, hx0, wy_, wx_, qy, qx)      // col_lo, korg, r0, c0: this wave's patch, the lane's window inside it
  float colv[8], rowv[2 * NKT];
  KD_NA_VALID_WORDS(KS, 2 * NKT, r0, c0, h2, colv, rowv)
  KD_WAIT_VM(0);
  mid();
  KD_BARRIER();

  // ---- S^T = K Q^T over the wave's key tiles: tile t, local key 32 t + i = patch row 2 t + (i >> 4), column i & 15 -------------------
  f32x16 S[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) S[t][i] = 0.f;
  // (round 4: the chunk swizzle of an image row is a function of its halo COLUMN, not of its row index: a lane's column is the same in
  // every patch row, so its fragment addresses differ from tile to tile by a compile-time constant -- immediate offsets of the LDS reads
  // instead of ~250 address instructions per wave)
  // The XOR part of an address (chunk pair of the k-step: bits 6 - 7, second chunk of the pair: bit 4) touches only bits below 8 and the tile
  // stride is a multiple of 256: (ka0 + t * stride) ^ m == (ka0 ^ m) + t * stride, so ONE base register per (k-step, chunk) serves every tile.
  const int kr0 = KD_NA_K_ROW0(G, korg, l31);
  const int ka0 = kr0 * ROWB + (((2 * h2) ^ rsw(col_lo + (l31 & 15))) << 4);      // chunk 2 h2 of the row; chunk + 1: ^ 16; step st: ^ (st << 6)
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    bf16x8 kc0[NKT], kc1[NKT], kh[NKT];
    const char* k0p = img + (ka0 ^ (st << 6));
    const char* k1p = img + (ka0 ^ (st << 6) ^ 16);
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const u32x4 c0 = *reinterpret_cast<const u32x4*>(k0p + t * (2 * HC * ROWB));
      const u32x4 c1 = *reinterpret_cast<const u32x4*>(k1p + t * (2 * HC * ROWB));
      kc0[t] = __builtin_bit_cast(bf16x8, c0);
      kc1[t] = __builtin_bit_cast(bf16x8, c1);
      kh[t] = __builtin_bit_cast(bf16x8, u32x4{c0[0], c0[1], c1[0], c1[1]});
    }
    // term-major: consecutive MFMAs go to different key tiles
#pragma unroll
    for (int t = 0; t < NKT; ++t) S[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kc0[t], qa[st][0], S[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NKT; ++t) S[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kc1[t], qa[st][1], S[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < NKT; ++t) S[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh[t], ql[st], S[t], 0, 0, 0);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  KD_BARRIER();                                          // every wave has its K fragments: the image is free
  stage(2 * a.nh * DH * 4);                              // V, in flight behind the softmax

  // ---- window mask + softmax ------------------------------------------------------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) S[t][i] = min3f(S[t][i], colv[i & 7], rowv[2 * t + (i >> 3)]);
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int i = 0; i < 16; i += 2) m = max3f(m, S[t][i], S[t][i + 1]);
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l;
  {
    constexpr float LOG2E = 1.4426950408889634f;
    const f32x2 mb = {-m * LOG2E, -m * LOG2E};
    f32x2 l2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        const f32x2 x = __builtin_elementwise_fma(f32x2{S[t][i], S[t][i + 1]}, f32x2{LOG2E, LOG2E}, mb);
        const f32x2 pv = {__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)};
        S[t][i] = pv.x;
        S[t][i + 1] = pv.y;
        l2 += pv;
      }
    l = l2.x + l2.y;
  }
  l += __shfl_xor(l, 32, 64);
  // probabilities -> hi / lo B fragments: step (t, u) = accumulator registers 8 u .. 8 u + 7 of tile t (k-slots: patch row 2 t + u,
  // columns 4 h2 + {0..3} and + 8)
  bf16x8 ph[NKT][2], pl[NKT][2];
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      u32x4 hi, lo;
      x3::split8(f32x4{S[t][8 * u], S[t][8 * u + 1], S[t][8 * u + 2], S[t][8 * u + 3]},
                 f32x4{S[t][8 * u + 4], S[t][8 * u + 5], S[t][8 * u + 6], S[t][8 * u + 7]}, hi, lo);
      ph[t][u] = __builtin_bit_cast(bf16x8, hi);
      pl[t][u] = __builtin_bit_cast(bf16x8, lo);
    }
  KD_WAIT_VM(0);
  KD_BARRIER();                                          // V image complete

  // ---- O^T = V^T P^T.  V^T fragment of step (t, u), feature block e: rows vr .. vr + 3 and vr + 8 .. + 11 of the image, the lane group's
  // 8-byte pieces [hi4] (or + 8: [lo4]) of chunks (lane & 3) + 4 ((lane >> 4) & 1) + 8 e, transposed by the read itself ---------------------
  f32x16 O[2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int i = 0; i < 16; ++i) O[e][i] = 0.f;
  const int vr0 = geo::na_v_row0(korg, h2, (lane & 15) >> 2);
  const int vc = (lane & 3) + 4 * ((lane >> 4) & 1);
  const int va0 = vr0 * ROWB + ((vc ^ rsw(col_lo + 4 * h2 + ((lane & 15) >> 2))) << 4);
  // four base addresses (feature block e, rows / rows + 8): block e = 1: ^ 128; rows + 8: (^ 32) + 8 rows; the step (t, u) and the lo quad (+ 8)
  // are immediate offsets (the same bits-below-8 argument as for the K fragments)
  const int vb[2][2] = {{va0, (va0 ^ 32) + 8 * ROWB}, {va0 ^ 128, ((va0 ^ 128) ^ 32) + 8 * ROWB}};
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      constexpr int step = HC * ROWB;
      bf16x8 vh[2], vl[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int a0 = vb[e][0] + (2 * t + u) * step, a1 = vb[e][1] + (2 * t + u) * step;
        const u32x2 h0 = tr_read(img, a0), h1 = tr_read(img, a1), l0 = tr_read(img, a0 + 8), l1 = tr_read(img, a1 + 8);
        vh[e] = __builtin_bit_cast(bf16x8, u32x4{h0[0], h0[1], h1[0], h1[1]});
        vl[e] = __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], l1[0], l1[1]});
      }
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl[0], ph[t][u], O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl[1], ph[t][u], O[1], 0, 0, 0);
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[0], pl[t][u], O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[1], pl[t][u], O[1], 0, 0, 0);
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[0], ph[t][u], O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[1], ph[t][u], O[1], 0, 0, 0);
    }

  sink(q_ok, q_tok, l, O);
}

}  // namespace x3a
}  // namespace kd
