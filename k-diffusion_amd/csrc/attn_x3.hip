// Attention cores of the fp32-parity ("split3") mode in the round-2 bf16 shape (attn_bf16.hip), gfx950.
//
//   neighbourhood attention, kernel sizes 3 .. 13 (natten na2d, image_transformer_v2.py:399-410,428; 7 is what the shipped configs use,
//   3 / 5 / 9 run the same kernel with other constants, 11 / 13 a densely packed patch), for qkv STORED SPLIT by the qkv projection
//   (KdGemm.qkv_packed, prep = 2 of kd_attn_na2d_f32): every 4 head dims are 16 bytes [hi: 4 x bf16][lo: 4 x bf16], q and k already
//   cosine-sim-scaled and rotated.  Every product is hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32 accumulation (per-product
//   error <= ~2^-15), scores / softmax / accumulators fp32, out fp32.
//
// What changed against attn_f32.hip's neighbourhood core (round 1: halo rows through registers, split / transposed by VALU, 16 ds_write
// per key pair, 82.8 us per level-0 launch = 3.2 TB/s of algorithmic traffic):
//   * halo rows go HBM / L2 -> LDS by global_load_lds as they are stored (256-byte rows, 4 rows per wave-instruction), the 16-byte chunk
//     index XOR-swizzled on the SOURCE side: no staging VALU, no ds_write pass;
//   * a K fragment (8 head dims, hi and lo) is two ds_read_b128 of adjacent chunks -- [hi4 | lo4][hi4 | lo4] regrouped in registers;
//   * V^T fragments come out of the row-major V image through ds_read_b64_tr_b16: an 8-byte piece of a row is exactly the hi (or lo)
//     quad of 4 head dims, which is what the transposing read moves;
//   * K and V share ONE 78 KiB image (two workgroups per CU): V is requested right behind the score MFMAs' barrier and lands behind the
//     mask / softmax / probability split;
//   * mask by v_min3 against per-lane column / row validity, exp2 softmax (attn_bf16.hip).
#include "x3_common.h"
#include "attn_x3_core.h"

namespace kd {
namespace x3 { extern unsigned long long* g_clk; }      // gemm_x3.hip (kd_prof_clock_buffer)
namespace x3a {

template <int KS>
__global__ __launch_bounds__(256, NaGeo<KS>::LDS <= 80 * 1024 ? 2 : 1) void attn_na2d_x3_kernel(const NArgs a) {
  extern __shared__ __attribute__((aligned(16))) char img[];
  const int tid = threadIdx.x, lane = tid & 63, h2 = lane >> 5;
  const auto warm = code_warm_begin<10240>((int)blockIdx.x < a.warm && tid < 64);
  const x3::WgStamp wgs = x3::wg_stamp_begin(a.clk);
  KD_NA_TILE(a, KD_XCD_CHUNK())      // tx, ty, head, b (attn_geo.h); XCD-aware order: neighbouring tiles (overlapping halos) run on ONE L2
  na2d_x3_tile<KS>(img, a, tid, b, head, ty, tx, [&]() { code_warm_end(warm); }, [&](bool q_ok, int q_tok, float l, const f32x16 (&O)[2]) {
    if (!q_ok) return;
    const float inv = 1.0f / l;
    float* op = a.out + ((size_t)b * (a.H * a.W) + q_tok) * (a.nh * DH) + head * DH;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st16(op + e * 32 + 8 * g + 4 * h2, f32x4(f32x4{O[e][4 * g], O[e][4 * g + 1], O[e][4 * g + 2], O[e][4 * g + 3]} * inv));
  });
  x3::wg_stamp_end(wgs);
}

// ---- neighbourhood core, kernel sizes 11 and 13 (no shipped config uses them: the form that covers the reference's interface,
// image_transformer_v2.py:399-410, not a tuned one) ----------------------------------------------------------------------------------------
// The 4 x 8 query block of a wave now needs a patch of (4 + KS - 1) rows x (8 + KS - 1) = 18 / 20 columns: no power-of-two width any
// more, so the patch is walked DENSELY as in attn_bf16.hip's form of these sizes: local key kl = 20 r + c (columns padded to 20, a
// multiple of 4: the 4-key groups of the V^T reads never straddle two patch rows), tiles of 32 keys, every key's (row, column) by constant
// division, validity per accumulator register from those.  One workgroup per CU (127 / 150 KiB of halo image: K and V still share it).
template <int KS> using NaWide = geo::NaWideX3<KS>;      // attn_geo.h
static_assert(NaWide<11>::LDS == 130048 && NaWide<13>::LDS == 153600 && NaWide<13>::LDS <= 160 * 1024, "image sizes");

template <int KS>
__global__ __launch_bounds__(256, 1) void attn_na2d_x3_wide_kernel(const NArgs a) {
  using G = NaWide<KS>;
  constexpr int HC = G::HC, NKT = G::NKT, ROWS = G::ROWS;
  extern __shared__ __attribute__((aligned(16))) char img[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, h2 = lane >> 5;
  const auto warm = code_warm_begin<16384>((int)blockIdx.x < a.warm && tid < 64);
  const int wy_ = wid >> 1, wx_ = wid & 1;
  KD_NA_TILE(a, blockIdx.x)      // tx, ty, head, b
  const int T = a.H * a.W;
  const size_t row_bytes = (size_t)3 * a.nh * DH * 4;
  const char* base = reinterpret_cast<const char*>(a.qkv) + (size_t)b * T * row_bytes + head * (DH * 4);
  KD_NA_HALO(G, a, ty, tx)      // ty0, tx0, hy0, hx0
  // image row 4 pc + (lane >> 4) = halo position (row / HC, row % HC); rows past the halo (the slack) take a real token: outside every window
  auto stage = [&](int part_bytes) {
    for (int pc = wid; pc < ROWS / 4; pc += 4) {
      const int row = 4 * pc + (lane >> 4);
      const int ky = min(hy0 + row / HC, a.H - 1), kx = min(hx0 + row % HC, a.W - 1);
      const char* src = base + (size_t)(unsigned)((ky * a.W + kx) * (int)row_bytes + (((lane & 15) ^ rsw(row)) << 4));
      glds16(src + part_bytes, img + pc * 1024);
    }
  };
  stage(a.nh * DH * 4);                                  // K
  KD_NA_QUERY(a, ty0, tx0, wy_, wx_, l31)      // q_ok, qy, qx, q_tok
  bf16x8 qh[4], ql[4];
  {
    const u32x4* qp = reinterpret_cast<const u32x4*>(base + (size_t)q_tok * row_bytes + 32 * h2);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const u32x4 c0 = qp[4 * st], c1 = qp[4 * st + 1];
      qh[st] = __builtin_bit_cast(bf16x8, u32x4{c0[0], c0[1], c1[0], c1[1]});
      ql[st] = __builtin_bit_cast(bf16x8, u32x4{c0[2], c0[3], c1[2], c1[3]});
    }
  }
  KD_NA_PATCH(G, a, ty0, tx0, hy0, hx0, wy_, wx_, qy, qx)      // korg, r0, c0
  auto img_row = [&](int kl) -> int { return min(geo::na_wide_row<G>(korg, kl), ROWS - 1); };     // image row of local key kl
  KD_WAIT_VM(0);
  code_warm_end(warm);
  KD_BARRIER();

  // ---- S^T = K Q^T, tile by tile: local key 32 t + l31 ----------------------------------------------------------------------------------
  f32x16 S[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) S[t][i] = 0.f;
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const int kr = img_row(32 * t + l31);
    const int ka = kr * ROWB + (((2 * h2) ^ rsw(kr)) << 4);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const u32x4 c0 = *reinterpret_cast<const u32x4*>(img + (ka ^ (st << 6)));
      const u32x4 c1 = *reinterpret_cast<const u32x4*>(img + (ka ^ (st << 6) ^ 16));
      const bf16x8 kh = __builtin_bit_cast(bf16x8, u32x4{c0[0], c0[1], c1[0], c1[1]});
      const bf16x8 kl = __builtin_bit_cast(bf16x8, u32x4{c0[2], c0[3], c1[2], c1[3]});
      S[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qh[st], S[t], 0, 0, 0);
      S[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, ql[st], S[t], 0, 0, 0);
      S[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qh[st], S[t], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  KD_BARRIER();                                          // every wave has its K fragments: the image is free
  stage(2 * a.nh * DH * 4);                              // V, in flight behind the softmax

  // ---- window mask (accumulator register i of tile t: local key 32 t + (i & 3) + 8 (i >> 2) + 4 h2) + softmax ----------------------------
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kl = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h2;
      S[t][i] = KD_NA_WIDE_VALID(G, kl, r0, c0) ? S[t][i] : -INFINITY;
    }
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
  KD_WAIT_VM(0);
  KD_BARRIER();                                          // V image complete

  // ---- O^T = V^T P^T: k-slots of lane-half h2 at step (t, u) are local keys 32 t + 16 u + 4 h2 + {0..3} and the same + 8 -- two 4-key
  // groups, each inside one patch row; the probabilities are split step by step --------------------------------------------------------------
  f32x16 O[2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int i = 0; i < 16; ++i) O[e][i] = 0.f;
  const int vsub = (lane & 15) >> 2;
  const int vc = (lane & 3) + 4 * ((lane >> 4) & 1);
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      u32x4 phi, plo;
      x3::split8(f32x4{S[t][8 * u], S[t][8 * u + 1], S[t][8 * u + 2], S[t][8 * u + 3]},
                 f32x4{S[t][8 * u + 4], S[t][8 * u + 5], S[t][8 * u + 6], S[t][8 * u + 7]}, phi, plo);
      const bf16x8 ph = __builtin_bit_cast(bf16x8, phi), pl = __builtin_bit_cast(bf16x8, plo);
      const int k0 = 32 * t + 16 * u + 4 * h2;
      const int ra = min(img_row(k0) + vsub, ROWS - 1), rb = min(img_row(k0 + 8) + vsub, ROWS - 1);
      bf16x8 vh[2], vl[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int a0 = ra * ROWB + (((vc + 8 * e) ^ rsw(ra)) << 4), a1 = rb * ROWB + (((vc + 8 * e) ^ rsw(rb)) << 4);
        const u32x2 h0 = tr_read(img, a0), h1 = tr_read(img, a1), l0 = tr_read(img, a0 + 8), l1 = tr_read(img, a1 + 8);
        vh[e] = __builtin_bit_cast(bf16x8, u32x4{h0[0], h0[1], h1[0], h1[1]});
        vl[e] = __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], l1[0], l1[1]});
      }
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl[0], ph, O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl[1], ph, O[1], 0, 0, 0);
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[0], pl, O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[1], pl, O[1], 0, 0, 0);
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[0], ph, O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[1], ph, O[1], 0, 0, 0);
    }
  if (q_ok) {
    const float inv = 1.0f / l;
    float* op = a.out + ((size_t)b * T + q_tok) * (a.nh * DH) + head * DH;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st16(op + e * 32 + 8 * g + 4 * h2, f32x4(f32x4{O[e][4 * g], O[e][4 * g + 1], O[e][4 * g + 2], O[e][4 * g + 3]} * inv));
  }
}

// ---- global attention, T = 32 NT keys (64, 128, 256) -----------------------------------------------------------------------------------------
// SDPA / flash-attn of the global level (image_transformer_v2.py:383,392) on the same operand scheme: one workgroup per (sample, head,
// block of 32 QW queries), QW = min(4, NT) waves; ALL keys of the (sample, head) go through one [T][256 B] image, K first, then V (64 KiB at
// T = 256: two workgroups per CU -- the round-1 core ran one 8-wave workgroup per CU, its halo staging through registers).  A wave owns
// 32 queries and the whole score row (NT tiles, no online softmax); the probabilities are split tile by tile inside the PV loop.
// (One 8-wave workgroup per (sample, head) with K AND V images requested together -- one memory latency instead of two -- was measured
// slower, 26.1 vs 21.2 us: with one workgroup per CU nothing overlaps that latency, and the 8-wave form spills.)
struct GArgs {
  const float* qkv; float* out;
  int batch, T, nh;
  int warm;
  unsigned long long* clk;
};

template <int NT>
__global__ __launch_bounds__((NT < 4 ? NT : 4) * 64, 2) void attn_global_x3_kernel(const GArgs a) {
  constexpr int QW = NT < 4 ? NT : 4, T = 32 * NT, QB = NT / QW;      // query blocks per (sample, head)
  extern __shared__ __attribute__((aligned(16))) char img[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, h2 = lane >> 5;
  const auto warm = code_warm_begin<10240>((int)blockIdx.x < a.warm && tid < 64);
  const x3::WgStamp wgs = x3::wg_stamp_begin(a.clk);
  int r = KD_XCD_CHUNK();      // XCD-aware order: the query blocks of one (sample, head) -- same K, V -- run on ONE L2
  const int qb = r % QB; r /= QB;
  const int head = r % a.nh, b = r / a.nh;
  const size_t row_bytes = (size_t)3 * a.nh * DH * 4;
  const char* base = reinterpret_cast<const char*>(a.qkv) + (size_t)b * T * row_bytes + head * (DH * 4);
  auto stage = [&](int part_bytes) {
    for (int pc = wid; pc < T / 4; pc += QW) {
      const int row = 4 * pc + (lane >> 4);
      glds16(base + (size_t)row * row_bytes + part_bytes + (((lane & 15) ^ rsw(row)) << 4), img + pc * 1024);
    }
  };
  stage(a.nh * DH * 4);                                  // K
  const int q_tok = 32 * (QW * qb + wid) + l31;
  bf16x8 qh[4], ql[4];
  {
    const u32x4* qp = reinterpret_cast<const u32x4*>(base + (size_t)q_tok * row_bytes + 32 * h2);
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const u32x4 c0 = qp[4 * st], c1 = qp[4 * st + 1];
      qh[st] = __builtin_bit_cast(bf16x8, u32x4{c0[0], c0[1], c1[0], c1[1]});
      ql[st] = __builtin_bit_cast(bf16x8, u32x4{c0[2], c0[3], c1[2], c1[3]});
    }
  }
  KD_WAIT_VM(0);
  code_warm_end(warm);
  KD_BARRIER();

  f32x16 S[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) S[t][i] = 0.f;
  const int ka = l31 * ROWB + (((2 * h2) ^ rsw(l31)) << 4);      // key 32 t + l31: + t * 32 * ROWB (32 rows on: the same swizzle word)
#pragma unroll
  for (int st = 0; st < 4; ++st) {
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += 4) {                        // four tiles' fragments at a time (registers)
      constexpr int TB = NT < 4 ? NT : 4;
      bf16x8 kh[TB], kl[TB];
#pragma unroll
      for (int t = 0; t < TB; ++t) {
        const char* kp = img + (t0 + t) * 32 * ROWB + (ka ^ (st << 6));
        const u32x4 c0 = *reinterpret_cast<const u32x4*>(kp);
        const u32x4 c1 = *reinterpret_cast<const u32x4*>(img + (t0 + t) * 32 * ROWB + (ka ^ (st << 6) ^ 16));
        kh[t] = __builtin_bit_cast(bf16x8, u32x4{c0[0], c0[1], c1[0], c1[1]});
        kl[t] = __builtin_bit_cast(bf16x8, u32x4{c0[2], c0[3], c1[2], c1[3]});
      }
#pragma unroll
      for (int t = 0; t < TB; ++t) S[t0 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl[t], qh[st], S[t0 + t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < TB; ++t) S[t0 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh[t], ql[st], S[t0 + t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < TB; ++t) S[t0 + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh[t], qh[st], S[t0 + t], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  KD_BARRIER();                                          // every wave has its K fragments: the image is free
  stage(2 * a.nh * DH * 4);                              // V, in flight behind the softmax

  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; i += 2) m = max3f(m, S[t][i], S[t][i + 1]);
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l;
  {
    constexpr float LOG2E = 1.4426950408889634f;
    const f32x2 mb = {-m * LOG2E, -m * LOG2E};
    f32x2 l2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t)
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
  KD_WAIT_VM(0);
  KD_BARRIER();                                          // V image complete

  f32x16 O[2];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int i = 0; i < 16; ++i) O[e][i] = 0.f;
  const int vr0 = 4 * h2 + ((lane & 15) >> 2);
  const int vc = (lane & 3) + 4 * ((lane >> 4) & 1);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // k-slots of step (t, u): keys 32 t + 16 u + 4 h2 + {0..3} and + 8
      const int vr = vr0 + 32 * t + 16 * u;
      const int va = vr * ROWB + ((vc ^ rsw(vr)) << 4);
      u32x4 phi, plo;
      x3::split8(f32x4{S[t][8 * u], S[t][8 * u + 1], S[t][8 * u + 2], S[t][8 * u + 3]},
                 f32x4{S[t][8 * u + 4], S[t][8 * u + 5], S[t][8 * u + 6], S[t][8 * u + 7]}, phi, plo);
      const bf16x8 ph = __builtin_bit_cast(bf16x8, phi), pl = __builtin_bit_cast(bf16x8, plo);
      bf16x8 vh[2], vl[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int a0 = va ^ (e << 7), a1 = (a0 ^ 32) + 8 * ROWB;
        const u32x2 h0 = tr_read(img, a0), h1 = tr_read(img, a1), l0 = tr_read(img, a0 + 8), l1 = tr_read(img, a1 + 8);
        vh[e] = __builtin_bit_cast(bf16x8, u32x4{h0[0], h0[1], h1[0], h1[1]});
        vl[e] = __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], l1[0], l1[1]});
      }
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl[0], ph, O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl[1], ph, O[1], 0, 0, 0);
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[0], pl, O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[1], pl, O[1], 0, 0, 0);
      O[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[0], ph, O[0], 0, 0, 0);
      O[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh[1], ph, O[1], 0, 0, 0);
    }
  {
    const float inv = 1.0f / l;
    float* op = a.out + ((size_t)b * T + q_tok) * (a.nh * DH) + head * DH;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st16(op + e * 32 + 8 * g + 4 * h2, f32x4(f32x4{O[e][4 * g], O[e][4 * g + 1], O[e][4 * g + 2], O[e][4 * g + 3]} * inv));
  }
  x3::wg_stamp_end(wgs);
}

template <int NT>
static int launch_global(const GArgs& a, hipStream_t s) {
  constexpr int QW = NT < 4 ? NT : 4, T = 32 * NT, lds = T * ROWB;
  const long nb = (long)a.batch * a.nh * (NT / QW);
  LaunchScope prof("attn_global_x3", 4.0 * (double)a.batch * a.nh * T * T * DH, 16.0 * (double)a.batch * T * a.nh * DH, s);
  launch<attn_global_x3_kernel<NT>>(dim3((unsigned)nb), dim3(QW * 64), lds, s, a);
  return check_launch("kd_attn_global_f32(x3)");
}

}  // namespace x3a

// Called by kd_attn_global_f32 (attn_f32.hip) for prep == 2, KD_PREC_SPLIT3, T = 64 / 128 / 256.  Returns 1 if not taken.
int attn_global_x3_try(const float* qkv, float* out, int batch, int T, int nh, hipStream_t s, int* rc) {
  using namespace x3a;
  if (!opt(KD_OPT_attn_x3) || (T != 64 && T != 128 && T != 256)) return 1;
  GArgs a{qkv, out, batch, T, nh, code_warm(), x3::g_clk};
  *rc = T == 256 ? launch_global<8>(a, s) : (T == 128 ? launch_global<4>(a, s) : launch_global<2>(a, s));
  return 0;
}

template <int KS, bool WIDE>
static int launch_na(const x3a::NArgs& a, hipStream_t s) {
  using namespace x3a;
  constexpr int lds = WIDE ? NaWide<(WIDE ? KS : 11)>::LDS : NaGeo<(WIDE ? 7 : KS)>::LDS;
  const long nb = geo::na_tiles(a.batch, a.nh, a.H, a.W);
  const ProfName nm = KS == 7 ? ProfName("attn_na2d_x3", "attn_na2d_x3 %dx%d nh=%d", a.H, a.W, a.nh)
                              : ProfName("attn_na2d_x3", "attn_na2d_x3 k%d %dx%d nh=%d", KS, a.H, a.W, a.nh);
  LaunchScope prof(nm, 4.0 * a.batch * (double)a.H * a.W * a.nh * DH * KS * KS, 16.0 * a.batch * (double)a.H * a.W * a.nh * DH, s);
  if constexpr (WIDE) launch<attn_na2d_x3_wide_kernel<KS>>(dim3((unsigned)nb), dim3(256), lds, s, a);
  else launch<attn_na2d_x3_kernel<KS>>(dim3((unsigned)nb), dim3(256), lds, s, a);
  return check_launch("kd_attn_na2d_f32(x3)");
}

// Called by kd_attn_na2d_f32 (attn_f32.hip) for prep == 2 (operands stored split), kernel sizes 3 .. 13 (odd).  Returns 1 if not taken.
int attn_na2d_x3_try(const float* qkv, float* out, int batch, int H, int W, int nh, int ks, hipStream_t s, int* rc) {
  using namespace x3a;
  if (!opt(KD_OPT_attn_x3)) return 1;
  NArgs a{qkv, out, batch, H, W, nh, code_warm(), x3::g_clk};
  switch (ks) {
    case 3: *rc = launch_na<3, false>(a, s); return 0;
    case 5: *rc = launch_na<5, false>(a, s); return 0;
    case 7: *rc = launch_na<7, false>(a, s); return 0;
    case 9: *rc = launch_na<9, false>(a, s); return 0;
    case 11: *rc = launch_na<11, true>(a, s); return 0;
    case 13: *rc = launch_na<13, true>(a, s); return 0;
    default: return 1;
  }
}

}  // namespace kd

KD_TEXT_PAD(attn_x3)      // last function of this code object: kd_common.h, code warm-up
