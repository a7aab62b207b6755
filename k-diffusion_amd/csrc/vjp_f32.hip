// Reverse-mode (vector-Jacobian) kernels of the HDiT denoiser, fp32 arithmetic (gfx950): the nonlinear pieces of the backward pass that
// takes a gradient on the denoiser's output back to its input (models/vjp.py).  Everything linear in the activations (projections, token
// merge / split, lerp, patch-in / -out, residual adds) runs its transpose on the existing GEMM kernels with transposed weights; only what is
// below needs a rule of its own:
//
//   kd_rmsnorm_vjp_f32       rms_norm / AdaRMSNorm (image_transformer_v2.py:98-103, :142-166): input gradient, scale held fixed
//   kd_geglu_vjp_f32         linear_geglu's gate (:89-95), erf-GELU (kd_geglu_vjp_drop_f32: with the hidden's dropout mask on g_y)
//   kd_qk_prep_vjp_f32       scale_for_cosine_sim (:106-121) + axial RoPE (:187-231), scale held fixed
//   kd_attn_*_vjp_f32        softmax attention: global (:383,:392), neighbourhood (:428), shifted window (:253-337)
//   kd_attn_global_drop(_vjp)_f32  global attention with dropout on the probabilities (the image_v1 U-Net's SelfAttention2d in training mode,
//                            k_diffusion/layers.py:181-200; include/kdiff_unet_drop.h): the same two passes under a DROP template flag
//   kd_precond_vjp_f32       the Karras preconditioning's per-sample scalings (k_diffusion/layers.py:70-74, :88-90) on a gradient
//
// Products are plain fp32 FMAs on the VALU.  Every reduction has a fixed shape and order (shuffle trees, fixed key / query sweeps): no
// atomics, bit-identical on repeat.
#include "kd_common.h"
#include "deriv_f32.h"
#include "philox.h"
#include "../../include/kdiff_unet_drop.h"

#include <cmath>

namespace kd {

namespace {

constexpr int VDH = 64;                 // head dim
constexpr float V_NEG_INF = -__builtin_huge_valf();

// ---- RMSNorm: one wave per row -------------------------------------------------------------------------------------
// y = s x r, r = rsqrt(mean(x^2) + eps)  =>  gx = s gy r - x r^3 mean(x s gy)  (+ g_add: the residual's pass-through gradient)
__global__ __launch_bounds__(256) void rmsnorm_vjp_kernel(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ scale,
                                                          int scale_stride, int rows_per_sample, const float* g_add, float* gx, int rows, int d,
                                                          float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                 // whole waves exit together
  const int nv = d >> 2;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + (long)row * d);
  const f32x4* gr = reinterpret_cast<const f32x4*>(gy + (long)row * d);
  const f32x4* sr = reinterpret_cast<const f32x4*>(scale + (long)(row / rows_per_sample) * scale_stride);
  float ss = 0.f, sg = 0.f;
  for (int i = lane; i < nv; i += 64) {
    const f32x4 a = xr[i], b = gr[i] * sr[i];
    ss += dot4(a, a);
    sg += dot4(a, b);
  }
  ss = wave_sum_xor(ss, 64);
  sg = wave_sum_xor(sg, 64);
  const float r = rsqrtf(ss / (float)d + eps);
  const float r3m = r * r * r * (sg / (float)d);
  const f32x4* ar = reinterpret_cast<const f32x4*>(g_add ? g_add + (long)row * d : nullptr);
  f32x4* outr = reinterpret_cast<f32x4*>(gx + (long)row * d);
  for (int i = lane; i < nv; i += 64) {
    f32x4 o = (gr[i] * sr[i]) * r - xr[i] * r3m;
    if (ar) o += ar[i];
    outr[i] = o;
  }
}

// ---- GEGLU: y = a * gelu(g)  =>  ga = gy gelu(g), gg = gy a gelu'(g) ------------------------------------------------------
__device__ __forceinline__ void geglu_vjp_elem(const float* __restrict__ h, float gyi, float* gh, long i, int d_ff) {
  const long row = i / d_ff;
  const int j = (int)(i - row * d_ff);
  const long ia = row * 2 * d_ff + j, ig = ia + d_ff;
  const float a = h[ia], g = h[ig];
  const float cdf = 0.5f * (1.0f + erff(g * 0.70710678118654752440f));
  const float dgelu = cdf + g * (0.39894228040143267794f * expf(-0.5f * g * g));
  gh[ia] = gyi * (g * cdf);
  gh[ig] = gyi * a * dgelu;
}

__global__ __launch_bounds__(256) void geglu_vjp_kernel(const float* __restrict__ h, const float* __restrict__ gy, float* gh, long n, int d_ff) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) geglu_vjp_elem(h, gy[i], gh, i, d_ff);
}

// the same with the dropout mask of the hidden activation on gy (dropout_f32.hip's contract): one Philox block per 4 elements per lane
__global__ __launch_bounds__(256) void geglu_vjp_drop_kernel(const float* __restrict__ h, const float* __restrict__ gy, float* gh, long n, int d_ff,
                                                             const long long* __restrict__ key_ptr, unsigned long long site, unsigned threshold,
                                                             float scale) {
  const unsigned long long key = (unsigned long long)key_ptr[0];
  const long quads = (n + 3) >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
    const Philox4 r = philox4x32_10(key, (unsigned long long)q, site);
    for (int k = 0; k < 4 && 4 * q + k < n; ++k) {
      const long i = 4 * q + k;
      geglu_vjp_elem(h, gy[i] * (philox_word(r, k) >= threshold ? scale : 0.0f), gh, i, d_ff);
    }
  }
}

// ---- q/k preparation: 16 lanes per 64-float row, lane c owns dims [4c, 4c+4) ---------------------------------------------
// p = R(c q rho), rho = rsqrt(|q|^2 + eps), c = sqrt(scale_h)  =>  u = R^T gp,  gq = c rho u - c rho^3 q (q . u).  v rows are left alone.
__global__ __launch_bounds__(256) void qk_prep_vjp_kernel(const float* __restrict__ qkv, float* gqkv, const float* scale_h, const float* cos_t,
                                                          const float* sin_t, long rows_total, int tokens_per_sample, int nh, float eps) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int c = threadIdx.x & 15;
  if (g >= rows_total) return;   // whole 16-lane groups exit together
  const int head = g % nh;
  const long r2 = g / nh;
  const int t = r2 & 1;
  const long tok = r2 >> 1;
  const long off = (tok * 3 + t) * (long)(nh * VDH) + head * VDH + 4 * c;
  const int tl = tok % tokens_per_sample;
  const float* csr = cos_t + ((long)tl * nh + head) * KD_ROT;
  const float* snr = sin_t + ((long)tl * nh + head) * KD_ROT;
  const f32x4 cs = *reinterpret_cast<const f32x4*>(csr + 4 * (c & 3));
  const f32x4 sn = *reinterpret_cast<const f32x4*>(snr + 4 * (c & 3));
  const f32x4 v = *reinterpret_cast<const f32x4*>(qkv + off);
  const f32x4 u = rope16(*reinterpret_cast<const f32x4*>(gqkv + off), c, cs, -sn);
  const float ss = row16_sum(dot4(v, v));
  const float su = row16_sum(dot4(v, u));
  const float cc = sqrtf(scale_h[head]);
  const float rho = rsqrtf(ss + eps);
  *reinterpret_cast<f32x4*>(gqkv + off) = u * (cc * rho) - v * (cc * rho * rho * rho * su);
}

// ---- attention: the flash-attention-2 decomposition on the key sets of the forward-mode kernels ----------------------------------
// With l_ij = q_i . k_j, P_ij = exp(l_ij - lse_i) over query i's key set, dP_ij = dO_i . v_j and D_i = dO_i . O_i = sum_j P_ij dP_ij:
//   dq_i = sum_j P_ij (dP_ij - D_i) k_j,   dk_j = sum_i P_ij (dP_ij - D_i) q_i,   dv_j = sum_i P_ij dO_i.
// Pass 1 (attn_vjp_q_kernel): a workgroup of 256 lanes serves 16 queries of one (sample, head), a 16-lane group per query, lane c owning
// dims [4c, 4c+4).  Keys (k, v) stream through LDS in chunks of VKC; a first sweep gives O, lse and D, a second sweep gives dq.
// Pass 2 (attn_vjp_kv_kernel): the same shape with 16 keys per workgroup over the queries that attend them, (q, dO, lse, D) streaming
// through LDS: all tokens (global), the key's own window (shifted window: the region predicate is symmetric), or the inverse
// neighbourhood (InvNaSet) of a 4x4 key tile.
constexpr int VKC = 32;                            // keys (pass 1) / queries (pass 2) per LDS chunk
constexpr int VJP_LDS_Q = VKC * 2 * VDH * 4;       // [VKC][k, v][64]: 16 KiB
constexpr int VJP_LDS_KV = VKC * (2 * VDH + 2) * 4;  // [VKC][q, dO][64] + lse[VKC] + D[VKC]

struct AttnVjpArgs {
  const float* qkv; const float* gout; float* gqkv; float* lse; float* dsum;
  int batch, nh, T, H, W, geo, shift;              // geo: window size (window) or kernel size (neighbourhood)
  int blocks_per_head;                             // query / key blocks per (sample, head)
  // probability dropout (the DROP instantiations only; include/kdiff_unet_drop.h, attention site): element ((b nh + h) T + i) T4 + j
  const long long* key; unsigned long long site; unsigned threshold; float scale; int T4;
  float* out;                                      // DROP_FWD: the attention output [batch, T, nh 64]
};

enum { DROP_NONE = 0, DROP_VJP = 1, DROP_FWD = 2 };

__device__ __forceinline__ unsigned row16_or(unsigned v) {
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROR8, 0xF, 0xF, true);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_ROR4, 0xF, 0xF, true);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_XOR2, 0xF, 0xF, true);
  v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, DPP_XOR1, 0xF, 0xF, true);
  return v;
}

// keep bits of the four mask elements 4 quad .. 4 quad + 3 of `site` (bit k: element 4 quad + k is kept)
__device__ __forceinline__ unsigned keep4(unsigned long long key, unsigned long long quad, unsigned long long site, unsigned threshold) {
  const Philox4 r = philox4x32_10(key, quad, site);
  return (r.x0 >= threshold ? 1u : 0u) | (r.x1 >= threshold ? 2u : 0u) | (r.x2 >= threshold ? 4u : 0u) | (r.x3 >= threshold ? 8u : 0u);
}

// Inverse neighbourhood along one axis: the queries i whose clamped window [start(i), start(i) + ks) holds key j.  start(i) =
// clamp(i - ks/2, 0, len - ks) is monotone in i, so the set is the interval [inv_lo(j), inv_hi(j)]; near a border it holds more than ks
// queries (every query whose window was clamped onto that border).
__device__ __forceinline__ int inv_lo(int j, int ks) { return j < ks ? 0 : j - ks / 2; }
__device__ __forceinline__ int inv_hi(int j, int len, int ks) { return j >= len - ks ? len - 1 : j + ks / 2; }

struct InvNaSet {
  int qtok; bool qactive;       // (the key of this lane group: named as KeySet's query side, which pass 2 reads)
  int kr, kc;                   // its row, column
  int n_keys;                   // queries in the set
  int base_r, base_c, span_c;   // their rectangle: origin and width

  template <class A>
  __device__ void init(const A& a, int kb, int g) {
    const int ks = a.geo, tw = (a.W + 3) / 4;
    const int th = kb / tw, tc = kb % tw;
    const int r0 = th * 4, c0 = tc * 4;
    const int r = r0 + (g >> 2), c = c0 + (g & 3);
    qactive = r < a.H && c < a.W;
    kr = min(r, a.H - 1);
    kc = min(c, a.W - 1);
    qtok = kr * a.W + kc;
    base_r = inv_lo(r0, ks);
    base_c = inv_lo(c0, ks);
    const int r_hi = inv_hi(min(r0 + 3, a.H - 1), a.H, ks) + 1, c_hi = inv_hi(min(c0 + 3, a.W - 1), a.W, ks) + 1;
    span_c = c_hi - base_c;
    n_keys = (r_hi - base_r) * span_c;
  }
  template <class A>
  __device__ int key_tok(const A& a, int j) const { return (base_r + j / span_c) * a.W + base_c + j % span_c; }
  template <class A>
  __device__ bool allowed(const A& a, int j) const {
    if (j >= n_keys) return false;
    const int sr = na_start(base_r + j / span_c, a.H, a.geo), sc = na_start(base_c + j % span_c, a.W, a.geo);
    return kr >= sr && kr < sr + a.geo && kc >= sc && kc < sc + a.geo;
  }
};

template <int MODE> struct QuerySetOf { using type = KeySet<MODE>; };
template <> struct QuerySetOf<KS_NA> { using type = InvNaSet; };

template <int MODE, int DROP = DROP_NONE>
__global__ __launch_bounds__(256) void attn_vjp_q_kernel(AttnVjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];       // [VKC][2: k, v][64]
  const int g = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int qb = blockIdx.x % a.blocks_per_head;
  const int bh = blockIdx.x / a.blocks_per_head;
  const int head = bh % a.nh, b = bh / a.nh;
  const long row_stride = 3L * a.nh * VDH, o_stride = (long)a.nh * VDH;
  const float* base = a.qkv + (long)b * a.T * row_stride + head * VDH;
  KeySet<MODE> ks;
  ks.init(a, qb, g);
  const f32x4 q = *reinterpret_cast<const f32x4*>(base + ks.qtok * row_stride + 4 * c);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 go = zero;
  if (DROP != DROP_FWD) go = *reinterpret_cast<const f32x4*>(a.gout + ((long)b * a.T + ks.qtok) * o_stride + head * VDH + 4 * c);
  // DROP: the keep bits of this query's keys j0 .. j0 + 31 (bit kk: key j0 + kk): lane c < 8 draws the 4 keys of quad c, the row ORs them
  unsigned long long mkey = 0, mrow = 0;
  if (DROP) {
    mkey = (unsigned long long)a.key[0];
    mrow = (((unsigned long long)b * a.nh + head) * a.T + ks.qtok) * (unsigned long long)a.T4;
  }
  auto keep_bits = [&](int j0) -> unsigned {
    unsigned bits = 0;
    if (c < VKC / 4) bits = keep4(mkey, (mrow + j0 + 4 * c) >> 2, a.site, a.threshold) << (4 * c);
    return row16_or(bits);
  };
  auto load_chunk = [&](int j0) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < VKC * 32; idx += 256) {
      const int kk = idx >> 5, part = (idx >> 4) & 1, c4 = idx & 15;
      f32x4 val = zero;
      if (j0 + kk < ks.n_keys) {
        const long tok = ks.key_tok(a, j0 + kk);
        val = *reinterpret_cast<const f32x4*>(base + tok * row_stride + (1 + part) * (long)(a.nh * VDH) + 4 * c4);
      }
      *reinterpret_cast<f32x4*>(lds + (kk * 2 + part) * VDH + 4 * c4) = val;
    }
    __syncthreads();
  };
  // sweep 1: O, lse, D (every group of a workgroup shares n_keys and the key -> token map)
  f32x4 A = zero;
  float Z = 0.f, m = V_NEG_INF;
  for (int j0 = 0; j0 < ks.n_keys; j0 += VKC) {
    load_chunk(j0);
    const unsigned keep = DROP ? keep_bits(j0) : 0u;
    float L[VKC];
    float mc = V_NEG_INF;
#pragma unroll
    for (int kk = 0; kk < VKC; ++kk) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(lds + (kk * 2 + 0) * VDH + 4 * c);
      const float l = row16_sum(dot4(q, kf));
      L[kk] = ks.allowed(a, j0 + kk) ? l : V_NEG_INF;
      mc = fmaxf(mc, L[kk]);
    }
    const float mn = fmaxf(m, mc);
    if (mn != V_NEG_INF) {               // (uniform over the query's 16 lanes)
      const float alpha = m == V_NEG_INF ? 0.f : expf(m - mn);
      Z *= alpha; A = A * alpha;
#pragma unroll
      for (int kk = 0; kk < VKC; ++kk) {
        const float e = L[kk] == V_NEG_INF ? 0.f : expf(L[kk] - mn);
        Z += e;
        if (DROP)
          A += ((keep >> kk & 1u) ? e * a.scale : 0.f) * *reinterpret_cast<const f32x4*>(lds + (kk * 2 + 1) * VDH + 4 * c);
        else
          A += e * *reinterpret_cast<const f32x4*>(lds + (kk * 2 + 1) * VDH + 4 * c);
      }
      m = mn;
    }
  }
  if (DROP == DROP_FWD) {
    if (ks.qactive) *reinterpret_cast<f32x4*>(a.out + ((long)b * a.T + ks.qtok) * o_stride + head * VDH + 4 * c) = A * (1.0f / Z);
    return;
  }
  const float lse = m + logf(Z);
  const float D = row16_sum(dot4(go, A * (1.0f / Z)));
  // sweep 2: dq
  f32x4 dq = zero;
  for (int j0 = 0; j0 < ks.n_keys; j0 += VKC) {
    load_chunk(j0);
    const unsigned keep = DROP ? keep_bits(j0) : 0u;
#pragma unroll 8
    for (int kk = 0; kk < VKC; ++kk) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(lds + (kk * 2 + 0) * VDH + 4 * c);
      const f32x4 vf = *reinterpret_cast<const f32x4*>(lds + (kk * 2 + 1) * VDH + 4 * c);
      const float l = row16_sum(dot4(q, kf));
      float dp = row16_sum(dot4(go, vf));
      if (DROP) dp = (keep >> kk & 1u) ? dp * a.scale : 0.f;
      const float p = ks.allowed(a, j0 + kk) ? expf(l - lse) : 0.f;
      dq += (p * (dp - D)) * kf;
    }
  }
  if (ks.qactive) {
    *reinterpret_cast<f32x4*>(a.gqkv + ((long)b * a.T + ks.qtok) * row_stride + head * VDH + 4 * c) = dq;
    if (c == 0) {
      const long s = ((long)b * a.nh + head) * a.T + ks.qtok;
      a.lse[s] = lse;
      a.dsum[s] = D;
    }
  }
}

template <int MODE, bool DROP = false>
__global__ __launch_bounds__(256) void attn_vjp_kv_kernel(AttnVjpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];       // [VKC][2: q, dO][64], then lse[VKC], D[VKC]
  float* lds_lse = lds + VKC * 2 * VDH;
  float* lds_d = lds_lse + VKC;
  const int g = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int kb = blockIdx.x % a.blocks_per_head;
  const int bh = blockIdx.x / a.blocks_per_head;
  const int head = bh % a.nh, b = bh / a.nh;
  const long row_stride = 3L * a.nh * VDH, o_stride = (long)a.nh * VDH;
  const float* base = a.qkv + (long)b * a.T * row_stride + head * VDH;
  const float* gbase = a.gout + (long)b * a.T * o_stride + head * VDH;
  const long st_base = ((long)b * a.nh + head) * a.T;
  typename QuerySetOf<MODE>::type qs;              // read from the key's side: qtok / qactive are this group's KEY
  qs.init(a, kb, g);
  const f32x4 k = *reinterpret_cast<const f32x4*>(base + qs.qtok * row_stride + o_stride + 4 * c);
  const f32x4 v = *reinterpret_cast<const f32x4*>(base + qs.qtok * row_stride + 2 * o_stride + 4 * c);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 dk = zero, dv = zero;
  // DROP: the keep bits of this KEY under the queries i0 .. i0 + 31 (bit ii: query i0 + ii): lane c draws the key's quad at the queries
  // i0 + c and i0 + c + 16 and takes the key's word, the row ORs them
  unsigned long long mkey = 0, mhead = 0;
  if (DROP) {
    mkey = (unsigned long long)a.key[0];
    mhead = ((unsigned long long)b * a.nh + head) * a.T;
  }
  for (int i0 = 0; i0 < qs.n_keys; i0 += VKC) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < VKC * 32; idx += 256) {
      const int ii = idx >> 5, part = (idx >> 4) & 1, c4 = idx & 15;
      f32x4 val = zero;
      if (i0 + ii < qs.n_keys) {
        const long tok = qs.key_tok(a, i0 + ii);
        val = *reinterpret_cast<const f32x4*>(part ? gbase + tok * o_stride + 4 * c4 : base + tok * row_stride + 4 * c4);
      }
      *reinterpret_cast<f32x4*>(lds + (ii * 2 + part) * VDH + 4 * c4) = val;
    }
    if (threadIdx.x < VKC) {
      const int ii = threadIdx.x;
      const bool in = i0 + ii < qs.n_keys;
      const long tok = in ? qs.key_tok(a, i0 + ii) : 0;
      lds_lse[ii] = in ? a.lse[st_base + tok] : 0.f;
      lds_d[ii] = in ? a.dsum[st_base + tok] : 0.f;
    }
    __syncthreads();
    unsigned keep = 0;
    if (DROP) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int ii = c + 16 * half;
        const unsigned long long e = (mhead + (unsigned long long)min(i0 + ii, a.T - 1)) * (unsigned long long)a.T4 + qs.qtok;
        keep |= (keep4(mkey, e >> 2, a.site, a.threshold) >> (qs.qtok & 3) & 1u) << ii;
      }
      keep = row16_or(keep);
    }
#pragma unroll 8
    for (int ii = 0; ii < VKC; ++ii) {
      const f32x4 qf = *reinterpret_cast<const f32x4*>(lds + (ii * 2 + 0) * VDH + 4 * c);
      const f32x4 gof = *reinterpret_cast<const f32x4*>(lds + (ii * 2 + 1) * VDH + 4 * c);
      const float l = row16_sum(dot4(qf, k));
      float dp = row16_sum(dot4(gof, v));
      const float p = qs.allowed(a, i0 + ii) ? expf(l - lds_lse[ii]) : 0.f;
      if (DROP) {
        const float mk = (keep >> ii & 1u) ? a.scale : 0.f;
        dp *= mk;
        dv += (p * mk) * gof;
      } else {
        dv += p * gof;
      }
      dk += (p * (dp - lds_d[ii])) * qf;
    }
  }
  if (qs.qactive) {
    float* dst = a.gqkv + ((long)b * a.T + qs.qtok) * row_stride + head * VDH + 4 * c;
    *reinterpret_cast<f32x4*>(dst + o_stride) = dk;
    *reinterpret_cast<f32x4*>(dst + 2 * o_stride) = dv;
  }
}

// ---- Karras preconditioning on a gradient: y = coef_g(sigma_b) g + coef_h(sigma_b) h ----------------------------------------
__device__ __forceinline__ float karras_coef(int which, float sg, float sd) {
  const float var = sg * sg + sd * sd;
  switch (which) {
    case KD_PC_SKIP: return sd * sd / var;
    case KD_PC_OUT: return sg * sd / sqrtf(var);
    case KD_PC_IN: return 1.0f / sqrtf(var);
    default: return 1.0f;
  }
}

__global__ __launch_bounds__(256) void precond_vjp_kernel(const float* __restrict__ g, int g_coef, const float* __restrict__ h, int h_coef,
                                                          const float* __restrict__ sigma, float sd, float* y, int batch, long per_sample) {
  const long n = (long)batch * per_sample;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float sg = sigma[i / per_sample];
    const float v = g[i] * karras_coef(g_coef, sg, sd);
    y[i] = h ? v + h[i] * karras_coef(h_coef, sg, sd) : v;
  }
}

static unsigned vjp_grid(long n) {
  long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

template <int MODE, bool DROP = false>
int launch_attn_vjp(const AttnVjpArgs& a, const char* name, hipStream_t s) {
  const long blocks = (long)a.batch * a.nh * a.blocks_per_head;
  if (blocks > 0x7FFFFFFFL) return fail(KD_EINVAL, "%s: grid too large", name);
  {
    LaunchScope prof(name, 0, 12.0 * (double)a.batch * a.T * a.nh * VDH, s);
    hipLaunchKernelGGL((attn_vjp_q_kernel<MODE, DROP ? DROP_VJP : DROP_NONE>), dim3((unsigned)blocks), dim3(256), VJP_LDS_Q, s, a);
    if (int e = check_launch(name)) return e;
  }
  LaunchScope prof(name, 0, 16.0 * (double)a.batch * a.T * a.nh * VDH, s);
  hipLaunchKernelGGL((attn_vjp_kv_kernel<MODE, DROP>), dim3((unsigned)blocks), dim3(256), VJP_LDS_KV, s, a);
  return check_launch(name);
}

}  // namespace
}  // namespace kd

using namespace kd;

extern "C" int kd_rmsnorm_vjp_f32(const float* x, const float* g_y, const float* scale, int scale_stride, int rows_per_sample, const float* g_add,
                                  float* g_x, int rows, int d, float eps, void* stream) {
  if (!x || !g_y || !scale || !g_x || rows <= 0 || d <= 0 || rows_per_sample <= 0 || scale_stride < 0)
    return fail(KD_EINVAL, "kd_rmsnorm_vjp_f32: bad arguments");
  if (d % 4 || scale_stride % 4) return fail(KD_EINVAL, "kd_rmsnorm_vjp_f32: d (%d) and scale_stride (%d) must be multiples of 4", d, scale_stride);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("rmsnorm_vjp_f32", 0, 16.0 * rows * d, s);
  hipLaunchKernelGGL(rmsnorm_vjp_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, g_y, scale, scale_stride, rows_per_sample, g_add,
                     g_x, rows, d, eps);
  return check_launch("kd_rmsnorm_vjp_f32");
}

extern "C" int kd_geglu_vjp_f32(const float* h, const float* g_y, float* g_h, int rows, int d_ff, void* stream) {
  if (!h || !g_y || !g_h || rows <= 0 || d_ff <= 0) return fail(KD_EINVAL, "kd_geglu_vjp_f32: bad arguments");
  const long n = (long)rows * d_ff;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("geglu_vjp_f32", 0, 20.0 * n, s);
  hipLaunchKernelGGL(geglu_vjp_kernel, dim3(vjp_grid(n)), dim3(256), 0, s, h, g_y, g_h, n, d_ff);
  return check_launch("kd_geglu_vjp_f32");
}

extern "C" int kd_geglu_vjp_drop_f32(const float* h, const float* g_y, float* g_h, int rows, int d_ff, const long long* key, unsigned long long site,
                                     unsigned threshold, float scale, void* stream) {
  if (!h || !g_y || !g_h || !key || rows <= 0 || d_ff <= 0) return fail(KD_EINVAL, "kd_geglu_vjp_drop_f32: bad arguments");
  const long n = (long)rows * d_ff;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("geglu_vjp_drop_f32", 0, 20.0 * n, s);
  hipLaunchKernelGGL(geglu_vjp_drop_kernel, dim3(vjp_grid((n + 3) >> 2)), dim3(256), 0, s, h, g_y, g_h, n, d_ff, key, site, threshold, scale);
  return check_launch("kd_geglu_vjp_drop_f32");
}

extern "C" int kd_qk_prep_vjp_f32(const float* qkv, float* g_qkv, const float* scale_h, const float* cos_t, const float* sin_t, int batch,
                                  int tokens_per_sample, int nh, float eps, void* stream) {
  if (!qkv || !g_qkv || !scale_h || !cos_t || !sin_t || batch <= 0 || tokens_per_sample <= 0 || nh <= 0)
    return fail(KD_EINVAL, "kd_qk_prep_vjp_f32: bad arguments");
  const long rows = (long)batch * tokens_per_sample * 2 * nh;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("qk_prep_vjp_f32", 0, (double)rows * VDH * 12, s);
  hipLaunchKernelGGL(qk_prep_vjp_kernel, dim3((unsigned)((rows * 16 + 255) / 256)), dim3(256), 0, s, qkv, g_qkv, scale_h, cos_t, sin_t, rows,
                     tokens_per_sample, nh, eps);
  return check_launch("kd_qk_prep_vjp_f32");
}

extern "C" int kd_attn_global_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int T, int nh,
                                      void* stream) {
  if (!qkv || !g_out || !g_qkv || !lse || !dsum || batch <= 0 || T <= 0 || nh <= 0) return fail(KD_EINVAL, "kd_attn_global_vjp_f32: bad arguments");
  AttnVjpArgs a{qkv, g_out, g_qkv, lse, dsum, batch, nh, T, 1, T, 0, 0, (T + 15) / 16};
  return launch_attn_vjp<KS_GLOBAL>(a, "attn_global_vjp_f32", (hipStream_t)stream);
}

// the U-Net's attention with dropout on the probabilities (include/kdiff_unet_drop.h): the forward is the q pass's first sweep
extern "C" int kd_attn_global_drop_f32(const float* qkv, float* out, int batch, int T, int nh, const long long* key, unsigned long long site,
                                       unsigned threshold, float scale, void* stream) {
  if (!qkv || !out || !key || batch <= 0 || T <= 0 || nh <= 0) return fail(KD_EINVAL, "kd_attn_global_drop_f32: bad arguments");
  AttnVjpArgs a{qkv, nullptr, nullptr, nullptr, nullptr, batch, nh, T, 1, T, 0, 0, (T + 15) / 16, key, site, threshold, scale, 4 * ((T + 3) / 4), out};
  const long blocks = (long)batch * nh * a.blocks_per_head;
  if (blocks > 0x7FFFFFFFL) return fail(KD_EINVAL, "kd_attn_global_drop_f32: grid too large");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("attn_global_drop_f32", 0, 16.0 * (double)batch * T * nh * VDH, s);
  hipLaunchKernelGGL((attn_vjp_q_kernel<KS_GLOBAL, DROP_FWD>), dim3((unsigned)blocks), dim3(256), VJP_LDS_Q, s, a);
  return check_launch("kd_attn_global_drop_f32");
}

extern "C" int kd_attn_global_drop_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int T, int nh,
                                           const long long* key, unsigned long long site, unsigned threshold, float scale, void* stream) {
  if (!qkv || !g_out || !g_qkv || !lse || !dsum || !key || batch <= 0 || T <= 0 || nh <= 0)
    return fail(KD_EINVAL, "kd_attn_global_drop_vjp_f32: bad arguments");
  AttnVjpArgs a{qkv, g_out, g_qkv, lse, dsum, batch, nh, T, 1, T, 0, 0, (T + 15) / 16, key, site, threshold, scale, 4 * ((T + 3) / 4), nullptr};
  return launch_attn_vjp<KS_GLOBAL, true>(a, "attn_global_drop_vjp_f32", (hipStream_t)stream);
}

extern "C" int kd_attn_window_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int H, int W, int nh,
                                      int ws, int shift, void* stream) {
  if (!qkv || !g_out || !g_qkv || !lse || !dsum || batch <= 0 || H <= 0 || W <= 0 || nh <= 0)
    return fail(KD_EINVAL, "kd_attn_window_vjp_f32: bad arguments");
  if (const int rc = geo::window_check("kd_attn_window_vjp_f32", H, W, ws, shift)) return rc;
  AttnVjpArgs a{qkv, g_out, g_qkv, lse, dsum, batch, nh, H * W, H, W, ws, shift, (H / ws) * (W / ws) * (ws * ws / 16)};
  return launch_attn_vjp<KS_WINDOW>(a, "attn_window_vjp_f32", (hipStream_t)stream);
}

extern "C" int kd_attn_na2d_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int H, int W, int nh,
                                    int ks, void* stream) {
  if (!qkv || !g_out || !g_qkv || !lse || !dsum || batch <= 0 || nh <= 0) return fail(KD_EINVAL, "kd_attn_na2d_vjp_f32: bad arguments");
  if (const int rc = geo::na_check("kd_attn_na2d_vjp_f32", ks, H, W)) return rc;
  AttnVjpArgs a{qkv, g_out, g_qkv, lse, dsum, batch, nh, H * W, H, W, ks, 0, ((H + 3) / 4) * ((W + 3) / 4)};
  return launch_attn_vjp<KS_NA>(a, "attn_na2d_vjp_f32", (hipStream_t)stream);
}

extern "C" int kd_precond_vjp_f32(const float* g, int g_coef, const float* h, int h_coef, const float* sigma, float sigma_data, float* y, int batch,
                                  long long per_sample, void* stream) {
  if (!g || !sigma || !y || batch <= 0 || per_sample <= 0 || g_coef < KD_PC_ONE || g_coef > KD_PC_IN || h_coef < KD_PC_ONE || h_coef > KD_PC_IN)
    return fail(KD_EINVAL, "kd_precond_vjp_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("precond_vjp_f32", 0, 12.0 * batch * (double)per_sample, s);
  hipLaunchKernelGGL(precond_vjp_kernel, dim3(vjp_grid((long)batch * per_sample)), dim3(256), 0, s, g, g_coef, h, h_coef, sigma, sigma_data, y,
                     batch, (long)per_sample);
  return check_launch("kd_precond_vjp_f32");
}
