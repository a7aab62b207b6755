// Forward-mode (tangent) kernels of the HDiT denoiser, fp32 arithmetic (gfx950): the nonlinear pieces of a DUAL pass, in which the
// primal x and its tangent xd run side by side, plus the per-sample reductions and the dopri5 vector arithmetic of log_likelihood
// (k_diffusion/sampling.py:280-301).  Everything linear in the activations (projections, token merge / split, lerp, patch-in / -out,
// residual adds) runs its tangent on the existing GEMM kernels; only what is below needs a rule of its own:
//
//   kd_rmsnorm_jvp_f32       rms_norm / AdaRMSNorm (image_transformer_v2.py:98-103, :142-166)
//   kd_geglu_jvp_f32         linear_geglu's gate (:89-95), erf-GELU
//   kd_qk_prep_jvp_f32       scale_for_cosine_sim (:106-121) + axial RoPE (:187-231)
//   kd_attn_*_jvp_f32        softmax attention: global (:383,:392), neighbourhood (:428), shifted window (:253-337)
//   kd_ll_div_f32            to_d (sampling.py:46) and the divergence term v . (v - J_D v) / sigma per sample
//   kd_rk_combine_f32 / kd_rk_error_f32 / kd_gauss_logp_f32   dopri5 stage sums, error norm, Gaussian prior
//
// Products are plain fp32 FMAs on the VALU (no bf16 splits): the tangent carries fp32 rounding only.  Every reduction has a fixed
// shape and order (shuffle trees, one workgroup per sample or a fixed grid of partials): no atomics, bit-identical on repeat.
#include "kd_common.h"
#include "deriv_f32.h"

#include <cmath>

namespace kd {

namespace {

constexpr int JDH = 64;                 // head dim
constexpr float NEG_INF = -__builtin_huge_valf();

// ---- RMSNorm: one wave per row -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmsnorm_jvp_kernel(const float* __restrict__ x, const float* __restrict__ xd, const float* __restrict__ scale,
                                                          int scale_stride, int rows_per_sample, float* y, float* yd, int rows, int d, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;                 // whole waves exit together
  const int nv = d >> 2;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + (long)row * d);
  const f32x4* xdr = reinterpret_cast<const f32x4*>(xd + (long)row * d);
  float ss = 0.f, sd = 0.f;
  for (int i = lane; i < nv; i += 64) {
    const f32x4 a = xr[i], b = xdr[i];
    ss += dot4(a, a);
    sd += dot4(a, b);
  }
  ss = wave_sum_xor(ss, 64);
  sd = wave_sum_xor(sd, 64);
  const float r = rsqrtf(ss / (float)d + eps);
  const float mdot = sd / (float)d;
  const float r3m = r * r * r * mdot;
  const f32x4* sr = reinterpret_cast<const f32x4*>(scale + (long)(row / rows_per_sample) * scale_stride);
  f32x4* yr = reinterpret_cast<f32x4*>(y + (long)row * d);
  f32x4* ydr = reinterpret_cast<f32x4*>(yd + (long)row * d);
  for (int i = lane; i < nv; i += 64) {
    const f32x4 a = xr[i], b = xdr[i], s = sr[i];
    yr[i] = a * (s * r);
    ydr[i] = s * (b * r - a * r3m);
  }
}

// ---- GEGLU: value * gelu(gate) -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geglu_jvp_kernel(const float* __restrict__ h, const float* __restrict__ hd, float* y, float* yd,
                                                        long n, int d_ff) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long row = i / d_ff;
    const int j = (int)(i - row * d_ff);
    const long ia = row * 2 * d_ff + j, ig = ia + d_ff;
    const float a = h[ia], g = h[ig], ad = hd[ia], gd = hd[ig];
    const float cdf = 0.5f * (1.0f + erff(g * 0.70710678118654752440f));
    const float gelu = g * cdf;
    const float dgelu = cdf + g * (0.39894228040143267794f * expf(-0.5f * g * g));
    y[i] = a * gelu;
    yd[i] = ad * gelu + a * dgelu * gd;
  }
}

// ---- q/k preparation: 16 lanes per 64-float row, lane c owns dims [4c, 4c+4) (rope16: deriv_f32.h) -------------------------
__global__ __launch_bounds__(256) void qk_prep_jvp_kernel(float* qkv, float* qkvd, const float* scale_h, const float* cos_t, const float* sin_t,
                                                          long rows_total, int tokens_per_sample, int nh, float eps) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int c = threadIdx.x & 15;
  if (g >= rows_total) return;   // whole 16-lane groups exit together
  const int head = g % nh;
  const long r2 = g / nh;
  const int t = r2 & 1;
  const long tok = r2 >> 1;
  const long off = (tok * 3 + t) * (long)(nh * JDH) + head * JDH + 4 * c;
  const int tl = tok % tokens_per_sample;
  const float* csr = cos_t + ((long)tl * nh + head) * KD_ROT;
  const float* snr = sin_t + ((long)tl * nh + head) * KD_ROT;
  const f32x4 cs = *reinterpret_cast<const f32x4*>(csr + 4 * (c & 3));
  const f32x4 sn = *reinterpret_cast<const f32x4*>(snr + 4 * (c & 3));
  f32x4 v = *reinterpret_cast<const f32x4*>(qkv + off);
  f32x4 vd = *reinterpret_cast<const f32x4*>(qkvd + off);
  const float ss = row16_sum(dot4(v, v));
  const float sd = row16_sum(dot4(v, vd));
  const float cc = sqrtf(scale_h[head]);
  const float rho = rsqrtf(ss + eps);
  const float f = cc * rho;
  const float fd = cc * rho * rho * rho * sd;
  const f32x4 q = v * f;
  const f32x4 qd = vd * f - v * fd;
  *reinterpret_cast<f32x4*>(qkv + off) = rope16(q, c, cs, sn);
  *reinterpret_cast<f32x4*>(qkvd + off) = rope16(qd, c, cs, sn);
}

// ---- attention: one template, three key-set policies (KeySet: deriv_f32.h) ----------------------------------------------
// A workgroup of 256 lanes serves 16 queries of one (sample, head) -- a 16-lane group per query, lane c owning dims [4c, 4c+4) of q, qd
// and of the accumulators -- over a key set they share: all T tokens (global), the window (shifted window; the reference's region mask is
// a per-pair predicate), or the union of the queries' clamped neighbourhoods for a 4x4 query tile (neighbourhood; the predicate keeps each
// query's own ks x ks window).  Keys stream through LDS in chunks of JKC (k, kd, v, vd: 1 KiB per key); per chunk and query the logits
// l_j = q.k_j and their tangents ld_j = qd.k_j + q.kd_j are kept in registers, the running maximum moves once, and
//   Z = sum e_j,  S = sum e_j ld_j,  A = sum e_j v_j,  B = sum e_j ld_j v_j,  C = sum e_j vd_j      (e_j = exp(l_j - m))
// give o = A / Z and od = (B + C) / Z - (S / Z) o.
constexpr int JKC = 32;                          // keys per LDS chunk
constexpr int JVP_LDS = JKC * 4 * JDH * 4;       // 32 KiB

struct AttnJvpArgs {
  const float* qkv; const float* qkvd; float* out; float* outd;
  int batch, nh, T, H, W, geo, shift;            // geo: window size (window) or kernel size (neighbourhood)
  int blocks_per_head;                           // query blocks per (sample, head)
};

template <int MODE>
__global__ __launch_bounds__(256) void attn_jvp_kernel(AttnJvpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];       // [JKC][4: k, kd, v, vd][64]
  const int g = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int qb = blockIdx.x % a.blocks_per_head;
  const int bh = blockIdx.x / a.blocks_per_head;
  const int head = bh % a.nh, b = bh / a.nh;
  const long row_stride = 3L * a.nh * JDH;
  const float* base = a.qkv + (long)b * a.T * row_stride + head * JDH;
  const float* based = a.qkvd + (long)b * a.T * row_stride + head * JDH;
  KeySet<MODE> ks;
  ks.init(a, qb, g);
  const f32x4 q = *reinterpret_cast<const f32x4*>(base + ks.qtok * row_stride + 4 * c);
  const f32x4 qd = *reinterpret_cast<const f32x4*>(based + ks.qtok * row_stride + 4 * c);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 A = zero, B = zero, Cv = zero;
  float Z = 0.f, S = 0.f, m = NEG_INF;
  // every group of a workgroup shares n_keys and the key -> token map (only the per-query predicate differs)
  for (int j0 = 0; j0 < ks.n_keys; j0 += JKC) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < JKC * 64; idx += 256) {
      const int kk = idx >> 6, part = (idx >> 4) & 3, c4 = idx & 15;
      f32x4 val = zero;
      if (j0 + kk < ks.n_keys) {
        const long tok = ks.key_tok(a, j0 + kk);
        const float* src = (part & 1) ? based : base;
        val = *reinterpret_cast<const f32x4*>(src + tok * row_stride + (1 + (part >> 1)) * (long)(a.nh * JDH) + 4 * c4);
      }
      *reinterpret_cast<f32x4*>(lds + (kk * 4 + part) * JDH + 4 * c4) = val;
    }
    __syncthreads();
    float L[JKC], LD[JKC];
    float mc = NEG_INF;
#pragma unroll
    for (int kk = 0; kk < JKC; ++kk) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(lds + (kk * 4 + 0) * JDH + 4 * c);
      const f32x4 kdf = *reinterpret_cast<const f32x4*>(lds + (kk * 4 + 1) * JDH + 4 * c);
      const float l = row16_sum(dot4(q, kf));
      LD[kk] = row16_sum(dot4(qd, kf) + dot4(q, kdf));
      L[kk] = ks.allowed(a, j0 + kk) ? l : NEG_INF;
      mc = fmaxf(mc, L[kk]);
    }
    const float mn = fmaxf(m, mc);
    if (mn != NEG_INF) {                 // (uniform over the query's 16 lanes)
      const float alpha = m == NEG_INF ? 0.f : expf(m - mn);
      Z *= alpha; S *= alpha; A = A * alpha; B = B * alpha; Cv = Cv * alpha;
#pragma unroll
      for (int kk = 0; kk < JKC; ++kk) {
        const float e = L[kk] == NEG_INF ? 0.f : expf(L[kk] - mn);
        const f32x4 vf = *reinterpret_cast<const f32x4*>(lds + (kk * 4 + 2) * JDH + 4 * c);
        const f32x4 vdf = *reinterpret_cast<const f32x4*>(lds + (kk * 4 + 3) * JDH + 4 * c);
        const float eld = e * LD[kk];
        Z += e;
        S += eld;
        A += e * vf;
        B += eld * vf;
        Cv += e * vdf;
      }
      m = mn;
    }
  }
  if (ks.qactive) {
    const float iz = 1.0f / Z;
    const f32x4 o = A * iz;
    const f32x4 od = (B + Cv) * iz - (S * iz) * o;
    const long o_off = ((long)b * a.T + ks.qtok) * (a.nh * JDH) + head * JDH + 4 * c;
    *reinterpret_cast<f32x4*>(a.out + o_off) = o;
    *reinterpret_cast<f32x4*>(a.outd + o_off) = od;
  }
}

// ---- per-sample reductions: one workgroup per sample, fixed order --------------------------------------------------------
__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum_xor(v, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void ll_div_kernel(const float* __restrict__ x, const float* __restrict__ D, const float* __restrict__ Dd,
                                                     const float* __restrict__ v, const float* __restrict__ sigma, float* d, float* d_ll, long per_sample) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const float s = sigma[b];
  const long o = (long)b * per_sample;
  float acc = 0.f;
  for (long i = threadIdx.x; i < per_sample; i += 256) {
    const float vi = v[o + i];
    d[o + i] = __fdiv_rn(x[o + i] - D[o + i], s);
    acc = fmaf(vi, vi - Dd[o + i], acc);
  }
  const float tot = block_sum256(acc, red);
  if (threadIdx.x == 0) d_ll[b] = tot / s;
}

__global__ __launch_bounds__(256) void gauss_logp_kernel(const float* __restrict__ z, float sigma, const float* add, float* out, long per_sample) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const long o = (long)b * per_sample;
  float acc = 0.f;
  for (long i = threadIdx.x; i < per_sample; i += 256) acc = fmaf(z[o + i], z[o + i], acc);
  const float tot = block_sum256(acc, red);
  if (threadIdx.x == 0) {
    const double s = sigma;
    const double lp = -(double)tot / (2.0 * s * s) - (double)per_sample * (std::log(s) + 0.91893853320467274178);
    out[b] = (float)((add ? (double)add[b] : 0.0) + lp);
  }
}

// ---- dopri5 vector arithmetic -----------------------------------------------------------------------------------------------
constexpr int RK_MAX = 7;
constexpr int RK_ERR_BLOCKS = 256;
struct RkTerms { const float* k[RK_MAX]; float c[RK_MAX]; int nk; };

__device__ __forceinline__ float rk_sum(const RkTerms& t, long i) {
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < RK_MAX; ++j)
    if (j < t.nk) acc = fmaf(t.c[j], t.k[j][i], acc);
  return acc;
}

__global__ __launch_bounds__(256) void rk_combine_kernel(float* out, const float* y0, RkTerms t, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (y0 ? y0[i] : 0.f) + rk_sum(t, i);
}

__global__ __launch_bounds__(256) void rk_error_kernel(RkTerms t, const float* y0, const float* y1, float atol, float rtol, long n, float* partial) {
  __shared__ float red[4];
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)RK_ERR_BLOCKS * 256) {
    const float a = fabsf(y0[i]), bb = y1 ? fabsf(y1[i]) : a;
    const float r = rk_sum(t, i) / (atol + rtol * fmaxf(a, bb));
    acc = fmaf(r, r, acc);
  }
  const float tot = block_sum256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

static unsigned ew_grid(long n) {
  long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

static int rk_terms(RkTerms& t, const float* const* k, const float* c, int nk, const char* who) {
  if (nk < 1 || nk > RK_MAX || !k || !c) return fail(KD_EINVAL, "%s: 1 .. %d terms (got %d)", who, RK_MAX, nk);
  t.nk = nk;
  for (int j = 0; j < RK_MAX; ++j) {
    t.k[j] = j < nk ? k[j] : nullptr;
    t.c[j] = j < nk ? c[j] : 0.f;
    if (j < nk && !t.k[j]) return fail(KD_EINVAL, "%s: term %d is NULL", who, j);
  }
  return KD_OK;
}

template <int MODE>
int launch_attn_jvp(const AttnJvpArgs& a, const char* name, hipStream_t s) {
  const long blocks = (long)a.batch * a.nh * a.blocks_per_head;
  if (blocks > 0x7FFFFFFFL) return fail(KD_EINVAL, "%s: grid too large", name);
  LaunchScope prof(name, 0, 16.0 * (double)a.batch * a.T * a.nh * JDH, s);
  hipLaunchKernelGGL(attn_jvp_kernel<MODE>, dim3((unsigned)blocks), dim3(256), JVP_LDS, s, a);
  return check_launch(name);
}

}  // namespace
}  // namespace kd

using namespace kd;

extern "C" int kd_rmsnorm_jvp_f32(const float* x, const float* x_dot, const float* scale, int scale_stride, int rows_per_sample, float* y,
                                  float* y_dot, int rows, int d, float eps, void* stream) {
  if (!x || !x_dot || !scale || !y || !y_dot || rows <= 0 || d <= 0 || rows_per_sample <= 0 || scale_stride < 0)
    return fail(KD_EINVAL, "kd_rmsnorm_jvp_f32: bad arguments");
  if (d % 4 || scale_stride % 4) return fail(KD_EINVAL, "kd_rmsnorm_jvp_f32: d (%d) and scale_stride (%d) must be multiples of 4", d, scale_stride);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("rmsnorm_jvp_f32", 0, 20.0 * rows * d, s);
  hipLaunchKernelGGL(rmsnorm_jvp_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, x_dot, scale, scale_stride, rows_per_sample, y,
                     y_dot, rows, d, eps);
  return check_launch("kd_rmsnorm_jvp_f32");
}

extern "C" int kd_geglu_jvp_f32(const float* h, const float* h_dot, float* y, float* y_dot, int rows, int d_ff, void* stream) {
  if (!h || !h_dot || !y || !y_dot || rows <= 0 || d_ff <= 0) return fail(KD_EINVAL, "kd_geglu_jvp_f32: bad arguments");
  const long n = (long)rows * d_ff;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("geglu_jvp_f32", 0, 24.0 * n, s);
  hipLaunchKernelGGL(geglu_jvp_kernel, dim3(ew_grid(n)), dim3(256), 0, s, h, h_dot, y, y_dot, n, d_ff);
  return check_launch("kd_geglu_jvp_f32");
}

extern "C" int kd_qk_prep_jvp_f32(float* qkv, float* qkv_dot, const float* scale_h, const float* cos_t, const float* sin_t, int batch,
                                  int tokens_per_sample, int nh, float eps, void* stream) {
  if (!qkv || !qkv_dot || !scale_h || !cos_t || !sin_t || batch <= 0 || tokens_per_sample <= 0 || nh <= 0)
    return fail(KD_EINVAL, "kd_qk_prep_jvp_f32: bad arguments");
  const long rows = (long)batch * tokens_per_sample * 2 * nh;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("qk_prep_jvp_f32", 0, (double)rows * JDH * 16, s);
  hipLaunchKernelGGL(qk_prep_jvp_kernel, dim3((unsigned)((rows * 16 + 255) / 256)), dim3(256), 0, s, qkv, qkv_dot, scale_h, cos_t, sin_t, rows,
                     tokens_per_sample, nh, eps);
  return check_launch("kd_qk_prep_jvp_f32");
}

extern "C" int kd_attn_global_jvp_f32(const float* qkv, const float* qkv_dot, float* out, float* out_dot, int batch, int T, int nh, void* stream) {
  if (!qkv || !qkv_dot || !out || !out_dot || batch <= 0 || T <= 0 || nh <= 0) return fail(KD_EINVAL, "kd_attn_global_jvp_f32: bad arguments");
  AttnJvpArgs a{qkv, qkv_dot, out, out_dot, batch, nh, T, 1, T, 0, 0, (T + 15) / 16};
  return launch_attn_jvp<KS_GLOBAL>(a, "attn_global_jvp_f32", (hipStream_t)stream);
}

extern "C" int kd_attn_window_jvp_f32(const float* qkv, const float* qkv_dot, float* out, float* out_dot, int batch, int H, int W, int nh, int ws,
                                      int shift, void* stream) {
  if (!qkv || !qkv_dot || !out || !out_dot || batch <= 0 || H <= 0 || W <= 0 || nh <= 0) return fail(KD_EINVAL, "kd_attn_window_jvp_f32: bad arguments");
  if (const int rc = geo::window_check("kd_attn_window_jvp_f32", H, W, ws, shift)) return rc;
  AttnJvpArgs a{qkv, qkv_dot, out, out_dot, batch, nh, H * W, H, W, ws, shift, (H / ws) * (W / ws) * (ws * ws / 16)};
  return launch_attn_jvp<KS_WINDOW>(a, "attn_window_jvp_f32", (hipStream_t)stream);
}

extern "C" int kd_attn_na2d_jvp_f32(const float* qkv, const float* qkv_dot, float* out, float* out_dot, int batch, int H, int W, int nh, int ks,
                                    void* stream) {
  if (!qkv || !qkv_dot || !out || !out_dot || batch <= 0 || nh <= 0) return fail(KD_EINVAL, "kd_attn_na2d_jvp_f32: bad arguments");
  if (const int rc = geo::na_check("kd_attn_na2d_jvp_f32", ks, H, W)) return rc;
  AttnJvpArgs a{qkv, qkv_dot, out, out_dot, batch, nh, H * W, H, W, ks, 0, ((H + 3) / 4) * ((W + 3) / 4)};
  return launch_attn_jvp<KS_NA>(a, "attn_na2d_jvp_f32", (hipStream_t)stream);
}

extern "C" int kd_ll_div_f32(const float* x, const float* D, const float* D_dot, const float* v, const float* sigma, float* d, float* d_ll,
                             int batch, long long per_sample, void* stream) {
  if (!x || !D || !D_dot || !v || !sigma || !d || !d_ll || batch <= 0 || per_sample <= 0) return fail(KD_EINVAL, "kd_ll_div_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("ll_div_f32", 0, 20.0 * batch * (double)per_sample, s);
  hipLaunchKernelGGL(ll_div_kernel, dim3((unsigned)batch), dim3(256), 0, s, x, D, D_dot, v, sigma, d, d_ll, (long)per_sample);
  return check_launch("kd_ll_div_f32");
}

extern "C" int kd_gauss_logp_f32(const float* z, float sigma, const float* add, float* out, int batch, long long per_sample, void* stream) {
  if (!z || !out || batch <= 0 || per_sample <= 0 || !(sigma > 0.f)) return fail(KD_EINVAL, "kd_gauss_logp_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("gauss_logp_f32", 0, 4.0 * batch * (double)per_sample, s);
  hipLaunchKernelGGL(gauss_logp_kernel, dim3((unsigned)batch), dim3(256), 0, s, z, sigma, add, out, (long)per_sample);
  return check_launch("kd_gauss_logp_f32");
}

extern "C" int kd_rk_combine_f32(float* out, const float* y0, const float* const* k, const float* c, int nk, long long n, void* stream) {
  if (!out || n <= 0) return fail(KD_EINVAL, "kd_rk_combine_f32: bad arguments");
  RkTerms t;
  if (int e = rk_terms(t, k, c, nk, "kd_rk_combine_f32")) return e;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("rk_combine_f32", 0, 4.0 * (nk + 2) * (double)n, s);
  hipLaunchKernelGGL(rk_combine_kernel, dim3(ew_grid(n)), dim3(256), 0, s, out, y0, t, (long)n);
  return check_launch("kd_rk_combine_f32");
}

extern "C" int kd_rk_error_partials(void) { return RK_ERR_BLOCKS; }

extern "C" int kd_rk_error_f32(const float* const* k, const float* c, int nk, const float* y0, const float* y1, float atol, float rtol, long long n,
                               float* partial, void* stream) {
  if (!y0 || !partial || n <= 0 || !(atol >= 0.f) || !(rtol >= 0.f)) return fail(KD_EINVAL, "kd_rk_error_f32: bad arguments");
  RkTerms t;
  if (int e = rk_terms(t, k, c, nk, "kd_rk_error_f32")) return e;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("rk_error_f32", 0, 4.0 * (nk + 2) * (double)n, s);
  hipLaunchKernelGGL(rk_error_kernel, dim3(RK_ERR_BLOCKS), dim3(256), 0, s, t, y0, y1, atol, rtol, (long)n, partial);
  return check_launch("kd_rk_error_f32");
}
