// The training step behind the loss (gfx950): gradient clipping, AdamW, the EMA model and the sigma draw of the reference's train.py:444-473
// as multi-tensor streaming kernels.  One launch covers every parameter of the optimizer: a device-resident table of tensors (KdMtTensor) and a
// list of (tensor, chunk) pairs that maps workgroups to KD_MT_CHUNK-element pieces, so that a few hundred tensors of very different sizes
// fill the machine together.  The caller owns and refreshes both (nothing here allocates, copies or synchronises).
//
//   kd_mt_sqnorm_f32      global L2 norm of the table's gradients: exact fp64 squares, one fp64 partial per chunk, a second one-workgroup
//                         launch that adds the partials in index order and writes {norm, clip coefficient}
//   kd_mt_adamw_ema_f32   one pass per element: clip scale, torch.optim.AdamW's update, the EMA lerp, the gradient zeroing
//   kd_mt_lerp_f32        the EMA lerp alone (K.utils.ema_update)
//   kd_sigma_density_f32  uniforms (and normals) -> sigmas for the six densities of utils.py:323-385, stratification folded in
//
// Memory-bound: 16-byte loads and stores where every pointer of a tensor is 16-byte aligned (chunk starts are multiples of 4 elements, so a
// tensor's alignment is its chunks'), an element-wise tail for the last n % 4, the grid capped at 8 workgroups per CU with a stride over the
// chunk list.  No atomics: every sum has a fixed order and repeat calls give the same bits.  The update rounds where torch's foreach kernels on
// the device round: once per foreach operation, the multiply-add inside lerp / addcmul / addcdiv fused.  Those are spelled fmaf here and the
// file is compiled with -ffp-contract=off (Makefile), so that the compiler fuses nothing else.
#include "kd_common.h"

namespace kd {

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_MAX_GROUPS = 16;       // groups per launch (the by-value argument block); kd_mt_adamw_ema_f32 splits beyond that

// per-group constants as the kernel uses them: torch converts its Python doubles to the tensor's dtype once per call, and so does this
struct AdamArgs {
  float decay_mul[MT_MAX_GROUPS];   // 1 - lr * wd
  float w1[MT_MAX_GROUPS];          // 1 - beta1
  float beta2[MT_MAX_GROUPS];
  float omb2[MT_MAX_GROUPS];        // 1 - beta2
  float bc2_sqrt[MT_MAX_GROUPS];    // sqrt(bc2)
  float eps[MT_MAX_GROUPS];
  float neg_step[MT_MAX_GROUPS];    // -(lr / bc1)
};

// torch.lerp (ATen/native/Lerp.h): the form that is exact at the nearer end, its multiply-add fused as torch's device kernels compile it
__device__ __forceinline__ float lerp_t(float a, float b, float w) {
  const float d = b - a;
  return fabsf(w) < 0.5f ? fmaf(w, d, a) : fmaf(-d, 1.0f - w, b);
}
__device__ __forceinline__ double lerp_t(double a, double b, double w) {
  const double d = b - a;
  return fabs(w) < 0.5 ? fma(w, d, a) : fma(-d, 1.0 - w, b);
}

// sum over the workgroup in a fixed order: xor butterfly inside each wave, then the four wave sums in wave order (result in every thread)
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                                          const void* e = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d) |
           reinterpret_cast<uintptr_t>(e)) & 15) == 0;
}

__global__ __launch_bounds__(MT_THREADS) void mt_sqnorm_kernel(const KdMtTensor* __restrict__ table, const int* __restrict__ chunks, int n_chunks,
                                                               double* __restrict__ ws) {
  __shared__ double lds[4];
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const KdMtTensor t = table[chunks[2 * c]];
    const long long base = (long long)chunks[2 * c + 1] * KD_MT_CHUNK;
    const int len = (int)min((long long)KD_MT_CHUNK, t.n - base);
    const float* g = t.g + base;
    double acc = 0.0;
    if (aligned16(t.g)) {
      const int nvec = len >> 2;
      for (int q = threadIdx.x; q < nvec; q += MT_THREADS) {
        const float4 x = reinterpret_cast<const float4*>(g)[q];
        acc += (double)x.x * (double)x.x;
        acc += (double)x.y * (double)x.y;
        acc += (double)x.z * (double)x.z;
        acc += (double)x.w * (double)x.w;
      }
      const int e = 4 * nvec + threadIdx.x;
      if (e < len) acc += (double)g[e] * (double)g[e];
    } else {
      for (int e = threadIdx.x; e < len; e += MT_THREADS) acc += (double)g[e] * (double)g[e];
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) ws[c] = s;
  }
}

// out[0] = the norm, out[1] = min(1, max_norm / (norm + 1e-6)) in fp32 from the rounded norm, as torch.nn.utils.clip_grad_norm_ forms it
// (a NaN norm gives a NaN coefficient, an infinite one gives 0)
__global__ __launch_bounds__(MT_THREADS) void mt_sqnorm_finish_kernel(const double* __restrict__ ws, int n_chunks, float max_norm,
                                                                      float* __restrict__ out) {
  __shared__ double lds[4];
  double acc = 0.0;
  for (int c = threadIdx.x; c < n_chunks; c += MT_THREADS) acc += ws[c];
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    const float coef = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = coef > 1.0f ? 1.0f : coef;
  }
}

struct AdamElem { float p, m, v, ema; };

template <bool EMA>
__device__ __forceinline__ AdamElem adam_elem(float p, float g, float m, float v, float ema, float clip, float decay_mul, float w1, float beta2,
                                              float omb2, float bc2_sqrt, float eps, float neg_step, float ema_w) {
  g = g * clip;
  p = p * decay_mul;
  m = lerp_t(m, g, w1);
  v = fmaf(omb2 * g, g, v * beta2);
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = fmaf(neg_step, m / denom, p);
  AdamElem o = {p, m, v, ema};
  if (EMA) o.ema = lerp_t(ema, p, ema_w);
  return o;
}

__global__ __launch_bounds__(MT_THREADS) void mt_adamw_ema_kernel(const KdMtTensor* __restrict__ table, const int* __restrict__ chunks, int n_chunks,
                                                                  AdamArgs a, int group_base, int n_groups, const float* __restrict__ clip_ptr,
                                                                  float ema_w, int use_ema, int zero_grad) {
  const float clip = clip_ptr ? clip_ptr[1] : 1.0f;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const KdMtTensor t = table[chunks[2 * c]];
    const int gi = t.group - group_base;
    if (gi < 0 || gi >= n_groups) continue;            // another launch's groups
    const long long base = (long long)chunks[2 * c + 1] * KD_MT_CHUNK;
    const int len = (int)min((long long)KD_MT_CHUNK, t.n - base);
    float* p = t.p + base;
    float* g = t.g + base;
    float* m = t.m + base;
    float* v = t.v + base;
    const bool ema_on = use_ema && t.ema != nullptr;
    float* ema = ema_on ? t.ema + base : nullptr;
    const float decay_mul = a.decay_mul[gi], w1 = a.w1[gi], beta2 = a.beta2[gi], omb2 = a.omb2[gi], bc2_sqrt = a.bc2_sqrt[gi], eps = a.eps[gi],
                neg_step = a.neg_step[gi];
    int done = 0;
    if (aligned16(t.p, t.g, t.m, t.v, t.ema)) {
      const int nvec = len >> 2;
      for (int q = threadIdx.x; q < nvec; q += MT_THREADS) {
        const float4 P = reinterpret_cast<const float4*>(p)[q], G = reinterpret_cast<const float4*>(g)[q];
        const float4 M = reinterpret_cast<const float4*>(m)[q], V = reinterpret_cast<const float4*>(v)[q];
        float4 E = {0.f, 0.f, 0.f, 0.f};
        AdamElem o0, o1, o2, o3;
        if (ema_on) {
          E = reinterpret_cast<const float4*>(ema)[q];
          o0 = adam_elem<true>(P.x, G.x, M.x, V.x, E.x, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          o1 = adam_elem<true>(P.y, G.y, M.y, V.y, E.y, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          o2 = adam_elem<true>(P.z, G.z, M.z, V.z, E.z, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          o3 = adam_elem<true>(P.w, G.w, M.w, V.w, E.w, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          st16(ema + 4 * q, float4{o0.ema, o1.ema, o2.ema, o3.ema});
        } else {
          o0 = adam_elem<false>(P.x, G.x, M.x, V.x, 0.f, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          o1 = adam_elem<false>(P.y, G.y, M.y, V.y, 0.f, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          o2 = adam_elem<false>(P.z, G.z, M.z, V.z, 0.f, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
          o3 = adam_elem<false>(P.w, G.w, M.w, V.w, 0.f, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
        }
        st16(p + 4 * q, float4{o0.p, o1.p, o2.p, o3.p});
        st16(m + 4 * q, float4{o0.m, o1.m, o2.m, o3.m});
        st16(v + 4 * q, float4{o0.v, o1.v, o2.v, o3.v});
        if (zero_grad) st16(g + 4 * q, float4{0.f, 0.f, 0.f, 0.f});
      }
      done = 4 * nvec;
    }
    for (int e = done + threadIdx.x; e < len; e += MT_THREADS) {
      AdamElem o;
      if (ema_on) {
        o = adam_elem<true>(p[e], g[e], m[e], v[e], ema[e], clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
        ema[e] = o.ema;
      } else {
        o = adam_elem<false>(p[e], g[e], m[e], v[e], 0.f, clip, decay_mul, w1, beta2, omb2, bc2_sqrt, eps, neg_step, ema_w);
      }
      p[e] = o.p;
      m[e] = o.m;
      v[e] = o.v;
      if (zero_grad) g[e] = 0.f;
    }
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_lerp_kernel(const KdMtTensor* __restrict__ table, const int* __restrict__ chunks, int n_chunks,
                                                             float w) {
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const KdMtTensor t = table[chunks[2 * c]];
    if (t.ema == nullptr) continue;
    const long long base = (long long)chunks[2 * c + 1] * KD_MT_CHUNK;
    const int len = (int)min((long long)KD_MT_CHUNK, t.n - base);
    const float* p = t.p + base;
    float* ema = t.ema + base;
    int done = 0;
    if (aligned16(t.p, t.ema)) {
      const int nvec = len >> 2;
      for (int q = threadIdx.x; q < nvec; q += MT_THREADS) {
        const float4 P = reinterpret_cast<const float4*>(p)[q], E = reinterpret_cast<const float4*>(ema)[q];
        st16(ema + 4 * q, float4{lerp_t(E.x, P.x, w), lerp_t(E.y, P.y, w), lerp_t(E.z, P.z, w), lerp_t(E.w, P.w, w)});
      }
      done = 4 * nvec;
    }
    for (int e = done + threadIdx.x; e < len; e += MT_THREADS) ema[e] = lerp_t(ema[e], p[e], w);
  }
}

// ---- sigma densities ---------------------------------------------------------------------------------------------------------------
// A training batch's worth of values: everything in fp64 from the drawn fp32 / fp64 uniforms (the log-logistic is fp64 in the reference
// too), one rounding at the store.
struct DensityArgs { double p[8]; };

__device__ __forceinline__ double logsnr_cosine(double t, double t_min, double t_max, double shift) {
  return -2.0 * log(tan(t_min + t * (t_max - t_min))) + shift;
}

__global__ __launch_bounds__(MT_THREADS) void sigma_density_kernel(int kind, const void* __restrict__ u_ptr, int u_f64, const void* __restrict__ n_ptr,
                                                                   void* __restrict__ out, int out_f64, long long n, int row_len, int group,
                                                                   int groups, DensityArgs a) {
  for (long long e = (long long)blockIdx.x * MT_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * MT_THREADS) {
    double u = u_f64 ? reinterpret_cast<const double*>(u_ptr)[e] : (double)reinterpret_cast<const float*>(u_ptr)[e];
    if (groups > 0) {                                     // utils.py:267-276: sample i of the row lies in stratum group + i * groups
      const long long i = e % row_len;
      u = ((double)(group + i * groups) + u) / ((double)row_len * (double)groups);
    }
    double s;
    switch (kind) {
      case KD_DENSITY_LOGNORMAL:                          // p = loc, scale
        s = exp(a.p[0] + a.p[1] * normcdfinv(u * (1.0 - 2e-7) + 1e-7));
        break;
      case KD_DENSITY_LOGLOGISTIC: {                      // p = loc, scale, min_cdf, max_cdf
        const double c = u * (a.p[3] - a.p[2]) + a.p[2];
        s = exp(log(c / (1.0 - c)) * a.p[1] + a.p[0]);
        break;
      }
      case KD_DENSITY_LOGUNIFORM:                         // p = log min, log max
        s = exp(u * (a.p[1] - a.p[0]) + a.p[0]);
        break;
      case KD_DENSITY_V_DIFFUSION: {                      // p = sigma_data, min_cdf, max_cdf
        const double c = u * (a.p[2] - a.p[1]) + a.p[1];
        s = tan(c * 3.14159265358979323846 / 2.0) * a.p[0];
        break;
      }
      case KD_DENSITY_COSINE_INTERPOLATED: {              // p = t_min, t_max, shift of the low schedule, the same of the high one, sigma_data
        const double lo = logsnr_cosine(u, a.p[0], a.p[1], a.p[2]);
        const double hi = logsnr_cosine(u, a.p[3], a.p[4], a.p[5]);
        s = exp(-lerp_t(lo, hi, u) / 2.0) * a.p[6];
        break;
      }
      default: {                                          // KD_DENSITY_SPLIT_LOGNORMAL: p = loc, scale_1, scale_2, ratio
        const double z = fabs(u_f64 ? reinterpret_cast<const double*>(n_ptr)[e] : (double)reinterpret_cast<const float*>(n_ptr)[e]);
        s = exp(u < a.p[3] ? z * -a.p[1] + a.p[0] : z * a.p[2] + a.p[0]);
        break;
      }
    }
    if (out_f64) reinterpret_cast<double*>(out)[e] = s;
    else reinterpret_cast<float*>(out)[e] = (float)s;
  }
}

unsigned mt_grid(int n_chunks) { return (unsigned)std::min(n_chunks, cu_count() * 8); }

bool bad_list(const void* table, const void* chunks, int n_chunks) { return !table || !chunks || n_chunks <= 0; }

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_mt_sqnorm_f32(const KdMtTensor* table, const int* chunks, int n_chunks, float max_norm, double* ws, float* out, void* stream) {
  if (bad_list(table, chunks, n_chunks) || !ws || !out) return fail(KD_EINVAL, "kd_mt_sqnorm_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  {
    LaunchScope prof("mt_sqnorm_f32", 0, 4.0 * KD_MT_CHUNK * (double)n_chunks, s);
    hipLaunchKernelGGL(mt_sqnorm_kernel, dim3(mt_grid(n_chunks)), dim3(MT_THREADS), 0, s, table, chunks, n_chunks, ws);
  }
  LaunchScope prof("mt_sqnorm_finish", 0, 8.0 * (double)n_chunks, s);
  hipLaunchKernelGGL(mt_sqnorm_finish_kernel, dim3(1), dim3(MT_THREADS), 0, s, (const double*)ws, n_chunks, max_norm, out);
  return check_launch("kd_mt_sqnorm_f32");
}

extern "C" int kd_mt_adamw_ema_f32(const KdMtTensor* table, const int* chunks, int n_chunks, const KdAdamGroup* groups, int n_groups,
                                   const float* clip, double ema_decay, int use_ema, int zero_grad, void* stream) {
  if (bad_list(table, chunks, n_chunks) || !groups || n_groups <= 0) return fail(KD_EINVAL, "kd_mt_adamw_ema_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const float ema_w = (float)(1.0 - ema_decay);
  for (int base = 0; base < n_groups; base += MT_MAX_GROUPS) {
    const int cnt = std::min(MT_MAX_GROUPS, n_groups - base);
    AdamArgs a = {};
    for (int i = 0; i < cnt; ++i) {
      const KdAdamGroup& g = groups[base + i];
      a.decay_mul[i] = (float)(1.0 - g.lr * g.wd);
      a.w1[i] = (float)(1.0 - g.beta1);
      a.beta2[i] = (float)g.beta2;
      a.omb2[i] = (float)(1.0 - g.beta2);
      a.bc2_sqrt[i] = (float)sqrt(g.bc2);
      a.eps[i] = (float)g.eps;
      a.neg_step[i] = (float)(-(g.lr / g.bc1));
    }
    LaunchScope prof("mt_adamw_ema_f32", 0, 40.0 * KD_MT_CHUNK * (double)n_chunks, s);
    hipLaunchKernelGGL(mt_adamw_ema_kernel, dim3(mt_grid(n_chunks)), dim3(MT_THREADS), 0, s, table, chunks, n_chunks, a, base, cnt, clip, ema_w,
                       use_ema, zero_grad);
  }
  return check_launch("kd_mt_adamw_ema_f32");
}

extern "C" int kd_mt_lerp_f32(const KdMtTensor* table, const int* chunks, int n_chunks, double weight, void* stream) {
  if (bad_list(table, chunks, n_chunks)) return fail(KD_EINVAL, "kd_mt_lerp_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("mt_lerp_f32", 0, 12.0 * KD_MT_CHUNK * (double)n_chunks, s);
  hipLaunchKernelGGL(mt_lerp_kernel, dim3(mt_grid(n_chunks)), dim3(MT_THREADS), 0, s, table, chunks, n_chunks, (float)weight);
  return check_launch("kd_mt_lerp_f32");
}

extern "C" int kd_sigma_density_f32(int kind, const void* u, int u_f64, const void* normal, void* out, int out_f64, long long n, int row_len,
                                    int group, int groups, const double* params, void* stream) {
  if (!u || !out || !params || n <= 0) return fail(KD_EINVAL, "kd_sigma_density_f32: bad arguments");
  if (kind < KD_DENSITY_LOGNORMAL || kind > KD_DENSITY_SPLIT_LOGNORMAL) return fail(KD_EINVAL, "kd_sigma_density_f32: unknown density %d", kind);
  if (kind == KD_DENSITY_SPLIT_LOGNORMAL && !normal) return fail(KD_EINVAL, "kd_sigma_density_f32: the split log-normal needs normals");
  if (groups < 0 || (groups > 0 && (group < 0 || group >= groups || row_len <= 0)))
    return fail(KD_EINVAL, "kd_sigma_density_f32: group must be in [0, groups) and row_len positive");
  DensityArgs a;
  for (int i = 0; i < 8; ++i) a.p[i] = params[i];
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("sigma_density_f32", 0, 8.0 * (double)n, s);
  const unsigned grid = (unsigned)std::min<long long>((n + MT_THREADS - 1) / MT_THREADS, 1024);
  hipLaunchKernelGGL(sigma_density_kernel, dim3(grid), dim3(MT_THREADS), 0, s, kind, u, u_f64, normal, out, out_f64, n, row_len, group, groups, a);
  return check_launch("kd_sigma_density_f32");
}
