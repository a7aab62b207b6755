// Sample-quality metrics of k_diffusion/evaluation.py:93-161 (gfx950): KID and FID over feature matrices the caller already has.
//
//   kd_mmd_poly_f32        squared MMD with the polynomial kernel k(x, y) = (x . y / d + 1)^3 of X [m, d] and Y [n, d] (per batch item):
//                          the Gram tiles of kxx, kyy (upper-triangle tiles only, off-diagonal ones counted twice, the diagonal dropped)
//                          and kxy are cubed and summed in registers; the m x n matrices are never written.  Per-tile partials (fp64) go
//                          to a workspace and a second launch adds them in a fixed order, so repeat calls give the same bits.
//   kd_poly_kernel_f32     the same tiles with a store epilogue: K[i, j] = (x_i . y_j / d + 1)^3
//   kd_mmd_mats_f32        squared MMD from three kernel matrices a caller's kernel function produced (kxx, kyy without their diagonal)
//   kd_jacobi_sweep_f64    one sweep of one-sided (Hestenes) Jacobi over the rows of symmetric matrices, in fp64: n - 1 rounds of n / 2
//                          disjoint row pairs in round-robin order, each rotated until orthogonal; the rotations are accumulated in Vt.  The
//                          largest |cos| between two rows of the sweep is written for the host's convergence test (one read per sweep).
//   kd_gemm_tn_f64         C = G^T diag(rs) A in fp64: the covariances, V diag(sqrt sigma) V^T, S cov_y S and the sqrtm_eig backward's products
//   kd_sym_lower_f64 / kd_row_sqrt_norm_f64 / kd_center_f32 / kd_transpose_f64 / kd_sqrtm_vjp_div_f64 / kd_f32_to_f64 / kd_fid_finish_f32
//                          the supporting passes of sqrtm_eig (and its backward) and fid
//
// Arithmetic of the Gram tiles: the backward pass's rule -- split3 on the matrix cores (bf16 hi + lo, 3 MFMAs per product, fp32 accumulate)
// under KDIFF_GEMM split3 / bf16 / fp8, fp32 FMAs under exact.  Both operands are K-contiguous rows, so a lane stages 8 consecutive k of one
// row without a transpose.  No atomics anywhere.
#include "kd_common.h"
#include "x3_common.h"

#include <cmath>

namespace kd {

namespace {

constexpr int MT = 64;                  // Gram tile: 64 rows of X x 64 rows of Y per workgroup of 4 waves
constexpr int MK = 32, MS = 40;         // split3: k per LDS step; LDS image row stride in bf16 (80 bytes)
constexpr int FK = 16;                  // fp32 FMA path: k per LDS step

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one tile of a Gram matrix: rows i of P against rows j of Q
struct Tile {
  const float* P;
  const float* Q;
  long rp, rq;           // rows of P / Q
  long i0, j0;
  bool diag;             // a diagonal tile of kxx / kyy: the diagonal is dropped
  double weight;         // 2 for an off-diagonal tile of kxx / kyy (its mirror is not computed), else 1
};

struct PolyArgs {
  const float* X;
  const float* Y;
  long m, n;
  int d;
  long sx, sy;           // batch strides of X / Y (elements)
  long tm, tn;           // tiles along m / n
  int store;             // 1: write K (sk per batch item), 0: MMD partials to ws (ntiles per batch item)
  float* K;
  double* ws;
  long ntiles;
};

// column bj of an upper triangle holds the tiles (0 .. bj, bj): t -> (bi, bj)
__device__ __forceinline__ void tri_decode(long t, long& bi, long& bj) {
  long c = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((c + 1) * (c + 2) / 2 <= t) ++c;
  while (c * (c + 1) / 2 > t) --c;
  bj = c;
  bi = t - c * (c + 1) / 2;
}

__device__ __forceinline__ Tile tile_of(const PolyArgs& a) {
  const long b = blockIdx.y;
  const float* X = a.X + b * a.sx;
  const float* Y = a.Y + b * a.sy;
  long t = blockIdx.x;
  Tile T;
  if (a.store) {
    T = Tile{X, Y, a.m, a.n, (t / a.tn) * MT, (t % a.tn) * MT, false, 1.0};
    return T;
  }
  const long txx = a.tm * (a.tm + 1) / 2, tyy = a.tn * (a.tn + 1) / 2;
  long bi, bj;
  if (t < txx) {
    tri_decode(t, bi, bj);
    return Tile{X, X, a.m, a.m, bi * MT, bj * MT, bi == bj, bi == bj ? 1.0 : 2.0};
  }
  t -= txx;
  if (t < tyy) {
    tri_decode(t, bi, bj);
    return Tile{Y, Y, a.n, a.n, bi * MT, bj * MT, bi == bj, bi == bj ? 1.0 : 2.0};
  }
  t -= tyy;
  return Tile{X, Y, a.m, a.n, (t / a.tn) * MT, (t % a.tn) * MT, false, 1.0};
}

// epilogue of one Gram entry g = x_i . y_j: the store form writes the kernel value, the MMD form adds it to the lane's sum
__device__ __forceinline__ void poly_epilogue(const PolyArgs& a, const Tile& T, float fd, long i, long j, float g, double& s) {
  const float t = g / fd + 1.0f;
  const float k = t * t * t;
  if (i >= T.rp || j >= T.rq) return;
  if (a.store) {
    a.K[(long)blockIdx.y * a.m * a.n + i * a.n + j] = k;
  } else if (!(T.diag && i == j)) {
    s += (double)k;
  }
}

// the workgroup's fp64 sum -> ws[batch item][tile]
__device__ __forceinline__ void tile_partial(const PolyArgs& a, const Tile& T, double s) {
  __shared__ double red[4];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.ws[(long)blockIdx.y * a.ntiles + blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * T.weight;
}

// ---- split3 on the matrix cores: lane t stages k .. k+7 of row t / 4 (k = 8 (t % 4)) of each operand as bf16 hi / lo -----------------------
template <bool VEC>
__device__ __forceinline__ void mmd_load(const float* P, long rows, int d, long r0, int k0, float (&v)[8]) {
  const long row = r0 + (threadIdx.x >> 2);
  const int k = k0 + (threadIdx.x & 3) * 8;
  const float* p = P + row * d + k;
  if (VEC && row < rows && k + 8 <= d) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = a[e];
      v[4 + e] = b[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (row < rows && k + e < d) ? p[e] : 0.f;
  }
}

__device__ __forceinline__ void mmd_stage(const float (&v)[8], b16::u16* hi_img, b16::u16* lo_img) {
  const int r = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 8;
  b16::u32x4 hi, lo;
  x3::split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, hi, lo);
  *reinterpret_cast<b16::u32x4*>(hi_img + r * MS + kq) = hi;
  *reinterpret_cast<b16::u32x4*>(lo_img + r * MS + kq) = lo;
}

__device__ __forceinline__ b16::bf16x8 mmd_frag(const b16::u16* img, int row, int k8) {
  return __builtin_bit_cast(b16::bf16x8, *reinterpret_cast<const b16::u32x4*>(img + row * MS + k8));
}

template <bool VEC>
__global__ __launch_bounds__(256) void poly_x3_kernel(PolyArgs a) {
  __shared__ __attribute__((aligned(16))) b16::u16 img[4][MT * MS];     // P hi, P lo, Q hi, Q lo
  const Tile T = tile_of(a);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wi = wave & 1, wj = wave >> 1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float pv[8], qv[8];
  mmd_load<VEC>(T.P, T.rp, a.d, T.i0, 0, pv);
  mmd_load<VEC>(T.Q, T.rq, a.d, T.j0, 0, qv);
  for (int k0 = 0; k0 < a.d; k0 += MK) {
    mmd_stage(pv, img[0], img[1]);
    mmd_stage(qv, img[2], img[3]);
    __syncthreads();
    if (k0 + MK < a.d) {
      mmd_load<VEC>(T.P, T.rp, a.d, T.i0, k0 + MK, pv);
      mmd_load<VEC>(T.Q, T.rq, a.d, T.j0, k0 + MK, qv);
    }
#pragma unroll
    for (int ks = 0; ks < MK / 16; ++ks) {
      const int k8 = ks * 16 + lh * 8;
      const b16::bf16x8 ph = mmd_frag(img[0], wi * 32 + l31, k8), pl = mmd_frag(img[1], wi * 32 + l31, k8);
      const b16::bf16x8 qh = mmd_frag(img[2], wj * 32 + l31, k8), ql = mmd_frag(img[3], wj * 32 + l31, k8);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pl, qh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ph, ql, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ph, qh, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const float fd = (float)a.d;
  const long j = T.j0 + wj * 32 + l31;
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 16; ++r) poly_epilogue(a, T, fd, T.i0 + wi * 32 + mfma32_row(r, lane), j, acc[r], s);
  if (!a.store) tile_partial(a, T, s);
}

// ---- fp32 FMAs (exact): 4 x 4 entries per lane, FK k per LDS step -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void poly_f32_kernel(PolyArgs a) {
  __shared__ float ps[FK][MT + 1];
  __shared__ float qs[FK][MT + 1];
  const Tile T = tile_of(a);
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < a.d; k0 += FK) {
#pragma unroll
    for (int e = tid; e < FK * MT; e += 256) {
      const int r = e / FK, k = e % FK;
      const long ip = T.i0 + r, jq = T.j0 + r;
      ps[k][r] = (ip < T.rp && k0 + k < a.d) ? T.P[ip * a.d + k0 + k] : 0.f;
      qs[k][r] = (jq < T.rq && k0 + k < a.d) ? T.Q[jq * a.d + k0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FK; ++k) {
      float pv[4], qv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) pv[i] = ps[k][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) qv[j] = qs[k][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(pv[i], qv[j], acc[i][j]);
    }
    __syncthreads();
  }
  const float fd = (float)a.d;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) poly_epilogue(a, T, fd, T.i0 + ty + 16 * i, T.j0 + tx + 16 * j, acc[i][j], s);
  if (!a.store) tile_partial(a, T, s);
}

// ---- MMD from three partial sums: one workgroup per batch item, each segment summed in a fixed order (strided lanes, then a tree) -----
__device__ double block_sum_d(const double* p, long n) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += p[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void mmd_finish_kernel(const double* __restrict__ ws, long stride, long o1, long n1, long o2, long n2, long o3,
                                                         long n3, long m, long n, float scale, int accumulate, float* __restrict__ out) {
  const double* w = ws + (long)blockIdx.x * stride;
  const double kxx = block_sum_d(w + o1, n1), kyy = block_sum_d(w + o2, n2), kxy = block_sum_d(w + o3, n3);
  if (threadIdx.x == 0) {
    const double mmd = kxx / (double)m / (double)(m - 1) + kyy / (double)n / (double)(n - 1) - kxy * 2.0 / (double)m / (double)n;
    const float v = (float)(mmd * (double)scale);
    out[blockIdx.x] = accumulate ? out[blockIdx.x] + v : v;
  }
}

// ---- MMD from kernel matrices: MC elements of one matrix per workgroup (fp64), the diagonal of kxx / kyy dropped ---------------------------
constexpr long MC = 4096;

__global__ __launch_bounds__(256) void mats_partial_kernel(const float* __restrict__ kxx, const float* __restrict__ kyy, const float* __restrict__ kxy,
                                                           long m, long n, long nchunk, double* __restrict__ ws) {
  const int which = blockIdx.y;
  const long b = blockIdx.z;
  const long rows = which == 1 ? n : m, cols = which == 0 ? m : n;
  const float* k = (which == 0 ? kxx + b * m * m : which == 1 ? kyy + b * n * n : kxy + b * m * n);
  const long e0 = (long)blockIdx.x * MC, e1 = min(rows * cols, e0 + MC);
  double s = 0.0;
  for (long e = e0 + threadIdx.x; e < e1; e += 256) {
    const long r = e / cols, c = e - r * cols;
    if (which == 2 || r != c) s += (double)k[e];
  }
  s = wave_sum_d(s);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ws[(b * 3 + which) * nchunk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- one-sided (Hestenes) Jacobi in fp64: a wave per row pair ------------------------------------------------------------------------------
// round-robin (circle) ordering over np = n rounded up to even players: in round r, pair 0 is (r, np - 1), pair k > 0 is
// ((r + k) mod (np - 1), (r - k) mod (np - 1)); a pair that names player n (odd n) sits the round out.  The rows of B and Vt are fp64: an
// fp32 solver of this form lost an order of magnitude against fp32 eigh over the ~17 sweeps a 2048-wide matrix takes.
__global__ __launch_bounds__(256) void jacobi_round_kernel(double* __restrict__ B, double* __restrict__ Vt, int n, int np, int round, double tol,
                                                           double* __restrict__ conv) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int half = np / 2;
  if (k >= half) return;                       // whole waves exit together
  const int m1 = np - 1;
  int p = k == 0 ? round : (round + k) % m1;
  int q = k == 0 ? m1 : (round - k + m1) % m1;
  if (p > q) {
    const int t = p;
    p = q;
    q = t;
  }
  if (q >= n) return;
  const long b = blockIdx.y;
  double* bp = B + (b * n + p) * (long)n;
  double* bq = B + (b * n + q) * (long)n;
  double al = 0.0, be = 0.0, ga = 0.0;
  for (int i = lane; i < n; i += 64) {
    const double x = bp[i], y = bq[i];
    al = fma(x, x, al);
    be = fma(y, y, be);
    ga = fma(x, y, ga);
  }
  al = wave_sum_d(al);                         // xor butterflies: every lane holds the same bits
  be = wave_sum_d(be);
  ga = wave_sum_d(ga);
  const double nrm = sqrt(al) * sqrt(be);
  const double off = nrm > 0.0 ? fabs(ga) / nrm : 0.0;
  if (lane == 0) conv[b * half + k] = fmax(conv[b * half + k], off);
  if (!(off > tol)) return;
  const double zeta = (be - al) / (2.0 * ga);
  const double t = copysign(1.0, zeta) / (fabs(zeta) + hypot(1.0, zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
  for (int i = lane; i < n; i += 64) {
    const double x = bp[i], y = bq[i];
    bp[i] = c * x - sn * y;
    bq[i] = sn * x + c * y;
  }
  if (Vt) {
    double* vp = Vt + (b * n + p) * (long)n;
    double* vq = Vt + (b * n + q) * (long)n;
    for (int i = lane; i < n; i += 64) {
      const double x = vp[i], y = vq[i];
      vp[i] = c * x - sn * y;
      vq[i] = sn * x + c * y;
    }
  }
}

__global__ __launch_bounds__(256) void max_kernel(const double* __restrict__ v, long n, double* __restrict__ out) {
  __shared__ double red[256];
  double m = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) m = fmax(m, v[i]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

unsigned grid_of(long n) { return (unsigned)std::min<long>((n + 255) / 256, 8192); }

// B = the symmetric matrix of a's lower triangle (fp64) + diag_add I; Vt = I if given
template <class T>
__global__ __launch_bounds__(256) void sym_lower_kernel(const T* __restrict__ a, double* __restrict__ B, double* __restrict__ Vt, long batch, int n,
                                                        double diag_add) {
  const long nn = (long)n * n, total = batch * nn;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long b = e / nn;
    const int i = (int)((e - b * nn) / n), j = (int)((e - b * nn) % n);
    B[e] = (double)a[b * nn + (long)max(i, j) * n + min(i, j)] + (i == j ? diag_add : 0.0);
    if (Vt) Vt[e] = i == j ? 1.0 : 0.0;
  }
}

// s[r] = sqrt(||B[r, :]||): the square root of the r-th singular value once the rows are orthogonal.  A wave per row.
__global__ __launch_bounds__(256) void row_sqrt_norm_kernel(const double* __restrict__ B, long rows, int n, double* __restrict__ s) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  const double* br = B + r * n;
  double ss = 0.0;
  for (int i = lane; i < n; i += 64) ss = fma(br[i], br[i], ss);
  ss = wave_sum_d(ss);
  if (lane == 0) s[r] = sqrt(sqrt(ss));
}

// C[b, n, k] = sum_m G[b, m, n] rs[b, m] A[b, m, k] in fp64 (rs may be NULL); to C64 or, rounded, to C32.  64 x 64 tile per workgroup,
// 4 x 4 entries per lane, 16 rows of m per LDS step.
constexpr int GT = 64, GR = 16;

__global__ __launch_bounds__(256) void gemm_tn_f64_kernel(const double* __restrict__ G, const double* __restrict__ A, const double* __restrict__ rs,
                                                          int M, int N, int K, double* __restrict__ C64, float* __restrict__ C32) {
  __shared__ double gs[GR][GT];
  __shared__ double as[GR][GT];
  const long b = blockIdx.z;
  G += b * (long)M * N;
  A += b * (long)M * K;
  if (rs) rs += b * (long)M;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.x * GT, k0 = blockIdx.y * GT;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int m0 = 0; m0 < M; m0 += GR) {
    for (int e = tid; e < GR * GT; e += 256) {
      const int r = e / GT, c = e % GT;
      const int m = m0 + r;
      gs[r][c] = (m < M && n0 + c < N) ? G[(long)m * N + n0 + c] : 0.0;
      as[r][c] = (m < M && k0 + c < K) ? A[(long)m * K + k0 + c] * (rs ? rs[m] : 1.0) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GR; ++r) {
      double gv[4], av[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) gv[i] = gs[r][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) av[j] = as[r][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(gv[i], av[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 16 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + tx + 16 * j;
      if (n < N && k < K) {
        const long o = b * (long)N * K + (long)n * K + k;
        if (C64) C64[o] = acc[i][j];
        else C32[o] = (float)acc[i][j];
      }
    }
  }
}

// mean = colsum / rows; xc = x - mean in fp64 (the covariance's operand)
__global__ __launch_bounds__(256) void center_kernel(const float* __restrict__ x, const float* __restrict__ colsum, long rows, int d,
                                                     double* __restrict__ xc, float* __restrict__ mean) {
  const long total = rows * d;
  const float inv = 1.0f / (float)rows;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int j = (int)(e % d);
    const float mu = colsum[j] * inv;
    xc[e] = (double)x[e] - (double)mu;
    if (mean && e < d) mean[e] = mu;
  }
}

// out[b] = a[b]^T (fp64), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void transpose_f64_kernel(const double* __restrict__ a, double* __restrict__ out, int n) {
  __shared__ double t[32][33];
  const long b = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const double* ab = a + b * (long)n * n;
  double* ob = out + b * (long)n * n;
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int r = e >> 5, c = e & 31;
    if (r0 + r < n && c0 + c < n) t[r][c] = ab[(long)(r0 + r) * n + c0 + c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int c = e >> 5, r = e & 31;
    if (r0 + r < n && c0 + c < n) ob[(long)(c0 + c) * n + r0 + r] = t[r][c];
  }
}

// out = m / (s_i + s_j) (the sqrtm_eig backward's divide; the denominator is symmetric), fp64
__global__ __launch_bounds__(256) void sqrtm_vjp_div_kernel(const double* __restrict__ m, const double* __restrict__ s, long batch, int n,
                                                            double* __restrict__ out) {
  const long nn = (long)n * n, total = batch * nn;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long b = e / nn;
    const int i = (int)((e - b * nn) / n), j = (int)((e - b * nn) % n);
    out[e] = m[e] / (s[b * n + i] + s[b * n + j]);
  }
}

__global__ __launch_bounds__(256) void f32_to_f64_kernel(const float* __restrict__ a, double* __restrict__ out, long n) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) out[e] = (double)a[e];
}

// fid = |mx - my|^2 + tr cx + tr cy - 2 sum sq (sq: sqrt of the singular values of S cov_y S), one workgroup, fp64
__global__ __launch_bounds__(256) void fid_finish_kernel(const float* __restrict__ mx, const float* __restrict__ my, const double* __restrict__ cx,
                                                         const double* __restrict__ cy, const double* __restrict__ sq, int d, float* __restrict__ out) {
  __shared__ double red[256][3];
  double mt = 0.0, tr = 0.0, st = 0.0;
  for (int i = threadIdx.x; i < d; i += 256) {
    const double dm = (double)mx[i] - (double)my[i];
    mt = fma(dm, dm, mt);
    tr += cx[(long)i * d + i] + cy[(long)i * d + i];
    st += sq[i];
  }
  red[threadIdx.x][0] = mt;
  red[threadIdx.x][1] = tr;
  red[threadIdx.x][2] = st;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w)
      for (int c = 0; c < 3; ++c) red[threadIdx.x][c] += red[threadIdx.x + w][c];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0][0] + (red[0][1] - 2.0 * red[0][2]));
}

int poly_launch(PolyArgs a, long batch, int split3, hipStream_t s) {
  const long grid = a.store ? a.tm * a.tn : a.ntiles;
  if (grid < 0 || grid > 0x7FFFFFFFL || batch > 65535) return fail(KD_EINVAL, "polynomial kernel: %ld tiles x %ld batch items: too many", grid, batch);
  const bool vec = (a.d % 4) == 0 && ((uintptr_t)a.X % 16) == 0 && ((uintptr_t)a.Y % 16) == 0 && (a.sx % 4) == 0 && (a.sy % 4) == 0;
  if (grid == 0) return KD_OK;
  const dim3 g((unsigned)grid, (unsigned)batch);
  if (!split3) hipLaunchKernelGGL(poly_f32_kernel, g, dim3(256), 0, s, a);
  else if (vec) hipLaunchKernelGGL(poly_x3_kernel<true>, g, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(poly_x3_kernel<false>, g, dim3(256), 0, s, a);
  return KD_OK;
}

}  // namespace
}  // namespace kd

using namespace kd;

extern "C" int kd_mmd_poly_f32(const float* X, long long sx, long long m, const float* Y, long long sy, long long n, int d, int batch, int split3,
                               double* ws, float scale, int accumulate, float* out, void* stream) {
  if ((!X && m) || (!Y && n) || !ws || !out || m < 0 || n < 0 || d <= 0 || batch <= 0 || sx < m * d || sy < n * d)
    return fail(KD_EINVAL, "kd_mmd_poly_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  PolyArgs a{X, Y, (long)m, (long)n, d, (long)sx, (long)sy, (long)((m + MT - 1) / MT), (long)((n + MT - 1) / MT), 0, nullptr, ws, 0};
  const long txx = a.tm * (a.tm + 1) / 2, tyy = a.tn * (a.tn + 1) / 2, txy = a.tm * a.tn;
  a.ntiles = txx + tyy + txy;
  {
    LaunchScope prof(split3 ? "mmd_poly_x3_f32" : "mmd_poly_f32", 2.0 * d * ((double)m * (m + MT) / 2 + (double)n * (n + MT) / 2 + (double)m * n) * batch,
                     4.0 * (double)(m + n) * d * batch, s);
    const int e = poly_launch(a, batch, split3, s);
    if (e) return e;
  }
  int e = check_launch("kd_mmd_poly_f32");
  if (e) return e;
  hipLaunchKernelGGL(mmd_finish_kernel, dim3((unsigned)batch), dim3(256), 0, s, ws, a.ntiles, 0L, txx, txx, tyy, txx + tyy, txy, (long)m, (long)n,
                     scale, accumulate, out);
  return check_launch("kd_mmd_poly_f32 (finish)");
}

extern "C" int kd_poly_kernel_f32(const float* X, long long sx, long long m, const float* Y, long long sy, long long n, int d, int batch, int split3,
                                  float* K, void* stream) {
  if (!X || !Y || !K || m <= 0 || n <= 0 || d <= 0 || batch <= 0 || sx < m * d || sy < n * d) return fail(KD_EINVAL, "kd_poly_kernel_f32: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  PolyArgs a{X, Y, (long)m, (long)n, d, (long)sx, (long)sy, (long)((m + MT - 1) / MT), (long)((n + MT - 1) / MT), 1, K, nullptr, 0};
  LaunchScope prof(split3 ? "poly_kernel_x3_f32" : "poly_kernel_f32", 2.0 * d * (double)m * n * batch, 4.0 * ((double)(m + n) * d + (double)m * n) * batch, s);
  const int e = poly_launch(a, batch, split3, s);
  if (e) return e;
  return check_launch("kd_poly_kernel_f32");
}

// chunks of MC elements per matrix (the largest of the three decides); ws holds 3 * that many doubles per batch item
static long long mats_chunks(long long m, long long n) {
  const long long mx = std::max(m * m, std::max(n * n, m * n));
  return (mx + MC - 1) / MC;
}

extern "C" int kd_mmd_mats_f32(const float* kxx, const float* kyy, const float* kxy, long long m, long long n, int batch, double* ws, float* out,
                               void* stream) {
  if ((!kxx && m) || (!kyy && n) || (!kxy && m && n) || !ws || !out || m < 0 || n < 0 || batch <= 0 || batch > 65535)
    return fail(KD_EINVAL, "kd_mmd_mats_f32: bad arguments");
  const long nchunk = (long)mats_chunks(m, n);
  if (nchunk > 0x7FFFFFFFL) return fail(KD_EINVAL, "kd_mmd_mats_f32: matrices too large");
  hipStream_t s = (hipStream_t)stream;
  if (nchunk) hipLaunchKernelGGL(mats_partial_kernel, dim3((unsigned)nchunk, 3, (unsigned)batch), dim3(256), 0, s, kxx, kyy, kxy, (long)m, (long)n, nchunk, ws);
  int e = check_launch("kd_mmd_mats_f32");
  if (e) return e;
  hipLaunchKernelGGL(mmd_finish_kernel, dim3((unsigned)batch), dim3(256), 0, s, ws, 3 * nchunk, 0L, nchunk, nchunk, nchunk, 2 * nchunk, nchunk,
                     (long)m, (long)n, 1.0f, 0, out);
  return check_launch("kd_mmd_mats_f32 (finish)");
}

extern "C" int kd_jacobi_sweep_f64(double* B, double* Vt, int batch, int n, double tol, double* conv, double* off, void* stream) {
  if (!B || !conv || !off || batch <= 0 || batch > 65535 || n <= 0) return fail(KD_EINVAL, "kd_jacobi_sweep_f64: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int np = n + (n & 1), half = np / 2;
  const long nconv = (long)batch * half;
  if (hipMemsetAsync(conv, 0, nconv * sizeof(double), s) != hipSuccess) return fail(KD_ELAUNCH, "kd_jacobi_sweep_f64: memset");
  {
    LaunchScope prof("jacobi_sweep_f64", 3.0 * (Vt ? 2 : 1) * (double)n * n * (np - 1) * batch, 16.0 * (Vt ? 2 : 1) * (double)n * n * (np - 1) * batch, s);
    const dim3 grid((unsigned)((half + 3) / 4), (unsigned)batch);
    for (int r = 0; r < np - 1; ++r) {
      hipLaunchKernelGGL(jacobi_round_kernel, grid, dim3(256), 0, s, B, Vt, n, np, r, tol, conv);
      const int e = check_launch("kd_jacobi_sweep_f64");
      if (e) return e;
    }
  }
  hipLaunchKernelGGL(max_kernel, dim3(1), dim3(256), 0, s, conv, nconv, off);
  return check_launch("kd_jacobi_sweep_f64 (max)");
}

extern "C" int kd_sym_lower_f64(const void* a, int a_f64, double* B, double* Vt, int batch, int n, double diag_add, void* stream) {
  if (!a || !B || batch <= 0 || n <= 0) return fail(KD_EINVAL, "kd_sym_lower_f64: bad arguments");
  const dim3 grid(grid_of((long)batch * n * n));
  if (a_f64) hipLaunchKernelGGL(sym_lower_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)a, B, Vt, (long)batch, n, diag_add);
  else hipLaunchKernelGGL(sym_lower_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)a, B, Vt, (long)batch, n, diag_add);
  return check_launch("kd_sym_lower_f64");
}

extern "C" int kd_row_sqrt_norm_f64(const double* B, long long rows, int n, double* s, void* stream) {
  if (!B || !s || rows <= 0 || n <= 0) return fail(KD_EINVAL, "kd_row_sqrt_norm_f64: bad arguments");
  hipLaunchKernelGGL(row_sqrt_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, B, (long)rows, n, s);
  return check_launch("kd_row_sqrt_norm_f64");
}

extern "C" int kd_gemm_tn_f64(const double* G, const double* A, const double* row_scale, int batch, int M, int N, int K, double* C64, float* C32,
                              void* stream) {
  if (!G || !A || (!C64 == !C32) || batch <= 0 || batch > 65535 || M <= 0 || N <= 0 || K <= 0) return fail(KD_EINVAL, "kd_gemm_tn_f64: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("gemm_tn_f64", 2.0 * (double)M * N * K * batch, 8.0 * (double)M * (N + K) * batch, s);
  const dim3 grid((unsigned)((N + GT - 1) / GT), (unsigned)((K + GT - 1) / GT), (unsigned)batch);
  hipLaunchKernelGGL(gemm_tn_f64_kernel, grid, dim3(256), 0, s, G, A, row_scale, M, N, K, C64, C32);
  return check_launch("kd_gemm_tn_f64");
}

extern "C" int kd_center_f32(const float* x, const float* colsum, long long rows, int d, double* xc, float* mean, void* stream) {
  if (!x || !colsum || !xc || rows <= 0 || d <= 0) return fail(KD_EINVAL, "kd_center_f32: bad arguments");
  hipLaunchKernelGGL(center_kernel, dim3(grid_of((long)rows * d)), dim3(256), 0, (hipStream_t)stream, x, colsum, (long)rows, d, xc, mean);
  return check_launch("kd_center_f32");
}

extern "C" int kd_transpose_f64(const double* a, double* out, int batch, int n, void* stream) {
  if (!a || !out || batch <= 0 || batch > 65535 || n <= 0) return fail(KD_EINVAL, "kd_transpose_f64: bad arguments");
  const dim3 grid((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32), (unsigned)batch);
  hipLaunchKernelGGL(transpose_f64_kernel, grid, dim3(256), 0, (hipStream_t)stream, a, out, n);
  return check_launch("kd_transpose_f64");
}

extern "C" int kd_sqrtm_vjp_div_f64(const double* m, const double* s, int batch, int n, double* out, void* stream) {
  if (!m || !s || !out || batch <= 0 || n <= 0) return fail(KD_EINVAL, "kd_sqrtm_vjp_div_f64: bad arguments");
  hipLaunchKernelGGL(sqrtm_vjp_div_kernel, dim3(grid_of((long)batch * n * n)), dim3(256), 0, (hipStream_t)stream, m, s, (long)batch, n, out);
  return check_launch("kd_sqrtm_vjp_div_f64");
}

extern "C" int kd_f32_to_f64(const float* a, double* out, long long n, void* stream) {
  if (!a || !out || n <= 0) return fail(KD_EINVAL, "kd_f32_to_f64: bad arguments");
  hipLaunchKernelGGL(f32_to_f64_kernel, dim3(grid_of((long)n)), dim3(256), 0, (hipStream_t)stream, a, out, (long)n);
  return check_launch("kd_f32_to_f64");
}

extern "C" int kd_fid_finish_f32(const float* mean_x, const float* mean_y, const double* cov_x, const double* cov_y, const double* sq, int d,
                                 float* out, void* stream) {
  if (!mean_x || !mean_y || !cov_x || !cov_y || !sq || !out || d <= 0) return fail(KD_EINVAL, "kd_fid_finish_f32: bad arguments");
  hipLaunchKernelGGL(fid_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mean_x, mean_y, cov_x, cov_y, sq, d, out);
  return check_launch("kd_fid_finish_f32");
}
