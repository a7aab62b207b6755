// fp32 pieces shared by the forward-mode (jvp_f32.hip) and reverse-mode (vjp_f32.hip) kernels of the HDiT denoiser: the RoPE rotation of
// a 64-float head row held by 16 lanes, and the key sets of the three attention geometries.
#pragma once
#include "kd_common.h"

namespace kd {
namespace {

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// RoPE of a 64-float row, 16 lanes, lane c owning dims [4c, 4c+4): dims [0,16) pair with [16,32) (image_transformer_v2.py:187-231).
// With sn negated it is the inverse rotation.
__device__ __forceinline__ f32x4 rope16(f32x4 v, int c, f32x4 cs, f32x4 sn) {
  f32x4 up, dn;
#pragma unroll
  for (int u = 0; u < 4; ++u) { up[u] = dpp_mov<DPP_ROR12>(v[u]); dn[u] = dpp_mov<DPP_ROR4>(v[u]); }
  const f32x4 rot = (c < 4) ? (v * cs - up * sn) : (v * cs + dn * sn);
  return c < 8 ? rot : v;
}

// Key sets: the keys a block of 16 queries of one (sample, head) attends (qb: the block within the head, g: the query within the block).
// All T tokens (global), the window (shifted window; the reference's region mask is a per-pair predicate), or the union of the queries'
// clamped neighbourhoods for a 4x4 query tile (neighbourhood; the predicate keeps each query's own ks x ks window).  The window's pair
// predicate is symmetric, so the same set, read from the key's side, is the set of queries that attend a key.  ``A`` carries T, H, W,
// geo (window size / kernel size) and shift.
enum { KS_GLOBAL = 0, KS_WINDOW = 1, KS_NA = 2 };

__device__ __forceinline__ int na_start(int i, int len, int ks) { return min(max(i - ks / 2, 0), len - ks); }
__device__ __forceinline__ int wrap(int i, int n) { return ((i % n) + n) % n; }

template <int MODE>
struct KeySet {
  // query side
  int qtok; bool qactive;
  int q_a, q_b;                 // window: region id parts / neighbourhood: window start row, col
  // key side
  int n_keys;
  int base_r, base_c, span_c;   // window: window origin (rows, cols of the rolled grid) / neighbourhood: halo origin and width
  int win_top, win_left;        // window: the window is in the top row / left column of windows

  template <class A>
  __device__ void init(const A& a, int qb, int g) {
    if (MODE == KS_GLOBAL) {
      const int t = qb * 16 + g;
      qactive = t < a.T;
      qtok = min(t, a.T - 1);
      n_keys = a.T;
    } else if (MODE == KS_WINDOW) {
      const int ws = a.geo, per_win = ws * ws / 16, nww = a.W / ws;
      const int win = qb / per_win, s = (qb % per_win) * 16 + g;
      const int wi = win / nww, wj = win % nww;
      base_r = wi * ws; base_c = wj * ws;
      win_top = wi == 0; win_left = wj == 0;
      const int qa = s / ws, qc = s % ws;
      qtok = wrap(base_r + qa - a.shift, a.H) * a.W + wrap(base_c + qc - a.shift, a.W);
      q_a = win_top ? (qa < a.shift) : 0;
      q_b = win_left ? (qc < a.shift) : 0;
      qactive = true;
      n_keys = ws * ws;
    } else {
      const int ks = a.geo, tw = (a.W + 3) / 4;
      const int th = qb / tw, tc = qb % tw;
      const int r0 = th * 4, c0 = tc * 4;
      const int qr = r0 + (g >> 2), qc = c0 + (g & 3);
      qactive = qr < a.H && qc < a.W;
      const int qr_c = min(qr, a.H - 1), qc_c = min(qc, a.W - 1);
      qtok = qr_c * a.W + qc_c;
      q_a = na_start(qr_c, a.H, ks);
      q_b = na_start(qc_c, a.W, ks);
      base_r = na_start(r0, a.H, ks);
      base_c = na_start(c0, a.W, ks);
      const int r_hi = na_start(min(r0 + 3, a.H - 1), a.H, ks) + ks, c_hi = na_start(min(c0 + 3, a.W - 1), a.W, ks) + ks;
      span_c = c_hi - base_c;
      n_keys = (r_hi - base_r) * span_c;
    }
  }
  template <class A>
  __device__ int key_tok(const A& a, int j) const {
    if (MODE == KS_GLOBAL) return j;
    if (MODE == KS_WINDOW) {
      const int ws = a.geo, ka = j / ws, kc = j % ws;
      return wrap(base_r + ka - a.shift, a.H) * a.W + wrap(base_c + kc - a.shift, a.W);
    }
    return (base_r + j / span_c) * a.W + base_c + j % span_c;
  }
  template <class A>
  __device__ bool allowed(const A& a, int j) const {
    if (j >= n_keys) return false;
    if (MODE == KS_GLOBAL) return true;
    if (MODE == KS_WINDOW) {
      const int ws = a.geo, ka = j / ws, kc = j % ws;
      return (win_top ? (ka < a.shift) : 0) == q_a && (win_left ? (kc < a.shift) : 0) == q_b;
    }
    const int r = base_r + j / span_c, cc = base_c + j % span_c;
    return r >= q_a && r < q_a + a.geo && cc >= q_b && cc < q_b + a.geo;
  }
};

}  // namespace
}  // namespace kd
