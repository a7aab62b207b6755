// fp32 pieces shared by the forward-mode (jvp_f32.hip) and reverse-mode (vjp_f32.hip) kernels of the HDiT denoiser: the RoPE rotation of
// a 64-float head row held by 16 lanes; the key sets of the three attention geometries come from attn_geo.h.
#pragma once
#include "kd_common.h"
#include "attn_geo.h"

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

// Key sets (which keys a block of 16 queries attends, in the three attention geometries) and the neighbourhood's window start: attn_geo.h
using geo::KS_GLOBAL;
using geo::KS_WINDOW;
using geo::KS_NA;
using geo::KeySet;
using geo::na_start;

}  // namespace
}  // namespace kd
