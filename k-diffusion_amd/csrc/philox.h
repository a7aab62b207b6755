// Counter-based random bits shared by the device generators: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
// 3", SC 2011) with a 64-bit key and a 128-bit counter given as two 64-bit halves.  Users: the Brownian trees and index-addressed normals
// (brownian.hip: counter (element, node) / (element / 4, draw | 2^63)) and the training loss's dropout masks (dropout_f32.hip,
// wgrad_f32.hip: counter (element / 4, site | 2^62)) and the augmentation draws (augment_f32.hip: counter (sample, block | 2^63 | 2^62)); the top
// bits of the second half keep the streams apart under one key.
#pragma once

namespace kd {

struct Philox4 { unsigned x0, x1, x2, x3; };

__device__ __forceinline__ Philox4 philox4x32_10(unsigned long long key, unsigned long long elem, unsigned long long node) {
  unsigned c0 = (unsigned)elem, c1 = (unsigned)(elem >> 32), c2 = (unsigned)node, c3 = (unsigned)(node >> 32);
  unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

// Dropout mask contract (include/kdiff_hip.h): element e of site s keeps iff word e & 3 of philox4x32_10(key, e >> 2, s) >= threshold
// (threshold = floor(p 2^32)); a kept element is multiplied by scale = (float)(1 / (1 - p)), a dropped one by 0.
__device__ __forceinline__ unsigned philox_word(const Philox4& x, int i) {
  return i == 0 ? x.x0 : i == 1 ? x.x1 : i == 2 ? x.x2 : x.x3;
}

// Box-Muller on hardware transcendentals (brownian.hip, augment_f32.hip): radius from a word mapped to (0, 1], cosine of `rev` revolutions
__device__ __forceinline__ float bm_radius(unsigned w) {
  const float u = (float)((w >> 8) + 1u) * 5.9604644775390625e-08f;                  // (0, 1]
  return __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u));   // sqrt(-2 ln u), v_log_f32 is log2
}
__device__ __forceinline__ float unit24(unsigned w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }   // [0, 1)

}  // namespace kd
