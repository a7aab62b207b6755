// The width-128, two-workgroups-per-CU fused feed-forward block of the fp32-parity ("split3") mode as a device function over a PANEL of
// 128 rows: ffn_x3.hip wraps it into ffn_x3h_kernel (a panel = 128 consecutive rows), attn_ffn_x3.hip runs it behind the neighbourhood
// attention core on the core's 8 x 16 query tile (the attention rows then come from LDS, not from HBM).  The block is row-wise: nothing
// in it depends on which rows share a panel beyond the addresses `Panel::row` hands out.  See ffn_x3.hip for the design.
#pragma once
#include "x3_common.h"

namespace kd {
namespace x3 {

struct FArgs3 {
  const float* X; float* Y;
  const char* Wu; const char* Wd;
  const float* scale; int scale_stride, rows_per_sample; float eps;
  int M, d_ff, n_tiles;
  int warm;
  unsigned long long* clk;
  const float* Att; const char* Wo;   // fused out projection in front of the block (round 3): X <- X + Att Wo^T first; NULL = none
};

template <int IDX>
__device__ __forceinline__ f32x4 areg_read4() {
  f32x4 v;
  asm volatile("v_accvgpr_read_b32 %0, a[%c4]\n\tv_accvgpr_read_b32 %1, a[%c5]\n\tv_accvgpr_read_b32 %2, a[%c6]\n\tv_accvgpr_read_b32 %3, a[%c7]"
               : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3]) : "i"(IDX), "i"(IDX + 1), "i"(IDX + 2), "i"(IDX + 3));
  return v;
}

template <int IDX>
__device__ __forceinline__ void mfma_acc_ag_lo(const bf16x8 w, const bf16x8 h) {
  asm volatile("v_mfma_f32_32x32x16_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" :: "v"(w), "v"(h), "i"(IDX), "i"(IDX + 15) : KD_AGPR_LO128);
}
// output accumulators (named AccVGPRs) += W fragment x activation fragment held in AccVGPRs too
template <int IDX, int BIDX>
__device__ __forceinline__ void mfma_acc_aa_lo(const bf16x8 w) {
  asm volatile("v_mfma_f32_32x32x16_bf16 a[%c1:%c2], %0, a[%c3:%c4], a[%c1:%c2]" :: "v"(w), "i"(IDX), "i"(IDX + 15), "i"(BIDX), "i"(BIDX + 3) : KD_AGPR_LO128);
}
template <int IDX>
__device__ __forceinline__ void areg_zero16_lo() {
  static_for<16>([&](auto i_) { asm volatile("v_accvgpr_write_b32 a[%c0], 0" :: "i"(IDX + decltype(i_)::value) : KD_AGPR_LO128); });
}

// 128 consecutive rows from m0 on (rows past M are clamped by the body)
struct PanelRows {
  static constexpr bool ATT_LDS = false;
  int m0;
  __device__ __forceinline__ int row(int i) const { return m0 + i; }
};

// Panel::row(i): row of X / Y / Att that panel row i (wave i >> 5, lane-row i & 31) stands for.  Panel::ATT_LDS: the caller has already put the
// wave's 32 attention rows into its borrowed ring slot (smem + wave * STG: row r at + 512 r, 16-byte chunk c in slot c ^ (r & 15), fp32) --
// the layout the LDS-DMA below produces from HBM otherwise.  `tid`: the thread of the 256.  `warm_end()` runs once behind the first vector-memory wait.
template <bool OUTP, class Panel, class WarmEnd>
__device__ __forceinline__ void ffn_x3h_body(const FArgs3& p, char* smem, int tid, const Panel& pn, WarmEnd&& warm_end) {
  constexpr int NC = 8, K = 128, NOB = 4;
  constexpr int NSTG = 4, PDIST = NSTG - 1, PB = 4, UNIT = 3;   // stages per half tile: 2 up + 1 down
  constexpr int AO = 64;
  constexpr int CPR = K / 4, PIECES = 32 * CPR / 64, SCL = 1024, SUB = 8192, HALF = 4096;
  const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T2 = 2 * p.n_tiles;                                 // half tiles
  const bool probe = p.clk && blockIdx.x == (gridDim.x * 5) / 8 && tid == 0;
  if (probe) { p.clk[0] = __builtin_amdgcn_s_memtime(); p.clk[1] = __builtin_amdgcn_s_memrealtime(); }

  // stage (th, u): u < 2: sub-stages 2 u, 2 u + 1 of half tile th's up rows (piece j: sub-stage j >> 1, hi / lo image j & 1: this wave's
  // KiB of that 4 KiB run); u == 2: the down block of k-step th (this wave's 4 KiB of it).  Requests past the end repeat the last stage.
  auto issue_rel = [&](int th, auto off_, int j) {
    constexpr int off = decltype(off_)::value, u = off % UNIT;
    const int tt = min(th + off / UNIT, T2 - 1);                 // (past the end: the same kind of stage of the last half tile, never read)
    char* slot = smem + ((th * UNIT + off) % NSTG) * STG;
    const char* src;
    char* dst;
    if constexpr (u < 2) {
      src = p.Wu + ((size_t)(tt >> 1) * (NC / 2) + 2 * u + (j >> 1)) * STG + (j & 1) * IMG + (tt & 1) * HALF + wid * 1024 + lane * 16;
      dst = slot + (j >> 1) * SUB + (j & 1) * HALF + wid * 1024;
    } else {
      src = p.Wd + (size_t)tt * STG + wid * (PB * 1024) + j * 1024 + lane * 16;
      dst = slot + wid * (PB * 1024) + j * 1024;
    }
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };

  // ---- this wave's 32 rows -> a0..a63 (hi / lo fragments of the normalised, scaled row; OUTP: of the attention row as it is) --------------
  const int row = pn.row(wid * 32 + l31);
  const bool ok = row < p.M;
  const int rowc = ok ? row : p.M - 1;
  float rs = 1.f;
  f32x4 xres[OUTP ? NOB : 1][4];                       // OUTP: x of the lane's row in the C layout (features 32 ob + 8 g + 4 lh + 0..3)
  if constexpr (OUTP) {
    const float* xr = p.X + (size_t)rowc * K + 4 * lh;
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) xres[ob][g] = *reinterpret_cast<const f32x4*>(xr + 32 * ob + 8 * g);
  }
  {
    char* stage = smem + wid * STG;
    char* scl = smem + NSTG * STG + wid * SCL;
    const int r_first = min(pn.row(wid * 32), p.M - 1), r_last = min(pn.row(wid * 32 + 31), p.M - 1);
    const bool uni = p.scale_stride == 0 || r_first / p.rows_per_sample == r_last / p.rows_per_sample;
    if (uni) {
      const char* ssrc = reinterpret_cast<const char*>(p.scale + (size_t)(r_first / p.rows_per_sample) * p.scale_stride);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ssrc + (lane * 16) % (K * 4)),
                                       (__attribute__((address_space(3))) void*)scl, 16, 0, 0);
    }
    const float* sp = p.scale + (size_t)(rowc / p.rows_per_sample) * p.scale_stride + 8 * lh;
    const float* spl = reinterpret_cast<const float*>(scl) + 8 * lh;
    float ssq = 0.f;
    if constexpr (!Panel::ATT_LDS) {
#pragma unroll
      for (int i = 0; i < PIECES; ++i) {
        const int ci = i * 64 + lane, rr = ci / CPR, qs = ci % CPR;
        const int grow = min(pn.row(wid * 32 + rr), p.M - 1);
        const char* src = reinterpret_cast<const char*>((OUTP ? p.Att : p.X) + (size_t)grow * K) + ((qs ^ (rr & 15)) << 4);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(stage + i * 1024), 16, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* rowp = stage + l31 * (K * 4);
    static_for<NC / 4>([&](auto c4_) {
      constexpr int c0 = 4 * decltype(c4_)::value;
      f32x4 x0[4], x1[4], s0[4], s1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = 4 * (c0 + u) + 2 * lh;
        x0[u] = *reinterpret_cast<const f32x4*>(rowp + ((q ^ (l31 & 15)) << 4));
        x1[u] = *reinterpret_cast<const f32x4*>(rowp + (((q + 1) ^ (l31 & 15)) << 4));
        if constexpr (!OUTP) {
          if (uni) {
            s0[u] = *reinterpret_cast<const f32x4*>(spl + 16 * (c0 + u));
            s1[u] = *reinterpret_cast<const f32x4*>(spl + 16 * (c0 + u) + 4);
          } else {
            s0[u] = *reinterpret_cast<const f32x4*>(sp + 16 * (c0 + u));
            s1[u] = *reinterpret_cast<const f32x4*>(sp + 16 * (c0 + u) + 4);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      static_for<4>([&](auto u_) {
        constexpr int u = decltype(u_)::value;
        u32x4 hi, lo;
        if constexpr (OUTP) {
          split8(x0[u], x1[u], hi, lo);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) ssq = fmaf(x0[u][e], x0[u][e], fmaf(x1[u][e], x1[u][e], ssq));
          split8(x0[u] * s0[u], x1[u] * s1[u], hi, lo);
        }
        areg_write4_lo<8 * (c0 + u)>(hi);
        areg_write4_lo<8 * (c0 + u) + 4>(lo);
      });
      __builtin_amdgcn_sched_barrier(0);
    });
    if constexpr (!OUTP) {
      ssq += __shfl_xor(ssq, 32, 64);
      rs = rsqrtf(ssq / (float)K + p.eps);
    }
  }
  if constexpr (OUTP) {                                // the output accumulators start from x
    static_for<NOB>([&](auto ob_) {
      static_for<4>([&](auto g_) {
        constexpr int ob = decltype(ob_)::value, gq = decltype(g_)::value;
        areg_write4_lo<AO + 16 * ob + 4 * gq>(__builtin_bit_cast(u32x4, xres[ob][gq]));
      });
    });
  } else {
    static_for<NOB>([&](auto ob_) { areg_zero16_lo<AO + 16 * decltype(ob_)::value>(); });
  }
  warm_end();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  KD_BARRIER();                                        // every wave has taken its rows out of the slot it borrowed
  // OUTP: the stream starts with the 4 stages of Wo ([128 out rows][32 k] hi | lo, plain layout); the block's own stages follow in the same
  // ring positions as without it (4 stages = once round the ring)
  auto issue_wo = [&](int q, int j) {
    const char* src = p.Wo + (size_t)q * STG + wid * (PB * 1024) + j * 1024 + lane * 16;
    char* dst = smem + (q % NSTG) * STG + wid * (PB * 1024) + j * 1024;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };
  if constexpr (OUTP) {
#pragma unroll
    for (int q = 0; q < PDIST; ++q)
#pragma unroll
      for (int j = 0; j < PB; ++j) issue_wo(q, j);
  } else {
    static_for<PDIST>([&](auto s_) {
#pragma unroll
      for (int j = 0; j < PB; ++j) issue_rel(0, s_, j);
    });
  }
  if (probe) p.clk[4] = __builtin_amdgcn_s_memtime();

  const int o0 = swz64(l31, lh), o1 = swz64(l31, 2 + lh);
  f32x16 acc[2];
  bf16x8 uh[2][2], ul[2][2];                           // up: [chunk parity][value / gate block]
  bf16x8 dh[2][4], dl[2][4];                           // down: [hidden chunk][output block]
  // chunk cc (0..3) of an up stage: sub-stage cc >> 1, 16-k chunk cc & 1 of it; rows 32 j + l31 of the half tile's 64
  auto read_up = [&](int slot, int cc, bf16x8 (&fh)[2], bf16x8 (&fl)[2]) {
    const char* st = smem + slot * STG + (cc >> 1) * SUB + ((cc & 1) ? o1 : o0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      fh[j] = *reinterpret_cast<const bf16x8*>(st + j * 32 * 64);
      fl[j] = *reinterpret_cast<const bf16x8*>(st + HALF + j * 32 * 64);
    }
  };
  auto read_dn = [&](int slot, int h, bf16x8 (&fh)[4], bf16x8 (&fl)[4]) {
    const char* st = smem + slot * STG + (h ? o1 : o0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fh[j] = *reinterpret_cast<const bf16x8*>(st + j * 32 * 64);
      fl[j] = *reinterpret_cast<const bf16x8*>(st + IMG + j * 32 * 64);
    }
  };
  auto next_stage_in = [&]() {
    wait_vm(PB * (PDIST - 2));
    KD_BARRIER();
  };
  constexpr std::integral_constant<int, 0> I0{};
  constexpr std::integral_constant<int, 1> I1{};
  constexpr std::integral_constant<int, 2> I2{};
  constexpr std::integral_constant<int, 3> I3{};
  wait_vm(PB * (PDIST - 1));
  KD_BARRIER();
  if constexpr (OUTP) {
    // ================= out projection: x (in the output accumulators) += att Wo^T, 4 stages of 24 MFMAs ===================================
    read_dn(0, 0, dh[0], dl[0]);
    static_for<4>([&](auto q_) {
      constexpr int q = decltype(q_)::value;
      auto oo = [&](auto b_, auto j_, bool w_lo, auto al_) {
        constexpr int b = decltype(b_)::value, j = decltype(j_)::value, al = decltype(al_)::value, c = 2 * q + b;
        mfma_acc_aa_lo<AO + 16 * j, 8 * c + 4 * al>(w_lo ? dl[b][j] : dh[b][j]);
      };
      auto request = [&](int j) {                      // stage q + 3 of the stream: Wo's last stage, then the block's first three
        if constexpr (q == 0) issue_wo(3, j);
        else issue_rel(0, std::integral_constant<int, (q > 0 ? q - 1 : 0)>{}, j);
      };
      oo(I0, I0, true, I0);
      __builtin_amdgcn_sched_barrier(0);
      read_dn(q % NSTG, 1, dh[1], dl[1]);
      __builtin_amdgcn_sched_barrier(0);
      oo(I0, I1, true, I0); oo(I0, I2, true, I0); oo(I0, I3, true, I0);
      oo(I0, I0, false, I1); oo(I0, I1, false, I1); oo(I0, I2, false, I1); oo(I0, I3, false, I1);
      oo(I0, I0, false, I0); oo(I0, I1, false, I0); oo(I0, I2, false, I0); oo(I0, I3, false, I0);
      __builtin_amdgcn_sched_barrier(0);
      next_stage_in();
      oo(I1, I0, true, I0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (q < 3) read_dn((q + 1) % NSTG, 0, dh[0], dl[0]);
      else read_up(0, 0, uh[0], ul[0]);
      __builtin_amdgcn_sched_barrier(0);
      oo(I1, I1, true, I0); oo(I1, I2, true, I0);
      request(0);
      __builtin_amdgcn_sched_barrier(0);
      oo(I1, I3, true, I0); oo(I1, I0, false, I1); oo(I1, I1, false, I1);
      request(1);
      __builtin_amdgcn_sched_barrier(0);
      oo(I1, I2, false, I1); oo(I1, I3, false, I1); oo(I1, I0, false, I0);
      request(2);
      __builtin_amdgcn_sched_barrier(0);
      oo(I1, I1, false, I0); oo(I1, I2, false, I0);
      request(3);
      oo(I1, I3, false, I0);
      __builtin_amdgcn_sched_barrier(0);
    });
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");  // asm MFMA results -> v_accvgpr_read
    // ---- new x (C layout, still in the accumulators) -> AdaRMSNorm statistics, scale, hi / lo fragments in the k order of pack layout 3:
    // chunk 2 ob + hc of the row = registers 8 hc .. + 7 of output block ob -----------------------------------------------------------
    {
      const char* scl = smem + NSTG * STG + wid * SCL;
      const int r_first = min(pn.row(wid * 32), p.M - 1), r_last = min(pn.row(wid * 32 + 31), p.M - 1);
      const bool uni = p.scale_stride == 0 || r_first / p.rows_per_sample == r_last / p.rows_per_sample;
      const float* sg = uni ? nullptr : p.scale + (size_t)(rowc / p.rows_per_sample) * p.scale_stride + 4 * lh;
      const float* sl = reinterpret_cast<const float*>(scl) + 4 * lh;
      float ssq = 0.f;
      static_for<NOB>([&](auto ob_) {
        constexpr int ob = decltype(ob_)::value;
        f32x4 v[4], sc[4];
        static_for<4>([&](auto g_) { v[decltype(g_)::value] = areg_read4<AO + 16 * ob + 4 * decltype(g_)::value>(); });
#pragma unroll
        for (int g = 0; g < 4; ++g) sc[g] = uni ? *reinterpret_cast<const f32x4*>(sl + 32 * ob + 8 * g) : *reinterpret_cast<const f32x4*>(sg + 32 * ob + 8 * g);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) ssq = fmaf(v[g][e], v[g][e], ssq);
        static_for<2>([&](auto hc_) {
          constexpr int hc = decltype(hc_)::value;
          u32x4 hi, lo;
          split8(v[2 * hc] * sc[2 * hc], v[2 * hc + 1] * sc[2 * hc + 1], hi, lo);
          areg_write4_lo<8 * (2 * ob + hc)>(hi);
          areg_write4_lo<8 * (2 * ob + hc) + 4>(lo);
        });
      });
      ssq += __shfl_xor(ssq, 32, 64);
      rs = rsqrtf(ssq / (float)K + p.eps);
    }
  } else {
    read_up(0, 0, uh[0], ul[0]);
  }
  const float rsh = 0.5f * rs;
  for (int th = 0; th < T2; ++th) {
    const int slot0 = (th * UNIT) % NSTG;
    if (probe && th == 4) p.clk[8] = __builtin_amdgcn_s_memtime();
    // ================= up projection of the half tile: value / gate accumulators of its 32 hidden features (2 stages of 4 chunks) ==========
    static_for<2>([&](auto u_) {
      constexpr int u = decltype(u_)::value;
      const int slot = (slot0 + u) % NSTG, nslot = (slot0 + u + 1) % NSTG;
      // the 6 MFMAs of chunk cc: (w_lo x a_hi), (w_hi x a_lo), (w_hi x a_hi) for the value block and the gate block in alternation
      auto mm = [&](auto cc_, auto i_) {
        constexpr int cc = decltype(cc_)::value, i = decltype(i_)::value, j = i & 1, term = i >> 1, c = 4 * u + cc;
        const bf16x8& w = term == 0 ? ul[cc & 1][j] : uh[cc & 1][j];
        constexpr int al = term == 1;
        if constexpr (c == 0 && term == 0) mfma_ag0<8 * c + 4 * al>(acc[j], w);      // first MFMA of the chain: C = 0
        else mfma_ag<8 * c + 4 * al>(acc[j], w);
      };
      constexpr std::integral_constant<int, 4> I4{};
      constexpr std::integral_constant<int, 5> I5{};
      // chunk 0
      mm(I0, I0);
      __builtin_amdgcn_sched_barrier(0);
      read_up(slot, 1, uh[1], ul[1]);
      __builtin_amdgcn_sched_barrier(0);
      mm(I0, I1); mm(I0, I2); mm(I0, I3); mm(I0, I4); mm(I0, I5);
      // chunk 1
      mm(I1, I0);
      __builtin_amdgcn_sched_barrier(0);
      read_up(slot, 2, uh[0], ul[0]);
      __builtin_amdgcn_sched_barrier(0);
      mm(I1, I1); mm(I1, I2); mm(I1, I3); mm(I1, I4); mm(I1, I5);
      __builtin_amdgcn_sched_barrier(0);
      next_stage_in();
      // chunk 2
      mm(I2, I0);
      __builtin_amdgcn_sched_barrier(0);
      read_up(slot, 3, uh[1], ul[1]);
      __builtin_amdgcn_sched_barrier(0);
      mm(I2, I1); mm(I2, I2);
      issue_rel(th, std::integral_constant<int, u + PDIST>{}, 0);
      __builtin_amdgcn_sched_barrier(0);
      mm(I2, I3); mm(I2, I4); mm(I2, I5);
      issue_rel(th, std::integral_constant<int, u + PDIST>{}, 1);
      __builtin_amdgcn_sched_barrier(0);
      // chunk 3
      mm(I3, I0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (u == 0) read_up(nslot, 0, uh[0], ul[0]);
      else read_dn(nslot, 0, dh[0], dl[0]);
      __builtin_amdgcn_sched_barrier(0);
      mm(I3, I1); mm(I3, I2);
      issue_rel(th, std::integral_constant<int, u + PDIST>{}, 2);
      __builtin_amdgcn_sched_barrier(0);
      mm(I3, I3); mm(I3, I4);
      issue_rel(th, std::integral_constant<int, u + PDIST>{}, 3);
      mm(I3, I5);
      __builtin_amdgcn_sched_barrier(0);
    });
    asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]));      // asm MFMA results -> vector reads
    if (probe && th == 4) p.clk[9] = __builtin_amdgcn_s_memtime();

    // ================= GEGLU in the lane that owns the row -> hi / lo fragments of the half tile's 2 hidden 16-chunks =====================
    bf16x8 hf_hi[2], hf_lo[2];
#pragma unroll
    for (int hc = 0; hc < 2; ++hc) {
      f32x4 v0, v1;
      const int r0 = 8 * hc;
      {
        const f32x2 a = geglu_pair(f32x2{acc[0][r0], acc[0][r0 + 1]} * rsh, f32x2{acc[1][r0], acc[1][r0 + 1]} * rs);
        const f32x2 b = geglu_pair(f32x2{acc[0][r0 + 2], acc[0][r0 + 3]} * rsh, f32x2{acc[1][r0 + 2], acc[1][r0 + 3]} * rs);
        v0 = f32x4{a.x, a.y, b.x, b.y};
      }
      {
        const f32x2 a = geglu_pair(f32x2{acc[0][r0 + 4], acc[0][r0 + 5]} * rsh, f32x2{acc[1][r0 + 4], acc[1][r0 + 5]} * rs);
        const f32x2 b = geglu_pair(f32x2{acc[0][r0 + 6], acc[0][r0 + 7]} * rsh, f32x2{acc[1][r0 + 6], acc[1][r0 + 7]} * rs);
        v1 = f32x4{a.x, a.y, b.x, b.y};
      }
      u32x4 hi, lo;
      split8(v0, v1, hi, lo);
      hf_hi[hc] = __builtin_bit_cast(bf16x8, hi);
      hf_lo[hc] = __builtin_bit_cast(bf16x8, lo);
    }
    asm volatile("s_nop 7" : "+v"(hf_hi[0]), "+v"(hf_hi[1]), "+v"(hf_lo[0]), "+v"(hf_lo[1]));   // vector-written fragments -> asm MFMA operands
    __builtin_amdgcn_sched_barrier(0);
    if (probe && th == 4) p.clk[10] = __builtin_amdgcn_s_memtime();

    // ================= down projection: the half tile's 32 hidden features into the row's 128 output features (1 stage) ===================
    {
      const int slot = (slot0 + 2) % NSTG, nslot = (slot0 + 3) % NSTG;
      auto dd = [&](auto b_, auto j_, bool w_lo, bool h_lo) {
        constexpr int b = decltype(b_)::value, j = decltype(j_)::value;
        const bf16x8& w = w_lo ? dl[b][j] : dh[b][j];
        const bf16x8& h = h_lo ? hf_lo[b] : hf_hi[b];
        mfma_acc_ag_lo<AO + 16 * j>(w, h);
      };
      dd(I0, I0, true, false);
      __builtin_amdgcn_sched_barrier(0);
      read_dn(slot, 1, dh[1], dl[1]);
      __builtin_amdgcn_sched_barrier(0);
      dd(I0, I1, true, false); dd(I0, I2, true, false); dd(I0, I3, true, false);
      dd(I0, I0, false, true); dd(I0, I1, false, true); dd(I0, I2, false, true); dd(I0, I3, false, true);
      dd(I0, I0, false, false); dd(I0, I1, false, false); dd(I0, I2, false, false); dd(I0, I3, false, false);
      __builtin_amdgcn_sched_barrier(0);
      next_stage_in();
      dd(I1, I0, true, false);
      __builtin_amdgcn_sched_barrier(0);
      read_up(nslot, 0, uh[0], ul[0]);
      __builtin_amdgcn_sched_barrier(0);
      dd(I1, I1, true, false); dd(I1, I2, true, false);
      issue_rel(th, std::integral_constant<int, 2 + PDIST>{}, 0);
      __builtin_amdgcn_sched_barrier(0);
      dd(I1, I3, true, false); dd(I1, I0, false, true); dd(I1, I1, false, true);
      issue_rel(th, std::integral_constant<int, 2 + PDIST>{}, 1);
      __builtin_amdgcn_sched_barrier(0);
      dd(I1, I2, false, true); dd(I1, I3, false, true); dd(I1, I0, false, false);
      issue_rel(th, std::integral_constant<int, 2 + PDIST>{}, 2);
      __builtin_amdgcn_sched_barrier(0);
      dd(I1, I1, false, false); dd(I1, I2, false, false);
      issue_rel(th, std::integral_constant<int, 2 + PDIST>{}, 3);
      dd(I1, I3, false, false);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (probe && th == 4) p.clk[11] = __builtin_amdgcn_s_memtime();
  }
  if (probe) p.clk[12] = __builtin_amdgcn_s_memtime();

  // ---- + x, store (as above) -------------------------------------------------------------------------------------------------------------
  char* strip = smem + NSTG * STG + 4 * SCL + wid * 2048;
  float* st_row[2];
  const float* sk_row[2];
  bool st_ok[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int r = pn.row(wid * 32 + 16 * it + (lane >> 2));
    st_ok[it] = r < p.M;
    st_row[it] = p.Y + (size_t)min(r, p.M - 1) * K + 4 * (lane & 3);
    sk_row[it] = p.X + (size_t)min(r, p.M - 1) * K + 4 * (lane & 3);
  }
  f32x4 skip_all[NOB][2][2];                           // (OUTP: the accumulators started from x: nothing to add)
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int it = 0; it < 2; ++it)
        skip_all[ob][hb][it] = OUTP ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(sk_row[it] + 32 * ob + 16 * hb);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 3" ::: "memory");       // tail LDS-DMA drained; last MFMA results readable
  static_for<NOB>([&](auto ob_) {
    constexpr int ob = decltype(ob_)::value;
    f32x4 blk[4];
    static_for<4>([&](auto g_) { blk[decltype(g_)::value] = areg_read4<AO + 16 * ob + 4 * decltype(g_)::value>(); });
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      const f32x4 (&skip)[2] = skip_all[ob][hb];
#pragma unroll
      for (int gg = 0; gg < 2; ++gg)
        *reinterpret_cast<f32x4*>(strip + l31 * 64 + (((2 * gg + lh) ^ ((l31 >> 2) & 1)) << 4)) = blk[2 * hb + gg];
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int r16 = 16 * it + (lane >> 2), c = lane & 3;
        const f32x4 o = *reinterpret_cast<const f32x4*>(strip + r16 * 64 + ((c ^ ((r16 >> 2) & 1)) << 4));
        if (st_ok[it]) st16(st_row[it] + 32 * ob + 16 * hb, f32x4(o + skip[it]));
      }
    }
  });
  if (probe) { p.clk[2] = __builtin_amdgcn_s_memtime(); p.clk[3] = __builtin_amdgcn_s_memrealtime(); p.clk[7] = (unsigned long long)(T2 * UNIT); }
}

}  // namespace x3
}  // namespace kd
