// bf16-mode GEMMs of the HDiT denoiser for gfx950 (see bf16_common.h for the operand formats and the swapped product).
//
// What shapes these kernels (measured: profiles/r02_pipe_overlap.md, r02_harness_*.log): a SIMD issues no vector instruction
// while it runs an MFMA (time = MFMA passes + vector issue slots + unhidden waits, so the COUNT of vector instructions per MFMA
// matters, not their placement); LDS fragment reads hide behind MFMAs; HBM gives 5.0-5.6 TB/s to a pure stream and the level-0
// shapes (131 072 rows, K = 128 / 384) are bound by it; L2 -> LDS through global_load_lds sustains 39-52 bytes / clock / CU.
//
//   wstat  "W-stationary": a persistent workgroup per CU parks its slice of the packed weight (<= 144 KiB) in LDS ONCE; its waves
//          then walk 32-row chunks of A independently: the chunk goes HBM -> registers as MFMA B-operand fragments (RMS statistics
//          and the AdaRMSNorm scale applied on the way), every weight fragment comes from LDS, the epilogue runs in the lane that
//          owns the row (no LDS, no cross-lane traffic but one half-wave exchange) and stores 16 bytes per lane.  After the
//          initial weight copy there is NO barrier and no counted wait: the 8 waves of a CU sit in different phases, so one wave's
//          memory waits are covered by the others' MFMA / epilogue work.
//   (astat / tiled forms for the deeper levels follow below.)
#include "bf16_common.h"

namespace kd {
namespace b16 {

struct GArgs {
  const u16* A; const char* Wp; u16* C; const u16* R;
  const float* scale; int scale_stride, rows_per_sample; float eps;
  int M, N;                 // N = output width (GEGLU: d_ff)
  int n_tiles;              // packed n-tiles in total
  int tiles_per_slice, n_slices;
  int n_heads; const float* qk_scale; const float* pos; const float* freq;
  unsigned long long* clk;  // kd_prof_clock_buffer: {s_memtime, s_memrealtime} at entry and exit of workgroup 0 (shader clock under load)
  int warm;                 // code warm-up workgroups (kd_common.h code_warm_begin; option "code_warm")
};

// ------------------------------------------------------------------------------------------------------------------
// wstat
// Every wave walks a CONTIGUOUS range of chunks (same sample for most consecutive chunks: the scale vector stays in L1).
// Next-chunk prefetch, software-pipelined tiles and 4 / 12 waves were measured and retired (profiles/r02_wstat_ablation.md: the
// first two level within noise, the last two slower).
constexpr int NW = 8;       // waves per workgroup: 2 per SIMD, up to 256 registers each
template <int NC /* K / 16 */, int EPI, bool NORM>
__global__ __launch_bounds__(NW * 64) void gemm_wstat_kernel(const GArgs p) {
  constexpr int K = NC * 16, NK = NC / 4;
  constexpr bool GEGLU = EPI == KD_EPI_GEGLU;
  constexpr int NCOL = GEGLU ? 64 : 128;
  static_assert(NC % 4 == 0, "K must be a multiple of 64");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const auto warm = code_warm_begin<((EPI == KD_EPI_QKV || EPI == KD_EPI_GEGLU) ? 8 : 4) * 1024>((int)blockIdx.x < p.warm && tid < 64);
  const int slice = blockIdx.x % p.n_slices, grp = blockIdx.x / p.n_slices, ngrp = gridDim.x / p.n_slices;
  const int nt0 = slice * p.tiles_per_slice;
  const int ntn = min(p.tiles_per_slice, p.n_tiles - nt0);
  if (p.clk && blockIdx.x == 0 && tid == 0) { p.clk[0] = __builtin_amdgcn_s_memtime(); p.clk[1] = __builtin_amdgcn_s_memrealtime(); }

  // ---- park this slice of the packed weight in LDS (lane-linear copy, 1 KiB per wave-instruction) --------------------------
  {
    const char* src = p.Wp + (size_t)nt0 * NK * WBLK + lane * 16;
    const int bytes = ntn * NK * WBLK;
    for (int off = wid * 1024; off < bytes; off += NW * 1024)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + off),
                                       (__attribute__((address_space(3))) void*)(smem + off), 16, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    code_warm_end(warm);
    __syncthreads();
  }

  // per-lane constants of the weight fragment reads: row l31 of a 32-row block, chunk 2*cc + lh of the 64-k step
  int off4[4];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) off4[cc] = swz128(l31, 2 * cc + lh);

  const int chunks = (p.M + 31) >> 5;
  const int nwaves = ngrp * NW, cpw = (chunks + nwaves - 1) / nwaves;
  const int ch0 = (grp * NW + wid) * cpw, ch1 = min(ch0 + cpw, chunks);
  auto load_raw = [&](int ch, u32x4 (&raw)[NC]) {
    const u32x4* ap = reinterpret_cast<const u32x4*>(p.A + (size_t)min(ch * 32 + l31, p.M - 1) * K + 8 * lh);
#pragma unroll
    for (int c = 0; c < NC; ++c) raw[c] = ap[2 * c];
  };
  for (int ch = ch0; ch < ch1; ++ch) {
    const int row = ch * 32 + l31;
    const bool ok = row < p.M;
    const int rowc = ok ? row : p.M - 1;

    // ---- this lane's row of A -> B-operand fragments: chunk c holds k = 16c + 8lh .. +7 --------------------------------------
    bf16x8 a[NC];
    float rs = 1.0f;
    {
      u32x4 raw[NC];
      load_raw(ch, raw);
      if (NORM) {
        const int b = rowc / p.rows_per_sample;
        const float* sp = p.scale + (size_t)b * p.scale_stride + 8 * lh;
        float ssq = 0.f;
        // the scale vector in groups of 8 chunks, every load of a group requested before the first is used (one L2 round trip
        // per group instead of one per chunk)
#pragma unroll
        for (int c0 = 0; c0 < NC; c0 += 8) {
          f32x4 s0[8], s1[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            s0[u] = *reinterpret_cast<const f32x4*>(sp + 16 * (c0 + u));
            s1[u] = *reinterpret_cast<const f32x4*>(sp + 16 * (c0 + u) + 4);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int c = c0 + u;
            float x[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[2 * e] = bf_lo(raw[c][e]); x[2 * e + 1] = bf_hi(raw[c][e]); }
#pragma unroll
            for (int e = 0; e < 8; ++e) ssq = fmaf(x[e], x[e], ssq);
            u32x4 o = {pack_bf16(x[0] * s0[u][0], x[1] * s0[u][1]), pack_bf16(x[2] * s0[u][2], x[3] * s0[u][3]),
                       pack_bf16(x[4] * s1[u][0], x[5] * s1[u][1]), pack_bf16(x[6] * s1[u][2], x[7] * s1[u][3])};
            asm volatile("" : "+v"(o));    // materialise the fragment here (see the astat kernel)
            a[c] = __builtin_bit_cast(bf16x8, o);
          }
        }
        ssq += __shfl_xor(ssq, 32, 64);
        rs = rsqrtf(ssq / (float)K + p.eps);
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] = __builtin_bit_cast(bf16x8, raw[c]);
      }
    }
    float py = 0.f, px = 0.f;
    if (EPI == KD_EPI_QKV) {
      const int tok = rowc % p.rows_per_sample;
      py = p.pos[2 * tok];
      px = p.pos[2 * tok + 1];
    }

    // ---- the tiles of this slice.  mma(t): products of tile t into the accumulators; epi(t): its epilogue, in the lane
    // that owns the row.
    u16* crow = p.C + (size_t)rowc * p.N;
    auto mma = [&](int t, f32x16 (&acc)[4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
      const char* wt = smem + (size_t)t * NK * WBLK;
      // weight fragments of chunk c + 1 are requested before the 4 MFMAs of chunk c (explicit double buffer)
      bf16x8 wf[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[0][j] = *reinterpret_cast<const bf16x8*>(wt + off4[0] + j * 32 * 128);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c + 1 < NC) {
          const char* wk = wt + ((c + 1) >> 2) * WBLK + off4[(c + 1) & 3];
#pragma unroll
          for (int j = 0; j < 4; ++j) wf[(c + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(wk + j * 32 * 128);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[c & 1][j], a[c], acc[j], 0, 0, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int c = 0; c + 1 < NC; ++c) {
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    };
    auto epi = [&](int t, f32x16 (&acc)[4], u32x4 (&rraw)[4][2]) {
      const int n0 = (nt0 + t) * NCOL;
      const bool st_ok = ok;
      if (GEGLU) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          float v[16];
          geglu_block(acc[2 * jj], acc[2 * jj + 1], rs, v);
          const int nb = n0 + 32 * jj;
          store_block_bf16(crow + min(nb, p.N - 32), v, lh, st_ok && nb < p.N);
        }
      } else if (EPI == KD_EPI_QKV) {
#pragma unroll
        for (int vv = 0; vv < 2; ++vv) {
          const int vec = (n0 >> 6) + vv;                       // (q|k|v, head) vector index of these 64 columns
          const int which = vec / p.n_heads, head = vec - which * p.n_heads;
          if (which < 2) {
            float fr[4], qsc;
            KD_HEAD_CONSTS(p.freq, p.qk_scale, head, lh, fr, qsc)
            qk_prep_blocks(acc[2 * vv], acc[2 * vv + 1], rs, sqrtf(qsc), p.eps, py, px, fr);
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[2 * vv][r] *= rs; acc[2 * vv + 1][r] *= rs; }
          }
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc[2 * vv + jj][r];
            store_block_bf16(crow + n0 + 64 * vv + 32 * jj, v, lh, st_ok);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int nb = n0 + 32 * j;
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = acc[j][r] * rs;
          if (EPI == KD_EPI_RESIDUAL) {
            float rr[16];
            block_from_raw(rraw[j], rr);
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] += rr[r];
          }
          store_block_bf16(crow + min(nb, p.N - 32), v, lh, st_ok && nb < p.N);
        }
      }
    };
    u32x4 rraw[4][2];
    for (int t = 0; t < ntn; ++t) {
      if (EPI == KD_EPI_RESIDUAL) {      // residual operand of this tile, requested before the products
        const int n0 = (nt0 + t) * NCOL;
#pragma unroll
        for (int j = 0; j < 4; ++j) load_block_raw(p.R + (size_t)rowc * p.N + min(n0 + 32 * j, p.N - 32), rraw[j], lh);
      }
      f32x16 acc[4];
      mma(t, acc);
      epi(t, acc, rraw);
    }
  }
  if (p.clk && blockIdx.x == 0 && tid == 0) { p.clk[2] = __builtin_amdgcn_s_memtime(); p.clk[3] = __builtin_amdgcn_s_memrealtime(); }
}

unsigned long long* g_clk = nullptr;


constexpr int WSTAT_LDS_MAX = 144 * 1024;

template <int NC, int EPI, bool NORM>
static int launch_wstat(const GArgs& a, int lds, const char* nm, double flops, double bytes, hipStream_t s) {
  const int chunks = (a.M + 31) / 32;
  int groups = cu_count() / a.n_slices;
  if (groups < 1) groups = 1;
  const int need = (chunks + NW - 1) / NW;
  if (groups > need) groups = need;
  const CfgName cfg(nm, "waves%d,pf0,slices%d", NW, a.n_slices);
  LaunchScope prof(cfg, flops, bytes, s);
  launch_max_lds<gemm_wstat_kernel<NC, EPI, NORM>>(WSTAT_LDS_MAX, dim3((unsigned)(groups * a.n_slices)), dim3(NW * 64), lds, s, a);
  return check_launch("kd_gemm_bf16(wstat)");
}

// Eligibility + dispatch.  Returns 1 if the descriptor was not taken.
int gemm_wstat_try(const KdGemm& d, hipStream_t s, int* rc) {
  if (d.a_mode != KD_A_PLAIN || !d.Wp || !opt(KD_OPT_wstat)) return 1;
  if (d.epi != KD_EPI_STORE && d.epi != KD_EPI_QKV && d.epi != KD_EPI_GEGLU && d.epi != KD_EPI_RESIDUAL) return 1;
  if (d.K != 128 && d.K != 256 && d.K != 384 && d.K != 512) return 1;
  if ((d.N & 31) || d.M < 2048) return 1;
  if (d.epi == KD_EPI_RESIDUAL && d.norm) return 1;
  if (d.epi != KD_EPI_RESIDUAL && !d.norm && d.epi != KD_EPI_STORE) return 1;
  if (d.epi == KD_EPI_STORE && d.out_add != 0.f) return 1;
  if ((d.norm || d.epi == KD_EPI_QKV) && (d.rows_per_sample <= 0 || (d.rows_per_sample & 31))) return 1;   // a 32-row chunk = one sample
  const bool geglu = d.epi == KD_EPI_GEGLU;
  const int ncol = geglu ? 64 : 128;
  if (d.epi == KD_EPI_QKV && (d.N & 127)) return 1;
  const int n_tiles = (d.N + ncol - 1) / ncol, nk = d.K / 64;
  const int max_tiles = WSTAT_LDS_MAX / (nk * WBLK);
  if (max_tiles < 1) return 1;
  const int n_slices = (n_tiles + max_tiles - 1) / max_tiles;
  // every slice re-reads (and, with a norm, re-normalises) A: mostly L2 / MALL hits, cheap next to a weight ring with barriers,
  // but a slice count near the CU count leaves too few row groups
  if (n_slices > opt(KD_OPT_wstat_max_slices) || n_slices * 4 > cu_count()) return 1;
  const int tps = (n_tiles + n_slices - 1) / n_slices;
  GArgs a{};
  a.A = reinterpret_cast<const u16*>(d.A); a.Wp = reinterpret_cast<const char*>(d.Wp);
  a.C = reinterpret_cast<u16*>(d.C); a.R = reinterpret_cast<const u16*>(d.R);
  a.scale = d.scale; a.scale_stride = d.scale_stride; a.rows_per_sample = d.rows_per_sample > 0 ? d.rows_per_sample : d.M; a.eps = d.eps;
  a.M = d.M; a.N = d.N; a.n_tiles = n_tiles; a.tiles_per_slice = tps; a.n_slices = n_slices;
  a.n_heads = d.n_heads; a.qk_scale = d.qk_scale; a.pos = d.rope_pos; a.freq = d.rope_freq;
  a.clk = g_clk;
  a.warm = code_warm();
  const int lds = tps * nk * WBLK;
  const double n_eff = geglu ? 2.0 * d.N : (double)d.N;
  const double flops = 2.0 * d.M * n_eff * d.K;
  const double bytes = 2.0 * ((double)d.M * d.K + n_eff * d.K + (double)d.M * d.N) + (d.epi == KD_EPI_RESIDUAL ? 2.0 * d.M * d.N : 0.0);
  const ProfName nm("gemm_wstat", "gemm_bf16_wstat<e%d,n%d> M=%d N=%d K=%d", d.epi, d.norm, d.M, d.N, d.K);
#define KD_WS(NCV, EP, NO) { *rc = launch_wstat<NCV, EP, NO>(a, lds, nm, flops, bytes, s); return 0; }
#define KD_WS_ALL(NCV)                                                       \
  {                                                                          \
    if (d.epi == KD_EPI_QKV) KD_WS(NCV, KD_EPI_QKV, true)                    \
    if (d.epi == KD_EPI_GEGLU) KD_WS(NCV, KD_EPI_GEGLU, true)                \
    if (d.epi == KD_EPI_STORE && d.norm) KD_WS(NCV, KD_EPI_STORE, true)      \
    if (d.epi == KD_EPI_STORE) KD_WS(NCV, KD_EPI_STORE, false)               \
    if (d.epi == KD_EPI_RESIDUAL) KD_WS(NCV, KD_EPI_RESIDUAL, false)         \
  }
  if (d.K == 128) KD_WS_ALL(8)
  if (d.K == 256) KD_WS_ALL(16)
  if (d.K == 384) {
    if (d.epi == KD_EPI_RESIDUAL) KD_WS(24, KD_EPI_RESIDUAL, false)
    if (d.epi == KD_EPI_STORE && !d.norm) KD_WS(24, KD_EPI_STORE, false)
  }
  if (d.K == 512) KD_WS_ALL(32)
#undef KD_WS_ALL
#undef KD_WS
  return 1;
}

// ------------------------------------------------------------------------------------------------------------------
// tiled: C tile [128 * BMT rows][128 features] per workgroup, BOTH operands through LDS by global_load_lds (the packed weight
// block verbatim; the activation tile as 8-row x 128-byte pieces whose 16-byte chunks are permuted on the SOURCE side into
// the same swizzled image), K stepped by 64 through a 3-slot ring with one barrier per step (counted vmcnt: the next step's
// pieces stay in flight across it).  The K loop is ds_read + MFMA only.  For the projections whose K is too long to keep a
// row's fragments in registers (down projections, token merges) or whose weight is too large to park (splits).
//   A gather  : plain | 2x2 token merge (a 64-wide k-step lies inside ONE fine token: Cin % 64 == 0)
//   epilogue  : store | + residual | 2x2 token split + lerp(skip)          (all bf16, in the lane that owns the row)
struct TArgs {
  const u16* A; const char* Wp; u16* C; const u16* R; const float* fac;
  int M, N, K, n_tiles_n, nk;
  int gh, gw, cin;
  int warm;                 // code warm-up workgroups (kd_common.h)
};

// DEEP (= LW): 4-slot ring -- for grids of at most one tile per CU (the level-2 shapes: 8192 rows), where the second workgroup of the
// 2-slot form does not exist.  (Without loader waves it measured no better than 2 slots: 10.2 vs 9.5 us, 21.5 vs 21.5; retired.)
// LW (round 4; BMT = 1, DEEP ring, one workgroup per CU): LOADER WAVES as in csrc/gemm_x3r.hip.  The level-2 shapes (8192 rows: one tile per
// CU) ran ~1 800 clocks per 64-wide K step against 512 of MFMA: every wave issued its 8 LDS-DMA requests of the next step in one burst behind
// the barrier, and a wave that is issuing requests issues nothing else.  The kernel needs 114 - 178 of a SIMD's 512 registers per lane, so the
// workgroup carries four more waves that do only the staging (requests, counted vmcnt, the step's barrier); the compute waves' K loop is
// ds_read + MFMA + the one barrier per step.
template <int AMODE, int EPI, int BMT, bool LW = false>
__global__ __launch_bounds__(LW ? 512 : 256 * BMT, BMT == 1 ? 2 : 1) void gemm_tiled_kernel(const TArgs p) {
  static_assert(!LW || BMT == 1, "loader waves: 128-row tiles");
  constexpr bool DEEP = LW;                          // loader waves: 4-slot ring
  constexpr int NWV = 4 * BMT, BMR = 128 * BMT;
  constexpr int A_IMG = BMR * 128, STG = A_IMG + WBLK, NSTG = BMT == 1 ? (DEEP ? 4 : 2) : 3;
  constexpr int WPC = 16 / NWV;                      // weight pieces (1 KiB) per staging wave per step
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid_all = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const bool loader = LW && wid_all >= NWV;          // (wave-uniform)
  const int wid = LW ? (wid_all & (NWV - 1)) : wid_all;      // compute role: position in the tile; staging role: which pieces
  const auto warm = code_warm_begin<(EPI == KD_EPI_SPLIT_LERP ? 6 : 4) * 1024>((int)blockIdx.x < p.warm && tid < 64);
  const int wc = wid & 1, wr = wid >> 1;
  const int tile = KD_XCD_CHUNK();      // XCD-aware order, n fastest: the n-tiles of one row panel run on ONE L2
  const int nt = tile % p.n_tiles_n, mt = tile / p.n_tiles_n;
  const int m0 = mt * BMR, n0 = nt * 128;
  const int K = p.K, nk = p.nk;

  // ---- this lane's 4 activation pieces per step: piece i = 4 * wid + ii covers tile rows 8i .. 8i+7 ----------------------------
  const char* aptr[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const int row = 8 * (4 * wid + ii) + (lane >> 3);
    const int q = (lane & 7) ^ ((row >> 1) & 7);
    const int gm = min(m0 + row, p.M - 1);
    if (AMODE == KD_A_PLAIN) {
      aptr[ii] = reinterpret_cast<const char*>(p.A + (size_t)gm * K) + q * 16;
    } else {      // merged token gm = (b, h, w) of the coarse grid; k = quadrant * cin + e
      const int hw = p.gh * p.gw, b = gm / hw, rr = gm - b * hw, h = rr / p.gw, w = rr - h * p.gw;
      aptr[ii] = reinterpret_cast<const char*>(p.A + (((size_t)b * (2 * p.gh) + 2 * h) * (2 * p.gw) + 2 * w) * p.cin) + q * 16;
    }
  }
  const char* wsrc = p.Wp + (size_t)nt * nk * WBLK + (wid * WPC) * 1024 + lane * 16;
  auto issue = [&](int kt) {
    char* st = smem + (kt % NSTG) * STG;
    size_t koff;
    if (AMODE == KD_A_PLAIN) {
      koff = (size_t)kt * 128;
    } else {
      const int k0 = kt * 64, qd = k0 / p.cin, e0 = k0 - qd * p.cin;
      koff = ((size_t)((qd >> 1) * (2 * p.gw) + (qd & 1)) * p.cin + e0) * 2;
    }
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(aptr[ii] + koff),
                                       (__attribute__((address_space(3))) void*)(st + (4 * wid + ii) * 1024), 16, 0, 0);
#pragma unroll
    for (int j = 0; j < WPC; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + (size_t)kt * WBLK + j * 1024),
                                       (__attribute__((address_space(3))) void*)(st + A_IMG + (wid * WPC + j) * 1024), 16, 0, 0);
  };

  f32x16 acc[2][2];      // [feature block i][row block j]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  int off4[4];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) off4[cc] = swz128(l31, 2 * cc + lh);

  // residual / skip operand of this lane's 4 output blocks: requested two K steps before the end of the loop (raw 16-byte pieces,
  // 32 registers), so that the epilogue does not start with a full memory round trip (8 000 of the workgroup's 37 000 clocks at
  // the level-1 down projection: profiles/r02_astat_timeline.md).  The last step's vmcnt(0) then also covers them.
  constexpr bool HAS_R = EPI == KD_EPI_RESIDUAL || EPI == KD_EPI_SPLIT_LERP;
  u32x4 rraw[2][2][2];
  size_t roff[2][2];
  if (HAS_R) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gmc = min(m0 + wr * 64 + 32 * j + l31, p.M - 1);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int nbc = min(n0 + wc * 64 + 32 * i, p.N - 32);
        if (EPI == KD_EPI_SPLIT_LERP) {
          const int hw = p.gh * p.gw, cout = p.N >> 2;
          const int b = gmc / hw, rr = gmc - b * hw, h = rr / p.gw, w = rr - h * p.gw;
          const int qd = nbc / cout, e = nbc - qd * cout;
          roff[i][j] = (((size_t)b * (2 * p.gh) + 2 * h + (qd >> 1)) * (2 * p.gw) + 2 * w + (qd & 1)) * cout + e;
        } else {
          roff[i][j] = (size_t)gmc * p.N + nbc;
        }
      }
    }
  }
  if constexpr (LW) {
    // The step's barrier sits in the MIDDLE of the step (as in the split3 kernels): behind it step kt + 1 is in LDS and everyone is past
    // step kt - 1, so the compute waves read the next step's first fragments during the last MFMAs of this one -- no LDS round trip is
    // exposed behind a barrier -- while step kt + 2 (requested one barrier earlier) has two more half steps to land.
    if (loader) {
      // ---- loader wave: the requests of its 4 activation pieces and its quarter of the weight block of every step, nothing else ----------
#pragma unroll
      for (int kt = 0; kt < NSTG - 1; ++kt)
        if (kt < nk) issue(kt);
      wait_vm_dyn<40>((4 + WPC) * min(NSTG - 2, nk - 1));            // step 0 in
      KD_BARRIER();
      for (int kt = 0; kt < nk; ++kt) {
        wait_vm_dyn<40>(kt + 2 <= nk - 1 ? 4 + WPC : 0);              // step kt + 1 in; step kt + 2 may stay in flight
        KD_BARRIER();                                            // mid step kt: the compute waves are done with step kt - 1, whose slot takes step kt + 3
        if (kt + NSTG - 1 < nk) issue(kt + NSTG - 1);
      }
      return;                                                    // (every request was waited for: the last wait is vmcnt(0))
    }
    const char* ab0 = smem + (wr * 64) * 128;
    const char* wb0 = smem + A_IMG + (wc * 64) * 128;
    bf16x8 af[2][2], wf[2][2];
    auto read_chunk = [&](int kt, int cc, int buf) {
      const int so = (kt % NSTG) * STG;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        af[buf][u] = *reinterpret_cast<const bf16x8*>(ab0 + so + u * 32 * 128 + off4[cc]);
        wf[buf][u] = *reinterpret_cast<const bf16x8*>(wb0 + so + u * 32 * 128 + off4[cc]);
      }
    };
    auto mma = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[buf][i], af[buf][j], acc[i][j], 0, 0, 0);
    };
    KD_BARRIER();                                                // step 0 in
    read_chunk(0, 0, 0);
    for (int kt = 0; kt < nk; ++kt) {
      read_chunk(kt, 1, 1);
      mma(0);
      __builtin_amdgcn_sched_barrier(0);
      read_chunk(kt, 2, 0);
      mma(1);
      __builtin_amdgcn_sched_barrier(0);
      KD_BARRIER();                                              // step kt + 1 in; everyone past step kt - 1
      if (HAS_R && kt == max(nk - 2, 0)) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i) load_block_raw(p.R + roff[i][j], rraw[i][j], lh);
      }
      read_chunk(kt, 3, 1);
      mma(0);
      __builtin_amdgcn_sched_barrier(0);
      read_chunk(min(kt + 1, nk - 1), 0, 0);                      // (past the end: a slot nobody refills any more; never used)
      mma(1);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll
    for (int kt = 0; kt < NSTG - 1; ++kt)
      if (kt < nk) issue(kt);
  }
  for (int kt = 0; !LW && kt < nk; ++kt) {
    wait_vm_dyn<40>((4 + WPC) * min(NSTG - 2, nk - 1 - kt));      // the steps requested after kt may stay in flight
    KD_BARRIER();                 // every wave's pieces of step kt are in; everyone is done reading the slot refilled next
    if (kt + NSTG - 1 < nk) issue(kt + NSTG - 1);
    if (HAS_R && kt == max(nk - 2, 0)) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) load_block_raw(p.R + roff[i][j], rraw[i][j], lh);
    }
    const char* st = smem + (kt % NSTG) * STG;
    const char* ab = st + (wr * 64) * 128;
    const char* wb = st + A_IMG + (wc * 64) * 128;
    // explicit double buffer: the 4 fragment reads of chunk cc + 1 are issued before the 4 MFMAs of chunk cc (with one wave per
    // SIMD -- grids of one tile per CU -- nobody else covers the LDS latency of a read-then-use sequence)
    bf16x8 af[2][2], wf[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      af[0][u] = *reinterpret_cast<const bf16x8*>(ab + u * 32 * 128 + off4[0]);
      wf[0][u] = *reinterpret_cast<const bf16x8*>(wb + u * 32 * 128 + off4[0]);
    }
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      if (cc + 1 < 4) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          af[(cc + 1) & 1][u] = *reinterpret_cast<const bf16x8*>(ab + u * 32 * 128 + off4[cc + 1]);
          wf[(cc + 1) & 1][u] = *reinterpret_cast<const bf16x8*>(wb + u * 32 * 128 + off4[cc + 1]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[cc & 1][i], af[cc & 1][j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  code_warm_end(warm);
  // ---- epilogue -------------------------------------------------------------------------------------------------------------------
  const float fac = EPI == KD_EPI_SPLIT_LERP ? *p.fac : 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gm = m0 + wr * 64 + 32 * j + l31;
    const bool ok = gm < p.M;
    const int gmc = ok ? gm : p.M - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int nb = n0 + wc * 64 + 32 * i;
      const int nbc = min(nb, p.N - 32);
      size_t off;
      if (EPI == KD_EPI_SPLIT_LERP) {
        const int hw = p.gh * p.gw, cout = p.N >> 2;
        const int b = gmc / hw, rr = gmc - b * hw, h = rr / p.gw, w = rr - h * p.gw;
        const int qd = nbc / cout, e = nbc - qd * cout;
        off = (((size_t)b * (2 * p.gh) + 2 * h + (qd >> 1)) * (2 * p.gw) + 2 * w + (qd & 1)) * cout + e;
      } else {
        off = (size_t)gmc * p.N + nbc;
      }
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = acc[i][j][r];
      if (EPI == KD_EPI_RESIDUAL || EPI == KD_EPI_SPLIT_LERP) {
        float rr_[16];
        block_from_raw(rraw[i][j], rr_);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (EPI == KD_EPI_RESIDUAL) {
            v[r] += rr_[r];
          } else {                                   // torch.lerp(skip, x, fac), ATen's two-branch form
            const float skip = rr_[r], diff = v[r] - skip;
            v[r] = (fabsf(fac) < 0.5f) ? skip + fac * diff : v[r] - diff * (1.0f - fac);
          }
        }
      }
      store_block_bf16(p.C + off, v, lh, ok && nb < p.N);
    }
  }
}

template <int AMODE, int EPI, int BMT, bool LW = false>
static int launch_tiled(const TArgs& a, const char* nm, double flops, double bytes, hipStream_t s) {
  constexpr int LDS = (BMT == 1 ? (LW ? 4 : 2) : 3) * (128 * BMT * 128 + WBLK);
  const long tiles = (long)((a.M + 128 * BMT - 1) / (128 * BMT)) * a.n_tiles_n;
  const CfgName cfg(nm, "bm%d,lw%d,deep%d", 128 * BMT, (int)LW, (int)LW);         // (the loader-wave form runs on the deep ring: lw1,deep1)
  LaunchScope prof(cfg, flops, bytes, s);
  launch<gemm_tiled_kernel<AMODE, EPI, BMT, LW>>(dim3((unsigned)tiles), dim3(LW ? 512 : 256 * BMT), LDS, s, a);
  return check_launch("kd_gemm_bf16(tiled)");
}

int gemm_tiled_try(const KdGemm& d, hipStream_t s, int* rc) {
  if (!d.Wp || d.norm || (d.K & 63) || (d.N & 31)) return 1;
  if (d.a_mode != KD_A_PLAIN && d.a_mode != KD_A_MERGE2x2) return 1;
  if (d.epi != KD_EPI_STORE && d.epi != KD_EPI_RESIDUAL && d.epi != KD_EPI_SPLIT_LERP) return 1;
  if (d.epi == KD_EPI_STORE && d.out_add != 0.f) return 1;
  if (d.a_mode == KD_A_MERGE2x2 && (d.epi == KD_EPI_SPLIT_LERP || ((d.K >> 2) & 63))) return 1;
  if (d.epi == KD_EPI_SPLIT_LERP && ((d.N >> 2) & 31)) return 1;
  TArgs a{};
  a.A = reinterpret_cast<const u16*>(d.A); a.Wp = reinterpret_cast<const char*>(d.Wp);
  a.C = reinterpret_cast<u16*>(d.C); a.R = reinterpret_cast<const u16*>(d.R); a.fac = d.fac;
  a.M = d.M; a.N = d.N; a.K = d.K; a.n_tiles_n = (d.N + 127) / 128; a.nk = d.K / 64;
  a.gh = d.gh; a.gw = d.gw; a.cin = d.K >> 2;
  a.warm = code_warm();
  const double flops = 2.0 * d.M * (double)d.N * d.K;
  const double bytes = 2.0 * ((double)d.M * d.K + (double)d.N * d.K + (double)d.M * d.N) + (d.epi != KD_EPI_STORE ? 2.0 * d.M * d.N : 0.0);
  const ProfName nm("gemm_tiled", "gemm_bf16_tiled<a%d,e%d> M=%d N=%d K=%d", d.a_mode, d.epi, d.M, d.N, d.K);
  // 256-row tiles halve the weight traffic per flop; worth it once they still give every CU a workgroup
  const long tiles256 = (long)((d.M + 255) / 256) * a.n_tiles_n, tiles128 = (long)((d.M + 127) / 128) * a.n_tiles_n;
  const int bmt = opt(KD_OPT_tiled_bm);
  const bool big = bmt ? bmt == 256 : tiles256 >= cu_count();
  // round 4: grids of at most ONE tile per CU (the level-2 shapes) on the loader-wave form (4-slot ring, 4 compute + 4 staging waves)
  // (from 12 K steps on: with fewer the launch's fixed cost decides and the smaller 2-slot form is ahead -- level-2 out projection 13.8 vs 14.2 us,
  // the 256-wide MNIST / CIFAR levels +4 us per launch: profiles/r04_tiled_bf16_bench.log, r04_small_batch.log)
  const bool lw = !big && tiles128 <= cu_count() && d.K >= 768 && opt(KD_OPT_tiled_lw);
#define KD_TL(AM, EP)                                                                       \
  if (d.a_mode == AM && d.epi == EP) {                                                      \
    *rc = big ? launch_tiled<AM, EP, 2>(a, nm, flops, bytes, s)                             \
              : (lw ? launch_tiled<AM, EP, 1, true>(a, nm, flops, bytes, s)                 \
                    : launch_tiled<AM, EP, 1>(a, nm, flops, bytes, s));                     \
    return 0;                                                                               \
  }
  KD_TL(KD_A_PLAIN, KD_EPI_STORE)
  KD_TL(KD_A_PLAIN, KD_EPI_RESIDUAL)
  KD_TL(KD_A_PLAIN, KD_EPI_SPLIT_LERP)
  KD_TL(KD_A_MERGE2x2, KD_EPI_STORE)
#undef KD_TL
  return 1;
}

// ------------------------------------------------------------------------------------------------------------------
// astat: AdaRMSNorm -> wide projection (qkv, up-projection + GEGLU) at K = 256 / 512, where the weight is too large to park.
// A workgroup of NWV = 4 waves owns a panel of 128 rows for a range of n-tiles: each wave keeps its 32 rows of the normalised,
// scaled panel in registers as B-operand fragments (read and converted once), the packed weight streams through an LDS ring
// (one 16 KiB block = [128 features][64 k] per slot, global_load_lds NSTG - 1 blocks ahead, counted vmcnt, one barrier per
// block), the epilogue of an n-tile runs in the lanes that own the rows while the next blocks are in flight.
// 4-slot ring, two workgroups per CU.  (256-row panels of 8 waves on an 8-slot ring, one workgroup per CU, halve the weight stream through
// the L2 -> LDS path but were never faster -- L1 qkv 30.4 vs 28.2 us, L2 qkv 47.0 vs 38.6, the GEGLU shapes equal,
// profiles/r02_harness_astat_rows.log: that stream is not what limits these kernels -- and were retired.)
// vmcnt bookkeeping (loads and stores retire in issue order): the wait before block s allows the blocks requested after it AND the
// epilogue stores issued after it to stay outstanding (full panels only; ragged panels wait for their stores).
template <int NC, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_astat_kernel(const GArgs p) {
  constexpr int NWV = 4, K = NC * 16, NK = NC / 4, NSTG = 4, PDIST = NSTG - 1;
  constexpr int PB = 16 / NWV;                       // 1 KiB pieces of a block per wave
  constexpr bool GEGLU = EPI == KD_EPI_GEGLU;
  constexpr int NCOL = GEGLU ? 64 : 128;
  constexpr int NST = GEGLU ? 4 : 8;                 // 16-byte stores per lane per n-tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const auto warm = code_warm_begin<(NC == 32 ? 26 : 16) * 1024>((int)blockIdx.x < p.warm && tid < 64);   // kd_common.h: this kernel's code -> L2
  const PanelSplit ps = panel_split(p.n_slices, p.n_tiles);      // (at level 2 the 8 splits otherwise read 67 MB for an 8 MB activation)
  const int nt_begin = ps.t_begin, nt_end = ps.t_end;
  const int n_tiles = nt_end - nt_begin, total = n_tiles * NK;
  const int m0 = ps.panel * (32 * NWV);

  const bool probe = p.clk && blockIdx.x == 0 && tid == 0;      // kd_prof_clock_buffer: workgroup 0's time line
  if (probe) { p.clk[0] = __builtin_amdgcn_s_memtime(); p.clk[1] = __builtin_amdgcn_s_memrealtime(); }
  const char* wp = p.Wp + (size_t)nt_begin * NK * WBLK + wid * (PB * 1024) + lane * 16;
  auto issue = [&](int s) {
    const char* src = wp + (size_t)s * WBLK;
    char* dst = smem + (s % NSTG) * WBLK + wid * (PB * 1024);
#pragma unroll
    for (int j = 0; j < PB; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + j * 1024),
                                       (__attribute__((address_space(3))) void*)(dst + j * 1024), 16, 0, 0);
  };

  const int row = m0 + wid * 32 + l31;
  const bool ok = row < p.M;
  const int rowc = ok ? row : p.M - 1;
  bf16x8 a[NC];
  float rs;
  {
    const int b = rowc / p.rows_per_sample;
    const float* sp = p.scale + (size_t)b * p.scale_stride + 8 * lh;
    float ssq = 0.f;
    // The wave's 32 rows come in through LDS: global_load_lds reads them as WHOLE rows (1 KiB contiguous per instruction, fully
    // coalesced) into the ring slot the wave borrows before the weight stream starts, and every lane then picks its own row's
    // fragments out of LDS.  Reading them straight from HBM, one 16-byte chunk per lane per instruction (32 different rows per
    // instruction, every 128-byte line touched by four instructions), cost 12 000 - 25 000 of the workgroup's 40 000 - 65 000
    // clocks (kd_prof_clock_buffer time line, profiles/r02_astat_timeline.md).  Chunk q of row r sits at slot q ^ (r & 15) of its
    // row image (source-side permutation), so the 16 lanes of a ds_read_b128 pass hit 16 different bank groups.
    constexpr int RPR = WBLK / (2 * K);                // rows per staging round (one 16 KiB slot): 16 at K = 512, 32 at K = 256
    constexpr int NR = 32 / RPR, CPR = K / 8;          // rounds; 16-byte chunks per row
    static_assert(RPR >= 16 && NR * RPR == 32, "staging geometry");
    u32x4 raw[NC];
    char* stage = smem + wid * WBLK;
    // the sample's scale vector (K floats) goes to a small LDS area of the wave as well when its 32 rows share one sample (every
    // real shape): 32 lanes asking L2 for the same 32 bytes, chunk after chunk, was the other half of the prologue
    char* scl = smem + NSTG * WBLK + wid * (K * 4);
    const int r_first = min(m0 + wid * 32, p.M - 1), r_last = min(m0 + wid * 32 + 31, p.M - 1);
    const bool uni = r_first / p.rows_per_sample == r_last / p.rows_per_sample;
    if (uni) {
      const char* ssrc = reinterpret_cast<const char*>(p.scale + (size_t)(r_first / p.rows_per_sample) * p.scale_stride) + lane * 16;
#pragma unroll
      for (int i = 0; i < K * 4 / 1024; ++i)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ssrc + i * 1024),
                                         (__attribute__((address_space(3))) void*)(scl + i * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int rr = (i * 64 + lane) / CPR, qs = (i * 64 + lane) % CPR;        // LDS row of this lane's piece, its slot in the row
        const int grow = min(m0 + wid * 32 + r * RPR + rr, p.M - 1);
        const char* src = reinterpret_cast<const char*>(p.A + (size_t)grow * K) + ((qs ^ (rr & 15)) << 4);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(stage + i * 1024), 16, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // wave-private slot: no barrier
      if (NR == 1 || (l31 / RPR) == r) {
        const int rr = l31 % RPR;
        const char* rowp = stage + rr * (2 * K);
#pragma unroll
        for (int c = 0; c < NC; ++c) raw[c] = *reinterpret_cast<const u32x4*>(rowp + (((2 * c + lh) ^ (rr & 15)) << 4));
      }
      if (NR > 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slot is overwritten by the next round
    }
    f32x4 s0[2][4], s1[2][4];
    const float* spl = reinterpret_cast<const float*>(scl) + 8 * lh;
    auto load_scales = [&](int c0, int g) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (uni) {
          s0[g][u] = *reinterpret_cast<const f32x4*>(spl + 16 * (c0 + u));
          s1[g][u] = *reinterpret_cast<const f32x4*>(spl + 16 * (c0 + u) + 4);
        } else {
          s0[g][u] = *reinterpret_cast<const f32x4*>(sp + 16 * (c0 + u));
          s1[g][u] = *reinterpret_cast<const f32x4*>(sp + 16 * (c0 + u) + 4);
        }
      }
    };
    load_scales(0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c0 = 0; c0 < NC; c0 += 4) {
      const int g = (c0 >> 2) & 1;
      if (c0 + 4 < NC) load_scales(c0 + 4, g ^ 1);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { x[2 * e] = bf_lo(raw[c0 + u][e]); x[2 * e + 1] = bf_hi(raw[c0 + u][e]); }
#pragma unroll
        for (int e = 0; e < 8; ++e) ssq = fmaf(x[e], x[e], ssq);
        u32x4 o = {pack_bf16(x[0] * s0[g][u][0], x[1] * s0[g][u][1]), pack_bf16(x[2] * s0[g][u][2], x[3] * s0[g][u][3]),
                   pack_bf16(x[4] * s1[g][u][0], x[5] * s1[g][u][1]), pack_bf16(x[6] * s1[g][u][2], x[7] * s1[g][u][3])};
        asm volatile("" : "+v"(o));      // materialise the fragment HERE: hipcc otherwise sinks the multiply + pack down to the
                                         // first MFMA that uses it and keeps x and the scales (4x the registers) alive until then
        a[c0 + u] = __builtin_bit_cast(bf16x8, o);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    ssq += __shfl_xor(ssq, 32, 64);
    rs = rsqrtf(ssq / (float)K + p.eps);
  }
  float py = 0.f, px = 0.f;
  if (EPI == KD_EPI_QKV) {
    const int tok = rowc % p.rows_per_sample;
    py = p.pos[2 * tok];
    px = p.pos[2 * tok + 1];
  }
  code_warm_end(warm);
  KD_BARRIER();                                        // every wave has taken its rows out of the slot it borrowed
#pragma unroll
  for (int s = 0; s < PDIST; ++s)
    if (s < total) issue(s);
  const bool full_panel = m0 + 32 * NWV <= p.M;
  if (probe) p.clk[4] = __builtin_amdgcn_s_memtime();          // end of the row prologue
  // every ordinary load above has been consumed (the compiler waited for them, which also drained the first ring blocks)

  int off4[4];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) off4[cc] = swz128(l31, 2 * cc + lh);
  u16* crow = p.C + (size_t)rowc * p.N;

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  for (int nt = 0; nt < n_tiles; ++nt) {
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const int s = nt * NK + ks;
      {
        // behind block s in the queue: the blocks requested after it, and the stores of the epilogues that ran since its request
        // (block s was requested in step s - PDIST; the epilogue of a tile follows its last step, ks + 1 resp. ks + 1 + NK steps ago)
        int allow = PB * min(PDIST - 1, total - 1 - s);
        if (full_panel) {
          if (nt > 0 && ks + 1 <= PDIST) allow += NST;
          if (nt > 1 && ks + 1 + NK <= PDIST) allow += NST;
        }
        wait_vm_dyn<40>(allow);
      }
      KD_BARRIER();                      // every wave's share of block s is in; everyone is done reading slot (s-1) % NSTG
      if (s + PDIST < total) issue(s + PDIST);
      const char* st = smem + (s % NSTG) * WBLK;
      // explicit double buffer, one sched_barrier per chunk: the 4 fragment reads of chunk cc + 1 go out BEFORE the 4 MFMAs of
      // chunk cc (left to itself the scheduler, short of registers at K = 512, emits read / wait / MFMA triples and every MFMA
      // eats a full LDS latency)
      bf16x8 wf[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[0][j] = *reinterpret_cast<const bf16x8*>(st + j * 32 * 128 + off4[0]);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        if (cc + 1 < 4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) wf[(cc + 1) & 1][j] = *reinterpret_cast<const bf16x8*>(st + j * 32 * 128 + off4[cc + 1]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[cc & 1][j], a[4 * ks + cc], acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int n0 = (nt_begin + nt) * NCOL;
    if (probe && nt == 0) p.clk[5] = __builtin_amdgcn_s_memtime();    // end of the first tile's K loop
    if (GEGLU) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        float v[16];
        geglu_block(acc[2 * jj], acc[2 * jj + 1], rs, v);
        store_block_bf16(crow + n0 + 32 * jj, v, lh, ok);
      }
    } else if (EPI == KD_EPI_QKV) {
#pragma unroll
      for (int vv = 0; vv < 2; ++vv) {
        const int vec = (n0 >> 6) + vv;
        const int which = vec / p.n_heads, head = vec - which * p.n_heads;
        if (which < 2) {
          float fr[4], qsc;
          KD_HEAD_CONSTS(p.freq, p.qk_scale, head, lh, fr, qsc)
          qk_prep_blocks(acc[2 * vv], acc[2 * vv + 1], rs, sqrtf(qsc), p.eps, py, px, fr);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) { acc[2 * vv][r] *= rs; acc[2 * vv + 1][r] *= rs; }
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = acc[2 * vv + jj][r];
          store_block_bf16(crow + n0 + 64 * vv + 32 * jj, v, lh, ok);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = acc[j][r] * rs;
        store_block_bf16(crow + n0 + 32 * j, v, lh, ok);
      }
    }
    if (probe && nt == 0) p.clk[6] = __builtin_amdgcn_s_memtime();    // end of the first tile's epilogue
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  }
  if (probe) { p.clk[2] = __builtin_amdgcn_s_memtime(); p.clk[3] = __builtin_amdgcn_s_memrealtime(); p.clk[7] = (unsigned long long)total; }
}

template <int NC, int EPI>
static int launch_astat(const GArgs& a, const char* nm, double flops, double bytes, hipStream_t s) {
  // panels x n-splits: 128-row panels, two workgroups per CU, n-tiles split until the grid fills them.
  // n-splits of a panel: best_n_splits with the row prologue at about one n-tile's worth of time (profiles/r02_astat_timeline.md)
  const int forced = opt(KD_OPT_astat_splits);
  const int s128 = best_n_splits((a.M + 127) / 128, a.n_tiles, 2 * cu_count(), 1);
  const int splits = forced > 0 && forced <= a.n_tiles ? forced : s128;
  constexpr int LDS = 4 * WBLK + 4 * NC * 64;         // ring + one scale vector (K floats) per wave
  const int panels = (a.M + 127) / 128;
  GArgs b = a;
  b.n_slices = splits;                                // (the astat kernel's use of this field: n-splits per panel)
  const CfgName cfg(nm, "rows128,splits%d", splits);
  LaunchScope prof(cfg, flops, bytes, s);
  launch<gemm_astat_kernel<NC, EPI>>(dim3((unsigned)(panels * splits)), dim3(256), LDS, s, b);
  return check_launch("kd_gemm_bf16(astat)");
}

int gemm_astat_try(const KdGemm& d, hipStream_t s, int* rc) {
  if (d.a_mode != KD_A_PLAIN || !d.Wp || !d.norm || !opt(KD_OPT_astat_bf16)) return 1;
  if (d.epi != KD_EPI_STORE && d.epi != KD_EPI_QKV && d.epi != KD_EPI_GEGLU) return 1;
  if (d.K != 256 && d.K != 512) return 1;
  if (d.epi == KD_EPI_STORE && d.out_add != 0.f) return 1;
  const bool geglu = d.epi == KD_EPI_GEGLU;
  const int ncol = geglu ? 64 : 128;
  if (d.N % ncol || d.M < 512) return 1;
  if (d.rows_per_sample <= 0) return 1;
  GArgs a{};
  a.A = reinterpret_cast<const u16*>(d.A); a.Wp = reinterpret_cast<const char*>(d.Wp); a.C = reinterpret_cast<u16*>(d.C);
  a.scale = d.scale; a.scale_stride = d.scale_stride; a.rows_per_sample = d.rows_per_sample; a.eps = d.eps;
  a.M = d.M; a.N = d.N; a.n_tiles = d.N / ncol;
  a.n_heads = d.n_heads; a.qk_scale = d.qk_scale; a.pos = d.rope_pos; a.freq = d.rope_freq;
  a.clk = g_clk;
  a.warm = code_warm();
  const double n_eff = geglu ? 2.0 * d.N : (double)d.N;
  const double flops = 2.0 * d.M * n_eff * d.K;
  const double bytes = 2.0 * ((double)d.M * d.K + n_eff * d.K + (double)d.M * d.N);
  const ProfName nm("gemm_astat", "gemm_bf16_astat<e%d> M=%d N=%d K=%d", d.epi, d.M, d.N, d.K);
#define KD_AS(NCV, EP) if (d.K == NCV * 16 && d.epi == EP) { *rc = launch_astat<NCV, EP>(a, nm, flops, bytes, s); return 0; }
  KD_AS(16, KD_EPI_STORE) KD_AS(16, KD_EPI_QKV) KD_AS(16, KD_EPI_GEGLU)
  KD_AS(32, KD_EPI_STORE) KD_AS(32, KD_EPI_QKV) KD_AS(32, KD_EPI_GEGLU)
#undef KD_AS
  return 1;
}

// ------------------------------------------------------------------------------------------------------------------
// generic: every A gather (plain | 2x2 merge | NCHW patch of the fp32 image), optional norm prologue, every epilogue, ragged
// M / N / K (K % 4 == 0).  128 x 128 tile, A register-staged (converted / scaled / zero-padded on its way into the swizzled LDS
// image), the packed weight block by global_load_lds, one K step of 64 at a time.  The fallback for the shapes the three fast
// kernels do not take (patch-in / patch-out, tiny models, odd sizes): correctness first, not tuned.
__device__ __forceinline__ float karras_c_in(float sigma, float sd) { return 1.0f / sqrtf(sigma * sigma + sd * sd); }

template <int AMODE, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_generic_bf16_kernel(const KdGemm p) {
  constexpr bool GEGLU = EPI == KD_EPI_GEGLU;
  constexpr int NCOL = GEGLU ? 64 : 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Aimg = smem;
  char* Wimg = smem + WBLK;
  float* rs_tab = reinterpret_cast<float*>(smem + 2 * WBLK);
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
  const int wc = wid & 1, wr = wid >> 1;
  const int n_tiles = (p.N + NCOL - 1) / NCOL;
  const int nt = blockIdx.x % n_tiles, mt = blockIdx.x / n_tiles;
  const int m0 = mt * 128, n0 = nt * NCOL;
  const int M = p.M, N = p.N, K = p.K, nk = (K + 63) / 64;
  const u16* A16 = reinterpret_cast<const u16*>(p.A);

  // staging coordinates: rows tid/8 + 32 j, 8-wide k chunk (tid & 7)
  const int kq = tid & 7;
  int a_b[4]; bool row_ok[4]; float a_cin[4]; long a_base[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gm = m0 + (tid >> 3) + 32 * j;
    row_ok[j] = gm < M;
    const int gmc = row_ok[j] ? gm : M - 1;
    if (AMODE == KD_A_PLAIN) {
      a_b[j] = gmc / p.rows_per_sample;
      a_base[j] = (long)gmc * K;
      a_cin[j] = 1.f;
    } else {
      const int hw = p.gh * p.gw, b = gmc / hw, rr = gmc - b * hw, h = rr / p.gw, w = rr - h * p.gw;
      a_b[j] = b;
      if (AMODE == KD_A_MERGE2x2) {
        a_base[j] = (((long)b * (2 * p.gh) + 2 * h) * (2 * p.gw) + 2 * w) * (K >> 2);
        a_cin[j] = 1.f;
      } else {
        a_base[j] = (((long)b * p.chan) * (p.gh * p.ph) + h * p.ph) * (long)(p.gw * p.pw) + w * p.pw;
        a_cin[j] = p.sigma ? karras_c_in(p.sigma[b], p.sigma_data) : 1.0f;
      }
    }
  }
  f32x4 ra[4][2];
  float ssq[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_regs = [&](int kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int k4 = min(kt * 64 + kq * 8 + 4 * g, K - 4);          // clamped; zeroed at the store when out of range
        f32x4 v;
        if (AMODE == KD_A_PLAIN) {
          const u32x2 w = *reinterpret_cast<const u32x2*>(A16 + a_base[j] + k4);
          v = f32x4{bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1])};
        } else if (AMODE == KD_A_MERGE2x2) {
          const int cin = K >> 2, qd = k4 / cin, e = k4 - qd * cin;
          const u32x2 w = *reinterpret_cast<const u32x2*>(A16 + a_base[j] + ((long)(qd >> 1) * (2 * p.gw) + (qd & 1)) * cin + e);
          v = f32x4{bf_lo(w[0]), bf_hi(w[0]), bf_lo(w[1]), bf_hi(w[1])};
        } else {      // fp32 NCHW image: k = (nh * pw + nw) * chan + c
          const long plane = (long)(p.gh * p.ph) * (p.gw * p.pw);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k4 + u, c = k % p.chan, q = k / p.chan, nh_ = q / p.pw, nw = q - nh_ * p.pw;
            v[u] = p.A[a_base[j] + c * plane + (long)nh_ * (p.gw * p.pw) + nw];
          }
        }
        ra[j][g] = v;
      }
  };
  auto store_regs = [&](int kt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned o[4];
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int k4r = kt * 64 + kq * 8 + 4 * g;
        const int k4 = min(k4r, K - 4);
        f32x4 v = (row_ok[j] && k4r < K) ? ra[j][g] : f32x4{0.f, 0.f, 0.f, 0.f};
        if (AMODE == KD_A_PATCH_NCHW) v = v * a_cin[j];
        if (p.norm) {
          ssq[j] += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
          v = v * *reinterpret_cast<const f32x4*>(p.scale + (long)a_b[j] * p.scale_stride + k4);
        }
        o[2 * g] = pack_bf16(v[0], v[1]);
        o[2 * g + 1] = pack_bf16(v[2], v[3]);
      }
      *reinterpret_cast<u32x4*>(Aimg + swz128((tid >> 3) + 32 * j, kq)) = u32x4{o[0], o[1], o[2], o[3]};
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  int off4[4];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) off4[cc] = swz128(l31, 2 * cc + lh);
  const char* wsrc = reinterpret_cast<const char*>(p.Wp) + (size_t)nt * nk * WBLK + wid * 4096 + lane * 16;

  load_regs(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                                 // the previous step's fragment reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + (size_t)kt * WBLK + j * 1024),
                                       (__attribute__((address_space(3))) void*)(Wimg + wid * 4096 + j * 1024), 16, 0, 0);
    store_regs(kt);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) load_regs(kt + 1);
    const char* ab = Aimg + (wr * 64) * 128;
    const char* wb = Wimg + (wc * 64) * 128;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      bf16x8 af[2], wf[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        af[u] = *reinterpret_cast<const bf16x8*>(ab + u * 32 * 128 + off4[cc]);
        wf[u] = *reinterpret_cast<const bf16x8*>(wb + u * 32 * 128 + off4[cc]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[i], af[j], acc[i][j], 0, 0, 0);
    }
  }
  if (p.norm) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sm = wave_sum_xor(ssq[j], 8);
      if (kq == 0) rs_tab[(tid >> 3) + 32 * j] = rsqrtf(sm / (float)K + p.eps);
    }
  }
  __syncthreads();

  // ---- epilogue: lane owns rows m0 + 64 wr + 32 j + l31 ------------------------------------------------------------------------
  const float fac = EPI == KD_EPI_SPLIT_LERP ? *p.fac : 0.f;
  u16* C16 = reinterpret_cast<u16*>(p.C);
  const u16* R16 = reinterpret_cast<const u16*>(p.R);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int rt = wr * 64 + 32 * j + l31, gm = m0 + rt;
    const bool ok = gm < M;
    const int gmc = ok ? gm : M - 1;
    const float rs = p.norm ? rs_tab[rt] : 1.0f;
    if (GEGLU) {
      float v[16];
      const float rsh = 0.5f * rs;
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2 o = geglu_pair(f32x2{acc[0][j][r], acc[0][j][r + 1]} * rsh, f32x2{acc[1][j][r], acc[1][j][r + 1]} * rs);
        v[r] = o.x;
        v[r + 1] = o.y;
      }
      const int nb = n0 + 32 * wc;
      store_block_bf16(C16 + (size_t)gmc * N + min(nb, N - 8), v, lh, ok && nb < N, N - nb);
    } else if (EPI == KD_EPI_QKV) {
      const int vec = (n0 >> 6) + wc;
      if (vec * 64 < N) {
        const int which = vec / p.n_heads, head = vec - which * p.n_heads;
        if (which < 2) {
          const int tok = gmc % p.rows_per_sample;
          float fr[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) fr[u] = lh ? p.rope_freq[head * 8 + 4 + u] : p.rope_freq[head * 8 + u];
          qk_prep_blocks(acc[0][j], acc[1][j], rs, sqrtf(p.qk_scale[head]), p.eps, p.rope_pos[2 * tok], p.rope_pos[2 * tok + 1], fr);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) { acc[0][j][r] *= rs; acc[1][j][r] *= rs; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          float v[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) v[r] = acc[i][j][r];
          store_block_bf16(C16 + (size_t)gmc * N + vec * 64 + 32 * i, v, lh, ok);
        }
      }
    } else if (EPI == KD_EPI_UNPATCH_NCHW) {
      // fp32 image out (+ Karras c_out / c_skip against the fp32 input image), element by element: n = (nh * pw + nw) * chan + c
      const int hw = p.gh * p.gw, b = gmc / hw, rr = gmc - b * hw, h = rr / p.gw, w = rr - h * p.gw;
      float c_out = 1.f, c_skip = 0.f;
      if (p.sigma) {
        const float sg = p.sigma[b], sd = p.sigma_data, var = sg * sg + sd * sd;
        c_out = sg * sd / sqrtf(var);
        c_skip = sd * sd / var;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + wc * 64 + 32 * i + mfma32_row(r, lane);
          if (ok && n < N) {
            const int c = n % p.chan, q = n / p.chan, nh_ = q / p.pw, nw = q - nh_ * p.pw;
            const long o = (((long)b * p.chan + c) * (p.gh * p.ph) + h * p.ph + nh_) * (long)(p.gw * p.pw) + w * p.pw + nw;
            float v = acc[i][j][r] * rs;
            if (p.sigma) v = v * c_out + p.R[o] * c_skip;
            p.C[o] = v;
          }
        }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int nb = n0 + wc * 64 + 32 * i, nbc = min(nb, N - 8), nv = N - nb;
        size_t off;
        if (EPI == KD_EPI_SPLIT_LERP) {
          const int hw = p.gh * p.gw, cout = N >> 2;
          const int b = gmc / hw, rr = gmc - b * hw, h = rr / p.gw, w = rr - h * p.gw;
          const int qd = nbc / cout, e = nbc - qd * cout;
          off = (((size_t)b * (2 * p.gh) + 2 * h + (qd >> 1)) * (2 * p.gw) + 2 * w + (qd & 1)) * cout + e;
        } else {
          off = (size_t)gmc * N + nbc;
        }
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = acc[i][j][r] * rs;
        if (EPI == KD_EPI_RESIDUAL || EPI == KD_EPI_SPLIT_LERP) {
          float rr_[16];
          load_block_bf16(R16 + off, rr_, lh, nv);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (EPI == KD_EPI_RESIDUAL) {
              v[r] += rr_[r];
            } else {
              const float skip = rr_[r], diff = v[r] - skip;
              v[r] = (fabsf(fac) < 0.5f) ? skip + fac * diff : v[r] - diff * (1.0f - fac);
            }
          }
        }
        store_block_bf16(C16 + off, v, lh, ok && nb < N, nv);
      }
    }
  }
}

template <int AMODE, int EPI>
static int launch_generic(const KdGemm& d, hipStream_t s) {
  constexpr int LDS = 2 * WBLK + 128 * 4;
  constexpr int NCOL = EPI == KD_EPI_GEGLU ? 64 : 128;
  const long tiles = (long)((d.M + 127) / 128) * ((d.N + NCOL - 1) / NCOL);
  const double n_eff = EPI == KD_EPI_GEGLU ? 2.0 * d.N : (double)d.N;
  const ProfName nm("gemm_generic", "gemm_bf16_generic<a%d,e%d> M=%d N=%d K=%d", AMODE, EPI, d.M, d.N, d.K);
  const double a_bytes = (AMODE == KD_A_PATCH_NCHW ? 4.0 : 2.0) * d.M * d.K;
  const double c_bytes = (EPI == KD_EPI_UNPATCH_NCHW ? (d.sigma ? 8.0 : 4.0) : (EPI == KD_EPI_RESIDUAL || EPI == KD_EPI_SPLIT_LERP ? 4.0 : 2.0)) * d.M * d.N;
  LaunchScope prof(nm, 2.0 * d.M * n_eff * d.K, a_bytes + 2.0 * n_eff * d.K + c_bytes, s);
  KdGemm e = d;
  if (e.rows_per_sample <= 0) e.rows_per_sample = e.M;
  launch<gemm_generic_bf16_kernel<AMODE, EPI>>(dim3((unsigned)tiles), dim3(256), LDS, s, e);
  return check_launch("kd_gemm_bf16(generic)");
}

int gemm_generic_try(const KdGemm& d, hipStream_t s, int* rc) {
  if (d.epi != KD_EPI_UNPATCH_NCHW && (d.N & 7)) return 1;                 // 16-byte stores: 8 bf16
  if (d.epi == KD_EPI_SPLIT_LERP && ((d.N >> 2) & 31)) return 1;            // a 32-feature block lies inside one quadrant
  if (d.epi == KD_EPI_STORE && d.out_add != 0.f) return 1;
  if (d.a_mode == KD_A_MERGE2x2 && ((d.K >> 2) & 3)) return 1;
#define KD_GN(AM, EP) if (d.a_mode == AM && d.epi == EP) { *rc = launch_generic<AM, EP>(d, s); return 0; }
  KD_GN(KD_A_PLAIN, KD_EPI_STORE) KD_GN(KD_A_PLAIN, KD_EPI_RESIDUAL) KD_GN(KD_A_PLAIN, KD_EPI_GEGLU) KD_GN(KD_A_PLAIN, KD_EPI_QKV)
  KD_GN(KD_A_PLAIN, KD_EPI_SPLIT_LERP) KD_GN(KD_A_PLAIN, KD_EPI_UNPATCH_NCHW)
  KD_GN(KD_A_MERGE2x2, KD_EPI_STORE) KD_GN(KD_A_PATCH_NCHW, KD_EPI_STORE)
#undef KD_GN
  return 1;
}

// ---- one-off weight packing -------------------------------------------------------------------------------------------
// one thread per (block, row, 16-byte chunk)
__global__ __launch_bounds__(256) void pack_weight_bf16_kernel(const float* __restrict__ W, char* __restrict__ out, int N, int K, int geglu,
                                                                int n_tiles, int nk) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)n_tiles * nk * WROWS * 8;
  if (idx >= total) return;
  const int q = idx & 7, r = (idx >> 3) & (WROWS - 1);
  const long blk = idx >> 10;
  const int ks = blk % nk, nt = blk / nk;
  const int wrow = w_row_of_tile(nt, r, N, (geglu & 1) != 0);
  float v[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    // layout 2 (down projection of the fused FF block): chunk q = 2 g + h of a k-step holds k 16 g + {4h .. 4h+3, 8 + 4h .. 8 + 4h+3}
    const int k = ks * WKS + ((geglu & 2) ? 16 * (q >> 1) + 4 * (q & 1) + (u & 3) + 8 * (u >> 2) : q * 8 + u);
    v[u] = (wrow >= 0 && k < K) ? W[(long)wrow * K + k] : 0.f;
  }
  *reinterpret_cast<u32x4*>(out + blk * WBLK + swz128(r, q)) =
      u32x4{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
}

int gemm_patch_try(const KdGemm& d, hipStream_t s, int* rc);      // patch_bf16.hip
int gemm_b16s_try(const KdGemm& d, hipStream_t s, int* rc);       // gemm_b16s.hip

}  // namespace b16
}  // namespace kd

using namespace kd;

namespace kd { void x3_set_clock_buffer(unsigned long long* p); }     // gemm_x3.hip

extern "C" int kd_prof_clock_buffer(void* dev_ptr) {
  b16::g_clk = reinterpret_cast<unsigned long long*>(dev_ptr);
  x3_set_clock_buffer(reinterpret_cast<unsigned long long*>(dev_ptr));
  return KD_OK;
}

// blocks of the packed image: n-tiles (GEGLU, bit 0 of `geglu`: 64 outputs a tile) x k-steps
static void bf16_tiling(int N, int K, int geglu, int* n_tiles, int* nk) {
  const int ncol = (geglu & 1) ? 64 : 128;
  *n_tiles = (N + ncol - 1) / ncol;
  *nk = (K + b16::WKS - 1) / b16::WKS;
}

extern "C" long long kd_packed_weight_bytes_bf16(int N, int K, int geglu) {
  if (N <= 0 || K <= 0) return 0;
  int n_tiles, nk;
  bf16_tiling(N, K, geglu, &n_tiles, &nk);
  return (long long)n_tiles * nk * b16::WBLK;
}

extern "C" int kd_pack_weight_bf16(const float* W, void* out, int N, int K, int geglu, void* stream) {
  if (!W || !out || N <= 0 || K <= 0 || geglu < 0 || geglu > 3) return fail(KD_EINVAL, "kd_pack_weight_bf16: bad arguments");
  int n_tiles, nk;
  bf16_tiling(N, K, geglu, &n_tiles, &nk);
  const long total = (long)n_tiles * nk * b16::WROWS * 8;
  hipLaunchKernelGGL(b16::pack_weight_bf16_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W,
                     reinterpret_cast<char*>(out), N, K, geglu, n_tiles, nk);
  return check_launch("kd_pack_weight_bf16");
}

extern "C" int kd_gemm_bf16(const KdGemm* dp, void* stream) {
  if (!dp) return fail(KD_EINVAL, "kd_gemm_bf16: null descriptor");
  const KdGemm& d = *dp;
  hipStream_t s = (hipStream_t)stream;
  if (d.precision != KD_PREC_BF16) return fail(KD_EINVAL, "kd_gemm_bf16: precision must be KD_PREC_BF16");
  if (d.M <= 0 || d.N <= 0 || d.K <= 0 || (d.K & 3)) return fail(KD_EINVAL, "kd_gemm_bf16: bad M/N/K %d/%d/%d (K %% 4 != 0?)", d.M, d.N, d.K);
  if (!d.A || !d.C || !d.Wp) return fail(KD_EINVAL, "kd_gemm_bf16: null A / C / Wp (kd_pack_weight_bf16)");
  if (d.norm && (!d.scale || d.rows_per_sample <= 0 || (d.scale_stride & 3))) return fail(KD_EINVAL, "kd_gemm_bf16: norm needs scale, rows_per_sample, scale_stride%%4==0");
  if (d.epi == KD_EPI_RESIDUAL && !d.R) return fail(KD_EINVAL, "kd_gemm_bf16: residual needs R");
  if (d.epi == KD_EPI_QKV && (d.n_heads <= 0 || d.N != 3 * d.n_heads * 64 || d.rows_per_sample <= 0 || !d.qk_scale || !d.rope_pos || !d.rope_freq))
    return fail(KD_EINVAL, "kd_gemm_bf16: qkv epilogue needs N == 3*n_heads*64, rows_per_sample, qk_scale, rope_pos, rope_freq");
  if (d.epi == KD_EPI_QKV && ((reinterpret_cast<uintptr_t>(d.rope_freq) & 31) || (reinterpret_cast<uintptr_t>(d.qk_scale) & 3)))
    return fail(KD_EINVAL, "kd_gemm_bf16: rope_freq must be 32-byte aligned (a head's 8 frequencies are one scalar load), qk_scale 4-byte aligned");
  if (d.a_mode != KD_A_PLAIN && (d.gh <= 0 || d.gw <= 0 || d.M % (d.gh * d.gw))) return fail(KD_EINVAL, "kd_gemm_bf16: gather mode needs gh, gw with M %% (gh*gw) == 0");
  if (d.epi == KD_EPI_SPLIT_LERP && (!d.R || !d.fac || (d.N & 3) || d.gh <= 0 || d.gw <= 0 || d.M % (d.gh * d.gw))) return fail(KD_EINVAL, "kd_gemm_bf16: split needs R, fac, N%%4==0, gh, gw");
  int rc = 0;
  // shape-driven choice (benchmarks/hip_harness, profiles/r02_*): level-0 shapes (K = 128, and K = 384 with N = 128) park the
  // weight; norm projections at K = 256 / 512 keep A in registers and stream the weight; the rest is tiled
  if (!opt(KD_OPT_bf16_fast)) {
    if (!b16::gemm_generic_try(d, s, &rc)) return rc;
    return fail(KD_EINVAL, "kd_gemm_bf16: no generic kernel for a_mode=%d epi=%d N=%d", d.a_mode, d.epi, d.N);
  }
  if ((d.a_mode == KD_A_PATCH_NCHW || d.epi == KD_EPI_UNPATCH_NCHW) && !b16::gemm_patch_try(d, s, &rc)) return rc;
  if (!b16::gemm_b16s_try(d, s, &rc)) return rc;                   // few rows (small batches): the latency form, gemm_b16s.hip
  const bool small_k = d.K == 128 || (d.K == 384 && d.N <= 128);
  if (small_k && !b16::gemm_wstat_try(d, s, &rc)) return rc;
  if (!b16::gemm_astat_try(d, s, &rc)) return rc;
  if (!b16::gemm_tiled_try(d, s, &rc)) return rc;
  if (!b16::gemm_wstat_try(d, s, &rc)) return rc;
  if (!b16::gemm_generic_try(d, s, &rc)) return rc;
  return fail(KD_EINVAL, "kd_gemm_bf16: unsupported combination a_mode=%d norm=%d epi=%d M=%d N=%d K=%d", d.a_mode, d.norm, d.epi, d.M, d.N, d.K);
}

KD_TEXT_PAD(gemm_bf16)      // last function of this code object: kd_common.h, code warm-up
