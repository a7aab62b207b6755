// Level 0 of the 256 x 256 configs in fp32-parity ("split3") arithmetic: neighbourhood attention core + out projection + residual +
// feed-forward block in ONE launch (kd_attn_ffn_f32).  As two launches (attn_na2d_x3<7>, then ffn_x3h<true>) the attention rows make a
// round trip through HBM that the result does not need -- 67 MB written, the same 67 MB read back as the out projection's B fragments, of
// the 469 MB the pair moves per layer -- and the two kernels, bound by different resources (the core by HBM and VALU, the block by the
// matrix pipe), never share a CU.
//
// The feed-forward block is row-wise, so its 128-row panel may be any 128 rows: here it is the core's 8 x 16 query tile, wave w's lane-row l
// being the query that wave w's lane l owns in the core (ffn_x3h_core.h: Panel).
//   phase A: attn_x3_core.h's tile body for head 0, then head 1, through one 78 KiB image; a lane keeps its query's normalised output of
//            both heads in registers (2 x 32 fp32) until every wave has left the image;
//   hand-over: each wave writes its 32 attention rows (128 fp32 features) into the ring slot the block's prologue borrows for them, in the
//            layout the prologue's LDS-DMA produces from HBM in the two-launch form -- wave-private, no barrier;
//   phase B: ffn_x3h_core.h's body as it is; the hi / lo split of the attention rows happens where it happens there.
// Every product keeps its term and accumulation order: the residual stream is bit-identical to the two-launch path's.
// The image and the block's ring + strips share one allocation (78 KiB: two workgroups per CU, so that one workgroup's memory-bound
// phase A can run beside the other's matrix-bound phase B).  Registers: phase B names a0..a127 itself (x3_common.h); in phase A the
// compiler may use that half of the file freely -- nothing of phase B is live yet (the `kd_phase_b` marker below is where
// check_x3_agpr.py starts to hold the kernel to "the AccVGPRs are the kernel's alone").
#include "attn_x3_core.h"
#include "ffn_x3h_core.h"

namespace kd {
namespace x3 {

extern unsigned long long* g_clk;      // gemm_x3.hip (kd_prof_clock_buffer)

constexpr int AF_KS = 7;
constexpr int AF_LDS_FFN = 4 * STG + 4 * 1024 + 4 * 2048;
constexpr int AF_LDS = x3a::NaGeo<AF_KS>::LDS > AF_LDS_FFN ? x3a::NaGeo<AF_KS>::LDS : AF_LDS_FFN;
static_assert(AF_LDS <= 80 * 1024, "two workgroups per CU");

// panel row i = wave (i >> 5)'s query (i & 31) of the 8 x 16 tile at (ty0, tx0) of sample b: token (ty0 + 4 (w >> 1) + (l >> 3), tx0 + 8 (w & 1) + (l & 7))
struct PanelTile {
  static constexpr bool ATT_LDS = true;
  int tok0, W;                          // b H W + ty0 W + tx0
  __device__ __forceinline__ int row(int i) const { return tok0 + (4 * (i >> 6) + ((i & 31) >> 3)) * W + 8 * ((i >> 5) & 1) + (i & 7); }
};

__global__ __launch_bounds__(256, 2) void attn_ffn_x3h_kernel(const x3a::NArgs a, const FArgs3 p) {
  using namespace x3a;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const auto warm = code_warm_begin<28 * 1024>((int)blockIdx.x < a.warm && tid < 64);
  (void)wg_stamp_begin(a.clk);
  const int tiles_x = a.W / NA_TW, tiles_y = a.H / NA_TH;
  int r = KD_XCD_CHUNK();      // XCD-aware order: neighbouring tiles (overlapping halos) run on ONE L2
  const int tx = r % tiles_x; r /= tiles_x;
  const int ty = r % tiles_y, b = r / tiles_y;
  // Each stage (head 0, head 1, hand-over + phase B) derives its lane constants afresh from an opaque copy of the thread index: values the
  // stages have in common (lane row, wave, tile addresses) would otherwise stay live from the first stage to the last, on top of head 0's
  // output -- and the kernel has no register to spare (128 + 128, no scratch)
  auto fresh = [&]() { int t = tid; asm volatile("" : "+v"(t)); return t; };

  // ---- phase A: both heads of the tile; on[head][e][g] = features 64 head + 32 e + 8 g + 4 h2 + 0..3 of this lane's query ------------------
  f32x4 on[2][2][4];
  static_for<2>([&](auto head_) {
    constexpr int head = decltype(head_)::value;
    na2d_x3_tile<AF_KS>(smem, a, fresh(), b, head, ty, tx, [&]() { if constexpr (head == 0) code_warm_end(warm); },
                        [&](bool, int, float l, const f32x16 (&O)[2]) {
      const float inv = 1.0f / l;
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int g = 0; g < 4; ++g) on[head][e][g] = f32x4(f32x4{O[e][4 * g], O[e][4 * g + 1], O[e][4 * g + 2], O[e][4 * g + 3]} * inv);
    });
    KD_BARRIER();                                        // every wave has its V fragments: the image is free
  });

  // ---- hand-over: the wave's 32 attention rows into its borrowed ring slot (chunk c of row r in slot c ^ (r & 15)) --------------------------
  const int tid_b = fresh();
  {
    const int lane = tid_b & 63, wid = __builtin_amdgcn_readfirstlane(tid_b >> 6), l31 = lane & 31, h2 = lane >> 5;
    char* rowp = smem + wid * STG + l31 * 512;
#pragma unroll
    for (int head = 0; head < 2; ++head)
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(rowp + (((16 * head + 8 * e + 2 * g + h2) ^ (l31 & 15)) << 4)) = on[head][e][g];
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\t; kd_phase_b" ::: "memory");

  // ---- phase B: out projection + residual + feed-forward block on the tile's 128 rows -----------------------------------------------------
  ffn_x3h_body<true>(p, smem, tid_b, PanelTile{(b * a.H + ty * NA_TH) * a.W + tx * NA_TW, a.W}, []() {});
  wg_stamp_end(wg_stamp_again(a.clk));
}

}  // namespace x3
}  // namespace kd

using namespace kd;

extern "C" int kd_attn_ffn_f32_supported(int batch, int H, int W, int nh, int ks, int K, int d_ff) {
  if (!opt(KD_OPT_attn_ffn_x3) || !opt(KD_OPT_attn_x3) || !opt(KD_OPT_ffn_x3)) return 0;
  if (ks != x3::AF_KS || nh != 2 || K != 128 || d_ff <= 0 || (d_ff & 63)) return 0;
  if (batch <= 0 || H <= 0 || W <= 0 || H % x3a::NA_TH || W % x3a::NA_TW) return 0;
  return kd_ffn_f32_supported(batch * H * W, K, d_ff);
}

extern "C" int kd_attn_ffn_f32(const float* qkv, const KdFfn* dp, int batch, int H, int W, int nh, int ks, void* stream) {
  if (!qkv || !dp) return fail(KD_EINVAL, "kd_attn_ffn_f32: null qkv / descriptor");
  const KdFfn& d = *dp;
  if (!d.x || !d.out || !d.scale || !d.Wp_up || !d.Wp_down || !d.Wp_out) return fail(KD_EINVAL, "kd_attn_ffn_f32: null x / out / scale / Wp_up / Wp_down / Wp_out");
  if (ks != x3::AF_KS || nh != 2 || d.K != 128 || d.d_ff <= 0 || (d.d_ff & 63) || batch <= 0 || H <= 0 || W <= 0 || H % x3a::NA_TH || W % x3a::NA_TW)
    return fail(KD_EINVAL, "kd_attn_ffn_f32: kernel size 7, 2 heads of 64, K = 128, d_ff a multiple of 64, token grid a multiple of 8 x 16 (ks=%d nh=%d K=%d d_ff=%d H=%d W=%d)",
                ks, nh, d.K, d.d_ff, H, W);
  if ((long long)batch * H * W != d.M || d.rows_per_sample != H * W || (d.scale_stride & 3))
    return fail(KD_EINVAL, "kd_attn_ffn_f32: M = batch H W, rows_per_sample = H W, scale_stride %% 4 == 0");
  x3a::NArgs a{qkv, nullptr, batch, H, W, nh, code_warm(), x3::g_clk};
  x3::FArgs3 f{};
  f.X = reinterpret_cast<const float*>(d.x); f.Y = reinterpret_cast<float*>(d.out);
  f.Wu = reinterpret_cast<const char*>(d.Wp_up); f.Wd = reinterpret_cast<const char*>(d.Wp_down);
  f.scale = d.scale; f.scale_stride = d.scale_stride; f.rows_per_sample = d.rows_per_sample; f.eps = d.eps;
  f.M = d.M; f.d_ff = d.d_ff; f.n_tiles = d.d_ff / 64;
  f.warm = 0;
  f.clk = x3::g_clk;
  f.Wo = reinterpret_cast<const char*>(d.Wp_out);
  // the two launches it replaces (attn_x3.hip: launch_na, ffn_x3.hip: kd_ffn_f32 with attn), minus the attention rows' round trip
  const double M = d.M, K = d.K;
  const double flops = 4.0 * M * nh * x3a::DH * ks * ks + 2.0 * M * 3.0 * d.d_ff * K + 2.0 * M * K * K;
  const double bytes = 16.0 * M * nh * x3a::DH + 4.0 * (3.0 * M * K + 3.0 * d.d_ff * K + K * K) - 8.0 * M * K;
  const ProfName nm("attn_ffn_x3", "attn_ffn_x3 %dx%d nh=%d K=%d d_ff=%d", H, W, nh, d.K, d.d_ff);
  LaunchScope prof(nm, flops, bytes, (hipStream_t)stream);
  launch<x3::attn_ffn_x3h_kernel>(dim3((unsigned)(d.M / 128)), dim3(256), x3::AF_LDS, (hipStream_t)stream, a, f);
  return check_launch("kd_attn_ffn_f32");
}

KD_TEXT_PAD(attn_ffn_x3)      // last function of this code object: kd_common.h, code warm-up
