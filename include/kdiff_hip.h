/*
 * kdiff_hip.h -- C ABI of libkdiff_hip.so: the MI355X (gfx950) kernels behind the k-diffusion
 * sampling hot path.
 *
 * The reference (crowsonkb/k-diffusion) is pure Python and has no FFI of its own; what this ABI
 * replaces are the reference's *native call sites* -- the third-party CUDA extensions and the
 * torch.compile'd functions it calls on the hot path.  Each entry point cites the reference
 * interface it stands in for (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer (device memory);
 *   - nothing here allocates, frees or synchronises; every launch goes to `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value: 0 on success, negative KD_E* on a rejected call (bad shape / alignment /
 *     unsupported size); kd_last_error() then describes it.  Nothing throws;
 *   - activations are token-major ("NHWC"): [batch, h, w, channels] row-major fp32;
 *     qkv buffers are [batch*h*w, 3, n_heads, 64] (feature index t*(nh*64) + head*64 + e,
 *     k_diffusion/models/image_transformer_v2.py:386,422,431,467); the head dim is 64 in EVERY arithmetic mode (fp32-parity and bf16
 *     alike: every shipped config, k_diffusion/config.py:135-136).  The reference's `d_head` (image_transformer_v2.py:355-363:
 *     n_heads = d_model // d_head, RoPE on d_head // 2) is therefore not an argument of any entry point -- n_heads is, and the feature
 *     width is n_heads * 64; the Python mirror's model constructor refuses other values with a ValueError that says so
 *     (k-diffusion_amd/models/image_transformer_v2.py) instead of handing the kernels a layout they would misread;
 *   - reproducibility: a call's result is a function of its arguments and of which kernel serves it; the choice between a throughput
 *     kernel and a few-rows / block form of the same projection follows the ROW COUNT and the device's CU count (cost rules of the
 *     launchers), and the forms sum in different orders.  So the same sample can differ in its last bits between batch sizes or chips with
 *     another CU count (inside every tolerance stated here; forms documented as bit-identical to each other are exactly that).  The options
 *     that pin a form (x3s_max_rows / b16s_max_rows = 0, attn_block_bf16 / proj_block_bf16 = 0) give batch-invariant results.
 */
#ifndef KDIFF_HIP_H
#define KDIFF_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define KD_OK 0
#define KD_EINVAL (-1)   /* bad argument / unsupported shape */
#define KD_ELAUNCH (-2)  /* HIP launch error */

int kd_version(void);
const char* kd_last_error(void);
/* Tuning / A-B switches of the library (benchmarks and tests).  kdiff_options.def, next to this header, is the table: one row per option
 * with its name, its default (the shipped configuration) and what it selects.
 *   - the library reads no environment variables: the Python package maps KDIFF_OPTIONS="name=value,..." onto these calls;
 *   - thread-safe; an unknown name is refused with KD_EINVAL;
 *   - kd_set_option(name, INT_MIN) puts the option back to its default;
 *   - kd_get_option returns the value the caller set; if there is none, `dflt` -- or, asked with dflt == INT_MIN, the table's default
 *     (INT_MIN itself where the launcher computes the default from the device: KD_OPT_AUTO in the table). */
int kd_set_option(const char* name, int value);
int kd_get_option(const char* name, int dflt);

/* ------------------------------------------------------------------------------------------
 * Fused GEMM  C = epilogue( prologue(A) @ W^T ).   W is [N_w, K] row-major (nn.Linear.weight).
 * Replaces: nn.Linear / F.linear call sites image_transformer_v2.py:126-129 (Linear),
 * :89-95,132-139 (linear_geglu / LinearGEGLU, torch.compile'd), fused with the ops around
 * them: rms_norm/AdaRMSNorm :98-103,155-166 (prologue), residual add :396,443,476,493,
 * TokenMerge :586-595, TokenSplit + lerp :610-621, TokenSplitWithoutSkip :598-607 and the
 * NCHW<->NHWC movedims :723,760, and the Karras preconditioner k_diffusion/layers.py:88-90.
 */
enum { KD_A_PLAIN = 0, KD_A_MERGE2x2 = 1, KD_A_PATCH_NCHW = 2 };
/* arithmetic of the products: exact fp32 MFMA (bit-for-bit an fmaf chain), or each fp32 operand split into two
 * bf16 (hi + lo, 16 significand bits) with hi*hi + hi*lo + lo*hi on the bf16 MFMA and fp32 accumulation */
enum { KD_PREC_EXACT = 0, KD_PREC_SPLIT3 = 1,
       KD_PREC_BF16 = 2 /* kd_gemm_bf16 only: bf16 activations in HBM, one bf16 MFMA per product, fp32 accumulate -- the
                           arithmetic of the reference under torch.autocast(bfloat16) (image_transformer_v2.py:98-103,376-384) */ };
enum { KD_EPI_STORE = 0, KD_EPI_RESIDUAL = 1, KD_EPI_GEGLU = 2, KD_EPI_SPLIT_LERP = 3, KD_EPI_UNPATCH_NCHW = 4,
       KD_EPI_QKV = 5 /* store a qkv projection with q,k prepared: cosine-sim scaling + axial RoPE
                         (image_transformer_v2.py:106-121,187-231) applied in the epilogue, v untouched */ };

typedef struct {
  int M, N, K;          /* C is [M, N]; K = reduction length (multiple of 4)                      */
  int a_mode, epi;      /* KD_A_*, KD_EPI_*                                                       */
  int norm;             /* 1: A'[m,k] = A[m,k] * scale[b(m)*scale_stride + k] * rsqrt(mean_k A^2 + eps) */
  int rows_per_sample;  /* b(m) = m / rows_per_sample (tokens per image)                          */
  int scale_stride;     /* K for per-sample AdaRMSNorm scales, 0 for a shared RMSNorm gain        */
  int gh, gw;           /* token grid of the COARSE side (merge/split: h,w of the merged grid;
                           patch modes: h,w of the patch grid)                                    */
  int ph, pw, chan;     /* patch modes: patch size and image channels                             */
  float eps;            /* rms-norm epsilon                                                       */
  float out_add;        /* KD_EPI_STORE: constant added to every output (AdaRMSNorm's "+1")       */
  float sigma_data;     /* patch modes: Karras preconditioner                                     */
  const float* A;       /* plain: [M,K]; merge: [B,2gh,2gw,K/4]; patch: image [B,chan,gh*ph,gw*pw] */
  const float* W;       /* [N,K]  (GEGLU: [2N,K], value rows first)                               */
  float* C;             /* store/residual/geglu: [M,N]; split: [B,2gh,2gw,N/4]; unpatch: image     */
  const float* R;       /* residual: [M,N]; split: skip [B,2gh,2gw,N/4]; unpatch: x_in image       */
  const float* scale;   /* norm scales                                                            */
  const float* sigma;   /* [B] per-sample sigma (patch modes; NULL = no preconditioning)           */
  const float* fac;     /* split: device pointer to the lerp factor                               */
  int precision;        /* KD_PREC_*                                                              */
  const void* Wp;       /* KD_PREC_SPLIT3: packed split image of W from kd_pack_weight_bf16x3     */
  int n_heads;          /* KD_EPI_QKV: N == 3 * n_heads * 64; token of row m = m % rows_per_sample   */
  const float* qk_scale;  /* KD_EPI_QKV: [n_heads] cosine-sim scale (self_attn.scale)                 */
  const float* rope_cos;  /* KD_EPI_QKV: [rows_per_sample, n_heads, 16] cos / sin of AxialRoPE theta  */
  const float* rope_sin;
  int qkv_packed;       /* KD_EPI_QKV + KD_PREC_SPLIT3: store every 4-column chunk of q, k, v as [hi: 4 x bf16][lo: 4 x bf16]
                           (hi = bf16(x), lo = bf16(x - hi)) in the 16 bytes of its 4 floats -- the operand format of the
                           split-bf16x3 attention cores, which then take it as stored (their prep = 2)        */
  const float* rope_pos;  /* kd_gemm_bf16 + KD_EPI_QKV: [rows_per_sample, 2] axial position (y, x) of every token       */
  const float* rope_freq; /* kd_gemm_bf16 + KD_EPI_QKV: [n_heads, 8] AxialRoPE freqs / (2 pi) (angles in revolutions); 32-byte aligned */
  /* ---- KD_PREC_SPLIT3 with PRE-SPLIT operands (round 3; kd_gemm_f32 only, norm must be 0, a_mode KD_A_PLAIN) ---------------------
   * a_split: A is not fp32 but two bf16 planes [M, K] (2 bytes per element): `A` = hi = bf16_rne(a), `A_lo` = bf16_rne(a - hi), as
   *          written by kd_norm_split_f32 or by a producer GEMM with c_split.  Both operands then move by LDS-DMA (gemm_x3t.hip).
   * c_split: the result is stored as two such planes ([M, N]: `C` = hi, `C_lo` = lo) instead of fp32 -- the A operand of the next
   *          a_split GEMM (KD_EPI_GEGLU -> down projection).  Not with KD_EPI_QKV (its split form is qkv_packed).                 */
  int a_split, c_split;
  const void* A_lo;
  void* C_lo;
  int per_row;          /* kd_gemm_f32, products with one row per SAMPLE (the conditioning chain): always use the per-row fp32 FMA
                           kernel, also above its 128-row default limit.  A row's result then does not depend on how many rows
                           share the launch, so the conditioning of a whole sigma schedule (steps x batch rows in one launch)
                           is bit-identical with computing it step by step */
} KdGemm;

int kd_gemm_f32(const KdGemm* desc, void* stream);

/* The same fused GEMM in bf16 arithmetic (precision must be KD_PREC_BF16).  Buffers: A, C, R are bf16 row-major (2 bytes per
 * element) EXCEPT the image side of the patch modes, which stays fp32 like the solver state: A of KD_A_PATCH_NCHW, C and R of
 * KD_EPI_UNPATCH_NCHW.  scale / sigma / fac / qk_scale are fp32.  Wp = image from kd_pack_weight_bf16 (W itself is not read).
 * KD_EPI_QKV computes the RoPE angles in the epilogue from rope_pos / rope_freq (hardware sin / cos) instead of reading
 * rope_cos / rope_sin tables.  Products: one v_mfma_f32_32x32x16_bf16 each, fp32 accumulation; RMS statistics, GELU, RoPE,
 * lerp and the Karras scalings in fp32 registers; one rounding to bf16 at the store. */
int kd_gemm_bf16(const KdGemm* desc, void* stream);
long long kd_packed_weight_bytes_bf16(int N, int K, int geglu);
/* W [N or 2N (geglu), K] fp32 -> blocks [n-tile][k-step][128 rows][64 k] bf16 (16 KiB each, the kernels' swizzled LDS image).
 * `geglu` selects the layout, as two bits: bit 0 = GEGLU rows (value / gate rows interleaved per 32 outputs), bit 1 = the k order in
 * which an MFMA result holds a row (inside every group of 16 k: 0-3, 8-11, 4-7, 12-15): 2 = the down projection of kd_ffn_bf16,
 * 3 = its up projection when the out projection is fused in front (KdFfn.attn). */
int kd_pack_weight_bf16(const float* W, void* out, int N, int K, int geglu, void* stream);

/* Fused feed-forward block in bf16 arithmetic:  out = x + down_proj(GEGLU(up_proj(AdaRMSNorm(x)))).
 * Replaces FeedForwardBlock.forward, image_transformer_v2.py:487-493 (norm :155-166, LinearGEGLU :132-139, dropout = identity at
 * inference, Linear :126-129, residual :493) -- the pair kd_gemm_bf16(KD_EPI_GEGLU) + kd_gemm_bf16(KD_EPI_RESIDUAL) without the
 * d_ff-wide hidden activation ever leaving the chip.  x, out: bf16 [M, K] (out may be x); scale: fp32 norm scales, row m uses
 * scale + (m / rows_per_sample) * scale_stride; Wp_up = kd_pack_weight_bf16(up_proj.weight [2 d_ff, K], N = d_ff, geglu = 1);
 * Wp_down = kd_pack_weight_bf16(down_proj.weight [K, d_ff], N = K, K = d_ff, geglu = 2).
 * Shapes: K == 128 or 256, d_ff % 64 == 0; anything else returns KD_EINVAL and the caller uses the pair.  kd_ffn_bf16_supported
 * additionally says where the fused form is the FASTER one (K == 128 and M >= 16384; K == 256 only with option "ffn_fused_256"). */
typedef struct KdFfn {
  const void* x;
  void* out;
  const float* scale;
  int scale_stride, rows_per_sample;
  float eps;
  const void* Wp_up;
  const void* Wp_down;
  int M, K, d_ff;
  /* Both NULL or both set: the attention block's out projection fused in front of the block (image_transformer_v2.py:473-476 then
   * :487-493):  x' = x + attn Wout^T;  out = x' + down(GEGLU(up(norm(x')))).  attn = [M, K] in the activation type of the call (the
   * attention core's output, heads merged), Wp_out = the packed out_proj.weight [K, K] (N = K, K, geglu = 0) and Wp_up must then be packed
   * with geglu = 3 (the k order in which an MFMA result holds a row).  kd_ffn_f32 takes it at K == 128 and K == 256 (fp32 attn,
   * kd_pack_weight_bf16x3 images); kd_ffn_bf16 at K == 128 (bf16 attn, kd_pack_weight_bf16 images; other K: KD_EINVAL). */
  const void* attn;
  const void* Wp_out;
} KdFfn;
int kd_ffn_bf16_supported(int M, int K, int d_ff);
int kd_ffn_bf16(const KdFfn* desc, void* stream);
/* The same block in fp32-parity arithmetic (KD_PREC_SPLIT3: fp32 x / out, three split-bf16 MFMA terms per product, fp32 accumulate):
 * Wp_up = kd_pack_weight_bf16x3(up_proj.weight, N = d_ff, K, geglu = 1), Wp_down = kd_pack_weight_bf16x3(down_proj.weight [K, d_ff],
 * N = K, K = d_ff, geglu = 2).  K == 128 or 256, d_ff % 64 == 0; out may be x.  kd_ffn_f32_supported says where it is the faster form
 * (M >= 2048; option "ffn_x3" = 0 answers no).  At K == 128 the kernel runs two workgroups per CU over half tiles of 32 hidden features
 * (option "ffn_x3_half" = 0: the one-workgroup form; same results). */
int kd_ffn_f32_supported(int M, int K, int d_ff);
int kd_ffn_f32(const KdFfn* desc, void* stream);
/* Neighbourhood attention core + out projection + residual + feed-forward block in ONE launch (KD_PREC_SPLIT3; csrc/attn_ffn_x3.hip):
 * what kd_attn_na2d_f32(qkv, att, ..., prep = 2) followed by kd_ffn_f32(desc with attn = att, Wp_out) computes, bit for bit, without the
 * attention rows' round trip through HBM (desc->attn is not read).  Kernel size 7, 2 heads of 64 (K == 128), H % 8 == 0, W % 16 == 0,
 * desc->M == batch H W, desc->rows_per_sample == H W; kd_attn_ffn_f32_supported says whether a shape is taken (and kd_ffn_f32_supported's
 * answer for the block; option "attn_ffn_x3" = 0 answers no). */
int kd_attn_ffn_f32_supported(int batch, int H, int W, int nh, int ks, int K, int d_ff);
int kd_attn_ffn_f32(const float* qkv, const KdFfn* desc, int batch, int H, int W, int nh, int ks, void* stream);

/* One-off packing of a weight for KD_PREC_SPLIT3 (weights are static during sampling): W [N or 2N (geglu == 1), K]
 * fp32 -> `out`, kd_packed_weight_bytes(N, K, geglu) bytes: [n-tile][k-step][hi|lo][128 rows][32 bf16] in the
 * kernel's swizzled LDS order, zero-padded.  N is the OUTPUT width (GEGLU: d_ff, W has 2*d_ff rows).
 * `geglu`, two bits as for kd_pack_weight_bf16: 0 plain, 1 GEGLU rows, 2 the k order of kd_ffn_f32's down projection (inside every
 * group of 16 k: 0-3, 8-11, 4-7, 12-15), 3 both (its up projection behind a fused out projection). */
long long kd_packed_weight_bytes(int N, int K, int geglu);
int kd_pack_weight_bf16x3(const float* W, void* out, int N, int K, int geglu, void* stream);

/* AdaRMSNorm / RMSNorm (image_transformer_v2.py:98-103, :155-166) of fp32 rows, written as the two bf16 planes of an a_split GEMM
 * operand: y[m, :] = x[m, :] * (scale[b(m) * scale_stride + :] * rsqrt(mean(x[m, :]^2) + eps)), hi = bf16_rne(y), lo = bf16_rne(y - hi);
 * b(m) = m / rows_per_sample.  scale == NULL: plain split of x (no norm).  K % 8 == 0, K <= 2048.  Used for the widths the fused norm ->
 * projection kernels (kd_gemm_f32 with norm = 1: K = 128 / 256 / 512, in registers) do not take -- 384, 640, ..., 2048 (K % 128 == 0):
 * the planes then feed an a_split kd_gemm_f32.  None of the shipped configs has such a width; tests/test_model_gpu.py covers 384 and 1152. */
int kd_norm_split_f32(const float* x, const float* scale, int scale_stride, int rows_per_sample, void* hi, void* lo, int M, int K,
                      float eps, void* stream);

/* Stand-alone RMS norm over the last dim (mapping network, image_transformer_v2.py:142-152):
 * y[m,:] = x[m,:] * scale[:] * rsqrt(mean(x[m,:]^2) + eps).  d <= 4096, d % 4 == 0. */
int kd_rmsnorm_f32(const float* x, const float* scale, float* y, int rows, int d, float eps, void* stream);

/* Conditioning front end (image_transformer_v2.py:734-740 + layers.py:285-293 FourierFeatures):
 * ff[b, :] = [cos(2*pi*c*w_j), sin(2*pi*c*w_j)], c = log(sigma_b)/4, w = time_emb.weight [half]. */
int kd_fourier_sigma_f32(const float* sigma, const float* weight, float* ff, int batch, int half, void* stream);
/* generic FourierFeatures for aug_cond: ff[b,:] = [cos(f), sin(f)], f = 2*pi * in[b,:] @ w^T, w [half, in_dim] */
int kd_fourier_f32(const float* in, const float* weight, float* ff, int batch, int in_dim, int half, void* stream);
/* out[b,:] = a[b,:] + (b_rows ? b[b,:] : b[:]) + (emb ? emb[ids[b],:] : 0) + (c ? c[b,:] : 0) */
int kd_cond_sum_f32(float* out, const float* a, const float* b, int b_rows, const float* emb,
                    const long long* ids, const float* c, int batch, int d, void* stream);

/* ------------------------------------------------------------------------------------------
 * q/k preparation, in place on a qkv buffer [tokens_total, 3, nh, 64]:
 *   q,k <- rope( x * sqrt(scale_h) * rsqrt(sum x^2 + eps) ),   v untouched.
 * Replaces scale_for_cosine_sim (image_transformer_v2.py:106-114) + apply_rotary_emb_
 * (:187-231, in place on a view).  cos/sin: [tokens_per_sample, nh, 16] tables of
 * AxialRoPE.forward's theta (:245-248), computed once on the host.
 * The attention kernels below take `prep`:
 *   0  q, k already prepared (by this call or by the KD_EPI_QKV epilogue), fp32
 *   1  raw fp32 q, k: prepared on the fly (needs scale_h, cos_t, sin_t)
 *   2  prepared AND stored split (KdGemm.qkv_packed: [hi: 4 x bf16][lo: 4 x bf16] per 4-column chunk): the split-bf16x3
 *      cores use the operands as stored; not available with KD_PREC_EXACT
 * `precision` (KD_PREC_EXACT / KD_PREC_SPLIT3) selects the arithmetic of the two products, as in KdGemm; the neighbourhood
 * core has the split-bf16x3 form only (the argument is accepted for symmetry). */
int kd_qk_prep_f32(float* qkv, const float* scale_h, const float* cos_t, const float* sin_t,
                   int batch, int tokens_per_sample, int nh, float eps, void* stream);

/* Dense softmax attention per (sample, head) over all T tokens (any T; T > 256 streams key blocks with an online
 * softmax and is served by the split-bf16x3 core only), softmax scale 1.0.
 * Replaces F.scaled_dot_product_attention / flash_attn_qkvpacked_func at
 * image_transformer_v2.py:383,392.  out: [batch*T, nh*64]. */
int kd_attn_global_f32(const float* qkv, float* out, int batch, int T, int nh,
                       int prep, const float* scale_h, const float* cos_t, const float* sin_t, float eps,
                       int precision, void* stream);

/* Shifted-window attention (window ws x ws tokens, ws in {4, 8, 16}), roll/window/mask/unwindow
 * folded into addressing.  Replaces apply_window_attention image_transformer_v2.py:319-337
 * (+ :253-316).  shift is 0 or ws/2. */
int kd_attn_window_f32(const float* qkv, float* out, int batch, int H, int W, int nh, int ws, int shift,
                       int prep, const float* scale_h, const float* cos_t, const float* sin_t, float eps,
                       int precision, void* stream);

/* 2-D neighbourhood attention, kernel ks x ks, window clamped inside the image, dilation 1, heads-last.  Replaces
 * natten.functional.na2d(q,k,v,kernel_size,scale=1.0) image_transformer_v2.py:428 (and the unfused pair :437-439; kernel_size is
 * the block's constructor argument, :399-410).  ks: odd, 3 .. 13 with split-stored operands (prep = 2: what the package's fp32-parity
 * mode runs -- 7 is the shipped size, 3 / 5 / 9 the same kernel with other constants, 11 / 13 a densely packed patch form);
 * ks == 7 only for fp32 operands (prep 0 / 1) and with option "attn_x3" = 0.  H, W >= ks. */
int kd_attn_na2d_f32(const float* qkv, float* out, int batch, int H, int W, int nh, int ks,
                     int prep, const float* scale_h, const float* cos_t, const float* sin_t, float eps,
                     int precision, void* stream);

/* The three attention cores in bf16 arithmetic (KD_PREC_BF16): qkv is the bf16 output of kd_gemm_bf16's KD_EPI_QKV epilogue
 * ([tokens, 3, nh, 64], q and k already prepared), out is bf16 [tokens, nh * 64].  bf16 MFMA products, fp32 scores / softmax /
 * accumulators.  Same reference call sites as the fp32 entry points above; kd_attn_na2d_bf16 takes kernel sizes 3 .. 13 (odd;
 * 3 .. 9 in the tuned form, 11 and 13 in a general one). */
int kd_attn_global_bf16(const void* qkv, void* out, int batch, int T, int nh, void* stream);
int kd_attn_window_bf16(const void* qkv, void* out, int batch, int H, int W, int nh, int ws, int shift, void* stream);
int kd_attn_na2d_bf16(const void* qkv, void* out, int batch, int H, int W, int nh, int ks, void* stream);

/* The global-attention block in front of its out projection as ONE launch (round 5; k_diffusion/models/image_transformer_v2.py:370-392:
 * norm -> qkv_proj -> scale_for_cosine_sim_qkv -> apply_rotary_emb_ -> scaled_dot_product_attention / flash_attn_qkvpacked_func).  `d` is the
 * descriptor of the block's qkv projection exactly as kd_gemm_bf16 takes it (A = residual stream, Wp = packed qkv weight, scale /
 * scale_stride / rows_per_sample = the AdaRMSNorm scales, qk_scale, rope_pos, rope_freq, n_heads; epi = KD_EPI_QKV, norm = 1, precision =
 * KD_PREC_BF16), except that C receives the ATTENTION OUTPUT [M, n_heads * 64] bf16: q, k, v never reach HBM.  One workgroup per (sample,
 * head).  Shapes: 256 tokens per sample, K = 64 * n_heads in {256, 512}, N = 3 K, M % 256 == 0 (kd_attn_block_bf16_supported tells);
 * anything else returns KD_EINVAL and the caller issues kd_gemm_bf16 + kd_attn_global_bf16, whose results this entry reproduces bit for bit.
 * (Round 5 also offered the block's out projection in the same launch behind a cross-workgroup rendezvous; it measured level with the separate
 * launch and was removed in round 6 -- a spin-wait between workgroups has no place in a library that must never hang or corrupt silently.) */
int kd_attn_block_bf16_supported(int tokens_per_sample, int width, int n_heads);
int kd_attn_block_bf16(const KdGemm* d, void* stream);

/* AdaRMSNorm -> wide projection in the same form (round 5): the FF block's norm -> up projection + GEGLU (image_transformer_v2.py:487-491) and,
 * for the levels whose attention core is a launch of its own, norm -> qkv projection + cosine-sim scale + RoPE (:370-380, :415-425).  A workgroup
 * per (256-row group, slice of six 64-row half blocks of the packed weight), the group's rows normalised once into register fragments, six passes
 * over K.  `d` is the projection's descriptor as kd_gemm_bf16 takes it (epi = KD_EPI_GEGLU with N = d_ff, or KD_EPI_QKV with N = 3 K; norm = 1,
 * precision = KD_PREC_BF16); the result is bit-identical to kd_gemm_bf16(d).  Shapes: rows per sample a multiple of 256, K in {256, 512},
 * d_ff % 192 == 0 (kd_proj_block_bf16_supported tells); else KD_EINVAL. */
int kd_proj_block_bf16_supported(int tokens_per_sample, int width, int n, int epi);
int kd_proj_block_bf16(const KdGemm* d, void* stream);

/* fp8 arithmetic mode (round 6; BASELINE configs[4] "fp8 MFMA weights" -- no reference counterpart: convert_for_inference.py:23 stops at
 * fp16 / bf16): the AdaRMSNorm -> wide projections of the K = 256 / 512 levels (image_transformer_v2.py:370-380 / :415-425 norm -> qkv_proj +
 * cosine-sim scale + RoPE; :487-491 norm -> up_proj + GEGLU; norm -> plain store) on the block-scaled fp8 matrix instruction
 * (v_mfma_scale_f32_32x32x64_f8f6f4, 2x the bf16 MFMA rate).  Weights: OCP e4m3 with ONE power-of-two scale per output channel
 * (checkpoint.quantize_fp8's rule: an fp8 checkpoint enters bit for bit; any other fp32 weight is rounded by kd_pack_weight_mx8).
 * Activations: x (bf16) * AdaRMSNorm scale (fp32) quantised per (row, 32-k block) to e4m3 with a power-of-two block scale 2^ceil(log2(amax / 448))
 * (OCP microscaling: one E8M0 byte per block, no saturation); fp32 accumulation; the RMS row factor (fp32 statistics of the unquantised row)
 * and the epilogues as in kd_gemm_bf16.  `d` is the projection's descriptor as kd_gemm_bf16 takes it (bf16 A / C, norm = 1, epi = KD_EPI_STORE /
 * KD_EPI_QKV / KD_EPI_GEGLU, precision = KD_PREC_BF16, rows_per_sample set) except that Wp points at the kd_pack_weight_mx8 image.
 * Shapes: K in {256, 512}, N a multiple of 128 (GEGLU: d_ff a multiple of 64), M >= 128 (kd_gemm_mx8_supported tells); else KD_EINVAL.
 * With c_split = 1 (KD_EPI_GEGLU only) the result leaves as the NEXT fp8 product's operand: C = e4m3 rows [M, N] (bytes), C_lo = one E8M0
 * byte per (row, 32 features) [M, N / 32], the activations' rule.
 * Second form, norm = 0 and a_split = 1 (:492 down_proj + the skip add; epi = KD_EPI_STORE / KD_EPI_RESIDUAL): A = such e4m3 rows [M, K],
 * A_lo = their scale bytes [M, K / 32] (4-byte aligned), both operands by LDS-DMA; K in {256, 512, 768, 1536}, N a multiple of 128; C / R bf16.
 * The arithmetic is restated in oracle/hdit.py (mx8_quantize_rows / mx8_quantize_weight). */
long long kd_packed_weight_bytes_mx8(int N, int K, int geglu);
int kd_pack_weight_mx8(const float* W, void* out, int N, int K, int geglu, void* stream);
int kd_gemm_mx8_supported(int M, int N, int K, int epi, int norm);
int kd_gemm_mx8(const KdGemm* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Solver step arithmetic (k_diffusion/sampling.py), one fused elementwise launch per step with
 * host-precomputed fp32 coefficients.  Operation order follows the reference expression trees
 * exactly (no FMA contraction) so results are bit-identical to the reference's CPU path.
 *   KD_STEP_EULER      : out = x + ((x - den) / c0) * c1                    (:129-134, :176, :558-560)
 *   KD_STEP_HEUN_PRED  : aux_out = (x - den)/c0 ; out = x + aux_out * c1     (:170,:179)
 *   KD_STEP_HEUN_CORR  : d2 = (x2 - den)/c0 ; out = x + ((aux + d2)/2) * c1   (:181-183)  [x2 = in2]
 *   KD_STEP_DPMPP_2M1  : out = c0 * x - c1 * den                             (:600, also :533,:535,:571,:579)
 *   KD_STEP_DPMPP_2M2  : out = c0 * x - c1 * (c2 * den - c3 * in2)            (:604-605)   [old = in2]
 *   KD_STEP_ADD_NOISE  : out = x + ((den * c0) * c1) * c2                    (:154,:572,:580,:648)  [den = noise]
 *   KD_STEP_LERP2      : out = c0 * den + c1 * in2                           (:578)
 *   KD_STEP_AXPY       : out = x + den * c0                                  (:127, :276 terms)
 *   KD_STEP_EULER_FROM : out = x + ((in2 - den) / c0) * c1                   (:213-214, :241-242)  [x2 = in2]
 *   KD_STEP_AXPBY      : out = c0 * x + c1 * den                             (:638, :679)
 *   KD_STEP_ADD_DIFF   : out = x + c0 * (den - in2)                          (:643, :645)
 *   KD_STEP_TO_D       : out = (x - den) / c0                                (:46-48 to_d)
 */
enum { KD_STEP_EULER = 0, KD_STEP_HEUN_PRED = 1, KD_STEP_HEUN_CORR = 2, KD_STEP_DPMPP_2M1 = 3,
       KD_STEP_DPMPP_2M2 = 4, KD_STEP_ADD_NOISE = 5, KD_STEP_LERP2 = 6, KD_STEP_AXPY = 7,
       KD_STEP_EULER_FROM = 8, KD_STEP_AXPBY = 9, KD_STEP_ADD_DIFF = 10, KD_STEP_TO_D = 11 };
int kd_sampler_step_f32(int op, const float* x, const float* den, const float* in2, float* out, float* aux,
                        float c0, float c1, float c2, float c3, long long n, void* stream);

/* Karras preconditioner for a foreign inner model (k_diffusion/layers.py:88-90):
 *   kd_precond_in : y = x * c_in(sigma_b)
 *   kd_precond_out: y = f * c_out(sigma_b) + x * c_skip(sigma_b)          per_sample = C*H*W */
int kd_precond_in_f32(const float* x, const float* sigma, float* y, float sigma_data, int batch, long long per_sample, void* stream);
int kd_precond_out_f32(const float* f, const float* x, const float* sigma, float* y, float sigma_data, int batch,
                       long long per_sample, void* stream);

/* DPM-Solver (k_diffusion/sampling.py:333-480) in the reference's operation order:
 *   kd_dpm_eps_f32:     out = (x - denoised) / sigma                                  (DPMSolver.eps :354)
 *   kd_dpm_combine_f32: out = x - a * eps [- b * (eps_r - eps) when eps_r != NULL]      (x_1 :363, u1 :371, x_2 :373, u2 :384, x_3 :387)
 *   kd_dpm_error_f32:   the adaptive solver's local error (:464-465) as kd_dpm_error_partials() per-block partial sums of
 *                       ((x_low - x_high) / max(atol, rtol * max(|x_low|, |x_prev|)))^2 on a fixed grid (reproducible total). */
int kd_dpm_eps_f32(float* out, const float* x, const float* denoised, float sigma, long long n, void* stream);
int kd_dpm_combine_f32(float* out, const float* x, const float* eps, const float* eps_r, float a, float b, long long n, void* stream);
int kd_dpm_error_partials(void);
int kd_dpm_error_f32(const float* x_low, const float* x_high, const float* x_prev, float atol, float rtol, long long n, float* partial,
                     void* stream);

/* Foreign-model wrappers (k_diffusion/external.py): the image-sized arithmetic of their forward()s,
 *   y[b, :] = f[b, :] * a[b] (+ x[b, :] * c[b] when x != NULL)          (:38, :113, :162)
 * and the discrete schedule's sigma <-> t maps over an ascending table log_sigmas[n] (:66-84). */
int kd_rows_affine_f32(const float* f, const float* x, const float* a, const float* c, float* y, int batch, long long per_sample, void* stream);
int kd_sigma_to_t_f32(const float* sigma, const float* log_sigmas, float* t, int count, int n, int quantize, void* stream);
int kd_t_to_sigma_f32(const float* t, const float* log_sigmas, float* sigma, int count, int n, void* stream);

/* Brownian-interval noise (stands in for torchsde.BrownianTree behind
 * k_diffusion/sampling.py:65-114): out[b, i] = sign * (W_b,i(t1) - W_b,i(t0)) * inv_norm where W is
 * a virtual Brownian tree on [T0, T1] (depth-`depth` dyadic bridge, Philox4x32-10 keyed by
 * seeds[b], counter = (element index, tree node)); path-consistent across nested queries.
 * kd_brownian_cached_f32 is the same function with the end-point values W(t0) / W(t1) kept by the
 * caller (the tensors torchsde's tree caches on the host, sampling.py:72-79): have0 / have1 != 0
 * reads that end point from w0 / w1 [batch, per_sample] instead of descending the tree; otherwise it
 * is computed and, when the pointer is non-NULL, stored there for a later query. */
int kd_brownian_f32(float* out, const unsigned long long* seeds, int batch, long long per_sample,
                    double T0, double T1, double t0, double t1, float mult, int depth, void* stream);
int kd_brownian_cached_f32(float* out, float* w0, float* w1, int have0, int have1, const unsigned long long* seeds, int batch,
                           long long per_sample, double T0, double T1, double t0, double t1, float mult, int depth, void* stream);

/* Index-addressed standard normals: the start noise of a sampling run (/root/reference sample.py:59, `torch.randn([n, C, H, W],
 * device=device) * sigma_max`) and the randn_like of the ancestral samplers (k_diffusion/sampling.py:61-62), drawn on the device as a
 * function of (seeds[b], draw, element) only -- so image i of a seeded job is the same for any batch size / GPU count (the reference's
 * draw comes from rank-local generator state).  out[b, e] = scale * z, z from Philox4x32-10 (key seeds[b], counter (e >> 2, draw | 2^63))
 * through two Box-Muller pairs per block; `draw` < 2^63 numbers the calls of one run (0 = start noise).  out: 16-byte aligned. */
int kd_randn_f32(float* out, const unsigned long long* seeds, int batch, long long per_sample, unsigned long long draw, float scale,
                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Forward-mode derivatives (tangents) for log_likelihood (k_diffusion/sampling.py:280-301), fp32 arithmetic: a DUAL pass runs the
 * primal x and its tangent x_dot side by side.  The reference takes v . (v^T J) with a reverse-mode pass through the model; this
 * package takes v^T (J v) forward.  The linear pieces of the network run their tangent on kd_gemm_f32; these are the nonlinear ones.
 * Products are fp32 FMAs on the vector ALU; every reduction has a fixed order (bit-identical on repeat, no atomics).
 *   kd_rmsnorm_jvp_f32 : rms_norm / AdaRMSNorm (image_transformer_v2.py:98-103, :142-166), rows x d (d % 4 == 0, scale_stride % 4 == 0):
 *                        r = rsqrt(mean(x^2) + eps), s = scale[(row / rows_per_sample) * scale_stride + :] (stride 0: a shared gain),
 *                        y = s * x * r,  y_dot = s * (x_dot * r - x * r^3 * mean(x * x_dot)).
 *   kd_geglu_jvp_f32   : linear_geglu's gate (:89-95): h = [a | g] rows of 2 d_ff (value first), y = a * gelu(g),
 *                        y_dot = a_dot * gelu(g) + a * gelu'(g) * g_dot, erf-GELU with gelu'(g) = Phi(g) + g * phi(g).
 *   kd_qk_prep_jvp_f32 : kd_qk_prep_f32 (:106-121, :187-231) in place on qkv AND its tangent qkv_dot (same layout and tables): with
 *                        rho = rsqrt(sum q^2 + eps), c = sqrt(scale_h), q' = c q rho, q'_dot = c (q_dot rho - q rho^3 (q . q_dot)), then
 *                        the same RoPE rotation of both.
 *   kd_attn_{global,window,na2d}_jvp_f32 : softmax attention (scale 1.0) on prepared q, k and its tangent, geometry as the fp32 cores
 *                        (global: any T; window: ws 4 / 8 / 16, shift 0 .. ws-1 under the reference's mask, :253-337; neighbourhood:
 *                        odd ks 3 .. 13, clamped window, H, W >= ks): with l_j = q . k_j and l_dot_j = q_dot . k_j + q . k_dot_j,
 *                        o = sum e_j v_j / Z and o_dot = (sum e_j l_dot_j v_j + sum e_j v_dot_j) / Z - (sum e_j l_dot_j / Z) o.
 *                        out / out_dot: [tokens, nh * 64].
 *   kd_ll_div_f32      : d = (x - D) / sigma_b (to_d, sampling.py:46) and d_ll[b] = sum over sample b of v * (v - D_dot) / sigma_b
 *                        (the divergence of d along v: v . J_d v).  sigma: [batch] device floats.
 *   kd_gauss_logp_f32  : out[b] = add[b] + sum over sample b of log N(z; 0, sigma^2) (add may be NULL).
 *   kd_rk_combine_f32  : out = y0 + sum_j c[j] * k[j]  (y0 may be NULL), nk <= 7 terms; k (device pointers) and c are HOST arrays read
 *                        at the call.
 *   kd_rk_error_f32    : kd_rk_error_partials() per-workgroup partial sums, on a fixed grid, of
 *                        (sum_j c[j] k[j] / (atol + rtol * max(|y0|, |y1|)))^2 (y1 NULL: |y0| alone); the caller adds them up. */
int kd_rmsnorm_jvp_f32(const float* x, const float* x_dot, const float* scale, int scale_stride, int rows_per_sample, float* y, float* y_dot,
                       int rows, int d, float eps, void* stream);
int kd_geglu_jvp_f32(const float* h, const float* h_dot, float* y, float* y_dot, int rows, int d_ff, void* stream);
int kd_qk_prep_jvp_f32(float* qkv, float* qkv_dot, const float* scale_h, const float* cos_t, const float* sin_t, int batch,
                       int tokens_per_sample, int nh, float eps, void* stream);
int kd_attn_global_jvp_f32(const float* qkv, const float* qkv_dot, float* out, float* out_dot, int batch, int T, int nh, void* stream);
int kd_attn_window_jvp_f32(const float* qkv, const float* qkv_dot, float* out, float* out_dot, int batch, int H, int W, int nh, int ws,
                           int shift, void* stream);
int kd_attn_na2d_jvp_f32(const float* qkv, const float* qkv_dot, float* out, float* out_dot, int batch, int H, int W, int nh, int ks,
                         void* stream);
int kd_ll_div_f32(const float* x, const float* D, const float* D_dot, const float* v, const float* sigma, float* d, float* d_ll, int batch,
                  long long per_sample, void* stream);
int kd_gauss_logp_f32(const float* z, float sigma, const float* add, float* out, int batch, long long per_sample, void* stream);
int kd_rk_combine_f32(float* out, const float* y0, const float* const* k, const float* c, int nk, long long n, void* stream);
int kd_rk_error_partials(void);
int kd_rk_error_f32(const float* const* k, const float* c, int nk, const float* y0, const float* y1, float atol, float rtol, long long n,
                    float* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reverse-mode derivatives (vector-Jacobian products) for gradients w.r.t. the denoiser's input (gradient guidance,
 * k_diffusion/sampling.py:286-294's autograd form of log_likelihood), fp32 arithmetic.  The backward pass recomputes the primal on the
 * unfused fp32 path and walks the network in reverse; its linear pieces run on kd_gemm_f32 with transposed weights, these are the others.
 * The conditioning and the weights are held fixed.  Products are fp32 FMAs on the vector ALU; every reduction has a fixed order
 * (bit-identical on repeat, no atomics).
 *   kd_rmsnorm_vjp_f32 : rms_norm / AdaRMSNorm (image_transformer_v2.py:98-103, :142-166), rows x d (d % 4 == 0, scale_stride % 4 == 0),
 *                        scale as in kd_rmsnorm_jvp_f32: r = rsqrt(mean(x^2) + eps), g_x = s * g_y * r - x * r^3 * mean(x * s * g_y)
 *                        (+ g_add, the gradient a residual add passes through; NULL for none; g_x may be g_add).
 *   kd_geglu_vjp_f32   : linear_geglu's gate (:89-95): h = [a | g] rows of 2 d_ff (value first), g_y rows of d_ff ->
 *                        g_h = [g_y * gelu(g) | g_y * a * gelu'(g)], erf-GELU.
 *   kd_qk_prep_vjp_f32 : the transpose of kd_qk_prep_f32 (:106-121, :187-231) at the UNPREPARED qkv: g_qkv (the gradient w.r.t. the
 *                        prepared q, k) is rewritten in place, u = R^T g, g_q = c rho u - c rho^3 q (q . u) with rho = rsqrt(sum q^2 + eps),
 *                        c = sqrt(scale_h); the v part of g_qkv is left as it is.
 *   kd_attn_{global,window,na2d}_vjp_f32 : softmax attention (scale 1.0) on prepared q, k, geometry and limits as the _jvp_ cores: g_out
 *                        [tokens, nh * 64] -> g_qkv [tokens, 3 * nh * 64] (every element written).  Two launches (flash-attention-2): a
 *                        query sweep that writes g_q and the per-query log-sum-exp / rowsum(dO * O) into lse / dsum ([batch, nh, T]
 *                        device workspace), then a key sweep over the queries that attend each key (neighbourhood: the inverse window,
 *                        which near a border holds more than ks queries per axis) that writes g_k, g_v.
 *   kd_precond_vjp_f32 : y = coef(g_coef) * g + coef(h_coef) * h per sample (h may be NULL), coef one of the KD_PC_* Karras scalings of
 *                        sigma[b] (layers.py:70-74): the transposes of the preconditioning (D = F(x c_in) c_out + x c_skip). */
enum { KD_PC_ONE = 0, KD_PC_SKIP = 1, KD_PC_OUT = 2, KD_PC_IN = 3 };
int kd_rmsnorm_vjp_f32(const float* x, const float* g_y, const float* scale, int scale_stride, int rows_per_sample, const float* g_add, float* g_x,
                       int rows, int d, float eps, void* stream);
int kd_geglu_vjp_f32(const float* h, const float* g_y, float* g_h, int rows, int d_ff, void* stream);
int kd_qk_prep_vjp_f32(const float* qkv, float* g_qkv, const float* scale_h, const float* cos_t, const float* sin_t, int batch,
                       int tokens_per_sample, int nh, float eps, void* stream);
int kd_attn_global_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int T, int nh, void* stream);
int kd_attn_window_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int H, int W, int nh, int ws,
                           int shift, void* stream);
int kd_attn_na2d_vjp_f32(const float* qkv, const float* g_out, float* g_qkv, float* lse, float* dsum, int batch, int H, int W, int nh, int ks,
                         void* stream);
int kd_precond_vjp_f32(const float* g, int g_coef, const float* h, int h_coef, const float* sigma, float sigma_data, float* y, int batch,
                       long long per_sample, void* stream);

/* Parameter gradients of the HDiT denoiser and its training loss (csrc/wgrad_f32.hip; models/vjp.py, layers.Denoiser.loss).  fp32 arithmetic,
 * fixed reduction orders through caller-provided workspaces, no atomics: bit-identical on repeat.
 *   kd_wgrad_f32       : dW[N, K] (+)= alpha * sum_m G[m, n] * A[m, k] over M rows (alpha: a device scalar or NULL; accumulate: add to dW).
 *                        g_mode / a_mode (KD_WG_*, one operand at most gathered) read the rows through the token merge (fine NHWC grid of
 *                        2gh x 2gw x chan, ph = pw = 2) or the NCHW patch gather (image chan x gh*ph x gw*pw); gathered columns are ordered
 *                        (py, px, channel).  A's prologue: a_geglu (A holds [value | gate] rows of 2K, the operand is value * gelu(gate)),
 *                        row_scale[m], col_scale[(m / rows_per_sample) * col_stride + k].  The rows are cut into nchunk chunks of chunk_rows
 *                        (chunk_rows * nchunk >= M); ws holds nchunk * N * K floats.  split3 selects the arithmetic.  1: bf16 hi / lo operands,
 *                        3 MFMAs per product, fp32 accumulate (the backward pass's rule under split3 / bf16 / fp8); 0: fp32 FMAs (exact);
 *                        2: bf16 operands, 1 MFMA per product, fp32 accumulate -- each operand element is rounded to bf16 (nearest even)
 *                        after its whole prologue (gather, GEGLU, dropout mask, row_scale, col_scale), where a Linear backward under
 *                        torch.autocast(bfloat16) rounds it; opt-in (ops.wgrad(bf16=True)), 128 x 128 output tiles.  Other values: KD_EINVAL.
 *   kd_row_rrms_f32    : rrms[r] = rsqrt(mean(x[r, :]^2) + eps).
 *   kd_colsum_f32      : out[s, j] (+)= sum over rows r of segment s (rows_per_seg rows each) of a[r, j] * (b[r, j] - b2[r, j]) * row_scale[r];
 *                        b, b2, row_scale may be NULL.  ws holds rows / 64 (rounded up per segment) * cols floats.
 *   kd_attn_scale_grad_f32 : out[h] (+)= sum of colsum's q and k columns of head h ([3, nh, 64] layout) / (2 scale[h]).
 *   kd_class_emb_grad_f32  : out[c, :] (+)= sum over b ascending with ids[b] == c of g[b, :].
 *   kd_loss_prep_f32   : noised = input + noise * sigma[b], x_in = noised * c_in (layers.py:78-81).
 *   kd_loss_f32        : losses[b] = mean((f - target)^2) * c_weight, target = (input - c_skip noised) / c_out (layers.py:82-84); weighting
 *                        one of KD_LW_* (KD_LW_GIVEN: c_weight[b] from the caller).
 *   kd_loss_vjp_f32    : g_f = g_loss[b] * c_weight * 2 (f - target) / per_sample. */
enum { KD_WG_PLAIN = 0, KD_WG_MERGE2x2 = 1, KD_WG_PATCH_NCHW = 2 };
enum { KD_LW_KARRAS = 0, KD_LW_SOFT_MIN_SNR = 1, KD_LW_SNR = 2, KD_LW_GIVEN = 3 };
int kd_wgrad_f32(const float* G, int g_mode, const float* A, int a_mode, int a_geglu, long long M, int N, int K, int gh, int gw, int ph, int pw,
                 int chan, const float* row_scale, const float* col_scale, int col_stride, int rows_per_sample, const float* alpha, int accumulate,
                 int split3, int chunk_rows, int nchunk, float* ws, float* dW, void* stream);
int kd_row_rrms_f32(const float* x, float* rrms, long long rows, int d, float eps, void* stream);
int kd_colsum_f32(const float* a, const float* b, const float* b2, const float* row_scale, long long rows, int cols, long long rows_per_seg,
                  int accumulate, float* ws, float* out, void* stream);
int kd_attn_scale_grad_f32(const float* colsum, const float* scale, int nh, int accumulate, float* out, void* stream);
int kd_class_emb_grad_f32(const float* g, const long long* ids, int batch, int d, int n_cls, int accumulate, float* out, void* stream);
int kd_loss_prep_f32(const float* input, const float* noise, const float* sigma, float sigma_data, float* noised, float* x_in, int batch,
                     long long per_sample, void* stream);
int kd_loss_f32(const float* f, const float* input, const float* noised, const float* sigma, float sigma_data, int weighting, const float* c_weight,
                float* losses, int batch, long long per_sample, void* stream);
int kd_loss_vjp_f32(const float* f, const float* input, const float* noised, const float* sigma, float sigma_data, int weighting,
                    const float* c_weight, const float* g_loss, float* g_f, int batch, long long per_sample, void* stream);

/* Dropout of the training loss (the reference's nn.Dropout at image_transformer_v2.py:394, :441, :474 (attention output, after the head
 * merge, before out_proj), :491 (FF hidden, after GEGLU, before down_proj), :564 (mapping block, GEGLU output before down_proj); csrc/dropout_f32.hip,
 * models/vjp.py).  No mask is stored: the primal, the backward's recomputation and the reverse walk regenerate the same bits.
 * Mask contract:
 *   key       one int64 per loss call, drawn on the device and read through a pointer (the kernels never sync with the host);
 *   site s    2^62 | (2 i) for the attention output and 2^62 | (2 i + 1) for the FF hidden of the layer at position i of
 *             image_transformer_v2.hourglass(model); 2^62 | 2^32 | k for mapping block k (image_transformer_v2.dropout_sites);
 *   element e the row-major index in the site's tensor: [B, h, w, nh * 64] (attention), [B, h, w, d_ff] (FF), [B, mapping d_ff];
 *   mask      w = word e & 3 of philox4x32_10(key, counter (e >> 2, s)) (csrc/philox.h, the generator of kd_brownian_f32 / kd_randn_f32,
 *             whose counters never set bit 62 of the second half); keep iff w >= threshold, threshold = floor(p 2^32); y = x * m with
 *             m = keep ? scale : 0 and scale = (float)(1 / (1 - p)) computed in double (NaN and Inf stay NaN at dropped elements).
 *   kd_dropout_f32        : y = x * m over n elements (y may be x).  Also the transpose: the gradient through the site.
 *   kd_geglu_vjp_drop_f32 : kd_geglu_vjp_f32 with g_y * m in place of g_y: the same bits as kd_dropout_f32 on g_y followed by kd_geglu_vjp_f32.
 *   kd_wgrad_drop_f32     : kd_wgrad_f32 with A's plain [M, K] operand (after its GEGLU prologue) times m, element e = m K + k: dW_down =
 *                           G^T (mask * geglu(U)) without a masked hidden in memory.  bits: (M K + 31) / 32 words of device workspace that
 *                           receive the mask (bit j of word w: element 32 w + j) ahead of the GEMM.  threshold 0: kd_wgrad_f32's bits. */
int kd_dropout_f32(const float* x, float* y, long long n, const long long* key, unsigned long long site, unsigned threshold, float scale, void* stream);
int kd_geglu_vjp_drop_f32(const float* h, const float* g_y, float* g_h, int rows, int d_ff, const long long* key, unsigned long long site,
                          unsigned threshold, float scale, void* stream);
int kd_wgrad_drop_f32(const float* G, int g_mode, const float* A, int a_mode, int a_geglu, long long M, int N, int K, int gh, int gw, int ph, int pw,
                      int chan, const float* row_scale, const float* col_scale, int col_stride, int rows_per_sample, const float* alpha, int accumulate,
                      int split3, int chunk_rows, int nchunk, float* ws, float* dW, const long long* key, unsigned long long site,
                      unsigned threshold, float scale, unsigned* bits, void* stream);

/* Karras et al. augmentation of a training batch (the reference's KarrasAugmentationPipeline.__call__, k_diffusion/augmentation.py:40-89, run
 * there per image on CPU data-loader workers with scikit-image; csrc/augment_f32.hip).  Neither entry point synchronises.
 *   kd_augment_draw_f32 : raw[batch, 8] = (a0 .. a7) per sample, the reference's draws (:44-70) in its order: a0 in {0, 1} ungated;
 *                         a1 in {0, 1} * do; a2 = N(0, 1) * do; a3 = U[-pi, pi) * do; a4 = U[-pi, pi) * do and a5 = N(0, 1) * do on ONE gate;
 *                         a6 = N * do and a7 = N * do on ONE gate; every do ~ Bernoulli(a_prob), 0 <= a_prob <= 1.  The torch RNG stream of the
 *                         reference is NOT reproduced.
 * Counter contract (key: one int64 per call, read through a device pointer like the dropout key):
 *   block j of sample b = philox4x32_10(key, counter (b, 2^63 | 2^62 | j)), j = 0 .. 3, words w0 .. w3 (csrc/philox.h; the dropout sites
 *   leave bit 63 clear, kd_randn_f32 sets bit 62 only from draw 2^62 on, the Brownian tree's nodes stay below 2^62);
 *     u(w) = (w >> 8) / 2^24 in [0, 1);  gate(w) = u(w) < a_prob (fp32);  bit(w) = w >> 31;
 *     angle(w) = (u(w) - 1/2) * 6.28318501f (the fp32 below 2 pi: the result stays inside [-pi, pi));
 *     normal(wr, wa) = sqrt(-2 ln(((wr >> 8) + 1) / 2^24)) * cos(2 pi u(wa)), kd_randn_f32's Box-Muller on the hardware log2 / sqrt / cos;
 *   block 0: a0 = bit(w0);  a1 = gate(w1) ? bit(w2) : 0;  a2 = gate(w3) ? normal(block 1 w0, w1) : 0;
 *   block 1: a3 = gate(w2) ? angle(w3) : 0;
 *   block 2: g = gate(w0);  a4 = g ? angle(w1) : 0;  a5 = g ? normal(w2, w3) : 0;
 *   block 3: g = gate(w0);  (a6, a7) = g ? the pair (r cos, r sin) of normal(w2, w3), sin as cos of a quarter turn less : (0, 0);  w1 unused.
 *   kd_augment_warp_f32 : y[b] = x[b] [batch, chan, H, W] warped by raw[b], cond[batch, 9] = (a0, a1, a2, cos a3 - 1, sin a3, a5 cos a4,
 *                         a5 sin a4, a6, a7) (:75), and with mat != NULL mat[batch, 6] = the top two rows of the inverse map that was used.
 *                         The reference's matrix (:42-74; PIL's image.size is (W, H), so its `h` is W and its `w` is H), acting on
 *                         (x = column, y = row, 1), with s = a_scale, n = a_aniso, t = a_trans, R(th) = [[cos th, -sin th], [sin th, cos th]]:
 *                           M = T(W/2 - .5, H/2 - .5) S(1 - 2 a0, 1) S(1, 1 - 2 a1) S(s^a2, s^a2) R(-a3) R(a4) S(n^a5, n^-a5) R(-a4)
 *                               T(t H a6, t W a7) T(-W/2 + .5, -H/2 + .5).
 *                         Output pixel (c, r) samples x at M^-1 (c, r, 1); M^-1 is composed from the inverse factors in reverse order (libm
 *                         sincosf / exp2f, no numeric inverse) and applied as L ((c, r) - centre) + (centre - translation).  Interpolation:
 *                         scikit-image's order = 3: separable 4 x 4 Catmull-Rom p1 + 0.5 t (p2 - p0 + t (2 p0 - 5 p1 + 4 p2 - p3 + t (3 (p1 - p2)
 *                         + p3 - p0))), along W first, taps at floor(coord) - 1 .. + 2, out-of-range tap indices folded by numpy-pad 'reflect'
 *                         (d c b | a b c d | c b a, period 2 (N - 1), any distance; cval plays no part).  H, W >= 2 and H W < 2^31 - 256; a_scale,
 *                         a_aniso > 0; y must not overlap x: KD_EINVAL otherwise.  A non-finite coordinate samples inside the image (no fault). */
int kd_augment_draw_f32(const long long* key, int batch, float a_prob, float* raw, void* stream);
int kd_augment_warp_f32(const float* x, const float* raw, float a_scale, float a_aniso, float a_trans, float* y, float* cond, float* mat,
                        int batch, int chan, int H, int W, void* stream);

/* Training batches from a dataset resident in device memory as uint8, and conditioning dropout of the class labels (the reference reaches
 * CIFAR-10 / MNIST through torchvision datasets, PIL and data-loader workers, train.py:207-210, and drops labels with torch.rand, :449-450;
 * csrc/data_u8.hip).  Neither entry point synchronises.
 *   kd_batch_u8_f32      : out[b] = data[idx[b]] as fp32, b < batch: data [N, chan, H, W] uint8, planar (a CIFAR pickle row and an MNIST idx image
 *                          both are), idx [batch] int64 with every entry in [0, N) -- the CALLER's check: N is not passed and nothing is
 *                          clamped -- out [batch, chan, H, W].  Element values: (float)u / 255 * 2 - 1 with the bits of three IEEE fp32
 *                          operations in that order (utils.from_pil_image; a 256-entry table evaluated at compile time, independent of the
 *                          device's division flags).  chan H W < 2^31 - 256, any value (an image may start at any byte address: byte loads).
 *                          labels [N] int64 and class_out [batch] int64 are both NULL (unlabelled data: key, drop_rate, num_classes unused)
 *                          or both given: class_out[b] = labels[idx[b]] under the dropout rule.  out / class_out must not overlap the inputs.
 *   kd_class_dropout_i64 : out[b] = labels[b] under the dropout rule, b < batch (labels that came through a DataLoader); out may be labels.
 * Dropout rule (key: one int64 per call, read through a device pointer like the dropout and augmentation keys; may be NULL iff drop_rate is 0):
 *   sample b is dropped iff u(w0) < drop_rate (fp32), u(w) = (w >> 8) / 2^24, w0 = word 0 of philox4x32_10(key, counter (b, 2^63 | 2^62 | 2^32))
 *   (csrc/philox.h; the augmentation's blocks are 2^63 | 2^62 | j with j = 0 .. 3, the dropout sites leave bit 63 clear: no collision under
 *   one key).  A dropped sample gets num_classes (the id of the model's extra embedding row), a kept one its label.  drop_rate 0 drops
 *   nothing, 1 everything; 0 <= drop_rate <= 1 and num_classes > 0, KD_EINVAL otherwise.  The torch RNG stream of the reference is NOT
 *   reproduced. */
int kd_batch_u8_f32(const unsigned char* data, const long long* labels, const long long* idx, const long long* key, float drop_rate,
                    int num_classes, float* out, long long* class_out, int batch, int chan, int H, int W, void* stream);
int kd_class_dropout_i64(const long long* labels, const long long* key, float drop_rate, int num_classes, long long* out, int batch, void* stream);

/* Sample-quality metrics (k_diffusion/evaluation.py:93-161; csrc/metrics_f32.hip).  fp32-grade arithmetic: the Gram tiles follow the backward
 * pass's rule (split3 = 1: bf16 hi / lo operands, 3 MFMAs per product, fp32 accumulate; 0: fp32 FMAs).  Every sum has a fixed order (fp64
 * workspace, no atomics): repeat calls give the same bits.  Matrices are row-major fp32; batch items sx / sy elements apart.
 *   kd_mmd_poly_f32     : out[b] (+)= scale * squared_mmd(X[b], Y[b]) with k(x, y) = (x . y / d + 1)^3, X [m, d], Y [n, d] (fewer than 2
 *                         rows give the reference's nan / inf); the
 *                         kernel matrices are never written.  ws holds batch * (tm (tm + 1) / 2 + tn (tn + 1) / 2 + tm tn) doubles, tm / tn =
 *                         m / n rounded up to 64-row tiles.
 *   kd_poly_kernel_f32  : K[b] = (X[b] Y[b]^T / d + 1)^3, [m, n] per batch item.
 *   kd_mmd_mats_f32     : out[b] = squared_mmd from kernel matrices kxx [m, m], kyy [n, n], kxy [m, n] (diagonals of kxx, kyy dropped); ws
 *                         holds batch * 3 * ceil(max(m m, n n, m n) / 4096) doubles.
 *   kd_jacobi_sweep_f64 : one sweep of one-sided Jacobi on the rows of B [batch, n, n] (fp64; n - 1 rounds, n even, of n / 2 disjoint row
 *                         pairs, round robin; a pair whose |cos| exceeds tol is rotated to orthogonal, and so are the rows of Vt if given).
 *                         conv holds batch * ceil(n / 2) doubles; off[0] = the largest |cos| the sweep met.
 *   kd_sym_lower_f64    : B = the symmetric matrices of a's lower triangles (a fp32, or fp64 if a_f64) + diag_add I (fp64); Vt = I if not NULL.
 *   kd_row_sqrt_norm_f64: s[r] = sqrt(||B[r, :]||).
 *   kd_gemm_tn_f64      : C[b] = G[b]^T diag(row_scale[b]) A[b] (G [M, N], A [M, K], row_scale [M] or NULL) in fp64, to C64 or rounded to C32.
 *   kd_center_f32       : mean = colsum / rows, xc = x - mean in fp64 (mean may be NULL).
 *   kd_transpose_f64    : out[b] = a[b]^T, [batch, n, n].
 *   kd_sqrtm_vjp_div_f64: out[b, i, j] = m[b, i, j] / (s[b, i] + s[b, j]).
 *   kd_f32_to_f64       : out = (double)a.
 *   kd_fid_finish_f32   : out = |mean_x - mean_y|^2 + tr cov_x + tr cov_y - 2 sum sq (fp64 covariances and sums). */
int kd_mmd_poly_f32(const float* X, long long sx, long long m, const float* Y, long long sy, long long n, int d, int batch, int split3, double* ws,
                    float scale, int accumulate, float* out, void* stream);
int kd_poly_kernel_f32(const float* X, long long sx, long long m, const float* Y, long long sy, long long n, int d, int batch, int split3, float* K,
                       void* stream);
int kd_mmd_mats_f32(const float* kxx, const float* kyy, const float* kxy, long long m, long long n, int batch, double* ws, float* out, void* stream);
int kd_jacobi_sweep_f64(double* B, double* Vt, int batch, int n, double tol, double* conv, double* off, void* stream);
int kd_sym_lower_f64(const void* a, int a_f64, double* B, double* Vt, int batch, int n, double diag_add, void* stream);
int kd_row_sqrt_norm_f64(const double* B, long long rows, int n, double* s, void* stream);
int kd_gemm_tn_f64(const double* G, const double* A, const double* row_scale, int batch, int M, int N, int K, double* C64, float* C32, void* stream);
int kd_center_f32(const float* x, const float* colsum, long long rows, int d, double* xc, float* mean, void* stream);
int kd_transpose_f64(const double* a, double* out, int batch, int n, void* stream);
int kd_sqrtm_vjp_div_f64(const double* m, const double* s, int batch, int n, double* out, void* stream);
int kd_f32_to_f64(const float* a, double* out, long long n, void* stream);
int kd_fid_finish_f32(const float* mean_x, const float* mean_y, const double* cov_x, const double* cov_y, const double* sq, int d, float* out,
                      void* stream);

/* The training step behind the loss (train.py:444-473: accelerator.clip_grad_norm_(model.parameters(), 1.) :464, opt.step() :465 with
 * optim.AdamW :156-160, opt.zero_grad() :467, K.utils.ema_update :472 = k_diffusion/utils.py:88-104) and the sigma draw in front of it
 * (train.py:453-454 -> make_sample_density, k_diffusion/config.py:234-268 -> utils.py:267-276, :323-385); csrc/optim_f32.hip.
 * Multi-tensor kernels: ONE launch covers every tensor of `table`.  The caller keeps two device arrays and refreshes them (an asynchronous
 * copy on the launch's stream) only when a pointer changes:
 *   table   one KdMtTensor per parameter: p, g (gradient), m (exp_avg), v (exp_avg_sq), ema (the averaged model's copy, or NULL), n elements,
 *           group (index into the call's group array);
 *   chunks  2 ints per workgroup-sized piece: {tensor index, chunk index}; the piece is elements [chunk * KD_MT_CHUNK, min(n, (chunk + 1) *
 *           KD_MT_CHUNK)) of that tensor.  n_chunks pieces; the grid is capped and strides over the list.
 * fp32, contiguous.  16-byte accesses where all of a tensor's pointers are 16-byte aligned, element-wise otherwise.  No atomics: fixed summation
 * order, the same bits on every call.
 *   kd_mt_sqnorm_f32    : the L2 norm of all gradients in the table: squares and sums in fp64 (a product of two fp32 values is exact), one
 *                         partial per piece in ws [n_chunks doubles], then a one-workgroup launch that adds the partials in index order.
 *                         out[0] = (float)sqrt(sum), out[1] = min(1, max_norm / (out[0] + 1e-6)) in fp32: torch.nn.utils.clip_grad_norm_'s
 *                         coefficient (a NaN norm gives NaN, an infinite one 0, as there).
 *   kd_mt_adamw_ema_f32 : per element, with group constants lr, wd, beta1, beta2, eps, bc1 = 1 - beta1^step, bc2 = 1 - beta2^step (computed by
 *                         the host in fp64, rounded to fp32 where torch rounds them): g' = g * clip[1] (clip = the out pair above; NULL: 1);
 *                         p *= 1 - lr wd;  m = lerp(m, g', 1 - beta1);  v = v beta2 + (1 - beta2) g' g';  p -= (lr / bc1) m / (sqrt(v) /
 *                         sqrt(bc2) + eps): torch.optim.AdamW with amsgrad = False, maximize = False, rounded once per foreach operation as torch's device path
 *                         rounds (the multiply-add inside lerp / addcmul / addcdiv fused).  With use_ema and
 *                         a tensor's ema set: ema = lerp(ema, p_new, 1 - ema_decay) (torch.lerp's two-sided form).  zero_grad: g = 0 in place
 *                         (otherwise g is left as it was, unclipped).  Tensors whose group lies outside [0, n_groups) are skipped; more than
 *                         16 groups take one launch per 16.
 *   kd_mt_lerp_f32      : ema = lerp(ema, p, weight) for every tensor with ema set: K.utils.ema_update's parameter loop in one launch.
 *   kd_sigma_density_f32: out[e] = the density's transform of the uniform u[e] (KD_DENSITY_*; u and normal fp32, or fp64 with u_f64; out fp32, or
 *                         fp64 with out_f64; evaluated in fp64).  groups > 0 folds the stratification in: u <- (group + (e % row_len) groups + u)
 *                         / (row_len groups).  params (8 doubles on the HOST, read at the call):
 *                           LOGNORMAL {loc, scale}: exp(loc + scale icdf(u (1 - 2e-7) + 1e-7));  LOGLOGISTIC {loc, scale, min_cdf, max_cdf};
 *                           LOGUNIFORM {log min, log max};  V_DIFFUSION {sigma_data, min_cdf, max_cdf};  COSINE_INTERPOLATED {t_min, t_max,
 *                           shift of the noise_d_low schedule, the same three of the noise_d_high one, sigma_data};  SPLIT_LOGNORMAL {loc,
 *                           scale_1, scale_2, scale_1 / (scale_1 + scale_2)} with `normal` = standard normal draws. */
#define KD_MT_CHUNK 8192
typedef struct {
  float* p;
  float* g;
  float* m;
  float* v;
  float* ema;
  long long n;
  int group;
  int reserved;
} KdMtTensor;
typedef struct {
  double lr, wd, beta1, beta2, eps, bc1, bc2;
} KdAdamGroup;
enum { KD_DENSITY_LOGNORMAL = 0, KD_DENSITY_LOGLOGISTIC = 1, KD_DENSITY_LOGUNIFORM = 2, KD_DENSITY_V_DIFFUSION = 3,
       KD_DENSITY_COSINE_INTERPOLATED = 4, KD_DENSITY_SPLIT_LOGNORMAL = 5 };
int kd_mt_sqnorm_f32(const KdMtTensor* table, const int* chunks, int n_chunks, float max_norm, double* ws, float* out, void* stream);
int kd_mt_adamw_ema_f32(const KdMtTensor* table, const int* chunks, int n_chunks, const KdAdamGroup* groups, int n_groups, const float* clip,
                        double ema_decay, int use_ema, int zero_grad, void* stream);
int kd_mt_lerp_f32(const KdMtTensor* table, const int* chunks, int n_chunks, double weight, void* stream);
int kd_sigma_density_f32(int kind, const void* u, int u_f64, const void* normal, void* out, int out_f64, long long n, int row_len, int group,
                         int groups, const double* params, void* stream);

/* ---- image_v1 U-Net (k_diffusion/models/image_v1.py), forward and dual (forward-mode JVP) pass (csrc/conv_x3.hip, csrc/unet_f32.hip) ----
 * Activations are fp32 NHWC, token-major [batch * H * W, C]; every `ld*` is a row stride in floats (>= the row's channels, a multiple of 4),
 * so an operand may be one column range of a wider buffer (the halves of a skip concatenation).  Rows are 16-byte aligned.  The kernels read
 * no library option, use no atomics, and give the same bits on every run.
 *
 * kd_pack_conv_x3     w [c_out, c_in, ks, ks] fp32 (nn.Conv2d's layout) -> `out`, 4 * ks * ks * c_out * c_in bytes: a hi image then a lo image,
 *                     each [ks * ks taps][c_out][c_in] bf16 with hi = bf16(w), lo = bf16(w - hi).
 * kd_conv2d_x3        y = conv2d(x, w, padding = ks / 2) + bias + res for ks = 1 or 3, stride 1, in the split-bf16x3 arithmetic (three bf16 MFMAs
 *                     per product, fp32 accumulation).  c_in and c_out are multiples of 64.  bias [c_out] and res (row stride ldr) may be NULL.
 *                     y must not overlap x (a workgroup reads the halo of pixels other workgroups write); y may be res.
 * kd_groupnorm_stats_f32   stats [batch, groups, 4] = {mean_hi, mean_lo, rstd, 0} per (sample, group) over (chan / groups channels x hw pixels):
 *                     mean_hi + mean_lo is the fp64 mean, rstd = 1 / sqrt(biased variance + eps) (F.group_norm), sums in fp64.
 * kd_adagn_apply_f32  y = (x - mean) * rstd * (1 + w_b) + b_b with w_b = wb[b * wb_stride + c], b_b = wb[b * wb_stride + chan + c] (the two
 *                     chunks of AdaGN's mapper output), then the exact (erf) GELU if `gelu`.  y may be x.
 * kd_conv2d_x3_stacked   kd_conv2d_x3 on a batch whose samples b >= bias_batch get no bias (0 <= bias_batch <= batch): the dual pass stacks
 *                     the tangent behind the primal as samples batch / 2 .. batch - 1, and the tangent of conv(x) + bias has no bias.  Same
 *                     kernel and accumulation order: a sample's output has the bits kd_conv2d_x3 gives it with or without the bias.
 * kd_groupnorm_stats_jvp_f32   stats as kd_groupnorm_stats_f32 writes them (same bits) and jstats [batch, groups, 4] = {mean_dot, rstd_dot, 0,
 *                     0}, their tangents along x_dot (row stride ldxd): mean_dot = sum x_dot / n, rstd_dot = -rstd^3 sum (x - mean) x_dot / n, x
 *                     centred with the fp64 mean, sums in fp64 in a fixed order.  Groups of a multiple of 4 channels.
 * kd_adagn_apply_jvp_f32   y as kd_adagn_apply_f32 (same bits) and its tangent with the conditioning held fixed: xh_dot = (x_dot - mean_dot) *
 *                     rstd + (x - mean) * rstd_dot, pre_dot = xh_dot * (1 + w_b), y_dot = pre_dot, or with `gelu` pre_dot * (Phi(pre) + pre *
 *                     phi(pre)) (exact erf form).  y may be x together with y_dot being x_dot.
 * kd_down2_f32 / kd_up2_f32   Downsample2d / Upsample2d with the 'linear' kernel and 'reflect' padding: [H, W] -> [H / 2, W / 2] (H, W even) and
 *                     [H, W] -> [2 H, 2 W]; H, W >= 2.  y must not overlap x.
 * kd_unet_in_f32      y[pixel][n] = bias[n] + sum_k w[n][k] * img[b][k][pixel] * c_in(b) for an NCHW image of c_img channels; c_in(b) =
 *                     1 / sqrt(sigma_b^2 + sigma_data^2), or 1 when sigma is NULL.
 * kd_unet_out_f32     F[b][o][pixel] = bias[o] + sum_n w[o][n] * x[pixel][n] for c_img <= 4 image channels, written NCHW; with sigma:
 *                     out = F * c_out(b) + img * c_skip(b) (the Karras preconditioning, k_diffusion/layers.py:88-90).
 * kd_cond_mlp_f32     y [rows, n_out] = act(x [rows, k_in] w[n_out, k_in]^T + bias + add) in fp32 FMAs, act = exact GELU if `gelu`; bias [n_out]
 *                     and add [rows, n_out] may be NULL.  Meant for a few rows (the conditioning vectors of a batch). */
int kd_pack_conv_x3(const float* w, void* out, int c_out, int c_in, int ks, void* stream);
int kd_conv2d_x3(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy, int batch, int H, int W,
                 int c_in, int c_out, int ks, void* stream);
int kd_conv2d_x3_stacked(const float* x, int ldx, const void* wp, const float* bias, const float* res, int ldr, float* y, int ldy, int batch, int H,
                         int W, int c_in, int c_out, int ks, int bias_batch, void* stream);
int kd_groupnorm_stats_f32(const float* x, int ldx, float* stats, int batch, int hw, int chan, int groups, float eps, void* stream);
int kd_groupnorm_stats_jvp_f32(const float* x, int ldx, const float* x_dot, int ldxd, float* stats, float* jstats, int batch, int hw, int chan,
                               int groups, float eps, void* stream);
int kd_adagn_apply_f32(const float* x, int ldx, const float* stats, const float* wb, int wb_stride, float* y, int ldy, int batch, int hw, int chan,
                       int groups, int gelu, void* stream);
int kd_adagn_apply_jvp_f32(const float* x, int ldx, const float* x_dot, int ldxd, const float* stats, const float* jstats, const float* wb,
                           int wb_stride, float* y, int ldy, float* y_dot, int ldyd, int batch, int hw, int chan, int groups, int gelu, void* stream);
int kd_down2_f32(const float* x, int ldx, float* y, int ldy, int batch, int H, int W, int chan, void* stream);
int kd_up2_f32(const float* x, int ldx, float* y, int ldy, int batch, int H, int W, int chan, void* stream);
int kd_unet_in_f32(const float* img, const float* w, const float* bias, const float* sigma, float sigma_data, float* y, int ldy, int batch, int hw,
                   int c_img, int chan, void* stream);
int kd_unet_out_f32(const float* x, int ldx, const float* w, const float* bias, const float* img, const float* sigma, float sigma_data, float* out,
                    int batch, int hw, int c_img, int chan, void* stream);
int kd_cond_mlp_f32(const float* x, const float* w, const float* bias, const float* add, float* y, int rows, int n_out, int k_in, int gelu,
                    void* stream);

/* Final image conversion (k_diffusion/utils.py:27-34 to_pil_image): u8 = trunc((clamp(x,-1,1)+1)/2*255)
 * (torchvision's to_pil_image does mul(255).byte(), i.e. truncation) */
int kd_to_uint8(const float* x, unsigned char* y, long long n, void* stream);

/* Per-launch timing hooks for bench.py (HIP events recorded on `stream` around each launch).  A record's name is the kernel (with its
 * template switches), the shape, and -- where the launcher chooses between configurations (n-splits, tile form, wave count, slices) -- one
 * field " cfg=..." stating what it launched, e.g. "gemm_x3_astat<e5> M=1000 N=384 K=128 cfg=splits3"; at most 95 characters. */
int kd_prof_enable(int on);
int kd_prof_count(void);
int kd_prof_get(int i, char* name, int name_cap, float* ms, double* flops, double* bytes);
int kd_prof_reset(void);
/* In-kernel time line probe (benchmarks/): while `dev_ptr` (16 x uint64 of device memory) is set, workgroup 0 of the bf16 GEMM kernels
 * (W-stationary, A-stationary, tiled) and of kd_ffn_bf16 writes s_memtime stamps: [0] entry, [2] exit, [1] / [3] s_memrealtime at
 * entry / exit (shader clock under load = ([2]-[0]) / ([3]-[1]) x 100 MHz), [4] end of the row prologue / first blocks in,
 * [5] end of the first tile's K loop (tiled, ffn: of the whole loop), [6] end of its epilogue, [7] number of ring blocks / tiles.
 * kd_ffn_f32 also stamps its third d_ff tile: [8] start, [9] up projection done, [10] GEGLU done, [11] down k-steps done, and [12]
 * the end of the tile loop.  NULL switches it off.  Not for concurrent launches.
 * Extended form (round 4; the fp32-parity kernels of gemm_x3.hip, gemm_x3r.hip, ffn_x3.hip, attn_x3.hip): when entry [15] holds 0x4b44 the buffer
 * must provide 32 + 3 * grid entries, and EVERY workgroup's first thread writes s_memrealtime (100 MHz ticks) at its entry to [32 + 3 b] and at
 * its exit to [32 + 3 b + 1] (b = blockIdx.x; [.. + 2]: exit of the workgroup's first loader wave where there is one): launch ramp, rounds,
 * tail and the spread of the workgroups' lifetimes (benchmarks/wg_timeline.py, benchmarks/x3r_bench.py). */
int kd_prof_clock_buffer(void* dev_ptr);

/* A forward's launch list in ONE host call (round 4).  The Python mirror used to issue the 58 - 66 launches of a model call one ctypes call
 * at a time; kd_run_list walks an array of calls and invokes the entry point each one names with the arguments it carries, in order, on
 * `stream`; it stops at the first failure, returns that entry point's code and stores the index in *failed (if not NULL).  A KdCall carries
 * the arguments of the entry point KD_OP_X names (kd_x) by one rule: its pointer arguments in declaration order in p[], its int arguments in
 * declaration order in i[], its one float (eps) in f; the trailing stream is the list's.  Descriptors (KdGemm, KdFfn) go in by ADDRESS like any
 * other pointer and are read at the call, so a caller may keep patching them between runs. */
enum { KD_OP_GEMM_F32 = 0, KD_OP_GEMM_BF16 = 1, KD_OP_FFN_F32 = 2, KD_OP_FFN_BF16 = 3,
       KD_OP_ATTN_GLOBAL_F32 = 4, KD_OP_ATTN_WINDOW_F32 = 5, KD_OP_ATTN_NA2D_F32 = 6,
       KD_OP_ATTN_GLOBAL_BF16 = 7, KD_OP_ATTN_WINDOW_BF16 = 8, KD_OP_ATTN_NA2D_BF16 = 9, KD_OP_NORM_SPLIT_F32 = 10,
       KD_OP_ATTN_BLOCK_BF16 = 11, KD_OP_PROJ_BLOCK_BF16 = 12, KD_OP_GEMM_MX8 = 13, KD_OP_ATTN_FFN_F32 = 14 };
typedef struct {
  int op;             /* KD_OP_* */
  float f;
  const void* p[5];
  int i[8];
} KdCall;
int kd_run_list(const KdCall* calls, int n, void* stream, int* failed);

#ifdef __cplusplus
}
#endif
#endif
