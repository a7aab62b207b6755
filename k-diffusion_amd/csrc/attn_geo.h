// The geometry of the three attention forms, written once: which keys a query attends and where a kernel finds them.  Plain integer
// code that compiles as ordinary C++17 on the host as well (tests/attn_geo_check.cpp holds it to oracle/hdit.py without a GPU); the
// kernels of attn_bf16.hip, attn_x3_core.h / attn_x3.hip / attn_ffn_x3.hip, attn_f32.hip and jvp_f32.hip / vjp_f32.hip take every
// index from here and keep only their own data movement (swizzles, fragment addresses, staging loops).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KD_GEO __host__ __device__ __forceinline__
#else
#define KD_GEO inline
#endif
#include "../../include/kdiff_hip.h"

namespace kd {
int fail(int code, const char* fmt, ...);      // common.cpp: records the reason (kd_last_error) and returns the code

namespace geo {

KD_GEO int imin(int a, int b) { return a < b ? a : b; }
KD_GEO int imax(int a, int b) { return a > b ? a : b; }

// ---- neighbourhood attention, one axis ----------------------------------------------------------------------------------------------------
// NATTEN semantics, dilation 1 (natten na2d, image_transformer_v2.py:428; oracle/hdit.py: na2d_window_start): query i of an axis of `len`
// tokens attends the `ks` keys from start(i) = clamp(i - ks/2, 0, len - ks), len >= ks.  `na_origin` is the same rule for any span, a
// tile's key halo included: clamped to 0 LAST, so that an axis shorter than the span starts at 0; na_origin(i, len, ks, ks) == na_start.
// (Two orders of the two clamps because hipcc keeps the order it is given: the tile kernels were written in the second, the derivative
// kernels in the first, and either family gets another instruction stream on the other's.  tests/attn_geo_check.cpp holds both to the rule.)
KD_GEO int na_start(int i, int len, int ks) { return imin(imax(i - ks / 2, 0), len - ks); }
KD_GEO int na_origin(int i, int len, int ks, int span) { return imax(0, imin(i - ks / 2, len - span)); }

// ---- neighbourhood tile -------------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per (sample, head, 8 x 16 query tile).  Wave w owns the 4 x 8 query block at rows 4 (w >> 1), columns
// 8 (w & 1) of the tile; lane l of either half-wave (l31 = lane & 31, h2 = lane >> 5) owns query (l31 >> 3, l31 & 7) of the block.
constexpr int NA_TH = 8, NA_TW = 16;
KD_GEO int na_tiles_y(int H) { return (H + NA_TH - 1) / NA_TH; }
KD_GEO int na_tiles_x(int W) { return (W + NA_TW - 1) / NA_TW; }
KD_GEO long na_tiles(int batch, int nh, int H, int W) { return (long)batch * nh * na_tiles_y(H) * na_tiles_x(W); }      // the launchers' grid

// The per-workgroup and per-lane blocks are MACROS that declare their results as locals of the kernel, each expanded where the kernel
// needs the values (tile and halo first, the query in front of the q loads, the patch behind them).  As __forceinline__ functions
// returning structs the same expressions reach hipcc in another order and every neighbourhood kernel gets another schedule and other
// register counts (profiles/attn_geometry_refactor.md); na_lane() below is the same text as one function, for code that is not a kernel.
// ``a`` carries H, W, nh and is read where a value is used.
//
// KD_NA_TILE: workgroup index R (XCD-chunked where neighbouring tiles should share an L2: the caller's choice; evaluated behind the tile
// counts) -> tx, ty, head, b, x fastest.
#define KD_NA_TILE(a, R) \
  const int tiles_x = kd::geo::na_tiles_x((a).W), tiles_y = kd::geo::na_tiles_y((a).H); \
  int r = (R); \
  const int tx = r % tiles_x; r /= tiles_x; \
  const int ty = r % tiles_y; r /= tiles_y; \
  const int head = r % (a).nh, b = r / (a).nh;

// The key halo of a tile, HR x HC = (8 + KS - 1) x (16 + KS - 1) keys from (hy0, hx0), goes to LDS as image rows: image row y HC + x is
// halo position (y, x), token (min(hy0 + y, H - 1), min(hx0 + x, W - 1)).  Positions clamped that way (images smaller than the halo) and
// image rows past the halo's last key hold a real token and lie outside every window.
// KD_NA_HALO -> ty0, tx0 (the tile's first query), hy0, hx0.
KD_GEO int na_halo_origin(int t0, int len, int ks, int halo) { return na_origin(t0, len, ks, halo); }
#define KD_NA_HALO(G, a, ty, tx) \
  const int ty0 = (ty) * kd::geo::NA_TH, tx0 = (tx) * kd::geo::NA_TW; \
  const int hy0 = kd::geo::na_halo_origin(ty0, (a).H, G::KS, G::HR), hx0 = kd::geo::na_halo_origin(tx0, (a).W, G::KS, G::HC);

// KD_NA_QUERY: wave block (wy_, wx_) = (wid >> 1, wid & 1), lane l31 -> q_ok, qy, qx, q_tok.  Overhanging lanes of a ragged tile (q_ok
// false) shadow a real query and never store.
#define KD_NA_QUERY(a, ty0, tx0, wy_, wx_, l31) \
  const int qy_raw = (ty0) + 4 * (wy_) + ((l31) >> 3), qx_raw = (tx0) + 8 * (wx_) + ((l31) & 7); \
  const bool q_ok = qy_raw < (a).H && qx_raw < (a).W; \
  const int qy = kd::geo::imin(qy_raw, (a).H - 1), qx = kd::geo::imin(qx_raw, (a).W - 1); \
  const int q_tok = qy * (a).W + qx;

// KD_NA_PATCH.  The clamped windows of a wave's 32 queries lie inside a patch of PR = 4 + KS - 1 rows x (8 + KS - 1) columns of the halo
// from (row_lo, col_lo): the window start of the block's first query, pulled in at the bottom / right border where the halo is.
// -> wy, wx (the lane's window start relative to the halo), row_lo, col_lo, korg (image row of patch key (0, 0)) and (r0, c0), the lane's
// window start inside the patch.
#define KD_NA_PATCH(G, a, ty0, tx0, hy0, hx0, wy_, wx_, qy, qx) \
  const int wy = kd::geo::na_origin(qy, (a).H, G::KS, G::KS) - (hy0), wx = kd::geo::na_origin(qx, (a).W, G::KS, G::KS) - (hx0); \
  const int row_lo = kd::geo::imin(kd::geo::na_origin(kd::geo::imin((ty0) + 4 * (wy_), (a).H - 1), (a).H, G::KS, G::KS) - (hy0), G::HR - G::PR); \
  const int col_lo = kd::geo::imin(kd::geo::na_origin(kd::geo::imin((tx0) + 8 * (wx_), (a).W - 1), (a).W, G::KS, G::KS) - (hx0), G::HC - (8 + G::KS - 1)); \
  const int korg = row_lo * G::HC + col_lo; \
  const int r0 = wy - row_lo, c0 = wx - col_lo;

struct NaLane {
  int tx, ty, head, b, hy0, hx0;
  bool q_ok;
  int qy, qx, q_tok, korg, r0, c0;
};
template <class G, class A>
KD_GEO NaLane na_lane(const A& a, int wg, int wid, int l31) {
  const int wy_ = wid >> 1, wx_ = wid & 1;
  KD_NA_TILE(a, wg)
  KD_NA_HALO(G, a, ty, tx)
  KD_NA_QUERY(a, ty0, tx0, wy_, wx_, l31)
  KD_NA_PATCH(G, a, ty0, tx0, hy0, hx0, wy_, wx_, qy, qx)
  return NaLane{tx, ty, head, b, hy0, hx0, q_ok, qy, qx, q_tok, korg, r0, c0};
}

// The patch walk.  Accumulator register i of a 32-key score tile holds, in lane-half h2, the tile's key na_acc_key(i, h2).
#define KD_NA_ACC_KEY(i, h2) (((i) & 3) + 8 * ((i) >> 2) + 4 * (h2))
KD_GEO int na_acc_key(int i, int h2) { return KD_NA_ACC_KEY(i, h2); }
// Tuned form (KS <= 9): 16 keys per patch row, local key 16 r + c = image row korg + HC r + c; tile t is patch rows 2 t, 2 t + 1.  The K
// fragment of lane l31 is the row of local key 32 t + l31; the V^T read of k-step (t, u) addresses patch row 2 t + u, columns
// 4 h2 + vrow, vrow = (lane & 15) >> 2, and the same + 8.
#define KD_NA_K_ROW0(G, korg, l31) ((korg) + ((l31) >> 4) * G::HC + ((l31) & 15))      // (the function below, in a kernel: another stream at KS = 5, 9)
template <class G> KD_GEO int na_k_row0(int korg, int l31) { return KD_NA_K_ROW0(G, korg, l31); }
template <class G> KD_GEO int na_k_row(int kr0, int t) { return kr0 + 2 * t * G::HC; }
KD_GEO int na_v_row0(int korg, int h2, int vrow) { return korg + 4 * h2 + vrow; }
template <class G> KD_GEO int na_v_row(int vr0, int t, int u) { return vr0 + (2 * t + u) * G::HC; }
// validity of patch column / patch row for ONE query as +inf (inside the window) / -inf words: one v_min3 per score applies both.
// Column word j = (i & 7) of any tile's register i (column (i & 3) + 8 ((i >> 2) & 1) + 4 h2), row word p = 2 t + (i >> 3).
#define KD_NA_COL_OK(KS, j, h2, c0) ((unsigned)(KD_NA_ACC_KEY(j, h2) - (c0)) < (unsigned)(KS))
#define KD_NA_ROW_OK(KS, p, r0) ((unsigned)((p) - (r0)) < (unsigned)(KS))
#define KD_NA_VALID_WORDS(KS, NROW, r0, c0, h2, colv, rowv) \
  { \
_Pragma("unroll") \
    for (int j = 0; j < 8; ++j) (colv)[j] = KD_NA_COL_OK(KS, j, h2, c0) ? __builtin_inff() : -__builtin_inff(); \
_Pragma("unroll") \
    for (int p = 0; p < (NROW); ++p) (rowv)[p] = KD_NA_ROW_OK(KS, p, r0) ? __builtin_inff() : -__builtin_inff(); \
  }
// Wide form (KS = 11, 13: 18 / 20 patch columns): the patch is walked densely, local key kl = PC r + c with PC = 20 (a multiple of 4: the
// 4-key groups of the V^T reads never straddle two patch rows), every key's (row, column) by constant division.
#define KD_NA_WIDE_ROW(G, korg, kl) ((korg) + ((kl) / G::PC) * G::HC + ((kl) % G::PC))
#define KD_NA_WIDE_VALID(G, kl, r0, c0) \
  ((unsigned)((kl) / G::PC - (r0)) < (unsigned)G::KS && (unsigned)((kl) % G::PC - (c0)) < (unsigned)G::KS && (kl) / G::PC < G::PR)
template <class G> KD_GEO int na_wide_row(int korg, int kl) { return KD_NA_WIDE_ROW(G, korg, kl); }
template <class G> KD_GEO bool na_wide_valid(int kl, int r0, int c0) { return KD_NA_WIDE_VALID(G, kl, r0, c0); }

// Image sizes.  ROW_GRAN: image rows per LDS-DMA instruction (1024 bytes / ROW_BYTES); IMAGES: 1 if K and V share the image, else 2.
// Tuned form: a patch may poke past the halo's last key.  The highest row a fragment read touches is that of the last patch
// (korg = (HR - PR) HC + HC - (8 + KS - 1)), last tile, for K lane 31 (row + HC + 15 + (PR - 2) HC), for V^T the + 8 rows of u = 1
// (row + 4 + 3 + 8 + (PR - 1) HC): (HR - 1) HC + (HC - (8 + KS - 1)) + 15 = HR HC - KS + 8 either way (PR is even: 2 NKT = PR).
template <int KS_, int ROW_GRAN, int ROW_BYTES, int IMAGES>
struct NaGeo {
  static constexpr int KS = KS_;
  static constexpr int HR = NA_TH + KS - 1, HC = NA_TW + KS - 1;      // key halo of an 8 x 16 query tile (KS = 7: 14 x 22)
  static constexpr int PR = 4 + KS - 1, PW = 16;                      // patch rows of a wave, keys per patch row
  static constexpr int NKT = (PR * PW + 31) / 32;                     // key tiles of 32 per wave (KS = 7: 5)
  static constexpr int ROWS = ((HR * HC - KS + 9 + ROW_GRAN - 1) / ROW_GRAN) * ROW_GRAN;
  static constexpr int LDS = IMAGES * ROWS * ROW_BYTES;
  static_assert(8 + KS - 1 <= PW, "16-key patch rows: kernel sizes up to 9");
};
// Wide form: slack of two padded patch rows for the padded columns and the last tile's tail (reads past it are clamped to ROWS - 1 by
// the kernels; no admitted key lies there).
template <int KS_, int ROW_GRAN, int ROW_BYTES, int IMAGES>
struct NaWide {
  static constexpr int KS = KS_;
  static constexpr int HR = NA_TH + KS - 1, HC = NA_TW + KS - 1;
  static constexpr int PR = 4 + KS - 1, PC = 20;                      // patch rows; padded patch width
  static constexpr int NKT = (PR * PC + 31) / 32;
  static constexpr int ROWS = ((HR * HC + 2 * PC + ROW_GRAN - 1) / ROW_GRAN) * ROW_GRAN;
  static constexpr int LDS = IMAGES * ROWS * ROW_BYTES;
  static_assert(8 + KS - 1 <= PC, "patch width");
};
// the instantiated forms: bf16 rows of 128 bytes, 8 per instruction, one image (K, then V) tuned, two wide; split3 rows of 256 bytes
// ([hi4 | lo4] chunks), 4 per instruction, one image in both
template <int KS> using NaGeoB16 = NaGeo<KS, 8, 128, 1>;
template <int KS> using NaWideB16 = NaWide<KS, 8, 128, 2>;
template <int KS> using NaGeoX3 = NaGeo<KS, 4, 256, 1>;
template <int KS> using NaWideX3 = NaWide<KS, 4, 256, 1>;

// ---- shifted window -----------------------------------------------------------------------------------------------------------------------
// The reference rolls the grid by (shift, shift), cuts it into ws x ws windows and masks pairs of different wrapped regions
// (image_transformer_v2.py:253-337): rolled[i] = orig[(i - shift) mod len] (:274), so slot (a, b) of window (wi, wj) is token
// (unroll(wi ws + a), unroll(wj ws + b)); 0 <= shift < ws <= len, so one conditional add is the modulo.  Region id
// (make_shifted_window_masks, :285-316): rows a < shift of the TOP window row and columns b < shift of the LEFT window column are the
// wrapped-around parts; a pair is allowed iff both slots have the same id.  ``g`` is the kernel's argument struct (H, W, shift), read
// where the values are used: as plain int parameters the loads stand in front of the sum and hipcc associates it the other way.
template <class A>
KD_GEO int win_token(const A& g, int ws, int wi, int wj, int a, int b) {
  int i = wi * ws + a - g.shift; if (i < 0) i += g.H;
  int j = wj * ws + b - g.shift; if (j < 0) j += g.W;
  return i * g.W + j;
}
KD_GEO int win_region(int shift, int wi, int wj, int a, int b) { return ((wi == 0 && a < shift) ? 2 : 0) + ((wj == 0 && b < shift) ? 1 : 0); }

// the dense cores carry log2(window_size) in a template value: 8 x 8 (the shipped config), 4 x 4, 16 x 16 windows; slot = a ws + b
enum { MODE_GLOBAL = 0, MODE_WINDOW = 1, MODE_WINDOW4 = 2, MODE_WINDOW16 = 3 };
template <int MODE> struct WinLog2 { static constexpr int v = MODE == MODE_WINDOW ? 3 : (MODE == MODE_WINDOW4 ? 2 : 4); };
// slot -> token index inside the sample; global mode: the slot itself (bounds and pad slots are the caller's)
template <int MODE, class A>
KD_GEO int slot_token(const A& g, int slot, int wi, int wj) {
  if (MODE == MODE_GLOBAL) return slot;
  constexpr int L = WinLog2<MODE>::v, WS = 1 << L;
  return win_token(g, WS, wi, wj, slot >> L, slot & (WS - 1));
}
template <int MODE>
KD_GEO int slot_region(int shift, int slot, int wi, int wj) {
  constexpr int L = WinLog2<MODE>::v, WS = 1 << L;
  return win_region(shift, wi, wj, slot >> L, slot & (WS - 1));
}

// ---- key sets of the derivative kernels (jvp_f32.hip, vjp_f32.hip) ---------------------------------------------------------------------------
// The keys a block of 16 queries of one (sample, head) attends (qb: the block within the head, g: the query within the block).
// All T tokens (global), the window (shifted window; the reference's region mask is a per-pair predicate), or the union of the queries'
// clamped neighbourhoods for a 4x4 query tile (neighbourhood; the predicate keeps each query's own ks x ks window).  The window's pair
// predicate is symmetric, so the same set, read from the key's side, is the set of queries that attend a key.  ``A`` carries T, H, W,
// geo (window size / kernel size) and shift.
// The window branch keeps the text it was written in (a true modulo for the roll, the region id as two flags): on win_token / win_region
// its three kernels change registers and length (profiles/attn_geometry_refactor.md).  tests/attn_geo_check.cpp holds it to both.
enum { KS_GLOBAL = 0, KS_WINDOW = 1, KS_NA = 2 };
KD_GEO int wrap(int i, int n) { return ((i % n) + n) % n; }

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
  KD_GEO void init(const A& a, int qb, int g) {
    if (MODE == KS_GLOBAL) {
      const int t = qb * 16 + g;
      qactive = t < a.T;
      qtok = imin(t, a.T - 1);
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
      const int qr_c = imin(qr, a.H - 1), qc_c = imin(qc, a.W - 1);
      qtok = qr_c * a.W + qc_c;
      q_a = na_start(qr_c, a.H, ks);
      q_b = na_start(qc_c, a.W, ks);
      base_r = na_start(r0, a.H, ks);
      base_c = na_start(c0, a.W, ks);
      const int r_hi = na_start(imin(r0 + 3, a.H - 1), a.H, ks) + ks, c_hi = na_start(imin(c0 + 3, a.W - 1), a.W, ks) + ks;
      span_c = c_hi - base_c;
      n_keys = (r_hi - base_r) * span_c;
    }
  }
  template <class A>
  KD_GEO int key_tok(const A& a, int j) const {
    if (MODE == KS_GLOBAL) return j;
    if (MODE == KS_WINDOW) {
      const int ws = a.geo, ka = j / ws, kc = j % ws;
      return wrap(base_r + ka - a.shift, a.H) * a.W + wrap(base_c + kc - a.shift, a.W);
    }
    return (base_r + j / span_c) * a.W + base_c + j % span_c;
  }
  template <class A>
  KD_GEO bool allowed(const A& a, int j) const {
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

// ---- host: what the entry points refuse -----------------------------------------------------------------------------------------------------
// KD_OK, or KD_EINVAL with the entry point's name `who` in front of the reason (kd_last_error)
inline int na_check(const char* who, int ks, int H, int W) {
  if (ks < 3 || ks > 13 || !(ks & 1)) return fail(KD_EINVAL, "%s: kernel_size %d unsupported (odd sizes 3 .. 13)", who, ks);
  if (H < ks || W < ks) return fail(KD_EINVAL, "%s: grid %dx%d smaller than the %dx%d neighbourhood", who, H, W, ks, ks);
  return KD_OK;
}
inline int window_check(const char* who, int H, int W, int ws, int shift) {
  if (ws != 4 && ws != 8 && ws != 16) return fail(KD_EINVAL, "%s: window_size %d unsupported (4, 8 or 16)", who, ws);
  if ((H % ws) || (W % ws)) return fail(KD_EINVAL, "%s: grid %dx%d not divisible by the window", who, H, W);
  if (shift < 0 || shift >= ws) return fail(KD_EINVAL, "%s: bad shift %d", who, shift);
  return KD_OK;
}

}  // namespace geo
}  // namespace kd
