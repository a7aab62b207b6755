// k-diffusion_amd/csrc/attn_geo.h on the host, without a GPU: a program of its own (tests/test_attn_geo_cpu.py builds it with the address and
// undefined-behaviour sanitizers and runs it directly).  It walks what the attention kernels walk -- tiles, waves, lanes, patches, validity
// words, image rows, window slots, key sets -- through the header's own macros and functions, and checks every query's key set against the
// published rules written out here a second time, the plain way.  Lines it prints in front of the final "ok" are compared with oracle/hdit.py
// by the pytest.
#include "../k-diffusion_amd/csrc/attn_geo.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

static std::string g_last_error;
namespace kd {
int fail(int code, const char* fmt, ...) {      // common.cpp's, recording
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
}  // namespace kd

using namespace kd::geo;

static long g_checks = 0;
#define CHECK(cond, ...) \
  do { \
    ++g_checks; \
    if (!(cond)) { \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__); \
      std::printf("\n"); \
      std::exit(1); \
    } \
  } while (0)

// the rule, the plain way (NATTEN, dilation 1): clamp(i - ks/2, 0, len - ks)
static int rule_start(int i, int len, int ks) {
  int s = i - ks / 2;
  if (s < 0) s = 0;
  if (s > len - ks) s = len - ks;
  return s;
}
static std::vector<int> rule_window(int qy, int qx, int H, int W, int ks) {
  std::vector<int> v;
  const int sy = rule_start(qy, H, ks), sx = rule_start(qx, W, ks);
  for (int y = sy; y < sy + ks; ++y)
    for (int x = sx; x < sx + ks; ++x) v.push_back(y * W + x);
  return v;      // sorted
}

struct Args { int T, H, W, nh, geo, shift; };      // what a kernel's argument struct carries

// grid sizes of one axis: L = ks; one below the halo, the halo, one above; one tile, one tile + 1, two tiles and a ragged remainder
static std::vector<int> axis_sizes(int ks, int halo, int tile, int ragged) {
  std::vector<int> v;
  for (int L : {ks, halo - 1, halo, halo + 1, tile, tile + 1, 2 * tile + ragged})
    if (L >= ks && std::find(v.begin(), v.end(), L) == v.end()) v.push_back(L);
  return v;
}
// every size of either axis, each with two sizes of the other one (the full product says no more and takes five times as long)
static std::vector<std::pair<int, int>> grids(int ks) {
  const std::vector<int> hs = axis_sizes(ks, NA_TH + ks - 1, NA_TH, 3), ws = axis_sizes(ks, NA_TW + ks - 1, NA_TW, 5);
  std::vector<std::pair<int, int>> v;
  const size_t n = std::max(hs.size(), ws.size());
  for (size_t i = 0; i < n; ++i)
    for (size_t d = 0; d < 2; ++d) v.emplace_back(hs[i % hs.size()], ws[(i + 2 * d) % ws.size()]);
  return v;
}

// ---- neighbourhood: one image form G (tuned: NaGeo<...>, 16-key patch rows and validity words; wide: NaWide<...>, dense patch and predicate) ----
template <class G, bool WIDE>
static void check_na_form(const char* name) {
  constexpr int KS = G::KS, HC = G::HC, NKT = G::NKT, ROWS = G::ROWS;
  int max_row = -1;
  for (const auto& hw : grids(KS)) {
      const int H = hw.first, W = hw.second;
      const Args a{H * W, H, W, 2, KS, 0};
      const int batch = H == KS ? 2 : 1;
      const long n_wg = na_tiles(batch, a.nh, H, W);
      CHECK(n_wg == (long)batch * a.nh * na_tiles_y(H) * na_tiles_x(W), "%s %dx%d", name, H, W);
      std::vector<int> owners((size_t)batch * a.nh * H * W, 0);
      for (int wg = 0; wg < (int)n_wg; ++wg)
        for (int wid = 0; wid < 4; ++wid)
          for (int l31 = 0; l31 < 32; ++l31) {
            const NaLane n = na_lane<G>(a, wg, wid, l31);
            CHECK(n.b >= 0 && n.b < batch && n.head >= 0 && n.head < a.nh && n.ty >= 0 && n.ty < na_tiles_y(H) && n.tx >= 0 && n.tx < na_tiles_x(W),
                  "%s %dx%d wg %d", name, H, W, wg);
            CHECK(((n.b * a.nh + n.head) * na_tiles_y(H) + n.ty) * na_tiles_x(W) + n.tx == wg, "%s %dx%d: tile decode of %d", name, H, W, wg);
            CHECK(n.q_tok == n.qy * W + n.qx && n.qy >= 0 && n.qy < H && n.qx >= 0 && n.qx < W, "%s %dx%d", name, H, W);
            CHECK(n.hy0 >= 0 && n.hx0 >= 0 && n.korg >= 0, "%s %dx%d: hy0 %d hx0 %d korg %d", name, H, W, n.hy0, n.hx0, n.korg);
            if (n.q_ok) ++owners[(size_t)(n.b * a.nh + n.head) * H * W + n.q_tok];
            // image row -> token as the staging loops load it; rows of admitted keys must be true halo positions inside the image
            std::vector<int> got;
            auto admit = [&](int row) {
              const int y = row / HC, x = row % HC;
              CHECK(row >= 0 && row < G::HR * HC && n.hy0 + y < H && n.hx0 + x < W, "%s %dx%d wg %d wave %d lane %d: admitted image row %d is no key", name, H,
                    W, wg, wid, l31, row);
              got.push_back(imin(n.hy0 + y, H - 1) * W + imin(n.hx0 + x, W - 1));
            };
            for (int h2 = 0; h2 < 2; ++h2) {
              float colv[8] = {}, rowv[2 * NKT] = {};
              if constexpr (!WIDE) KD_NA_VALID_WORDS(KS, 2 * NKT, n.r0, n.c0, h2, colv, rowv)
              for (int t = 0; t < NKT; ++t)
                for (int i = 0; i < 16; ++i) {
                  const int key = na_acc_key(i, h2);      // of the tile: the K fragment row that lane `key` supplies
                  if constexpr (WIDE) {
                    const int row = na_wide_row<G>(n.korg, 32 * t + key);
                    CHECK(na_wide_valid<G>(32 * t + key, n.r0, n.c0) == (bool)(KD_NA_WIDE_VALID(G, 32 * t + key, n.r0, n.c0)), "wide predicate forms");
                    CHECK(row == KD_NA_WIDE_ROW(G, n.korg, 32 * t + key), "wide row forms");
                    if (na_wide_valid<G>(32 * t + key, n.r0, n.c0)) {
                      CHECK(row < ROWS, "%s: admitted row %d of %d", name, row, ROWS);
                      admit(row);
                    }
                  } else {
                    const int row = na_k_row<G>(na_k_row0<G>(n.korg, key), t);
                    if (l31 == 0) CHECK(row == n.korg + (2 * t + (key >> 4)) * HC + (key & 15), "local key 16 r + c is image row korg + HC r + c");
                    max_row = std::max(max_row, row);      // every K fragment row of the wave (the V rows are the same rows, below)
                    const bool ok = colv[i & 7] > 0 && rowv[2 * t + (i >> 3)] > 0;
                    CHECK((colv[i & 7] > 0) == (bool)KD_NA_COL_OK(KS, i & 7, h2, n.c0) && (rowv[2 * t + (i >> 3)] > 0) == (bool)KD_NA_ROW_OK(KS, 2 * t + (i >> 3), n.r0), "words");
                    if (ok) admit(row);
                  }
                }
              // V^T reads of k-step (t, u): k-slot s of lane-half h2 is probability register 8 u + s, the same key as on the K side
              // (the patch is the wave's: once per wave)
              for (int t = 0; t < NKT && l31 == 0; ++t)
                for (int u = 0; u < 2; ++u)
                  for (int s = 0; s < 8; ++s) {
                    const int key = na_acc_key(8 * u + s, h2);
                    if constexpr (WIDE) {
                      const int k0 = 32 * t + 16 * u + 4 * h2 + 8 * (s >> 2);      // the group's first key: the kernels add (lane & 15) >> 2
                      CHECK(na_wide_row<G>(n.korg, k0) + (s & 3) == na_wide_row<G>(n.korg, 32 * t + key), "a 4-key group lies in one patch row");
                    } else {
                      const int row = na_v_row<G>(na_v_row0(n.korg, h2, s & 3), t, u) + 8 * (s >> 2);
                      CHECK(row == na_k_row<G>(na_k_row0<G>(n.korg, key), t), "%s: V row %d of step (%d, %d) slot %d", name, row, t, u, s);
                      CHECK(row < ROWS, "%s %dx%d: V fragment row %d of %d", name, H, W, row, ROWS);
                    }
                  }
            }
            std::sort(got.begin(), got.end());
            const std::vector<int> want = rule_window(n.qy, n.qx, H, W, KS);
            CHECK(got == want, "%s %dx%d wg %d wave %d lane %d: query (%d, %d) admits %zu keys, first %d; the rule: %zu, first %d", name, H, W, wg, wid, l31, n.qy,
                  n.qx, got.size(), got.empty() ? -1 : got[0], want.size(), want[0]);
          }
      for (size_t i = 0; i < owners.size(); ++i) CHECK(owners[i] == 1, "%s %dx%d: token %zu is the query of %d lanes", name, H, W, i, owners[i]);
    }
  if (!WIDE) CHECK(max_row < ROWS, "%s: fragment row %d of %d", name, max_row, ROWS);
  if (!WIDE) CHECK(max_row == G::HR * HC - KS + 8, "%s: the highest fragment row is %d, the derivation says %d", name, max_row, G::HR * HC - KS + 8);
}

// ---- KeySet<KS_NA>: allowed and j < n_keys give every query of every 4 x 4 block its window ----------------------------------------------------
static void check_keyset_na(int ks) {
  for (const auto& hw : grids(ks)) {
      const int H = hw.first, W = hw.second;
      const Args a{H * W, H, W, 1, ks, 0};
      std::vector<int> owners(H * W, 0);
      const int blocks = ((H + 3) / 4) * ((W + 3) / 4);
      for (int qb = 0; qb < blocks; ++qb)
        for (int g = 0; g < 16; ++g) {
          KeySet<KS_NA> k;
          k.init(a, qb, g);
          CHECK(k.qtok >= 0 && k.qtok < H * W && k.n_keys > 0 && k.n_keys <= H * W, "keyset %d %dx%d", ks, H, W);
          if (!k.qactive) continue;
          ++owners[k.qtok];
          std::vector<int> got;
          for (int j = 0; j < k.n_keys + 8; ++j) {
            if (!k.allowed(a, j)) continue;
            CHECK(j < k.n_keys, "allowed past n_keys");
            const int tok = k.key_tok(a, j);
            CHECK(tok >= 0 && tok < H * W, "key token");
            got.push_back(tok);
          }
          std::sort(got.begin(), got.end());
          CHECK(got == rule_window(k.qtok / W, k.qtok % W, H, W, ks), "KeySet<KS_NA> ks %d %dx%d block %d query %d", ks, H, W, qb, g);
        }
      for (int t = 0; t < H * W; ++t) CHECK(owners[t] == 1, "KeySet<KS_NA> ks %d %dx%d: token %d owned %d times", ks, H, W, t, owners[t]);
    }
}

// ---- shifted window ------------------------------------------------------------------------------------------------------------------------------
template <int MODE>
static void check_window() {
  constexpr int L = WinLog2<MODE>::v, ws = 1 << L, T = ws * ws;
  for (int shift = 0; shift < ws; ++shift)
    for (int nwh = 1; nwh <= 3; ++nwh)
      for (int nww = 1; nww <= 3; ++nww) {
        const int H = nwh * ws, W = nww * ws;
        const Args a{H * W, H, W, 1, ws, shift};
        std::vector<int> seen(H * W, 0), tok(T), reg(T);
        for (int wi = 0; wi < nwh; ++wi)
          for (int wj = 0; wj < nww; ++wj) {
            for (int s = 0; s < T; ++s) {
              tok[s] = slot_token<MODE>(a, s, wi, wj);
              reg[s] = slot_region<MODE>(shift, s, wi, wj);
              const int i = ((wi * ws + (s >> L) - shift) % H + H) % H, j = ((wj * ws + (s & (ws - 1)) - shift) % W + W) % W;      // rolled[i] = orig[(i - shift) mod H]
              CHECK(tok[s] == i * W + j, "ws %d shift %d %dx%d window (%d, %d) slot %d", ws, shift, H, W, wi, wj, s);
              CHECK(tok[s] == win_token(a, ws, wi, wj, s / ws, s % ws) && reg[s] == win_region(shift, wi, wj, s / ws, s % ws), "run-time form");
              CHECK(reg[s] == ((wi == 0 && (s >> L) < shift) ? 2 : 0) + ((wj == 0 && (s & (ws - 1)) < shift) ? 1 : 0), "region");
              ++seen[tok[s]];
            }
            // KeySet<KS_WINDOW>: blocks of 16 queries, window-major
            const int win = wi * nww + wj;
            for (int s = 0; s < T; ++s) {
              KeySet<KS_WINDOW> k;
              k.init(a, win * (T / 16) + s / 16, s % 16);
              CHECK(k.qactive && k.qtok == tok[s] && k.n_keys == T, "KeySet<KS_WINDOW> ws %d shift %d %dx%d window %d slot %d", ws, shift, H, W, win, s);
              for (int j = 0; j < T; ++j) {
                if (s % 16 == 0) CHECK(k.key_tok(a, j) == tok[j], "KeySet<KS_WINDOW> key %d", j);      // the key side is the block's
                CHECK(k.allowed(a, j) == (reg[s] == reg[j]), "KeySet<KS_WINDOW> ws %d shift %d %dx%d window %d pair (%d, %d)", ws, shift, H, W, win, s, j);
              }
              CHECK(!k.allowed(a, T), "allowed past n_keys");
            }
          }
        for (int t = 0; t < H * W; ++t) CHECK(seen[t] == 1, "ws %d shift %d %dx%d: token %d in %d slots", ws, shift, H, W, t, seen[t]);
      }
}

// ---- what the pytest compares with oracle/hdit.py ------------------------------------------------------------------------------------------------
static void print_starts(int len, int ks) {
  std::printf("start %d %d", len, ks);
  for (int i = 0; i < len; ++i) {
    CHECK(na_start(i, len, ks) == na_origin(i, len, ks, ks) && na_start(i, len, ks) == rule_start(i, len, ks), "na_start(%d, %d, %d)", i, len, ks);
    std::printf(" %d", na_start(i, len, ks));
  }
  std::printf("\n");
}
template <int MODE>
static void print_window(int nwh, int nww, int shift) {
  constexpr int L = WinLog2<MODE>::v, ws = 1 << L, T = ws * ws;
  const int H = nwh * ws, W = nww * ws;
  const Args a{H * W, H, W, 1, ws, shift};
  std::printf("wintok %d %d %d %d", H, W, ws, shift);
  for (int wi = 0; wi < nwh; ++wi)
    for (int wj = 0; wj < nww; ++wj)
      for (int s = 0; s < T; ++s) std::printf(" %d", slot_token<MODE>(a, s, wi, wj));
  std::printf("\nwinmask %d %d %d %d ", H, W, ws, shift);
  for (int wi = 0; wi < nwh; ++wi)
    for (int wj = 0; wj < nww; ++wj)
      for (int s = 0; s < T; ++s)
        for (int j = 0; j < T; ++j) std::putchar(slot_region<MODE>(shift, s, wi, wj) == slot_region<MODE>(shift, j, wi, wj) ? '1' : '0');
  std::printf("\n");
}

int main() {
  // image sizes as the kernels' files pin them
  static_assert(NaGeoB16<7>::LDS == 39936 && NaGeoX3<7>::LDS == 79872 && NaWideB16<11>::LDS == 131072 && NaWideX3<13>::LDS == 153600, "image sizes");
  check_na_form<NaGeoB16<3>, false>("bf16 3");
  check_na_form<NaGeoB16<5>, false>("bf16 5");
  check_na_form<NaGeoB16<7>, false>("bf16 7");
  check_na_form<NaGeoB16<9>, false>("bf16 9");
  check_na_form<NaGeoX3<3>, false>("split3 3");
  check_na_form<NaGeoX3<5>, false>("split3 5");
  check_na_form<NaGeoX3<7>, false>("split3 7");
  check_na_form<NaGeoX3<9>, false>("split3 9");
  check_na_form<NaWideB16<11>, true>("bf16 wide 11");
  check_na_form<NaWideB16<13>, true>("bf16 wide 13");
  check_na_form<NaWideX3<11>, true>("split3 wide 11");
  check_na_form<NaWideX3<13>, true>("split3 wide 13");
  for (int ks = 3; ks <= 13; ks += 2) check_keyset_na(ks);
  check_window<MODE_WINDOW4>();
  check_window<MODE_WINDOW>();
  check_window<MODE_WINDOW16>();
  // the halo origin of an axis shorter than the halo is 0, else the clamp rule with the halo for the window
  for (int ks = 3; ks <= 13; ks += 2)
    for (int len = ks; len <= 40; ++len)
      for (int t0 = 0; t0 < len; t0 += NA_TH) {
        const int halo = NA_TW + ks - 1, o = na_halo_origin(t0, len, ks, halo);
        CHECK(o == (len <= halo ? 0 : std::min(std::max(t0 - ks / 2, 0), len - halo)), "halo origin %d %d %d", t0, len, ks);
      }
  // the entry points' refusals
  CHECK(na_check("kd_x", 7, 7, 9) == KD_OK && window_check("kd_x", 16, 32, 8, 7) == KD_OK, "accepted");
  CHECK(na_check("kd_x", 4, 8, 8) == KD_EINVAL && g_last_error == "kd_x: kernel_size 4 unsupported (odd sizes 3 .. 13)", "%s", g_last_error.c_str());
  CHECK(na_check("kd_x", 15, 32, 32) == KD_EINVAL && na_check("kd_x", 1, 32, 32) == KD_EINVAL, "sizes");
  CHECK(na_check("kd_x", 7, 6, 9) == KD_EINVAL && g_last_error == "kd_x: grid 6x9 smaller than the 7x7 neighbourhood", "%s", g_last_error.c_str());
  CHECK(window_check("kd_x", 16, 16, 5, 0) == KD_EINVAL && g_last_error == "kd_x: window_size 5 unsupported (4, 8 or 16)", "%s", g_last_error.c_str());
  CHECK(window_check("kd_x", 16, 20, 8, 0) == KD_EINVAL && g_last_error == "kd_x: grid 16x20 not divisible by the window", "%s", g_last_error.c_str());
  CHECK(window_check("kd_x", 16, 16, 8, 8) == KD_EINVAL && g_last_error == "kd_x: bad shift 8" && window_check("kd_x", 16, 16, 8, -1) == KD_EINVAL, "%s",
        g_last_error.c_str());

  for (int ks = 3; ks <= 13; ks += 2)
    for (int len : {ks, ks + 1, 16 + ks - 2, 16 + ks - 1, 37}) print_starts(len, ks);
  print_window<MODE_WINDOW4>(1, 1, 0);
  print_window<MODE_WINDOW4>(2, 3, 1);
  print_window<MODE_WINDOW4>(3, 2, 3);
  print_window<MODE_WINDOW>(1, 1, 4);
  print_window<MODE_WINDOW>(2, 3, 1);
  print_window<MODE_WINDOW>(3, 3, 7);
  print_window<MODE_WINDOW16>(1, 2, 8);
  print_window<MODE_WINDOW16>(2, 1, 15);
  std::printf("checks %ld\nok\n", g_checks);
  return 0;
}
