// Stand-alone check of kd_run_list's unpacking (k-diffusion_amd/csrc/run_list.cpp) without a GPU: compiled together with run_list.cpp, the
// 15 entry points a list can name are stubs that record what they receive.  For every KD_OP_* a KdCall is filled with distinct sentinels by
// the rule of include/kdiff_hip.h (pointers in declaration order in p[], ints in i[], the float in f) and each value must arrive at the
// parameter the header declares it at; an op outside the table must be refused with KD_EINVAL, *failed set and nothing launched.
// Prints one line per op, "<op> <entry point> <kinds>" (p / i / f per parameter, stream included), for tests/test_abi_cpu.py, then "ok".
#include "../include/kdiff_hip.h"
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace kd {
static char g_err[512];
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace kd

namespace {
struct Arg {
  char kind;
  const void* p;
  int i;
  float f;
};
struct Record {
  int op;
  const char* name;
  std::vector<Arg> args;
};
std::vector<Record> g_seen;
int g_return = KD_OK;

void push(Record& r, const void* p) { r.args.push_back({'p', p, 0, 0.f}); }
void push(Record& r, int i) { r.args.push_back({'i', nullptr, i, 0.f}); }
void push(Record& r, float f) { r.args.push_back({'f', nullptr, 0, f}); }
// every stub hands over ALL its parameters in declaration order
template <class... A>
int rec(int op, const char* name, A... a) {
  Record r{op, name, {}};
  (push(r, a), ...);
  g_seen.push_back(r);
  return g_return;
}
}  // namespace

extern "C" {
int kd_gemm_f32(const KdGemm* desc, void* stream) { return rec(KD_OP_GEMM_F32, "kd_gemm_f32", desc, stream); }
int kd_gemm_bf16(const KdGemm* desc, void* stream) { return rec(KD_OP_GEMM_BF16, "kd_gemm_bf16", desc, stream); }
int kd_ffn_f32(const KdFfn* desc, void* stream) { return rec(KD_OP_FFN_F32, "kd_ffn_f32", desc, stream); }
int kd_ffn_bf16(const KdFfn* desc, void* stream) { return rec(KD_OP_FFN_BF16, "kd_ffn_bf16", desc, stream); }
int kd_attn_global_f32(const float* qkv, float* out, int batch, int T, int nh, int prep, const float* scale_h, const float* cos_t,
                       const float* sin_t, float eps, int precision, void* stream) {
  return rec(KD_OP_ATTN_GLOBAL_F32, "kd_attn_global_f32", qkv, out, batch, T, nh, prep, scale_h, cos_t, sin_t, eps, precision, stream);
}
int kd_attn_window_f32(const float* qkv, float* out, int batch, int H, int W, int nh, int ws, int shift, int prep, const float* scale_h,
                       const float* cos_t, const float* sin_t, float eps, int precision, void* stream) {
  return rec(KD_OP_ATTN_WINDOW_F32, "kd_attn_window_f32", qkv, out, batch, H, W, nh, ws, shift, prep, scale_h, cos_t, sin_t, eps, precision,
             stream);
}
int kd_attn_na2d_f32(const float* qkv, float* out, int batch, int H, int W, int nh, int ks, int prep, const float* scale_h, const float* cos_t,
                     const float* sin_t, float eps, int precision, void* stream) {
  return rec(KD_OP_ATTN_NA2D_F32, "kd_attn_na2d_f32", qkv, out, batch, H, W, nh, ks, prep, scale_h, cos_t, sin_t, eps, precision, stream);
}
int kd_attn_global_bf16(const void* qkv, void* out, int batch, int T, int nh, void* stream) {
  return rec(KD_OP_ATTN_GLOBAL_BF16, "kd_attn_global_bf16", qkv, out, batch, T, nh, stream);
}
int kd_attn_window_bf16(const void* qkv, void* out, int batch, int H, int W, int nh, int ws, int shift, void* stream) {
  return rec(KD_OP_ATTN_WINDOW_BF16, "kd_attn_window_bf16", qkv, out, batch, H, W, nh, ws, shift, stream);
}
int kd_attn_na2d_bf16(const void* qkv, void* out, int batch, int H, int W, int nh, int ks, void* stream) {
  return rec(KD_OP_ATTN_NA2D_BF16, "kd_attn_na2d_bf16", qkv, out, batch, H, W, nh, ks, stream);
}
int kd_norm_split_f32(const float* x, const float* scale, int scale_stride, int rows_per_sample, void* hi, void* lo, int M, int K, float eps,
                      void* stream) {
  return rec(KD_OP_NORM_SPLIT_F32, "kd_norm_split_f32", x, scale, scale_stride, rows_per_sample, hi, lo, M, K, eps, stream);
}
int kd_attn_block_bf16(const KdGemm* d, void* stream) { return rec(KD_OP_ATTN_BLOCK_BF16, "kd_attn_block_bf16", d, stream); }
int kd_proj_block_bf16(const KdGemm* d, void* stream) { return rec(KD_OP_PROJ_BLOCK_BF16, "kd_proj_block_bf16", d, stream); }
int kd_gemm_mx8(const KdGemm* d, void* stream) { return rec(KD_OP_GEMM_MX8, "kd_gemm_mx8", d, stream); }
int kd_attn_ffn_f32(const float* qkv, const KdFfn* desc, int batch, int H, int W, int nh, int ks, void* stream) {
  return rec(KD_OP_ATTN_FFN_F32, "kd_attn_ffn_f32", qkv, desc, batch, H, W, nh, ks, stream);
}
}

#define CHECK(cond, ...)                                       \
  do {                                                         \
    if (!(cond)) {                                             \
      std::fprintf(stderr, "run_list_check: " __VA_ARGS__);    \
      std::fprintf(stderr, "  [%s]\n", #cond);                 \
      return 1;                                                \
    }                                                          \
  } while (0)

static char g_memory[64];                    // sentinel addresses point into real storage; nothing dereferences them
static KdCall sentinel_call(int op) {
  KdCall c;
  c.op = op;
  c.f = 0.25f + float(op);
  for (int k = 0; k < 5; ++k) c.p[k] = g_memory + 1 + 8 * k + (op & 7);
  for (int k = 0; k < 8; ++k) c.i[k] = 1000 * (op + 1) + 10 * k + 3;
  return c;
}

int main() {
  const int n_ops = KD_OP_ATTN_FFN_F32 + 1;
  void* const stream = g_memory + 60;
  // one list with every op in turn: each stub is reached once, in order, with its values at the declared parameters
  std::vector<KdCall> calls;
  for (int op = 0; op < n_ops; ++op) calls.push_back(sentinel_call(op));
  int failed = -7;
  CHECK(kd_run_list(calls.data(), n_ops, stream, &failed) == KD_OK && failed == -7, "a good list failed: %s\n", kd::g_err);
  CHECK(int(g_seen.size()) == n_ops, "%d launches for %d entries\n", int(g_seen.size()), n_ops);
  for (int op = 0; op < n_ops; ++op) {
    const Record& r = g_seen[op];
    const KdCall& c = calls[op];
    CHECK(r.op == op, "entry %d reached the stub of op %d (%s)\n", op, r.op, r.name);
    CHECK(!r.args.empty() && r.args.back().kind == 'p' && r.args.back().p == stream, "%s: the stream is not the last argument\n", r.name);
    int np = 0, ni = 0, nf = 0;
    std::string kinds;
    for (std::size_t a = 0; a + 1 < r.args.size(); ++a) {
      const Arg& g = r.args[a];
      kinds += g.kind;
      if (g.kind == 'p') {
        CHECK(np < 5 && g.p == c.p[np], "%s: parameter %d is not p[%d]\n", r.name, int(a), np);
        ++np;
      } else if (g.kind == 'i') {
        CHECK(ni < 8 && g.i == c.i[ni], "%s: parameter %d is %d, not i[%d] = %d\n", r.name, int(a), g.i, ni, ni < 8 ? c.i[ni] : 0);
        ++ni;
      } else {
        CHECK(nf == 0 && g.f == c.f, "%s: parameter %d is %g, not f = %g\n", r.name, int(a), g.f, c.f);
        ++nf;
      }
    }
    std::printf("%d %s %sp\n", op, r.name, kinds.c_str());
  }
  // an op outside the table: KD_EINVAL, the entry's index in *failed, the message of the library, nothing launched after the good entries
  const int bad_ops[] = {-1, n_ops, 99};
  for (int bad : bad_ops) {
    g_seen.clear();
    KdCall three[3] = {sentinel_call(KD_OP_GEMM_MX8), sentinel_call(0), sentinel_call(KD_OP_FFN_F32)};
    three[1].op = bad;
    failed = -7;
    kd::g_err[0] = 0;
    CHECK(kd_run_list(three, 3, stream, &failed) == KD_EINVAL, "op %d was not refused\n", bad);
    CHECK(failed == 1, "op %d: *failed = %d\n", bad, failed);
    CHECK(g_seen.size() == 1 && g_seen[0].op == KD_OP_GEMM_MX8, "op %d: %d launches\n", bad, int(g_seen.size()));
    char want[128];
    std::snprintf(want, sizeof(want), "kd_run_list: entry 1 names no entry point (op %d)", bad);
    CHECK(!std::strcmp(kd::g_err, want), "op %d: message '%s'\n", bad, kd::g_err);
    CHECK(kd_run_list(three + 1, 1, stream, nullptr) == KD_EINVAL && g_seen.size() == 1, "op %d with failed == NULL\n", bad);
  }
  // an entry point's own failure stops the list there and comes back as it is
  g_seen.clear();
  g_return = KD_ELAUNCH;
  failed = -7;
  CHECK(kd_run_list(calls.data(), n_ops, stream, &failed) == KD_ELAUNCH && failed == 0 && g_seen.size() == 1, "a failing entry did not stop the list\n");
  g_return = KD_OK;
  CHECK(kd_run_list(nullptr, 1, stream, &failed) == KD_EINVAL && kd_run_list(calls.data(), -1, stream, &failed) == KD_EINVAL, "null list / negative n\n");
  CHECK(kd_run_list(calls.data(), 0, stream, nullptr) == KD_OK, "empty list\n");
  std::printf("ok\n");
  return 0;
}
