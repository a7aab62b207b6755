// kd_run_list (include/kdiff_hip.h): a launch list in one host call.  Host code only -- no HIP header, so this file (and the check of it in
// tests/run_list_check.cpp) compiles with any C++17 compiler.
//
// g_rows is the table: one row per KD_OP_* with the entry point it names.  A KdCall carries the entry point's arguments by one rule -- its
// pointer parameters in declaration order in p[], its int parameters in declaration order in i[], its one float in f, the trailing
// void* stream from the list's own -- and Unpack reads that rule off the entry point's TYPE: nothing per op is written out by hand.
#include "../../include/kdiff_hip.h"
#include <cstddef>
#include <tuple>
#include <type_traits>
#include <utility>

namespace kd {
int fail(int code, const char* fmt, ...);      // common.cpp
}

namespace {

enum Kind { K_PTR, K_INT, K_FLOAT, K_OTHER };
template <class T>
constexpr Kind kind_of() {
  return std::is_pointer<T>::value ? K_PTR : std::is_same<T, int>::value ? K_INT : std::is_same<T, float>::value ? K_FLOAT : K_OTHER;
}
// how many of the first n parameters P... are of `kind`: the slot of parameter n within its kind
template <class... P>
constexpr int count_kind(Kind kind, std::size_t n) {
  constexpr Kind kinds[] = {kind_of<P>()...};
  int c = 0;
  for (std::size_t k = 0; k < n; ++k) c += kinds[k] == kind;
  return c;
}
template <class T, int Slot>
T fetch(const KdCall& c) {
  if constexpr (std::is_pointer<T>::value) return static_cast<T>(const_cast<void*>(c.p[Slot]));
  else if constexpr (std::is_same<T, int>::value) return c.i[Slot];
  else return c.f;
}

template <auto Fn>
struct Unpack;
template <class... P, int (*Fn)(P...)>
struct Unpack<Fn> {
  using Params = std::tuple<P...>;
  static constexpr std::size_t N = sizeof...(P) - 1;      // parameters a KdCall carries: all but the trailing stream
  static_assert(std::is_same<std::tuple_element_t<N, Params>, void*>::value, "the last parameter of a run-list entry point is void* stream");
  static_assert(count_kind<P...>(K_PTR, N) <= int(sizeof(KdCall{}.p) / sizeof(KdCall{}.p[0])), "more pointer parameters than KdCall.p holds");
  static_assert(count_kind<P...>(K_INT, N) <= int(sizeof(KdCall{}.i) / sizeof(KdCall{}.i[0])), "more int parameters than KdCall.i holds");
  static_assert(count_kind<P...>(K_FLOAT, N) <= 1, "KdCall carries one float");
  static_assert(count_kind<P...>(K_OTHER, N) == 0, "a parameter that is neither a pointer, an int nor a float");
  template <std::size_t... K>
  static int call(const KdCall& c, void* stream, std::index_sequence<K...>) {
    return Fn(fetch<std::tuple_element_t<K, Params>, count_kind<P...>(kind_of<std::tuple_element_t<K, Params>>(), K)>(c)..., stream);
  }
  static int run(const KdCall& c, void* stream) { return call(c, stream, std::make_index_sequence<N>{}); }
};

struct Row {
  int op;
  int (*run)(const KdCall&, void*);
};
#define KD_ROW(OP, fn) {OP, &Unpack<&fn>::run}
constexpr Row g_rows[] = {
    KD_ROW(KD_OP_GEMM_F32, kd_gemm_f32),
    KD_ROW(KD_OP_GEMM_BF16, kd_gemm_bf16),
    KD_ROW(KD_OP_FFN_F32, kd_ffn_f32),
    KD_ROW(KD_OP_FFN_BF16, kd_ffn_bf16),
    KD_ROW(KD_OP_ATTN_GLOBAL_F32, kd_attn_global_f32),
    KD_ROW(KD_OP_ATTN_WINDOW_F32, kd_attn_window_f32),
    KD_ROW(KD_OP_ATTN_NA2D_F32, kd_attn_na2d_f32),
    KD_ROW(KD_OP_ATTN_GLOBAL_BF16, kd_attn_global_bf16),
    KD_ROW(KD_OP_ATTN_WINDOW_BF16, kd_attn_window_bf16),
    KD_ROW(KD_OP_ATTN_NA2D_BF16, kd_attn_na2d_bf16),
    KD_ROW(KD_OP_NORM_SPLIT_F32, kd_norm_split_f32),
    KD_ROW(KD_OP_ATTN_BLOCK_BF16, kd_attn_block_bf16),
    KD_ROW(KD_OP_PROJ_BLOCK_BF16, kd_proj_block_bf16),
    KD_ROW(KD_OP_GEMM_MX8, kd_gemm_mx8),
    KD_ROW(KD_OP_ATTN_FFN_F32, kd_attn_ffn_f32),
};
#undef KD_ROW
constexpr int N_ROWS = int(sizeof(g_rows) / sizeof(g_rows[0]));
template <int K>
constexpr bool rows_in_order() {              // one static_assert per row: row k of the table is KD_OP number k
  static_assert(g_rows[K].op == K, "g_rows: a row is not at the index of its KD_OP_* number");
  if constexpr (K + 1 < N_ROWS) return rows_in_order<K + 1>();
  return true;
}
static_assert(rows_in_order<0>(), "");

}  // namespace

extern "C" int kd_run_list(const KdCall* calls, int n, void* stream, int* failed) {
  if (!calls || n < 0) return kd::fail(KD_EINVAL, "kd_run_list: null list");
  for (int k = 0; k < n; ++k) {
    const KdCall& c = calls[k];
    const int rc = c.op >= 0 && c.op < N_ROWS ? g_rows[c.op].run(c, stream)
                                               : kd::fail(KD_EINVAL, "kd_run_list: entry %d names no entry point (op %d)", k, c.op);
    if (rc != KD_OK) {
      if (failed) *failed = k;
      return rc;
    }
  }
  return KD_OK;
}
