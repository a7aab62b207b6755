// Training batches from a dataset that lives in device memory as uint8 (gfx950): CIFAR-10 and MNIST are arrays, 150 MB and 47 MB, and the
// reference reaches them through torchvision datasets, PIL and data-loader workers (train.py:207-210, :449-450).  Here one launch assembles a
// step's batch from the resident array, and the same rule drops the class labels of a batch that came through a DataLoader.
//
//   kd_batch_u8_f32       out[b] = data[idx[b]] as fp32 in [-1, 1] with the bits of utils.from_pil_image, class_out[b] = labels[idx[b]] after
//                         conditioning dropout
//   kd_class_dropout_i64  out[b] = labels[b] after conditioning dropout
//
// Contract (arithmetic, counter): include/kdiff_hip.h.  The kernels are launch-sized (0.2 MB in, 0.8 MB out at CIFAR batch 64): one lane per
// element, byte loads throughout -- an image of C H W bytes starts at any byte address, so there is no alignment to exploit without a second
// path -- and stores contiguous along the sample.
#include "kd_common.h"
#include "philox.h"

namespace kd {

namespace {

constexpr unsigned long long COND_DROP_STREAM = 0xC000000100000000ull;     // 2^63 | 2^62 | 2^32: beside the augmentation's blocks 0 .. 3

// (float)u / 255 * 2 - 1 for the 256 byte values, evaluated by the COMPILER in IEEE fp32 (round to nearest): the bits torch's three fp32
// operations give.  On the device the divide would depend on the build's division flags; the multiply by 2 is exact, so contracting it with
// the subtraction changes nothing -- the table takes both questions away.
struct U8Table { float v[256]; };
constexpr U8Table make_u8_table() {
  U8Table t{};
  for (int u = 0; u < 256; ++u) {
    const float q = (float)u / 255.0f;
    const float d = q * 2.0f;
    t.v[u] = d - 1.0f;
  }
  return t;
}
constexpr U8Table U8_HOST = make_u8_table();
static_assert(U8_HOST.v[0] == -1.0f && U8_HOST.v[255] == 1.0f && U8_HOST.v[85] == -0.33333331f, "u8 -> [-1, 1] table");
__device__ const U8Table U8_TO_UNIT = make_u8_table();

// conditioning dropout of sample b of a batch: the label, or num_classes iff u(w0) < drop_rate (fp32)
__device__ __forceinline__ long long cond_dropout(long long label, unsigned long long key, long b, float drop_rate, int num_classes) {
  const Philox4 r = philox4x32_10(key, (unsigned long long)b, COND_DROP_STREAM);
  return unit24(r.x0) < drop_rate ? (long long)num_classes : label;
}

__global__ __launch_bounds__(256) void batch_u8_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ labels,
                                                       const long long* __restrict__ idx, const long long* __restrict__ key_ptr, float drop_rate,
                                                       int num_classes, float* __restrict__ out, long long* __restrict__ class_out, int chw,
                                                       unsigned tiles) {
  const unsigned b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const long long src = idx[b];
  if (class_out && tile == 0 && threadIdx.x == 0) {
    const unsigned long long key = drop_rate > 0.0f ? (unsigned long long)key_ptr[0] : 0ull;
    class_out[b] = cond_dropout(labels[src], key, (long)b, drop_rate, num_classes);
  }
  const int e = (int)(tile * 256u + threadIdx.x);
  if (e >= chw) return;
  out[(size_t)b * chw + e] = U8_TO_UNIT.v[data[(size_t)src * chw + e]];
}

// (labels and out are not __restrict__: out may be labels)
__global__ __launch_bounds__(256) void class_dropout_kernel(const long long* labels, const long long* key_ptr, float drop_rate, int num_classes,
                                                            long long* out, int batch) {
  const unsigned long long key = drop_rate > 0.0f ? (unsigned long long)key_ptr[0] : 0ull;
  for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < batch; b += (long)gridDim.x * 256)
    out[b] = cond_dropout(labels[b], key, b, drop_rate, num_classes);
}

bool rate_ok(float r) { return r >= 0.0f && r <= 1.0f; }

}  // namespace

}  // namespace kd

using namespace kd;

extern "C" int kd_batch_u8_f32(const unsigned char* data, const long long* labels, const long long* idx, const long long* key, float drop_rate,
                               int num_classes, float* out, long long* class_out, int batch, int chan, int H, int W, void* stream) {
  if (!data || !idx || !out || batch <= 0 || chan <= 0 || H <= 0 || W <= 0) return fail(KD_EINVAL, "kd_batch_u8_f32: bad arguments");
  if ((labels == nullptr) != (class_out == nullptr))
    return fail(KD_EINVAL, "kd_batch_u8_f32: labels and class_out go together (both NULL for unlabelled data)");
  if (labels) {
    if (!rate_ok(drop_rate)) return fail(KD_EINVAL, "kd_batch_u8_f32: drop_rate %g outside [0, 1]", (double)drop_rate);
    if (num_classes <= 0) return fail(KD_EINVAL, "kd_batch_u8_f32: labelled data needs num_classes > 0 (got %d)", num_classes);
    if (drop_rate > 0.0f && !key) return fail(KD_EINVAL, "kd_batch_u8_f32: drop_rate > 0 needs a key");
  }
  const long long chw = (long long)chan * H * W;
  if (chw > 0x7FFFFFFFll - 256) return fail(KD_EINVAL, "kd_batch_u8_f32: C * H * W = %lld does not fit the 32-bit element index", chw);
  const long long tiles = (chw + 255) / 256;
  if (tiles * batch > 0x7FFFFFFFll) return fail(KD_EINVAL, "kd_batch_u8_f32: %lld workgroups exceed the grid", tiles * batch);
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("batch_u8_f32", 0, 5.0 * (double)batch * (double)chw + (labels ? 24.0 : 8.0) * batch, s);
  launch<batch_u8_kernel>(dim3((unsigned)(tiles * batch)), dim3(256), 0, s, data, labels, idx, key, drop_rate, num_classes, out, class_out,
                          (int)chw, (unsigned)tiles);
  return check_launch("kd_batch_u8_f32");
}

extern "C" int kd_class_dropout_i64(const long long* labels, const long long* key, float drop_rate, int num_classes, long long* out, int batch,
                                    void* stream) {
  if (!labels || !out || batch <= 0) return fail(KD_EINVAL, "kd_class_dropout_i64: bad arguments");
  if (!rate_ok(drop_rate)) return fail(KD_EINVAL, "kd_class_dropout_i64: drop_rate %g outside [0, 1]", (double)drop_rate);
  if (num_classes <= 0) return fail(KD_EINVAL, "kd_class_dropout_i64: num_classes must be positive (got %d)", num_classes);
  if (drop_rate > 0.0f && !key) return fail(KD_EINVAL, "kd_class_dropout_i64: drop_rate > 0 needs a key");
  hipStream_t s = (hipStream_t)stream;
  LaunchScope prof("class_dropout_i64", 0, 16.0 * batch, s);
  const unsigned blocks = (unsigned)std::min<long>(((long)batch + 255) / 256, 16384);
  launch<class_dropout_kernel>(dim3(blocks), dim3(256), 0, s, labels, key, drop_rate, num_classes, out, batch);
  return check_launch("kd_class_dropout_i64");
}
