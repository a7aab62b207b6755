// The second pass of the convolution weight gradients (conv_wgrad_x3.hip, conv_wgrad_bf16.hip): the partial tiles of the workspace
// [nchunk][tap][co][ci] summed in ascending order into nn.Conv2d's [co][ci][ky][kx] layout.  One text for both arithmetics: the first pass alone
// differs.
#pragma once
#include "kd_common.h"

namespace kd {

namespace {

// dw[co][ci][tap] (+)= scale(co) * sum over the chunks, ascending, of ws[chunk][tap][co][ci]; a thread's index runs ci-fastest over the workspace
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int c_out, int c_in, int taps,
                                                                int nchunk, int q_rows, int accumulate) {
  const long plane = (long)c_out * c_in, n_el = plane * taps;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long)gridDim.x * 256) {
    const int tap = (int)(i / plane);
    const long rem = i - tap * plane;
    const int co = (int)(rem / c_in);
    float sum = 0.f;
    for (int k = 0; k < nchunk; ++k) sum += ws[(long)k * n_el + i];
    if (co < q_rows) sum *= 0.125f;
    float* o = dw + rem * taps + tap;
    *o = accumulate ? *o + sum : sum;
  }
}

}  // namespace

}  // namespace kd
