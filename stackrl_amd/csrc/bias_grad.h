// bias_grad.h — the bias gradient of the update path as fixed-order partial sums: what the backward passes of
// csrc/epilogue.hip (k_bias_act_bwd, 8 channels per thread) and csrc/train_conv.hip (k_tact_bwd, 4 channels per thread) share.
// Each of their blocks walks `pixb` consecutive pixels and writes one partial sum per channel; k_bias_grad_finish adds the
// partials in index order: a fixed summation order and no cross-block synchronisation inside a kernel.
#ifndef SRL_BIAS_GRAD_H_
#define SRL_BIAS_GRAD_H_

#include <hip/hip_runtime.h>

// pixels per block of the backward pass (thread = pixel lane x group of `group` channels): at most 1,024 blocks, whole
// iterations of the block's pixel lanes
static inline int bias_grad_pixb(long long npix, int C, int group) {
  const int ppi = 256 / (C / group);
  long long pixb = (npix + 1023) / 1024;
  if (pixb < 4 * ppi) pixb = 4 * ppi;
  return (int)((pixb + ppi - 1) / ppi * ppi);
}

// gb[c] = sum over blocks of partial[b][c], in a fixed order: a workgroup takes 32 channels (or all C < 32), its 256
// threads are (row r, channel): row r adds the blocks r, r + rows, ... in turn (coalesced 128-byte reads), then the rows
// are added in index order.
static __global__ void __launch_bounds__(256) k_bias_grad_finish(const float* __restrict__ partial, int nblk, int C,
                                                                 float* __restrict__ gb) {
  __shared__ float sh[256];
  const int cw = C < 32 ? C : 32, rows = 256 / cw;
  const int c = blockIdx.x * cw + threadIdx.x % cw, r = threadIdx.x / cw;
  float s = 0.0f;
  if (r < rows && c < C)
    for (int b = r; b < nblk; b += rows) s += partial[(long long)b * C + c];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < cw && c < C) {
    float t = 0.0f;
    for (int q = 0; q < rows; ++q) t += sh[q * cw + threadIdx.x];
    gb[c] = t;
  }
}

#endif
