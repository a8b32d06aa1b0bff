// mfma_bf16.h — what the rollout's matrix-core convolutions (csrc/conv_mfma.hip, csrc/conv_gemm.hip) share around
// v_mfma_f32_16x16x32_bf16, gfx950: the fragment types (csrc/xcorr_mfma.hip takes these too), the fp32-class ("bf16x3")
// operand split and product, and the bias + ReLU of the four consecutive output channels a lane holds of an accumulator tile.
#ifndef SRL_MFMA_BF16_H_
#define SRL_MFMA_BF16_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srl_bf16.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));   // an A or B fragment: 8 consecutive k of one row / column
typedef float f32x4 __attribute__((ext_vector_type(4)));    // a D fragment: rows 4 (lane >> 4) .. + 3 of column lane & 15

// The three pieces below are macros: as inline functions each of them changed the instruction schedule of kernels that use
// it, as macros none does (profiles/rollout_conv_refactor.txt).  The two statement macros are braced blocks: no `;` after them.

// Eight consecutive float32 channels (the float4 a, then c) as a hi and a lo bf16 fragment, each a uint4 (stored to an LDS
// plane as it is, or bit-cast to bf16x8): x = hi + lo up to 2^-17 |x| (srl_split_bf16).
#define SRL_SPLIT8(a, c, hi, lo) \
  { \
    const float v_[8] = {(a).x, (a).y, (a).z, (a).w, (c).x, (c).y, (c).z, (c).w}; \
    uint32_t ph_[4], pl_[4]; \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) srl_split_bf16(v_[2 * j_], v_[2 * j_ + 1], ph_[j_], pl_[j_]); \
    hi = make_uint4(ph_[0], ph_[1], ph_[2], ph_[3]); \
    lo = make_uint4(pl_[0], pl_[1], pl_[2], pl_[3]); \
  }

// acc += W X in fp32-class precision from the split operands: the small terms first (lo hi, hi lo), then the leading one
#define SRL_MFMA_X3(acc, wh, wl, xh, xl) \
  { \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc, 0, 0, 0); \
  }

// relu(acc + bias) of the lane's four channels, as a float4 (acc: f32x4, bz: the float4 of biases)
#define SRL_BIAS_RELU(acc, bz) \
  make_float4(fmaxf((acc)[0] + (bz).x, 0.0f), fmaxf((acc)[1] + (bz).y, 0.0f), fmaxf((acc)[2] + (bz).z, 0.0f), fmaxf((acc)[3] + (bz).w, 0.0f))

#endif
