// qnet.hip — hand-written ops of the Q-network rollout path (include/stackrl_qnet.h), gfx950.
//
// K6 xcorr: out[b,u,v] = sum_{c,i,j} x[b,c,u+i,v+j] * w[b,c,i,j]   (layers.py:21-38)
//   fp32 FMA on the vector ALU (the reference computes in fp32; gfx950 has no faster exact-fp32 matrix path:
//   v_mfma_f32_*_f32 runs at the vector rate).  One thread owns a strip of 8 adjacent outputs of one row: for
//   every (channel, kernel row) it loads the 8 + kw - 1 inputs the strip needs into registers once and sweeps the
//   kernel row over them; the kernel row w[b,c,i,:] is wave-uniform, so it comes in through scalar loads and sits
//   in SGPRs as the FMA operand — no LDS traffic at all, 256 FMAs per 39 vector loads.
//
// policy head: one workgroup per env row; (value, index) arg-max with lowest-index ties, then epsilon-greedy select.
// Boltzmann head: the same arg-max over adv / T + Gumbel noise made in registers from the sample's Philox stream
//   (the definition: include/stackrl_explore.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/stackrl_explore.h"
#include "../../include/stackrl_qnet.h"

namespace {
thread_local char q_err[256] = "";

template <int KW, int SW>
__global__ void __launch_bounds__(256) k_xcorr_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                   float* __restrict__ out, int C, int H, int W, int kh, int OH, int OW) {
  const int b = blockIdx.y;
  const int u = blockIdx.x * blockDim.y + threadIdx.y;
  const int v0 = threadIdx.x * SW;
  const bool active = (u < OH) && (v0 < OW);
  const int uc = u < OH ? u : OH - 1;
  float acc[SW];
#pragma unroll
  for (int k = 0; k < SW; ++k) acc[k] = 0.0f;
  for (int c = 0; c < C; ++c) {
    const float* xc = x + ((size_t)b * C + c) * H * W;
    const float* wc = w + ((size_t)b * C + c) * kh * KW;     // uniform across the wave: scalar loads
    for (int i = 0; i < kh; ++i) {
      const float* xr = xc + (size_t)(uc + i) * W;
      float xs[SW + KW - 1];
#pragma unroll
      for (int t = 0; t < SW + KW - 1; ++t) {
        int col = v0 + t;
        xs[t] = xr[col < W ? col : W - 1];                     // clamped: only feeds outputs that are not stored
      }
      const float* wr = wc + i * KW;
#pragma unroll
      for (int j = 0; j < KW; ++j) {
        const float wj = wr[j];
#pragma unroll
        for (int k = 0; k < SW; ++k) acc[k] = fmaf(xs[k + j], wj, acc[k]);
      }
    }
  }
  if (active) {
    float* o = out + ((size_t)b * OH + u) * OW + v0;
#pragma unroll
    for (int k = 0; k < SW; ++k)
      if (v0 + k < OW) o[k] = acc[k];
  }
}

__global__ void __launch_bounds__(256) k_policy_head(const float* __restrict__ adv, const float* __restrict__ u,
                                                     const int64_t* __restrict__ rnd, float eps,
                                                     int64_t* __restrict__ actions, int A) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* a = adv + (size_t)b * A;
  // start: -inf at the thread's own first index — a pair that wins only what it may (a row of nothing but -inf or NaN
  // resolves to index 0); a thread without an entry holds an index that loses to every real one
  float best = -INFINITY; int bi = tid < A ? tid : 0x7fffffff;
  for (int k = tid; k < A; k += 256) {
    float t = a[k];
    if (t > best) { best = t; bi = k; }          // ascending k per thread: lowest index of its maxima
  }
  sv[tid] = best; si[tid] = bi;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) {
      float ov = sv[tid + s]; int oi = si[tid + s];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) actions[b] = (u[b] > eps) ? (int64_t)si[0] : rnd[b];   // tf.where(uniform > e, argmax, random), dqn.py:336-348
}

// Philox4x32-10 of the counter (c0, 0, 0, 0) under the key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t x[4]) {
  uint32_t c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

__global__ void __launch_bounds__(256) k_boltzmann_head(const float* __restrict__ adv, const int64_t* __restrict__ keys,
                                                        float temperature, int64_t* __restrict__ actions, int A) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* a = adv + (size_t)b * A;
  const uint32_t k0 = (uint32_t)keys[2 * (size_t)b], k1 = (uint32_t)keys[2 * (size_t)b + 1];
  // -inf at the thread's first index (a row of nothing but -inf resolves to index 0); a thread without a quad keeps an index
  // that loses to any real one
  float best = -INFINITY; int bi = 4 * tid < A ? 4 * tid : 0x7fffffff;
  const int quads = (A + 3) >> 2;
  for (int j = tid; j < quads; j += 256) {
    uint32_t x[4];
    philox4x32_10((uint32_t)j, k0, k1, x);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int k = 4 * j + l;
      if (k < A) {                                  // lanes of the last quad beyond A: neither read nor scored
        const float u = ((float)(x[l] >> 9) + 0.5f) * 1.1920928955078125e-07f;       // 2^-23; exact
        const float t = a[k] / temperature - logf(-logf(u));
        if (t > best) { best = t; bi = k; }        // ascending k per thread: lowest index of its maxima
      }
    }
  }
  sv[tid] = best; si[tid] = bi;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) {
      float ov = sv[tid + s]; int oi = si[tid + s];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid == 0) actions[b] = (int64_t)si[0];
}
}  // namespace

// for the other files of the library that report through srl_qnet_last_error (heuristics.hip); not part of the ABI
__attribute__((visibility("hidden"))) void srl_qnet_set_error(const char* msg) { snprintf(q_err, sizeof q_err, "%s", msg); }

extern "C" {

const char* srl_qnet_last_error(void) { return q_err; }

#ifndef SRL_BUILD_INFO
#define SRL_BUILD_INFO "SRL_BUILD_INFO<unknown|>"
#endif
const char* srl_qnet_build_info(void) { static const char info[] = SRL_BUILD_INFO; return info; }

int srl_xcorr_forward(const float* x, const float* w, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                      int32_t kh, int32_t kw, void* stream) {
  if (!x || !w || !out || B < 1 || C < 1 || kh < 1 || H < kh || W < kw) {
    snprintf(q_err, sizeof q_err, "srl_xcorr_forward: bad arguments");
    return 1;
  }
  const int OH = H - kh + 1, OW = W - kw + 1;
  constexpr int SW = 8;
  const int strips = (OW + SW - 1) / SW;
  if (strips > 64) { snprintf(q_err, sizeof q_err, "srl_xcorr_forward: output row too wide"); return 1; }
  const int rows = 256 / strips > 0 ? 256 / strips : 1;
  dim3 block(strips, rows), grid((OH + rows - 1) / rows, B);
  hipStream_t st = (hipStream_t)stream;
  if (kw == 32) hipLaunchKernelGGL((k_xcorr_fwd<32, SW>), grid, block, 0, st, x, w, out, C, H, W, kh, OH, OW);
  else if (kw == 16) hipLaunchKernelGGL((k_xcorr_fwd<16, SW>), grid, block, 0, st, x, w, out, C, H, W, kh, OH, OW);
  else { snprintf(q_err, sizeof q_err, "srl_xcorr_forward: kw must be 16 or 32"); return 1; }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(q_err, sizeof q_err, "srl_xcorr_forward: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

int srl_policy_head(const float* adv, const float* u, const int64_t* rnd, float epsilon, int64_t* actions, int32_t B,
                    int32_t A, void* stream) {
  if (!adv || !u || !rnd || !actions || B < 1 || A < 1) {
    snprintf(q_err, sizeof q_err, "srl_policy_head: bad arguments");
    return 1;
  }
  hipLaunchKernelGGL(k_policy_head, dim3(B), dim3(256), 0, (hipStream_t)stream, adv, u, rnd, epsilon, actions, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(q_err, sizeof q_err, "srl_policy_head: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

int srl_boltzmann_head(const float* adv, const int64_t* keys, float temperature, int64_t* actions, int32_t B, int32_t A,
                       void* stream) {
  if (!adv || !keys || !actions || B < 1 || A < 1 || !(temperature > 0.0f)) {
    snprintf(q_err, sizeof q_err, "srl_boltzmann_head: bad arguments (pointers must be non-null, B >= 1, A >= 1, temperature > 0)");
    return 1;
  }
  hipLaunchKernelGGL(k_boltzmann_head, dim3(B), dim3(256), 0, (hipStream_t)stream, adv, keys, temperature, actions, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(q_err, sizeof q_err, "srl_boltzmann_head: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

}  // extern "C"
