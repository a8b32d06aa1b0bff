// greedy.hip — the greedy head of the rollout path (include/stackrl_greedy.h), gfx950.
//
// One workgroup of 256 threads (four wave64) per env.  Per valid row two passes: the float64 sum of the row (the dueling
// mean), then q = (adv - mean) + v with the running (value, flat index) pair, the minimum and the float64 sums of q and
// q^2; the second pass of a row (37 KB at A = 9,409) comes from cache.  A thread walks its elements in ascending flat
// index and takes a new best only on a strict >, so it holds the lowest index of its maxima; the workgroup then reduces
// (value, index) with ties to the lower index.  Every reduction has a fixed order — a shuffle tree inside each wave, the
// four wave results added in wave order — no atomics, no cross-workgroup reduction: an env's
// results do not depend on the batch it is evaluated in.  Rows of a multiple of four floats at 16-byte aligned addresses
// are read (and q written) as float4.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/stackrl_greedy.h"

__attribute__((visibility("hidden"))) void srl_qnet_set_error(const char* msg);   // qnet.hip: the text srl_qnet_last_error() returns (not exported)

namespace {
#define SET_ERR(...) do { char msg_[256]; snprintf(msg_, sizeof msg_, __VA_ARGS__); srl_qnet_set_error(msg_); } while (0)

constexpr int NO_INDEX = 0x7fffffff;     // loses a tie to every real index

// sum over the workgroup, the same value in every thread: lanes pairwise at distance 32, 16, ..., 1, then the waves in order
__device__ __forceinline__ double block_sum_f64(double x, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o);
  __syncthreads();                                   // the previous sum has been read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

struct Run {                 // what a thread carries over the rows of its env
  float best; int bi; float mn; double s1, s2;
  __device__ __forceinline__ void take(float q, int idx) {
    if (q > best) { best = q; bi = idx; }            // NaN: false
    if (q < mn) mn = q;
    const double d = (double)q;
    s1 += d; s2 += d * d;
  }
};

template <bool VEC>
__global__ void __launch_bounds__(256) k_greedy_head(const float* __restrict__ adv, const float* __restrict__ v, int G,
                                                     int n_valid, int A, int64_t* __restrict__ actions,
                                                     double* __restrict__ stats, float* __restrict__ qout) {
  __shared__ double red[4];
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ float sm[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* ab = adv + (size_t)b * G * A;
  float* qb = qout ? qout + (size_t)b * G * A : nullptr;
  const bool dueling = v != nullptr;
  const float vb = dueling ? v[b] : 0.0f;
  const int quads = A >> 2;                          // VEC: A is a multiple of 4
  Run run = {-INFINITY, NO_INDEX, INFINITY, 0.0, 0.0};
  for (int r = 0; r < n_valid; ++r) {
    const float* a = ab + (size_t)r * A;
    float m = 0.0f;
    if (dueling) {
      double s = 0.0;
      if (VEC) {
        const float4* a4 = reinterpret_cast<const float4*>(a);
        for (int j = tid; j < quads; j += 256) {
          const float4 t = a4[j];
          s += (double)t.x; s += (double)t.y; s += (double)t.z; s += (double)t.w;
        }
      } else {
        for (int k = tid; k < A; k += 256) s += (double)a[k];
      }
      m = (float)(block_sum_f64(s, red) / (double)A);
    }
    const int base = r * A;
    if (VEC) {
      const float4* a4 = reinterpret_cast<const float4*>(a);
      float4* q4 = qb ? reinterpret_cast<float4*>(qb + (size_t)r * A) : nullptr;
      for (int j = tid; j < quads; j += 256) {
        float4 t = a4[j];
        if (dueling) { t.x = (t.x - m) + vb; t.y = (t.y - m) + vb; t.z = (t.z - m) + vb; t.w = (t.w - m) + vb; }
        run.take(t.x, base + 4 * j); run.take(t.y, base + 4 * j + 1); run.take(t.z, base + 4 * j + 2); run.take(t.w, base + 4 * j + 3);
        if (q4) q4[j] = t;
      }
    } else {
      for (int k = tid; k < A; k += 256) {
        float t = a[k];
        if (dueling) t = (t - m) + vb;
        run.take(t, base + k);
        if (qb) qb[(size_t)r * A + k] = t;
      }
    }
  }
  if (qb) {                                          // rows without a rock: -inf, never read
    float* tail = qb + (size_t)n_valid * A;
    const size_t n = (size_t)(G - n_valid) * A;
    for (size_t k = tid; k < n; k += 256) tail[k] = -INFINITY;
  }
  sv[tid] = run.best; si[tid] = run.bi; sm[tid] = run.mn;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) {
      const float ov = sv[tid + s]; const int oi = si[tid + s];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
      const float om = sm[tid + s];
      if (om < sm[tid]) sm[tid] = om;
    }
    __syncthreads();
  }
  const double s1 = block_sum_f64(run.s1, red);
  const double s2 = block_sum_f64(run.s2, red);
  if (tid == 0) {
    actions[b] = si[0] == NO_INDEX ? (int64_t)0 : (int64_t)si[0];     // nothing won: 0
    if (stats) {
      double* st = stats + 4 * (size_t)b;
      st[0] = (double)sv[0]; st[1] = (double)sm[0]; st[2] = s1; st[3] = s2;
    }
  }
}
}  // namespace

extern "C" {

int srl_greedy_head(const float* adv, const float* v, int32_t B, int32_t G, int32_t n_valid, int32_t A, int64_t* actions,
                    double* stats, float* q, void* stream) {
  if (!adv || !actions || B < 1 || G < 1 || A < 1 || n_valid < 1 || n_valid > G || (int64_t)G * A > 0x7ffffffeLL) {
    SET_ERR("srl_greedy_head: bad arguments (adv and actions must be non-null, B >= 1, G >= 1, A >= 1, 1 <= n_valid <= G, "
            "G * A < 2^31 - 1)");
    return 1;
  }
  const bool vec = A % 4 == 0 && (uintptr_t)adv % 16 == 0 && (uintptr_t)q % 16 == 0;
  if (vec) hipLaunchKernelGGL(k_greedy_head<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, adv, v, G, n_valid, A, actions, stats, q);
  else hipLaunchKernelGGL(k_greedy_head<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, adv, v, G, n_valid, A, actions, stats, q);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_greedy_head: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

}  // extern "C"
