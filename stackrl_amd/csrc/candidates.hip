// libstackrl_candidates.so — the candidates of a lookahead, spread by greedy non-maximum suppression (include/
// stackrl_candidates.h holds the definition; tests/candidates_cases.py restates it in numpy).  One kernel, one path:
//   k_candidates  one workgroup of 1,024 threads per env.  The order of the definition is a total order on (rank key, index):
//                 the rank key is the value's bits made monotone (NaN the largest key, -0 the key of +0), compared as an
//                 unsigned integer of the value's own width, so float64 is never narrowed.  A thread owns the entries
//                 tid, tid + 1024, ... of the considered maps and holds the best of them that no pick suppresses.  A round
//                 reduces the held bests — a butterfly over the wave, the sixteen waves through LDS, every thread reading all
//                 sixteen in the same order — to the next pick, and a thread reads its entries again only if that pick struck
//                 the entry it held.  The values are read where they lie: the first pass streams them once, coalesced, and
//                 what is read again comes from L2.  The picks live in LDS; the suppression test (an integer division and a
//                 few compares per pick) is made only for an entry that beats the best found so far.  No atomics: the
//                 result does not depend on the order of anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/stackrl_candidates.h"

namespace {

thread_local char c_err[256] = "";
#define SET_ERR(...) snprintf(c_err, sizeof c_err, __VA_ARGS__)

constexpr int MAXK = SRL_CANDIDATES_MAX_K;
constexpr int THREADS = SRL_CANDIDATES_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr uint32_t NONE = 0xffffffffu;      // the index of "no entry"; its key is 0, below the key of every value

// Larger key = earlier in the order.  Non-NaN values give keys in 0x007fffff.. (-inf) to 0xff800000.. (+inf).
__device__ __forceinline__ uint32_t rank_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if ((u << 1) == 0) u = 0;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t rank_key(double v) {
  uint64_t u = (uint64_t)__double_as_longlong(v);
  if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;
  if ((u << 1) == 0) u = 0;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

template <typename K>
__device__ __forceinline__ bool before(K ka, uint32_t ia, K kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia < ib);
}

struct Picks {
  int64_t flat[MAXK];
  int32_t g[MAXK], y[MAXK], x[MAXK];
};

template <typename T, typename K>
__global__ __launch_bounds__(THREADS) void k_candidates(const T* __restrict__ values, const int64_t* __restrict__ action,
                                                        uint32_t GA, uint32_t A, uint32_t OH, uint32_t N, int32_t k,
                                                        int32_t radius, int64_t* __restrict__ cand, int32_t* __restrict__ count) {
  __shared__ Picks picks;
  __shared__ K red_key[WAVES];
  __shared__ uint32_t red_idx[WAVES];
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const T* v = values + (size_t)b * GA;       // entries 0..N-1 of this env are read, N <= GA

  auto place = [&](uint32_t i, int32_t* g, int32_t* y, int32_t* x) {
    const uint32_t gg = i / A, rem = i - gg * A, yy = rem / OH;
    *g = (int32_t)gg; *y = (int32_t)yy; *x = (int32_t)(rem - yy * OH);
  };
  auto near = [&](int32_t a, int32_t c) { return (a > c ? a - c : c - a) <= radius; };
  auto record = [&](int n, uint32_t i) {
    picks.flat[n] = (int64_t)i;
    place(i, &picks.g[n], &picks.y[n], &picks.x[n]);
  };

  K held_key;
  uint32_t held_idx;
  // the best of this thread's entries that none of the picks 0..n-1 suppresses
  auto scan = [&](int n) {
    held_key = 0; held_idx = NONE;
    auto consider = [&](T value, uint32_t i) {
      const K key = rank_key(value);
      if (key > held_key) {                    // i rises, so an equal key never takes over
        int32_t g, y, x;
        place(i, &g, &y, &x);
        bool struck = false;
        for (int c = 0; c < n; ++c) struck |= picks.g[c] == g && near(picks.y[c], y) && near(picks.x[c], x);
        if (!struck) { held_key = key; held_idx = i; }
      }
    };
    uint32_t i = tid;
    for (; i < N && N - i > 3u * THREADS; i += 4u * THREADS) {       // four loads in flight
      const T v0 = v[i], v1 = v[i + THREADS], v2 = v[i + 2u * THREADS], v3 = v[i + 3u * THREADS];
      consider(v0, i); consider(v1, i + THREADS); consider(v2, i + 2u * THREADS); consider(v3, i + 3u * THREADS);
    }
    for (; i < N; i += THREADS) consider(v[i], i);
  };

  int n = 0;
  if (action) {
    const int64_t a = action[b];
    if (tid == 0) record(0, (uint32_t)(a < 0 ? 0 : (a > (int64_t)GA - 1 ? (int64_t)GA - 1 : a)));
    n = 1;
    __syncthreads();
  }
  scan(n);
  while (n < k) {
    K key = held_key;
    uint32_t idx = held_idx;
    for (int off = 32; off >= 1; off >>= 1) {
      const K ok = __shfl_xor(key, off);
      const uint32_t oi = __shfl_xor(idx, off);
      if (before(ok, oi, key, idx)) { key = ok; idx = oi; }
    }
    if ((tid & 63) == 0) { red_key[tid >> 6] = key; red_idx[tid >> 6] = idx; }
    __syncthreads();
    key = red_key[0]; idx = red_idx[0];
    for (int w = 1; w < WAVES; ++w)
      if (before(red_key[w], red_idx[w], key, idx)) { key = red_key[w]; idx = red_idx[w]; }
    if (idx == NONE) break;                    // every considered entry is chosen or struck (the same in every thread)
    if (tid == 0) record(n, idx);
    ++n;
    __syncthreads();                           // the pick is in LDS, and red_* may be written again
    if (n == k) break;
    if (held_idx != NONE) {
      int32_t pg, py, px, g, y, x;
      place(idx, &pg, &py, &px);
      place(held_idx, &g, &y, &x);
      if (pg == g && near(py, y) && near(px, x)) scan(n);
    }
  }
  __syncthreads();
  if (tid < (uint32_t)k) cand[(size_t)b * k + tid] = picks.flat[tid < (uint32_t)n ? tid : 0];
  if (tid == 0) count[b] = n;
}

}  // namespace

extern "C" {

const char* srl_candidates_last_error(void) { return c_err; }

#ifndef SRL_BUILD_INFO
#define SRL_BUILD_INFO "SRL_BUILD_INFO<unknown|>"
#endif
const char* srl_candidates_build_info(void) { static const char info[] = SRL_BUILD_INFO; return info; }

int srl_candidates_select(const void* values, int32_t f64, const int64_t* action, int32_t B, int32_t G, int32_t OH,
                          int32_t n_valid, int32_t k, int32_t radius, int64_t* cand, int32_t* count, void* stream) {
  if (B < 1) { SET_ERR("srl_candidates_select: B must be at least 1, got %d", B); return SRL_EINVAL; }
  if (G < 1) { SET_ERR("srl_candidates_select: G must be at least 1, got %d", G); return SRL_EINVAL; }
  if (OH < 1) { SET_ERR("srl_candidates_select: OH must be at least 1, got %d", OH); return SRL_EINVAL; }
  const int64_t A = (int64_t)OH * OH;
  if (A > (int64_t)INT32_MAX - 1 || (int64_t)G * A > (int64_t)INT32_MAX - 1) {
    SET_ERR("srl_candidates_select: G * A must be at most 2^31-2, got %d * %lld", G, (long long)A);
    return SRL_EINVAL;
  }
  if (n_valid < 1 || n_valid > G) { SET_ERR("srl_candidates_select: n_valid must be in 1..%d, got %d", G, n_valid); return SRL_EINVAL; }
  if (k < 1 || k > MAXK) { SET_ERR("srl_candidates_select: k must be in 1..%d, got %d", MAXK, k); return SRL_EINVAL; }
  if (radius < 0) { SET_ERR("srl_candidates_select: radius must be at least 0, got %d", radius); return SRL_EINVAL; }
  if (!values || !cand || !count) {
    SET_ERR("srl_candidates_select: a required pointer is null (values %d, cand %d, count %d)", values != nullptr, cand != nullptr,
            count != nullptr);
    return SRL_EINVAL;
  }
  const uint32_t GA = (uint32_t)(G * A), N = (uint32_t)(n_valid * A);
  if (f64)
    hipLaunchKernelGGL((k_candidates<double, uint64_t>), dim3(B), dim3(THREADS), 0, (hipStream_t)stream, (const double*)values,
                       action, GA, (uint32_t)A, (uint32_t)OH, N, k, radius, cand, count);
  else
    hipLaunchKernelGGL((k_candidates<float, uint32_t>), dim3(B), dim3(THREADS), 0, (hipStream_t)stream, (const float*)values,
                       action, GA, (uint32_t)A, (uint32_t)OH, N, k, radius, cand, count);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_candidates_select: %s", hipGetErrorString(e)); return SRL_EHIP; }
  return SRL_OK;
}

}  // extern "C"
