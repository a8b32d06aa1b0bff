// compare.hip — the statistics that compare the value maps of several policies (include/stackrl_compare.h), gfx950.
//
// k_compare<P>: one workgroup of 256 threads (four wave64) per env.  The P maps of an env (P * 37 KB at A = 9,409: 301 KB at
// P = 8, more than the LDS holds) are swept three times, the second and third time from cache: the float64 sums and the
// float32 maxima (-> mu), the centred squares (-> sigma), then the products and the flags.  A thread keeps NP = P (P + 1) / 2
// float64 products; the flags of a wave's 64 actions become one 64-bit mask per policy (a ballot), so a pair's
// intersection count is the population count of the and of two masks, the same number in every lane, and needs no reduction
// inside the wave; the union is |a| + |b| - |a and b| of those exact integers.
// Every float64 sum is reduced by a shuffle tree inside each wave and the four wave results are added in wave order.  The
// workgroup writes its env's partial record; k_fold (one workgroup) adds the partials of a step onto the running record in
// env order.  No atomics: the record does not depend on anything but the inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/stackrl_compare.h"

namespace {
thread_local char c_err[256] = "";
#define SET_ERR(...) snprintf(c_err, sizeof c_err, __VA_ARGS__)

constexpr int MAXP = SRL_COMPARE_MAX_POLICIES;
constexpr int pairs(int P) { return P * (P + 1) / 2; }
constexpr int record_doubles(int P) { return 1 + P + 5 * pairs(P); }

struct Maps { const void* p[MAXP]; };

__device__ __forceinline__ float load_f32(const void* p, bool f64, int k) {
  return f64 ? (float)static_cast<const double*>(p)[k] : static_cast<const float*>(p)[k];
}

// lanes pairwise at distance 32, 16, ..., 1: lane 0 holds the wave's sum
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o);
  return x;
}

template <int P>
__global__ void __launch_bounds__(256) k_compare(Maps maps, int f64_mask, int G, int A, const int64_t* __restrict__ actions,
                                                 float* __restrict__ amax, double* __restrict__ partial) {
  constexpr int NP = pairs(P), R = record_doubles(P);
  constexpr int O_S = 1 + P, O_I1 = O_S + NP, O_U1 = O_I1 + NP, O_I2 = O_U1 + NP, O_U2 = O_I2 + NP;
  __shared__ double red[4][R];
  __shared__ float redm[4][P];
  __shared__ int redn[4][P];
  const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const void* base[P];
  bool f64[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    f64[j] = (f64_mask >> j) & 1;
    int64_t row = 0;
    if (actions) {
      row = actions[(size_t)j * B + b] / A;
      row = row < 0 ? 0 : (row > G - 1 ? G - 1 : row);
    }
    const size_t off = ((size_t)b * G + (size_t)row) * A;
    base[j] = f64[j] ? static_cast<const void*>(static_cast<const double*>(maps.p[j]) + off)
                     : static_cast<const void*>(static_cast<const float*>(maps.p[j]) + off);
  }
  // sweep 1: sums and maxima
  double s[P];
  {
    float mx[P];
    int nan[P];
#pragma unroll
    for (int j = 0; j < P; ++j) { s[j] = 0.0; mx[j] = -INFINITY; nan[j] = 0; }
#pragma unroll 4
    for (int k = tid; k < A; k += 256) {             // four iterations' loads in flight; the adds keep their order
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const float x = load_f32(base[j], f64[j], k);
        s[j] += (double)x;
        if (x > mx[j]) mx[j] = x;
        nan[j] |= x != x;
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      s[j] = wave_sum_f64(s[j]);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float om = __shfl_down(mx[j], o);
        if (om > mx[j]) mx[j] = om;
        nan[j] |= __shfl_down(nan[j], o);
      }
      if (lane == 0) { red[wave][j] = s[j]; redm[wave][j] = mx[j]; redn[wave][j] = nan[j]; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P; ++j) s[j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    if (tid < P) {
      float m = redm[0][tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) if (redm[w][tid] > m) m = redm[w][tid];
      const int n = redn[0][tid] | redn[1][tid] | redn[2][tid] | redn[3][tid];
      amax[(size_t)tid * B + b] = n ? __builtin_nanf("") : m;
    }
    __syncthreads();                                 // red is written again below
  }
  double mu[P], t2[P];
#pragma unroll
  for (int j = 0; j < P; ++j) mu[j] = s[j] / (double)A;
  // sweep 2: centred squares
  {
    double q[P];
#pragma unroll
    for (int j = 0; j < P; ++j) q[j] = 0.0;
#pragma unroll 4
    for (int k = tid; k < A; k += 256) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const double d = (double)load_f32(base[j], f64[j], k) - mu[j];
        q[j] += d * d;
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      q[j] = wave_sum_f64(q[j]);
      if (lane == 0) red[wave][j] = q[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P; ++j) t2[j] = mu[j] + sqrt(((red[0][j] + red[1][j]) + (red[2][j] + red[3][j])) / (double)A);
    __syncthreads();
  }
  // sweep 3: products and flags.  The trip count is the same in every thread (the ballots need the whole wave).
  double S[NP];
  int cI1[NP], cI2[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) { S[p] = 0.0; cI1[p] = cI2[p] = 0; }
#pragma unroll 2
  for (int k0 = 0; k0 < A; k0 += 256) {
    const int k = k0 + tid;
    const bool act = k < A;
    double x[P];
    unsigned long long m1[P], m2[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      x[j] = act ? (double)load_f32(base[j], f64[j], k) : 0.0;
      m1[j] = __ballot(act && x[j] > mu[j]);
      m2[j] = __ballot(act && x[j] > t2[j]);
    }
    int p = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
      for (int j = i; j < P; ++j, ++p) {
        if (act) S[p] += x[i] * x[j];
        cI1[p] += __popcll(m1[i] & m1[j]);
        cI2[p] += __popcll(m2[i] & m2[j]);
      }
    }
  }
  {
    int p = 0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
#pragma unroll
      for (int j = i; j < P; ++j, ++p) {
        S[p] = wave_sum_f64(S[p]);
        if (lane == 0) {                             // |a or b| = |a| + |b| - |a and b|; the pair (i, i) counts flag i
          const int pi = i * P - i * (i - 1) / 2, pj = j * P - j * (j - 1) / 2;
          red[wave][O_S + p] = S[p];
          red[wave][O_I1 + p] = (double)cI1[p];
          red[wave][O_U1 + p] = (double)(cI1[pi] + cI1[pj] - cI1[p]);
          red[wave][O_I2 + p] = (double)cI2[p];
          red[wave][O_U2 + p] = (double)(cI2[pi] + cI2[pj] - cI2[p]);
        }
      }
    }
  }
  if (lane == 0) {                                   // the env itself and its sums: wave 0 holds them, the others add zero
    red[wave][0] = wave == 0 ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < P; ++j) red[wave][1 + j] = wave == 0 ? s[j] : 0.0;
  }
  __syncthreads();
  if (tid < R) partial[(size_t)b * R + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// record[r] += partial[0][r] + partial[1][r] + ... in env order
__global__ void __launch_bounds__(256) k_fold(const double* __restrict__ partial, double* __restrict__ record, int B, int R) {
  const int r = threadIdx.x;
  if (r >= R) return;
  double acc = record[r];
  int b = 0;
  for (; b + 16 <= B; b += 16) {                     // sixteen loads in flight, then their adds in env order
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = partial[(size_t)(b + u) * R + r];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += v[u];
  }
  for (; b < B; ++b) acc += partial[(size_t)b * R + r];
  record[r] = acc;
}

template <int P>
void launch(const Maps& maps, int f64_mask, int B, int G, int A, const int64_t* actions, float* amax, double* partial,
            hipStream_t stream) {
  hipLaunchKernelGGL(k_compare<P>, dim3(B), dim3(256), 0, stream, maps, f64_mask, G, A, actions, amax, partial);
}
}  // namespace

extern "C" {

const char* srl_compare_last_error(void) { return c_err; }

#ifndef SRL_BUILD_INFO
#define SRL_BUILD_INFO "SRL_BUILD_INFO<unknown|>"
#endif
const char* srl_compare_build_info(void) { static const char info[] = SRL_BUILD_INFO; return info; }

int32_t srl_compare_record_doubles(int32_t P) { return P >= 1 && P <= MAXP ? record_doubles(P) : 0; }

int srl_compare_step(int32_t P, const void* map0, const void* map1, const void* map2, const void* map3, const void* map4,
                     const void* map5, const void* map6, const void* map7, int32_t f64_mask, int32_t B, int32_t G, int32_t A,
                     const int64_t* actions, float* amax, double* partial, double* record, void* stream) {
  const Maps maps = {{map0, map1, map2, map3, map4, map5, map6, map7}};
  bool ok = P >= 1 && P <= MAXP && B >= 1 && G >= 1 && A >= 1 && (int64_t)G * A <= 0x7ffffffeLL && amax && partial && record;
  for (int j = 0; ok && j < P; ++j) ok = maps.p[j] != nullptr;
  if (!ok) {
    SET_ERR("srl_compare_step: bad arguments (1 <= P <= 8, B >= 1, G >= 1, A >= 1, G * A < 2^31 - 1, the first P maps, amax, "
            "partial and record must be non-null)");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  switch (P) {
    case 1: launch<1>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    case 2: launch<2>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    case 3: launch<3>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    case 4: launch<4>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    case 5: launch<5>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    case 6: launch<6>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    case 7: launch<7>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
    default: launch<8>(maps, f64_mask, B, G, A, actions, amax, partial, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_compare_step: %s", hipGetErrorString(e)); return 4; }
  hipLaunchKernelGGL(k_fold, dim3(1), dim3(256), 0, st, partial, record, B, record_doubles(P));
  e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_compare_step: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

}  // extern "C"
