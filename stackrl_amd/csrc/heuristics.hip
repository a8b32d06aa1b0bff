// heuristics.hip — the reference's heuristic baseline policies as device kernels (float64 like numpy).
//
// stackrl/baselines.py: `height` :28-43, `difference` :45-77, `corrcoef` :79-114, `correlate` :141-143,
// `goal_overlap` :152-156 and the selection of `Baseline.call` :201-217.  All of them are sliding-window reductions of
// the (h x w) object map over the (H x W) height map — (H-h+1)(W-w+1) windows of h*w taps — which the reference runs
// as double Python loops per observation.  Here: one 256-thread workgroup per env, the uint8 maps staged once in LDS
// (2 x 16 KB + 1 KB at 128 / 32; the host refuses a map that does not fit the device's LDS), a 256-entry table
// k -> k / gmax so that every tap value is the same double numpy computes, one thread per window (strided), float64
// accumulation in row-major tap order.  An env whose goal channel is all zero has gmax = 0 and, like the reference,
// gets NaN / inf values; the other envs of the batch are not touched by it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/stackrl_qnet.h"
#include "../../include/stackrl_baseline_rows.h"

__attribute__((visibility("hidden"))) void srl_qnet_set_error(const char* msg);   // qnet.hip: the text srl_qnet_last_error() returns (not exported)

namespace {
#define SET_ERR(...) do { char msg_[256]; snprintf(msg_, sizeof msg_, __VA_ARGS__); srl_qnet_set_error(msg_); } while (0)

// LDS of one workgroup: the three byte maps, then (8-byte aligned: H*H and h*h may be odd) the doubles, then the ints.
__host__ __device__ inline size_t lds_doubles_offset(int H, int h) { return (2 * (size_t)H * H + (size_t)h * h + 7) & ~(size_t)7; }
inline size_t lds_bytes(int H, int h) { return lds_doubles_offset(H, h) + sizeof(double) * (256 + (size_t)h * h + 256) + sizeof(int) * 256; }

enum { M_CORRELATE = 1, M_HEIGHT = 2, M_DIFFERENCE = 3, M_CORRCOEF = 4 };

__device__ __forceinline__ double ipow(double x, int e) {   // numpy: x**1 = x, x**2 = x*x; otherwise pow
  if (e == 1) return x;
  if (e == 2) return x * x;
  return pow(x, (double)e);
}

// One observation (overhead map m [H][H][2], object map o [h][h]) -> its value map and goal-overlap mask, [A] each: the
// whole arithmetic of a workgroup, shared by k_heuristic (one observation per env) and k_heuristic_rows (G object maps
// per env over one overhead map, include/stackrl_baseline_rows.h).
__device__ __forceinline__ void heuristic_observation(int method, const uint8_t* __restrict__ m, const uint8_t* __restrict__ o,
                                                      double* __restrict__ values, uint8_t* __restrict__ mask, int H, int h,
                                                      int dexp, int wexp, int localized, double threshold) {
  extern __shared__ unsigned char lds[];
  const int tid = threadIdx.x;
  const int OH = H - h + 1, A = OH * OH;
  uint8_t* sm = lds;                    // [H*H] height channel
  uint8_t* sg = sm + H * H;             // [H*H] (height < goal) flags
  uint8_t* so = sg + H * H;             // [h*h] object map
  double* lut = (double*)(lds + lds_doubles_offset(H, h));   // [256] k / gmax
  double* wts = lut + 256;              // [h*h] difference weights / centred n for corrcoef
  double* red = wts + h * h;            // [256] reductions
  int* redi = (int*)(red + 256);        // [256]
  int gl = 0;
  for (int k = tid; k < H * H; k += 256) {
    uint8_t hv = m[2 * k], gv = m[2 * k + 1];
    sm[k] = hv; sg[k] = hv < gv;
    gl = gl > gv ? gl : gv;
  }
  for (int k = tid; k < h * h; k += 256) so[k] = o[k];
  redi[tid] = gl;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) { if (tid < s) redi[tid] = redi[tid] > redi[tid + s] ? redi[tid] : redi[tid + s]; __syncthreads(); }
  const double gmax = (double)redi[0];                    // baselines.py:23
  __syncthreads();
  lut[tid] = (double)tid / gmax;
  __syncthreads();
  // ---- per-method constants of the object map
  double nsum = 0.0, ncount = 0.0, nmean = 0.0, nvar = 0.0, wsum = 0.0;
  if (method == M_DIFFERENCE) {
    double part = 0.0;
    for (int k = tid; k < h * h; k += 256) {
      int i = k / h, j = k - i * h;
      double w = 0.0;
      if (so[k] > 0) {
        if (wexp > 0) {
          double wi = ((double)i - h / 2.0), wj = ((double)j - h / 2.0);
          double r2 = wi * wi + wj * wj;
          w = wexp == 2 ? r2 : pow(r2, wexp / 2.0);          // (wi^2 + wj^2) ** (wexp / 2)
        } else w = 1.0;
      }
      wts[k] = w; part += w;
    }
    red[tid] = part; __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    wsum = red[0]; __syncthreads();
    for (int k = tid; k < h * h; k += 256) wts[k] = wts[k] / wsum;
    __syncthreads();
  } else if (method == M_CORRCOEF || method == M_CORRELATE) {
    double part = 0.0, cnt = 0.0;
    for (int k = tid; k < h * h; k += 256) {
      bool in = localized ? so[k] > 0 : true;
      if (method == M_CORRELATE) in = true;
      if (in) { part += lut[so[k]]; cnt += 1.0; }
    }
    red[tid] = part; __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    nsum = red[0]; __syncthreads();
    red[tid] = cnt; __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    ncount = red[0]; __syncthreads();
    if (method == M_CORRCOEF) {
      nmean = nsum / ncount;
      double pv = 0.0;
      for (int k = tid; k < h * h; k += 256) {
        bool in = localized ? so[k] > 0 : true;
        double c = lut[so[k]] - nmean;                       // n -= mean (baselines.py:94)
        wts[k] = c;
        if (in) pv += c * c;
      }
      red[tid] = pv; __syncthreads();
      for (int s = 128; s >= 1; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
      nvar = red[0]; __syncthreads();
    }
  }
  // ---- windows
  int fmax_local = 0;
  for (int a = tid; a < A; a += 256) {
    const int i = a / OH, j = a - i * OH;
    double f = 0.0;
    if (method == M_HEIGHT || method == M_DIFFERENCE) {
      double h0 = 0.0;                                       // np.max(np.where(n_where, o + n, 0))
      for (int p = 0; p < h; ++p)
        for (int q = 0; q < h; ++q) {
          uint8_t nv = so[p * h + q];
          if (nv > 0) { double s = lut[sm[(i + p) * H + j + q]] + lut[nv]; h0 = s > h0 ? s : h0; }
        }
      if (method == M_HEIGHT) f = h0;
      else {
        for (int p = 0; p < h; ++p)
          for (int q = 0; q < h; ++q) {
            double hh = lut[sm[(i + p) * H + j + q]] + lut[so[p * h + q]];
            f += wts[p * h + q] * ipow(fabs(h0 - hh), dexp);
          }
      }
    } else if (method == M_CORRELATE) {
      for (int p = 0; p < h; ++p)
        for (int q = 0; q < h; ++q) f += lut[sm[(i + p) * H + j + q]] * lut[so[p * h + q]];
      f = f / nsum;
    } else if (method == M_CORRCOEF) {
      if (nvar != 0.0) {
        double osum = 0.0;
        for (int p = 0; p < h; ++p)
          for (int q = 0; q < h; ++q)
            if (!localized || so[p * h + q] > 0) osum += lut[sm[(i + p) * H + j + q]];
        const double omean = osum / ncount;
        double ovar = 0.0, num = 0.0;
        for (int p = 0; p < h; ++p)
          for (int q = 0; q < h; ++q)
            if (!localized || so[p * h + q] > 0) {
              double c = lut[sm[(i + p) * H + j + q]] - omean;
              ovar += c * c; num += wts[p * h + q] * c;
            }
        if (ovar != 0.0) f = num / sqrt(nvar * ovar);
      }
    }
    values[a] = f;
    if (mask) {                                              // goal_overlap numerator (integers): running maximum
      int ov = 0;
      for (int p = 0; p < h; ++p)
        for (int q = 0; q < h; ++q) ov += (so[p * h + q] > 0) & sg[(i + p) * H + j + q];
      fmax_local = fmax_local > ov ? fmax_local : ov;
    }
  }
  if (!mask) return;
  __syncthreads();
  redi[tid] = fmax_local; __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) { if (tid < s) redi[tid] = redi[tid] > redi[tid + s] ? redi[tid] : redi[tid + s]; __syncthreads(); }
  const double thr = threshold * (double)redi[0];            // f >= threshold * f.max()  (baselines.py:156)
  for (int a = tid; a < A; a += 256) {
    const int i = a / OH, j = a - i * OH;
    int ov = 0;
    for (int p = 0; p < h; ++p)
      for (int q = 0; q < h; ++q) ov += (so[p * h + q] > 0) & sg[(i + p) * H + j + q];
    mask[a] = (double)ov >= thr ? 1 : 0;
  }
}

__global__ void __launch_bounds__(256)
k_heuristic(int method, const uint8_t* __restrict__ obs_map, const uint8_t* __restrict__ obs_obj,
            double* __restrict__ values, uint8_t* __restrict__ mask, int H, int h, int dexp, int wexp, int localized,
            double threshold) {
  const int b = blockIdx.x;
  const size_t A = (size_t)(H - h + 1) * (H - h + 1);
  heuristic_observation(method, obs_map + (size_t)b * H * H * 2, obs_obj + (size_t)b * h * h, values + b * A,
                        mask ? mask + b * A : nullptr, H, h, dexp, wexp, localized, threshold);
}

// Stack-v2: env blockIdx.y, object map blockIdx.x < n_valid of its G.  Every row of an env reads the env's one overhead map
// (so its goal maximum, its k / gmax table and its height < goal flags are the env's); rows >= n_valid have no workgroup.
__global__ void __launch_bounds__(256)
k_heuristic_rows(int method, const uint8_t* __restrict__ obs_map, const uint8_t* __restrict__ obs_obj,
                 double* __restrict__ values, uint8_t* __restrict__ mask, int G, int H, int h, int dexp, int wexp,
                 int localized, double threshold) {
  const int b = blockIdx.y;
  const size_t row = (size_t)b * G + blockIdx.x, A = (size_t)(H - h + 1) * (H - h + 1);
  heuristic_observation(method, obs_map + (size_t)b * H * H * 2, obs_obj + row * h * h, values + row * A,
                        mask ? mask + row * A : nullptr, H, h, dexp, wexp, localized, threshold);
}

// Baseline.call (baselines.py:201-217): goal mask, optional local-minimum filter (scipy minimum_filter, size
// 1 + 2 minorder, mode 'constant' -> 0 outside), arg-min with first-occurrence ties; also the negated value map.
// The rule for one value map v [A] (+ mask mk [A]): returns the action to every thread, writes the negated map to neg (may
// be NULL) and the largest masked value to *masked_max_out.  sv / si [256] and any_minima are the workgroup's LDS; they are
// free again when the function returns.  Shared by k_baseline_select and k_baseline_rows_select.
__device__ __forceinline__ int baseline_select_map(const double* __restrict__ v, const uint8_t* __restrict__ mk, int use_goal,
                                                   int minorder, double* __restrict__ neg, int OH, double* sv, int* si,
                                                   int* any_minima, double* masked_max_out) {
  const int tid = threadIdx.x, A = OH * OH;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  if (tid == 0) *any_minima = 0;
  __syncthreads();
  // pass 1: is there any masked local minimum?  and max of masked values (for the returned map)
  double vmax = -INF; int found = 0;
  for (int a = tid; a < A; a += 256) {
    if (use_goal && mk[a]) {
      vmax = v[a] > vmax ? v[a] : vmax;
      if (minorder > 0) {
        const int i = a / OH, j = a - i * OH;
        double mn = INF;
        for (int di = -minorder; di <= minorder; ++di)
          for (int dj = -minorder; dj <= minorder; ++dj) {
            const int ii = i + di, jj = j + dj;
            const double t = (ii >= 0 && ii < OH && jj >= 0 && jj < OH) ? v[ii * OH + jj] : 0.0;
            mn = t < mn ? t : mn;
          }
        if (mn == v[a]) found = 1;
      }
    }
  }
  if (found) atomicOr(any_minima, 1);
  sv[tid] = vmax; __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) { if (tid < s) sv[tid] = sv[tid] > sv[tid + s] ? sv[tid] : sv[tid + s]; __syncthreads(); }
  const double masked_max = sv[0];
  const bool use_minima = use_goal && minorder > 0 && *any_minima;
  __syncthreads();
  // pass 2: arg-min over the candidate set
  double best = INF; int bi = 0x7fffffff;
  for (int a = tid; a < A; a += 256) {
    bool cand = true;
    if (use_goal) {
      cand = mk[a];
      if (cand && use_minima) {
        const int i = a / OH, j = a - i * OH;
        double mn = INF;
        for (int di = -minorder; di <= minorder; ++di)
          for (int dj = -minorder; dj <= minorder; ++dj) {
            const int ii = i + di, jj = j + dj;
            const double t = (ii >= 0 && ii < OH && jj >= 0 && jj < OH) ? v[ii * OH + jj] : 0.0;
            mn = t < mn ? t : mn;
          }
        cand = (mn == v[a]);
      }
    }
    const double t = cand ? v[a] : INF;
    if (t < best || (t == best && a < bi)) { best = t; bi = a; }
    if (neg) neg[a] = use_goal ? -(mk[a] ? v[a] : masked_max + 0.001) : -v[a];
  }
  sv[tid] = best; si[tid] = bi; __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s && (sv[tid + s] < sv[tid] || (sv[tid + s] == sv[tid] && si[tid + s] < si[tid]))) { sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; }
    __syncthreads();
  }
  const int action = si[0] == 0x7fffffff ? 0 : si[0];   // np.argmin of an all-inf array is 0
  *masked_max_out = masked_max;
  __syncthreads();
  return action;
}

// Baseline.call (baselines.py:201-217): goal mask, optional local-minimum filter (scipy minimum_filter, size
// 1 + 2 minorder, mode 'constant' -> 0 outside), arg-min with first-occurrence ties; also the negated value map.
__global__ void __launch_bounds__(256)
k_baseline_select(const double* __restrict__ values, const uint8_t* __restrict__ mask, int use_goal, int minorder,
                  int64_t* __restrict__ actions, double* __restrict__ neg_values, int OH) {
  __shared__ double sv[256];
  __shared__ int si[256];
  __shared__ int any_minima;
  const size_t b = blockIdx.x, A = (size_t)OH * OH;
  double masked_max;
  const int action = baseline_select_map(values + b * A, mask + b * A, use_goal, minorder, neg_values ? neg_values + b * A : nullptr,
                                         OH, sv, si, &any_minima, &masked_max);
  if (threadIdx.x == 0) actions[b] = (int64_t)action;
}

// The batch-wise choice of PyGreedy.__call__ (agents/policies.py:57-91) over the rows of one env, one workgroup per env:
// row after row the rule above, c_r = the negated map at the row's action, and the first row with the largest c_r.  Every
// thread holds the same running best (all of them read the row's result from LDS), so the choice is a fixed-order scan.
__global__ void __launch_bounds__(256)
k_baseline_rows_select(const double* __restrict__ values, const uint8_t* __restrict__ mask, int use_goal, int minorder, int G,
                       int n_valid, int OH, int64_t* __restrict__ actions, double* __restrict__ chosen,
                       double* __restrict__ neg_values) {
  __shared__ double sv[256];
  __shared__ int si[256];
  __shared__ int any_minima;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x, A = (size_t)OH * OH;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  double best_c = -INF; int best_r = 0, best_a = 0;
  for (int r = 0; r < n_valid; ++r) {
    const size_t row = b * G + r;
    const double* v = values + row * A;
    const uint8_t* mk = mask + row * A;
    double masked_max;
    const int a = baseline_select_map(v, mk, use_goal, minorder, neg_values ? neg_values + row * A : nullptr, OH, sv, si,
                                      &any_minima, &masked_max);
    const double c = use_goal ? -(mk[a] ? v[a] : masked_max + 0.001) : -v[a];   // the negated map at a
    if (tid == 0 && chosen) chosen[row] = c;
    if (r == 0 || c > best_c) { best_c = c; best_r = r; best_a = a; }
  }
  if (tid == 0) actions[b] = (int64_t)best_r * (int64_t)A + best_a;
  for (int r = n_valid; r < G; ++r) {     // rows without a rock: never read, -inf in what is returned
    const size_t row = b * G + r;
    if (tid == 0 && chosen) chosen[row] = -INF;
    if (neg_values)
      for (size_t a = tid; a < A; a += 256) neg_values[row * A + a] = -INF;
  }
}

}  // namespace

extern "C" {

int srl_heuristic(int32_t method, const uint8_t* obs_map, const uint8_t* obs_obj, double* values, uint8_t* mask,
                  int32_t B, int32_t H, int32_t h, int32_t difference_exponent, int32_t weights_exponent,
                  int32_t localized, double threshold, void* stream) {
  if (!obs_map || !obs_obj || !values || B < 1 || h < 1 || H < h || method < 1 || method > 4) {
    SET_ERR("srl_heuristic: bad arguments");
    return 1;
  }
  const size_t lds = lds_bytes(H, h);
  int dev = 0, lds_max = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) { SET_ERR("srl_heuristic: %s", hipGetErrorString(e)); return 4; }
  if (lds > (size_t)lds_max) {      // the whole map of one env is staged in LDS: nothing is launched when it cannot be
    SET_ERR("srl_heuristic: H = %d, h = %d needs %zu bytes of LDS per workgroup, the device has %d", (int)H, (int)h, lds, lds_max);
    return 1;
  }
  e = hipFuncSetAttribute((const void*)k_heuristic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    SET_ERR("srl_heuristic: H = %d, h = %d, %zu bytes of LDS: %s", (int)H, (int)h, lds, hipGetErrorString(e));
    return 4;
  }
  hipLaunchKernelGGL(k_heuristic, dim3(B), dim3(256), lds, (hipStream_t)stream, method, obs_map, obs_obj, values, mask,
                     H, h, difference_exponent, weights_exponent, localized, threshold);
  e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_heuristic: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

int srl_heuristic_rows(int32_t method, const uint8_t* obs_map, const uint8_t* obs_obj, double* values, uint8_t* mask,
                       int32_t B, int32_t G, int32_t n_valid, int32_t H, int32_t h, int32_t difference_exponent,
                       int32_t weights_exponent, int32_t localized, double threshold, void* stream) {
  if (!obs_map || !obs_obj || !values || B < 1 || B > 65535 || G < 1 || n_valid < 1 || n_valid > G || h < 1 || H < h ||
      method < 1 || method > 4) {
    SET_ERR("srl_heuristic_rows: bad arguments (B = %d of 1..65535, G = %d, n_valid = %d of 1..G, H = %d, h = %d, method = %d)",
            (int)B, (int)G, (int)n_valid, (int)H, (int)h, (int)method);
    return 1;
  }
  const size_t lds = lds_bytes(H, h);
  int dev = 0, lds_max = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) { SET_ERR("srl_heuristic_rows: %s", hipGetErrorString(e)); return 4; }
  if (lds > (size_t)lds_max) {      // as srl_heuristic: nothing is launched when one env's maps cannot be staged
    SET_ERR("srl_heuristic_rows: H = %d, h = %d needs %zu bytes of LDS per workgroup, the device has %d", (int)H, (int)h, lds, lds_max);
    return 1;
  }
  e = hipFuncSetAttribute((const void*)k_heuristic_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    SET_ERR("srl_heuristic_rows: H = %d, h = %d, %zu bytes of LDS: %s", (int)H, (int)h, lds, hipGetErrorString(e));
    return 4;
  }
  hipLaunchKernelGGL(k_heuristic_rows, dim3(n_valid, B), dim3(256), lds, (hipStream_t)stream, method, obs_map, obs_obj, values,
                     mask, G, H, h, difference_exponent, weights_exponent, localized, threshold);
  e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_heuristic_rows: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

int srl_baseline_select(const double* values, const uint8_t* mask, int32_t use_goal, int32_t minorder,
                        int64_t* actions, double* neg_values, int32_t B, int32_t OH, void* stream) {
  if (!values || !actions || (use_goal && !mask) || B < 1 || OH < 1 || minorder < 0) {
    SET_ERR("srl_baseline_select: bad arguments");
    return 1;
  }
  hipLaunchKernelGGL(k_baseline_select, dim3(B), dim3(256), 0, (hipStream_t)stream, values, mask ? mask : (const uint8_t*)values,
                     use_goal, minorder, actions, neg_values, OH);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_baseline_select: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

int srl_baseline_rows_select(const double* values, const uint8_t* mask, int32_t use_goal, int32_t minorder, int32_t B,
                             int32_t G, int32_t n_valid, int32_t OH, int64_t* actions, double* chosen, double* neg_values,
                             void* stream) {
  if (!values || !actions || (use_goal && !mask) || B < 1 || G < 1 || n_valid < 1 || n_valid > G || OH < 1 || OH > 32768 ||
      minorder < 0) {
    SET_ERR("srl_baseline_rows_select: bad arguments (B = %d, G = %d, n_valid = %d of 1..G, OH = %d, minorder = %d)", (int)B,
            (int)G, (int)n_valid, (int)OH, (int)minorder);
    return 1;
  }
  hipLaunchKernelGGL(k_baseline_rows_select, dim3(B), dim3(256), 0, (hipStream_t)stream, values,
                     mask ? mask : (const uint8_t*)values, use_goal, minorder, G, n_valid, OH, actions, chosen, neg_values);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_baseline_rows_select: %s", hipGetErrorString(e)); return 4; }
  return 0;
}

}  // extern "C"
