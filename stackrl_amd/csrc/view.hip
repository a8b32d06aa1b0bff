// view.hip — `StackEnv.render('rgb_array')` (env.py:295-332; `TestStackEnv.render`, :558-596) for a batch, on the device.
//
// The reference colours its two elevation maps by height: for a float32 map m (the overhead map, or the pending rock's)
//   R = m / max(m), or m where the max is 0   (float32 by float32: a float32, env.py:300-301)
//   B = 1 - R                                 (float32)
//   G = 0.5, and 0.5 + 0.1 inside the goal rectangle rows u .. u + h, columns v .. v + w (`Rewarder.goal_bin`,
//       rewarder.py:255-259; float64: `np.ones`); the object view has no goal
// stacked as float64 [.., 3].  srl_k_view is that function of exactly the arrays srl_get_maps hands out — DevParams::H, the
// object map of the rock on show in orientation 0 (the first rock still unplaced with ordering freedom, `n[0]` of
// env.py:563; the empty-map constant when there is none) and EnvHdr::goal — read where srl_k_render left them.
//
// One workgroup of 256 threads per env, two phases:
//   max     np.max of both maps: 128-bit loads, a running max per thread, the wave by shuffles, the four waves through
//           LDS.  A max does not depend on the order it is taken in.
//   colour  the maps again (64 KB an env: they are in the L2) and the images out.  A thread owns a run of consecutive
//           pixels whose channels fill whole 128-bit stores: 4 pixels of float64 RGB are 96 contiguous bytes (6 stores), 16
//           pixels of uint8 RGB 48 (3 stores); a wave's stores of one round together cover one contiguous span.
// Maps whose pixel count is no multiple of the run, or images that are not 16-byte aligned, take the pixel-by-pixel path.
// The division is the correctly rounded one (the library is built without fast-math) and nothing is contracted
// (-ffp-contract=off), so every value has the bits numpy gives.  uint8 frames: x * 255 + 0.5 in double, clamped to 0 .. 255,
// truncated.
#pragma once
#include "srl_device.h"
#include "srl_kernels.h"

#define SRL_VIEW_THREADS 256
#define SRL_VIEW_F64 0   // srl_render_rgb's dtype codes
#define SRL_VIEW_U8 1

// what the kernel reads, by value (48 bytes: no need to hand it the whole DevParams)
struct ViewParams {
  const float* H;         // [n_envs][res * res]
  const float* objmap;    // [n_mesh][n_orient][r * r]
  const EnvHdr* hdr;
  int32_t res, r, n_orient, ordering;
  float obj_empty;        // every pixel of the object map when no rock is on show
};

__device__ __forceinline__ float view_red(float m, float mx) { return mx != 0.0f ? m / mx : m; }
__device__ __forceinline__ double view_green(bool goal) { return goal ? 0.5 + 0.1 : 0.5; }
__device__ __forceinline__ uint32_t view_byte(double x) {
  double y = x * 255.0 + 0.5;
  y = y < 0.0 ? 0.0 : (y > 255.0 ? 255.0 : y);
  return (uint32_t)y;
}

// A thread's run of PX consecutive pixels, gathered in registers and stored as whole 128-bit vectors.
template <int DT> struct ViewRun;
template <> struct ViewRun<SRL_VIEW_F64> {
  typedef double elem;
  static constexpr int PX = 4;
  double d[12];
  __device__ __forceinline__ void set(int k, float r, double g, float b) { d[3 * k] = (double)r; d[3 * k + 1] = g; d[3 * k + 2] = (double)b; }
  __device__ __forceinline__ void store(elem* out) const {
    double2* o = reinterpret_cast<double2*>(out);
#pragma unroll
    for (int q = 0; q < 6; ++q) o[q] = make_double2(d[2 * q], d[2 * q + 1]);
  }
  static __device__ __forceinline__ void store_one(elem* out, float r, double g, float b) { out[0] = (double)r; out[1] = g; out[2] = (double)b; }
};
template <> struct ViewRun<SRL_VIEW_U8> {
  typedef uint8_t elem;
  static constexpr int PX = 16;
  uint32_t w[12];
  __device__ __forceinline__ void put(int byte, uint32_t v) { w[byte >> 2] = (byte & 3) ? (w[byte >> 2] | (v << (8 * (byte & 3)))) : v; }
  __device__ __forceinline__ void set(int k, float r, double g, float b) {
    put(3 * k, view_byte((double)r)); put(3 * k + 1, view_byte(g)); put(3 * k + 2, view_byte((double)b));
  }
  __device__ __forceinline__ void store(elem* out) const {
    uint4* o = reinterpret_cast<uint4*>(out);
#pragma unroll
    for (int q = 0; q < 3; ++q) o[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
  static __device__ __forceinline__ void store_one(elem* out, float r, double g, float b) {
    out[0] = (uint8_t)view_byte((double)r); out[1] = (uint8_t)view_byte(g); out[2] = (uint8_t)view_byte((double)b);
  }
};

// this thread's share of np.max over src[0 .. n) (a constant map when src is null)
__device__ __forceinline__ float view_thread_max(const float* __restrict__ src, float cst, int n, int tid) {
  if (!src) return cst;
  float mx = -INFINITY;
  if ((n & 3) == 0) {   // (every map starts at a multiple of n floats from a hipMalloc'ed base: 16-byte aligned)
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (int g = tid; g < (n >> 2); g += SRL_VIEW_THREADS) {
      const float4 v = s4[g];
      mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
  } else {
    for (int p = tid; p < n; p += SRL_VIEW_THREADS) mx = fmaxf(mx, src[p]);
  }
  return mx;
}

// One image: the map src[0 .. n) (rows of `width` pixels; a constant map when src is null) with its max mx -> out[n][3];
// goal = (u, v, h, w) or null.
template <int DT>
__device__ __forceinline__ void view_colour(const float* __restrict__ src, float cst, int n, int width, const int32_t* goal, float mx,
                                            typename ViewRun<DT>::elem* __restrict__ out, int tid) {
  typedef ViewRun<DT> Run;
  int u0 = 0, u1 = 0, v0 = 0, v1 = 0;   // an empty rectangle: no pixel is inside
  if (goal) { u0 = goal[0]; v0 = goal[1]; u1 = u0 + goal[2]; v1 = v0 + goal[3]; }
  if (n % Run::PX == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    for (int g = tid; g < n / Run::PX; g += SRL_VIEW_THREADS) {
      const int p0 = g * Run::PX;
      float m[Run::PX];
#pragma unroll
      for (int q = 0; q < Run::PX / 4; ++q) {
        const float4 v = src ? reinterpret_cast<const float4*>(src + p0)[q] : make_float4(cst, cst, cst, cst);
        m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w;
      }
      int i = p0 / width, j = p0 - i * width;
      Run run;
#pragma unroll
      for (int k = 0; k < Run::PX; ++k) {
        const float r = view_red(m[k], mx);
        run.set(k, r, view_green(i >= u0 && i < u1 && j >= v0 && j < v1), 1.0f - r);
        if (++j == width) { j = 0; ++i; }
      }
      run.store(out + 3 * (size_t)p0);
    }
  } else {
    for (int p = tid; p < n; p += SRL_VIEW_THREADS) {
      const int i = p / width, j = p - i * width;
      const float r = view_red(src ? src[p] : cst, mx);
      Run::store_one(out + 3 * (size_t)p, r, view_green(i >= u0 && i < u1 && j >= v0 && j < v1), 1.0f - r);
    }
  }
}

template <int DT>
__device__ __forceinline__ void view_body(const ViewParams& V, typename ViewRun<DT>::elem* __restrict__ overhead,
                                          typename ViewRun<DT>::elem* __restrict__ object) {
  __shared__ float wave_max[2][SRL_VIEW_THREADS / 64];
  const int e = blockIdx.x, tid = threadIdx.x;
  const int n_over = V.res * V.res, n_obj = V.r * V.r;
  const EnvHdr& hdr = V.hdr[e];
  const float* H = V.H + (size_t)e * n_over;
  // the rock on show: srl_get_maps' choice (stackrl_hip.hip), orientation 0
  const int mesh = V.ordering ? (hdr.list_pos > 0 ? hdr.ids[0] : -1) : hdr.pending;
  const float* O = mesh >= 0 ? V.objmap + (size_t)mesh * V.n_orient * n_obj : nullptr;
  float mx[2] = {overhead ? view_thread_max(H, 0.0f, n_over, tid) : 0.0f, object ? view_thread_max(O, V.obj_empty, n_obj, tid) : 0.0f};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], s, 64));
    if ((tid & 63) == 0) wave_max[k][tid >> 6] = mx[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) mx[k] = fmaxf(fmaxf(wave_max[k][0], wave_max[k][1]), fmaxf(wave_max[k][2], wave_max[k][3]));
  if (overhead) view_colour<DT>(H, 0.0f, n_over, V.res, hdr.goal, mx[0], overhead + 3 * (size_t)e * n_over, tid);
  if (object) view_colour<DT>(O, V.obj_empty, n_obj, V.r, nullptr, mx[1], object + 3 * (size_t)e * n_obj, tid);
}

extern "C" __global__ void __launch_bounds__(SRL_VIEW_THREADS) srl_k_view(ViewParams V, double* __restrict__ overhead, double* __restrict__ object) {
  view_body<SRL_VIEW_F64>(V, overhead, object);
}
extern "C" __global__ void __launch_bounds__(SRL_VIEW_THREADS) srl_k_view_u8(ViewParams V, uint8_t* __restrict__ overhead, uint8_t* __restrict__ object) {
  view_body<SRL_VIEW_U8>(V, overhead, object);
}
