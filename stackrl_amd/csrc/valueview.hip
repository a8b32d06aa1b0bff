// libstackrl_valueview.so — the frames of a visualised comparison run (include/stackrl_valueview.h holds the definition;
// tests/value_view_cases.py restates it in numpy).  Two kernels per call:
//   k_value_range  one workgroup per (tile, frame): the minimum and maximum over the finite cells of the chosen row of the
//                  tile's policy — lanes stride over the map, a butterfly over the wave, the waves through LDS (minimum and
//                  maximum are exact, so the order does not matter) — into range_scratch[policy][frame];
//   k_value_frame  the output is addressed as the flat array of aligned 32-bit words (the allocation is aligned; a row of
//                  FW * 3 bytes need not be): a thread makes four whole pixels = three words per trip, and one thread writes
//                  the at most three pixels beyond the last whole quad by byte stores.  The observation images and the maps
//                  are read where they lie, through the frame's env and the policy's chosen row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/stackrl_valueview.h"

#pragma clang fp contract(off)

namespace {

thread_local char v_err[256] = "";
#define SET_ERR(...) snprintf(v_err, sizeof v_err, __VA_ARGS__)

constexpr int MAXP = SRL_VALUEVIEW_MAX_POLICIES;
constexpr int GAP = SRL_VALUEVIEW_GAP;
constexpr int BW = SRL_VALUEVIEW_BORDER;
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 256 * 16;          // grid-stride beyond this: 256 CUs x 16 workgroups of 256 threads
constexpr uint32_t BACKGROUND = 0xffffffu;
constexpr uint32_t RED = 0x0000ffu;           // packed as r | g << 8 | b << 16

// LUT[k] = (uint8)(viridis[k] * 255) of matplotlib's 256-entry table (`matplotlib.cm.viridis.colors`), r | g << 8 | b << 16
#define SRL_VIRIDIS_WORDS \
  0x540144, 0x550244, 0x570344, 0x580545, 0x5a0645, 0x5b0845, 0x5c0946, 0x5e0b46, \
  0x5f0c46, 0x610e46, 0x620f47, 0x631147, 0x651247, 0x661447, 0x671547, 0x691647, \
  0x6a1847, 0x6b1948, 0x6c1a48, 0x6e1c48, 0x6f1d48, 0x701e48, 0x712048, 0x722148, \
  0x732248, 0x742348, 0x752547, 0x762647, 0x772747, 0x782847, 0x792a47, 0x7a2b47, \
  0x7b2c47, 0x7c2d46, 0x7c2f46, 0x7d3046, 0x7e3146, 0x7f3245, 0x7f3445, 0x803545, \
  0x813645, 0x813744, 0x823944, 0x833a43, 0x833b43, 0x843c43, 0x843d42, 0x853e42, \
  0x854042, 0x864141, 0x864241, 0x874340, 0x874440, 0x87453f, 0x88473f, 0x88483e, \
  0x89493e, 0x894a3d, 0x894b3d, 0x894c3d, 0x8a4d3c, 0x8a4e3c, 0x8a503b, 0x8a513b, \
  0x8b523a, 0x8b533a, 0x8b5439, 0x8b5539, 0x8b5638, 0x8c5738, 0x8c5837, 0x8c5937, \
  0x8c5a36, 0x8c5b36, 0x8c5c35, 0x8c5d35, 0x8d5e34, 0x8d5f34, 0x8d6033, 0x8d6133, \
  0x8d6232, 0x8d6332, 0x8d6431, 0x8d6531, 0x8d6631, 0x8d6730, 0x8d6830, 0x8d692f, \
  0x8d6a2f, 0x8e6b2e, 0x8e6c2e, 0x8e6d2e, 0x8e6e2d, 0x8e6f2d, 0x8e702c, 0x8e712c, \
  0x8e722c, 0x8e732b, 0x8e742b, 0x8e752a, 0x8e762a, 0x8e772a, 0x8e7829, 0x8e7929, \
  0x8e7a28, 0x8e7a28, 0x8e7b28, 0x8e7c27, 0x8e7d27, 0x8e7e27, 0x8e7f26, 0x8e8026, \
  0x8e8126, 0x8e8225, 0x8d8325, 0x8d8424, 0x8d8524, 0x8d8624, 0x8d8723, 0x8d8823, \
  0x8d8923, 0x8d8922, 0x8d8a22, 0x8d8b22, 0x8d8c21, 0x8c8d21, 0x8c8e21, 0x8c8f20, \
  0x8c9020, 0x8c9120, 0x8c921f, 0x8b931f, 0x8b941f, 0x8b951f, 0x8b961f, 0x8a971e, \
  0x8a981e, 0x8a991e, 0x8a991e, 0x899a1e, 0x899b1e, 0x899c1e, 0x889d1e, 0x889e1e, \
  0x889f1e, 0x87a01e, 0x87a11f, 0x86a21f, 0x86a31f, 0x85a420, 0x85a520, 0x85a621, \
  0x84a721, 0x84a722, 0x83a823, 0x82a923, 0x82aa24, 0x81ab25, 0x81ac26, 0x80ad27, \
  0x7fae28, 0x7faf29, 0x7eb02a, 0x7db12b, 0x7db12c, 0x7cb22e, 0x7bb32f, 0x7ab430, \
  0x7ab532, 0x79b633, 0x78b735, 0x77b836, 0x76b938, 0x76b939, 0x75ba3b, 0x74bb3d, \
  0x73bc3e, 0x72bd40, 0x71be42, 0x70be44, 0x6fbf45, 0x6ec047, 0x6dc149, 0x6cc24b, \
  0x6bc24d, 0x69c34f, 0x68c451, 0x67c553, 0x66c655, 0x65c657, 0x64c759, 0x62c85b, \
  0x61c95e, 0x60c960, 0x5fca62, 0x5dcb64, 0x5ccc67, 0x5bcc69, 0x59cd6b, 0x58ce6d, \
  0x56ce70, 0x55cf72, 0x54d074, 0x52d077, 0x51d179, 0x4fd27c, 0x4ed27e, 0x4cd381, \
  0x4bd383, 0x49d486, 0x47d588, 0x46d58b, 0x44d68d, 0x43d690, 0x41d792, 0x3fd795, \
  0x3ed897, 0x3cd89a, 0x3ad99d, 0x38d99f, 0x37daa2, 0x35daa5, 0x33dba7, 0x32dbaa, \
  0x30dcad, 0x2edcaf, 0x2cddb2, 0x2bddb5, 0x29ddb7, 0x27deba, 0x26debd, 0x24dfbf, \
  0x22dfc2, 0x21dfc5, 0x1fe0c7, 0x1ee0ca, 0x1de0cd, 0x1ce1cf, 0x1be1d2, 0x1ae1d4, \
  0x19e2d7, 0x18e2da, 0x18e2dc, 0x18e3df, 0x18e3e1, 0x18e3e4, 0x19e4e7, 0x19e4e9, \
  0x1ae4ec, 0x1be5ee, 0x1ce5f1, 0x1ee5f3, 0x1fe6f6, 0x21e6f8, 0x22e6fa, 0x24e7fd

const uint32_t h_lut[256] = {SRL_VIRIDIS_WORDS};
__device__ const uint32_t d_lut[256] = {SRL_VIRIDIS_WORDS};

struct Layout {
  int32_t FH, FW, nv, ncol, nline, TB, SH, Sh, OH;
};

// The layout arithmetic of the definition, once.  64-bit, so that the callers can refuse what does not fit.
bool layout_of(int32_t H, int32_t h, int32_t P, int32_t s, Layout* l, int64_t* frame_bytes) {
  if (h < 1 || H < h || P < 1 || P > MAXP || s < 1 || s > SRL_VALUEVIEW_MAX_SCALE) return false;
  const int64_t OH = (int64_t)H - h + 1, SH = (int64_t)s * H, Sh = (int64_t)s * h, TB = s * OH + 2 * BW;
  const int nv = P < SRL_VALUEVIEW_MAX_SHOWN ? P : SRL_VALUEVIEW_MAX_SHOWN;
  const int ncol = nv < 3 ? nv : 3, nline = 1 + (nv > 3);
  const int64_t FW = 2 * GAP + SH + ncol * (TB + GAP);
  const int64_t left = 3 * GAP + SH + Sh, right = GAP + nline * (TB + GAP);
  const int64_t FH = left > right ? left : right;
  if (FW > INT32_MAX / 3 || FH > INT32_MAX || FH * FW * 3 > (int64_t)INT32_MAX) return false;
  *l = Layout{(int32_t)FH, (int32_t)FW, nv, ncol, nline, (int32_t)TB, (int32_t)SH, (int32_t)Sh, (int32_t)OH};
  *frame_bytes = FH * FW * 3;
  return true;
}

int window_of(int P, int nv, int index) {
  const int lo = index - nv / 2;
  return lo < 0 ? 0 : (lo > P - nv ? P - nv : lo);
}

struct Args {
  const void* map[MAXP];
  const uint8_t* rgb0;
  const uint8_t* rgb1;
  const int64_t* actions;
  const int32_t* indexes;
  float* range;
  uint32_t* words;             // the frames as aligned 32-bit words
  uint32_t n_quads, n_pixels;  // whole quads of pixels (three words each), and all pixels (n_pixels - 4 n_quads < 4: the tail)
  int32_t f64_mask, B, G, H, h, A, n, index, min_j, s, mark;
  Layout l;
};

__device__ __forceinline__ const void* map_of(const Args& g, int j) {
  const void* p = g.map[0];
#pragma unroll
  for (int k = 1; k < MAXP; ++k) p = j == k ? g.map[k] : p;
  return p;
}

__device__ __forceinline__ int env_of(const Args& g, int f) {
  const int b = g.indexes[f];
  return b < 0 ? 0 : (b > g.B - 1 ? g.B - 1 : b);
}

// (row clamped to 0..G-1, pixel = the non-negative remainder) of policy j's action in env b; (0, -1) without actions
__device__ __forceinline__ void chosen(const Args& g, int j, int b, int* row, int* pixel) {
  *row = 0;
  *pixel = -1;
  if (g.actions) {
    const int64_t a = g.actions[(int64_t)j * g.B + b];
    int64_t r, p;
    if ((uint64_t)a <= (uint64_t)INT32_MAX) {        // every action of a valid run: a 32-bit division
      const uint32_t q = (uint32_t)a / (uint32_t)g.A;
      r = q;
      p = (uint32_t)a - q * (uint32_t)g.A;
    } else {
      r = a / g.A;
      p = a % g.A;
      if (p < 0) p += g.A;
      r = a < 0 ? 0 : r;
    }
    *row = (int)(r > g.G - 1 ? g.G - 1 : r);
    *pixel = (int)p;
  }
}

// element a of the chosen row, rounded to float32
__device__ __forceinline__ float cell(const Args& g, int j, int64_t base, int a) {
  const void* m = map_of(g, j);
  return (g.f64_mask >> j) & 1 ? (float)((const double*)m)[base + a] : ((const float*)m)[base + a];
}

__device__ __forceinline__ bool finite32(float x) { return fabsf(x) < INFINITY; }       // false for NaN

__global__ __launch_bounds__(THREADS) void k_value_range(Args g) {
  const int f = blockIdx.x, k = blockIdx.y, j = g.min_j + k;
  const int b = env_of(g, f);
  int row, pixel;
  chosen(g, j, b, &row, &pixel);
  const int64_t base = ((int64_t)b * g.G + row) * g.A;
  float lo = INFINITY, hi = -INFINITY;
  for (int a = threadIdx.x; a < g.A; a += THREADS) {
    const float x = cell(g, j, base, a);
    if (finite32(x)) {
      lo = fminf(lo, x);
      hi = fmaxf(hi, x);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  __shared__ float s_lo[THREADS / 64], s_hi[THREADS / 64];
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) {
      lo = fminf(lo, s_lo[w]);
      hi = fmaxf(hi, s_hi[w]);
    }
    float* out = g.range + ((int64_t)j * g.n + f) * 2;
    out[0] = lo;                                     // (+inf, -inf): no finite cell
    out[1] = hi;
  }
}

// the colour of pixel (r, c) of frame f, packed
__device__ __forceinline__ uint32_t colour(const Args& g, const uint32_t* lut, int f, int r, int c) {
  const Layout& l = g.l;
  const int b = env_of(g, f);
  const int s = g.s;
  const int x0 = c - GAP;
  if (x0 < 0) return BACKGROUND;
  if (x0 < l.SH) {                                   // the column of the two views
    const int y0 = r - GAP;
    if (y0 < 0) return BACKGROUND;
    if (y0 < l.SH) {
      const int sr = y0 / s, sc = x0 / s;
      if (g.mark && g.actions) {
        int row, pixel;
        chosen(g, g.index, b, &row, &pixel);
        const int u = pixel / l.OH, v = pixel % l.OH;
        const int dr = sr - u, dc = sc - v;
        if (dr >= 0 && dr < g.h && dc >= 0 && dc < g.h && (dr == 0 || dr == g.h - 1 || dc == 0 || dc == g.h - 1)) return RED;
      }
      const uint8_t* p = g.rgb0 + (((int64_t)b * g.H + sr) * g.H + sc) * 3;
      return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
    const int y1 = y0 - l.SH - GAP;
    if (y1 >= 0 && y1 < l.Sh && x0 < l.Sh) {
      const uint8_t* p = g.rgb1 + (((int64_t)b * g.h + y1 / s) * g.h + x0 / s) * 3;
      return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
    return BACKGROUND;
  }
  const int x1 = x0 - l.SH - GAP, y1 = r - GAP;       // relative to the first tile's box
  if (x1 < 0 || y1 < 0) return BACKGROUND;
  const int pitch = l.TB + GAP;
  const int tc = x1 / pitch, wc = x1 % pitch, tr = y1 / pitch, wr = y1 % pitch;
  const int k = tr * 3 + tc;
  if (tc >= l.ncol || tr >= l.nline || k >= l.nv || wc >= l.TB || wr >= l.TB) return BACKGROUND;
  const int j = g.min_j + k;
  const int cr = wr - BW, cc = wc - BW, ST = l.TB - 2 * BW;
  if (cr < 0 || cc < 0 || cr >= ST || cc >= ST) return j == g.index ? lut[255] : BACKGROUND;     // the ring
  const int a = (cr / s) * l.OH + cc / s;
  int row, pixel;
  chosen(g, j, b, &row, &pixel);
  if (g.mark && a == pixel) return RED;
  const float x = cell(g, j, ((int64_t)b * g.G + row) * g.A, a);
  const float vmin = g.range[((int64_t)j * g.n + f) * 2], vmax = g.range[((int64_t)j * g.n + f) * 2 + 1];
  if (!finite32(x) || !(vmin <= vmax)) return BACKGROUND;
  float t = x - vmin;
  t = __fdiv_rn(t, vmax - vmin);
  t = t * 256.0f;
  if (vmax == vmin) t = 0.0f;
  const int q = !(t > 0.0f) ? 0 : (t >= 255.0f ? 255 : (int)t);
  return lut[q];
}

// the colours of `count` <= 4 consecutive pixels of the flat output from pixel p on, packed
__device__ __forceinline__ void pixels_at(const Args& g, const uint32_t* lut, uint32_t p, int count, uint32_t* out) {
  const Layout& l = g.l;
  const uint32_t frame_pixels = (uint32_t)l.FW * (uint32_t)l.FH;
  int f = (int)(p / frame_pixels);
  const uint32_t rem = p - (uint32_t)f * frame_pixels;
  int r = (int)(rem / (uint32_t)l.FW);
  int c = (int)(rem - (uint32_t)r * (uint32_t)l.FW);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    out[q] = q < count ? colour(g, lut, f, r, c) : 0;
    if (++c == l.FW) {
      c = 0;
      if (++r == l.FH) { r = 0; ++f; }
    }
  }
}

// A thread makes four whole pixels = three aligned words (12 bytes) per trip; the at most three pixels beyond the last whole
// quad are written by one thread, byte by byte.
__global__ __launch_bounds__(THREADS) void k_value_frame(Args g) {
  __shared__ uint32_t lut[256];
  lut[threadIdx.x] = d_lut[threadIdx.x];             // THREADS == 256
  __syncthreads();
  const uint32_t stride = gridDim.x * THREADS;
  const uint32_t gid = blockIdx.x * THREADS + threadIdx.x;
  // gridDim.x = min(ceil(n_quads / THREADS), MAX_BLOCKS): at most ceil(2^31 / 12 / (MAX_BLOCKS * THREADS)) = 171 trips
  for (uint32_t q = gid; q < g.n_quads; q += stride) {
    uint32_t c[4];
    pixels_at(g, lut, q * 4, 4, c);
    uint32_t* w = g.words + (size_t)q * 3;
    w[0] = c[0] | c[1] << 24;
    w[1] = c[1] >> 8 | c[2] << 16;
    w[2] = c[2] >> 16 | c[3] << 8;
  }
  const int tail = (int)(g.n_pixels - g.n_quads * 4);
  if (gid == 0 && tail) {
    uint32_t c[4];
    pixels_at(g, lut, g.n_quads * 4, tail, c);
    uint8_t* out = (uint8_t*)g.words + (size_t)g.n_quads * 12;
    for (int q = 0; q < tail; ++q)
      for (int ch = 0; ch < 3; ++ch) out[3 * q + ch] = (uint8_t)(c[q] >> (8 * ch));
  }
}

}  // namespace

extern "C" {

const char* srl_valueview_last_error(void) { return v_err; }

#ifndef SRL_BUILD_INFO
#define SRL_BUILD_INFO "SRL_BUILD_INFO<unknown|>"
#endif
const char* srl_valueview_build_info(void) { static const char info[] = SRL_BUILD_INFO; return info; }

int srl_valueview_layout(int32_t H, int32_t h, int32_t P, int32_t scale, int32_t* out) {
  Layout l;
  int64_t bytes;
  if (!out) { SET_ERR("srl_valueview_layout: out is null"); return SRL_EINVAL; }
  if (!layout_of(H, h, P, scale, &l, &bytes)) {
    SET_ERR("srl_valueview_layout: no frame for H %d, h %d, P %d, scale %d (1 <= h <= H, P in 1..%d, scale in 1..%d, a frame "
            "within 2^31-1 bytes)", H, h, P, scale, MAXP, SRL_VALUEVIEW_MAX_SCALE);
    return SRL_EINVAL;
  }
  const int32_t v[8] = {l.FH, l.FW, l.nv, l.ncol, l.nline, l.TB, window_of(P, l.nv, 0), window_of(P, l.nv, P - 1)};
  memcpy(out, v, sizeof v);
  return SRL_OK;
}

int srl_valueview_window(int32_t P, int32_t index, int32_t* min_j) {
  if (P < 1 || P > MAXP) { SET_ERR("srl_valueview_window: the number of policies must be in 1..%d, got %d", MAXP, P); return SRL_EINVAL; }
  if (index < 0 || index >= P) { SET_ERR("srl_valueview_window: index must be in 0..%d, got %d", P - 1, index); return SRL_EINVAL; }
  if (!min_j) { SET_ERR("srl_valueview_window: min_j is null"); return SRL_EINVAL; }
  *min_j = window_of(P, P < SRL_VALUEVIEW_MAX_SHOWN ? P : SRL_VALUEVIEW_MAX_SHOWN, index);
  return SRL_OK;
}

int srl_valueview_lut(uint8_t* out) {
  if (!out) { SET_ERR("srl_valueview_lut: out is null"); return SRL_EINVAL; }
  for (int k = 0; k < 256; ++k)
    for (int c = 0; c < 3; ++c) out[3 * k + c] = (uint8_t)(h_lut[k] >> (8 * c));
  return SRL_OK;
}

int srl_valueview_frames(int32_t P, const void* map0, const void* map1, const void* map2, const void* map3, const void* map4,
                         const void* map5, const void* map6, const void* map7, int32_t f64_mask, int32_t B, int32_t G,
                         int32_t H, int32_t h, const uint8_t* rgb0, const uint8_t* rgb1, const int64_t* actions,
                         const int32_t* indexes, int32_t n, int32_t index, int32_t scale, int32_t mark, float* range_scratch,
                         uint8_t* frames, void* stream) {
  const void* maps[MAXP] = {map0, map1, map2, map3, map4, map5, map6, map7};
  if (P < 1 || P > MAXP) { SET_ERR("srl_valueview_frames: the number of policies must be in 1..%d, got %d", MAXP, P); return SRL_EINVAL; }
  if (index < 0 || index >= P) { SET_ERR("srl_valueview_frames: index must be in 0..%d, got %d", P - 1, index); return SRL_EINVAL; }
  if (scale < 1 || scale > SRL_VALUEVIEW_MAX_SCALE) {
    SET_ERR("srl_valueview_frames: scale must be in 1..%d, got %d", SRL_VALUEVIEW_MAX_SCALE, scale);
    return SRL_EINVAL;
  }
  if (n < 1) { SET_ERR("srl_valueview_frames: n must be at least 1, got %d", n); return SRL_EINVAL; }
  if (B < 1) { SET_ERR("srl_valueview_frames: B must be at least 1, got %d", B); return SRL_EINVAL; }
  if (G < 1) { SET_ERR("srl_valueview_frames: G must be at least 1, got %d", G); return SRL_EINVAL; }
  if (h < 1 || H < h) { SET_ERR("srl_valueview_frames: the views need 1 <= h <= H, got H %d, h %d", H, h); return SRL_EINVAL; }
  const int64_t OH = (int64_t)H - h + 1, A = OH * OH;
  if (A > (int64_t)INT32_MAX - 1 || (int64_t)G * A > (int64_t)INT32_MAX - 1) {
    SET_ERR("srl_valueview_frames: G * A must be at most 2^31-2, got %d * %lld", G, (long long)A);
    return SRL_EINVAL;
  }
  for (int j = 0; j < P; ++j)
    if (!maps[j]) { SET_ERR("srl_valueview_frames: map %d of %d policies is null", j, P); return SRL_EINVAL; }
  if (!rgb0 || !rgb1 || !indexes || !range_scratch || !frames) {
    SET_ERR("srl_valueview_frames: a required pointer is null (rgb0 %d, rgb1 %d, indexes %d, range_scratch %d, frames %d)",
            rgb0 != nullptr, rgb1 != nullptr, indexes != nullptr, range_scratch != nullptr, frames != nullptr);
    return SRL_EINVAL;
  }
  Args g = {};
  int64_t frame_bytes = 0;
  if (!layout_of(H, h, P, scale, &g.l, &frame_bytes) || n * frame_bytes > (int64_t)INT32_MAX) {
    SET_ERR("srl_valueview_frames: the frames must fit 2^31-1 bytes, got n %d at H %d, h %d, scale %d, P %d", n, H, h, scale, P);
    return SRL_EINVAL;
  }
  for (int j = 0; j < MAXP; ++j) g.map[j] = j < P ? maps[j] : maps[0];
  g.rgb0 = rgb0; g.rgb1 = rgb1; g.actions = actions; g.indexes = indexes; g.range = range_scratch;
  g.words = (uint32_t*)frames;
  g.n_pixels = (uint32_t)(n * frame_bytes / 3);
  g.n_quads = g.n_pixels / 4;
  g.f64_mask = f64_mask; g.B = B; g.G = G; g.H = H; g.h = h; g.A = (int32_t)A; g.n = n; g.index = index;
  g.min_j = window_of(P, g.l.nv, index);
  g.s = scale; g.mark = mark != 0;
  if ((uintptr_t)frames & 3) { SET_ERR("srl_valueview_frames: frames must be 4-byte aligned"); return SRL_EINVAL; }
  hipLaunchKernelGGL(k_value_range, dim3(n, g.l.nv), dim3(THREADS), 0, (hipStream_t)stream, g);
  const uint32_t want = (g.n_quads + THREADS - 1) / THREADS;
  const uint32_t blocks = want < 1 ? 1 : (want > MAX_BLOCKS ? MAX_BLOCKS : want);
  hipLaunchKernelGGL(k_value_frame, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, g);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_valueview_frames: %s", hipGetErrorString(e)); return SRL_EHIP; }
  return SRL_OK;
}

}  // extern "C"
