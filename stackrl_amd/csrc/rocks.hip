// rocks.hip — the procedural rock generator (include/stackrl_rocks.h), gfx950.
//
// k_rocks: one wavefront (a workgroup of 64 threads) per rock, the whole rock in LDS (about 30 KB).
//   points   lanes over the points of a level; Philox4x32-10 per draw, normcdfinv in float64
//   hull     gift wrapping.  A pivot is a tournament of the 64 lanes on the float64 orient3d determinant: every lane runs
//            through its points in ascending order, then lane l takes lane l + o (o = 32 .. 1) and lane 0 holds the winner.
//            The bookkeeping (vertex numbers, the bitmap of directed edges, the first-in first-out list of open edges, the
//            triangle list) is written by every lane with the same values, so each lane reads back what it wrote itself and
//            the control flow is the same in all lanes; no atomics, no arrival order.
//   box      for every face the vertices are projected once into the face's plane (lanes over vertices), then lanes over the
//            hull's edges, each running through the vertices (LDS broadcast reads)
//   sums     a lane's elements in ascending order, then a butterfly: the same bits in every lane and on every call
// The determinants and sums are float64 with one rounding per written operation (no contraction into fused multiply-adds):
// tests/rocks_cases.py writes the same operations in numpy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <array>
#include <utility>
#include <vector>

#include "../../include/stackrl_rocks.h"

#pragma clang fp contract(off)

namespace {
thread_local char r_err[256] = "";
#define SET_ERR(...) snprintf(r_err, sizeof r_err, __VA_ARGS__)

constexpr int MAXP = SRL_ROCKS_MAX_POINTS;
constexpr int MAXV = SRL_MAX_VERTS;
constexpr int MAXT = SRL_MAX_TRIS;
constexpr int QCAP = 3 * MAXT + 4;           // every face opens at most three edges, and the first edge
constexpr uint32_t TAG = 0x524f434bu;        // the key's second word: this export's stream
constexpr uint32_t DENSITY_DRAW = 0xffffffffu;

struct Parents { uint16_t p[MAXP][2]; };      // point k >= 8: the two points it is the midpoint of

struct Args {
  double half_ext[3];      // ext / 2
  double scale0;           // irregularity * radius
  double bound;            // 1 / irregularity
  double Fa, Fw;           // Phi(-bound), Phi(bound) - Phi(-bound)
  double radius, density_lo, density_hi;
  int64_t first_index;
  const float* points_in;
  float* points_out;
  float* verts; int32_t* vert_src; int32_t* tris; int32_t* counts;
  float* mass_com; float* inertia; float* xform; float* metrics; int32_t* status;
  uint32_t seed;
  int32_t P, levels, fit;
};

// Philox4x32-10 of the counter (c0, c1, c2, 0) under the key (k0, k1): word 0
__device__ __forceinline__ uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1) {
  uint32_t c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ double uniform64(uint32_t x) { return ((double)x + 0.5) * 2.3283064365386963e-10; }   // 2^-32

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 u, D3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ double dot(D3 u, D3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ D3 scaled(D3 u, double s) { return {u.x * s, u.y * s, u.z * s}; }
__device__ __forceinline__ D3 unit(D3 u) { const double l = sqrt(dot(u, u)); return {u.x / l, u.y / l, u.z / l}; }
__device__ __forceinline__ D3 ldp(const float* pf, int k) { return {(double)pf[3 * k], (double)pf[3 * k + 1], (double)pf[3 * k + 2]}; }

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ double wave_min(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmin(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}

// The pivot about the directed line A -> B: the point c (not a, not b, not on the line) with orient(A, B, c, q) <= 0 for every
// other q, the lowest index among equals; -1 if there is no candidate.  "q beats c" (orient > 0, or = 0 and q < c) is a strict
// total order wherever the points lie within half a turn about the line, so the winner does not depend on the order of the
// comparisons.  The same value in every lane.
__device__ int pivot(const float* pf, int P, int a, int b, D3 A, D3 B, int lane) {
  const D3 e = sub(B, A);
  int best = -1;
  D3 nb = {0, 0, 0};                                  // e x (best - A)
  for (int q = lane; q < P; q += 64) {
    if (q == a || q == b) continue;
    const D3 w = sub(ldp(pf, q), A), cr = cross(e, w);
    if (cr.x == 0.0 && cr.y == 0.0 && cr.z == 0.0) continue;
    if (best < 0 || dot(nb, w) > 0.0) { best = q; nb = cr; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int other = __shfl_down(best, o);
    if (other >= 0) {
      const D3 Q = ldp(pf, other);
      const double d = best < 0 ? 1.0 : dot(nb, sub(Q, A));
      if (d > 0.0 || (d == 0.0 && other < best)) { best = other; nb = cross(e, sub(Q, A)); }
    }
  }
  return __shfl(best, 0);
}

// second moments of the tetrahedron (0, a, b, c) times 120 / det: sum_p v_p v_p^T + (sum_p v_p)(sum_p v_p)^T
__device__ __forceinline__ double moment(double a, double b, double c, double a2, double b2, double c2) {
  return ((a * a2 + b * b2) + c * c2) + ((a + b) + c) * ((a2 + b2) + c2);
}

// a rock that is not ok: counts (0, 0), zeros elsewhere
__device__ void fail(const Args& g, int i, int lane, int status) {
  float* verts = g.verts + (size_t)i * MAXV * 3;
  int32_t* vsrc = g.vert_src + (size_t)i * MAXV;
  int32_t* tris = g.tris + (size_t)i * MAXT * 3;
  for (int k = lane; k < MAXV * 3; k += 64) verts[k] = 0.f;
  for (int k = lane; k < MAXV; k += 64) vsrc[k] = -1;
  for (int k = lane; k < MAXT * 3; k += 64) tris[k] = 0;
  if (lane < 2) g.counts[2 * (size_t)i + lane] = 0;
  if (lane < 4) { g.mass_com[4 * (size_t)i + lane] = 0.f; g.metrics[4 * (size_t)i + lane] = 0.f; }
  if (lane < 6) g.inertia[6 * (size_t)i + lane] = 0.f;
  if (lane < 13) g.xform[13 * (size_t)i + lane] = 0.f;
  if (lane == 0) g.status[i] = status;
}

__global__ void __launch_bounds__(64) k_rocks(const Args g, const Parents par) {
  __shared__ double pd[MAXP * 3];                     // the points in float64 while they are made
  __shared__ float pf[MAXP * 3];                      // the points
  __shared__ int lid[MAXP];                           // point -> hull vertex in the order of discovery, -1
  __shared__ int src_of[MAXV];                        // hull vertex (discovery order) -> point
  __shared__ int rank_of[MAXV];                       // hull vertex (discovery order) -> its number (ascending point index)
  __shared__ uint32_t done[MAXV * (MAXV / 32)];       // directed edge (i, j) has its face
  __shared__ int queue[QCAP];                         // open directed edges, i * MAXV + j
  __shared__ int tl[MAXT * 3];                        // triangles, final vertex numbers
  __shared__ double hv[MAXV * 3];                     // hull vertices minus the centre of mass, final numbering
  __shared__ double px[MAXV], py[MAXV];               // their projection into a face's plane
  __shared__ float fv[MAXV * 3];                      // the final vertices
  __shared__ int vs[MAXV];                            // hull vertex (final numbering) -> point

  const int i = blockIdx.x, lane = threadIdx.x, P = g.P;
  const uint64_t gi = (uint64_t)(g.first_index + (int64_t)i);
  const uint32_t g0 = (uint32_t)gi, g1 = (uint32_t)(gi >> 32);

  // ---- 1. points
  if (g.points_in) {
    for (int k = lane; k < 3 * P; k += 64) pf[k] = g.points_in[(size_t)i * 3 * P + k];
  } else {
    int start = 0, end = 8;
    for (int l = 0; l <= g.levels; ++l) {
      const double scale = g.scale0 * (1.0 / (double)(1 << l));
      for (int k = start + lane; k < end; k += 64) {
        for (int j = 0; j < 3; ++j) {
          double base;
          if (l == 0) base = ((k >> (2 - j)) & 1) ? g.half_ext[j] : -g.half_ext[j];
          else base = (pd[3 * par.p[k][0] + j] + pd[3 * par.p[k][1] + j]) / 2.0;
          const double u = uniform64(philox_word0(g0, g1, (uint32_t)(3 * k + j), g.seed, TAG));
          double x = normcdfinv(g.Fa + u * g.Fw);
          x = fmin(fmax(x, -g.bound), g.bound);
          pd[3 * k + j] = base + scale * x;
        }
      }
      __syncthreads();
      start = end;
      end = 4 * end - 6;                              // 8, 26, 98, 386
    }
    for (int k = lane; k < 3 * P; k += 64) pf[k] = (float)pd[k];
  }
  for (int k = lane; k < MAXP; k += 64) lid[k] = -1;
  for (int k = lane; k < MAXV * (MAXV / 32); k += 64) done[k] = 0u;
  __syncthreads();
  if (g.points_out) for (int k = lane; k < 3 * P; k += 64) g.points_out[(size_t)i * 3 * P + k] = pf[k];

  // ---- 2. hull
  int status = SRL_ROCKS_OK, nv = 0, nt = 0;
  {
    int p0 = 0;                                       // the lowest (x, y, z, index): every lane runs through all points
    for (int k = 1; k < P; ++k) {
      const float ax = pf[3 * k], ay = pf[3 * k + 1], az = pf[3 * k + 2], bx = pf[3 * p0], by = pf[3 * p0 + 1], bz = pf[3 * p0 + 2];
      if (ax < bx || (ax == bx && (ay < by || (ay == by && az < bz)))) p0 = k;
    }
    const D3 A0 = ldp(pf, p0);
    const int p1 = pivot(pf, P, p0, -1, A0, {A0.x, A0.y + 1.0, A0.z}, lane);
    int head = 0, tail = 0;
    if (p1 < 0) status = SRL_ROCKS_DEGENERATE;
    else {
      lid[p0] = 0; src_of[0] = p0; lid[p1] = 1; src_of[1] = p1; nv = 2;
      queue[tail++] = 0 * MAXV + 1;
    }
    while (status == SRL_ROCKS_OK && head < tail) {   // at most QCAP pops: a face is emitted or the edge is skipped
      const int e = queue[head++], la = e / MAXV, lb = e % MAXV;
      if ((done[la * (MAXV / 32) + (lb >> 5)] >> (lb & 31)) & 1u) continue;
      const int a = src_of[la], b = src_of[lb];
      const int c = pivot(pf, P, a, b, ldp(pf, a), ldp(pf, b), lane);
      if (c < 0) { status = SRL_ROCKS_DEGENERATE; break; }
      int lc = lid[c];
      if (lc < 0) {
        if (nv >= MAXV) { status = SRL_ROCKS_OVERFLOW; break; }
        lc = nv++; lid[c] = lc; src_of[lc] = c;
      }
      if (nt >= MAXT) { status = SRL_ROCKS_OVERFLOW; break; }
      const int v3[3] = {la, lb, lc};
      bool twice = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int s = v3[k], t = v3[(k + 1) % 3], w = s * (MAXV / 32) + (t >> 5);
        const uint32_t old = done[w];
        twice |= (old >> (t & 31)) & 1u;
        done[w] = old | (1u << (t & 31));
      }
      if (twice) { status = SRL_ROCKS_DEGENERATE; break; }
      tl[3 * nt] = la; tl[3 * nt + 1] = lb; tl[3 * nt + 2] = lc; ++nt;
#pragma unroll
      for (int k = 0; k < 3; ++k) {                   // the opposite of each edge, unless it has its face
        const int s = v3[(k + 1) % 3], t = v3[k];
        if (!((done[s * (MAXV / 32) + (t >> 5)] >> (t & 31)) & 1u) && tail < QCAP) queue[tail++] = s * MAXV + t;
      }
    }
    if (status == SRL_ROCKS_OK) {                     // closed: every directed edge has its opposite, and Euler's formula
      bool open = false;
      for (int k = lane; k < 3 * nt; k += 64) {
        const int s = tl[k], t = tl[(k / 3) * 3 + (k % 3 + 1) % 3];
        open |= !((done[t * (MAXV / 32) + (s >> 5)] >> (s & 31)) & 1u);
      }
      if (__any(open) || nv < 4 || nt != 2 * nv - 4) status = SRL_ROCKS_DEGENERATE;
    }
    if (status == SRL_ROCKS_OK) {                     // convex: every point on or behind every face (ties may have folded the wrap)
      bool front = false;
      for (int f = 0; f < nt; ++f) {
        const int a = src_of[tl[3 * f]], b = src_of[tl[3 * f + 1]], c = src_of[tl[3 * f + 2]];
        const D3 A = ldp(pf, a);
        const D3 n = cross(sub(ldp(pf, b), A), sub(ldp(pf, c), A));
        for (int q = lane; q < P; q += 64) front |= q != a && q != b && q != c && dot(n, sub(ldp(pf, q), A)) > 0.0;
      }
      if (__any(front)) status = SRL_ROCKS_DEGENERATE;
    }
  }
  __syncthreads();

  float* verts = g.verts + (size_t)i * MAXV * 3;
  int32_t* vsrc = g.vert_src + (size_t)i * MAXV;
  int32_t* tris = g.tris + (size_t)i * MAXT * 3;
  if (status != SRL_ROCKS_OK) {
    fail(g, i, lane, status);
    return;
  }

  // vertices by ascending point index
  for (int v = lane; v < nv; v += 64) {
    int r = 0;
    const int s = src_of[v];
    for (int w = 0; w < nv; ++w) r += src_of[w] < s;
    rank_of[v] = r;
  }
  __syncthreads();
  for (int k = lane; k < 3 * nt; k += 64) tl[k] = rank_of[tl[k]];
  for (int v = lane; v < nv; v += 64) vs[rank_of[v]] = src_of[v];
  __syncthreads();
  for (int v = lane; v < MAXV; v += 64) vsrc[v] = v < nv ? vs[v] : -1;

  // ---- 3. centre of mass of the hull (signed tetrahedra from the origin)
  D3 com;
  {
    double s0 = 0, sx = 0, sy = 0, sz = 0;
    for (int t = lane; t < nt; t += 64) {
      const D3 a = ldp(pf, vs[tl[3 * t]]), b = ldp(pf, vs[tl[3 * t + 1]]), c = ldp(pf, vs[tl[3 * t + 2]]);
      const double d = dot(a, cross(b, c));
      s0 += d; sx += ((a.x + b.x) + c.x) * d; sy += ((a.y + b.y) + c.y) * d; sz += ((a.z + b.z) + c.z) * d;
    }
    s0 = wave_sum(s0); sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    if (!(s0 > 0.0)) {                                // no volume: degenerate after all (uniform: s0 is the same in all lanes)
      status = SRL_ROCKS_DEGENERATE;
    }
    com = {sx / (4.0 * s0), sy / (4.0 * s0), sz / (4.0 * s0)};
  }
  double maxr2 = 0;
  for (int v = lane; v < nv; v += 64) {
    const D3 u = sub(ldp(pf, vs[v]), com);
    hv[3 * v] = u.x; hv[3 * v + 1] = u.y; hv[3 * v + 2] = u.z;
    maxr2 = fmax(maxr2, dot(u, u));
  }
  maxr2 = wave_max(maxr2);
  // every edge once: the slots k = 3 * triangle + corner whose edge runs from the lower to the higher vertex, in ascending
  // order, compacted by ballot into the list the open edges were in
  int ne = 0;
  for (int base = 0; base < 3 * nt; base += 64) {
    const int k = base + lane;
    const bool up = k < 3 * nt && tl[k] < tl[(k / 3) * 3 + (k % 3 + 1) % 3];
    const unsigned long long mask = __ballot(up);
    if (up) queue[ne + __popcll(mask & ((1ull << lane) - 1ull))] = k;
    ne += __popcll(mask);
  }
  __syncthreads();

  // ---- 4. the minimum-volume box over (face normal, edge) pairs
  double best_vol = INFINITY;
  int best_key = 0x7fffffff;                          // face * 1024 + edge slot
  for (int f = 0; f < nt && status == SRL_ROCKS_OK; ++f) {
    const D3 a = {hv[3 * tl[3 * f]], hv[3 * tl[3 * f] + 1], hv[3 * tl[3 * f] + 2]};
    const D3 b = {hv[3 * tl[3 * f + 1]], hv[3 * tl[3 * f + 1] + 1], hv[3 * tl[3 * f + 1] + 2]};
    const D3 c = {hv[3 * tl[3 * f + 2]], hv[3 * tl[3 * f + 2] + 1], hv[3 * tl[3 * f + 2] + 2]};
    const D3 n = unit(cross(sub(b, a), sub(c, a)));
    const D3 ref = fabs(n.x) < 0.9 ? D3{1, 0, 0} : D3{0, 1, 0};
    const D3 x = unit(cross(n, ref)), y = cross(n, x);
    double lo = INFINITY, hi = -INFINITY;
    for (int v = lane; v < nv; v += 64) {
      const D3 u = {hv[3 * v], hv[3 * v + 1], hv[3 * v + 2]};
      px[v] = dot(u, x); py[v] = dot(u, y);
      const double h = dot(u, n);
      lo = fmin(lo, h); hi = fmax(hi, h);
    }
    const double height = wave_max(hi) - wave_min(lo);
    __syncthreads();
    for (int j = lane; j < ne; j += 64) {
      const int k = queue[j], s = tl[k], t = tl[(k / 3) * 3 + (k % 3 + 1) % 3];
      const double dx = px[t] - px[s], dy = py[t] - py[s], len = sqrt(dx * dx + dy * dy);
      if (!(len > 0.0)) continue;                     // an edge along the normal names no direction
      const double cs = dx / len, sn = dy / len;
      double xl = INFINITY, xh = -INFINITY, yl = INFINITY, yh = -INFINITY;
      for (int v = 0; v < nv; ++v) {
        const double X = px[v] * cs + py[v] * sn, Y = py[v] * cs - px[v] * sn;
        xl = fmin(xl, X); xh = fmax(xh, X); yl = fmin(yl, Y); yh = fmax(yh, Y);
      }
      const double vol = ((xh - xl) * (yh - yl)) * height;
      if (vol < best_vol) { best_vol = vol; best_key = f * 1024 + k; }
    }
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(best_vol, o);
    const int ok = __shfl_xor(best_key, o);
    if (ov < best_vol || (ov == best_vol && ok < best_key)) { best_vol = ov; best_key = ok; }
  }
  if (best_key == 0x7fffffff) status = SRL_ROCKS_DEGENERATE;
  if (status != SRL_ROCKS_OK) {                       // uniform
    fail(g, i, lane, status);
    return;
  }
  double R[3][3], centre[3], ext[3];
  {
    const int f = best_key / 1024, k = best_key % 1024;
    const D3 a = {hv[3 * tl[3 * f]], hv[3 * tl[3 * f] + 1], hv[3 * tl[3 * f] + 2]};
    const D3 b = {hv[3 * tl[3 * f + 1]], hv[3 * tl[3 * f + 1] + 1], hv[3 * tl[3 * f + 1] + 2]};
    const D3 c = {hv[3 * tl[3 * f + 2]], hv[3 * tl[3 * f + 2] + 1], hv[3 * tl[3 * f + 2] + 2]};
    const D3 n = unit(cross(sub(b, a), sub(c, a)));
    const D3 ref = fabs(n.x) < 0.9 ? D3{1, 0, 0} : D3{0, 1, 0};
    const D3 x = unit(cross(n, ref)), y = cross(n, x);
    const int s = tl[k], t = tl[(k / 3) * 3 + (k % 3 + 1) % 3];
    const D3 es = {hv[3 * s], hv[3 * s + 1], hv[3 * s + 2]}, et = {hv[3 * t], hv[3 * t + 1], hv[3 * t + 2]};
    const double dx = dot(et, x) - dot(es, x), dy = dot(et, y) - dot(es, y), len = sqrt(dx * dx + dy * dy);
    const double cs = dx / len, sn = dy / len;
    const D3 rows[3] = {{cs * x.x + sn * y.x, cs * x.y + sn * y.y, cs * x.z + sn * y.z},
                        {cs * y.x - sn * x.x, cs * y.y - sn * x.y, cs * y.z - sn * x.z}, n};
    double lo[3], hi[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double l = INFINITY, h = -INFINITY;
      for (int v = lane; v < nv; v += 64) {
        const double d = dot(D3{hv[3 * v], hv[3 * v + 1], hv[3 * v + 2]}, rows[r]);
        l = fmin(l, d); h = fmax(h, d);
      }
      lo[r] = wave_min(l); hi[r] = wave_max(h);
    }
    // ascending extents (stable), right-handed, then the turn about Y: rows (longest, middle, -shortest)
    int o0 = 0, o1 = 1, o2 = 2;
    const double e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
    const double ee[3] = {e0, e1, e2};
    if (ee[o1] < ee[o0]) { const int t2 = o0; o0 = o1; o1 = t2; }
    if (ee[o2] < ee[o1]) { const int t2 = o1; o1 = o2; o2 = t2; }
    if (ee[o1] < ee[o0]) { const int t2 = o0; o0 = o1; o1 = t2; }
    D3 r0 = rows[o0], r1 = rows[o1], r2 = rows[o2];
    double l2 = lo[o2], h2 = hi[o2];
    if (dot(r0, cross(r1, r2)) < 0.0) { r2 = scaled(r2, -1.0); const double t2 = l2; l2 = -h2; h2 = -t2; }
    const double m0 = (lo[o0] + hi[o0]) / 2.0, m1 = (lo[o1] + hi[o1]) / 2.0, m2 = (l2 + h2) / 2.0;
    centre[0] = (r0.x * m0 + r1.x * m1) + r2.x * m2;   // R^T (lo + hi) / 2
    centre[1] = (r0.y * m0 + r1.y * m1) + r2.y * m2;
    centre[2] = (r0.z * m0 + r1.z * m1) + r2.z * m2;
    R[0][0] = r2.x; R[0][1] = r2.y; R[0][2] = r2.z;
    R[1][0] = r1.x; R[1][1] = r1.y; R[1][2] = r1.z;
    R[2][0] = -r0.x; R[2][1] = -r0.y; R[2][2] = -r0.z;
    ext[0] = h2 - l2; ext[1] = hi[o1] - lo[o1]; ext[2] = hi[o0] - lo[o0];
  }
  double s = g.fit == 0 ? g.radius / sqrt(maxr2) : 2.0 * g.radius / ext[0];
  if (!(s < 1.0)) s = 1.0;
  // the transform as stored, and the final vertices from the stored values
  float xf[13];
  xf[0] = (float)s;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) xf[1 + 3 * r + c] = (float)R[r][c];
    xf[10 + r] = (float)((r == 0 ? com.x : r == 1 ? com.y : com.z) + centre[r]);
  }
  for (int v = lane; v < nv; v += 64) {
    const D3 p = ldp(pf, vs[v]);
    const D3 d = {p.x - (double)xf[10], p.y - (double)xf[11], p.z - (double)xf[12]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
      fv[3 * v + r] = (float)((double)xf[0] * (((double)xf[1 + 3 * r] * d.x + (double)xf[2 + 3 * r] * d.y) + (double)xf[3 + 3 * r] * d.z));
  }
  __syncthreads();

  // ---- 5. the outputs, from the final vertices
  double vol6 = 0, sx = 0, sy = 0, sz = 0, mxx = 0, mxy = 0, mxz = 0, myy = 0, myz = 0, mzz = 0;
  for (int t = lane; t < nt; t += 64) {
    const D3 a = ldp(fv, tl[3 * t]), b = ldp(fv, tl[3 * t + 1]), c = ldp(fv, tl[3 * t + 2]);
    const double d = dot(a, cross(b, c));
    vol6 += d;
    sx += ((a.x + b.x) + c.x) * d; sy += ((a.y + b.y) + c.y) * d; sz += ((a.z + b.z) + c.z) * d;
    mxx += moment(a.x, b.x, c.x, a.x, b.x, c.x) * d; mxy += moment(a.x, b.x, c.x, a.y, b.y, c.y) * d;
    mxz += moment(a.x, b.x, c.x, a.z, b.z, c.z) * d; myy += moment(a.y, b.y, c.y, a.y, b.y, c.y) * d;
    myz += moment(a.y, b.y, c.y, a.z, b.z, c.z) * d; mzz += moment(a.z, b.z, c.z, a.z, b.z, c.z) * d;
  }
  vol6 = wave_sum(vol6); sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
  mxx = wave_sum(mxx); mxy = wave_sum(mxy); mxz = wave_sum(mxz); myy = wave_sum(myy); myz = wave_sum(myz); mzz = wave_sum(mzz);
  double fl[3] = {INFINITY, INFINITY, INFINITY}, fh[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int v = lane; v < nv; v += 64) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { fl[r] = fmin(fl[r], (double)fv[3 * v + r]); fh[r] = fmax(fh[r], (double)fv[3 * v + r]); }
  }
  double fe[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) fe[r] = wave_max(fh[r]) - wave_min(fl[r]);

  for (int k = lane; k < MAXV * 3; k += 64) verts[k] = k < 3 * nv ? fv[k] : 0.f;
  for (int k = lane; k < MAXT * 3; k += 64) tris[k] = k < 3 * nt ? tl[k] : 0;
  if (lane == 0) {
    const double volume = vol6 / 6.0;
    const double cx = sx / (4.0 * vol6), cy = sy / (4.0 * vol6), cz = sz / (4.0 * vol6);
    const double rho = g.density_lo + uniform64(philox_word0(g0, g1, DENSITY_DRAW, g.seed, TAG)) * (g.density_hi - g.density_lo);
    // second moments about the centre of mass: C = M / 120 - V c c^T;  I = rho (tr(C) 1 - C)
    const double cxx = mxx / 120.0 - volume * (cx * cx), cyy = myy / 120.0 - volume * (cy * cy), czz = mzz / 120.0 - volume * (cz * cz);
    const double cxy = mxy / 120.0 - volume * (cx * cy), cxz = mxz / 120.0 - volume * (cx * cz), cyz = myz / 120.0 - volume * (cy * cz);
    float* mc = g.mass_com + 4 * (size_t)i;
    mc[0] = (float)(rho * volume); mc[1] = (float)cx; mc[2] = (float)cy; mc[3] = (float)cz;
    float* in = g.inertia + 6 * (size_t)i;
    in[0] = (float)(rho * (cyy + czz)); in[1] = (float)(-(rho * cxy)); in[2] = (float)(-(rho * cxz));
    in[3] = (float)(rho * (cxx + czz)); in[4] = (float)(-(rho * cyz)); in[5] = (float)(rho * (cxx + cyy));
    const double bv = (fe[0] * fe[1]) * fe[2];
    float* me = g.metrics + 4 * (size_t)i;
    me[0] = (float)volume; me[1] = (float)(volume / bv); me[2] = (float)(fmax(fmax(fe[0], fe[1]), fe[2]) / fmin(fmin(fe[0], fe[1]), fe[2]));
    me[3] = (float)bv;
    g.counts[2 * (size_t)i] = nv; g.counts[2 * (size_t)i + 1] = nt;
    g.status[i] = SRL_ROCKS_OK;
  }
  if (lane < 13) g.xform[13 * (size_t)i + lane] = xf[lane];
}

// The parent table: `assets._subdivide` applied three times to the 12 triangles of the box (the new vertices are the unique
// sorted edges, numbered in lexicographic order after the old ones).
const Parents& parents() {
  static const Parents table = [] {
    Parents p = {};
    std::vector<std::array<int, 3>> t = {{0, 1, 3}, {0, 3, 2}, {4, 6, 7}, {4, 7, 5}, {0, 4, 5}, {0, 5, 1},
                                         {2, 3, 7}, {2, 7, 6}, {0, 2, 6}, {0, 6, 4}, {1, 5, 7}, {1, 7, 3}};
    int nv = 8;
    for (int level = 0; level < 3; ++level) {
      std::vector<std::pair<int, int>> e;
      for (const auto& f : t)
        for (int k = 0; k < 3; ++k) e.emplace_back(std::min(f[k], f[(k + 1) % 3]), std::max(f[k], f[(k + 1) % 3]));
      std::sort(e.begin(), e.end());
      e.erase(std::unique(e.begin(), e.end()), e.end());
      auto mid = [&](int a, int b) {
        return nv + (int)(std::lower_bound(e.begin(), e.end(), std::make_pair(std::min(a, b), std::max(a, b))) - e.begin());
      };
      for (size_t k = 0; k < e.size(); ++k) { p.p[nv + k][0] = (uint16_t)e[k].first; p.p[nv + k][1] = (uint16_t)e[k].second; }
      std::vector<std::array<int, 3>> t2(4 * t.size());
      const size_t n = t.size();
      for (size_t k = 0; k < n; ++k) {
        const int a = t[k][0], b = t[k][1], c = t[k][2], ab = mid(a, b), bc = mid(b, c), ca = mid(c, a);
        t2[k] = {a, ab, ca}; t2[n + k] = {ab, b, bc}; t2[2 * n + k] = {ca, bc, c}; t2[3 * n + k] = {ab, bc, ca};
      }
      nv += (int)e.size();
      t.swap(t2);
    }
    return p;
  }();
  return table;
}

int points_of(int subdivisions) { return subdivisions == 0 ? 8 : subdivisions == 1 ? 26 : subdivisions == 2 ? 98 : 386; }
}  // namespace

extern "C" {

const char* srl_rocks_last_error(void) { return r_err; }

#ifndef SRL_BUILD_INFO
#define SRL_BUILD_INFO "SRL_BUILD_INFO<unknown|>"
#endif
const char* srl_rocks_build_info(void) { static const char info[] = SRL_BUILD_INFO; return info; }

int srl_rocks_points(int32_t subdivisions, int32_t* n_points) {
  if (subdivisions < 0 || subdivisions > 3) { SET_ERR("srl_rocks_points: subdivisions must be in 0..3, got %d", subdivisions); return SRL_EINVAL; }
  if (!n_points) { SET_ERR("srl_rocks_points: n_points is null"); return SRL_EINVAL; }
  *n_points = points_of(subdivisions);
  return SRL_OK;
}

int srl_rocks_generate(const srl_rocks_params* p, int64_t first_index, int32_t n, const float* points_in, int32_t n_points_in,
                       float* points_out, float* verts, int32_t* vert_src, int32_t* tris, int32_t* counts, float* mass_com,
                       float* inertia, float* xform, float* metrics, int32_t* status, void* stream) {
  if (!p) { SET_ERR("srl_rocks_generate: the parameters are null"); return SRL_EINVAL; }
  if (n < 1) { SET_ERR("srl_rocks_generate: n must be at least 1, got %d", n); return SRL_EINVAL; }
  if (p->subdivisions < 0 || p->subdivisions > 3) {
    SET_ERR("srl_rocks_generate: subdivisions must be in 0..3, got %d", p->subdivisions);
    return SRL_EINVAL;
  }
  if (!points_in && !(p->irregularity > 0.f && p->irregularity <= 1.f)) {
    SET_ERR("srl_rocks_generate: irregularity must be in (0, 1], got %g", (double)p->irregularity);
    return SRL_EINVAL;
  }
  if (points_in && (n_points_in < 4 || n_points_in > MAXP)) {
    SET_ERR("srl_rocks_generate: given points must number 4..%d a rock, got %d", MAXP, n_points_in);
    return SRL_EINVAL;
  }
  if (!verts || !vert_src || !tris || !counts || !mass_com || !inertia || !xform || !metrics || !status) {
    SET_ERR("srl_rocks_generate: a required output pointer is null (verts, vert_src, tris, counts, mass_com, inertia, xform, "
            "metrics, status)");
    return SRL_EINVAL;
  }
  const double e0 = p->extents[0], e1 = p->extents[1], e2 = p->extents[2], radius = p->radius;
  if (!(radius > 0.0) || !(e0 > 0.0) || !(e1 > 0.0) || !(e2 > 0.0) || (p->fit != 0 && p->fit != 1) ||
      !(p->density_hi >= p->density_lo)) {
    SET_ERR("srl_rocks_generate: radius and extents must be positive, fit 0 or 1, density_hi >= density_lo");
    return SRL_EINVAL;
  }
  Args g = {};
  const double norm = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
  g.half_ext[0] = e0 * 2.0 * radius / norm / 2.0;
  g.half_ext[1] = e1 * 2.0 * radius / norm / 2.0;
  g.half_ext[2] = e2 * 2.0 * radius / norm / 2.0;
  if (!points_in) {
    const double irr = p->irregularity;
    g.scale0 = irr * radius;
    g.bound = 1.0 / irr;
    g.Fa = 0.5 * erfc(g.bound / sqrt(2.0));
    g.Fw = (1.0 - g.Fa) - g.Fa;
  }
  g.radius = radius; g.density_lo = p->density_lo; g.density_hi = p->density_hi;
  g.first_index = first_index;
  g.points_in = points_in; g.points_out = points_out;
  g.verts = verts; g.vert_src = vert_src; g.tris = tris; g.counts = counts;
  g.mass_com = mass_com; g.inertia = inertia; g.xform = xform; g.metrics = metrics; g.status = status;
  g.seed = p->seed;
  g.P = points_in ? n_points_in : points_of(p->subdivisions);
  g.levels = p->subdivisions;
  g.fit = p->fit;
  hipLaunchKernelGGL(k_rocks, dim3(n), dim3(64), 0, (hipStream_t)stream, g, parents());
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { SET_ERR("srl_rocks_generate: %s", hipGetErrorString(e)); return SRL_EHIP; }
  return SRL_OK;
}

}  // extern "C"
