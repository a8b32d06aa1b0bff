// contacts.hip — `Simulator.contact_points` (simulator.py:131-133: pybullet's getContactPoints) of every env, gathered on the
// device.  The definition is in include/stackrl_hip.h ("Contact points"); this file is its kernel.
//
// Nothing is simulated: the ground manifolds (OFF_GM), the pair manifolds (OFF_MAN / OFF_POS) and the poses (OFF_X / OFF_Q)
// persist in every env's blob between steps.  srl_k_contact_points reads them from global memory, puts the points into world
// coordinates and compacts them into rows, one wave of 64 lanes per env:
//   table    lane = manifold slot: the bodies (i | j << 16, pair_word) of every slot in use, to LDS once (one wave: the
//            barrier after it is the only one of the kernel)
//   rows     lane = candidate point, 4 nb ground candidates then 4 NS pair candidates in chunks of 64.  A lane decides
//            whether its candidate is a point (and, with last_only, whether it touches the last body); __ballot and a
//            popcount of the lower lanes give its rank in the chunk, a wave-uniform running base the rank in the env: the
//            order of the definition with no atomics and no barrier.  A lane that holds a row within the capacity makes and
//            stores it with 128-bit vector stores.
//   wrench   lane = body slot: walks the env's points in the same order and sums the force and the torque of its own rows
//            in that order — no atomics, so a loop in the same order gives the same bits.
// Arithmetic: float32, one rounding per written operation (-ffp-contract=off), the fused operations those of srl_device.h
// (mmul_add, madd, cross); R is quat_to_mat, the solver's.
#pragma once
#include "srl_device.h"
#include "srl_kernels.h"

#define SRL_CONTACT_THREADS 64
#define SRL_CONTACT_ROW_WORDS 20   // pa3 pb3 n3 dist fn f1 t1_3 f2 t2_3, 0: five 128-bit stores
#define SRL_CONTACT_WRENCH_WORDS 8 // force xyz, points, torque xyz, 0

// what the kernel reads and writes, by value
struct ContactParams {
  const EnvHdr* hdr;
  const float* blob;        // [n_envs][BLOB]
  const MeshHdr* mh;
  const float4* mv;         // mesh vertices, COM frame
  int32_t BLOB, OFF_X, OFF_Q, OFF_MESH, OFF_GM, OFF_MAN, OFF_POS, NS, NP, L, n_mesh;
  float dt;                 // sim_time_step
  int32_t last_only, capacity;
  int32_t* count;           // [n_envs]
  int32_t* bodies;          // [n_envs][capacity][2]
  float* rows;              // [n_envs][capacity][SRL_CONTACT_ROW_WORDS]
  float* wrench;            // [n_envs][L][SRL_CONTACT_WRENCH_WORDS], or null
};

struct ContactRow {
  int a, b;                 // body slots, b = -1: the ground
  v3 pa, pb, n, t1, t2;
  float dist, fn, f1, f2;
};

// one env's blob as the kernel reads it
struct ContactEnv {
  const ContactParams* C;
  const float* gb;
  const int* gi;
  int nb;
  __device__ __forceinline__ v3 X(int b) const { return ld3(gb + C->OFF_X + 4 * b); }
  __device__ __forceinline__ m3 R(int b) const {
    const float* p = gb + C->OFF_Q + 4 * b;
    q4 q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3];
    return quat_to_mat(q);
  }
  __device__ __forceinline__ int clamp_np(float w) const {   // a manifold's point count, kept inside its four points
    const int n = __float_as_int(w);
    return n < 0 ? 0 : (n > SRL_GMAXP ? SRL_GMAXP : n);
  }
  __device__ __forceinline__ int ground_np(int b) const { return clamp_np(gb[C->OFF_GM + SRL_GM_WORDS * b]); }
  __device__ __forceinline__ int pair_np(int sl) const { return clamp_np(gb[C->OFF_MAN + SRL_MAN_WORDS * sl]); }
};

// ground point k of body b: position on A = the world position of mesh vertex vid as the settle kernel makes it
// (x + R lv), position on B = that point dropped to the plane z = 0, normal +z, directions plane_space(+z)
__device__ __forceinline__ ContactRow ground_row(const ContactEnv& E, int b, int k) {
  const ContactParams& C = *E.C;
  const float* g = E.gb + C.OFF_GM + SRL_GM_WORDS * b;
  ContactRow r;
  r.a = b; r.b = -1;
  int mesh = E.gi[C.OFF_MESH + b];
  mesh = mesh < 0 ? 0 : (mesh >= C.n_mesh ? C.n_mesh - 1 : mesh);
  const MeshHdr mh = C.mh[mesh];
  int vid = __float_as_int(g[SRL_GM_VID + k]);
  vid = vid < 0 ? 0 : (vid >= mh.nv ? mh.nv - 1 : vid);
  const float4 lv = C.mv[mh.vo + vid];
  r.pa = mmul_add(E.R(b), V(lv.x, lv.y, lv.z), E.X(b));
  r.pb = V(r.pa.x, r.pa.y, 0.0f);
  r.n = V(0.0f, 0.0f, 1.0f);
  plane_space(r.n, r.t1, r.t2);
  r.dist = g[SRL_GM_DIST + k];
  r.fn = g[SRL_GM_IN + k] / C.dt; r.f1 = g[SRL_GM_T1 + k] / C.dt; r.f2 = g[SRL_GM_T2 + k] / C.dt;
  return r;
}

// point k of manifold slot sl between bodies i < j: la / lb are in the frames of i / j about their positions (narrowphase_slot:
// mtmul(Ra, sa - xa)), the stored normal is in world coordinates and points from j towards i (gjk_distance: v = a - b; a
// positive normal impulse moves i along +n, make_row / prow_apply), so A = i and B = j, unswapped
__device__ __forceinline__ ContactRow pair_row(const ContactEnv& E, int sl, int i, int j, int k) {
  const ContactParams& C = *E.C;
  const float* q = E.gb + C.OFF_MAN + SRL_MAN_WORDS * sl + 4 + SRL_MP_WORDS * k;
  ContactRow r;
  r.a = i; r.b = j;
  r.pa = mmul_add(E.R(i), ld3(q), E.X(i));
  r.pb = mmul_add(E.R(j), ld3(q + 3), E.X(j));
  r.n = ld3(q + 6);
  plane_space(r.n, r.t1, r.t2);
  r.dist = q[9];
  r.fn = q[10] / C.dt; r.f1 = q[11] / C.dt; r.f2 = q[12] / C.dt;
  return r;
}

__device__ __forceinline__ void contact_store(const ContactRow& r, int32_t* bodies, float* row) {
  *reinterpret_cast<int2*>(bodies) = make_int2(r.a, r.b);
  float4* o = reinterpret_cast<float4*>(row);
  o[0] = make_float4(r.pa.x, r.pa.y, r.pa.z, r.pb.x);
  o[1] = make_float4(r.pb.y, r.pb.z, r.n.x, r.n.y);
  o[2] = make_float4(r.n.z, r.dist, r.fn, r.f1);
  o[3] = make_float4(r.t1.x, r.t1.y, r.t1.z, r.f2);
  o[4] = make_float4(r.t2.x, r.t2.y, r.t2.z, 0.0f);
}

// a body's share of a row: the force on it (+F on A, -F on B, F = fn n + f1 t1 + f2 t2) and its torque about the body's position
struct Wrench { v3 f, t; int n; };
__device__ __forceinline__ void wrench_add(Wrench& w, const ContactRow& r, bool is_a, v3 x) {
  v3 F = madd(madd(r.n * r.fn, r.t1, r.f1), r.t2, r.f2);
  if (!is_a) F = neg(F);
  // (value selects per component: a select between the two members became a load at a computed scratch offset)
  const v3 arm = V(is_a ? r.pa.x : r.pb.x, is_a ? r.pa.y : r.pb.y, is_a ? r.pa.z : r.pb.z) - x;
  w.f = w.f + F;
  w.t = w.t + cross(arm, F);
  w.n += 1;
}

extern "C" __global__ void __launch_bounds__(SRL_CONTACT_THREADS) srl_k_contact_points(ContactParams C) {
  __shared__ int slot_pair[SRL_NSLOT_MAX];   // bodies i | j << 16 of a manifold slot in use, -1 otherwise
  const int e = blockIdx.x, lane = threadIdx.x;
  ContactEnv E;
  E.C = &C;
  E.gb = C.blob + (size_t)e * C.BLOB;
  E.gi = reinterpret_cast<const int*>(E.gb);
  {
    const int nb = C.hdr[e].nb;
    E.nb = nb < 0 ? 0 : (nb > C.L ? C.L : nb);
  }
  const int nb = E.nb, NS = C.NS < SRL_NSLOT_MAX ? C.NS : SRL_NSLOT_MAX;
  for (int sl = lane; sl < NS; sl += SRL_CONTACT_THREADS) {
    const int pid = E.gi[C.OFF_POS + sl];
    slot_pair[sl] = pid >= 0 && pid < C.NP ? pair_word(pid) : -1;   // (pid < NP: both bodies are below episode_length)
  }
  __syncthreads();

  // ---- rows
  const int last = nb - 1;
  const int n_cand = 4 * nb + 4 * NS;
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0;                              // wave-uniform: rows kept by the chunks before this one
  for (int c0 = 0; c0 < n_cand; c0 += SRL_CONTACT_THREADS) {
    const int c = c0 + lane;
    const bool ground = c < 4 * nb;
    const int k = c & 3;
    int i = 0, j = -1, sl = 0;
    bool keep = false;
    if (ground) {
      i = c >> 2;
      keep = k < E.ground_np(i);
    } else if (c < n_cand) {
      sl = (c - 4 * nb) >> 2;
      const int w = slot_pair[sl];
      if (w >= 0) { i = w & 0xffff; j = w >> 16; keep = k < E.pair_np(sl); }
    }
    if (C.last_only) keep = keep && (i == last || j == last);
    const unsigned long long mask = __ballot(keep);
    const int at = base + __popcll(mask & below);
    if (keep && at < C.capacity) {
      const ContactRow r = ground ? ground_row(E, i, k) : pair_row(E, sl, i, j, k);
      const size_t o = (size_t)e * C.capacity + at;
      contact_store(r, C.bodies + 2 * o, C.rows + SRL_CONTACT_ROW_WORDS * o);
    }
    base += __popcll(mask);
  }
  if (lane == 0) C.count[e] = base;

  // ---- wrench: lane = body slot, every contact of the env whatever capacity and last_only say
  if (C.wrench && lane < C.L) {
    Wrench w; w.f = V(0.0f, 0.0f, 0.0f); w.t = V(0.0f, 0.0f, 0.0f); w.n = 0;
    if (lane < nb) {
      const v3 x = E.X(lane);
      const int gn = E.ground_np(lane);
      for (int k = 0; k < gn; ++k) wrench_add(w, ground_row(E, lane, k), true, x);
      for (int sl = 0; sl < NS; ++sl) {
        const int pw = slot_pair[sl];
        if (pw < 0) continue;
        const int i = pw & 0xffff, j = pw >> 16;
        if (i != lane && j != lane) continue;
        const int pn = E.pair_np(sl);
        for (int k = 0; k < pn; ++k) wrench_add(w, pair_row(E, sl, i, j, k), i == lane, x);
      }
    }
    float4* o = reinterpret_cast<float4*>(C.wrench + ((size_t)e * C.L + lane) * SRL_CONTACT_WRENCH_WORDS);
    o[0] = make_float4(w.f.x, w.f.y, w.f.z, (float)w.n);
    o[1] = make_float4(w.t.x, w.t.y, w.t.z, 0.0f);
  }
}
