// push.hip — the three device hooks of a push test (include/stackrl_hip.h "Push test"): the poses of every pile
// (`Simulator.poses`, simulator.py:85-93), a velocity increment for its bodies, and how far they have moved since
// (`Simulator.distances`, simulator.py:95-111, and `distances_from_place`, :113-128).  The header holds the definition; this
// file is its kernels.
//
// Nothing is simulated here: a push is srl_poses -> srl_kick -> srl_step_simulation -> srl_pose_distances, and the sub-steps are
// the settle kernel's.  All three kernels run one wave of 64 lanes per env, lane = body slot (episode_length is at most
// SRL_MAX_BODIES = 32), and move a body's words with 128-bit accesses: its position (x y z -), its quaternion and its
// interleaved velocities (v.x w.x v.y w.y | v.z w.z - -) each start on a multiple of 4 words of a blob that is itself a multiple
// of 4 words long (csrc/env_host.h layout).
//   poses      a lane gathers its body's two rows of four words; lane 0 writes the count.
//   kick       a selected lane below nb loads its body's eight velocity words, adds its increment to six of them (one float32
//              add each) and stores the eight; the two spare words go back as they came.
//   distances  a lane makes its body's row (perr, oerr, dz, speed) with the arithmetic of the reward's body_discount
//              (render.hip) and stores it; then the wave walks the slots below nb in order, every lane reading slot b's values
//              with a shuffle, so that the summary is the one a loop in slot order gives — no atomics, no barrier — and lane 0
//              stores its eight words.
// Arithmetic: float32, one rounding per written operation (-ffp-contract=off); the fused operation is dot of srl_device.h.
#pragma once
#include "../../include/stackrl_hip.h"   // SRL_KICK_ALL, SRL_KICK_LAST
#include "srl_device.h"
#include "srl_kernels.h"

#define SRL_PUSH_THREADS 64
#define SRL_PUSH_ROW_WORDS 4       // perr oerr dz speed: one 128-bit store
#define SRL_PUSH_SUMMARY_WORDS 8   // nb moved max_perr max_oerr | sum_perr min_dz max_speed max_spin: two 128-bit stores
static_assert(SRL_MAX_BODIES <= SRL_PUSH_THREADS, "lane = body slot");

// what the kernels read and write, by value
struct PushParams {
  const EnvHdr* hdr;
  float* blob;              // [n_envs][BLOB]
  int32_t BLOB, OFF_X, OFF_Q, OFF_V, OFF_PX, OFF_PQ, OFF_MESH, L;
};

// the header's nb, kept inside the env's slots
__device__ __forceinline__ int push_nb(const PushParams& C, int e) {
  const int nb = C.hdr[e].nb;
  return nb < 0 ? 0 : (nb > C.L ? C.L : nb);
}
__device__ __forceinline__ float4 push_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

extern "C" __global__ void __launch_bounds__(SRL_PUSH_THREADS) srl_k_poses(PushParams C, float* poses, int32_t* n_bodies) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int nb = push_nb(C, e);
  if (lane == 0) n_bodies[e] = nb;
  if (lane >= C.L) return;
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
  if (lane < nb) {
    const float* gb = C.blob + (size_t)e * C.BLOB;
    const float4 x = push_ld4(gb + C.OFF_X + 4 * lane), q = push_ld4(gb + C.OFF_Q + 4 * lane);
    a = make_float4(x.x, x.y, x.z, q.x);
    b = make_float4(q.y, q.z, q.w, gb[C.OFF_MESH + lane]);   // (the mesh id's int32 word, moved as it is)
  }
  float4* o = reinterpret_cast<float4*>(poses + ((size_t)e * C.L + lane) * 8);
  o[0] = a; o[1] = b;
}

extern "C" __global__ void __launch_bounds__(SRL_PUSH_THREADS) srl_k_kick(PushParams C, const float* dv, int per_body, int select) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int nb = push_nb(C, e);
  const int target = select == SRL_KICK_ALL ? lane : (select == SRL_KICK_LAST ? nb - 1 : select);
  if (lane >= nb || lane != target) return;                  // (nb <= L: the lane's words are the env's own)
  const float* d = dv + (per_body ? ((size_t)e * C.L + lane) * 8 : (size_t)e * 8);
  const float4 lin = push_ld4(d), ang = push_ld4(d + 4);
  float4* vw = reinterpret_cast<float4*>(C.blob + (size_t)e * C.BLOB + C.OFF_V + 8 * lane);
  float4 a = vw[0], b = vw[1];
  a.x = a.x + lin.x; a.y = a.y + ang.x; a.z = a.z + lin.y; a.w = a.w + ang.y;
  b.x = b.x + lin.z; b.y = b.y + ang.z;
  vw[0] = a; vw[1] = b;
}

extern "C" __global__ void __launch_bounds__(SRL_PUSH_THREADS) srl_k_pose_distances(PushParams C, const float* ref, const int32_t* ref_nb,
                                                                                float tol_p, float tol_o, float* rows,
                                                                                float* summary) {
  const int e = blockIdx.x, lane = threadIdx.x;
  const int nb = push_nb(C, e);
  float perr = 0.0f, oerr = 0.0f, dz = 0.0f, speed = 0.0f, spin = 0.0f;
  if (lane < nb) {
    const float* gb = C.blob + (size_t)e * C.BLOB;
    const float4 x = push_ld4(gb + C.OFF_X + 4 * lane), q = push_ld4(gb + C.OFF_Q + 4 * lane);
    v3 rx; float a[4];
    if (ref && (!ref_nb || lane < ref_nb[e])) {
      const float* r = ref + ((size_t)e * C.L + lane) * 8;
      const float4 r0 = push_ld4(r), r1 = push_ld4(r + 4);
      rx = V(r0.x, r0.y, r0.z); a[0] = r0.w; a[1] = r1.x; a[2] = r1.y; a[3] = r1.z;
    } else {                // the place pose: no reference, or a body the reference does not hold yet (simulator.py:227-237)
      const float4 p = push_ld4(gb + C.OFF_PX + 4 * lane), pq = push_ld4(gb + C.OFF_PQ + 4 * lane);
      rx = V(p.x, p.y, p.z); a[0] = pq.x; a[1] = pq.y; a[2] = pq.z; a[3] = pq.w;
    }
    // body_discount (render.hip): the same subtraction order, dot, grouping, fabsf, fminf, acos polynomial
    const v3 dp = rx - V(x.x, x.y, x.z);
    perr = sqrtf(dot(dp, dp));
    const float dw = fabsf((a[0] * q.x + a[1] * q.y) + (a[2] * q.z + a[3] * q.w));
    oerr = 2.0f * srl_acosf(fminf(dw, 1.0f));
    dz = x.z - rx.z;
    const float4 v0 = push_ld4(gb + C.OFF_V + 8 * lane), v1 = push_ld4(gb + C.OFF_V + 8 * lane + 4);
    const v3 v = V(v0.x, v0.z, v1.x), w = V(v0.y, v0.w, v1.y);
    speed = sqrtf(dot(v, v));
    spin = sqrtf(dot(w, w));
  }
  if (lane < C.L) *reinterpret_cast<float4*>(rows + ((size_t)e * C.L + lane) * SRL_PUSH_ROW_WORDS) = make_float4(perr, oerr, dz, speed);
  // ---- summary: the slots below nb in order (nb is wave-uniform: every lane takes every shuffle)
  float moved = 0.0f, max_p = 0.0f, max_o = 0.0f, sum_p = 0.0f, min_dz = 0.0f, max_v = 0.0f, max_w = 0.0f;
  for (int b = 0; b < nb; ++b) {
    const float p = __shfl(perr, b), o = __shfl(oerr, b);
    if (!(p <= tol_p && o <= tol_o)) moved = moved + 1.0f;   // (a NaN compares false: moved)
    max_p = fmaxf(max_p, p); max_o = fmaxf(max_o, o);
    sum_p = sum_p + p;
    min_dz = fminf(min_dz, __shfl(dz, b));
    max_v = fmaxf(max_v, __shfl(speed, b)); max_w = fmaxf(max_w, __shfl(spin, b));
  }
  if (lane == 0) {
    float4* o = reinterpret_cast<float4*>(summary + (size_t)e * SRL_PUSH_SUMMARY_WORDS);
    o[0] = make_float4((float)nb, moved, max_p, max_o);
    o[1] = make_float4(sum_p, min_dz, max_v, max_w);
  }
}
