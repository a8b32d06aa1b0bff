// env_host.h — the host arithmetic of libstackrl_hip.so (stackrl_hip.hip): derived constants, the settle kernel's variant
// choice, the LDS / blob / state-record layouts and the mesh table's preprocessing.  No HIP runtime call is made here (only
// HIP's vector types are used), so tests/host/env_host_main.hip runs all of it on a CPU.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>
#include "stage.h"   // StageLds, SRL_STAGE_STRIDE and, through srl_device.h / srl_kernels.h, the word counts and DevParams

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* arg = "") {
  snprintf(g_err, sizeof g_err, fmt, arg);
  return code;
}

// settle.hip's M_WORDS and solver.h's SRL_CG_WORDS, which are defined among device code: stackrl_hip.hip asserts the equality
constexpr int HOST_M_WORDS = 20, HOST_CG_WORDS = 20;

// Manifold slots per env: every pair up to 8 rocks (28), 64 up to 16 rocks, 128 above — one contact point per thread in
// every kernel variant (4 lanes per slot).  Pairs whose AABBs overlap at the same time: at most 36 over 512 random
// 16-rock episodes, 85 over 24 32-rock ones (the oracle's statistics); an env that needs more reports
// SRL_ST_PAIR_OVERFLOW and srl_sync_status fails, as it did at the old cap of 192.
int nslots(int L) {
  int np = L * (L - 1) / 2;
  if (np < 1) np = 1;
  const int cap = L <= 16 ? 64 : 128;
  return np < cap ? np : cap;
}

// derived constants: identical expressions to the oracle's derive() so both sides round alike
int derive(DevParams& P) {
  srl_config& c = P.c;
  if (c.n_envs < 1 || c.episode_length < 1 || c.episode_length > SRL_MAX_BODIES)
    return fail(SRL_EINVAL, "n_envs/episode_length out of range");
  if (c.overhead_res < c.object_res || c.object_res < 2 || c.overhead_res > 256 || (c.overhead_res % 8) != 0)
    return fail(SRL_EINVAL, "bad resolutions (overhead_res must be a multiple of 8, <= 256)");
  if (c.metric < 0 || c.metric > SRL_METRIC_EVAL) return fail(SRL_EINVAL, "Invalid value for argument metric");
  if (c.obs_dtype < SRL_DTYPE_UINT8 || c.obs_dtype > SRL_DTYPE_FLOAT64) return fail(SRL_EINVAL, "Invalid value for argument dtype.");
  P.px = c.object_max_dimension / (float)c.object_res;
  P.inv_px = (float)c.object_res / c.object_max_dimension;
  P.lin_damp = (float)pow(1.0 - (double)c.linear_damping, (double)c.sim_time_step);
  P.ang_damp = (float)pow(1.0 - (double)c.angular_damping, (double)c.sim_time_step);
  // simulator.py:46 int(MAX_STEP_TIME / time_step).  The host mirror passes the value computed from its double (config.py);
  // for a C caller the quotient of the float32 time step is nudged by 1e-6 of itself so that 0.0125f (23999.9996) gives
  // the reference's 24000
  P.max_substeps = c.max_substeps > 0 ? c.max_substeps : (int)(300.0 / (double)c.sim_time_step * (1.0 + 1e-6));
  int H = c.overhead_res, h = c.object_res;
  P.goal_min_h = h; P.goal_min_w = h; P.goal_max_h = H; P.goal_max_w = H;   // rewarder.py:65-80
  P.goal_size = (int)((double)c.goal_size_ratio * H * H);
  if (P.goal_size <= 0) return fail(SRL_EINVAL, "goal_size_ratio must be a scalar in (0,1]");
  if (P.goal_size / P.goal_max_w > P.goal_min_h) P.goal_min_h = P.goal_size / P.goal_max_w;
  if (P.goal_size / P.goal_min_w < P.goal_max_h) P.goal_max_h = P.goal_size / P.goal_min_w;
  P.goal_z = c.max_z - c.object_max_dimension;                                 // observer.py:378-382
  P.scale = c.reward_scale > 0.0f ? c.reward_scale : (float)c.episode_length;  // rewarder.py:97
  P.AW = H - h + 1;                                                            // env.py:207-211
  P.A = P.AW * P.AW;
  if (c.orientation_freedom < 0 || (1 << c.orientation_freedom) > SRL_MAX_ORIENT)
    return fail(SRL_EINVAL, "orientation_freedom must be in 0..4");
  P.n_orient = 1 << c.orientation_freedom;                                     // observer.py:127
  if (c.ordering_freedom != 0 && c.ordering_freedom != 1) return fail(SRL_EINVAL, "ordering_freedom must be 0 or 1");
  P.n_slots = c.ordering_freedom ? c.episode_length * P.n_orient : P.n_orient;  // env.py:472-480
  for (int i = 0; i < P.n_orient; ++i) {   // inverse of getQuaternionFromEuler([0, 0, i 2 pi / n]) (observer.py:129-139)
    const double half = -0.5 * ((double)i * 2.0 * 3.14159265358979323846 / (double)P.n_orient);
    P.orient_q[i][0] = 0.0f; P.orient_q[i][1] = 0.0f;
    P.orient_q[i][2] = i == 0 ? 0.0f : (float)sin(half); P.orient_q[i][3] = i == 0 ? 1.0f : (float)cos(half);
  }
  // observer.py:259-260 / :274-275 constants, rounded to float32 the way numpy rounds python scalars
  double oz = (double)c.object_max_dimension;
  P.elev_num = (float)((double)SRL_FAR * ((double)SRL_FAR - (double)c.max_z));
  P.obj_c1 = (float)((double)SRL_FAR + oz / 2);
  P.obj_c2 = (float)((double)SRL_FAR * (double)SRL_FAR - (oz / 2) * (oz / 2));
  return SRL_OK;
}

// 9 - 16 rocks in batches of 3,072 envs or more run two waves per env with two contact points per thread and without
// the LDS copy of the local vertices: 35 KB per env, so four workgroups share a CU instead of three — these batches are
// throughput-bound (+6 % at 4,096 envs: 47.5 against 50.6 ms per launch; -1 % at 2,048, -6 % at 1,024, where the launch
// lasts as long as its slowest env).  What counts is the number of envs that step on the device at the same time: a
// caller that splits its batch over several handles says so with srl_set_concurrent_envs (`concurrent`, 0 = this handle
// alone).  SRL_STEP_VARIANT=two_wave | four_wave overrides the choice (parity tests).
bool two_wave_variant(const DevParams& P, int concurrent) {
  const char* v = getenv("SRL_STEP_VARIANT");
  if (v && !strcmp(v, "two_wave")) return true;
  if (v && !strcmp(v, "four_wave")) return false;
  return (concurrent > P.c.n_envs ? concurrent : P.c.n_envs) >= 3072;
}

// The settle kernel's variants (settle.hip "Variants"): <waves per env>W_PP<pair-manifold points per thread>, one row each
// (the kernel of each row: k_step_kernels, stackrl_hip.hip).  `reports` is what srl_get_step_variant says of the kernel;
// `lds_verts`: the env's LDS holds a copy of its bodies' local vertices (without it they are read from the L2-resident
// mesh table: 70 instead of 97 KB per env above 16 rocks, so that two workgroups share a CU).
enum StepVariant { STEP_2W_PP1 = 0, STEP_4W_PP1, STEP_4W_PP2, STEP_2W_PP2, STEP_VARIANTS };
struct StepRow { int threads, pp, reports; bool lds_verts; };
const StepRow k_step_variants[STEP_VARIANTS] = {
    /* STEP_2W_PP1: up to 8 rocks          */ {128, 1, 0, true},
    /* STEP_4W_PP1: 9 - 16 rocks           */ {256, 1, 1, true},
    /* STEP_4W_PP2: above 16 rocks         */ {256, 2, 2, false},
    /* STEP_2W_PP2: 9 - 16, large batches  */ {128, 2, 3, false},
};

// one contact point of the pair manifolds per thread where the slots allow it (4 lanes per slot, SRL_GMAXP per body)
StepVariant step_variant_of(const DevParams& P, int concurrent) {
  const int L = P.c.episode_length, NS = nslots(L);
  if (4 * NS <= 128 && SRL_GMAXP * L <= 128) return STEP_2W_PP1;
  if (4 * NS > 256) return STEP_4W_PP2;
  return two_wave_variant(P, concurrent) ? STEP_2W_PP2 : STEP_4W_PP1;
}

void layout(DevParams& P, int concurrent) {
  int L = P.c.episode_length;
  const StepRow& sv = k_step_variants[step_variant_of(P, concurrent)];
  P.NS = nslots(L);
  P.NP = L * (L - 1) / 2 > 0 ? L * (L - 1) / 2 : 1;
  int o = 0;
  // xyz vectors are stored with a stride of 4 words so that the kernels move them with 16-byte LDS accesses
  // a body's velocities interleaved, 8 words per body: (v.x, w.x, v.y, w.y, v.z, w.z, -, -) — settle.hip Lds::VW
  P.OFF_V = o; P.OFF_W = o + 1; o += 8 * L;
  P.OFF_X = o; o += 4 * L;
  P.OFF_Q = o; o += 4 * L;
  P.OFF_PX = o; o += 4 * L;
  P.OFF_PQ = o; o += 4 * L;
  P.OFF_MESH = o; o += L;
  P.OFF_GM = o; o += SRL_GM_WORDS * L;
  P.OFF_MAN = o; o += SRL_MAN_WORDS * P.NS;
  P.OFF_SOP = o; o += P.NP;
  P.OFF_POS = o; o += P.NS;
  P.OFF_COL = o; o += P.NS;
  P.BLOB = (o + 3) & ~3;
  int s = 0;
  P.S_R = s; s += 9 * L;
  P.S_IW = s; s += 9 * L;
  P.S_AMIN = s; s += 3 * L;
  P.S_AMAX = s; s += 3 * L;
  P.S_BC = s; s += 8 * L;
  // (during the solve the region holds the ground points' row constants instead: SRL_GMAXP x SRL_CG_WORDS words per body)
  P.S_WV = s; s += (3 * P.VS > SRL_GMAXP * HOST_CG_WORDS ? 3 * P.VS : SRL_GMAXP * HOST_CG_WORDS) * L;
  if (sv.lds_verts) { P.S_LV = s; s += 3 * P.VS * L; } else P.S_LV = -1;
  // the tail of the settle kernels stages the env's rocks for the render kernel (stage.h): one StageLds per wave, laid over
  // the scratch words above, which are dead by then — the words below (colouring scratch, misc, pair table) are not
  {
    const int waves = sv.threads / 64;
    const int need = waves * (int)(sizeof(StageLds) / sizeof(float));
    if (s < need) s = need;
  }
  s = (s + 1) & ~1;
  P.S_USED = s; s += 2 * SRL_MAX_BODIES;   // colouring scratch (uint64 per body); BLOB is a multiple of 4 words
  P.S_MISC = s; s += HOST_M_WORDS;
  P.S_PAIR = s; s += P.NP;                 // pair id -> (i | j << 16), filled once per launch (settle.hip pair_word)
  P.LDS_WORDS = P.BLOB + s;
}

// FNV-1a over bytes, chained through `h` (the state signature and the mesh table's hash)
uint64_t fnv1a(const void* data, size_t bytes, uint64_t h = 0xcbf29ce484222325ull) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
  return h;
}

// The state record of one env (state.hip) in 32-bit words: EnvHdr, the blob, the height map, the staged records, each part
// on a multiple of 4 words.  Host arithmetic on a configuration alone; P needs derive() and layout() done.
struct StateLayout { int64_t words, off[4], size[4]; };
StateLayout state_layout(const DevParams& P) {
  StateLayout s;
  s.size[0] = ((int64_t)(sizeof(EnvHdr) / sizeof(int32_t)) + 3) & ~(int64_t)3;
  s.size[1] = P.BLOB;                                                      // a multiple of 4 (layout)
  s.size[2] = (int64_t)P.c.overhead_res * P.c.overhead_res;                // overhead_res is a multiple of 8 (derive)
  s.size[3] = (int64_t)P.c.episode_length * SRL_STAGE_STRIDE * 4;
  s.words = 0;
  for (int k = 0; k < 4; ++k) { s.off[k] = s.words; s.words += s.size[k]; }
  return s;
}

// the parameters of a configuration before any mesh is loaded: derive() and the layout at the smallest vertex stride
int host_params(const srl_config& cfg, DevParams& P) {
  memset(&P, 0, sizeof P);
  P.c = cfg; P.VS = 4;
  const int rc = derive(P);
  if (!rc) layout(P, 0);
  return rc;
}

// every pixel of an object map with no rock in view = elev_object(1.0), evaluated like the kernel does
float empty_object_elevation(const DevParams& P) {
  return P.obj_c1 - P.obj_c2 / (SRL_FAR + P.c.object_max_dimension * (0.5f - 1.0f));
}

// The device mesh table as srl_load_meshes uploads it: headers, COM-frame vertices, triangles, face planes and the edge
// list, with the vertex stride (the largest vertex count, at least 4) and the hash of the arrays it was made from.
struct MeshTable {
  std::vector<MeshHdr> mh; std::vector<float4> mv, mp; std::vector<uchar4> mt, me;
  int vs = 4; uint64_t hash = 0;
  int build(const float* verts, const int32_t* vert_off, const int32_t* tris, const int32_t* tri_off, const float* mass_com, int32_t n_mesh);
};

// `verts` / `tris` are indexed through the caller's offsets, and only after the offsets of the mesh in question have been
// checked: a first offset >= 0 and counts >= 4 keep every later offset inside what the caller says the arrays hold.
int MeshTable::build(const float* verts, const int32_t* vert_off, const int32_t* tris, const int32_t* tri_off, const float* mass_com,
                     int32_t n_mesh) {
  if (vert_off[0] < 0 || tri_off[0] < 0) return fail(SRL_EINVAL, "mesh offsets must not be negative");
  *this = MeshTable();
  mh.resize((size_t)n_mesh);
  for (int m = 0; m < n_mesh; ++m) {
    MeshHdr& M = mh[m];
    M.vo = vert_off[m]; M.nv = vert_off[m + 1] - vert_off[m];
    M.to = tri_off[m]; M.nt = tri_off[m + 1] - tri_off[m];
    if (M.nv < 4 || M.nv > SRL_MAX_VERTS || M.nt < 4 || M.nt > SRL_MAX_TRIS)
      return fail(SRL_EINVAL, "mesh exceeds SRL_MAX_VERTS/SRL_MAX_TRIS");
    mv.resize((size_t)M.vo + M.nv); mt.resize((size_t)M.to + M.nt); mp.resize((size_t)M.to + M.nt);
    if (M.nv > vs) vs = M.nv;
    float mass = mass_com[4 * m];
    M.cx = mass_com[4 * m + 1]; M.cy = mass_com[4 * m + 2]; M.cz = mass_com[4 * m + 3];
    float lox = 1e30f, loy = 1e30f, loz = 1e30f, hix = -1e30f, hiy = -1e30f, hiz = -1e30f, r2 = 0.0f;
    for (int k = 0; k < M.nv; ++k) {
      const float* p = verts + 3 * (size_t)(M.vo + k);
      float ax = p[0] - M.cx, ay = p[1] - M.cy, az = p[2] - M.cz;   // COM frame
      mv[(size_t)M.vo + k] = make_float4(ax, ay, az, 0.0f);
      lox = fminf(lox, ax); loy = fminf(loy, ay); loz = fminf(loz, az);
      hix = fmaxf(hix, ax); hiy = fmaxf(hiy, ay); hiz = fmaxf(hiz, az);
      float d2 = fmaf(ax, ax, fmaf(ay, ay, az * az));   // dot(a, a) as the kernels define it
      if (d2 > r2) r2 = d2;
    }
    M.radius = sqrtf(r2);
    for (int k = 0; k < M.nt; ++k) {
      const int32_t* t = tris + 3 * (size_t)(M.to + k);
      for (int j = 0; j < 3; ++j)
        if (t[j] < 0 || t[j] >= M.nv) return fail(SRL_EINVAL, "triangle index out of range");
      mt[(size_t)M.to + k] = make_uchar4((unsigned char)t[0], (unsigned char)t[1], (unsigned char)t[2], 0);
      // face plane in the COM frame: unit normal and offset (same expression order as the solver's dot/cross)
      const float4 a = mv[(size_t)M.vo + t[0]], b = mv[(size_t)M.vo + t[1]], c = mv[(size_t)M.vo + t[2]];
      float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
      float nx = fmaf(uy, wz, -(uz * wy)), ny = fmaf(uz, wx, -(ux * wz)), nz = fmaf(ux, wy, -(uy * wx));   // cross
      float len = sqrtf(fmaf(nx, nx, fmaf(ny, ny, nz * nz)));
      if (!(len > 0.0f)) return fail(SRL_EINVAL, "degenerate triangle");
      float il = 1.0f / len;
      nx = nx * il; ny = ny * il; nz = nz * il;
      mp[(size_t)M.to + k] = make_float4(nx, ny, nz, fmaf(nx, a.x, fmaf(ny, a.y, nz * a.z)));
    }
    {   // edge list of the closed triangulated surface (the renderer's silhouette test): edge (a < b) -> its two faces
      std::vector<int> first((size_t)M.nv * M.nv, -1);
      M.eo = (int32_t)me.size();
      for (int k = 0; k < M.nt; ++k) {
        const int32_t* t = tris + 3 * (size_t)(M.to + k);
        for (int j = 0; j < 3; ++j) {
          int a = t[j], b = t[(j + 1) % 3];
          if (a > b) { int tmp = a; a = b; b = tmp; }
          if (a == b) return fail(SRL_EINVAL, "degenerate triangle");
          int& slot = first[(size_t)a * M.nv + b];
          if (slot == -1) slot = k;
          else if (slot >= 0) {
            me.push_back(make_uchar4((unsigned char)a, (unsigned char)b, (unsigned char)slot, (unsigned char)k));
            slot = -2;
          } else return fail(SRL_EINVAL, "mesh is not a closed two-manifold (an edge has more than two faces)");
        }
      }
      for (size_t q = 0; q < first.size(); ++q)
        if (first[q] >= 0) return fail(SRL_EINVAL, "mesh is not a closed surface (an edge has only one face)");
      M.ne = (int32_t)me.size() - M.eo;
    }
    // Bullet's default for hull shapes when the URDF inertia is not requested (simulator.py:300 passes no
    // flags): inertia of the solid box spanned by the AABB (btCompoundShape::calculateLocalInertia restated)
    float lx = hix - lox, ly = hiy - loy, lz = hiz - loz;
    float k12 = mass / 12.0f;
    float Ix = k12 * (ly * ly + lz * lz), Iy = k12 * (lx * lx + lz * lz), Iz = k12 * (lx * lx + ly * ly);
    M.inv_mass = 1.0f / mass;
    M.iix = 1.0f / Ix; M.iiy = 1.0f / Iy; M.iiz = 1.0f / Iz;
  }
  // the table's contents as one number: records of another pool are refused (srl_state_set)
  uint64_t h = fnv1a(&n_mesh, sizeof n_mesh);
  h = fnv1a(vert_off, sizeof(int32_t) * ((size_t)n_mesh + 1), h);
  h = fnv1a(verts, sizeof(float) * 3 * (size_t)vert_off[n_mesh], h);
  h = fnv1a(tri_off, sizeof(int32_t) * ((size_t)n_mesh + 1), h);
  h = fnv1a(tris, sizeof(int32_t) * 3 * (size_t)tri_off[n_mesh], h);
  hash = fnv1a(mass_com, sizeof(float) * 4 * (size_t)n_mesh, h);
  return SRL_OK;
}

}  // namespace
