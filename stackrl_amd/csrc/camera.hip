// camera.hip — the pile itself in perspective, for a batch, on the device: srl_render_camera (include/stackrl_hip.h holds
// the definition: scene, camera, rock hit, ground and sky, shading, uint8).  Rocks are convex hulls, so a ray meets one by
// clipping against its face planes: no acceleration structure, no triangles.
//
// srl_k_camera: a workgroup of 256 threads owns a tile of 32 x 8 pixels of one env; a wave owns two rows of the tile (lane =
// row << 5 | column), so its stores are two contiguous runs: 2 x 96 bytes of rgb, 2 x 128 bytes of depth and of ids.
// Images that are no multiple of the tile take the same path with masked lanes (they cast no ray, vote for nothing and
// store nothing).
//   bodies   pose, bounding sphere (radius about the centre of mass, widened by 5 % + 0.1 mm) and face range of every body
//            into LDS, one thread per body
//   votes    per wave, per body: may any of my rays meet its sphere?  One test per lane (the squared distance of the centre
//            from the ray's line against the squared radius, with 1e-5 of the compared products on top: hundreds of float32
//            roundings) and one wave-wide vote; the waves' masks meet in LDS.  The test is conservative, so skipping a
//            body never changes a result — a ray that misses the sphere misses the hull inside it.
//   chunks   the bodies some wave asked for are staged SRL_CAM_CHUNK at a time: a thread per face turns the plane into the
//            world frame ONCE per workgroup — (nw, dw) as one float4, and beside it what depends on the face alone:
//            dw - dot(nw, eye), the numerator of every ray from the eye, and dot(nw, light), the denominator of every shadow
//            ray — 24 bytes a face, 18 KB a chunk, so that eight workgroups share a CU (all 32 bodies at 252 faces would be 129 KB
//            and more, and pin a CU to one workgroup).
//            Lanes then sweep the faces of the bodies their wave voted for: every lane reads the same address (LDS
//            broadcast, 128 + 64 bits a face), two dot products less per face than from the definition's text, same bits.
//   shadows  a second round of votes (the ray from the hit point towards the light) and sweeps; bodies still staged from the
//            last chunk are swept where they lie, the others are staged again; a lane leaves at its first blocker and a
//            wave skips what no lane of it still needs.
// No atomics, no scratch, plain vector stores.  The arithmetic is the definition's, operation for operation (the library is
// built with -ffp-contract=off and IEEE division), so ids, faces and depths do not depend on tiles, chunks or votes.
#pragma once
#include "../../include/stackrl_hip.h"
#include "srl_device.h"
#include "srl_kernels.h"
#include "view.hip"   // view_byte: the uint8 rule

#define SRL_CAM_THREADS 256
#define SRL_CAM_WAVES (SRL_CAM_THREADS / 64)
#define SRL_CAM_TW 32
#define SRL_CAM_TH 8
#define SRL_CAM_CHUNK 3
#define SRL_CAM_MAX_SIDE 1024
static_assert(SRL_CAM_TW * SRL_CAM_TH == SRL_CAM_THREADS && SRL_CAM_TW == 32, "lane = row << 5 | column");
static_assert(SRL_MAX_TRIS <= SRL_CAM_THREADS, "staging: a thread per face");
static_assert(SRL_MAX_BODIES <= 32, "body masks are 32-bit words");

// what the kernel reads, by value
struct CamParams {
  srl_camera cam;
  const EnvHdr* hdr; const float* blob; const MeshHdr* mh; const float4* mp;
  const float* poses; const int32_t* mesh_ids; const int32_t* n_bodies; const int32_t* goal;   // the explicit scene, or all null
  int32_t BLOB, OFF_X, OFF_Q, OFF_MESH, n_mesh, max_bodies;
  float px, sx, sy;                // pixel size of the overhead map, the observable square
  int32_t tiles_x, tiles;          // tiles per image row, per image
  uint8_t* rgb; float* depth; int32_t* ids;
};

struct CamLds {
  float4 plane[SRL_CAM_CHUNK][SRL_MAX_TRIS];   // nw, dw
  float2 aux[SRL_CAM_CHUNK][SRL_MAX_TRIS];     // dw - dot(nw, eye), dot(nw, light)
  float4 sphere[SRL_MAX_BODIES];               // centre of mass (the body's position), widened radius squared
  float4 quat[SRL_MAX_BODIES];
  int2 faces[SRL_MAX_BODIES];                  // first plane in mp, count
  uint32_t votes[2][SRL_CAM_WAVES];            // [eye rays, shadow rays][wave]: bodies the wave asked for
};

// May the ray o + t d meet the sphere?  (false only when it certainly does not; a NaN anywhere says true)
__device__ __forceinline__ bool cam_may_meet(v3 o, v3 d, float4 sp) {
  const v3 m = V(sp.x, sp.y, sp.z) - o;
  const float b = dot(m, d), dd = dot(d, d), mm = dot(m, m);
  const float mmdd = mm * dd;
  return !(mmdd - b * b > sp.w * dd + 1e-5f * mmdd);
}

// bodies (bits) whose sphere some ray of the wave may meet; `on`: this lane has a ray
__device__ __forceinline__ uint32_t cam_votes(const CamLds& L, int nb, bool on, v3 o, v3 d) {
  uint32_t mask = 0u;
  for (int b = 0; b < nb; ++b)
    if (__any(on && cam_may_meet(o, d, L.sphere[b]))) mask |= 1u << b;
  return mask;
}

// Stage the up to SRL_CAM_CHUNK lowest bodies of `todo` (workgroup-uniform) into the chunk's slots: cb[s] = the body of slot s or
// -1; returns what is left of `todo`.  Ends with the barrier after which the slots may be read; the caller has made sure that
// nobody still reads the slots' previous contents.
__device__ __forceinline__ uint32_t cam_stage(const CamParams& C, CamLds& L, uint32_t todo, int (&cb)[SRL_CAM_CHUNK], int tid) {
  const v3 eye = V(C.cam.eye[0], C.cam.eye[1], C.cam.eye[2]), light = V(C.cam.light[0], C.cam.light[1], C.cam.light[2]);
#pragma unroll
  for (int s = 0; s < SRL_CAM_CHUNK; ++s) {
    cb[s] = -1;
    if (todo) {
      const int b = __ffs(todo) - 1;
      todo &= todo - 1u;
      cb[s] = b;
      const int2 fr = L.faces[b];
      if (tid < fr.y) {
        const float4 sp = L.sphere[b], qq = L.quat[b];
        q4 q; q.x = qq.x; q.y = qq.y; q.z = qq.z; q.w = qq.w;
        const m3 R = quat_to_mat(q);
        const float4 pl = C.mp[fr.x + tid];
        const v3 nw = mmul(R, V(pl.x, pl.y, pl.z));                  // (the first two lines of make_rplane, stage.h)
        const float dw = pl.w + dot(nw, V(sp.x, sp.y, sp.z));
        L.plane[s][tid] = make_float4(nw.x, nw.y, nw.z, dw);
        L.aux[s][tid] = make_float2(dw - dot(nw, eye), dot(nw, light));
      }
    }
  }
  __syncthreads();
  return todo;
}

// The clip of one ray against the faces of the body in slot s.  SHADOW: the ray from o along the light (the denominators are
// the staged ones); otherwise the ray from the eye along d (the numerators are).  Returns t_in < t_out and no parallel face
// outside; tin / tout / fin as the definition has them.
template <bool SHADOW>
__device__ __forceinline__ bool cam_clip(const CamLds& L, int s, int nt, v3 o, v3 d, float& tin, float& tout, int& fin) {
  tin = -INFINITY; tout = INFINITY; fin = 0;
  bool miss = false;
  for (int f = 0; f < nt; ++f) {
    const float4 pl = L.plane[s][f];
    const float2 ax = L.aux[s][f];
    const v3 nw = V(pl.x, pl.y, pl.z);
    const float den = SHADOW ? ax.y : dot(nw, d);
    const float num = SHADOW ? pl.w - dot(nw, o) : ax.x;
    const float t = num / den;
    if (den < 0.0f) { if (t > tin) { tin = t; fin = f; } }
    else if (den > 0.0f) tout = fminf(tout, t);
    else if (num < 0.0f) miss = true;
  }
  return !miss && tin < tout;
}

extern "C" __global__ void __launch_bounds__(SRL_CAM_THREADS) srl_k_camera(CamParams C) {
  __shared__ CamLds L;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int e = blockIdx.x / C.tiles, tile = blockIdx.x - e * C.tiles;
  const int ty = tile / C.tiles_x, tx = tile - ty * C.tiles_x;
  const int W = C.cam.width, H = C.cam.height;
  const int i = ty * SRL_CAM_TH + 2 * wave + (lane >> 5), j = tx * SRL_CAM_TW + (lane & 31);
  const bool on = i < H && j < W;
  const bool ext = C.poses != nullptr;
  int nb = ext ? C.n_bodies[e] : C.hdr[e].nb;
  nb = min(max(nb, 0), C.max_bodies);
  // ---- bodies (every slot the scene has, placed or not: the loads do not wait for the count; only slots below nb are used)
  if (tid < C.max_bodies) {
    float4 x, q; int m;
    if (ext) {
      const float* p = C.poses + ((size_t)e * SRL_MAX_BODIES + tid) * 7;
      x = make_float4(p[0], p[1], p[2], 0.0f); q = make_float4(p[3], p[4], p[5], p[6]);
      m = C.mesh_ids[(size_t)e * SRL_MAX_BODIES + tid];
    } else {
      const float* gb = C.blob + (size_t)e * C.BLOB;
      const float* xx = gb + C.OFF_X + 4 * tid; const float* qq = gb + C.OFF_Q + 4 * tid;
      x = make_float4(xx[0], xx[1], xx[2], 0.0f); q = make_float4(qq[0], qq[1], qq[2], qq[3]);
      m = ((const int*)gb)[C.OFF_MESH + tid];
    }
    m = min(max(m, 0), C.n_mesh - 1);
    const MeshHdr mh = C.mh[m];
    const float r = mh.radius * 1.05f + 1e-4f;
    x.w = r * r;
    L.sphere[tid] = x; L.quat[tid] = q; L.faces[tid] = make_int2(mh.to, min(mh.nt, SRL_MAX_TRIS));
  }
  // ---- the ray
  const v3 eye = V(C.cam.eye[0], C.cam.eye[1], C.cam.eye[2]), light = V(C.cam.light[0], C.cam.light[1], C.cam.light[2]);
  const float s = (float)(2 * j + 1) / (float)W - 1.0f, u = 1.0f - (float)(2 * i + 1) / (float)H;
  const v3 d = V((C.cam.fwd[0] + s * C.cam.right[0]) + u * C.cam.up[0], (C.cam.fwd[1] + s * C.cam.right[1]) + u * C.cam.up[1],
                 (C.cam.fwd[2] + s * C.cam.right[2]) + u * C.cam.up[2]);
  __syncthreads();
  const uint32_t mine = cam_votes(L, nb, on, eye, d);
  if (lane == 0) L.votes[0][wave] = mine;
  __syncthreads();
  uint32_t todo = 0u;
#pragma unroll
  for (int w = 0; w < SRL_CAM_WAVES; ++w) todo |= L.votes[0][w];
  // ---- nearest rock
  float best = INFINITY;
  int bid = -1;
  v3 nrm = V(0.0f, 0.0f, 1.0f);
  int cb[SRL_CAM_CHUNK];
#pragma unroll
  for (int k = 0; k < SRL_CAM_CHUNK; ++k) cb[k] = -1;
  bool first = true;
  while (todo) {
    if (!first) __syncthreads();                       // every wave is done with the chunk before
    first = false;
    todo = cam_stage(C, L, todo, cb, tid);
#pragma unroll
    for (int k = 0; k < SRL_CAM_CHUNK; ++k) {
      const int b = cb[k];
      if (b < 0 || !((mine >> b) & 1u)) continue;      // (wave-uniform)
      float tin, tout; int fin;
      const bool hit = cam_clip<false>(L, k, L.faces[b].y, eye, d, tin, tout, fin) && tin > 0.0f;
      if (hit && tin < best) {                         // (bodies come in slot order: a tie stays with the lower slot)
        best = tin; bid = b;
        const float4 pl = L.plane[k][fin];
        nrm = V(pl.x, pl.y, pl.z);
      }
    }
  }
  // ---- ground and sky
  const float tg = d.z < 0.0f ? -eye.z / d.z : INFINITY;
  int id = -2;
  float t = INFINITY;
  if (bid >= 0 && best < tg) { id = bid; t = best; }
  else if (d.z < 0.0f) { id = -1; t = tg; nrm = V(0.0f, 0.0f, 1.0f); }
  const v3 p = madd(eye, d, t);
  // ---- shadows
  float lit = 1.0f;
  if (C.cam.shadows) {
    const v3 o = madd(p, nrm, 1e-4f);
    bool open = on && id != -2;                        // this lane's shadow ray has met no rock yet
    const uint32_t smine = cam_votes(L, nb, open, o, light);
    if (lane == 0) L.votes[1][wave] = smine;
    __syncthreads();                                   // (also: every wave is done with the last chunk's sweeps)
    uint32_t stodo = 0u;
#pragma unroll
    for (int w = 0; w < SRL_CAM_WAVES; ++w) stodo |= L.votes[1][w];
    // the bodies still staged are swept where they lie
#pragma unroll
    for (int k = 0; k < SRL_CAM_CHUNK; ++k) {
      const int b = cb[k];
      if (b < 0) continue;
      stodo &= ~(1u << b);
      if (!((smine >> b) & 1u) || !__any(open)) continue;
      float tin, tout; int fin;
      if (open && cam_clip<true>(L, k, L.faces[b].y, o, light, tin, tout, fin) && tout > 0.0f) { open = false; lit = 0.0f; }
    }
    while (stodo) {
      __syncthreads();
      stodo = cam_stage(C, L, stodo, cb, tid);
#pragma unroll
      for (int k = 0; k < SRL_CAM_CHUNK; ++k) {
        const int b = cb[k];
        if (b < 0 || !((smine >> b) & 1u) || !__any(open)) continue;
        float tin, tout; int fin;
        if (open && cam_clip<true>(L, k, L.faces[b].y, o, light, tin, tout, fin) && tout > 0.0f) { open = false; lit = 0.0f; }
      }
    }
  }
  if (!on) return;
  // ---- shading and the stores
  const size_t pix = ((size_t)e * H + i) * W + j;
  if (C.depth) C.depth[pix] = t;
  if (C.ids) C.ids[pix] = id;
  if (C.rgb) {
    float r, g, b;
    if (id == -2) { r = C.cam.sky_rgb[0]; g = C.cam.sky_rgb[1]; b = C.cam.sky_rgb[2]; }
    else {
      if (id >= 0) { r = C.cam.rock_rgb[0]; g = C.cam.rock_rgb[1]; b = C.cam.rock_rgb[2]; }
      else {
        r = g = b = 0.8f;
        if (p.x >= 0.0f && p.x <= C.sx && p.y >= 0.0f && p.y <= C.sy) {
          r = 0.5f * r + 0.5f; g = 0.5f * g + 0.5f; b = 0.5f * b + 0.5f;
          const int32_t* gr = ext ? C.goal + 4 * (size_t)e : C.hdr[e].goal;
          const float gx0 = (float)gr[0] * C.px, gx1 = (float)(gr[0] + gr[2]) * C.px;
          const float gy0 = (float)gr[1] * C.px, gy1 = (float)(gr[1] + gr[3]) * C.px;
          if (p.x >= gx0 && p.x <= gx1 && p.y >= gy0 && p.y <= gy1) { r = 0.5f * r; g = 0.5f * g + 0.5f; b = 0.5f * b; }
        }
      }
      const float shade = C.cam.ambient + (C.cam.diffuse * fmaxf(0.0f, dot(nrm, light))) * lit;
      r = r * shade; g = g * shade; b = b * shade;
    }
    uint8_t* o = C.rgb + 3 * pix;
    o[0] = (uint8_t)view_byte((double)r); o[1] = (uint8_t)view_byte((double)g); o[2] = (uint8_t)view_byte((double)b);
  }
}
